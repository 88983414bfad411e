"""First-hit feature buffers (vr_render_features*, vanrijn_amd/csrc/vr_features.hip).

The reference is built from the oracle alone: the camera rays from orc_stream_base / orc_stream_draw /
orc_u64_to_standard and ray_for_pixel, their first hits from OracleScene.trace, the per-pixel sums
replayed by a sequential Python loop in sample order, and the albedo photons from the oracle's
Spectrum::intensity_at_wavelength of the traced material at the oracle's wavelength; the expected
albedo state is accumulate_photons_device of those photons (tests/test_gpu_display.py holds that
function to exact references).  Where the oracle has no counterpart (a pose, a lens) the rays and hits
come from camera_rays_device and query_closest, which their own tests pin.  Everything is compared bit
for bit; a NaN normal sum must be NaN in the same place.

Every case is at most 64x48 pixels and 3 samples per pixel.
"""
import numpy as np
import pytest
import torch

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE
from vanrijn_amd.render import (Film, PHOTON_DTYPE, Tile, accumulate_photons_device, camera_rays_device, query_closest,
                                render_features, render_features_device, resolve_state, tone_map_device)
from vanrijn_amd.scene import CameraLens, DeviceScene, Scene, look_at

from scene_edit_checks import edited_spec, rotation_about, transformed
from test_gpu_fullframe import nan_scene
from test_gpu_mesh_materials import _soup_scenes, _with_mesh

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F17
GUARD = 5           # records / state doubles past the tile's last pixel
GUARD_BYTE = 0xA5
GUARD_VALUE = -7.0


# ----------------------------------------------------------------------------------- the reference
def _stream_draws(oracle, tile, W, spp, seed, first_sample, draws):
    """Standard draws `draws` of every (sample, pixel) stream of the tile, [s][p][k], from the oracle."""
    L = oracle.lib()
    tw, n = tile.width(), tile.width() * tile.height()
    out = np.empty((spp, n, len(draws)))
    for s in range(spp):
        for p in range(n):
            row, col = tile.start_row + p // tw, tile.start_column + p % tw
            base = L.orc_stream_base(seed, row * W + col, first_sample + s)
            for k, draw in enumerate(draws):
                out[s, p, k] = L.orc_u64_to_standard(L.orc_stream_draw(base, draw))
    return out


def _oracle_hits(oracle, scene, tile, H, W, spp, seed, first_sample=0):
    """The first hits of the default camera's rays, [s][p], from the oracle alone: valid, distance, normal,
    object, primitive, material and the wavelength (draw 2)."""
    spec = scene.spec()
    tw, n = tile.width(), tile.width() * tile.height()
    u = _stream_draws(oracle, tile, W, spp, seed, first_sample, (0, 1, 2))
    o, d = np.empty((spp, n, 3)), np.empty((spp, n, 3))
    for s in range(spp):
        for p in range(n):
            row, col = tile.start_row + p // tw, tile.start_column + p % tw
            o[s, p], d[s, p] = oracle.ray_for_pixel(spec.camera_location, W, H, row, col, u[s, p, 0], u[s, p, 1])
    hits, _ = oracle.OracleScene(spec).trace(o.reshape(-1, 3), d.reshape(-1, 3))
    out = {"valid": np.array([h.valid for h in hits]), "distance": np.array([h.distance for h in hits]),
           "normal": np.array([list(h.normal) for h in hits]), "object": np.array([h.object for h in hits]),
           "primitive": np.array([h.primitive for h in hits]), "material": np.array([h.material for h in hits]),
           "wavelength": 380.0 + 360.0 * u[:, :, 2].reshape(-1)}
    return {k: v.reshape((spp, n) + v.shape[1:]) for k, v in out.items()}


def _material_of(spec, obj, primitive):
    o = spec.objects[obj]
    return o.primitives[primitive].material if o.kind == "primitives" else spec.meshes[o.mesh].material


def _staged_hits(oracle, ds, spec, tile, H, W, spp, seed, first_sample=0, lens=False):
    """The same arrays from the staged route of the scene's own camera (pose and lens included):
    camera_rays_device, then query_closest with records; the wavelength is the oracle's draw 2 (4 with a
    lens); the material follows from the object (meshes with one material only)."""
    n = tile.width() * tile.height()
    o = torch.zeros(spp * n * 3, dtype=torch.float64, device="cuda")
    d = torch.zeros(spp * n * 3, dtype=torch.float64, device="cuda")
    ids = torch.zeros(spp * n, dtype=torch.int64, device="cuda")
    camera_rays_device(ds, tile, H, W, spp, seed, first_sample, o.data_ptr(), d.data_ptr(), ids.data_ptr())
    torch.cuda.synchronize()
    hits, rec = query_closest(ds, o.cpu().numpy().reshape(-1, 3), d.cpu().numpy().reshape(-1, 3), records=True)
    u = _stream_draws(oracle, tile, W, spp, seed, first_sample, (4 if lens else 2,))
    out = {"valid": hits["valid"], "distance": hits["distance"], "normal": rec["normal"], "object": hits["object"],
           "primitive": hits["primitive"],
           "material": np.array([_material_of(spec, h["object"], h["primitive"]) if h["valid"] else -1 for h in hits]),
           "wavelength": 380.0 + 360.0 * u[:, :, 0].reshape(-1)}
    return {k: np.ascontiguousarray(v).reshape((spp, n) + v.shape[1:]) for k, v in out.items()}


def _replay(h, records=None):
    """The per-pixel records of the hits h ([s][p] arrays), folded one sample at a time in sample order by a
    sequential loop of Python floats (IEEE binary64 additions); `records`: continue these."""
    spp, n = h["valid"].shape
    rec = np.zeros(n, dtype=PIXEL_FEATURES_DTYPE) if records is None else records.reshape(-1).copy()
    if records is None:
        rec["object"], rec["primitive"] = -1, -1
    for p in range(n):
        nx, ny, nz = (float(v) for v in rec["normal_sum"][p])
        dsum, dmin, count = float(rec["distance_sum"][p]), float(rec["distance_min"][p]), int(rec["hits"][p])
        obj, prim = int(rec["object"][p]), int(rec["primitive"][p])
        for s in range(spp):
            if not h["valid"][s, p]:
                continue
            dist = float(h["distance"][s, p])
            if count == 0 or dist < dmin:
                dmin, obj, prim = dist, int(h["object"][s, p]), int(h["primitive"][s, p])
            count += 1
            nx = nx + float(h["normal"][s, p, 0])
            ny = ny + float(h["normal"][s, p, 1])
            nz = nz + float(h["normal"][s, p, 2])
            dsum = dsum + dist
        rec[p] = ((nx, ny, nz), dsum, dmin, count, int(rec["samples"][p]) + spp, obj, 0, prim)
    return rec


def _photons(oracle, spec, h):
    """One photon per sample, [s][p]: {0, 0} for a miss, else {wavelength, the oracle's
    Spectrum::intensity_at_wavelength of the traced material's colour}, 1.0 for a dielectric."""
    spp, n = h["valid"].shape
    ph = np.zeros((spp, n), dtype=PHOTON_DTYPE)
    for s in range(spp):
        for p in range(n):
            if not h["valid"][s, p]:
                continue
            m = spec.materials[int(h["material"][s, p])]
            wl = float(h["wavelength"][s, p])
            a = 1.0 if m.kind == N.MATERIAL_DIELECTRIC else oracle.spectrum_intensity(
                m.colour.shortest_wavelength, m.colour.longest_wavelength, m.colour.samples, wl)
            ph[s, p] = (wl, a)
    return ph


def _state_of(photons, state=None):
    """accumulate_photons_device of [s][p] photons (continuing `state`): the expected albedo state."""
    spp, n = photons.shape
    st = torch.zeros(8 * n, dtype=torch.float64, device="cuda") if state is None else torch.from_numpy(state.copy()).cuda()
    ph = torch.from_numpy(np.ascontiguousarray(photons).view(np.float64).reshape(-1).copy()).cuda()
    accumulate_photons_device(st.data_ptr(), ph.data_ptr(), n, spp, accumulate=state is not None)
    torch.cuda.synchronize()
    return st.cpu().numpy()


# --------------------------------------------------------------------------- the pass under test
class Buffers:
    """Device outputs of one tile with GUARD records / doubles after them, filled with guard values."""

    def __init__(self, npix, features=True, albedo=True):
        self.npix = npix
        self.f = torch.full(((npix + GUARD) * 64,), GUARD_BYTE, dtype=torch.uint8, device="cuda") if features else None
        self.a = torch.full((8 * npix + GUARD,), GUARD_VALUE, dtype=torch.float64, device="cuda") if albedo else None
        torch.cuda.synchronize()

    def records(self):
        raw = self.f.cpu().numpy()
        assert (raw[self.npix * 64:] == GUARD_BYTE).all(), "records past the tile were written"
        return raw[:self.npix * 64].view(PIXEL_FEATURES_DTYPE)

    def state(self):
        raw = self.a.cpu().numpy()
        assert (raw[8 * self.npix:] == GUARD_VALUE).all(), "state past the tile was written"
        return raw[:8 * self.npix]


def _run(ds, tile, H, W, spp, seed=SEED, first=0, bufs=None, accumulate=False, features=True, albedo=True, stream=None):
    """vr_render_features_device into guarded torch buffers -> (records or None, state or None, buffers)."""
    b = bufs or Buffers(tile.width() * tile.height(), features, albedo)
    render_features_device(ds, tile, H, W, spp, seed, first, b.f.data_ptr() if b.f is not None else None,
                           b.a.data_ptr() if b.a is not None else None,
                           stream_ptr=stream.cuda_stream if stream is not None else None, accumulate=accumulate)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return (b.records() if b.f is not None else None), (b.state() if b.a is not None else None), b


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_records(got, want, nan_normals=False, fields=PIXEL_FEATURES_DTYPE.names):
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.shape == want.shape
    for f in fields:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if f == "normal_sum" and nan_normals:  # NaN where the reference has NaN, the same bits elsewhere
            gn, wn = np.isnan(g), np.isnan(w)
            assert np.array_equal(gn, wn), f
            assert np.array_equal(_bits(g)[~wn], _bits(w)[~wn]), f
        else:
            assert g.tobytes() == w.tobytes(), (f, int((g != w).sum()))


def _assert_state(got, want):
    assert np.array_equal(_bits(got), _bits(want)), int((_bits(got) != _bits(want)).sum())


def _window(records, state, full: Tile, tile: Tile):
    """The part of a full tile's records and state that covers `tile`."""
    r0, r1 = tile.start_row - full.start_row, tile.end_row - full.start_row
    c0, c1 = tile.start_column - full.start_column, tile.end_column - full.start_column
    rec = records.reshape(full.height(), full.width())[r0:r1, c0:c1].reshape(-1)
    halves = state.reshape(2, full.height(), full.width(), 4)[:, r0:r1, c0:c1]
    return rec, np.ascontiguousarray(halves).reshape(-1)


# ------------------------------------------------------------------------------------ the cases
class Case:
    """A scene, a tile, the oracle's first hits and the expected records and state, computed once."""

    def __init__(self, oracle, scene, tile, H, W, spp, first=0):
        self.scene, self.tile, self.H, self.W, self.spp, self.first = scene, tile, H, W, spp, first
        self.ds = scene.device_scene(0)
        self.hits = _oracle_hits(oracle, scene, tile, H, W, spp, SEED, first)
        self.records = _replay(self.hits)
        self.photons = _photons(oracle, scene.spec(), self.hits)
        self.state = _state_of(self.photons)
        for a in (self.records, self.photons, self.state, *self.hits.values()):
            a.setflags(write=False)

    def stats(self):
        r, v = self.records, self.hits["valid"]
        first_hit = np.argmax(v, axis=0)  # the first sample that hit, per pixel
        first_d = np.take_along_axis(self.hits["distance"], first_hit[None], 0)[0]
        mesh = {i for i, o in enumerate(self.scene.spec().objects) if o.kind == "bvh"}
        return {"hit": int(v.sum()), "miss": int((v == 0).sum()),
                "partial": int(((r["hits"] > 0) & (r["hits"] < r["samples"])).sum()),
                "objects": sorted(set(r["object"].tolist())),
                "mesh_pixels": int(np.isin(r["object"], list(mesh)).sum()),
                "later_nearest": int(((r["hits"] > 1) & (r["distance_min"] < first_d)).sum())}

    def check(self, nan_normals=False):
        rec, st, _ = _run(self.ds, self.tile, self.H, self.W, self.spp, first=self.first)
        _assert_records(rec, self.records, nan_normals)
        _assert_state(st, self.state)
        return rec, st


FULL = Tile(0, 64, 0, 48)


@pytest.fixture(scope="module")
def main_case(oracle):
    c = Case(oracle, scenes.main_scene(), FULL, 48, 64, 2)
    s = c.stats()
    # (the oracle's counts on the CPU: 3430 hit and 2714 missed samples, 8 pixels hit by one of their two
    # samples, objects -1, 0 and 1, the mesh nearest in 462 pixels, the second sample nearer in 865)
    assert s["hit"] > 3000 and s["miss"] > 2000 and s["partial"] >= 5, s
    assert len(s["objects"]) >= 3 and s["mesh_pixels"] > 400 and s["later_nearest"] >= 500, s
    return c


@pytest.fixture(scope="module")
def materials_case(oracle):
    c = Case(oracle, scenes.materials_scene(), Tile(0, 48, 0, 32), 32, 48, 2)
    s = c.stats()
    # (the oracle's counts: 1712 hit, 1360 missed, 12 partly covered pixels, the second sample nearer in 425)
    assert s["hit"] > 1500 and s["miss"] > 1000 and s["partial"] >= 5 and s["later_nearest"] >= 300, s
    assert len(s["objects"]) >= 3 and s["mesh_pixels"] > 150, s
    return c


@pytest.fixture(scope="module")
def full_result(main_case):
    """The full tile's result of the pass itself (held to the oracle by test_main_scene)."""
    rec, st, _ = _run(main_case.ds, FULL, 48, 64, 2)
    rec.setflags(write=False)
    st.setflags(write=False)
    return rec, st


def test_main_scene(main_case):
    rec, _ = main_case.check()
    # the primitive list (plane and spheres) and the mesh are both under pixels; with the materials scene's
    # and the NaN scene's objects the three oracle cases see more than three distinct (scene, object) pairs
    assert set(rec["object"].tolist()) >= {-1, 0, 1}
    assert (rec["samples"] == 2).all() and (rec["reserved"] == 0).all()
    miss = rec["hits"] == 0
    assert miss.sum() > 400 and (rec["primitive"][miss] == -1).all() and not rec["distance_min"][miss].any()


def test_every_material_kind(materials_case):
    c = materials_case
    spec = c.scene.spec()
    kinds = np.array([m.kind for m in spec.materials])
    hit = c.hits["valid"] == 1
    seen = set(kinds[c.hits["material"][hit]].tolist())
    assert seen == {N.MATERIAL_LAMBERTIAN, N.MATERIAL_REFLECTIVE, N.MATERIAL_PHONG, N.MATERIAL_DIELECTRIC}
    glass = hit & (kinds[np.where(hit, c.hits["material"], 0)] == N.MATERIAL_DIELECTRIC)
    assert glass.sum() > 20 and (c.photons["intensity"][glass] == 1.0).all()
    other = hit & ~glass
    assert (c.photons["intensity"][other] != 1.0).all()
    rec, _ = c.check()
    assert len(set(rec["object"].tolist()) - {-1}) == 2 and len(set(rec["primitive"][rec["object"] == 0].tolist())) == 4


def test_nan_normals_reach_the_sums(oracle, tmp_path):
    """test_gpu_fullframe.py's objects seen from behind the normal-less wall's edge: the wall (zero normals,
    mesh.rs:37) covers part of the view, and every hit on it has a NaN normal."""
    base = nan_scene(tmp_path)
    c = Case(oracle, Scene((16.5, 1.0, -9.0), base.objects), Tile(0, 32, 0, 24), 24, 32, 2)
    nan = np.isnan(c.records["normal_sum"]).any(axis=1)
    finite = (c.records["hits"] > 0) & ~nan
    assert nan.sum() > 200 and finite.sum() > 200 and (c.records["hits"] == 0).sum() > 200
    assert set(c.records["object"][nan].tolist()) == {2}  # the wall
    rec, st = c.check(nan_normals=True)
    assert np.isfinite(rec["distance_sum"]).all() and np.isfinite(st).all()


# ------------------------------------------------------------------ pose, lens, per-triangle materials
def _posed(ds_scene, lens):
    ds = DeviceScene(ds_scene.spec(), 0)
    ds.set_camera_pose(look_at((-7.0, 0.0, -4.0), (-3.5, 0.0, 1.0), film_distance=1.3))
    if lens:
        ds.set_camera_lens(CameraLens(0.15, 6.0))
    return ds


@pytest.mark.parametrize("lens", [False, True], ids=["pose", "pose_and_lens"])
def test_pose_and_lens(oracle, lens):
    scene = scenes.materials_scene()
    ds = _posed(scene, lens)
    tile, H, W, spp = Tile(3, 43, 2, 30), 32, 48, 2
    h = _staged_hits(oracle, ds, scene.spec(), tile, H, W, spp, SEED, lens=lens)
    assert h["valid"].sum() > 1200 and (h["valid"] == 0).sum() > 500
    want = _replay(h)
    assert len(set(want["object"].tolist())) == 3
    rec, st, _ = _run(ds, tile, H, W, spp)
    _assert_records(rec, want)
    _assert_state(st, _state_of(_photons(oracle, scene.spec(), h)))
    # the default camera's result is another one
    other, _, _ = _run(scene.device_scene(0), tile, H, W, spp)
    assert other.tobytes() != rec.tobytes()


def test_per_triangle_materials(oracle):
    """One mesh with four materials: geometry and albedo against the oracle's run of the split scene (four
    meshes, a scene it can express); object and primitive against the staged route on the merged scene."""
    merged, split, ids = _soup_scenes(260, 21)
    tile, H, W, spp = Tile(0, 32, 0, 32), 32, 32, 2
    h = _oracle_hits(oracle, split, tile, H, W, spp, SEED)
    on_mesh = (h["valid"] == 1) & (h["object"] >= 1)
    assert on_mesh.sum() > 120 and len(set(h["material"][on_mesh].tolist())) == 4
    ds = DeviceScene(merged.spec(), 0)
    rec, st, _ = _run(ds, tile, H, W, spp)
    _assert_records(rec, _replay(h), fields=("normal_sum", "distance_sum", "distance_min", "hits", "samples", "reserved"))
    assert [m.kind for m in merged.spec().materials] == [m.kind for m in split.spec().materials]
    _assert_state(st, _state_of(_photons(oracle, split.spec(), h)))
    staged = _staged_hits(oracle, ds, merged.spec(), tile, H, W, spp, SEED)
    _assert_records(rec, _replay(staged))


# -------------------------------------------------------------------------------------- edge shapes
@pytest.mark.parametrize("tile", [Tile(5, 37, 3, 30), Tile(41, 42, 17, 18), Tile(26, 27, 0, 48), Tile(0, 64, 31, 32)],
                         ids=["odd_offsets", "one_pixel", "one_column", "one_row"])
def test_edge_shapes_equal_the_window_of_the_full_tile(main_case, full_result, tile):
    rec, st, _ = _run(main_case.ds, tile, 48, 64, 2)
    want_rec, want_st = _window(*full_result, FULL, tile)
    _assert_records(rec, want_rec)
    _assert_state(st, want_st)


# ---------------------------------------------------------------------------- tiling and continuation
def test_two_half_tiles_equal_the_full_tile(main_case, full_result):
    for a, b in ((Tile(0, 29, 0, 48), Tile(29, 64, 0, 48)), (Tile(0, 64, 0, 21), Tile(0, 64, 21, 48))):
        for t in (a, b):
            rec, st, _ = _run(main_case.ds, t, 48, 64, 2)
            want_rec, want_st = _window(*full_result, FULL, t)
            _assert_records(rec, want_rec)
            _assert_state(st, want_st)


def test_continuation_equals_one_call(oracle, main_case):
    """spp 2, then first_sample 2 @1 with accumulate, equals spp 3: both arrays, and the oracle's replay."""
    ds, tile, H, W = main_case.ds, Tile(8, 56, 6, 42), 48, 64
    rec3, st3, _ = _run(ds, tile, H, W, 3)
    _, _, b = _run(ds, tile, H, W, 2)
    rec, st, _ = _run(ds, tile, H, W, 1, first=2, bufs=b, accumulate=True)
    _assert_records(rec, rec3)
    _assert_state(st, st3)
    assert (rec["samples"] == 3).all() and (st[:4 * b.npix].reshape(-1, 4)[:, 3] == 3.0).all()
    # sample 2 alone changed the nearest sample somewhere: the continuation carries the nearest sample
    first2, _ = _window(*(_run(ds, FULL, H, W, 2)[:2]), FULL, tile)
    assert ((rec["hits"] > first2["hits"]) & (rec["distance_min"] < first2["distance_min"]) & (first2["hits"] > 0)).sum() > 20
    # and the three samples against the oracle
    h = _oracle_hits(oracle, main_case.scene, tile, H, W, 3, SEED)
    _assert_records(rec3, _replay(h))
    _assert_state(st3, _state_of(_photons(oracle, main_case.scene.spec(), h)))


def test_first_sample_well_above_zero(oracle):
    c = Case(oracle, scenes.main_scene(), Tile(16, 48, 12, 40), 48, 64, 1, first=4_000_000_123)
    assert c.hits["valid"].sum() > 300 and (c.hits["valid"] == 0).sum() > 50
    c.check()


# --------------------------------------------------------------------------------------------- forms
def test_host_form_equals_the_device_form(main_case):
    ds, tile, H, W = main_case.ds, Tile(5, 37, 3, 30), 48, 64
    rec, st, _ = _run(ds, tile, H, W, 2)
    fb = render_features(ds, tile, H, W, 2, SEED)
    assert fb.records.shape == (27, 32)
    _assert_records(fb.records, rec)
    _assert_state(fb.albedo_state, st)
    only = render_features(ds, tile, H, W, 2, SEED, albedo=False)
    assert only.albedo_state is None
    _assert_records(only.records, rec)
    # continuing host buffers: the records and the Kahan state are uploaded first
    rec3, st3, _ = _run(ds, tile, H, W, 3)
    more = render_features(ds, tile, H, W, 1, SEED, first_sample=2, accumulate=fb)
    assert more is fb
    _assert_records(fb.records, rec3)
    _assert_state(fb.albedo_state, st3)
    assert np.array_equal(fb.alpha() > 0, rec3.reshape(27, 32)["hits"] > 0)


def test_a_torch_stream_and_single_outputs(main_case, full_result):
    ds, H, W = main_case.ds, 48, 64
    rec, st, _ = _run(ds, FULL, H, W, 2, stream=torch.cuda.Stream())
    _assert_records(rec, full_result[0])
    _assert_state(st, full_result[1])
    rec, st, _ = _run(ds, FULL, H, W, 2, albedo=False)
    assert st is None
    _assert_records(rec, full_result[0])
    rec, st, _ = _run(ds, FULL, H, W, 2, features=False)
    assert rec is None
    _assert_state(st, full_result[1])


def test_wide_offset_scene(main_case, full_result):
    """The 64-bit-offset form of a scene (VR_SCENE_WIDE_OFFSETS), as vr_query_closest_device supports it."""
    rec, st, _ = _run(main_case.scene.device_scene(0, wide_offsets=True), FULL, 48, 64, 2)
    _assert_records(rec, full_result[0])
    _assert_state(st, full_result[1])


def test_debug_hooks_are_ignored(main_case, full_result):
    ds = DeviceScene(main_case.scene.spec(), 0)
    ds.set_fault_object(1)
    ds.set_launch_flags(no_cull=True, no_dist_cull=True)
    rec, st, _ = _run(ds, FULL, 48, 64, 2)
    _assert_records(rec, full_result[0])
    _assert_state(st, full_result[1])


# --------------------------------------------------------------------------------------- scene edits
def test_after_transform_mesh_and_set_mesh_materials():
    merged, _, ids = _soup_scenes(260, 21)
    spec = merged.spec()
    tile, H, W, spp = Tile(0, 32, 0, 32), 32, 32, 2
    plain = _with_mesh(spec, spec.meshes[0].material)  # the same mesh with its single material
    ds = DeviceScene(plain, 0)
    before, before_st, _ = _run(ds, tile, H, W, spp)
    # 1. per-triangle materials set on the live scene == a scene created with them
    ds.set_mesh_materials(0, spec.meshes[0].triangle_materials)
    rec, st, _ = _run(ds, tile, H, W, spp)
    fresh_rec, fresh_st, _ = _run(DeviceScene(spec, 0), tile, H, W, spp)
    _assert_records(rec, fresh_rec)
    _assert_state(st, fresh_st)
    _assert_records(rec, before)  # the geometry did not move
    assert st.tobytes() != before_st.tobytes()
    # 2. the mesh moved on the live scene == a scene created from the moved arrays.  `primitive` is the
    # creation-time leaf position (include/vanrijn_amd.h vr_scene_transform_mesh): compared as the input
    # triangle that leaf_order maps it to
    m = rotation_about(0.7, (0.0, 0.0, 0.0), (0.1, 0.2, 0.0))
    ds.transform_mesh(0, m)
    v, n = transformed(m, spec.meshes[0].vertices, spec.meshes[0].normals)
    moved = edited_spec(spec, meshes={0: (v, n)})
    moved.meshes[0].triangle_materials = spec.meshes[0].triangle_materials  # (the assignment survives the transform)
    fresh = DeviceScene(moved, 0)
    rec, st, _ = _run(ds, tile, H, W, spp)
    fresh_rec, fresh_st, _ = _run(fresh, tile, H, W, spp)
    others = tuple(f for f in PIXEL_FEATURES_DTYPE.names if f != "primitive")
    _assert_records(rec, fresh_rec, fields=others)
    _assert_state(st, fresh_st)
    on_mesh = rec["object"] == 1
    assert on_mesh.sum() > 100 and rec["distance_sum"].tobytes() != before["distance_sum"].tobytes()
    assert np.array_equal(ds.leaf_order(0)[rec["primitive"][on_mesh]], fresh.leaf_order(0)[fresh_rec["primitive"][on_mesh]])
    assert np.array_equal(rec["primitive"][~on_mesh], fresh_rec["primitive"][~on_mesh])


# --------------------------------------------------------------------------------------- composition
def test_albedo_state_feeds_the_display_path(main_case):
    ds, tile, H, W, spp = main_case.ds, Tile(8, 56, 6, 42), 48, 64, 2
    _, st, b = _run(ds, tile, H, W, spp)
    n = b.npix
    rgb = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
    tone_map_device(b.a.data_ptr(), n, rgb.data_ptr())
    torch.cuda.synchronize()
    colour = resolve_state(st)
    host = np.zeros(3 * n, dtype=np.uint8)
    N.check(N.lib().vr_tone_map(colour.ctypes.data, n, host.ctypes.data, 0))
    assert np.array_equal(rgb.cpu().numpy(), host) and len(np.unique(host)) > 20
    # Film.merge_state takes it as a tile's records
    with Film(W, H) as film:
        assert film.merge_state(tile, b.a.data_ptr()) == 0
        buf, seen = film.read()
    assert seen == 1
    inside = np.zeros((H, W), dtype=bool)
    inside[tile.start_row:tile.end_row, tile.start_column:tile.end_column] = True
    assert (buf.weight_buffer[inside] == float(spp)).all() and not buf.weight_buffer[~inside].any()
    # merge_tile into an empty film: (0 * 0 + c * w) * (1 / w), three roundings of at most 2^-53 each
    got = buf.colour_buffer[tile.start_row:tile.end_row, tile.start_column:tile.end_column].reshape(-1, 3)
    assert np.allclose(got, colour, rtol=4 * 2.0 ** -53, atol=0.0) and colour.max() > 0.1
