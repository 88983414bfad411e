"""The camera pose (VR_HAS_CAMERA_POSE) on the device: the render kernel's camera step (the POSED
instantiations of vanrijn_amd/csrc/vr_render_kernel.h), camera_rays_kernel and the block cull under a pose.

The chain of evidence:
  1. the default pose set explicitly changes no bit, and is the oracle's ImageSampler;
  2. camera_rays_device equals vr_camera_ray -- the rule on the host, pinned to its restatement in
     tests/test_camera_pose_host.py -- with the jitter rebuilt from the oracle's own stream functions;
  3. with those rays the pinned integrator (vr_integrate_rays_device, tests/test_gpu_integrate.py) gives the
     posed megakernel's records bit for bit, and accumulated they give its state: the kernel traces the
     rule's rays and nothing else;
  4. the first hits are the oracle's trace of the same rays;
  5. the block cull changes no bit under any pose, and does cull;
  6. the film and the other scene edits see the pose.
"""
import numpy as np
import pytest
import torch

from camera_pose_checks import mirrored, pose_bits, poses, rule_ray
from scene_edit_checks import edited_spec, rotation_about, transformed
from test_gpu_scene_edit import CENTRE, _main_like
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import (PATH_INFO_DTYPE, PHOTON_DTYPE, AccumulationBuffer, Film, Tile, accumulate_photons_device,
                                camera_rays_device, integrate_rays_device, render_samples, render_tile,
                                render_tile_device, stream_check_error)
from vanrijn_amd.scene import (CameraPose, ColourRgbF, DeviceScene, DirectionalLight, MaterialSpec, NamedColour, Spectrum,
                               WhittedIntegrator, look_at)

pytestmark = pytest.mark.gpu

SPP, SEED = 2, 0x5EED0001
# both film-aspect branches, tiles that cut 8x8 blocks
FRAMES = {"wide": (40, 24, Tile(3, 37, 2, 21)), "tall": (24, 40, Tile(2, 21, 3, 37))}
POSES = poses()


@pytest.fixture(scope="module")
def mesh():
    return scenes.displaced_mesh(16, scenes._BUNNY_BUMPS, noise_seed=0xB0BB1E, noise_count=48, noise_amp=0.04,
                                 scale=(1.25, 1.05, 1.15), centre=CENTRE)


@pytest.fixture(scope="module")
def main_spec(mesh):
    return _main_like(*mesh).spec()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _staging_order(rec):
    """[tile_h][tile_w][spp] records -> [s][p] order, flat."""
    spp = rec.shape[2]
    return np.ascontiguousarray(rec.reshape(-1, spp).T).reshape(-1)


def _jitter(oracle, W, row, col, sample, seed=SEED):
    L = oracle.lib()
    base = L.orc_stream_base(seed, row * W + col, sample)
    return L.orc_u64_to_standard(L.orc_stream_draw(base, 0)), L.orc_u64_to_standard(L.orc_stream_draw(base, 1))


def _host_rays(oracle, pose, W, H, tile, spp, first_sample=0):
    """vr_camera_ray for every (sample, pixel) of the tile in [s][p] order, with the oracle's jitter."""
    tw, n = tile.width(), tile.width() * tile.height()
    o, d, ids = np.empty((spp, n, 3)), np.empty((spp, n, 3)), np.empty((spp, n), dtype=np.uint64)
    for s in range(spp):
        for p in range(n):
            row, col = tile.start_row + p // tw, tile.start_column + p % tw
            ux, uy = _jitter(oracle, W, row, col, first_sample + s)
            o[s, p], d[s, p] = pose.ray(W, H, row, col, ux, uy)
            ids[s, p] = ((row * W + col) << 32) + first_sample + s
    return o.reshape(-1, 3), d.reshape(-1, 3), ids.reshape(-1)


def _device_rays(ds, W, H, tile, spp, first_sample=0):
    n = tile.width() * tile.height() * spp
    o = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
    d = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
    ids = torch.zeros(n, dtype=torch.int64, device="cuda")
    camera_rays_device(ds, tile, H, W, spp, SEED, first_sample, o.data_ptr(), d.data_ptr(), ids.data_ptr())
    torch.cuda.synchronize()
    return o, d, ids


def _state(ds, W, H, tile, spp=SPP, seed=SEED, **kw):
    st = torch.zeros(tile.width() * tile.height() * 8, dtype=torch.float64, device="cuda")
    stats = render_tile_device(ds, tile, H, W, spp, seed, 0, st.data_ptr(), timed=True, **kw)
    torch.cuda.synchronize()
    return st.cpu().numpy(), stats


def _posed(spec, pose):
    ds = DeviceScene(spec, 0)
    ds.set_camera_pose(pose)
    return ds


# ------------------------------------------------------------------ 1. the default pose
@pytest.mark.parametrize("frame", list(FRAMES))
def test_default_pose_set_explicitly_changes_nothing(frame, main_spec, oracle):
    W, H, tile = FRAMES[frame]
    plain, explicit = DeviceScene(main_spec, 0), DeviceScene(main_spec, 0)
    explicit.set_camera_pose(CameraPose(location=main_spec.camera_location))
    assert pose_bits(explicit.camera_pose()) == pose_bits(plain.camera_pose())
    a, b = render_samples(plain, tile, H, W, 4, SEED), render_samples(explicit, tile, H, W, 4, SEED)
    assert a.tobytes() == b.tobytes()
    (sa, va), (sb, vb) = _state(plain, W, H, tile), _state(explicit, W, H, tile)
    assert sa.tobytes() == sb.tobytes() and va["variant"] == vb["variant"]
    for x, y in zip(_device_rays(plain, W, H, tile, SPP), _device_rays(explicit, W, H, tile, SPP)):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    # ... and is the oracle's camera, as test_edited_scene_tile_against_the_oracle checks an edited scene
    ref = oracle.OracleScene(main_spec).render_samples(tile, H, W, 4, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert np.array_equal(b["flags"], ref["flags"])
    assert np.array_equal(b["bounces"], ref["bounces"])
    assert np.array_equal(b["wavelength"], ref["wavelength"])
    nz = ref["intensity"] != 0
    assert (np.abs(b["intensity"] - ref["intensity"])[nz] / np.abs(ref["intensity"])[nz] < 1e-12).all()
    assert np.array_equal(b["intensity"] == 0, ref["intensity"] == 0)
    assert (ref["flags"] & 1).sum() > 100


# ------------------------------------------------------------------ 2. camera_rays_device against the rule
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", list(POSES))
def test_camera_rays_device_equals_the_rule(name, frame, main_spec, oracle):
    W, H, tile = FRAMES[frame]
    pose = POSES[name]
    ds = _posed(main_spec, pose)
    for first in (0, 5):
        o, d, ids = _device_rays(ds, W, H, tile, SPP, first)
        ho, hd, hids = _host_rays(oracle, pose, W, H, tile, SPP, first)
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(ho.reshape(-1)))
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(hd.reshape(-1)))
        assert np.array_equal(ids.cpu().numpy().view(np.uint64), hids)
    # one pixel against the restated rule itself (tests/test_camera_pose_host.py pins every pixel on the host)
    row, col = tile.start_row, tile.start_column
    ux, uy = _jitter(oracle, W, row, col, 5)
    assert rule_ray(oracle, pose, W, H, row, col, ux, uy)[1].tobytes() == hd[0].tobytes()


# ------------------------------------------------------------------ 3 + 4. the megakernel, the integrator, the oracle
def _check_megakernel(ds, pose, W, H, tile, oracle=None, orc_scene=None):
    """The posed render's records and state against the staged pipeline over camera_rays_device's rays."""
    npix = tile.width() * tile.height()
    n = npix * SPP
    o, d, ids = _device_rays(ds, W, H, tile, SPP)
    ph = torch.full((n, 2), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    staged = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    integrate_rays_device(ds, n, o.data_ptr(), d.data_ptr(), ph.data_ptr(), SEED, stream_ids_ptr=ids.data_ptr(),
                          info_ptr=info.data_ptr(), first_draw=2)
    accumulate_photons_device(staged.data_ptr(), ph.data_ptr(), npix, SPP)
    torch.cuda.synchronize()
    stream_check_error(ds)
    photons = ph.cpu().numpy().reshape(-1).view(PHOTON_DTYPE)
    paths = info.cpu().numpy().reshape(-1).view(PATH_INFO_DTYPE)
    rec = _staging_order(render_samples(ds, tile, H, W, SPP, SEED))
    assert np.array_equal(_bits(photons["wavelength"]), _bits(rec["wavelength"]))
    assert np.array_equal(_bits(photons["intensity"]), _bits(rec["intensity"]))
    assert np.array_equal(paths["bounces"], rec["bounces"]) and np.array_equal(paths["flags"], rec["flags"])
    state, stats = _state(ds, W, H, tile)
    assert np.array_equal(_bits(state), _bits(staged.cpu().numpy()))
    hit = (rec["flags"] & 1) != 0
    assert 0 < hit.sum() < n  # hits and misses in frame
    if orc_scene is not None:  # 4. first hits: the oracle's trace of the rule's rays
        ho, hd, _ = _host_rays(oracle, pose, W, H, tile, SPP)
        hits, _ = orc_scene.trace(ho, hd)
        assert np.array_equal(np.array([h.valid != 0 for h in hits]), hit)
    return rec, stats


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", list(POSES))
def test_megakernel_equals_the_pinned_integrator(name, frame, main_spec, oracle):
    W, H, tile = FRAMES[frame]
    pose = POSES[name]
    ds = _posed(main_spec, pose)
    rec, _ = _check_megakernel(ds, pose, W, H, tile, oracle, oracle.OracleScene(main_spec))
    default = _staging_order(render_samples(DeviceScene(main_spec, 0), tile, H, W, SPP, SEED))
    assert rec.tobytes() != default.tobytes()


def test_megakernel_on_the_reflective_scene(mesh, oracle):
    """The bench scene: reflective paths and the cooperative tail's instantiation."""
    spec = scenes.bench_scene(mesh).spec()
    W, H, tile = FRAMES["tall"]
    pose = POSES["look_at"]
    ds = _posed(spec, pose)
    rec, stats = _check_megakernel(ds, pose, W, H, tile, oracle, oracle.OracleScene(spec))
    assert stats["variant"] & N.VARIANT_COOP
    assert rec["bounces"].max() >= 2


def test_megakernel_on_a_whitted_scene(mesh, oracle):
    spec = scenes.whitted_scene(mesh).spec()
    W, H, tile = FRAMES["tall"]
    pose = POSES["mirrored"]
    _check_megakernel(_posed(spec, pose), pose, W, H, tile, oracle, oracle.OracleScene(spec))


# ------------------------------------------------------------------ 5. the block cull
def _cull_pair(ds, W, H, tile):
    """States and counters with the cull off and on, after other photons went through the call contexts'
    staging buffers (tests/test_gpu_cull.py: a sample the render skips but the reduce reads would show)."""
    npix = tile.width() * tile.height()

    def run(cull):
        junk = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        for k in range(2):
            render_tile_device(ds, tile, H, W, 4, 0x1234 + k, 0, junk.data_ptr(), cull=False)
        st = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        render_tile_device(ds, tile, H, W, 3, 0x77, 0, st.data_ptr(), cull=cull)
        c = render_tile_device(ds, tile, H, W, 2, 0x77, 3, st.data_ptr(), accumulate=True, counters=True, cull=cull)
        torch.cuda.synchronize()
        return st.cpu(), c

    return run(False), run(True)


def test_the_poses_meet_the_cull_cases(main_spec, oracle):
    """On the CPU: "up" puts the mesh's root box partly behind the camera, which is outside the box's bounding
    sphere (the cull's fallback); "mirrored" has the plane's horizon in frame -- plane hits below it, misses
    above -- and every pose has hits and misses in frame."""
    ds = DeviceScene(main_spec, 0)
    box = ds.bvh_roots()[0]["root_box"]
    up = POSES["up"]
    corners = np.array([[box[i], box[2 + j], box[4 + k]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    pz = (corners - np.array(up.location)) @ np.array(up.forward)
    assert pz.min() < -0.1 and pz.max() > 1.0
    centre, radius = corners.mean(axis=0), 0.5 * np.linalg.norm(corners.max(axis=0) - corners.min(axis=0))
    assert np.linalg.norm(centre - np.array(up.location)) > radius * 1.01
    orc = oracle.OracleScene(main_spec)
    for name, pose in POSES.items():
        for W, H, _ in FRAMES.values():
            rays = [pose.ray(W, H, r, c, 0.5, 0.5) for r in range(H) for c in range(W)]
            hits, _ = orc.trace(np.array([o for o, _ in rays]), np.array([d for _, d in rays]))
            valid = np.array([h.valid != 0 for h in hits])
            assert 10 < valid.sum() < W * H - 10, (name, W, H)
            if name == "mirrored":
                plane = np.array([h.valid != 0 and h.object == 0 and h.primitive == 0 for h in hits])
                heading_down = np.array([d[1] < 0 for _, d in rays])
                assert plane.sum() > 100 and (~valid & ~heading_down).sum() > 100
                assert not (plane & ~heading_down).any()


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", list(POSES))
def test_cull_is_bit_identical_under_a_pose(name, frame, main_spec):
    W, H, tile = FRAMES[frame]
    ds = _posed(main_spec, POSES[name])
    (a, ca), (b, cb) = _cull_pair(ds, W, H, tile)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert ca["samples"] == tile.width() * tile.height() * 2 and cb["samples"] <= ca["samples"]
    assert a.count_nonzero() > tile.width() * tile.height()  # the weights, and colour where rays hit


def test_posed_cull_does_cull(main_spec):
    W, H = 128, 96
    tile = Tile(0, W, 0, H)
    for name in ("look_at", "up"):  # the box projection test; the bounding-sphere fallback
        ds = _posed(main_spec, POSES[name])
        (a, ca), (b, cb) = _cull_pair(ds, W, H, tile)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
        assert ca["samples"] == W * H * 2
        assert 0 < cb["samples"] < ca["samples"], name


def test_looking_away_culls_everything(mesh):
    """No plane in the scene and the mesh behind the camera: every block is culled, and the state is the
    one of W * H * spp missed camera rays."""
    spec = scenes.bench_scene(mesh).spec()
    eye = np.array(spec.camera_location)
    away = look_at(eye, 2.0 * eye - np.array(CENTRE), (0.0, 1.0, 0.0), 1.0)
    W, H, tile = FRAMES["wide"]
    ds = _posed(spec, away)
    (a, ca), (b, cb) = _cull_pair(ds, W, H, tile)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert ca["samples"] == tile.width() * tile.height() * 2 and cb["samples"] == 0
    weights = a.numpy()[:4 * tile.width() * tile.height()].reshape(-1, 4)
    assert (weights[:, 3] == 5.0).all() and not weights[:, :3].any()


# ------------------------------------------------------------------ 6. the film and the other edits
def test_film_under_a_pose(main_spec):
    W, H = 40, 24
    pose = POSES["look_at"]
    ds = _posed(main_spec, pose)
    tiles = [Tile(0, 24, 0, 16), Tile(24, 40, 0, 16), Tile(0, 24, 16, 24), Tile(24, 40, 16, 24), Tile(3, 37, 2, 21)]
    want = AccumulationBuffer(W, H)
    with Film(W, H) as film:
        for k, t in enumerate(tiles):
            assert film.render_tile(ds, t, 2, 11, 2 * k) == (k, 2 * k)
            want.merge_tile(t, render_tile(ds, t, H, W, 2, 11, 2 * k))
        got, seen = film.read()
    assert seen == len(tiles)
    assert np.array_equal(got.colour_buffer, want.colour_buffer) and np.array_equal(got.weight_buffer, want.weight_buffer)
    default = AccumulationBuffer(W, H)
    plain = DeviceScene(main_spec, 0)
    for k, t in enumerate(tiles):
        default.merge_tile(t, render_tile(plain, t, H, W, 2, 11, 2 * k))
    assert not np.array_equal(got.colour_buffer, default.colour_buffer)


def test_a_pose_survives_the_other_edits(mesh, main_spec):
    v, n = mesh
    W, H, tile = FRAMES["wide"]
    pose = POSES["look_at"]
    turn = rotation_about(0.6, CENTRE, (0.4, 0.1, -0.2))
    cyan = MaterialSpec(N.MATERIAL_LAMBERTIAN, Spectrum.reflection_from_linear_rgb(ColourRgbF.from_named(NamedColour.Cyan)),
                        0.08)
    w, wn = v * np.array([1.0, 0.9, 1.0]) + np.array([0.1, 0.0, 0.0]), n
    edits = {
        "transform_mesh": (lambda ds: ds.transform_mesh(0, turn), dict(meshes={0: transformed(turn, v, n)})),
        "update_mesh": (lambda ds: ds.update_mesh(0, w, wn), dict(meshes={0: (w, wn)})),
        "update_material": (lambda ds: ds.update_material(3, cyan), dict(materials={3: cyan})),
    }
    for what, (edit, replaced) in edits.items():
        ds = _posed(main_spec, pose)
        before = _state(ds, W, H, tile)[0]
        edit(ds)
        assert pose_bits(ds.camera_pose()) == pose_bits(pose), what
        after = _state(ds, W, H, tile)[0]
        fresh = _posed(edited_spec(main_spec, **replaced), pose)
        assert np.array_equal(_bits(after), _bits(_state(fresh, W, H, tile)[0])), what
        assert not np.array_equal(_bits(after), _bits(before)), what
    # the lights of a Whitted scene
    spec = scenes.whitted_scene(mesh).spec()
    lights = WhittedIntegrator(Spectrum.grey(0.02), [
        DirectionalLight((-0.7, 0.6, -0.4), Spectrum.reflection_from_linear_rgb(ColourRgbF.new(0.9, 0.5, 0.3))),
        spec.integrator.lights[1]])
    ds = _posed(spec, mirrored(pose))
    before = _state(ds, W, H, tile)[0]
    ds.set_lights(lights)
    assert pose_bits(ds.camera_pose()) == pose_bits(mirrored(pose))
    after = _state(ds, W, H, tile)[0]
    fresh = _posed(edited_spec(spec, integrator=lights), mirrored(pose))
    assert np.array_equal(_bits(after), _bits(_state(fresh, W, H, tile)[0]))
    assert not np.array_equal(_bits(after), _bits(before))
    # and vr_scene_set_camera moves the posed camera without turning it
    ds.set_camera((0.6, 0.3, -2.5))
    moved = CameraPose((0.6, 0.3, -2.5), *[getattr(mirrored(pose), f) for f in ("right", "up", "forward", "film_distance")])
    assert pose_bits(ds.camera_pose()) == pose_bits(moved)
    fresh.set_camera_pose(moved)
    assert np.array_equal(_bits(_state(ds, W, H, tile)[0]), _bits(_state(fresh, W, H, tile)[0]))
