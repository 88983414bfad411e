"""The camera lens (VR_HAS_CAMERA_LENS) on the device: the render kernel's camera step under a lens (the
CAM = 2 instantiations of vanrijn_amd/csrc/vr_render_kernel.h), camera_rays_kernel and the block cull.

The chain of evidence, as tests/test_gpu_camera_pose.py builds it for the pose:
  1. a lens of radius 0 set explicitly changes no bit and not the kernel;
  2. camera_rays_device equals vr_camera_lens_ray -- the lens rule on the host, pinned to its restatement in
     tests/test_camera_lens_host.py -- with draws 0 to 3 rebuilt from the oracle's own stream functions;
  3. with those rays the pinned integrator (vr_integrate_rays_device, first_draw = 4) gives the lens
     megakernel's records bit for bit, and accumulated they give its state; the first hits are the oracle's
     trace of the same rays;
  4. the block cull keeps every block only the lens reaches;
  5. the block cull changes no bit under pose and lens, still culls, and survives a huge lens;
  6. the film and the other scene edits see the lens, and turning it off restores the pinhole.
"""
import numpy as np
import pytest
import torch

from camera_lens_checks import lens_bits, lens_rule_ray
from camera_pose_checks import pose_bits, poses
from scene_edit_checks import edited_spec, rotation_about, transformed
from test_gpu_camera_pose import FRAMES, SEED, SPP, _bits, _cull_pair, _device_rays, _staging_order, _state
from test_gpu_scene_edit import CENTRE, _main_like
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import (PATH_INFO_DTYPE, PHOTON_DTYPE, AccumulationBuffer, Film, Tile, accumulate_photons_device,
                                integrate_rays_device, render_samples, render_tile, stream_check_error)
from vanrijn_amd.scene import (CameraLens, CameraPose, ColourRgbF, DeviceScene, LambertianMaterial, MaterialSpec,
                               NamedColour, Scene, Spectrum, Sphere)

pytestmark = pytest.mark.gpu

POSES = poses()
LENS = CameraLens(0.15, 5.0)  # the main-like scene's mesh is about 5 in front of its camera


@pytest.fixture(scope="module")
def mesh():
    return scenes.displaced_mesh(16, scenes._BUNNY_BUMPS, noise_seed=0xB0BB1E, noise_count=48, noise_amp=0.04,
                                 scale=(1.25, 1.05, 1.15), centre=CENTRE)


@pytest.fixture(scope="module")
def main_spec(mesh):
    return _main_like(*mesh).spec()


def _draws(oracle, W, row, col, sample, seed=SEED):
    """Draws 0 to 3 of the (pixel, sample) stream as Standard f64: ux, uy, lu, lv."""
    L = oracle.lib()
    base = L.orc_stream_base(seed, row * W + col, sample)
    return tuple(L.orc_u64_to_standard(L.orc_stream_draw(base, k)) for k in range(4))


def _host_rays(oracle, pose, lens, W, H, tile, spp, first_sample=0):
    """vr_camera_lens_ray for every (sample, pixel) of the tile in [s][p] order, with the oracle's draws."""
    tw, n = tile.width(), tile.width() * tile.height()
    o, d, ids = np.empty((spp, n, 3)), np.empty((spp, n, 3)), np.empty((spp, n), dtype=np.uint64)
    for s in range(spp):
        for p in range(n):
            row, col = tile.start_row + p // tw, tile.start_column + p % tw
            ux, uy, lu, lv = _draws(oracle, W, row, col, first_sample + s)
            o[s, p], d[s, p] = pose.ray(W, H, row, col, ux, uy, lens=lens, lu=lu, lv=lv)
            ids[s, p] = ((row * W + col) << 32) + first_sample + s
    return o.reshape(-1, 3), d.reshape(-1, 3), ids.reshape(-1)


def _with_lens(spec, pose=None, lens=LENS, **flags):
    ds = DeviceScene(spec, 0, **flags)
    if pose is not None:
        ds.set_camera_pose(pose)
    ds.set_camera_lens(lens)
    return ds


def _pose_of(spec, name):
    return CameraPose(location=spec.camera_location) if name == "default" else POSES[name]


# ------------------------------------------------------------------ 1. lens off
@pytest.mark.parametrize("frame", list(FRAMES))
def test_lens_of_radius_zero_changes_nothing(frame, main_spec):
    W, H, tile = FRAMES[frame]
    for pose in (None, POSES["look_at"]):
        plain, explicit = _with_lens(main_spec, pose, CameraLens(0.0, 1.0)), _with_lens(main_spec, pose, CameraLens(0.0, 7.5))
        untouched = DeviceScene(main_spec, 0)
        if pose is not None:
            untouched.set_camera_pose(pose)
        assert lens_bits(explicit.camera_lens()) == lens_bits(CameraLens(0.0, 7.5))
        recs = [render_samples(ds, tile, H, W, 4, SEED) for ds in (untouched, plain, explicit)]
        assert recs[0].tobytes() == recs[1].tobytes() == recs[2].tobytes()
        states = [_state(ds, W, H, tile) for ds in (untouched, plain, explicit)]
        assert states[0][0].tobytes() == states[1][0].tobytes() == states[2][0].tobytes()
        assert states[0][1]["variant"] == states[1][1]["variant"] == states[2][1]["variant"]
        for x, y in zip(_device_rays(untouched, W, H, tile, SPP), _device_rays(explicit, W, H, tile, SPP)):
            assert torch.equal(x.view(torch.int64), y.view(torch.int64))


# ------------------------------------------------------------------ 2. camera_rays_device against the lens rule
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", ["default", "look_at"])
def test_camera_rays_device_equals_the_lens_rule(name, frame, main_spec, oracle):
    W, H, tile = FRAMES[frame]
    pose = _pose_of(main_spec, name)
    ds = _with_lens(main_spec, None if name == "default" else pose)
    for first in (0, 5):
        o, d, ids = _device_rays(ds, W, H, tile, SPP, first)
        ho, hd, hids = _host_rays(oracle, pose, LENS, W, H, tile, SPP, first)
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(ho.reshape(-1)))
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(hd.reshape(-1)))
        assert np.array_equal(ids.cpu().numpy().view(np.uint64), hids)
    assert len(np.unique(ho, axis=0)) > len(ho) // 2  # origins vary per entry
    # one pixel against the restated rule itself (tests/test_camera_lens_host.py pins the rule on the host)
    row, col = tile.start_row, tile.start_column
    ro, rd = lens_rule_ray(oracle, pose, LENS, W, H, row, col, *_draws(oracle, W, row, col, 5))
    assert ro.tobytes() == ho[0].tobytes() and rd.tobytes() == hd[0].tobytes()


# ------------------------------------------------------------------ 3. the megakernel, the integrator, the oracle
def _check_megakernel(ds, pose, lens, W, H, tile, oracle=None, orc_scene=None, **launch):
    """The lens render's records and state against the staged pipeline over camera_rays_device's rays."""
    npix = tile.width() * tile.height()
    n = npix * SPP
    o, d, ids = _device_rays(ds, W, H, tile, SPP)
    ph = torch.full((n, 2), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    staged = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    integrate_rays_device(ds, n, o.data_ptr(), d.data_ptr(), ph.data_ptr(), SEED, stream_ids_ptr=ids.data_ptr(),
                          info_ptr=info.data_ptr(), first_draw=4)
    accumulate_photons_device(staged.data_ptr(), ph.data_ptr(), npix, SPP)
    torch.cuda.synchronize()
    stream_check_error(ds)
    photons = ph.cpu().numpy().reshape(-1).view(PHOTON_DTYPE)
    paths = info.cpu().numpy().reshape(-1).view(PATH_INFO_DTYPE)
    rec = _staging_order(render_samples(ds, tile, H, W, SPP, SEED))
    assert np.array_equal(_bits(photons["wavelength"]), _bits(rec["wavelength"]))
    assert np.array_equal(_bits(photons["intensity"]), _bits(rec["intensity"]))
    assert np.array_equal(paths["bounces"], rec["bounces"]) and np.array_equal(paths["flags"], rec["flags"])
    state, stats = _state(ds, W, H, tile, **launch)
    assert np.array_equal(_bits(state), _bits(staged.cpu().numpy()))
    hit = (rec["flags"] & 1) != 0
    assert 0 < hit.sum() < n  # hits and misses in frame
    if orc_scene is not None:  # first hits: the oracle's trace of the lens rule's rays
        ho, hd, _ = _host_rays(oracle, pose, lens, W, H, tile, SPP)
        hits, _ = orc_scene.trace(ho, hd)
        assert np.array_equal(np.array([h.valid != 0 for h in hits]), hit)
    return rec, stats


@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("name", ["default", "look_at"])
def test_megakernel_equals_the_pinned_integrator(name, frame, main_spec, oracle):
    W, H, tile = FRAMES[frame]
    pose = _pose_of(main_spec, name)
    ds = _with_lens(main_spec, None if name == "default" else pose)
    rec, _ = _check_megakernel(ds, pose, LENS, W, H, tile, oracle, oracle.OracleScene(main_spec))
    ds.set_camera_lens(CameraLens(0.0, 1.0))
    pinhole = _staging_order(render_samples(ds, tile, H, W, SPP, SEED))
    assert rec.tobytes() != pinhole.tobytes()


def test_megakernel_on_the_reflective_scene(mesh, oracle):
    """The bench scene: reflective paths and the cooperative tail's instantiation."""
    spec = scenes.bench_scene(mesh).spec()
    W, H, tile = FRAMES["tall"]
    pose = POSES["look_at"]
    ds = _with_lens(spec, pose)
    rec, stats = _check_megakernel(ds, pose, LENS, W, H, tile, oracle, oracle.OracleScene(spec))
    assert stats["variant"] & N.VARIANT_COOP
    assert rec["bounces"].max() >= 2


def test_megakernel_on_a_whitted_scene(mesh, oracle):
    spec = scenes.whitted_scene(mesh).spec()
    W, H, tile = FRAMES["tall"]
    pose = POSES["mirrored"]
    _check_megakernel(_with_lens(spec, pose), pose, LENS, W, H, tile, oracle, oracle.OracleScene(spec))


def test_megakernel_with_wide_offsets_and_32_bit_stacks(main_spec):
    """The lens instantiations of the 64-bit-offset kernels and of the 32-bit stack entries run too."""
    W, H, tile = FRAMES["wide"]
    pose = _pose_of(main_spec, "default")
    _, wide = _check_megakernel(_with_lens(main_spec, wide_offsets=True), pose, LENS, W, H, tile)
    assert wide["variant"] & N.VARIANT_WIDE_OFFSETS
    ds = _with_lens(main_spec)
    _, s16 = _check_megakernel(ds, pose, LENS, W, H, tile)
    _, s32 = _check_megakernel(ds, pose, LENS, W, H, tile, stack16=False)
    assert s16["variant"] & N.VARIANT_STACK16 and not s32["variant"] & N.VARIANT_STACK16


# ------------------------------------------------------------------ 4. the cull does not cut lens hits
def _sphere_blocks(pose, lens, W, H, centre, radius):
    """Per 8x8 block: does a pinhole ray reach the sphere, does a lens ray (vr_camera_lens_ray over a grid of
    lens points, jitter at the pixel's centre and corners)?"""
    centre = np.array(centre)

    def reaches(o, d):
        v = centre - o
        t = np.dot(v, d)
        return t > 0 and np.dot(v, v) - t * t < radius * radius

    top = 1.0 - 2.0 ** -53
    jitters = [(0.5, 0.5), (0.0, 0.0), (top, 0.0), (0.0, top), (top, top)]
    grid = [(u, v) for u in np.linspace(0.0, top, 7) for v in np.linspace(0.0, top, 7)]
    pin = np.zeros(((H + 7) // 8, (W + 7) // 8), dtype=bool)
    through = np.zeros_like(pin)
    for row in range(H):
        for col in range(W):
            b = (row // 8, col // 8)
            pin[b] |= any(reaches(*pose.ray(W, H, row, col, ux, uy)) for ux, uy in jitters)
            through[b] |= any(reaches(*pose.ray(W, H, row, col, 0.5, 0.5, lens=lens, lu=lu, lv=lv)) for lu, lv in grid)
    return pin, through


def test_cull_keeps_the_blocks_only_the_lens_reaches():
    W, H = 40, 24
    tile = Tile(0, W, 0, H)
    centre, radius = (0.0, 0.0, 1.5), 0.1
    spec = Scene((0.0, 0.0, 0.0), [[Sphere(centre, radius, LambertianMaterial(Spectrum.grey(0.6), 0.1))]]).spec()
    lens = CameraLens(0.4, 12.0)
    pin, through = _sphere_blocks(CameraPose(), lens, W, H, centre, radius)
    assert pin.size == 15 and pin.sum() == 1
    assert (through & ~pin).sum() >= 4  # the case is met: blocks reached through the lens alone
    ds = _with_lens(spec, None, lens)
    (a, ca), (b, cb) = _cull_pair(ds, W, H, tile)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert ca["samples"] == W * H * 2 and cb["samples"] <= ca["samples"]
    # the sphere shows in blocks the pinhole never reaches it from
    colour = a.numpy()[:4 * W * H].reshape(H, W, 4)[..., :3].any(axis=2)  # the sums {X, Y, Z, weight}
    lit = np.array([[colour[8 * r:8 * r + 8, 8 * c:8 * c + 8].any() for c in range(5)] for r in range(3)])
    assert (lit & ~pin).sum() >= 1
    no_lens = DeviceScene(spec, 0)
    (p, _), (q, _) = _cull_pair(no_lens, W, H, tile)
    assert torch.equal(p.view(torch.int64), q.view(torch.int64)) and not torch.equal(p.view(torch.int64), a.view(torch.int64))


# ------------------------------------------------------------------ 5. the cull still culls, and a huge lens
@pytest.mark.parametrize("name", list(POSES))
def test_cull_is_bit_identical_and_culls_under_pose_and_lens(name, main_spec):
    W, H = 128, 96
    tile = Tile(0, W, 0, H)
    ds = _with_lens(main_spec, POSES[name], CameraLens(0.05, 5.0))
    (a, ca), (b, cb) = _cull_pair(ds, W, H, tile)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert ca["samples"] == W * H * 2
    print(name, "traced samples with the cull", cb["samples"], "of", ca["samples"])
    assert cb["samples"] < ca["samples"], name
    assert a.count_nonzero() > W * H


@pytest.mark.parametrize("frame", list(FRAMES))
def test_cull_is_bit_identical_in_small_frames_and_under_a_huge_lens(frame, main_spec):
    W, H, tile = FRAMES[frame]
    for name, lens in (("look_at", CameraLens(0.05, 5.0)), ("up", CameraLens(0.05, 5.0)), ("mirrored", CameraLens(0.05, 5.0)),
                       ("look_at", CameraLens(50.0, 5.0)), ("mirrored", CameraLens(50.0, 1e-3))):
        ds = _with_lens(main_spec, POSES[name], lens)
        (a, ca), (b, cb) = _cull_pair(ds, W, H, tile)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), (name, lens)
        assert ca["samples"] == tile.width() * tile.height() * 2 and cb["samples"] <= ca["samples"]


# ------------------------------------------------------------------ 6. the film and the other edits
def test_film_under_a_lens(main_spec):
    W, H = 40, 24
    ds = _with_lens(main_spec, POSES["look_at"])
    tiles = [Tile(0, 24, 0, 16), Tile(24, 40, 0, 16), Tile(0, 24, 16, 24), Tile(24, 40, 16, 24), Tile(3, 37, 2, 21)]
    want = AccumulationBuffer(W, H)
    with Film(W, H) as film:
        for k, t in enumerate(tiles):
            assert film.render_tile(ds, t, 2, 11, 2 * k) == (k, 2 * k)
            want.merge_tile(t, render_tile(ds, t, H, W, 2, 11, 2 * k))
        got, seen = film.read()
    assert seen == len(tiles)
    assert np.array_equal(got.colour_buffer, want.colour_buffer) and np.array_equal(got.weight_buffer, want.weight_buffer)
    pinhole = AccumulationBuffer(W, H)
    ds.set_camera_lens(CameraLens(0.0, 5.0))
    for k, t in enumerate(tiles):
        pinhole.merge_tile(t, render_tile(ds, t, H, W, 2, 11, 2 * k))
    assert not np.array_equal(got.colour_buffer, pinhole.colour_buffer)


def test_a_lens_survives_the_other_edits_and_can_be_turned_off(mesh, main_spec):
    v, n = mesh
    W, H, tile = FRAMES["wide"]
    pose = POSES["look_at"]
    turn = rotation_about(0.6, CENTRE, (0.4, 0.1, -0.2))
    cyan = MaterialSpec(N.MATERIAL_LAMBERTIAN, Spectrum.reflection_from_linear_rgb(ColourRgbF.from_named(NamedColour.Cyan)),
                        0.08)
    edits = {
        "transform_mesh": (lambda ds: ds.transform_mesh(0, turn), dict(meshes={0: transformed(turn, v, n)})),
        "update_material": (lambda ds: ds.update_material(3, cyan), dict(materials={3: cyan})),
    }
    for what, (edit, replaced) in edits.items():
        ds = _with_lens(main_spec, pose)
        before = _state(ds, W, H, tile)[0]
        edit(ds)
        assert lens_bits(ds.camera_lens()) == lens_bits(LENS), what
        after = _state(ds, W, H, tile)[0]
        fresh = _with_lens(edited_spec(main_spec, **replaced), pose)
        assert np.array_equal(_bits(after), _bits(_state(fresh, W, H, tile)[0])), what
        assert not np.array_equal(_bits(after), _bits(before)), what
    # set_camera_pose keeps the lens: the default-pose lens scene turned equals a scene posed first
    ds = _with_lens(main_spec)
    ds.set_camera_pose(pose)
    assert lens_bits(ds.camera_lens()) == lens_bits(LENS) and pose_bits(ds.camera_pose()) == pose_bits(pose)
    lens_state = _state(ds, W, H, tile)[0]
    assert np.array_equal(_bits(lens_state), _bits(_state(_with_lens(main_spec, pose), W, H, tile)[0]))
    # turning the lens off again restores the pinhole's records
    pinhole = DeviceScene(main_spec, 0)
    pinhole.set_camera_pose(pose)
    want = render_samples(pinhole, tile, H, W, SPP, SEED)
    assert render_samples(ds, tile, H, W, SPP, SEED).tobytes() != want.tobytes()
    ds.set_camera_lens(CameraLens(0.0, LENS.focus_distance))
    assert render_samples(ds, tile, H, W, SPP, SEED).tobytes() == want.tobytes()
    assert np.array_equal(_bits(_state(ds, W, H, tile)[0]), _bits(_state(pinhole, W, H, tile)[0]))
    assert not np.array_equal(_bits(lens_state), _bits(_state(pinhole, W, H, tile)[0]))
