"""The single-BVH instantiations of the render kernel (render_kernel<.., ONE>, VR_VARIANT_ONE_BVH) against
the generic ones (VR_LAUNCH_MULTI_BVH), through the C ABI on the GPU.

A scene whose BVH list is one mesh with a wide root runs timed kernels without the list walk: start_bvhs
is straight-line code for BVH 0, phase B has no "next BVH" step, and the walked BVH's object is a
wave-uniform value in the tie rule (takes_hit), in leaf_round's fold and in the material lookup.  It removes
only code such a scene never takes, so every case renders once with the default choice and once with
VR_LAUNCH_MULTI_BVH and compares the raw device records bit for bit; both launches' variant bits are
checked.  64 x 64 @4 is 16 K work items over 64 workgroups: each wave sees camera rays, bounce rays,
root-box misses, lanes whose stack ran empty and leaf rounds.

test_gpu_ties.py has no cross-object tie with a single mesh (its second object is a second mesh, and a
primitive's distance comes out of another formula than a triangle's, so they do not meet bit for bit);
the "earlier object across objects" side of the rule runs here whenever a mesh hit is weighed against a
primitive's, with unequal distances.

Scenes that must keep the generic kernel (two meshes, a one-triangle mesh, a launch small enough for the
cooperative tail) report so and render what the oracle renders.
"""
import numpy as np
import pytest
import torch

from camera_pose_checks import poses
from test_gpu_launch_variants import _decisions_equal, _mirror_bunny_on_a_plane, _two_mirror_scene
from test_gpu_scene_edit import CENTRE, _main_like
from test_gpu_ties import _tied_scene
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import Tile, render_samples, render_tile, render_tile_device
from vanrijn_amd.scene import (BoundingVolumeHierarchy, CameraLens, DeviceScene, LambertianMaterial, Mesh, Plane, Scene,
                               Spectrum)

pytestmark = pytest.mark.gpu

SEED = 0x5EED0001
ONE, S16, COOP = N.VARIANT_ONE_BVH, N.VARIANT_STACK16, N.VARIANT_COOP


def _pair(ds, tile, H, W, spp, one_variant, multi_variant, more=0, **kw):
    """The records of the default launch and of the VR_LAUNCH_MULTI_BVH one (then `more` samples added onto
    each), as int64 tensors; asserts the variant bits both report."""
    out = []
    for one_bvh, want in ((True, one_variant), (False, multi_variant)):
        st = torch.zeros(tile.width() * tile.height() * 8, dtype=torch.float64, device="cuda")
        s = render_tile_device(ds, tile, H, W, spp, SEED, 0, st.data_ptr(), one_bvh=one_bvh, **kw)
        assert s["variant"] == want
        if more:
            s = render_tile_device(ds, tile, H, W, more, SEED, spp, st.data_ptr(), accumulate=True, one_bvh=one_bvh, **kw)
            assert s["variant"] == want
        torch.cuda.synchronize()
        out.append(st.cpu().view(torch.int64))
    return out


@pytest.fixture(scope="module")
def main_ds():
    return scenes.main_scene().device_scene(0)


@pytest.mark.parametrize("case", ["fresh", "continued", "cut_blocks", "stack32"])
def test_main_scene_is_bit_identical(case, main_ds):
    H = W = 64
    tile = Tile(5, 59, 3, 61) if case == "cut_blocks" else Tile(0, W, 0, H)
    if case == "stack32":  # the 32-bit-stack instantiation
        a, b = _pair(main_ds, tile, H, W, 4, ONE, 0, stack16=False)
    else:
        a, b = _pair(main_ds, tile, H, W, 4, ONE | S16, S16, more=3 if case == "continued" else 0)
    assert torch.equal(a, b)
    assert np.count_nonzero(a.numpy()) > 1000


def test_general_material_kernel_with_a_32_bit_stack_is_bit_identical():
    """The DARK0 = false kernel's single-BVH instantiation with 32-bit stack entries (the materials scene: a
    Phong and a glass sphere beside the bunny), a 16 x 16 tile @2 on the bunny."""
    ds = scenes.materials_scene().device_scene(0)
    a, b = _pair(ds, Tile(72, 88, 72, 88), 128, 128, 2, ONE, 0, stack16=False)
    assert torch.equal(a, b)
    assert np.count_nonzero(a.numpy()) > 100


@pytest.mark.parametrize("scene", ["mirror", "mixed"])
@pytest.mark.parametrize("stack16", [True, False])
def test_large_launches_of_mirror_scenes_are_bit_identical(scene, stack16):
    """A scene with a reflective material takes the single-BVH kernels only in a launch too large for the
    cooperative tail (more than 4 Mi pixel-samples: vr_host.cpp coop_gated), so 512 x 512 @17 here and not a
    small tile: benches/simple_scene.rs (the reflective-only kernels) and its bunny over a Lambertian plane
    (the kernels of both kinds), with 16- and with 32-bit stack entries."""
    ds = (scenes.bench_scene() if scene == "mirror" else _mirror_bunny_on_a_plane()).device_scene(0)
    s16 = S16 if stack16 else 0
    a, b = _pair(ds, Tile(0, 512, 0, 512), 512, 512, 17, ONE | s16, s16, stack16=stack16)
    assert torch.equal(a, b)
    assert np.count_nonzero(a.numpy()) > 10000


def test_debug_flag_forces_the_generic_kernel(main_ds):
    """vr_debug_set_launch_flags honours VR_LAUNCH_MULTI_BVH (every later render of the scene)."""
    ds = DeviceScene(scenes.main_scene().spec(), 0)
    ds.set_launch_flags(multi_bvh=True)
    st = torch.zeros(64 * 64 * 8, dtype=torch.float64, device="cuda")
    s = render_tile_device(ds, Tile(0, 64, 0, 64), 64, 64, 4, SEED, 0, st.data_ptr())
    torch.cuda.synchronize()
    assert s["variant"] == S16
    a, _ = _pair(main_ds, Tile(0, 64, 0, 64), 64, 64, 4, ONE | S16, S16)
    assert torch.equal(st.cpu().view(torch.int64), a)


@pytest.mark.parametrize("lens", [False, True])
def test_posed_cameras_are_bit_identical(lens):
    """The CAM = 1 (posed) and CAM = 2 (posed, with a lens) instantiations, on the scene the poses were
    chosen for."""
    mesh = scenes.displaced_mesh(16, scenes._BUNNY_BUMPS, noise_seed=0xB0BB1E, noise_count=48, noise_amp=0.04,
                                 scale=(1.25, 1.05, 1.15), centre=CENTRE)
    ds = DeviceScene(_main_like(*mesh).spec(), 0)
    ds.set_camera_pose(poses()["look_at"])
    if lens:
        ds.set_camera_lens(CameraLens(0.15, 5.0))
    a, b = _pair(ds, Tile(0, 48, 0, 48), 48, 48, 2, ONE | S16, S16)
    assert torch.equal(a, b)
    assert np.count_nonzero(a.numpy()) > 1000


@pytest.mark.parametrize("seed", [1, 2])
def test_tied_triangles_with_a_uniform_object(seed, oracle):
    """test_gpu_ties.py's first mesh alone (every triangle two or three times at the same place): the later
    in-order leaf wins each tie, with the walked BVH's object a wave-uniform value in the rule."""
    both = _tied_scene(seed)
    scene = Scene(both.camera_location, both.objects[:2])  # the plane and the first mesh
    ds = scene.device_scene(0)
    H = W = 64
    t = Tile(0, W, 0, H)
    a, b = _pair(ds, t, H, W, 6, ONE | S16, S16)
    assert torch.equal(a, b)
    orc = oracle.OracleScene(scene.spec())
    ref = orc.render_samples(t, H, W, 6, seed=0x7135 + seed, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert (ref["flags"] & 1).sum() > 1000  # the camera sees the tied mesh
    _decisions_equal(render_samples(ds, t, H, W, 6, seed=0x7135 + seed), ref)
    # the timed kernel (the single-BVH one) against the oracle's image of the same samples
    img = render_tile(ds, t, H, W, 6, seed=0x7135 + seed)
    refi = orc.render_tile(t, H, W, 6, seed=0x7135 + seed, mode=oracle.MODE_PRUNED, nthreads=8)
    assert np.linalg.norm(img.colour_buffer - refi["colour"], axis=2).max() < 1e-5
    assert np.array_equal(img.weight_buffer, refi["weight"])


def _against_the_oracle(scene, ds, oracle, H, W, spp):
    t = Tile(0, W, 0, H)
    orc = oracle.OracleScene(scene.spec())
    img = render_tile(ds, t, H, W, spp, seed=SEED)
    refi = orc.render_tile(t, H, W, spp, seed=SEED, mode=oracle.MODE_PRUNED, nthreads=8)
    assert np.linalg.norm(img.colour_buffer - refi["colour"], axis=2).max() < 1e-5
    assert np.array_equal(img.weight_buffer, refi["weight"])
    _decisions_equal(render_samples(ds, t, H, W, 2, seed=SEED), orc.render_samples(t, H, W, 2, seed=SEED,
                                                                                   mode=oracle.MODE_PRUNED, nthreads=8))


def test_two_meshes_keep_the_generic_kernel(oracle):
    scene = _two_mirror_scene()
    ds = scene.device_scene(0)
    a, b = _pair(ds, Tile(0, 64, 0, 64), 64, 64, 4, COOP, COOP)
    assert torch.equal(a, b)
    a, b = _pair(ds, Tile(0, 64, 0, 64), 64, 64, 4, S16, S16, coop=False)
    assert torch.equal(a, b)
    _against_the_oracle(scene, ds, oracle, 64, 64, 4)


def test_one_triangle_mesh_keeps_the_generic_kernel(oracle):
    mat = LambertianMaterial(Spectrum.grey(0.7), 0.4)
    v = np.array([[[-1.5, -1.0, 0.5], [1.5, -1.2, 0.0], [0.2, 1.4, -0.3]]])
    n = np.array([[[0.1, 0.2, -1.0], [-0.2, 0.1, -1.0], [0.0, -0.1, -1.0]]])
    scene = Scene((0.0, 0.0, -4.0), [[Plane((0.0, 1.0, 0.0), -1.5, LambertianMaterial(Spectrum.grey(0.5), 0.5))],
                                     BoundingVolumeHierarchy.build(Mesh(v, n, mat))])
    ds = scene.device_scene(0)
    a, b = _pair(ds, Tile(0, 64, 0, 64), 64, 64, 4, S16, S16)
    assert torch.equal(a, b)
    _against_the_oracle(scene, ds, oracle, 64, 64, 4)


def test_small_bench_launches_keep_the_cooperative_tail(oracle):
    """benches/simple_scene.rs at 64 x 64 @4 is small enough for the cooperative tail: the COOP kernel runs,
    and without the tail (VR_LAUNCH_NO_COOP) the generic kernel it is compared with."""
    scene = scenes.bench_scene()
    ds = scene.device_scene(0)
    a, b = _pair(ds, Tile(0, 64, 0, 64), 64, 64, 4, COOP, COOP)
    assert torch.equal(a, b)
    a, b = _pair(ds, Tile(0, 64, 0, 64), 64, 64, 4, S16, S16, coop=False)
    assert torch.equal(a, b)
    _against_the_oracle(scene, ds, oracle, 64, 64, 4)
