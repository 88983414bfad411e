"""vr_scene_update_mesh on the device (vanrijn_amd/csrc/vr_refit.hip): new vertices for a mesh of a
resident scene, both trees refitted in place, one launch per tree level.

Bar: the device refit stores what the host refit stores (tests/test_scene_update_host.py pins that one
against numpy), and an updated scene answers every entry point bit for bit like a scene created from
the new geometry -- the closest hit depends only on each triangle's own box and its mesh's root box
(DESIGN.md section 5), which an exact refit reproduces.
"""
import numpy as np
import pytest

import magnitude_scenes as M
from scene_update_checks import assert_dumps_equal, check_refit, dumps
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import (Tile, integrate_rays, query_closest, render_samples, render_tile_device)
from vanrijn_amd.scene import (BoundingVolumeHierarchy, ColourRgbF, DeviceScene, LambertianMaterial, Mesh, NamedColour,
                               Plane, Scene, Sphere, Spectrum)

pytestmark = pytest.mark.gpu

FLAG_SETS = {"default": {}, "reference_bvh": {"reference_bvh": True}, "device_bvh": {"device_bvh": True},
             "device_sah": {"device_sah": True}, "wide_offsets": {"wide_offsets": True}}


def _normals(v):
    n = np.zeros_like(v)
    n[..., 2] = 1.0
    return n


def _random_scene(v):
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    return Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(v, _normals(v), mat))])


def _pair(n):
    a = np.random.default_rng(n).normal(size=(n, 3, 3))
    b = 3.0 * np.random.default_rng(1000 + n).normal(size=(n, 3, 3)) + 0.5
    return a, b


# ------------------------------------------------------------------ the refit itself
@pytest.mark.parametrize("reference_bvh", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 1000, 4097])
def test_device_refit_equals_host_refit(n, reference_bvh):
    """A device scene and a host-only scene of one Scene share the host-built topology: after the
    same update their four dumps are equal (1: the root is a leaf; 4097: many workgroups and levels)."""
    a, b = _pair(n)
    spec = _random_scene(a).spec()
    dev = DeviceScene(spec, 0, reference_bvh=reference_bvh)
    host = DeviceScene(spec, 0, host_only=True, reference_bvh=reference_bvh)
    assert_dumps_equal(dumps(dev), dumps(host))
    bytes_before = dev.info()["device_bytes"]
    dev.update_mesh(0, b, _normals(b))
    host.update_mesh(0, b, _normals(b))
    assert_dumps_equal(dumps(dev), dumps(host))
    for key in ("extent", "nan_free", "node_count", "wide_node_count", "traversal_stack", "max_bvh_depth"):
        assert dev.info()[key] == host.info()[key], key
    assert dev.info()["device_bytes"] > bytes_before  # the plan is resident and counted


@pytest.mark.parametrize("flags", ["device_bvh", "device_sah"])
@pytest.mark.parametrize("n", [2, 17, 1000])
def test_device_built_topologies(n, flags):
    a, b = _pair(n)
    ds = DeviceScene(_random_scene(a).spec(), 0, **FLAG_SETS[flags])
    before = check_refit(ds, [(a, _normals(a))])
    ds.update_mesh(0, b, _normals(b))
    check_refit(ds, [(b, _normals(b))], before)


@pytest.mark.parametrize("flags", ["device_bvh", "device_sah"])
@pytest.mark.parametrize("regime", M.REFIT_REGIMES, ids=M.regime_id)
def test_device_built_topologies_at_magnitude(regime, flags):
    """write_level_kernel / sah_level_kernel / fill_wide_kernel on a fresh scene, and the refit kernels
    after update_mesh (host arrays, then device arrays), where the bounds are beyond what f32 resolves,
    in its denormal range (1e-42), all 0 or the smallest denormal (1e-46) or beyond FLT_MAX (1e39):
    the device's __double2float_rd / ru against the exact refit's nextafter.  The update carries the
    mesh from the control into the regime and back."""
    import torch
    base, _ = _pair(257)
    nb = _normals(base)
    there = M.mapped(base, *regime)
    fresh = DeviceScene(_random_scene(there).spec(), 0, **FLAG_SETS[flags])
    check_refit(fresh, [(there, nb)])
    ds = DeviceScene(_random_scene(base).spec(), 0, **FLAG_SETS[flags])
    before = check_refit(ds, [(base, nb)])
    home = {key: ds.info()[key] for key in ("extent", "nan_free")}
    ds.update_mesh(0, there, nb)
    check_refit(ds, [(there, nb)], before)
    for key in ("extent", "nan_free"):
        assert ds.info()[key] == fresh.info()[key], key
    tn = torch.from_numpy(nb).cuda()
    for v in (base, there, base):
        tv = torch.from_numpy(np.ascontiguousarray(v)).cuda()
        ds.update_mesh_device(0, tv.data_ptr(), tn.data_ptr())
        check_refit(ds, [(v, nb)], before)
    assert {key: ds.info()[key] for key in home} == home


@pytest.mark.parametrize("flags", ["default", "device_bvh", "device_sah"])
def test_mesh_that_backs_no_object(flags):
    """No root record; a device-built median tree still has 4-wide nodes for it: refitted like any other."""
    import copy

    from vanrijn_amd.scene import MeshSpec
    a, b = _pair(17)
    c, d = _pair(5)
    spec = copy.copy(_random_scene(a).spec())
    spec.meshes = spec.meshes + [MeshSpec(c, _normals(c), 0)]
    ds = DeviceScene(spec, 0, **FLAG_SETS[flags])
    before = check_refit(ds, [(a, _normals(a)), (c, _normals(c))])
    assert len(before["roots"]) == 1
    ds.update_mesh(1, d, _normals(d))
    check_refit(ds, [(a, _normals(a)), (d, _normals(d))], before)
    assert ds.info()["extent"] == max(np.abs(a).max(), np.abs(d).max())
    ds.update_mesh(0, b, _normals(b))
    check_refit(ds, [(b, _normals(b)), (d, _normals(d))], before)


# ------------------------------------------------------------------ the same results as a fresh scene
CAMERA = scenes.CAMERA_LOCATION
W, H, SPP, SEED = 48, 40, 3, 0x5EED0001


def _mesh():
    return scenes.displaced_mesh(16, scenes._BUNNY_BUMPS, noise_seed=0xB0BB1E, noise_count=48, noise_amp=0.04,
                                 scale=(1.25, 1.05, 1.15), centre=(-1.7, -0.8, 0.0))


def _moved(v, scale):
    c = np.array([-1.7, -0.8, 0.0])
    return np.ascontiguousarray((v - c) * scale + c + np.array([0.8, 0.0, 0.0]))


def _main_like(v, n):
    def lam(c, d):
        return LambertianMaterial(Spectrum.reflection_from_linear_rgb(c), d)
    return Scene(CAMERA, [
        [Plane((0.0, 1.0, 0.0), -2.0, lam(ColourRgbF.new(0.55, 0.27, 0.04), 0.1)),
         Sphere((-6.25, -0.5, 1.0), 1.0, lam(ColourRgbF.from_named(NamedColour.Green), 0.1)),
         Sphere((-4.25, -0.5, 2.0), 1.0, lam(ColourRgbF.from_named(NamedColour.Blue), 0.1))],
        BoundingVolumeHierarchy.build(Mesh(v, n, lam(ColourRgbF.from_named(NamedColour.Yellow), 0.05)))])


def _rays(n=4096, seed=5):
    g = np.random.default_rng(seed)
    cam = np.array(CAMERA)
    d = g.uniform([-3.5, -2.5, -1.5], [0.5, 1.5, 1.5], (n, 3)) - cam
    return np.repeat(cam[None], n, 0), d / np.linalg.norm(d, axis=1, keepdims=True)


def _state(ds, w=W, h=H, spp=SPP, stream=None, **kw):
    import torch
    st = torch.zeros(h * w * 8, dtype=torch.float64, device="cuda")
    stats = render_tile_device(ds, Tile(0, w, 0, h), h, w, spp, SEED, 0, st.data_ptr(), stream_ptr=stream, timed=True,
                               **kw)
    return st.cpu().numpy(), stats


def _answers(ds):
    o, d = _rays()
    hits, rec = query_closest(ds, o, d, records=True)
    photons, info = integrate_rays(ds, o, d, seed=SEED, info=True)
    return {"samples": render_samples(ds, Tile(0, W, 0, H), H, W, SPP, SEED), "state": _state(ds)[0], "hits": hits,
            "records": rec, "photons": photons, "info": info}


def _assert_answers_equal(a, b):
    for key in a:
        x, y = a[key], b[key]
        if x.dtype.names:
            for f in x.dtype.names:
                assert np.array_equal(x[f], y[f], equal_nan=x[f].dtype.kind == "f"), (key, f)
        else:
            assert np.array_equal(x, y, equal_nan=True), key


@pytest.fixture(scope="module")
def mesh():
    return _mesh()


@pytest.mark.parametrize("scale", [0.7, 1.4])
@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_updated_scene_answers_like_a_fresh_one(flags, scale, mesh):
    v, n = mesh
    assert len(v) == 3072
    w = _moved(v, scale)
    ds = DeviceScene(_main_like(v, n).spec(), 0, **FLAG_SETS[flags])
    old = _answers(ds)
    ds.update_mesh(0, w, n)
    new = _answers(ds)
    fresh = DeviceScene(_main_like(w, n).spec(), 0, **FLAG_SETS[flags])
    _assert_answers_equal(new, _answers(fresh))
    for key in ("extent", "nan_free"):
        assert ds.info()[key] == fresh.info()[key]
    assert not np.array_equal(old["state"], new["state"])  # the mesh did move in the image
    assert (new["hits"]["valid"] != 0).sum() > 1000 and not np.array_equal(old["hits"]["distance"], new["hits"]["distance"])


def test_updated_scene_tile_against_the_oracle(mesh, oracle):
    """As tests/test_gpu_parity.py does for a fresh scene: decisions identical, intensities to 1e-12."""
    v, n = mesh
    w = _moved(v, 0.7)
    ds = DeviceScene(_main_like(v, n).spec(), 0)
    ds.update_mesh(0, w, n)
    t = Tile(8, 40, 6, 34)
    gpu = render_samples(ds, t, H, W, 4, seed=SEED)
    ref = oracle.OracleScene(_main_like(w, n).spec()).render_samples(t, H, W, 4, seed=SEED, mode=oracle.MODE_REFERENCE,
                                                                    nthreads=8)
    assert np.array_equal(gpu["flags"], ref["flags"])
    assert np.array_equal(gpu["bounces"], ref["bounces"])
    assert np.array_equal(gpu["wavelength"], ref["wavelength"])
    nz = ref["intensity"] != 0
    assert (np.abs(gpu["intensity"] - ref["intensity"])[nz] / np.abs(ref["intensity"])[nz] < 1e-12).all()
    assert np.array_equal(gpu["intensity"] == 0, ref["intensity"] == 0)
    assert (ref["flags"] & 1).sum() > 100


@pytest.mark.parametrize("coop", [True, False])
def test_reflective_scene(coop, mesh):
    """scenes.bench_scene: the cooperative-tail kernels, and without them the 16-bit-stack kernels."""
    v, n = mesh
    w = _moved(v, 0.7)
    ds = DeviceScene(scenes.bench_scene((v, n)).spec(), 0)
    ds.update_mesh(0, w, n)
    fresh = DeviceScene(scenes.bench_scene((w, n)).spec(), 0)
    a, sa = _state(ds, 64, 64, 2, coop=coop)
    b, sb = _state(fresh, 64, 64, 2, coop=coop)
    assert sa["variant"] == sb["variant"] == (N.VARIANT_COOP if coop else N.VARIANT_STACK16)
    assert np.array_equal(a, b, equal_nan=True)
    assert np.count_nonzero(a) > 1000


def test_device_pointer_form(mesh):
    """Torch tensors, updated on a non-default stream and rendered on it; the tensors are overwritten
    right after the call returns: they are no longer read."""
    import torch
    v, n = mesh
    w = _moved(v, 0.7)
    spec = _main_like(v, n).spec()
    by_host = DeviceScene(spec, 0)
    by_host.update_mesh(0, w, n)
    want = _state(by_host)[0]
    ds = DeviceScene(spec, 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tv, tn = torch.from_numpy(w).cuda(), torch.from_numpy(n).cuda()
        ds.update_mesh_device(0, tv.data_ptr(), tn.data_ptr(), s.cuda_stream)
        tv.fill_(float("nan"))
        tn.zero_()
        got = _state(ds, stream=s.cuda_stream)[0]
    s.synchronize()
    assert np.array_equal(got, want, equal_nan=True)
    assert_dumps_equal(dumps(ds), dumps(by_host))


def test_there_and_back(mesh):
    v, n = mesh
    ds = DeviceScene(_main_like(v, n).spec(), 0)
    d0, r0 = dumps(ds), _state(ds)[0]
    ds.update_mesh(0, _moved(v, 1.4), n)
    assert not np.array_equal(_state(ds)[0], r0)
    ds.update_mesh(0, v, n)
    assert_dumps_equal(d0, dumps(ds))
    assert np.array_equal(_state(ds)[0], r0, equal_nan=True)


def test_nan_free_toggle(mesh):
    v, n = mesh
    ds = DeviceScene(_main_like(v, n).spec(), 0)
    assert ds.info()["nan_free"]
    r0 = _state(ds)[0]
    zero = np.zeros_like(n)
    ds.update_mesh(0, v, zero)  # mesh.rs:37: an OBJ without normals
    assert not ds.info()["nan_free"]
    fresh = DeviceScene(_main_like(v, zero).spec(), 0)
    assert not fresh.info()["nan_free"]
    got = _state(ds)[0]
    assert np.array_equal(got, _state(fresh)[0], equal_nan=True)
    assert np.isnan(got).any()  # the reference's 0 * NaN reaches the pixel: nothing stopped early
    ds.update_mesh(0, v, n)
    assert ds.info()["nan_free"]
    assert np.array_equal(_state(ds)[0], r0)


def test_failed_update_changes_nothing(mesh):
    v, n = mesh
    ds = DeviceScene(_main_like(v, n).spec(), 0)
    r0, d0, i0 = _state(ds)[0], dumps(ds), ds.info()
    bad = _moved(v, 0.7)
    bad[1234, 1, 2] = np.nan
    with pytest.raises(N.VrError) as e:
        ds.update_mesh(0, bad, n)
    assert e.value.code == -7
    i1 = ds.info()
    assert {k: i0[k] for k in i0 if k != "device_bytes"} == {k: i1[k] for k in i1 if k != "device_bytes"}
    assert_dumps_equal(d0, dumps(ds))
    assert np.array_equal(_state(ds)[0], r0)
