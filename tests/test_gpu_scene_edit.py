"""The scene edits (VR_HAS_SCENE_EDIT) on the device: camera, primitives, materials and lights of a
resident scene, and vr_scene_transform_mesh (vanrijn_amd/csrc/vr_refit.hip: transform-validate and
transform-write over the mesh's resident base records, then the refit of vr_scene_update_mesh).

Bar: the device transform stores what the host form stores (tests/test_scene_edit_host.py pins that one
against the numpy restatement), and an edited scene answers every entry point bit for bit like a scene
created from the edited description.
"""
import copy

import numpy as np
import pytest

import magnitude_scenes as M
from scene_edit_checks import IDENTITY, MATRICES, OVERFLOW, SINGULAR, edited_spec, rotation_about, rows_equal, transformed
from scene_update_checks import assert_dumps_equal, check_refit, dumps
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import Tile, integrate_rays, query_closest, render_samples, render_tile_device
from vanrijn_amd.scene import (BoundingVolumeHierarchy, ColourRgbF, DeviceScene, DirectionalLight, LambertianMaterial,
                               MaterialSpec, Mesh, MeshSpec, NamedColour, Plane, PrimitiveSpec, Scene, Sphere, Spectrum,
                               WhittedIntegrator)

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


def _info(ds):
    return {k: v for k, v in ds.info().items() if k != "device_bytes"}


# ------------------------------------------------------------------ the transform itself
@pytest.mark.parametrize("reference_bvh", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 1000, 4097])
def test_device_transform_equals_host_transform(n, reference_bvh):
    """A device scene and a host-only scene of one Scene share the host-built topology: after the same
    transforms their four dumps are equal (1: the root is a leaf; 4097: many workgroups and levels)."""
    a = np.random.default_rng(n).normal(size=(n, 3, 3))
    spec = _random_scene(a).spec()
    dev = DeviceScene(spec, 0, reference_bvh=reference_bvh)
    host = DeviceScene(spec, 0, host_only=True, reference_bvh=reference_bvh)
    bytes_created = dev.info()["device_bytes"]
    for i, name in enumerate(("rotation", "scale")):
        dev.transform_mesh(0, MATRICES[name])
        host.transform_mesh(0, MATRICES[name])
        assert_dumps_equal(dumps(dev), dumps(host))
        assert _info(dev) == _info(host)
        if i == 0:
            bytes_first = dev.info()["device_bytes"]
            assert bytes_first >= bytes_created + 160 * n  # the base (and the plan) are resident and counted
    assert dev.info()["device_bytes"] == bytes_first       # the second transform allocates nothing
    w, wn = transformed(MATRICES["scale"], a, _normals(a))
    assert np.array_equal(np.sort(dumps(dev)["verts"]["v"].reshape(-1)), np.sort(w.reshape(-1)))


@pytest.mark.parametrize("flags", ["device_bvh", "device_sah"])
@pytest.mark.parametrize("n", [2, 17, 1000])
def test_device_built_topologies(n, flags):
    a = np.random.default_rng(n).normal(size=(n, 3, 3))
    ds = DeviceScene(_random_scene(a).spec(), 0, **FLAG_SETS[flags])
    before = check_refit(ds, [(a, _normals(a))])
    for name in ("rotation", "reflection"):
        ds.transform_mesh(0, MATRICES[name])
        check_refit(ds, [transformed(MATRICES[name], a, _normals(a))], before)


@pytest.mark.parametrize("flags", ["device_bvh", "device_sah"])
@pytest.mark.parametrize("regime", M.REFIT_REGIMES, ids=M.regime_id)
def test_transform_into_each_magnitude_and_back(regime, flags):
    """The transform kernels and the refit they start, where the bounds are beyond what f32 resolves,
    in its denormal range, all 0 or the smallest denormal, or beyond FLT_MAX (tests/magnitude_scenes.py):
    a translation by T and a uniform scale by S carry a unit mesh from the control into the regime, and
    the identity carries it back; extent and nan_free are a fresh scene's."""
    a = np.random.default_rng(257).normal(size=(257, 3, 3))
    ds = DeviceScene(_random_scene(a).spec(), 0, **FLAG_SETS[flags])
    before = check_refit(ds, [(a, _normals(a))])
    home = {key: ds.info()[key] for key in ("extent", "nan_free")}
    m = M.map_matrix(*regime)
    w, wn = transformed(m, a, _normals(a))
    assert np.array_equal(w, M.mapped(a, *regime))
    ds.transform_mesh(0, m)
    check_refit(ds, [(w, wn)], before)
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    fresh = DeviceScene(Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(w, wn, mat))]).spec(), 0,
                        **FLAG_SETS[flags])
    check_refit(fresh, [(w, wn)])
    for key in ("extent", "nan_free"):
        assert ds.info()[key] == fresh.info()[key], key
    ds.transform_mesh(0, IDENTITY)
    check_refit(ds, [transformed(IDENTITY, a, _normals(a))], before)
    assert {key: ds.info()[key] for key in home} == home


@pytest.mark.parametrize("flags", ["default", "device_bvh", "device_sah"])
def test_mesh_that_backs_no_object(flags):
    a = np.random.default_rng(17).normal(size=(17, 3, 3))
    c = np.random.default_rng(5).normal(size=(5, 3, 3))
    spec = copy.copy(_random_scene(a).spec())
    spec.meshes = spec.meshes + [MeshSpec(c, _normals(c), 0)]
    ds = DeviceScene(spec, 0, **FLAG_SETS[flags])
    before = check_refit(ds, [(a, _normals(a)), (c, _normals(c))])
    assert len(before["roots"]) == 1
    m = [30.0 * x for x in MATRICES["rotation"]]
    w, wn = transformed(m, c, _normals(c))
    ds.transform_mesh(1, m)
    check_refit(ds, [(a, _normals(a)), (w, wn)], before)
    assert ds.info()["extent"] == np.abs(w).max()
    ds.transform_mesh(0, MATRICES["scale"])
    check_refit(ds, [transformed(MATRICES["scale"], a, _normals(a)), (w, wn)], before)


# ------------------------------------------------------------------ the same results as a fresh scene
CAMERA = scenes.CAMERA_LOCATION
W, H, SPP, SEED = 48, 40, 3, 0x5EED0001
CENTRE = (-1.7, -0.8, 0.0)
NEW_CAMERA = (-2.5, 1.25, -5.5)
NEW_PLANE = PrimitiveSpec(N.PRIMITIVE_PLANE, 0, (0.05, 1.0, 0.02), -1.9)
NEW_SPHERE = PrimitiveSpec(N.PRIMITIVE_SPHERE, 2, (-3.6, 0.2, 1.5), 0.8)
TURN = rotation_about(0.6, CENTRE, (0.4, 0.1, -0.2))


def _cyan():
    return MaterialSpec(N.MATERIAL_LAMBERTIAN, Spectrum.reflection_from_linear_rgb(ColourRgbF.from_named(NamedColour.Cyan)),
                        0.08)


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


def _by_input_triangle(ds, a):
    """A mesh hit's `primitive` is its leaf position in the reference tree, which an edited scene keeps
    from its creation where a fresh scene re-ranks (the caveat of vr_scene_update_mesh): compare the
    input triangle it stands for, vr_scene_bvh_leaf_order[primitive].  The mesh is object 1, mesh 0."""
    a = a.copy()
    on_mesh = (a["valid"] != 0) & (a["object"] == 1)
    a["primitive"][on_mesh] = ds.leaf_order(0)[a["primitive"][on_mesh]].astype(np.int64)
    return a


def _answers(ds):
    o, d = _rays()
    hits, rec = query_closest(ds, o, d, records=True)
    hits, rec = _by_input_triangle(ds, hits), _by_input_triangle(ds, rec)
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
    v, n = scenes.displaced_mesh(16, scenes._BUNNY_BUMPS, noise_seed=0xB0BB1E, noise_count=48, noise_amp=0.04,
                                 scale=(1.25, 1.05, 1.15), centre=CENTRE)
    assert len(v) == 3072
    return v, n


def _assert_records_like(ds, fresh):
    assert rows_equal(ds.primitives(), fresh.primitives())
    assert rows_equal(ds.materials(), fresh.materials())
    assert ds.camera().tobytes() == fresh.camera().tobytes()
    for key in ("extent", "nan_free"):
        assert ds.info()[key] == fresh.info()[key]


@pytest.mark.parametrize("flags", list(FLAG_SETS))
def test_edited_scene_answers_like_a_fresh_one(flags, mesh):
    v, n = mesh
    spec = _main_like(v, n).spec()
    ds = DeviceScene(spec, 0, **FLAG_SETS[flags])
    old = _answers(ds)
    bytes_created = ds.info()["device_bytes"]
    ds.set_camera(NEW_CAMERA)
    ds.update_primitives(0, [NEW_PLANE])
    ds.update_primitives(2, [NEW_SPHERE])
    ds.update_material(3, _cyan())
    assert ds.info()["device_bytes"] == bytes_created  # the scene block's allocation stays
    ds.transform_mesh(0, TURN)
    new = _answers(ds)
    fresh = DeviceScene(edited_spec(spec, camera=NEW_CAMERA, primitives={(0, 0): NEW_PLANE, (0, 2): NEW_SPHERE},
                                    materials={3: _cyan()}, meshes={0: transformed(TURN, v, n)}), 0, **FLAG_SETS[flags])
    _assert_answers_equal(new, _answers(fresh))
    _assert_records_like(ds, fresh)
    for key in ("samples", "state", "photons"):
        x, y = old[key], new[key]
        assert x.tobytes() != y.tobytes(), key
    assert (new["hits"]["valid"] != 0).sum() > 1000 and not np.array_equal(old["hits"]["distance"], new["hits"]["distance"])


@pytest.mark.parametrize("edit", ["camera", "primitives", "material", "glass", "transform"])
def test_each_edit_alone_against_a_fresh_scene(edit, mesh):
    v, n = mesh
    spec = _main_like(v, n).spec()
    ds = DeviceScene(spec, 0)
    r0 = _state(ds)[0]
    if edit == "camera":
        ds.set_camera(NEW_CAMERA)
        want = edited_spec(spec, camera=NEW_CAMERA)
    elif edit == "primitives":
        ds.update_primitives(0, [NEW_PLANE, spec.objects[0].primitives[1], NEW_SPHERE])
        want = edited_spec(spec, primitives={(0, 0): NEW_PLANE, (0, 2): NEW_SPHERE})
    elif edit == "material":
        ds.update_material(3, _cyan())
        want = edited_spec(spec, materials={3: _cyan()})
    elif edit == "glass":  # a sphere becomes a dielectric: NAN_FREE, the early stop and dark0 go, as on a fresh scene
        glass = MaterialSpec(N.MATERIAL_DIELECTRIC, Spectrum.grey(1.5), 0.0)
        ds.update_material(2, glass)
        want = edited_spec(spec, materials={2: glass})
        assert not ds.info()["nan_free"]
    else:
        ds.transform_mesh(0, np.array(TURN).reshape(3, 4))
        want = edited_spec(spec, meshes={0: transformed(TURN, v, n)})
    fresh = DeviceScene(want, 0)
    (a, sa), (b, sb) = _state(ds), _state(fresh)
    assert np.array_equal(a, b, equal_nan=True) and not np.array_equal(a, r0)
    assert sa["variant"] == sb["variant"]
    _assert_records_like(ds, fresh)


def test_material_edit_switches_the_kernel_variant(mesh):
    """enqueue_passes reads mats and dark0 per call: a mesh that becomes reflective takes the
    cooperative-tail kernels, and a colour that is not 0 at 0 nm (dark0 off) leaves them again."""
    v, n = mesh
    yellow = Spectrum.reflection_from_linear_rgb(ColourRgbF.from_named(NamedColour.Yellow))
    ds = DeviceScene(Scene(CAMERA, [BoundingVolumeHierarchy.build(Mesh(v, n, LambertianMaterial(yellow, 0.05)))]).spec(), 0)
    r0, s0 = _state(ds, 64, 64, 2)
    assert not s0["variant"] & N.VARIANT_COOP
    ds.update_material(0, MaterialSpec(N.MATERIAL_REFLECTIVE, yellow, 0.05, 0.9))
    fresh = DeviceScene(scenes.bench_scene((v, n)).spec(), 0)
    (a, sa), (b, sb) = _state(ds, 64, 64, 2), _state(fresh, 64, 64, 2)
    assert sa["variant"] == sb["variant"] == N.VARIANT_COOP
    assert np.array_equal(a, b, equal_nan=True) and not np.array_equal(a, r0) and np.count_nonzero(a) > 1000
    lit = MaterialSpec(N.MATERIAL_REFLECTIVE, Spectrum(0.0, 740.0, np.array([0.25, 0.5, 0.75])), 0.05, 0.9)
    ds.update_material(0, lit)
    fresh = DeviceScene(edited_spec(scenes.bench_scene((v, n)).spec(), materials={0: lit}), 0)
    (a, sa), (b, sb) = _state(ds, 64, 64, 2), _state(fresh, 64, 64, 2)
    assert sa["variant"] == sb["variant"] and not sa["variant"] & N.VARIANT_COOP
    assert np.array_equal(a, b, equal_nan=True)


def test_block_cull_after_a_camera_move(mesh):
    v, n = mesh
    spec = _main_like(v, n).spec()
    cam = (1.5, 2.0, -6.0)
    ds = DeviceScene(spec, 0)
    r0 = _state(ds)[0]
    ds.set_camera(cam)
    culled = _state(ds)[0]
    traced = _state(ds, cull=False)[0]
    fresh = _state(DeviceScene(edited_spec(spec, camera=cam), 0))[0]
    assert np.array_equal(culled, traced, equal_nan=True) and np.array_equal(culled, fresh, equal_nan=True)
    assert not np.array_equal(culled, r0)


def test_edited_scene_tile_against_the_oracle(mesh, oracle):
    """As tests/test_gpu_scene_update.py does for an updated scene: decisions identical, intensities to 1e-12."""
    v, n = mesh
    spec = _main_like(v, n).spec()
    ds = DeviceScene(spec, 0)
    ds.set_camera(NEW_CAMERA)
    ds.update_primitives(2, [NEW_SPHERE])
    ds.transform_mesh(0, TURN)
    want = edited_spec(spec, camera=NEW_CAMERA, primitives={(0, 2): NEW_SPHERE}, meshes={0: transformed(TURN, v, n)})
    t = Tile(8, 40, 6, 34)
    gpu = render_samples(ds, t, H, W, 4, seed=SEED)
    ref = oracle.OracleScene(want).render_samples(t, H, W, 4, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert np.array_equal(gpu["flags"], ref["flags"])
    assert np.array_equal(gpu["bounces"], ref["bounces"])
    assert np.array_equal(gpu["wavelength"], ref["wavelength"])
    nz = ref["intensity"] != 0
    assert (np.abs(gpu["intensity"] - ref["intensity"])[nz] / np.abs(ref["intensity"])[nz] < 1e-12).all()
    assert np.array_equal(gpu["intensity"] == 0, ref["intensity"] == 0)
    assert (ref["flags"] & 1).sum() > 100


def test_whitted_lights(mesh):
    spec = scenes.whitted_scene(mesh).spec()
    ds = DeviceScene(spec, 0)
    r0 = _state(ds)[0]
    new = WhittedIntegrator(Spectrum.grey(0.02),
                            [DirectionalLight((-0.7, 0.6, -0.4), Spectrum.reflection_from_linear_rgb(ColourRgbF.new(0.9, 0.5, 0.3))),
                             spec.integrator.lights[1]])
    ds.set_lights(new)
    fresh = DeviceScene(edited_spec(spec, integrator=new), 0)
    a, b = _state(ds)[0], _state(fresh)[0]
    assert np.array_equal(a, b, equal_nan=True) and not np.array_equal(a, r0, equal_nan=True)
    assert rows_equal(ds.materials(), fresh.materials())
    ds.set_lights(spec.integrator)
    assert np.array_equal(_state(ds)[0], r0, equal_nan=True)


def test_stream_form(mesh):
    """Transformed on a non-default stream and rendered on it: the null-stream result."""
    import torch
    v, n = mesh
    spec = _main_like(v, n).spec()
    plain = DeviceScene(spec, 0)
    plain.transform_mesh(0, TURN)
    want = _state(plain)[0]
    ds = DeviceScene(spec, 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        ds.transform_mesh(0, TURN, s.cuda_stream)
        got = _state(ds, stream=s.cuda_stream)[0]
    s.synchronize()
    assert np.array_equal(got, want, equal_nan=True)
    assert_dumps_equal(dumps(ds), dumps(plain))


def test_there_and_back(mesh):
    v, n = mesh
    assert not np.signbit(v[v == 0]).any()  # the base has no negative zeros: the identity gives its very bits
    ds = DeviceScene(_main_like(v, n).spec(), 0)
    d0, r0 = dumps(ds), _state(ds)[0]
    ds.transform_mesh(0, TURN)
    assert not np.array_equal(_state(ds)[0], r0)
    ds.transform_mesh(0, IDENTITY)
    assert_dumps_equal(d0, dumps(ds))
    assert np.array_equal(_state(ds)[0], r0, equal_nan=True)


def test_failed_transform_changes_nothing(mesh):
    v, n = mesh
    ds = DeviceScene(_main_like(v, n).spec(), 0)
    r0, d0, i0 = _state(ds)[0], dumps(ds), _info(ds)
    prims, mats = ds.primitives(), ds.materials()
    with pytest.raises(N.VrError) as e:
        ds.transform_mesh(0, OVERFLOW)
    assert e.value.code == -7
    assert _info(ds) == i0
    assert_dumps_equal(d0, dumps(ds))
    assert rows_equal(ds.primitives(), prims) and rows_equal(ds.materials(), mats)
    assert np.array_equal(_state(ds)[0], r0)
    ds.transform_mesh(0, TURN)  # from the same base
    twin = DeviceScene(_main_like(v, n).spec(), 0)
    twin.update_mesh(0, *transformed(TURN, v, n))
    assert_dumps_equal(dumps(ds), dumps(twin))


def test_singular_matrix(mesh):
    v, n = mesh
    spec = _main_like(v, n).spec()
    ds, twin = DeviceScene(spec, 0), DeviceScene(spec, 0)
    assert ds.info()["nan_free"]
    ds.transform_mesh(0, SINGULAR)
    twin.update_mesh(0, *transformed(SINGULAR, v, n))
    assert not ds.info()["nan_free"]
    assert_dumps_equal(dumps(ds), dumps(twin))
    assert _info(ds) == _info(twin)
    assert np.array_equal(_state(ds)[0], _state(twin)[0], equal_nan=True)
