"""Per-triangle materials (VR_HAS_MESH_MATERIALS) through the C ABI on the GPU.

1. Same tree: a mesh whose triangles all name material k through the table -- or, at random, k and a
   byte-identical copy j of it -- answers bit for bit as the scene created with the mesh's material set
   to k: the table changes which row a hit reads and nothing else.  An icosphere (shared edges, exact
   ties), every material kind, both integrators, the launch flags that pick other instantiations.
2. Different materials: a soup of disjoint triangles with four materials at random, one mesh, against
   the oracle's run of the same triangles split into four meshes (a scene it can express), and against
   that split scene on the device bit for bit.  No sample is left out: the hit rule depends only on each
   triangle's own box (a line that passes a leaf box passes every box containing it), and disjoint
   triangles in general position give no equal distances for the object / leaf order to break.
3. The assignment changes the render (fails without the feature), 4. the device form, 5. persistence
   through update_mesh_device and transform_mesh.

Images are 16 x 16 at 4 spp with fixed seeds.
"""
import numpy as np
import pytest
import torch

from scene_edit_checks import MATRICES, transformed
from scene_update_checks import dumps
from test_gpu_integrate import _bits, _matches_oracle
from vanrijn_amd import _native as N
from vanrijn_amd.render import Tile, integrate_rays, render_samples, render_tile_device
from vanrijn_amd.scene import (BoundingVolumeHierarchy, ColourRgbF, DeviceScene, DirectionalLight, LambertianMaterial,
                               Mesh, MeshSpec, ObjectSpec, PhongMaterial, Plane, ReflectiveMaterial, Scene, SceneSpec,
                               SmoothTransparentDialectric, Spectrum, WhittedIntegrator)

pytestmark = pytest.mark.gpu

H = W = 16
SPP = 4
TILE = Tile(0, W, 0, H)
SEED = 0x5EED0C01
INVALID = -1
FIELDS = ("flags", "bounces", "wavelength", "intensity")


def _whitted():
    warm = Spectrum.reflection_from_linear_rgb(ColourRgbF.new(1.0, 0.9, 0.7))
    cool = Spectrum.reflection_from_linear_rgb(ColourRgbF.new(0.3, 0.4, 0.8))
    return WhittedIntegrator(Spectrum.grey(0.05), [DirectionalLight((0.4, 1.0, -0.3), warm),
                                                   DirectionalLight((-0.6, 0.8, 0.2), cool)])


def _kind(name):
    green = Spectrum.reflection_from_linear_rgb(ColourRgbF.new(0.2, 0.9, 0.4))
    return {"lambertian": lambda: LambertianMaterial(green, 0.8),
            "reflective": lambda: ReflectiveMaterial(green, 0.3, 0.7),
            "phong": lambda: PhongMaterial(green, 0.4, 0.3, 30.0),
            "dielectric": lambda: SmoothTransparentDialectric(Spectrum.grey(1.5))}[name]()


def _icosphere():
    """An icosahedron subdivided once: 80 triangles on the unit sphere, outward normals (the positions)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    p = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    tris = []
    for a, b, c in f:
        va, vb, vc = p[a], p[b], p[c]
        mid = [x / np.linalg.norm(x) for x in (va + vb, vb + vc, vc + va)]
        tris += [(va, mid[0], mid[2]), (vb, mid[1], mid[0]), (vc, mid[2], mid[1]), (mid[0], mid[1], mid[2])]
    v = np.array(tris)
    assert v.shape == (80, 3, 3)
    return np.ascontiguousarray(v * 1.1), np.ascontiguousarray(v)


def _soup(n, seed):
    """n triangles, each inside its own cell of a grid (no two touch), vertex normals on the face
    normal's side."""
    g = np.random.default_rng(seed)
    cells = np.array([(x, y, z) for x in range(8) for y in range(7) for z in range(5)], dtype=np.float64)
    assert len(cells) >= n
    centre = (cells[g.permutation(len(cells))[:n]] - np.array([3.5, 2.5, 2.0])) * 0.4
    v = centre[:, None, :] + g.uniform(-0.16, 0.16, size=(n, 3, 3))
    face = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    face /= np.linalg.norm(face, axis=1, keepdims=True)
    nn = face[:, None, :] + g.uniform(-0.2, 0.2, size=(n, 3, 3))
    return np.ascontiguousarray(v), np.ascontiguousarray(nn)


def _floor():
    return LambertianMaterial(Spectrum.grey(0.5), 0.5)


def _records_equal(a, b):
    for f in FIELDS:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        assert x.tobytes() == y.tobytes(), f


def _rays(n, seed):
    g = np.random.default_rng(seed)
    o = np.tile(np.array([0.0, 0.0, -5.0]), (n, 1))
    d = g.uniform([-1.2, -1.4, -1.0], [1.2, 1.2, 1.0], size=(n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d


RAYS = _rays(256, 11)


def _state(ds, **kw):
    st = torch.zeros(W * H * 8, dtype=torch.float64, device="cuda")
    render_tile_device(ds, TILE, H, W, SPP, SEED, 0, st.data_ptr(), **kw)
    torch.cuda.synchronize()
    return st.cpu().view(torch.int64).numpy()


def _answers(ds):
    """Everything case 1 compares: per-sample records and device state under each launch flag, and the
    photons of caller-supplied rays."""
    out = {"samples": render_samples(ds, TILE, H, W, SPP, seed=SEED)}
    for name, kw in (("default", {}), ("multi_bvh", {"one_bvh": False}), ("stack32", {"stack16": False}),
                     ("no_coop", {"coop": False}), ("no_coop_multi_bvh", {"coop": False, "one_bvh": False})):
        out["state_" + name] = _state(ds, **kw)
    ds.set_launch_flags(multi_bvh=True, stack32=True)
    out["samples_multi_bvh_stack32"] = render_samples(ds, TILE, H, W, SPP, seed=SEED)
    ds.set_launch_flags()
    ph, info = integrate_rays(ds, RAYS[0], RAYS[1], SEED, info=True)
    out["photons"], out["info"] = ph, info
    return out


def _assert_answers_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("samples"):
            _records_equal(a[k], b[k])
        else:
            assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k
    assert (a["samples"]["flags"] & 1).sum() > 100  # the camera sees the mesh
    assert np.count_nonzero(a["state_default"]) > 500


def _with_mesh(spec, material, triangle_materials=None):
    m = spec.meshes[0]
    return SceneSpec(spec.camera_location, list(spec.materials), [MeshSpec(m.vertices, m.normals, material, triangle_materials)],
                     [ObjectSpec(o.kind, list(o.primitives), o.mesh) for o in spec.objects], spec.integrator)


# ------------------------------------------------------------------ 1. same tree, bit for bit
@pytest.mark.parametrize("integrator", ["simple_random", "whitted"])
@pytest.mark.parametrize("kind", ["lambertian", "reflective", "phong", "dielectric"])
def test_same_tree_bit_for_bit(kind, integrator):
    v, nn = _icosphere()
    other = ReflectiveMaterial(Spectrum.grey(0.9), 0.2, 0.8)  # the mesh's own: never the answer below
    k, j = _kind(kind), _kind(kind)  # two rows with the same bytes
    ids = np.random.default_rng(3).integers(0, 2, size=len(v)).astype(np.uint32)
    scene = Scene((0.0, 0.0, -5.0), [[Plane((0.0, 1.0, 0.0), -2.0, _floor())],
                                     BoundingVolumeHierarchy.build(Mesh(v, nn, other, triangle_materials=([k, j], ids)))],
                  _whitted() if integrator == "whitted" else None)
    spec = scene.spec()
    assert len(spec.materials) == 4 and sorted(set(spec.meshes[0].triangle_materials.tolist())) == [2, 3]
    rows = DeviceScene(spec, 0, host_only=True).materials()
    assert rows[2].tobytes() == rows[3].tobytes()
    want = _answers(DeviceScene(_with_mesh(spec, 2), 0))  # the mesh's material set to k
    all_k = DeviceScene(_with_mesh(spec, 1, np.full(len(v), 2, dtype=np.uint32)), 0)
    assert all_k.mesh_materials(0).tolist() == [2] * len(v)
    _assert_answers_equal(_answers(all_k), want)
    mixed = DeviceScene(spec, 0)
    assert np.array_equal(mixed.mesh_materials(0), spec.meshes[0].triangle_materials)
    _assert_answers_equal(_answers(mixed), want)
    # and it is the table that answers: without it the mesh's own (reflective grey) material renders otherwise
    mixed.set_mesh_materials(0, None)
    plain = render_samples(mixed, TILE, H, W, SPP, seed=SEED)
    assert plain["intensity"].tobytes() != want["samples"]["intensity"].tobytes()


@pytest.mark.parametrize("case", ["wide_offsets", "one_triangle", "device_bvh"])
def test_same_tree_other_layouts(case):
    v, nn = _icosphere()
    kw = {"wide_offsets": True} if case == "wide_offsets" else ({"device_bvh": True} if case == "device_bvh" else {})
    if case == "one_triangle":  # the root is a leaf
        v = np.array([[[-1.5, -1.0, 0.5], [1.5, -1.2, 0.0], [0.2, 1.4, -0.3]]])
        nn = np.array([[[0.1, 0.2, -1.0], [-0.2, 0.1, -1.0], [0.0, -0.1, -1.0]]])
    other, k = ReflectiveMaterial(Spectrum.grey(0.9), 0.2, 0.8), _kind("lambertian")
    ids = np.zeros(len(v), dtype=np.uint32)
    spec = Scene((0.0, 0.0, -5.0), [[Plane((0.0, 1.0, 0.0), -2.0, _floor())],
                                    BoundingVolumeHierarchy.build(Mesh(v, nn, other, triangle_materials=([k], ids)))]).spec()
    want = _answers(DeviceScene(_with_mesh(spec, 2), 0, **kw))
    _assert_answers_equal(_answers(DeviceScene(spec, 0, **kw)), want)


# ------------------------------------------------------------------ 2. different materials, against the oracle
def _palette():
    return [LambertianMaterial(Spectrum.grey(0.9), 0.8), LambertianMaterial(Spectrum.grey(0.05), 0.3),
            ReflectiveMaterial(Spectrum.reflection_from_linear_rgb(ColourRgbF.new(0.9, 0.2, 0.2)), 0.3, 0.7),
            SmoothTransparentDialectric(Spectrum.grey(1.5))]


def _soup_scenes(n, seed, integrator=None):
    """(merged, split, ids): one mesh with per-triangle materials, and the same triangles as four meshes.
    The geometry is shading-finite, but glass in the desc clears NAN_FREE for both scenes alike (it is
    derived from all of the desc's materials); the early stop is live in test_assignment_changes_the_render,
    whose two Lambertians keep it."""
    v, nn = _soup(n, seed)
    palette = _palette()
    ids = np.random.default_rng(seed + 1).integers(0, 4, size=n).astype(np.uint32)
    assert len(set(ids.tolist())) == 4
    plane = [Plane((0.0, 1.0, 0.0), -2.0, _floor())]
    merged = Scene((0.0, 0.0, -5.0), [plane, BoundingVolumeHierarchy.build(
        Mesh(v, nn, palette[0], triangle_materials=(palette, ids)))], integrator)
    split = Scene((0.0, 0.0, -5.0), [plane] + [BoundingVolumeHierarchy.build(
        Mesh(np.ascontiguousarray(v[ids == m]), np.ascontiguousarray(nn[ids == m]), palette[m])) for m in range(4)],
        integrator)
    return merged, split, ids


@pytest.fixture(scope="module", params=["simple_random", "whitted"])
def soup_case(request, oracle):
    merged, split, ids = _soup_scenes(260, 21, _whitted() if request.param == "whitted" else None)
    assert [m.kind for m in merged.spec().materials] == [m.kind for m in split.spec().materials]
    ref = oracle.OracleScene(split.spec()).render_samples(TILE, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE,
                                                          nthreads=8)
    ref.setflags(write=False)
    assert (ref["flags"] & 1).sum() > 300 and ref["bounces"].max() >= 3
    return merged, split, ids, ref


@pytest.mark.parametrize("build", ["host", "device_bvh", "device_sah"])
def test_merged_soup_against_the_oracle_and_the_split_scene(soup_case, build):
    merged, split, ids, ref = soup_case
    kw = {} if build == "host" else {build: True}
    ds = DeviceScene(merged.spec(), 0, **kw)
    assert np.array_equal(ds.mesh_materials(0), ids + 1)  # the plane's material is row 0
    got = render_samples(ds, TILE, H, W, SPP, seed=SEED)
    _matches_oracle(got.reshape(-1), got.reshape(-1), ref.reshape(-1))  # every sample, none left out
    on_device = render_samples(DeviceScene(split.spec(), 0, **kw), TILE, H, W, SPP, seed=SEED)
    _records_equal(got, on_device)
    ph = integrate_rays(ds, RAYS[0], RAYS[1], SEED)
    ph_split = integrate_rays(DeviceScene(split.spec(), 0, **kw), RAYS[0], RAYS[1], SEED)
    assert np.array_equal(_bits(ph["wavelength"]), _bits(ph_split["wavelength"]))
    assert np.array_equal(_bits(ph["intensity"]), _bits(ph_split["intensity"]))
    assert np.array_equal(_state(ds), _state(DeviceScene(split.spec(), 0, **kw)))


# ------------------------------------------------------------------ 3. fails without the feature
def test_assignment_changes_the_render():
    v, nn = _soup(260, 21)
    bright, dark = _palette()[:2]
    ids = np.random.default_rng(5).integers(0, 2, size=len(v)).astype(np.uint32)
    plane = [Plane((0.0, 1.0, 0.0), -2.0, _floor())]
    single = Scene((0.0, 0.0, -5.0), [plane, BoundingVolumeHierarchy.build(Mesh(v, nn, bright))])
    two = Scene((0.0, 0.0, -5.0), [plane, BoundingVolumeHierarchy.build(
        Mesh(v, nn, bright, triangle_materials=([bright, dark], ids)))])
    ds = DeviceScene(two.spec(), 0)
    assert np.array_equal(ds.mesh_materials(0), ids + 1)
    a = render_samples(ds, TILE, H, W, SPP, seed=SEED)
    b = render_samples(DeviceScene(single.spec(), 0), TILE, H, W, SPP, seed=SEED)
    assert np.array_equal(a["wavelength"], b["wavelength"])  # the same camera rays
    differ = a["intensity"] != b["intensity"]
    assert differ.any()  # the records differ from the single-material render
    # both Lambertians sample the same directions, so a path differs only in the factors of the dark
    # triangles it met: it can only be darker
    assert (a["intensity"][differ] < b["intensity"][differ]).all()
    assert np.array_equal(a["bounces"], b["bounces"]) and np.array_equal(a["flags"], b["flags"])


# ------------------------------------------------------------------ 4. the device form
def _bytes(ds):
    return {k: x.tobytes() for k, x in dumps(ds).items()}


@pytest.mark.parametrize("dtype", [torch.int32, torch.uint32], ids=["int32", "uint32"])
def test_device_form_equals_the_host_form(dtype):
    merged, _, ids = _soup_scenes(257, 33)  # 257: a partial last block
    spec = _with_mesh(merged.spec(), 1)
    ids = (ids + 1).astype(np.uint32)
    host = DeviceScene(spec, 0)
    host.set_mesh_materials(0, ids)
    dev = DeviceScene(spec, 0)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(ids.astype(np.int32)).cuda().view(dtype)
    dev.set_mesh_materials_device(0, t.data_ptr(), stream.cuda_stream)
    assert _bytes(dev) == _bytes(host)
    assert np.array_equal(dev.mesh_materials(0), ids)
    _records_equal(render_samples(dev, TILE, H, W, SPP, seed=SEED), render_samples(host, TILE, H, W, SPP, seed=SEED))
    # an index out of range is found on the device before anything is written
    before, info = _bytes(dev), dev.info()
    for bad_at, bad in ((0, 5), (256, 5), (100, 0x7FFFFFFF)):
        wrong = ids.astype(np.int32)
        wrong[bad_at] = bad
        with torch.cuda.stream(stream):
            tw = torch.from_numpy(wrong).cuda()
        with pytest.raises(N.VrError) as e:
            dev.set_mesh_materials_device(0, tw.data_ptr(), stream.cuda_stream)
        assert e.value.code == INVALID
        assert _bytes(dev) == before and dev.info() == info
    with pytest.raises(N.VrError) as e:
        wrong = ids.copy()
        wrong[7] = 5
        dev.set_mesh_materials(0, wrong)
    assert e.value.code == INVALID and _bytes(dev) == before and dev.info() == info


# ------------------------------------------------------------------ 5. persistence on the device
def test_assignment_survives_device_update_and_transform():
    merged, _, ids = _soup_scenes(260, 21)
    spec = _with_mesh(merged.spec(), 1)
    ids = (ids + 1).astype(np.uint32)
    v0, n0 = spec.meshes[0].vertices, spec.meshes[0].normals
    v1 = np.ascontiguousarray(v0 * 1.05 + 0.02)
    m = MATRICES["rotation"][:3] + [0.1] + MATRICES["rotation"][4:7] + [-0.2] + MATRICES["rotation"][8:11] + [0.3]
    ds = DeviceScene(spec, 0)
    ds.set_mesh_materials(0, ids)
    tv, tn = torch.from_numpy(v1).cuda(), torch.from_numpy(n0).cuda()
    torch.cuda.synchronize()
    ds.update_mesh_device(0, tv.data_ptr(), tn.data_ptr())
    ds.transform_mesh(0, m)
    assert np.array_equal(ds.mesh_materials(0), ids)
    vf, nf = transformed(m, v1, n0)
    final = SceneSpec(spec.camera_location, spec.materials, [MeshSpec(vf, nf, 1)], spec.objects, spec.integrator)
    fresh = DeviceScene(final, 0)
    fresh.set_mesh_materials(0, ids)
    want = render_samples(fresh, TILE, H, W, SPP, seed=SEED)
    assert (want["flags"] & 1).sum() > 200
    _records_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED), want)
    # a set call after the first transform reaches the base: the next transform keeps it
    ids2 = (ids % 4 + 1).astype(np.uint32)
    ds.set_mesh_materials(0, ids2)
    ds.transform_mesh(0, m)
    assert np.array_equal(ds.mesh_materials(0), ids2)
    fresh.set_mesh_materials(0, ids2)
    _records_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED), render_samples(fresh, TILE, H, W, SPP, seed=SEED))
    # the reset equals the plain scene
    ds.set_mesh_materials(0, None)
    ds.transform_mesh(0, m)
    _records_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED),
                   render_samples(DeviceScene(final, 0), TILE, H, W, SPP, seed=SEED))
    assert not dumps(ds)["normals"]["pad"].view("<i8").any()
