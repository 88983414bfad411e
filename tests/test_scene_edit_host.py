"""The scene edits (VR_HAS_SCENE_EDIT) on VR_SCENE_HOST_ONLY scenes (no GPU): there every call changes
the host records only -- the same row builders vr_scene_create uses, and for vr_scene_transform_mesh
the per-record steps the device kernels run (vr_refit.h).

Bar: after an edit the inspectors and vr_scene_get_info equal those of a scene created from the edited
description, byte for byte; a transform equals vr_scene_update_mesh with the arrays of the numpy
restatement (tests/scene_edit_checks.py).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from scene_edit_checks import IDENTITY, MATRICES, OVERFLOW, SINGULAR, edited_spec, rows_equal, transformed
from scene_update_checks import assert_dumps_equal, check_refit, dumps
from vanrijn_amd import _native as N
from vanrijn_amd.scene import (BoundingVolumeHierarchy, DeviceScene, DirectionalLight, LambertianMaterial, MaterialSpec,
                               Mesh, Plane, PrimitiveSpec, ReflectiveMaterial, Scene, Sphere, Spectrum,
                               WhittedIntegrator)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {
    "vr_scene_set_camera": r"int vr_scene_set_camera\(vr_scene\* scene, vr_vec3 location\);",
    "vr_scene_update_primitives":
        r"int vr_scene_update_primitives\(vr_scene\* scene, uint32_t first, uint32_t count, const vr_primitive_desc\* \w+\);",
    "vr_scene_update_material":
        r"int vr_scene_update_material\(vr_scene\* scene, uint32_t index, const vr_material_desc\* material\);",
    "vr_scene_set_lights": r"int vr_scene_set_lights\(vr_scene\* scene, const vr_integrator_desc\* integrator\);",
    "vr_scene_transform_mesh":
        r"int vr_scene_transform_mesh\(vr_scene\* scene, uint32_t mesh, const double matrix\[12\], void\* stream\);",
    "vr_scene_primitives": r"int vr_scene_primitives\(const vr_scene\* scene, void\* out, uint32_t\* count\);",
    "vr_scene_materials": r"int vr_scene_materials\(const vr_scene\* scene, void\* out, uint32_t\* count\);",
    "vr_scene_get_camera": r"int vr_scene_get_camera\(const vr_scene\* scene, vr_vec3\* out\);",
}


def _normals(v):
    n = np.zeros_like(v)
    n[..., 2] = 1.0
    return n


def _random_mesh(seed, n):
    return np.random.default_rng(seed).normal(size=(n, 3, 3))


def _mesh_scene(v):
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    return Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(v, _normals(v), mat))])


def _main_like(v):
    """A plane, two spheres (three materials) and a mesh (a fourth): extent 7.5 from the first sphere."""
    grey = [LambertianMaterial(Spectrum.grey(g), 0.1) for g in (0.2, 0.4, 0.6, 0.8)]
    return Scene((-2.0, 1.0, -5.0), [
        [Plane((0.0, 1.0, 0.0), -2.0, grey[0]), Sphere((-6.25, -0.5, 1.0), 1.25, grey[1]),
         Sphere((-4.25, -0.5, 2.0), 1.0, grey[2])],
        BoundingVolumeHierarchy.build(Mesh(v, _normals(v), grey[3]))])


def _host(spec, **kw):
    return DeviceScene(spec, 0, host_only=True, **kw)


def _code(call):
    try:
        call()
    except N.VrError as e:
        return e.code
    return 0


def _snapshot(ds):
    return {"prims": ds.primitives(), "mats": ds.materials(), "camera": ds.camera(), "info": ds.info(),
            "dumps": dumps(ds)}


def _assert_unchanged(ds, snap):
    assert rows_equal(ds.primitives(), snap["prims"])
    assert rows_equal(ds.materials(), snap["mats"])
    assert ds.camera().tobytes() == snap["camera"].tobytes()
    assert ds.info() == snap["info"]
    assert_dumps_equal(dumps(ds), snap["dumps"])


def _assert_like_fresh(ds, spec, **kw):
    """The edited scene's records and scalars against a host-only scene created from `spec`."""
    fresh = _host(spec, **kw)
    assert rows_equal(ds.primitives(), fresh.primitives())
    assert rows_equal(ds.materials(), fresh.materials())
    assert ds.camera().tobytes() == fresh.camera().tobytes()
    assert ds.info()["extent"] == fresh.info()["extent"]
    assert ds.info()["nan_free"] == fresh.info()["nan_free"]
    return fresh


# ------------------------------------------------------------------ header and ABI
def test_header_define_symbols_and_abi():
    text = open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()
    assert re.search(r"^#define VR_HAS_SCENE_EDIT 1\b", text, flags=re.M)
    assert re.search(r"^#define VR_ABI_VERSION 10\b", text, flags=re.M)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    lib = N.lib()
    for name, prototype in NEW_SYMBOLS.items():
        assert re.search(prototype, flat), name
        assert hasattr(lib, name) and name in N.SIGNATURES, name
    assert lib.vr_abi_version() == 10
    assert DeviceScene.PRIM_DTYPE.itemsize == 128 and DeviceScene.MATERIAL_DTYPE.itemsize == 1080


# ------------------------------------------------------------------ argument errors
def test_argument_errors_leave_the_scene_untouched():
    v = _random_mesh(3, 17)
    spec = _main_like(v).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    L = N.lib()
    # camera
    assert L.vr_scene_set_camera(None, N.Vec3(0, 0, 0)) == -1
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            xyz = [1.0, 2.0, 3.0]
            xyz[axis] = bad
            assert _code(lambda: ds.set_camera(xyz)) == -1
    # primitives
    sphere = PrimitiveSpec(N.PRIMITIVE_SPHERE, 0, (0.0, 50.0, 0.0), 1.0)
    one = (N.PrimitiveDesc * 1)(N.PrimitiveDesc(1, 0, N.Vec3(0, 50, 0), 1.0))
    assert L.vr_scene_update_primitives(None, 0, 1, one) == -1
    assert _code(lambda: ds.update_primitives(3, [sphere])) == -1          # range past primitive_count
    assert _code(lambda: ds.update_primitives(2, [sphere, sphere])) == -1
    assert L.vr_scene_update_primitives(ds.handle, 0xFFFFFFFF, 2, one) == -1  # first + count does not wrap
    assert L.vr_scene_update_primitives(ds.handle, 0, 1, None) == -1       # null array, count > 0
    assert _code(lambda: ds.update_primitives(0, [PrimitiveSpec(2, 0, (0.0, 1.0, 0.0), 1.0)])) == -1  # unknown kind
    assert _code(lambda: ds.update_primitives(0, [PrimitiveSpec(-1, 0, (0.0, 1.0, 0.0), 1.0)])) == -1
    assert _code(lambda: ds.update_primitives(0, [PrimitiveSpec(1, 4, (0.0, 1.0, 0.0), 1.0)])) == -1  # 4 materials
    assert _code(lambda: ds.update_primitives(0, [sphere, PrimitiveSpec(1, 9, (0.0, 1.0, 0.0), 1.0)])) == -1  # the 2nd is bad
    assert L.vr_scene_update_primitives(ds.handle, 3, 0, None) == 0        # count == 0
    ds.update_primitives(1, [])
    # materials
    ok = MaterialSpec(N.MATERIAL_LAMBERTIAN, Spectrum.grey(0.9), 0.3)
    keep = np.full(65, 0.5)
    assert L.vr_scene_update_material(None, 0, None) == -1
    assert L.vr_scene_update_material(ds.handle, 0, None) == -1
    assert _code(lambda: ds.update_material(4, ok)) == -1                  # the light and sky rows are not addressable
    assert _code(lambda: ds.update_material(0, MaterialSpec(4, Spectrum.grey(0.9), 0.3))) == -1   # kind
    assert _code(lambda: ds.update_material(0, MaterialSpec(-1, Spectrum.grey(0.9), 0.3))) == -1
    assert _code(lambda: ds.update_material(0, MaterialSpec(0, Spectrum(380.0, 740.0, keep), 0.3))) == -1  # 65 samples
    assert _code(lambda: ds.update_material(0, MaterialSpec(0, Spectrum(380.0, 740.0, keep[:0]), 0.3))) == -1  # none
    null_samples = N.MaterialDesc(0, 0, N.Spectrum(380.0, 740.0, 2, None), 0.3, 0.0, 0.0)
    assert L.vr_scene_update_material(ds.handle, 0, C.byref(null_samples)) == -1
    # lights: a SimpleRandomIntegrator scene takes only None (or its own kind with no lights)
    assert L.vr_scene_set_lights(None, None) == -1
    ds.set_lights(None)
    assert _code(lambda: ds.set_lights(WhittedIntegrator(Spectrum.grey(0.1), []))) == -1
    # transform
    m = (C.c_double * 12)(*IDENTITY)
    assert L.vr_scene_transform_mesh(None, 0, m, None) == -1
    assert L.vr_scene_transform_mesh(ds.handle, 0, None, None) == -1
    assert L.vr_scene_transform_mesh(ds.handle, 1, m, None) == -1          # bad mesh index
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 7, 11):
            x = list(IDENTITY)
            x[k] = bad
            assert _code(lambda: ds.transform_mesh(0, x)) == -1
    with pytest.raises(ValueError):
        ds.transform_mesh(0, np.eye(4))
    # inspectors
    n = C.c_uint32()
    assert L.vr_scene_primitives(None, None, C.byref(n)) == -1
    assert L.vr_scene_materials(None, None, C.byref(n)) == -1
    assert L.vr_scene_primitives(ds.handle, None, None) == -1
    assert L.vr_scene_get_camera(ds.handle, None) == -1 and L.vr_scene_get_camera(None, C.byref(N.Vec3())) == -1
    assert L.vr_scene_materials(ds.handle, None, C.byref(n)) == 0 and n.value == 5  # 4 + the sky row
    _assert_unchanged(ds, snap)
    assert len(snap["prims"]) == 3 and snap["info"]["device_bytes"] == 0


def test_whitted_light_errors_leave_the_scene_untouched():
    from vanrijn_amd import scenes
    v = _random_mesh(5, 17)
    spec = scenes.whitted_scene((v, _normals(v))).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    two = spec.integrator.lights
    assert _code(lambda: ds.set_lights(None)) == -1                                       # the scene is Whitted
    assert _code(lambda: ds.set_lights(WhittedIntegrator(Spectrum.grey(0.1), two[:1]))) == -1   # light-count mismatch
    assert _code(lambda: ds.set_lights(WhittedIntegrator(Spectrum.grey(0.1), two + two[:1]))) == -1
    bad = Spectrum(380.0, 740.0, np.zeros(65))
    assert _code(lambda: ds.set_lights(WhittedIntegrator(bad, two))) == -1
    assert _code(lambda: ds.set_lights(WhittedIntegrator(Spectrum.grey(0.1), [two[0], DirectionalLight((0, 1, 0), bad)]))) == -1
    null_list = N.IntegratorDesc(N.INTEGRATOR_WHITTED, 2, N.Spectrum(380.0, 740.0, 2, (C.c_double * 2)(0.1, 0.1)), None)
    assert N.lib().vr_scene_set_lights(ds.handle, C.byref(null_list)) == -1
    wrong_kind = N.IntegratorDesc(N.INTEGRATOR_SIMPLE_RANDOM, 2, N.Spectrum(), None)
    assert N.lib().vr_scene_set_lights(ds.handle, C.byref(wrong_kind)) == -1
    _assert_unchanged(ds, snap)


# ------------------------------------------------------------------ camera, primitives, materials, lights
def test_camera_becomes_the_extent_and_stops_being_it():
    spec = _main_like(_random_mesh(7, 17)).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    assert ds.info()["extent"] == 7.5
    for cam, extent in (((0.0, -40.0, 3.0), 40.0), ((1.0, 2.0, -7.0), 7.5), ((0.0, 0.0, 9.0), 9.0)):
        ds.set_camera(cam)
        assert np.array_equal(ds.camera(), cam) and ds.info()["extent"] == extent
        _assert_like_fresh(ds, edited_spec(spec, camera=cam))
        assert_dumps_equal(dumps(ds), snap["dumps"])
    ds.set_camera(spec.camera_location)
    _assert_unchanged(ds, snap)


def test_sphere_grows_the_extent_and_shrinks_it():
    spec = _main_like(_random_mesh(8, 17)).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    big = PrimitiveSpec(N.PRIMITIVE_SPHERE, 2, (1.0, -30.0, 2.0), 4.5)
    ds.update_primitives(2, [big])
    assert ds.info()["extent"] == 34.5
    _assert_like_fresh(ds, edited_spec(spec, primitives={(0, 2): big}))
    small = Sphere((0.5, 0.25, -0.125), 0.5, 1)  # a Sphere with a material index; the other sphere's 7.5 is the extent again
    ds.update_primitives(2, [small])
    assert ds.info()["extent"] == 7.5
    _assert_like_fresh(ds, edited_spec(spec, primitives={(0, 2): PrimitiveSpec(1, 1, (0.5, 0.25, -0.125), 0.5)}))
    tiny = [Sphere((0.0, 0.0, 0.0), 0.5, 0), Sphere((1.0, 0.0, 0.0), 0.25, 0)]  # both spheres: the camera's 5 is left
    ds.update_primitives(1, tiny)
    assert ds.info()["extent"] == 5.0
    ds.update_primitives(1, spec.objects[0].primitives[1:])
    _assert_unchanged(ds, snap)


def test_plane_turned_into_a_sphere_and_back():
    spec = _main_like(_random_mesh(9, 17)).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    sphere = PrimitiveSpec(N.PRIMITIVE_SPHERE, 3, (0.3, -11.0, 0.7), 2.0)
    ds.update_primitives(0, [sphere])
    row = ds.primitives()[0]
    assert row["kind"] == 1 and row["material"] == 3 and row["object"] == 0 and row["position"] == 0
    assert np.array_equal(row["tan"], [0, 0, 0]) and row["scalar2"] == 4.0 and ds.info()["extent"] == 13.0
    _assert_like_fresh(ds, edited_spec(spec, primitives={(0, 0): sphere}))
    plane = Plane((1.0, 2.0, -2.0), -20.0, 1)  # normalised as Plane::new does; its distance is the extent
    ds.update_primitives(0, [plane])
    row = ds.primitives()[0]
    assert row["kind"] == 0 and row["scalar2"] == 0.0 and abs(np.linalg.norm(row["vec"]) - 1.0) < 1e-15
    assert ds.info()["extent"] == 20.0
    _assert_like_fresh(ds, edited_spec(spec, primitives={(0, 0): PrimitiveSpec(0, 1, (1.0, 2.0, -2.0), -20.0)}))
    ds.update_primitives(0, spec.objects[0].primitives[:1])
    _assert_unchanged(ds, snap)


class _RawScene(DeviceScene):
    """A host-only scene from primitive lists given as (first, count) ranges over one primitive array,
    which SceneSpec cannot express: lists that overlap, entries that no list refers to."""

    def __init__(self, prims, lists):
        L = N.lib()
        s = np.array([0.5, 0.5])
        mats = (N.MaterialDesc * 2)(*[N.MaterialDesc(0, 0, N.Spectrum(380.0, 740.0, 2, s.ctypes.data_as(C.POINTER(C.c_double))),
                                                     0.1 * (i + 1), 0.0, 0.0) for i in range(2)])
        parr = (N.PrimitiveDesc * len(prims))(*[N.PrimitiveDesc(p.kind, p.material, N.Vec3(*p.vector), p.scalar)
                                                for p in prims])
        objs = (N.ObjectDesc * len(lists))(*[N.ObjectDesc(N.OBJECT_PRIMITIVE_LIST, f, c, 0) for f, c in lists])
        desc = N.SceneDesc(N.Vec3(0.0, 0.0, -5.0), 2, len(prims), 0, len(lists), mats, parr, None, objs, None)
        h = C.c_void_p()
        N.check(L.vr_scene_create(C.byref(desc), 0, N.SCENE_HOST_ONLY, C.byref(h)))
        self.handle, self.device, self.host_only, self.spec, self._destroy = h, 0, True, None, L.vr_scene_destroy


def test_entries_in_two_overlapping_lists_and_in_none():
    prims = [PrimitiveSpec(1, 0, (float(i), 0.0, 0.0), 0.5) for i in range(5)]
    lists = [(0, 3), (1, 2)]  # entries 1 and 2 are in both lists, 3 and 4 in none
    ds = _RawScene(prims, lists)
    rows = ds.primitives()
    assert [(int(r["object"]), int(r["position"])) for r in rows] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    assert ds.info()["extent"] == 5.0  # the camera; entries 3 and 4 (x = 3, 4) do not count
    new = list(prims)
    new[2] = PrimitiveSpec(0, 1, (0.0, 3.0, 4.0), -9.0)   # both of its rows become this plane
    new[3] = PrimitiveSpec(1, 1, (100.0, 0.0, 0.0), 1.0)  # no row: nothing to see, and no extent
    ds.update_primitives(2, new[2:4])
    rows = ds.primitives()
    assert [int(k) for k in rows["kind"]] == [1, 1, 0, 1, 0] and [int(k) for k in rows["material"]] == [0, 0, 1, 0, 1]
    assert [(int(r["object"]), int(r["position"])) for r in rows] == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
    fresh = _RawScene(new, lists)
    assert rows_equal(rows, fresh.primitives()) and ds.info() == fresh.info() and ds.info()["extent"] == 9.0
    ds.update_primitives(4, [PrimitiveSpec(1, 0, (0.0, 0.0, 77.0), 1.0)])  # only an entry without rows
    assert rows_equal(ds.primitives(), fresh.primitives()) and ds.info() == fresh.info()
    assert _code(lambda: ds.update_primitives(4, [prims[0], prims[0]])) == -1
    ds.update_primitives(0, prims)
    assert rows_equal(ds.primitives(), _RawScene(prims, lists).primitives()) and ds.info()["extent"] == 5.0


def test_material_kinds_toggle_nan_free():
    spec = _main_like(_random_mesh(10, 17)).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    assert ds.info()["nan_free"]
    for kind in (N.MATERIAL_DIELECTRIC, N.MATERIAL_PHONG):
        glass = MaterialSpec(kind, Spectrum.grey(1.5), 0.2, 0.3, 40.0)
        ds.update_material(1, glass)
        assert not ds.info()["nan_free"]
        row = ds.materials()[1]
        assert row["kind"] == kind and row["reflection"] == 0.3 and row["smoothness"] == 40.0
        _assert_like_fresh(ds, edited_spec(spec, materials={1: glass}))
        ds.update_material(1, spec.materials[1])
        assert ds.info()["nan_free"]
        _assert_unchanged(ds, snap)
    mirror = MaterialSpec(N.MATERIAL_REFLECTIVE, Spectrum(400.0, 700.0, np.linspace(0.1, 0.9, 33)), 0.05, 0.9)
    ds.update_material(3, mirror)  # the mesh's material
    assert ds.info()["nan_free"]
    row = ds.materials()[3]
    assert row["n"] == 33 and row["inv_step"] == 32.0 / 300.0 and row["knots"][32] == 700.0 and row["knots"][33] == 0.0
    _assert_like_fresh(ds, edited_spec(spec, materials={3: mirror}))


def test_colour_that_is_not_dark_at_zero():
    """dark0 has no public view: the row is what a fresh scene's is (the render variant: on the GPU)."""
    spec = _main_like(_random_mesh(11, 17)).spec()
    ds = _host(spec)
    lit = MaterialSpec(N.MATERIAL_LAMBERTIAN, Spectrum(0.0, 740.0, np.array([0.25, 0.5, 0.75])), 0.1)
    assert lit.colour.intensity_at_wavelength(0.0) == 0.25
    ds.update_material(0, lit)
    row = ds.materials()[0]
    assert row["shortest"] == 0.0 and np.array_equal(row["samples"][:4], [0.25, 0.5, 0.75, 0.0])
    assert np.array_equal(row["knots"][:3], [0.0, 370.0, 740.0])
    _assert_like_fresh(ds, edited_spec(spec, materials={0: lit}))


def test_whitted_lights_replaced():
    from vanrijn_amd import scenes
    v = _random_mesh(12, 17)
    spec = scenes.whitted_scene((v, _normals(v))).spec()
    ds = _host(spec)
    snap = _snapshot(ds)
    assert len(snap["mats"]) == 5 + 3 + 1  # the desc's, ambient + two lights, the sky
    new = WhittedIntegrator(Spectrum(390.0, 730.0, np.array([0.01, 0.02, 0.03])),
                            [DirectionalLight((0.0, 2.0, 0.0), Spectrum.grey(0.7)),  # stored as given: not normalised
                             DirectionalLight((-1.0, 0.5, 0.25), Spectrum(380.0, 740.0, np.linspace(0.0, 1.0, 64)))])
    ds.set_lights(new)
    mats = ds.materials()
    assert rows_equal(mats[:5], snap["mats"][:5]) and rows_equal(mats[8:], snap["mats"][8:])
    assert mats[5]["n"] == 3 and mats[6]["samples"][0] == 0.7 and mats[7]["n"] == 64
    _assert_like_fresh(ds, edited_spec(spec, integrator=new))
    ds.set_lights(spec.integrator)
    _assert_unchanged(ds, snap)


# ------------------------------------------------------------------ the transform
@pytest.mark.parametrize("reference_bvh", [False, True])
@pytest.mark.parametrize("matrix", list(MATRICES))
@pytest.mark.parametrize("n", [1, 2, 3, 17, 1000])
def test_transform_equals_update_with_the_restated_arrays(n, matrix, reference_bvh):
    a = _random_mesh(n, n)
    spec = _mesh_scene(a).spec()
    ds, twin = _host(spec, reference_bvh=reference_bvh), _host(spec, reference_bvh=reference_bvh)
    before = dumps(ds)
    w, wn = transformed(MATRICES[matrix], a, _normals(a))
    ds.transform_mesh(0, np.array(MATRICES[matrix]).reshape(3, 4))
    twin.update_mesh(0, w, wn)
    assert_dumps_equal(dumps(ds), dumps(twin))
    assert ds.info() == twin.info()
    check_refit(ds, [(w, wn)], before)
    if matrix == "zero":
        assert ds.info()["extent"] == 5.0 and not ds.info()["nan_free"]  # the camera; every triangle is a point
    else:
        assert ds.info()["extent"] == max(5.0, np.abs(w).max())


def test_reflection_keeps_normals_on_their_side():
    """(A a) x (A b) = K (a x b): geometric normals as vertex normals stay exactly that under any A."""
    a = _random_mesh(41, 17)
    f = np.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0])
    good = np.repeat(f[:, None, :], 3, axis=1)
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    ds = _host(Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(a, good, mat))]).spec())
    assert ds.info()["nan_free"]
    for name in ("reflection", "scale", "rotation"):
        ds.transform_mesh(0, MATRICES[name])
        assert ds.info()["nan_free"], name
    ds.transform_mesh(0, SINGULAR)
    assert not ds.info()["nan_free"]
    ds.transform_mesh(0, IDENTITY)
    assert ds.info()["nan_free"]


def _twin_after(spec, geometry, **kw):
    t = _host(spec, **kw)
    t.update_mesh(0, *geometry)
    return t


def test_the_base_follows():
    a, b = _random_mesh(51, 17), 2.0 * _random_mesh(52, 17) + 0.25
    na, nb = _normals(a), _normals(b)
    spec = _mesh_scene(a).spec()
    m1, m2 = MATRICES["rotation"], MATRICES["scale"]

    def same(ds, geometry):
        twin = _twin_after(spec, geometry)
        assert_dumps_equal(dumps(ds), dumps(twin))
        assert ds.info() == twin.info()

    ds = _host(spec)  # transforms do not compound
    ds.transform_mesh(0, m1)
    ds.transform_mesh(0, m2)
    same(ds, transformed(m2, a, na))
    ds = _host(spec)  # an update before the first transform is the base
    ds.update_mesh(0, b, nb)
    ds.transform_mesh(0, m1)
    same(ds, transformed(m1, b, nb))
    ds = _host(spec)  # an update between two transforms replaces the base
    ds.transform_mesh(0, m1)
    ds.update_mesh(0, b, nb)
    same(ds, (b, nb))
    ds.transform_mesh(0, m2)
    same(ds, transformed(m2, b, nb))
    ds.transform_mesh(0, m1)
    same(ds, transformed(m1, b, nb))
    bad = b.copy()  # a failed update leaves the base as well
    bad[3, 1, 1] = np.nan
    assert _code(lambda: ds.update_mesh(0, bad, nb)) == -7
    ds.transform_mesh(0, m2)
    same(ds, transformed(m2, b, nb))


def test_failed_transform_changes_nothing():
    a = _random_mesh(61, 17)
    a[5, 1, 0] = 5.0  # 5e308 overflows
    spec = _mesh_scene(a).spec()
    for first in (False, True):  # as the mesh's first transform, and after one
        ds = _host(spec)
        if not first:
            ds.transform_mesh(0, MATRICES["rotation"])
        snap = _snapshot(ds)
        assert _code(lambda: ds.transform_mesh(0, OVERFLOW)) == -7
        _assert_unchanged(ds, snap)
        ds.transform_mesh(0, MATRICES["scale"])  # still from the same base
        twin = _twin_after(spec, transformed(MATRICES["scale"], a, _normals(a)))
        assert_dumps_equal(dumps(ds), dumps(twin))
        assert ds.info() == twin.info()


def test_identity_restores_the_base_without_negative_zeros():
    a = _random_mesh(71, 17)
    a[2, 0, 1] = -0.0
    ds = _host(_mesh_scene(a).spec())
    before = dumps(ds)
    ds.transform_mesh(0, MATRICES["rotation"])
    ds.transform_mesh(0, IDENTITY)
    after = dumps(ds)
    assert_dumps_equal(before, after)  # by value
    assert np.signbit(before["verts"]["v"]).sum() > np.signbit(after["verts"]["v"]).sum()
    assert not np.signbit(after["verts"]["v"][after["verts"]["v"] == 0]).any()  # -0.0 + 0.0 == +0.0


def test_empty_mesh_and_mesh_that_backs_no_object():
    import copy

    from vanrijn_amd.scene import MeshSpec
    ds = _host(_mesh_scene(np.zeros((0, 3, 3))).spec())
    ds.transform_mesh(0, MATRICES["rotation"])
    assert _code(lambda: ds.transform_mesh(0, [np.nan] * 12)) == -1  # the matrix check comes first
    a, c = _random_mesh(81, 17), _random_mesh(82, 5)
    spec = copy.copy(_mesh_scene(a).spec())
    spec.meshes = spec.meshes + [MeshSpec(c, _normals(c), 0)]
    ds, twin = _host(spec), _host(spec)
    before = dumps(ds)
    m = [30.0 * x for x in MATRICES["rotation"]]
    w, wn = transformed(m, c, _normals(c))
    ds.transform_mesh(1, m)
    twin.update_mesh(1, w, wn)
    assert_dumps_equal(dumps(ds), dumps(twin))
    assert ds.info() == twin.info() and ds.info()["extent"] == np.abs(w).max()
    check_refit(ds, [(a, _normals(a)), (w, wn)], before)
