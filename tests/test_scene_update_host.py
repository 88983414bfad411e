"""vr_scene_update_mesh on VR_SCENE_HOST_ONLY scenes (no GPU): there the host form runs the refit in
plain C++ on the host arrays -- the same per-record steps the device kernels run (vr_refit.h), and
the reference tests/test_gpu_scene_update.py compares the device refit with.

Checked against tests/scene_update_checks.py: an exact bottom-up refit computed with numpy.
"""
import os
import re

import numpy as np
import pytest

from scene_update_checks import assert_dumps_equal, check_refit, dumps
from vanrijn_amd import _native as N
from vanrijn_amd.scene import (BoundingVolumeHierarchy, DeviceScene, LambertianMaterial, Mesh, Plane, Scene, Sphere,
                               Spectrum)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _normals(v):
    n = np.zeros_like(v)
    n[..., 2] = 1.0
    return n


def _random_mesh(rng, n):
    return rng.normal(size=(n, 3, 3))


def _mesh_scene(v):
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    return Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(v, _normals(v), mat))])


def _host(scene, **kw):
    return DeviceScene(scene.spec(), 0, host_only=True, **kw)


def _code(call):
    try:
        call()
    except N.VrError as e:
        return e.code
    return 0


def test_header_define_and_abi():
    text = open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()
    assert re.search(r"^#define VR_HAS_SCENE_UPDATE 1\b", text, flags=re.M)
    assert re.search(r"^#define VR_ABI_VERSION 10\b", text, flags=re.M)
    assert N.lib().vr_abi_version() == 10


def test_argument_errors_leave_the_scene_untouched():
    rng = np.random.default_rng(3)
    v = _random_mesh(rng, 17)
    ds = _host(_mesh_scene(v))
    before = dumps(ds)
    info = ds.info()
    w = _random_mesh(rng, 17)
    L = N.lib()
    ptr = w.ctypes.data
    assert L.vr_scene_update_mesh(None, 0, 17, ptr, ptr) == -1           # null scene
    assert L.vr_scene_update_mesh(ds.handle, 0, 17, None, ptr) == -1     # null arrays
    assert L.vr_scene_update_mesh(ds.handle, 0, 17, ptr, None) == -1
    assert L.vr_scene_update_mesh(ds.handle, 1, 17, ptr, ptr) == -1      # bad mesh index
    assert L.vr_scene_update_mesh(ds.handle, 0, 16, ptr, ptr) == -1      # count mismatch
    assert _code(lambda: ds.update_mesh(0, w[:16], _normals(w[:16]))) == -1
    assert L.vr_scene_update_mesh_device(ds.handle, 0, 17, ptr, ptr, None) == -8  # device form, host-only scene
    for bad in (np.nan, np.inf, -np.inf):
        x = w.copy()
        x[11, 2, 1] = bad
        assert _code(lambda: ds.update_mesh(0, x, _normals(x))) == -7    # non-finite vertex: VR_ERROR_UNSUPPORTED
    assert_dumps_equal(before, dumps(ds))
    assert ds.info() == info
    # normals may be anything: NaN normals are accepted (and clear NAN_FREE)
    nn = _normals(w)
    nn[3, 0, 0] = np.nan
    ds.update_mesh(0, w, nn)
    assert not ds.info()["nan_free"]
    check_refit(ds, [(w, nn)], before)


def test_empty_mesh_update_is_ok():
    ds = _host(_mesh_scene(np.zeros((0, 3, 3))))
    ds.update_mesh(0, np.zeros((0, 3, 3)), np.zeros((0, 3, 3)))
    assert N.lib().vr_scene_update_mesh(ds.handle, 0, 0, None, None) == 0
    assert _code(lambda: ds.update_mesh(0, np.zeros((1, 3, 3)), np.zeros((1, 3, 3)))) == -1


@pytest.mark.parametrize("reference_bvh", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 1000])
def test_refit_to_uncorrelated_geometry(n, reference_bvh):
    """New random geometry from another seed: every box of the old tree is stale, the worst case."""
    a = _random_mesh(np.random.default_rng(n), n)
    b = 3.0 * _random_mesh(np.random.default_rng(1000 + n), n) + 0.5
    ds = _host(_mesh_scene(a), reference_bvh=reference_bvh)
    before = check_refit(ds, [(a, _normals(a))])
    ds.update_mesh(0, b, _normals(b))
    check_refit(ds, [(b, _normals(b))], before)
    fresh = _host(_mesh_scene(b), reference_bvh=reference_bvh)
    assert ds.info()["extent"] == fresh.info()["extent"]
    assert ds.info()["nan_free"] == fresh.info()["nan_free"]
    for key in ("triangle_count", "node_count", "wide_node_count", "traversal_stack", "max_bvh_depth"):
        assert ds.info()[key] == _host(_mesh_scene(a), reference_bvh=reference_bvh).info()[key]
    ds.update_mesh(0, a, _normals(a))  # on the cached plan
    assert_dumps_equal(before, dumps(ds))
    assert ds.info()["extent"] == _host(_mesh_scene(a)).info()["extent"]


def test_nan_free_follows_the_normals():
    rng = np.random.default_rng(8)
    # facing triangles: vertex normals on the geometric normal's side
    v = _random_mesh(rng, 17)
    f = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    good = np.repeat((f / np.linalg.norm(f, axis=1, keepdims=True))[:, None, :], 3, axis=1)
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    ds = _host(Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(v, good, mat))]))
    assert ds.info()["nan_free"]
    ds.update_mesh(0, v, np.zeros_like(v))  # mesh.rs:37: an OBJ without normals
    assert not ds.info()["nan_free"]
    fresh = _host(Scene((0.0, 0.0, -5.0), [BoundingVolumeHierarchy.build(Mesh(v, np.zeros_like(v), mat))]))
    assert not fresh.info()["nan_free"]
    ds.update_mesh(0, v, good)
    assert ds.info()["nan_free"]


def test_mesh_that_backs_no_object():
    """It has triangle records and binary nodes but no root record and no 4-wide nodes; it is updated
    like any other, and counts for the extent as it did at creation, not for NAN_FREE."""
    import copy

    from vanrijn_amd.scene import MeshSpec
    rng = np.random.default_rng(31)
    a, b = _random_mesh(rng, 17), _random_mesh(rng, 5)
    spec = copy.copy(_mesh_scene(a).spec())
    spec.meshes = spec.meshes + [MeshSpec(b, _normals(b), 0)]
    ds = DeviceScene(spec, 0, host_only=True)
    before = check_refit(ds, [(a, _normals(a)), (b, _normals(b))])
    assert len(before["roots"]) == 1 and len(before["verts"]) == 22
    nan_free = ds.info()["nan_free"]
    big = 50.0 * _random_mesh(rng, 5)
    ds.update_mesh(1, big, np.zeros_like(big))
    check_refit(ds, [(a, _normals(a)), (big, np.zeros_like(big))], before)
    assert ds.info()["extent"] == np.abs(big).max()
    assert ds.info()["nan_free"] == nan_free
    ds.update_mesh(1, b, _normals(b))
    assert_dumps_equal(before, dumps(ds))


def test_two_meshes_plane_and_sphere():
    rng = np.random.default_rng(21)
    mat = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    m0, m1 = 40.0 * _random_mesh(rng, 17), 100.0 * _random_mesh(rng, 1000)

    def scene(a, b):
        return Scene((0.0, 0.0, -5.0), [[Plane((0.0, 1.0, 0.0), -2.0, mat), Sphere((1.0, 2.0, 3.0), 1.5, mat)],
                                        BoundingVolumeHierarchy.build(Mesh(a, _normals(a), mat)),
                                        BoundingVolumeHierarchy.build(Mesh(b, _normals(b), mat))])

    ds = _host(scene(m0, m1))
    before = check_refit(ds, [(m0, _normals(m0)), (m1, _normals(m1))])
    assert ds.info()["extent"] == np.abs(m1).max() > np.abs(m0).max()
    small = 0.01 * _random_mesh(rng, 1000)  # mesh 1 shrinks: the extent follows mesh 0
    ds.update_mesh(1, small, _normals(small))
    after = check_refit(ds, [(m0, _normals(m0)), (small, _normals(small))], before)
    assert ds.info()["extent"] == np.abs(m0).max() == _host(scene(m0, small)).info()["extent"]
    # mesh 0's slots, nodes and root record are untouched
    def mesh0(d):  # 17 slots, 16 interior nodes, the first root record; its wide nodes below
        return {"verts": d["verts"][:17], "normals": d["normals"][:17], "nodes": d["nodes"][:16],
                "roots": d["roots"][:1], "wide": d["wide"][:0]}

    assert_dumps_equal(mesh0(before), mesh0(after))
    reach, todo = set(), [int(before["roots"]["root4"][0])]
    while todo:  # mesh 0's wide nodes, from its root
        x = todo.pop()
        reach.add(x)
        todo += [int(c) for c in before["wide"]["child"][x] if c >= 0]
    idx = np.array(sorted(reach))
    assert np.array_equal(before["wide"][idx]["bound"], after["wide"][idx]["bound"], equal_nan=True)
    ds.update_mesh(1, m1, _normals(m1))
    assert_dumps_equal(before, dumps(ds))
    assert ds.info()["extent"] == np.abs(m1).max()
