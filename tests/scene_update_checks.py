"""Checks of vr_scene_update_mesh shared by test_scene_update_host.py and test_gpu_scene_update.py:
the dumps of a DeviceScene (binary nodes, 4-wide nodes, triangle records, root records) against what
an exact bottom-up refit of the same topology must hold, computed here with numpy alone.

Comparisons are by value (==, NaN == NaN where a NaN is expected): a zero's sign may differ.
"""
import numpy as np

from vanrijn_amd.scene import DeviceScene

EMPTY = DeviceScene.EMPTY_CHILD


def dumps(ds):
    """The four dumps of a scene's current state."""
    v, n = ds.triangles()
    return {"nodes": ds.bvh_nodes(), "wide": ds.wide_nodes(), "verts": v, "normals": n, "roots": ds.bvh_roots()}


def assert_dumps_equal(a, b):
    for key in ("nodes", "wide", "verts", "normals", "roots"):
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        for f in a[key].dtype.names:
            x, y = a[key][f], b[key][f]
            if x.dtype.kind == "f":
                assert np.array_equal(x, y, equal_nan=True), (key, f)
            else:
                assert np.array_equal(x, y), (key, f)


def round_outward(box):
    """[.., 6] f64 {min, max} x 3 -> f32, lower bounds rounded down and upper bounds up."""
    box = np.asarray(box, dtype=np.float64)
    f = box.astype(np.float32)
    down = np.nextafter(f, np.float32(-np.inf))
    up = np.nextafter(f, np.float32(np.inf))
    lower = np.where(f.astype(np.float64) > box, down, f)
    upper = np.where(f.astype(np.float64) < box, up, f)
    is_upper = (np.arange(6) % 2 == 1)
    return np.where(is_upper, upper, lower).astype(np.float32)


def _tri_boxes(v):
    """[n][3][3] vertices -> [n][6] {min x, max x, min y, max y, min z, max z}."""
    out = np.empty((len(v), 6))
    out[:, 0::2] = v.min(axis=1)
    out[:, 1::2] = v.max(axis=1)
    return out


def _union(boxes):
    boxes = np.asarray(boxes).reshape(-1, 6)
    out = np.empty(6, dtype=boxes.dtype)
    out[0::2] = boxes[:, 0::2].min(axis=0)
    out[1::2] = boxes[:, 1::2].max(axis=0)
    return out


def check_refit(ds, geometry, before=None):
    """`geometry`: per mesh of ds.spec, in order, its current (vertices, normals) as [n][3][3] arrays.
    `before`: dumps taken earlier -- ranks and child links must be unchanged since.  Asserts that
    every slot holds its input triangle, every binary child box == the union of its subtree's triangle
    boxes, every 4-wide leaf slot == the outward-rounded triangle box, every interior slot == the
    union below it, empty slots are NaN, and every root record is the union of its mesh."""
    d = dumps(ds)
    nodes, wide, verts, normals, roots = d["nodes"], d["wide"], d["verts"], d["normals"], d["roots"]
    if before is not None:
        assert np.array_equal(before["verts"]["rank"], verts["rank"])
        assert np.array_equal(before["nodes"]["child"], nodes["child"])
        assert np.array_equal(before["wide"]["child"], wide["child"])
        assert np.array_equal(before["roots"][["root", "root4", "object", "tri_base", "material"]],
                              roots[["root", "root4", "object", "tri_base", "material"]])
    # slots: slot i of a mesh holds input triangle leaf_order[rank - tri_base]
    want_v = np.empty((len(verts), 3, 3))
    want_n = np.empty((len(verts), 3, 3))
    base = 0
    mesh_range = []
    for mi, (gv, gn) in enumerate(geometry):
        gv = np.asarray(gv, dtype=np.float64).reshape(-1, 3, 3)
        gn = np.asarray(gn, dtype=np.float64).reshape(-1, 3, 3)
        n = len(gv)
        assert n == len(ds.spec.meshes[mi].vertices)
        order = ds.leaf_order(mi).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(n))
        rank = verts["rank"][base:base + n] - base
        assert np.array_equal(np.sort(rank), np.arange(n))
        want_v[base:base + n] = gv[order[rank]]
        want_n[base:base + n] = gn[order[rank]]
        mesh_range.append((base, n))
        base += n
    assert base == len(verts)
    assert np.array_equal(verts["v"], want_v)
    assert np.array_equal(normals["n"], want_n, equal_nan=True)
    tbox = _tri_boxes(want_v)
    tbox32 = round_outward(tbox)
    # binary tree: box[c] == union of the subtree's triangle boxes
    memo = {}

    def subtree(ch):  # child code -> f64 box
        if ch < 0:
            return tbox[~ch]
        if ch not in memo:
            memo[ch] = _union([subtree(int(nodes["child"][ch, 0])), subtree(int(nodes["child"][ch, 1]))])
        return memo[ch]

    for i in range(len(nodes)):
        for c in range(2):
            assert np.array_equal(nodes["box"][i, c], subtree(int(nodes["child"][i, c]))), (i, c)
    # 4-wide tree: leaf slots the rounded triangle box, interior slots the union below, empty slots NaN
    memo4 = {}

    def subtree4(ch):  # child code -> f32 box
        if ch < 0:
            return tbox32[~ch]
        if ch not in memo4:
            kids = [int(k) for k in wide["child"][ch] if k != EMPTY]
            assert len(kids) >= 2
            memo4[ch] = _union([subtree4(k) for k in kids])
        return memo4[ch]

    for i in range(len(wide)):
        for s in range(4):
            ch = int(wide["child"][i, s])
            got = wide["bound"][i, :, s]
            if ch == EMPTY:
                assert np.isnan(got).all(), (i, s)
            else:
                assert np.array_equal(got, subtree4(ch)), (i, s)
    # roots: the union of everything, and that rounded outward
    mesh_of_object = {}
    for oi, o in enumerate(ds.spec.objects):
        if o.kind == "bvh":
            mesh_of_object[oi] = o.mesh
    assert len(roots) == len(mesh_of_object)
    for r in roots:
        b, n = mesh_range[mesh_of_object[int(r["object"])]]
        assert int(r["tri_base"]) == b
        if n == 0:
            continue
        u = _union(tbox[b:b + n])
        assert np.array_equal(r["root_box"], u)
        assert np.array_equal(r["root_box32"], round_outward(u))
    return d
