"""Device ray queries (vr_query_*, vanrijn_amd/csrc/vr_query.hip) against the oracle's reference mode.

The query kernel walks the render kernel's 4-wide f32 tree for caller-supplied rays; the oracle walks
the reference's binary tree in f64.  The closest hit and its geometry do not depend on the tree
walked and hit_info is shared code, so every comparison here is exact: no tolerances.
"""
import threading

import numpy as np
import pytest

from vanrijn_amd import scenes
from vanrijn_amd.render import (HIT_RECORD_DTYPE, RAY_HIT_DTYPE, query_any, query_any_device, query_closest,
                                query_closest_device, trace_rays)
from vanrijn_amd.scene import (BoundingVolumeHierarchy, ColourRgbF, DeviceScene, LambertianMaterial, Mesh, Plane, Scene,
                               Spectrum)

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 257, 8002)  # one lane, a partial wave, a partial workgroup, many workgroups


# ------------------------------------------------------------------------------------- helpers
def _ref_arrays(ref):
    """The oracle's hits as arrays: valid, object, primitive, distance and the five vectors."""
    out = {"valid": np.array([h.valid for h in ref], dtype=bool), "object": np.array([h.object for h in ref]),
           "primitive": np.array([h.primitive for h in ref]), "distance": np.array([h.distance for h in ref])}
    for f in ("location", "normal", "tangent", "cotangent", "retro"):
        out[f] = np.array([list(getattr(h, f)) for h in ref]).reshape(-1, 3)
    return out


def _slice(r, sel):
    return {k: v[sel] for k, v in r.items()}


def _bits_equal(a, b):
    """Equal as numbers, NaN matching NaN (tests/test_gpu_parity.py _compare_hits)."""
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _compare_ray_hits(hits, r):
    v = r["valid"]
    assert np.array_equal(hits["valid"].astype(bool), v)
    assert np.array_equal(hits["object"][v], r["object"][v])
    assert np.array_equal(hits["primitive"][v], r["primitive"][v])
    assert _bits_equal(hits["distance"][v], r["distance"][v])
    assert not hits["distance"][~v].any()  # 0 when valid == 0


def _compare_records(rec, r):
    v = r["valid"]
    assert np.array_equal(rec["valid"].astype(bool), v)
    assert np.array_equal(rec["object"][v], r["object"][v])
    assert np.array_equal(rec["primitive"][v], r["primitive"][v])
    assert _bits_equal(rec["distance"][v], r["distance"][v])
    for f in ("location", "normal", "tangent", "cotangent", "retro"):
        assert _bits_equal(rec[f][v], r[f][v]), f


def _check_all(scene, o, d, r, **kw):
    """Closest (compact and full records) and any against the oracle's arrays `r`."""
    hits, rec = query_closest(scene, o, d, records=True, **kw)
    _compare_ray_hits(hits, r)
    _compare_records(rec, r)
    _compare_ray_hits(query_closest(scene, o, d, **kw), r)
    assert np.array_equal(query_any(scene, o, d, **kw), r["valid"])


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _ray_batch(spec, n, seed):
    """tests/test_gpu_parity.py's recipe: n camera rays into the scene's volume, n random rays inside it."""
    g = np.random.default_rng(seed)
    cam = np.array(spec.camera_location)
    tgt = g.uniform([-3.5, -2.5, -1.5], [0.5, 1.5, 1.5], (n, 3))
    o = np.concatenate([np.repeat(cam[None], n, 0), g.uniform([-3.5, -1.9, -1.5], [0.0, 1.2, 1.3], (n, 3))])
    d = np.concatenate([tgt - cam, g.normal(size=(n, 3))])
    return o, _unit(d)


def _main_rays(spec, orc, oracle):
    """8002 rays of the main scene, shuffled so that every prefix mixes the kinds: camera and random
    rays (_ray_batch), bounce-like rays from surface points (hit point + 1e-7 d, d random), and rays
    that start on a surface and point outward (d on the side the surface was seen from: the boxes
    they leave lie behind the origin, pass the line test, and the triangle test rejects them)."""
    o, d = _ray_batch(spec, 2600, 1)
    first, _ = orc.trace(o[:2600], d[:2600], oracle.MODE_REFERENCE)
    pts = np.array([list(h.location) for h in first if h.valid])
    retro = np.array([list(h.retro) for h in first if h.valid])
    g = np.random.default_rng(3)
    dirs = _unit(g.normal(size=pts.shape))
    out = _unit(g.normal(size=pts.shape))
    out = np.where((np.sum(out * retro, axis=1) < 0)[:, None], -out, out)
    kind = np.concatenate([np.zeros(2600, int), np.ones(2600, int), np.full(len(pts), 2), np.full(len(pts), 3)])
    o = np.concatenate([o, pts + dirs * 1e-7, pts + out * 1e-7])
    d = np.concatenate([d, dirs, out])
    assert len(o) >= BATCHES[-1]
    order = np.random.default_rng(4).permutation(len(o))[:BATCHES[-1]]
    return np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order]), kind[order]


# ------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def main_case(oracle):
    """The main scene, its 8002 rays and the oracle's answers (computed once, never modified); the
    rays' kinds (0 camera, 1 random, 2 bounce-like, 3 outward from a surface) ride on the scene."""
    scene = scenes.main_scene(scenes.procedural_bunny())
    orc = oracle.OracleScene(scene.spec())
    o, d, scene.query_test_kinds = _main_rays(scene.spec(), orc, oracle)
    ref, _ = orc.trace(o, d, oracle.MODE_REFERENCE)
    r = _ref_arrays(ref)
    for a in (o, d, *r.values()):
        a.setflags(write=False)
    return scene, orc, o, d, r


# --------------------------------------------------------------------- 1. oracle parity, main scene
@pytest.mark.parametrize("n", BATCHES)
def test_main_scene_matches_oracle(n, main_case):
    scene, _, o, d, r = main_case
    _check_all(scene, o[:n], d[:n], _slice(r, slice(0, n)))


# -------------------------------------------------------------------------- 2. the three walks agree
def test_three_walks_give_identical_records(main_case):
    scene, _, o, d, _ = main_case
    wide_hits, wide = query_closest(scene, o, d, records=True)
    ref_hits, ref = query_closest(scene, o, d, records=True, reference_walk=True)
    old = trace_rays(scene, o, d)
    for f in HIT_RECORD_DTYPE.names:
        assert np.array_equal(wide[f], ref[f]), f
        assert np.array_equal(wide[f], old[f]), f
    for f in RAY_HIT_DTYPE.names:
        assert np.array_equal(wide_hits[f], ref_hits[f]), f
    assert np.array_equal(query_any(scene, o, d), query_any(scene, o, d, reference_walk=True))
    assert wide["valid"].sum() > 1000


# -------------------------------------------------------------------------------------------- 3. ties
def _tied_scene(seed):
    """tests/test_gpu_ties.py's construction: every triangle two or three times at the same place, a
    second BVH object repeating 300 of them, and a plane."""
    g = np.random.default_rng(seed)
    n = 600
    centre = g.uniform([-1.2, -0.8, -0.6], [1.2, 0.8, 0.6], (n, 1, 3))
    verts = centre + g.normal(scale=0.18, size=(n, 3, 3))
    reps = g.integers(2, 4, n)
    v_all, n_all = [], []
    for i in range(n):
        for _ in range(reps[i]):
            v_all.append(verts[i])
            n_all.append(g.normal(size=(3, 3)) + np.array([0.0, 0.0, -1.5]))
    order = g.permutation(len(v_all))
    v_all = np.array(v_all)[order]
    n_all = np.array(n_all)[order]
    a = LambertianMaterial(Spectrum.grey(0.7), 0.6)
    b = LambertianMaterial(Spectrum.reflection_from_linear_rgb(ColourRgbF(0.2, 0.9, 0.4)), 0.8)
    floor = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    first = BoundingVolumeHierarchy.build(Mesh(v_all, n_all, a))
    second = BoundingVolumeHierarchy.build(Mesh(v_all[:300].copy(), n_all[:300][:, ::-1].copy(), b))
    return Scene((0.0, 0.0, -4.0), [[Plane((0.0, 1.0, 0.0), -1.5, floor)], first, second])


def _pixel_centre_rays(oracle, camera, width, height):
    rays = [oracle.ray_for_pixel(camera, width, height, row, col, 0.5, 0.5) for row in range(height)
            for col in range(width)]
    return np.array([r[0] for r in rays]), np.array([r[1] for r in rays])


@pytest.mark.parametrize("seed", [1, 2])
def test_ties_go_to_the_reference_winner(seed, oracle):
    scene = _tied_scene(seed)
    orc = oracle.OracleScene(scene.spec())
    o, d = _pixel_centre_rays(oracle, scene.spec().camera_location, 64, 64)
    ref, _ = orc.trace(o, d, oracle.MODE_REFERENCE)
    r = _ref_arrays(ref)
    assert (r["valid"] & (r["object"] > 0)).sum() > 1000  # of the 4096 rays, those that hit a mesh
    for kw in ({}, {"reference_walk": True}):
        hits = query_closest(scene, o, d, **kw)
        v = r["valid"]
        assert np.array_equal(hits["valid"].astype(bool), v)
        assert np.array_equal(hits["object"][v], r["object"][v])
        assert np.array_equal(hits["primitive"][v], r["primitive"][v])
        assert np.array_equal(query_any(scene, o, d, **kw), v)


# ------------------------------------------------------------------- 4. small trees and scene flags
SCENE_FLAGS = ({}, {"reference_bvh": True}, {"greedy_collapse": True}, {"device_sah": True}, {"wide_offsets": True})


@pytest.mark.parametrize("tris", [0, 1, 2, 3, 4, 5, 17, 4097])
def test_small_trees_under_every_scene_flag(tris, oracle):
    """An empty mesh, a leaf root, a root Node4 with empty (NaN) slots, a partial last level and
    several levels; random triangles in a unit box, the camera outside."""
    g = np.random.default_rng(100 + tris)
    verts = g.uniform(-0.5, 0.5, (tris, 1, 3)) + g.normal(scale=0.25 if tris < 100 else 0.03, size=(tris, 3, 3))
    verts = np.clip(verts, -0.5, 0.5)
    norms = g.normal(size=(tris, 3, 3)) + np.array([0.0, 0.0, -2.0])
    mat = LambertianMaterial(Spectrum.grey(0.8), 0.5)
    scene = Scene((0.1, 0.2, -3.0), [BoundingVolumeHierarchy.build(Mesh(verts, norms, mat))])
    n = 300
    cam = np.array(scene.spec().camera_location)
    o = np.concatenate([np.repeat(cam[None], n, 0), g.uniform(-0.7, 0.7, (n, 3))])
    d = _unit(np.concatenate([g.uniform(-0.6, 0.6, (n, 3)) - cam, g.normal(size=(n, 3))]))
    ref, _ = oracle.OracleScene(scene.spec()).trace(o, d, oracle.MODE_REFERENCE)
    r = _ref_arrays(ref)
    assert r["valid"].any() == (tris > 0)
    for flags in SCENE_FLAGS:
        ds = DeviceScene(scene.spec(), 0, **flags)
        _check_all(ds, o, d, r)


# --------------------------------------------------------------------------------------- 5. hard rays
def _hard_rays(spec):
    """The issue's hard directions and origins on the main scene.  Origins avoid the mesh's planes of
    symmetry only so that no ray runs along a lattice edge; that is not what test_hard_rays leaves out."""
    g = np.random.default_rng(11)
    cam = np.array(spec.camera_location)
    centre = np.array([-1.7, -0.8, 0.0])  # of the mesh's root box
    inside = centre + [0.0137, 0.0211, -0.0173]  # a generic point inside it
    o, d = [], []
    # directions with one or two exactly-zero components, -0.0 components and 1e-200 components
    # (renormalised: the vector stays unit length in f64), from origins around and inside the mesh
    origins = [cam, inside, inside + [0.0, 3.0, 0.0], inside + [3.0, 0.2, 0.1], inside - [0.3, 0.1, 4.0],
               np.array([-1.6831, -2.0, 0.0127]), np.array([0.5013, -2.0, -1.0191])]  # the last two: exactly on the plane
    for oo in origins:
        for axis in range(3):
            for sign in (1.0, -1.0):
                for tiny in (0.0, -0.0, 1e-200, -1e-200):
                    v = np.full(3, tiny)
                    v[axis] = sign
                    o.append(oo); d.append(v)  # two zero (or tiny) components
                    w = g.normal(size=3)
                    w[axis] = tiny
                    o.append(oo); d.append(w)  # one
    o, d = np.array(o, dtype=float), np.array(d, dtype=float)
    d = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    # origins 1e6 away, pointing at the scene and away from it
    far_d = _unit(g.normal(size=(40, 3)))
    far_o = inside + g.uniform(-0.8, 0.8, (40, 3)) - far_d * 1e6
    back = _unit(far_o - inside)
    # origins inside the root box and exactly on the plane, random directions
    ins_o = inside + g.uniform(-0.9, 0.9, (60, 3))
    on_o = np.stack([g.uniform(-4, 1, 40), np.full(40, -2.0), g.uniform(-2, 2, 40)], axis=1)
    o = np.concatenate([o, far_o, far_o, ins_o, on_o])
    d = np.concatenate([d, far_d, back, _unit(g.normal(size=(60, 3))), _unit(g.normal(size=(40, 3)))])
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


def test_hard_rays(main_case, oracle):
    """Equal to the oracle for closest and any, on every ray for which the reference's answer is a
    function of the scene.  It is not one where the oracle's closest hit is a triangle at distance
    NaN: a direction whose largest signed component is 0 (such as (-1, 0, 0)) makes the reference's
    shear -d/0 (triangle.rs:129-131), every edge function NaN, and the `hit` a matter of NaN sign
    bits; closest_intersection then keeps the right subtree's hit unless the left one is smaller, so
    which NaN hit survives depends on the shape of the reference's own tree (and not only on the leaf
    order, which is all another tree can reproduce).  The kernels' rule there is the one of the
    parent's walk: a NaN distance never replaces a hit and is never replaced.  Measured on the first
    version of this set (the same rays from origins on the mesh's axes): 4 of the 516 rays were of
    that kind, as 4 are now; on them vr_trace_rays differs from the
    oracle in 3, the binary query walk in 3 and the 4-wide walk in 4 (the triangle named; `valid`
    agreed on all), and the binary any-hit walk differs from the oracle's `valid` on 4 rays of the set
    while the 4-wide one agrees on all 516.  Those rays are traced with the rest and left out of the
    comparison; the selection reads the oracle alone."""
    scene, orc, _, _, _ = main_case
    o, d = _hard_rays(scene.spec())
    ref, _ = orc.trace(o, d, oracle.MODE_REFERENCE)
    r = _ref_arrays(ref)
    undefined = r["valid"] & (r["object"] == 1) & np.isnan(r["distance"])
    assert undefined.sum() <= len(o) // 50
    sel = ~undefined
    r = _slice(r, sel)
    assert r["valid"].sum() >= 10 and (~r["valid"]).sum() >= 10
    assert np.isnan(r["distance"][r["valid"]]).any()  # NaN-distance plane hits (a ray inside the plane) stay in
    assert len(query_closest(scene, o, d)) == len(o) and len(query_any(scene, o, d)) == len(o)
    _check_all(scene, o[sel], d[sel], r)
    hits, rec = query_closest(scene, o[sel], d[sel], records=True, reference_walk=True)
    _compare_ray_hits(hits, r)
    _compare_records(rec, r)


# ---------------------------------------------------------------------- 6. any-hit is not vacuous
def test_any_hit_set_is_mixed(main_case):
    scene, _, _, _, r = main_case
    frac = r["valid"].mean()
    assert 0.2 < frac < 0.8, frac
    # the rays that start on a surface and point outward: the surface they leave is behind them
    outward = scene.query_test_kinds == 3
    assert outward.sum() > 1000
    assert (outward & ~r["valid"]).sum() > 100 and (outward & r["valid"]).sum() > 100


# ------------------------------------------------------------------------------ 7. VR_QUERY_NORMALIZE
def test_normalize_flag_is_ray_new(main_case, oracle):
    scene, orc, o, d, _ = main_case
    g = np.random.default_rng(21)
    n = 512
    scaled = d[:n] * np.exp(g.uniform(np.log(1e-3), np.log(1e3), (n, 1)))
    unit = np.array([oracle.ray_new(o[i], scaled[i])[1] for i in range(n)])
    ref, _ = orc.trace(o[:n], unit, oracle.MODE_REFERENCE)
    _check_all(scene, o[:n], scaled, _ref_arrays(ref), normalize=True)


# ------------------------------------------------- 8. device form, stream order, no stray writes
def test_device_form_is_stream_ordered_and_writes_only_n(main_case):
    import torch
    scene, _, o, d, _ = main_case
    n, pad = 2049, 64
    want_hits, want_rec = query_closest(scene, o[:n], d[:n], records=True)
    want_any = query_any(scene, o[:n], d[:n])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        # the inputs are products of torch ops queued on this stream: the queries must run after them
        to = torch.from_numpy(o[:n].copy()).cuda(non_blocking=True) * 2.0 * 0.5
        td = torch.from_numpy(d[:n].copy()).cuda(non_blocking=True) + 0.0
        hits = torch.full(((n + pad) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
        rec = torch.full(((n + pad) * 144,), 0xA5, dtype=torch.uint8, device="cuda")
        hits2 = torch.full(((n + pad) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
        anyh = torch.full((n + pad,), 0xA5, dtype=torch.uint8, device="cuda")
        query_closest_device(scene, n, to.data_ptr(), td.data_ptr(), hits.data_ptr(), rec.data_ptr(),
                             stream_ptr=stream.cuda_stream)
        query_closest_device(scene, n, to.data_ptr(), td.data_ptr(), hits2.data_ptr(), None,
                             stream_ptr=stream.cuda_stream, reference_walk=True)
        query_any_device(scene, n, to.data_ptr(), td.data_ptr(), anyh.data_ptr(), stream_ptr=stream.cuda_stream)
    stream.synchronize()
    hits, rec, hits2, anyh = (t.cpu().numpy() for t in (hits, rec, hits2, anyh))
    assert hits[:n * 32].tobytes() == want_hits.tobytes()
    assert hits2[:n * 32].tobytes() == want_hits.tobytes()
    assert rec[:n * 144].tobytes() == want_rec.tobytes()
    assert np.array_equal(anyh[:n].astype(bool), want_any)
    assert (hits[n * 32:] == 0xA5).all() and (rec[n * 144:] == 0xA5).all()  # the canaries
    assert (hits2[n * 32:] == 0x5A).all() and (anyh[n:] == 0xA5).all()


# --------------------------------------------------------------------------------- 9. concurrency
def test_four_threads_share_a_scene(main_case):
    scene, _, o, d, _ = main_case
    parts = [slice(k * 2000, k * 2000 + 1500 + 37 * k) for k in range(4)]
    serial = [(query_closest(scene, o[p], d[p], records=True), query_any(scene, o[p], d[p])) for p in parts]
    got, errors = [None] * 4, []

    def work(k):
        try:
            p = parts[k]
            got[k] = (query_closest(scene, o[p], d[p], records=True), query_any(scene, o[p], d[p]))
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(4):
        (h, r), a = got[k]
        (sh, sr), sa = serial[k]
        assert h.tobytes() == sh.tobytes() and r.tobytes() == sr.tobytes() and np.array_equal(a, sa)
