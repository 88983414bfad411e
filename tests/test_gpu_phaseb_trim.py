"""The trimmed node step and leaf append of the render kernel's traversal loop (vr_render_kernel.h phase B).

The leaf append tells a queued leaf by one unsigned compare on the hit child's link, (uint32_t)link >
0x80000000u: negative and not the empty slot's INT32_MIN.  An empty slot's link alone keeps it off the stack
(its key has bit 31 set) and out of the leaf queue, also for rays whose margin e2 is +inf, for which the f32
test says "maybe" to the slot's NaN bounds -- so these cases hold with the step's emptiness test in front of
the box test (what the kernels do) and would hold without it (measured, not adopted).
The 16-bit stack kernels of one material kind push raw child keys with exactly 16 index bits, so bit 15 of a
node index shares a store with the distance bits above it.  Each case compares device records bit for bit against a launch that does not depend
on the change in the same way (another tree, the 32-bit stack) and decisions against the oracle.

  a. trees whose nodes have empty slots (2, 3, 5, 6, 7 triangles: one or two per node -- a 4-wide node has
     at least two children, so no tree has a node with three)
  b. the same under e2 = +inf (tests/magnitude_scenes.py's map at (3e34, 0): some rays, and (1e36, 0): every ray)
  c. a tree of 32,768 to 65,535 wide nodes on the 16-bit stack
  d. distance ties (tests/test_gpu_ties.py's scene) on the 16-bit stack
"""
import numpy as np
import pytest
import torch

import magnitude_scenes as M
from test_gpu_build import _mesh_scene, _random_mesh
from test_gpu_node_layout import _decisions_equal
from test_gpu_ties import _tied_scene
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import Tile, render_samples, render_tile_device
from vanrijn_amd.scene import DeviceScene

pytestmark = pytest.mark.gpu

SEED = 0x5EED0A11
ONE, S16 = N.VARIANT_ONE_BVH, N.VARIANT_STACK16
EMPTY = DeviceScene.EMPTY_CHILD
SMALL = (2, 3, 5, 6, 7)


def _small_scene(n, regime=(1.0, 0.0), seed=None):
    v = M.mapped(_random_mesh(np.random.default_rng(46 + n if seed is None else seed), n), *regime)
    return _mesh_scene(v, camera=tuple(M.mapped((0.0, 0.0, -5.0), *regime)))


def _records(ds, tile, H, W, spp, more=0, seed=SEED, **kw):
    """The device records of one launch (then `more` samples added onto them) as int64, and the last launch's stats"""
    st = torch.zeros(tile.width() * tile.height() * 8, dtype=torch.float64, device="cuda")
    s = render_tile_device(ds, tile, H, W, spp, seed, 0, st.data_ptr(), **kw)
    if more:
        s = render_tile_device(ds, tile, H, W, more, seed, spp, st.data_ptr(), accumulate=True, **kw)
    torch.cuda.synchronize()
    return st.cpu().view(torch.int64), s


# ------------------------------------------------------------------------------------- a. empty slots
def test_the_small_trees_have_empty_slots():
    """What the cases below rely on: among the five meshes' wide trees (either SAH build) there are full
    nodes and nodes with one and with two empty slots."""
    seen = set()
    for n in SMALL:
        for kw in ({}, {"device_sah": True}):
            child = DeviceScene(_small_scene(n).spec(), 0, **kw).wide_nodes()["child"]
            seen |= set((child == EMPTY).sum(axis=1).tolist())
    assert {0, 1, 2} <= seen


@pytest.mark.parametrize("n", SMALL)
def test_empty_slots_change_no_record_and_no_decision(n, oracle):
    scene = _small_scene(n)
    H = W = 64
    t = Tile(0, W, 0, H)
    want, s = _records(DeviceScene(scene.spec(), 0, reference_bvh=True), t, H, W, 4)
    assert np.count_nonzero(want.numpy()) > 1000
    ref = oracle.OracleScene(scene.spec()).render_samples(t, H, W, 4, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert (ref["flags"] & 1).sum() >= 900  # the camera sees the mesh
    for kw in ({}, {"device_sah": True}):
        ds = DeviceScene(scene.spec(), 0, **kw)
        got, s = _records(ds, t, H, W, 4)
        assert s["variant"] & S16
        assert torch.equal(got, want), kw
        assert torch.equal(_records(ds, t, H, W, 4, stack16=False)[0], want), kw
        _decisions_equal(render_samples(ds, t, H, W, 4, seed=SEED), ref)


# (n, mesh seed, tree): the five meshes on both SAH trees, and a 5-triangle mesh whose reference tree is two
# nodes of three children each -- a multi-node tree in which every node has an empty slot
COUNTED = [(n, None, kw) for n in SMALL for kw in ({}, {"device_sah": True})] + [(5, 18, {"reference_bvh": True})]


@pytest.mark.parametrize("n,seed,kw", COUNTED, ids=lambda v: "-".join(v) if isinstance(v, dict) and v else str(v))
def test_counted_box_tests_leave_empty_slots_out(n, seed, kw):
    """The counting kernel's rule: one box test per traced ray for the BVH's root box, and one per non-empty
    slot of every node visited -- an empty slot is never counted.  With f_i filled slots and V_i visits of
    node i the count is rays + sum f_i V_i; the launch reports sum V_i only.

    Exact where every node has the same f: the one-node trees (2, 3 triangles) and the (3, 3) reference tree.
    The SAH builders always fill the root, so for their multi-node trees the count is bounded by what the
    structure gives: a ray visits the root at most once (V_root <= rays), so at least visits - rays visits are
    of non-root nodes, each of which has an empty slot here (asserted).  A kernel that counted empty slots
    would report rays + 4 visits, above the upper bound whenever visits > rays (asserted)."""
    ds = DeviceScene(_small_scene(n, seed=seed).spec(), 0, **kw)
    H = W = 64
    t = Tile(0, W, 0, H)
    filled = (ds.wide_nodes()["child"] != EMPTY).sum(axis=1)
    want, _ = _records(ds, t, H, W, 4)
    got, s = _records(ds, t, H, W, 4, counters=True)
    assert torch.equal(got, want)
    visits, rays, boxes = int(s["node_visits"]), int(s["rays"]), int(s["box_tests"])
    print(f"n = {n} {kw}: filled slots per node {filled.tolist()}, rays {rays}, node visits {visits}, box tests {boxes}")
    assert visits >= H * W  # most camera rays meet the root box
    if len(set(filled.tolist())) == 1:
        assert filled[0] < 4 and boxes == rays + int(filled[0]) * visits
        return
    assert n >= 5 and seed is None
    r4 = int(ds.bvh_roots()["root4"][0])  # the wide root's index
    root, rest = int(filled[r4]), np.delete(filled, r4)
    assert root == 4 and rest.max() < 4 and visits > rays
    below = visits - rays  # at least this many visits are of non-root nodes
    assert boxes <= rays + 4 * visits - (4 - int(rest.max())) * below < rays + 4 * visits
    # ... and at most visits - visits / (1 + non-root nodes) are: a node is visited at most once per root visit
    most_below = visits - -(-visits // (1 + len(rest)))
    assert boxes >= rays + 4 * visits - (4 - int(rest.min())) * most_below


# --------------------------------------------------------------------- b. empty slots under e2 = +inf
@pytest.mark.parametrize("regime", [(3e34, 0.0), (1e36, 0.0)], ids=M.regime_id)
@pytest.mark.parametrize("n", [5, 7])
def test_empty_slots_with_an_infinite_margin(n, regime, oracle):
    """prepare32's margin is E = 3.001 ek, ek = 6e-7 (max(extent, |o|) + 1) max|1 / d|, and infinite from
    ek >= 1e30 (tests/test_slab_bound.py): the f32 box test then excludes nothing, an empty slot's NaN bounds
    included, and only the link keeps the slot out of the stack and the leaf queue.  At (3e34, 0) that is so
    for the rays with a direction component below about 0.1; at (1e36, 0) for every ray, camera and bounce
    alike (asserted from the scene's extent: |d| = 1 gives max|1 / d| >= sqrt(3))."""
    scene = _small_scene(n, regime=regime)
    H = W = 64
    t = Tile(0, W, 0, H)
    ref = oracle.OracleScene(scene.spec()).render_samples(t, H, W, 4, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert (ref["flags"] & 1).sum() >= 900
    for kw in ({}, {"device_sah": True}):
        ds = DeviceScene(scene.spec(), 0, **kw)
        assert kw or (ds.wide_nodes()["child"] == EMPTY).any()  # (the host tree: checked without a GPU)
        if regime[0] == 1e36:
            assert 6e-7 * ds.info()["extent"] * np.sqrt(3.0) >= 1e30
        for no_dist_cull in (True, False):
            ds.set_launch_flags(no_dist_cull=no_dist_cull)
            _decisions_equal(render_samples(ds, t, H, W, 4, seed=SEED), ref)
        ds.set_launch_flags()
        want, s = _records(ds, t, H, W, 4, stack16=False)
        got, s = _records(ds, t, H, W, 4)
        assert s["variant"] & S16
        assert torch.equal(got, want)
        if regime[0] == 1e36:  # every box test of the launch was too close to call: each queued leaf is re-tested in f64
            c = _records(ds, t, H, W, 4, counters=True)[1]
            assert int(c["exact_box_tests"]) >= int(c["triangle_tests"]) > 0


# ------------------------------------------------------------------- c. bit 15 of the node index in use
def test_stack16_with_bit_15_of_the_index_in_use(oracle):
    """110,592 triangles: node indices up to 2^16 need all 16 bits of a stack entry, and a raw key's bit 15
    is an index bit, not a distance bit."""
    scene = scenes.main_scene(scenes.procedural_bunny(96))
    assert len(scene.spec().meshes[0].vertices) == 110592
    ds = scene.device_scene(0)
    assert 32768 <= ds.info()["wide_node_count"] <= 65535
    H = W = 128
    t = Tile(0, W, 0, H)
    for more in (0, 2):  # fresh, accumulating
        got, s = _records(ds, t, H, W, 2, more=more)
        assert s["variant"] == ONE | S16
        want, s = _records(ds, t, H, W, 2, more=more, stack16=False)
        assert s["variant"] == ONE
        assert torch.equal(got, want)
        assert np.count_nonzero(got.numpy()) > 10000
    crop = Tile(48, 80, 48, 80)
    ref = oracle.OracleScene(scene.spec()).render_samples(crop, H, W, 2, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert (ref["flags"] & 1).sum() >= 500
    _decisions_equal(render_samples(ds, crop, H, W, 2, seed=SEED), ref)


# ---------------------------------------------------------------------------------------------- d. ties
@pytest.mark.parametrize("seed", [1, 2])
def test_ties_on_the_16_bit_stack(seed):
    ds = _tied_scene(seed).device_scene(0)
    H = W = 64
    t = Tile(0, W, 0, H)
    got, s = _records(ds, t, H, W, 6, seed=0x7135 + seed)
    assert s["variant"] == S16  # two meshes: the generic kernel
    want, s = _records(ds, t, H, W, 6, seed=0x7135 + seed, stack16=False)
    assert s["variant"] == 0
    assert torch.equal(got, want)
    assert np.count_nonzero(got.numpy()) > 1000
