"""The f32 pre-tests, the distance cull and the device-built trees against the oracle where their
margins depend on the scene's magnitude (tests/magnitude_scenes.py: one unit description through
x -> S x + T at twelve (S, T)).

Every other GPU test runs scenes of size 1 to 5 near the origin, where f32 resolves the geometry,
its squares are normal numbers and prepare32's E is small and finite.  Here the same kernels (the
v_rcp_f32 reciprocal and packed fma of the node step, coop_step, lone_walk, walk4, the cull pass,
fill_wide_kernel) meet boxes f32 cannot tell apart, E = inf for some or all rays of a launch, squares
that underflow or overflow, and rays that pass a box corner within a few ulp -- the only rays that
sit on the margin at all (random rays give no near-ties).  The reference is the oracle's f64
reference mode throughout; guards read the oracle and numpy alone.

  a. caller rays (query_closest with records, query_any, both walks; trace_rays; integrate_rays)
  b. the megakernel's per-sample decisions, for five trees with the distance cull on and off
  c. kernel instantiations and culls leave the device records bit-identical; the mix of f32 and
     f64 box tests is the intended one (counters)
  d. distance ties (tests/test_gpu_ties.py's scene) where cull_far + E meets equal distances
"""
import json

import numpy as np
import pytest
import torch

import magnitude_scenes as M
from vanrijn_amd.render import (Tile, integrate_rays, query_any, query_closest, render_samples, render_tile_device,
                                trace_rays)
from vanrijn_amd.scene import DeviceScene

from test_gpu_integrate import _matches_oracle, _oracle_rays, _staging_order
from test_gpu_node_layout import _decisions_equal
from test_gpu_ray_query import (SCENE_FLAGS, _check_all, _compare_ray_hits, _compare_records, _ref_arrays, _slice)

pytestmark = pytest.mark.gpu

H, W, SPP, SEED = 40, 48, 3, 0x5EED0007  # tests/test_gpu_node_layout.py's tile
TILE = Tile(0, W, 0, H)
regimes = pytest.mark.parametrize("regime", M.REGIMES, ids=M.REGIME_IDS)


@pytest.fixture(scope="module")
def scene_of():
    """Each regime's scene and oracle, built once"""
    cache = {}

    def get(regime, oracle):
        if regime not in cache:
            scene = M.scaled_scene(*regime)
            cache[regime] = (scene, oracle.OracleScene(scene.spec()))
        return cache[regime]

    return get


# ------------------------------------------------------------------ a. caller rays against the oracle
@regimes
def test_caller_rays_match_the_oracle(regime, scene_of, oracle):
    scene, orc = scene_of(regime, oracle)
    default = DeviceScene(scene.spec(), 0)
    # interior-slot corners of the 4-wide tree: read from the library's dump, for aiming only
    wide = M.wide_corner_boxes(default.wide_nodes(), DeviceScene.EMPTY_CHILD)
    o, d, family, aimed = M.ray_batch(regime, orc, oracle, wide)
    assert len(o) <= M.MAX_RAYS and set(family) == set(range(6))
    ref, _ = orc.trace(o, d, oracle.MODE_REFERENCE)
    r = _ref_arrays(ref)
    # left out, as in test_hard_rays: the oracle's closest hit is a triangle at distance NaN (which NaN
    # hit survives depends on the shape of the reference's own tree); the selection reads the oracle alone
    undefined = r["valid"] & (r["object"] >= 1) & np.isnan(r["distance"])
    assert undefined.sum() <= len(o) // 50
    sel = ~undefined
    o, d, r, aimed = o[sel], d[sel], _slice(r, sel), aimed[sel]
    # not vacuous: answers of both kinds, mesh hits, and rays on the box test's margin with both verdicts
    assert r["valid"].sum() >= 500 and (~r["valid"]).sum() >= 500
    assert (r["valid"] & (r["object"] >= 1)).sum() >= 500
    at = aimed >= 0
    tie, verdict = M.near_ties(M.leaf_boxes(*regime)[aimed[at]], o[at], d[at])
    print(f"{M.regime_id(regime)}: {len(o)} rays, {int(r['valid'].sum())} valid, "
          f"{int((r['valid'] & (r['object'] >= 1)).sum())} mesh hits, {int(undefined.sum())} left out, "
          f"{int(tie.sum())} near-ties ({int((tie & verdict).sum())} pass)")
    assert tie.sum() >= 500 and (tie & verdict).sum() >= 50 and (tie & ~verdict).sum() >= 50
    for flags in SCENE_FLAGS + ({"device_bvh": True},):
        ds = default if not flags else DeviceScene(scene.spec(), 0, **flags)
        _check_all(ds, o, d, r)
        hits, rec = query_closest(ds, o, d, records=True, reference_walk=True)
        _compare_ray_hits(hits, r)
        _compare_records(rec, r)
        assert np.array_equal(query_any(ds, o, d, reference_walk=True), r["valid"])
        _compare_records(trace_rays(ds, o, d), r)


@regimes
def test_integrated_rays_match_the_oracle(regime, scene_of, oracle):
    """integrate_rays on the oracle's own camera rays (rebuilt from its stream functions) against its
    per-sample records, as tests/test_gpu_integrate.py's Case does."""
    scene, orc = scene_of(regime, oracle)
    o, d, ids, wl = _oracle_rays(oracle, scene.spec().camera_location, TILE, H, W, SPP, SEED)
    ref = _staging_order(orc.render_samples(TILE, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8))
    assert (ref["flags"] & 1).sum() >= 3000
    for flags in ({}, {"device_bvh": True}):
        ds = DeviceScene(scene.spec(), 0, **flags)
        ph, info = integrate_rays(ds, o, d, SEED, stream_ids=ids, info=True, first_draw=2)
        _matches_oracle(ph, info, ref)
        ph, info = integrate_rays(ds, o, d, SEED, stream_ids=ids, info=True, wavelengths=wl, first_draw=3)
        _matches_oracle(ph, info, ref)


# ------------------------------------------------------------- b. the megakernel against the oracle
TREES = ({}, {"reference_bvh": True}, {"device_bvh": True}, {"device_sah": True}, {"wide_offsets": True})


def _pixel_centre_rays(oracle, camera):
    rays = [oracle.ray_for_pixel(camera, W, H, row, col, 0.5, 0.5) for row in range(H) for col in range(W)]
    return np.array([r[0] for r in rays]), np.array([r[1] for r in rays])


@regimes
def test_megakernel_matches_the_oracle(regime, scene_of, oracle):
    """At (1e-21, 0) the sphere pre-test's f32 squares are denormal (vr_device.h sphere_maybe32_lanes), but
    these two spheres are large: the band of wrong verdicts a purely relative margin leaves is a
    thousandth of the radius and no ray of this frame meets it (measured on an MI355X: the library
    without the absolute term passes here).  test_sphere_field_matches_the_oracle decides that margin.
    At (1e20, 0), (3e34, 0) and (1e36, 0) every path stays trapped on its surface to the recursion
    limit, through levels whose shading is NaN: where the kernels' forward product must discard what the
    reference discards (vr_render_kernel.h shade(), kPathCut)."""
    scene, orc = scene_of(regime, oracle)
    ref = orc.render_samples(TILE, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert (ref["flags"] & 1).sum() >= 3000
    o, d = _pixel_centre_rays(oracle, scene.spec().camera_location)
    centre = _ref_arrays(orc.trace(o, d, oracle.MODE_REFERENCE)[0])
    sphere_first = centre["valid"] & (centre["object"] == 0) & (centre["primitive"] >= 1)
    assert SPP * sphere_first.sum() >= 200
    for tree in TREES:
        ds = DeviceScene(scene.spec(), 0, **tree)
        for no_dist_cull in (True, False):
            ds.set_launch_flags(no_dist_cull=no_dist_cull)
            _decisions_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED), ref)


@pytest.mark.parametrize("S", [1.0, 1e-20, 1e-21, 1e-22], ids=lambda S: f"S{S:g}")
def test_sphere_field_matches_the_oracle(S, oracle):
    """The sphere pre-test where it can go wrong: 120 small spheres, so that r^2 is a few denormal
    steps of f32 at S = 1e-21 and less than one at 1e-22, and a frame's camera rays cross limbs by the
    hundred.  The guard restates the pre-test with its relative margin alone (tests/test_sphere_bound.py
    missed32, abs_term=0): at 1e-22 it would skip hundreds of the spheres the oracle hits first."""
    from test_sphere_bound import F32, missed32
    scene = M.sphere_field_scene(S, 0.0)
    orc = oracle.OracleScene(scene.spec())
    o, d, _, _ = _oracle_rays(oracle, scene.spec().camera_location, TILE, H, W, SPP, SEED)
    first = _ref_arrays(orc.trace(o, d, oracle.MODE_REFERENCE)[0])
    prims = scene.spec().objects[0].primitives
    on_sphere = first["valid"] & (first["primitive"] >= 1)
    assert on_sphere.sum() >= 1000
    c = np.array([p.vector for p in prims])[first["primitive"][on_sphere]]
    r = np.array([p.scalar for p in prims])[first["primitive"][on_sphere]]
    with np.errstate(under="ignore"):
        would_skip = missed32(o[on_sphere], d[on_sphere], c, r, abs_term=F32(0.0))
        assert not missed32(o[on_sphere], d[on_sphere], c, r).any()
    print(f"S = {S:g}: {int(on_sphere.sum())} samples hit a sphere first; the relative margin alone skips {int(would_skip.sum())}")
    if S == 1e-22:
        assert would_skip.sum() >= 100
    ref = orc.render_samples(TILE, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    ds = DeviceScene(scene.spec(), 0)
    for no_dist_cull in (True, False):
        ds.set_launch_flags(no_dist_cull=no_dist_cull)
        _decisions_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED), ref)


# --------------------------------------------------- c. instantiations and culls change no bit
MIXED = {(1.0, 1e3), (1.0, 3e4), (1e-3, 30.0)}     # some box tests in f32, some in f64
ALL_F32 = {(1.0, 0.0), (1e6, 0.0)}                  # the control and its scaled copy: f64 tests are rare


def _records(ds, stream, accumulate_twice=False, **kw):
    st = torch.zeros(H * W * 8, dtype=torch.float64, device="cuda")
    s = render_tile_device(ds, TILE, H, W, SPP, SEED, 0, st.data_ptr(), stream, **kw)
    if accumulate_twice:
        render_tile_device(ds, TILE, H, W, SPP, SEED, SPP, st.data_ptr(), stream, accumulate=True, **kw)
    torch.cuda.synchronize()
    return st.cpu().view(torch.int64), s


@regimes
def test_instantiations_and_culls_change_no_bit(regime, scene_of, oracle):
    scene, _ = scene_of(regime, oracle)
    ds = DeviceScene(scene.spec(), 0)
    stream = torch.cuda.current_stream().cuda_stream
    want, _ = _records(ds, stream)
    want2, _ = _records(ds, stream, accumulate_twice=True)
    assert (want.view(torch.float64)[: H * W * 4].view(-1, 4)[:, 3] > 0).all()  # the records were written
    assert not torch.equal(want, want2)
    for kw in ({"lone_walk": False}, {"coop": False}, {"coop": False, "stack16": False}, {"cull": False},
               {"dist_cull": False}):
        assert torch.equal(_records(ds, stream, **kw)[0], want), kw
        assert torch.equal(_records(ds, stream, accumulate_twice=True, **kw)[0], want2), kw
    got, s = _records(ds, stream, counters=True)
    assert torch.equal(got, want)
    c = {k: int(s[k]) for k in ("box_tests", "exact_box_tests", "node_visits", "triangle_tests", "rays", "samples")}
    print("magnitude counters", json.dumps({"regime": M.regime_id(regime), **c}))  # profiles/r11/magnitudes/counters.json
    # the emulated shares (tests/test_slab_bound.py) are per leaf box, not per walked box: no ratios
    if regime in MIXED:
        assert 0 < c["exact_box_tests"] < c["box_tests"]
    if regime not in ALL_F32:
        assert c["exact_box_tests"] > 0


# ----------------------------------------------------------------------------- d. ties at magnitude
@pytest.mark.parametrize("regime", [(1.0, 3e4), (1e-3, 30.0)], ids=M.regime_id)
@pytest.mark.parametrize("seed", [1, 2])
def test_ties_at_magnitude_decide_like_the_reference(seed, regime, oracle):
    """tests/test_gpu_ties.py's scene through the same map, culling on: cull_far carries E, which here
    is far larger than the spacing of f64 distances, and the copies' distances are exactly equal."""
    scene = M.tied_scene(seed, *regime)
    S = 64
    t = Tile(0, S, 0, S)
    ref = oracle.OracleScene(scene.spec()).render_samples(t, S, S, 6, seed=0x7135 + seed, mode=oracle.MODE_REFERENCE,
                                                          nthreads=8)
    assert (ref["flags"] & 1).sum() > 1000
    for tree in ({}, {"device_bvh": True}):
        _decisions_equal(render_samples(DeviceScene(scene.spec(), 0, **tree), t, S, S, 6, seed=0x7135 + seed), ref)
