"""vr_reproject_host (include/vanrijn_amd.h "Temporal reprojection") against the independent numpy reference of
tests/reproject_reference.py, bit for bit: a NaN must be a NaN in the same place and zeros must match in sign.
No GPU: the host form makes no device call, and every argument check of the device forms runs before the
first one.  The device forms are held to the same references in tests/test_gpu_reproject.py."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import reproject_cases as cases
from reproject_reference import MATCH_OBJECT, reproject_reference, same_bits
from vanrijn_amd import _native as N
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE
from vanrijn_amd.render import FeatureBuffers, ReprojectParams, motion_rows, reproject
from vanrijn_amd.scene import CameraPose

OK, INVALID, UNSUPPORTED = 0, -1, -7
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (37, 29)]
GUARD = 1234.5
ids = lambda s: "%dx%d" % s  # noqa: E731


def c_pose(pose):
    return CameraPose(pose.location, pose.right, pose.up, pose.forward, pose.film_distance)


def params(inp, flags=MATCH_OBJECT, cap=math.inf):
    p = ReprojectParams(inp.width, inp.height, c_pose(inp.pose), c_pose(inp.previous_pose), *cases.TOLERANCES, cap,
                        motion_count=inp.motion_count)
    p.flags = flags
    return p


def run_host(inp, flags=MATCH_OBJECT, cap=math.inf, in_place=False):
    """vr_reproject_host on copies of the inputs with 16 guard doubles after the output."""
    n = inp.width * inp.height
    state = np.concatenate([inp.state, np.full(16, GUARD)])
    out = state if in_place else np.full(8 * n + 16, GUARD)
    feat, pstate, pfeat = inp.features.copy(), inp.previous_state.copy(), inp.previous_features.copy()
    motion = None if inp.motion is None else np.ascontiguousarray(inp.motion).copy()
    p = params(inp, flags, cap)
    N.check(N.lib().vr_reproject_host(C.byref(p), state.ctypes.data, feat.ctypes.data, pstate.ctypes.data,
                                      pfeat.ctypes.data, motion.ctypes.data if motion is not None else None,
                                      out.ctypes.data))
    assert (out[8 * n:] == GUARD).all(), "guard values past the last pixel changed"
    assert feat.tobytes() == inp.features.tobytes() and pfeat.tobytes() == inp.previous_features.tobytes()
    assert same_bits(pstate, inp.previous_state)
    assert motion is None or same_bits(motion, inp.motion)
    if not in_place:
        assert same_bits(state[:8 * n], inp.state), "the input state was written"
    assert (out[4 * n:8 * n] == 0.0).all() and not np.signbit(out[4 * n:8 * n]).any(), "the bias half is not +0"
    return out[:8 * n]


def test_header_has_the_section_and_abi_stays_10():
    text = open(N.HERE + "/../include/vanrijn_amd.h").read()
    assert re.search(r"^#define\s+VR_HAS_REPROJECT\s+1\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_REPROJECT_MATCH_OBJECT\s+1u\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_ABI_VERSION\s+10\b", text, flags=re.M)
    assert N.lib().vr_abi_version() == 10
    assert C.sizeof(N.ReprojectParams) == 256 and C.sizeof(N.CameraPose) == 104


def test_default_params():
    a, b = c_pose(cases.POSES["rotation"][0])._c(), c_pose(cases.BASE)._c()
    p = N.ReprojectParams()
    assert N.lib().vr_reproject_default_params(640, 480, C.byref(a), C.byref(b), C.byref(p)) == OK
    assert (p.width, p.height, p.flags, p.motion_count) == (640, 480, MATCH_OBJECT, 0)
    assert (p.depth_tolerance, p.normal_tolerance, p.max_history_weight) == (0.05, 0.25, 64.0)
    assert bytes(p.pose) == bytes(a) and bytes(p.previous_pose) == bytes(b)
    for args in ((None, C.byref(b), C.byref(p)), (C.byref(a), None, C.byref(p)), (C.byref(a), C.byref(b), None)):
        assert N.lib().vr_reproject_default_params(1, 1, *args) == INVALID


@pytest.mark.parametrize("poses", list(cases.POSES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_pose_pairs_match_the_reference(shape, poses):
    inp = cases.inputs(*shape, poses)
    want, _ = cases.reference(*shape, poses)
    assert same_bits(run_host(inp), want)


@pytest.mark.parametrize("poses", cases.MOVED)
def test_the_moved_poses_do_find_history(poses):
    """A condition on the inputs, asserted on the reference alone: the camera steps of tests/reproject_cases.py
    leave history at half of the hit pixels or more at 37 x 29, so the comparisons above do exercise the
    gather.  No result of the library enters."""
    inp = cases.inputs(37, 29, poses)
    _, history = cases.reference(37, 29, poses)
    share = cases.history_share(inp, history)
    print(f"{poses}: history at {share:.3f} of the hit pixels")
    assert share >= 0.5


def test_a_previous_camera_turned_away_leaves_the_frame_as_it_is():
    inp = cases.inputs(37, 29, "turned_away")
    want, history = cases.reference(37, 29, "turned_away")
    assert not history.any()
    out = run_host(inp)
    assert same_bits(out, want) and same_bits(out[:4 * 37 * 29], inp.state[:4 * 37 * 29])


def test_a_third_of_the_image_leaves_the_frame():
    inp = cases.inputs(37, 29, "out_of_frame")
    _, history = cases.reference(37, 29, "out_of_frame")
    hit = inp.features["hits"] > 0
    columns_without = [x for x in range(37) if hit[:, x].any() and not history[:, x].any()]
    assert 8 <= len(columns_without) <= 16, columns_without  # about a third of 37 columns


@pytest.mark.parametrize("specials", cases.SPECIALS)
@pytest.mark.parametrize("poses", ["identical", "translation", "rotation"])
@pytest.mark.parametrize("shape", [(5, 5), (37, 29)], ids=ids)
def test_special_values_match_and_stay_contained(shape, poses, specials):
    inp = cases.inputs(*shape, poses, specials=specials)
    want, _ = cases.reference(*shape, poses, specials=specials)
    out = run_host(inp)
    assert same_bits(out, want)
    n = shape[0] * shape[1]
    cur_finite = np.isfinite(inp.state[:4 * n]).reshape(-1, 4).all(axis=1)
    assert np.isfinite(out[:4 * n].reshape(-1, 4)[cur_finite]).all(), "a special value of the history reached the output"


@pytest.mark.parametrize("specials", ["nan_sum", "absent_cur", "background", "mixed"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)], ids=ids)
def test_special_values_on_thin_images(shape, specials):
    for poses in ("identical", "translation"):
        inp = cases.inputs(*shape, poses, specials=specials)
        want, _ = cases.reference(*shape, poses, specials=specials)
        assert same_bits(run_host(inp), want)


def test_special_pixels_do_what_the_rule_says():
    """Read off the output directly, on the still view: an absent current pixel gives 8 zeros; an absent, NaN
    or infinite history pixel and NaN guides leave the current sums as they are."""
    n = 37 * 29
    for specials, changed in (("absent_cur", "state"), ("absent_prev", "previous_state"), ("nan_sum", "previous_state"),
                              ("inf_sum", "previous_state"), ("nan_cur_normal", "features"),
                              ("nan_prev_normal", "previous_features")):
        plain, inp = cases.inputs(37, 29, "identical"), cases.inputs(37, 29, "identical", specials=specials)
        a, b = getattr(plain, changed), getattr(inp, changed)
        if a.dtype == np.float64:
            at = np.nonzero((a[:4 * n].view(np.uint64) != b[:4 * n].view(np.uint64)).reshape(-1, 4).any(axis=1))[0]
        else:
            at = np.nonzero(np.frombuffer(a.tobytes(), np.uint8).reshape(n, 64) !=
                            np.frombuffer(b.tobytes(), np.uint8).reshape(n, 64))[0]
        at = np.unique(at)
        assert len(at) >= 3, specials
        out = run_host(inp)[:4 * n].reshape(n, 4)
        cur = inp.state[:4 * n].reshape(n, 4)
        if specials == "absent_cur":
            assert (out[at] == 0.0).all()
        else:
            assert same_bits(out[at], cur[at]), specials
        hit = inp.features["hits"].reshape(-1) > 0
        others = np.setdiff1d(np.nonzero(hit)[0], at)
        assert (out[others, 3] > cur[others, 3]).all(), "every other hit pixel of a still view has history"


def test_a_tap_of_weight_zero_is_never_read():
    inp, (row, column), tap = cases.zero_weight_tap()
    want, history = reproject_reference(37, 29, inp.pose, inp.previous_pose, *cases.TOLERANCES, math.inf, MATCH_OBJECT,
                                        inp.state, inp.features, inp.previous_state, inp.previous_features)
    prev = inp.previous_state[:4 * 37 * 29].reshape(29, 37, 4)
    assert np.isnan(prev[tap[0], tap[1], 1]) and history[row, column]
    out = run_host(inp)
    assert same_bits(out, want)
    rec = out[:4 * 37 * 29].reshape(29, 37, 4)[row, column]
    assert np.isfinite(rec).all() and rec[3] > inp.state[:4 * 37 * 29].reshape(29, 37, 4)[row, column, 3]


@pytest.mark.parametrize("specials", [None, "mixed"])
@pytest.mark.parametrize("poses", ["identical", "translation", "rotation", "out_of_frame"])
def test_without_match_object(poses, specials):
    inp = cases.inputs(37, 29, poses, specials=specials)
    want, _ = cases.reference(37, 29, poses, specials=specials, flags=0)
    assert same_bits(run_host(inp, flags=0), want)
    if specials == "mixed":  # "other_object": only the flag keeps those taps out
        assert not same_bits(want, cases.reference(37, 29, poses, specials=specials)[0]), "the flag changed nothing"


@pytest.mark.parametrize("cap", [math.inf, 8.0, 0.5])
@pytest.mark.parametrize("poses", ["identical", "translation", "film_distance"])
def test_caps(poses, cap):
    inp = cases.inputs(37, 29, poses, specials="mixed")
    want, history = cases.reference(37, 29, poses, specials="mixed", cap=cap)
    out = run_host(inp, cap=cap)
    assert same_bits(out, want)
    n = 37 * 29
    brought = (out[:4 * n].reshape(-1, 4)[:, 3] - inp.state[:4 * n].reshape(-1, 4)[:, 3])[history.reshape(-1)]
    assert (brought <= cap * (1 + 1e-14)).all() and (brought > 0).all()
    if cap == 0.5:
        assert np.allclose(brought, 0.5, rtol=1e-15, atol=0)  # every history weight here is 1 or more


@pytest.mark.parametrize("motion", [m for m in cases.MOTIONS if m != "none"])
@pytest.mark.parametrize("poses", ["identical", "translation"])
@pytest.mark.parametrize("shape", [(5, 5), (37, 29)], ids=ids)
def test_motion_rows(shape, poses, motion):
    inp = cases.inputs(*shape, poses, motion, specials="mixed" if shape == (37, 29) else None)
    want, history = cases.reference(*shape, poses, motion, specials="mixed" if shape == (37, 29) else None)
    assert same_bits(run_host(inp), want)
    if shape == (37, 29):
        assert cases.history_share(inp, history) >= 0.5


def test_motion_rows_are_needed_where_an_object_moved():
    """On the reference alone: with a still camera and sphere 0 moved, its pixels find more history with the
    row than without, and the identity rows change nothing."""
    inp = cases.inputs(37, 29, "identical", "translation")
    _, with_rows = cases.reference(37, 29, "identical", "translation")
    _, without = reproject_reference(37, 29, inp.pose, inp.previous_pose, *cases.TOLERANCES, math.inf, MATCH_OBJECT,
                                     inp.state, inp.features, inp.previous_state, inp.previous_features)
    on_sphere = inp.features["object"] == 0
    assert with_rows[on_sphere].sum() > without[on_sphere].sum()
    a, _ = cases.reference(37, 29, "translation", "identity")
    b, _ = cases.reference(37, 29, "translation", "none")
    assert same_bits(a, b)


@pytest.mark.parametrize("poses,motion,specials", [("identical", "none", None), ("translation", "none", "mixed"),
                                                   ("rotation", "rotation", "mixed"), ("out_of_frame", "none", None)])
def test_in_place_gives_the_same_bits(poses, motion, specials):
    inp = cases.inputs(37, 29, poses, motion, specials)
    want, _ = cases.reference(37, 29, poses, motion, specials)
    assert same_bits(run_host(inp, in_place=True), want)


def test_a_still_view_accumulates_exactly():
    """Equal poses, no cap, four successive calls: wherever a pixel's own tap passes the tests the output's sums
    are the element-wise sum of the sums halves, bit for bit (b = 1, r = 1: no rounding but the additions);
    elsewhere the output is the reference's."""
    w, h = 37, 29
    n = w * h
    first = cases.inputs(w, h, "identical", specials="mixed")
    history, hist_feat = first.previous_state, first.previous_features
    total = history[:4 * n].copy()
    for frame in range(4):
        inp = cases.inputs(w, h, "identical", specials="mixed", seed=10 + frame)
        inp = cases.Inputs(w, h, inp.pose, inp.previous_pose, inp.state, inp.features, history, hist_feat, None)
        want, got_history = reproject_reference(w, h, inp.pose, inp.previous_pose, *cases.TOLERANCES, math.inf, MATCH_OBJECT,
                                                inp.state, inp.features, history, hist_feat)
        out = run_host(inp)
        assert same_bits(out, want)
        mask = np.repeat(got_history.reshape(-1), 4)
        assert got_history.sum() > n // 3
        with np.errstate(all="ignore"):
            summed = inp.state[:4 * n] + total
        assert same_bits(out[:4 * n][mask], summed[mask])
        total = np.where(mask, summed, out[:4 * n])
        history, hist_feat = out.copy(), inp.features


def test_python_wrapper_host_form():
    inp = cases.inputs(37, 29, "translation", "translation")
    want, _ = cases.reference(37, 29, "translation", "translation")
    p = params(inp)
    p.motion_count = 0  # the wrapper counts the rows itself
    out = reproject(inp.state, FeatureBuffers(inp.features), inp.previous_state, inp.previous_features, p,
                    motion=inp.motion, host=True)
    assert same_bits(out, want) and p.motion_count == 0
    plain = cases.inputs(37, 29, "translation")
    out = reproject(plain.state, plain.features, plain.previous_state, plain.previous_features, params(plain), host=True)
    assert same_bits(out, cases.reference(37, 29, "translation")[0])
    with pytest.raises(ValueError):
        reproject(plain.state[:-8], plain.features, plain.previous_state, plain.previous_features, params(plain), host=True)


def test_motion_rows_helper():
    prev = [np.hstack([cases.rotation((0, 1, 0), 10.0), [[1.0], [2.0], [3.0]]]), np.eye(3, 4)]
    cur = [np.hstack([cases.rotation((1, 0, 0), -20.0), [[0.5], [0.0], [-1.0]]]), np.eye(3, 4)]
    rows = motion_rows(prev, cur)
    assert rows.shape == (2, 12) and np.array_equal(rows[1], np.eye(3, 4).reshape(12))
    base = np.array([0.3, -0.2, 0.9])
    now = cur[0][:, :3] @ base + cur[0][:, 3]
    before = prev[0][:, :3] @ base + prev[0][:, 3]
    m = rows[0].reshape(3, 4)
    assert np.allclose(m[:, :3] @ now + m[:, 3], before, rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        motion_rows(prev, cur[:1])


def _forms(p, a):
    """The three entry points with one set of arguments; no call reaches a device when a check fails."""
    L = N.lib()
    ref = C.byref(p) if p is not None else None
    common = (ref, a["state"], a["features"], a["previous_state"], a["previous_features"], a["motion"], a["out"])
    return [("host", L.vr_reproject_host(*common)), ("staged", L.vr_reproject(*common, 0)),
            ("device", L.vr_reproject_device(*common, 0, None))]


@pytest.fixture
def arrays():
    n = 16
    a = {"state": np.ones(8 * n), "features": np.zeros(n, dtype=PIXEL_FEATURES_DTYPE), "previous_state": np.ones(8 * n),
         "previous_features": np.zeros(n, dtype=PIXEL_FEATURES_DTYPE), "motion": np.tile(np.eye(3, 4).reshape(12), 2),
         "out": np.full(8 * n, GUARD)}
    return a, {k: v.ctypes.data for k, v in a.items()}


def _good(**fields):
    p = ReprojectParams(4, 4, c_pose(cases.POSES["rotation"][0]), c_pose(cases.BASE), motion_count=2)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def _expect(code, p, ptr, arrays, **replace):
    for name, rc in _forms(p, dict(ptr, **replace)):
        assert rc == code, (name, rc, N.lib().vr_last_error())
    assert (arrays["out"] == GUARD).all(), "written before the error"


def _bad_pose(**change):
    pose = c_pose(cases.BASE)._c()
    for k, v in change.items():
        if k == "film_distance":
            pose.film_distance = v
        else:
            setattr(pose, k, N.Vec3(*v))
    return pose


def test_every_listed_error(arrays):
    a, ptr = arrays
    _expect(INVALID, None, ptr, a)
    for missing in ("state", "features", "previous_state", "previous_features", "out"):
        _expect(INVALID, _good(), ptr, a, **{missing: None})
    _expect(INVALID, _good(), ptr, a, motion=None)              # motion_count 2 without rows
    _expect(INVALID, _good(), ptr, a, previous_state=ptr["out"])  # the output may not be the history
    for flags in (2, 4, 1 << 31, 3):
        _expect(INVALID, _good(flags=flags), ptr, a)
    for field in ("depth_tolerance", "normal_tolerance"):
        for bad in (0.0, -1.0, math.inf, math.nan):
            _expect(INVALID, _good(**{field: bad}), ptr, a)
    for bad in (0.0, -1.0, -math.inf, math.nan):
        _expect(INVALID, _good(max_history_weight=bad), ptr, a)
    bad_poses = [_bad_pose(location=(math.nan, 0, 0)), _bad_pose(right=(math.inf, 0, 0)), _bad_pose(up=(0, 1.001, 0)),
                 _bad_pose(forward=(1e-6, 0, 1)), _bad_pose(film_distance=1e-4), _bad_pose(film_distance=1e4),
                 _bad_pose(film_distance=math.nan), _bad_pose(right=(0, 0, 0))]
    for pose in bad_poses:
        for which in ("pose", "previous_pose"):
            _expect(INVALID, _good(**{which: pose}), ptr, a)
    _expect(UNSUPPORTED, _good(width=1 << 16, height=(1 << 15) + 1), ptr, a)
    _expect(UNSUPPORTED, _good(width=1 << 40, height=1 << 40), ptr, a)
    # the device form alone: alignment of every array, and the block-count limit of a thin image
    L = N.lib()
    p = _good()
    order = ("state", "features", "previous_state", "previous_features", "motion", "out")
    for name in order:
        args = [ptr[k] + (8 if k == name else 0) for k in order]
        assert L.vr_reproject_device(C.byref(p), *args, 0, None) == INVALID, name
    thin = _good(width=1, height=1 << 26)
    args = [ptr[k] for k in order]
    assert L.vr_reproject_device(C.byref(thin), *args, 0, None) == UNSUPPORTED
    assert L.vr_reproject(C.byref(thin), *args, 0) == UNSUPPORTED
    assert (a["out"] == GUARD).all()


def test_plus_infinity_is_a_cap_and_a_null_motion_is_fine(arrays):
    a, ptr = arrays
    p = _good(max_history_weight=math.inf, motion_count=0)
    args = dict(ptr, motion=None)
    assert N.lib().vr_reproject_host(C.byref(p), args["state"], args["features"], args["previous_state"],
                                     args["previous_features"], None, args["out"]) == OK
    assert (a["out"][:64].reshape(16, 4) == 1.0).all() and (a["out"][64:] == 0.0).all()  # background: the frame as it is


@pytest.mark.parametrize("shape", [(0, 4), (4, 0), (0, 0)])
def test_empty_image_is_ok_and_touches_nothing(arrays, shape):
    a, ptr = arrays
    p = _good(width=shape[0], height=shape[1])
    for name, rc in _forms(p, ptr):
        assert rc == OK, name
    assert (a["out"] == GUARD).all()
