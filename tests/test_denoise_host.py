"""vr_denoise_host (include/vanrijn_amd.h "Denoiser") against the independent numpy reference of
tests/denoise_reference.py, bit for bit: a NaN must be a NaN in the same place and zeros must match in sign.
No GPU: the host form makes no device call, and every argument check of the device forms runs before the
first one.  The device forms are held to the same references in tests/test_gpu_denoise.py."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import denoise_cases as cases
from denoise_reference import DEMODULATE, MATCH_OBJECT, exp_tab, same_bits
from vanrijn_amd import _native as N
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE
from vanrijn_amd.render import DenoiseParams, FeatureBuffers, denoise, denoise_workspace_bytes

OK, INVALID, UNSUPPORTED = 0, -1, -7
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (37, 29)]
KINDS = ["nan_colour", "inf_colour", "nan_normal", "zero_depth", "background", "absent"]
GUARD = 1234.5


def params(width, height, iterations, flags=0):
    p = DenoiseParams(width, height, iterations, *cases.SIGMAS)
    p.flags = flags
    return p


def run_host(inp, iterations, flags=0, in_place=False):
    """vr_denoise_host on a copy of the inputs with 16 guard doubles after the output."""
    n = inp.width * inp.height
    state = np.concatenate([inp.state, np.full(16, GUARD)])
    out = state if in_place else np.full(8 * n + 16, GUARD)
    albedo = inp.albedo_state.copy()
    feat = inp.features.copy()
    p = params(inp.width, inp.height, iterations, flags)
    N.check(N.lib().vr_denoise_host(C.byref(p), state.ctypes.data, feat.ctypes.data,
                                    albedo.ctypes.data if flags & DEMODULATE else None, out.ctypes.data))
    assert (out[8 * n:] == GUARD).all(), "guard values past the last pixel changed"
    assert feat.tobytes() == inp.features.tobytes() and same_bits(albedo, inp.albedo_state)
    if not in_place:
        assert same_bits(state[:8 * n], inp.state), "the input state was written"
    return out[:8 * n]


def check_contained(inp, out):
    """Everything outside the pixels whose own colour is NaN or infinite comes out finite."""
    n = inp.width * inp.height
    rec = out[:4 * n].reshape(inp.height, inp.width, 4)
    assert np.isfinite(rec[~inp.nonfinite]).all()
    assert (out[4 * n:] == 0.0).all() and not np.signbit(out[4 * n:]).any()


def test_header_has_the_section_and_abi_stays_10():
    text = open(N.HERE + "/../include/vanrijn_amd.h").read()
    assert re.search(r"^#define\s+VR_HAS_DENOISE\s+1\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_ABI_VERSION\s+10\b", text, flags=re.M)
    assert N.lib().vr_abi_version() == 10
    assert C.sizeof(N.DenoiseParams) == 48
    assert N.DENOISE_ALBEDO_FLOOR == 1.0 / 1024.0


def test_default_params_and_workspace():
    p = N.DenoiseParams()
    assert N.lib().vr_denoise_default_params(640, 480, C.byref(p)) == OK
    assert (p.width, p.height, p.iterations, p.flags, p.sigma_normal, p.sigma_depth) == (640, 480, 5, 0, 0.5, 0.1)
    assert p.sigma_colour > 0 and math.isfinite(p.sigma_colour)
    assert N.lib().vr_denoise_default_params(1, 1, None) == INVALID
    assert 0 < denoise_workspace_bytes(DenoiseParams(640, 480)) <= 128 * 640 * 480
    assert denoise_workspace_bytes(DenoiseParams(0, 480)) == 0
    out = C.c_uint64()
    assert N.lib().vr_denoise_workspace_bytes(None, C.byref(out)) == INVALID
    assert N.lib().vr_denoise_workspace_bytes(C.byref(DenoiseParams(1 << 16, (1 << 15) + 1)), C.byref(out)) == UNSUPPORTED


def test_reference_exp_is_the_table():
    x = np.array([0.0, -0.0, -1.0, -745.0, -2000.0, -np.inf, np.nan])
    y = exp_tab(x)
    assert y[0] == 1.0 and y[1] == 1.0 and abs(y[2] - math.exp(-1.0)) < 1e-15
    assert y[4] == 0.0 and y[5] == 0.0 and not np.signbit(y[4:6]).any() and np.isnan(y[6])


@pytest.mark.parametrize("iterations", [1, 3, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_plain_images_match_the_reference(shape, iterations):
    inp = cases.inputs(*shape)
    out = run_host(inp, iterations)
    assert same_bits(out, cases.reference(*shape, iterations))
    check_contained(inp, out)
    n = shape[0] * shape[1]
    assert (out[:4 * n].reshape(-1, 4)[:, 3] == 1.0).all()


def test_steps_past_the_image_leave_the_centre_tap():
    """At 8 iterations on 5x5 the steps 8 .. 128 reach no other pixel: iterations 4 .. 7 change nothing that
    a centre-only fold does not (c * w * (1 / w) may round), and the reference agrees bit for bit."""
    inp = cases.inputs(5, 5)
    assert same_bits(run_host(inp, 8), cases.reference(5, 5, 8))
    a, b = run_host(inp, 4), run_host(inp, 8)
    assert np.allclose(a, b, rtol=1e-14, atol=0)


@pytest.mark.parametrize("iterations", [1, 3, 8])
@pytest.mark.parametrize("specials", ["a", "b"])
@pytest.mark.parametrize("shape", [(5, 5), (37, 29)], ids=lambda s: "%dx%d" % s)
def test_special_values_match_and_stay_contained(shape, specials, iterations):
    inp = cases.inputs(*shape, specials=specials)
    out = run_host(inp, iterations)
    assert same_bits(out, cases.reference(*shape, iterations, specials=specials))
    check_contained(inp, out)


def test_special_pixels_pass_through_or_vanish():
    """What the rule says of each special centre, read off the output directly."""
    inp = cases.inputs(37, 29, specials="a")
    out = run_host(inp, 3)[:4 * 37 * 29].reshape(29, 37, 4)
    src = inp.state[:4 * 37 * 29].reshape(29, 37, 4)
    with np.errstate(all="ignore"):
        mean = src[..., :3] * (1.0 / src[..., 3:])
    assert np.isnan(out[0, 0, 1]) and out[0, 0, 0] == mean[0, 0, 0]       # NaN colour: unchanged
    assert np.isinf(out[0, 36, 0]) and out[0, 36, 1] == mean[0, 36, 1]    # +inf colour: unchanged
    assert np.array_equal(out[28, 0, :3], src[28, 0, :3] * (1.0 / src[28, 0, 3]))    # NaN normals: unchanged
    assert np.array_equal(out[28, 36, :3], src[28, 36, :3] * (1.0 / src[28, 36, 3]))  # mean depth 0: unchanged
    inp = cases.inputs(37, 29, specials="b")
    out = run_host(inp, 3)[:4 * 37 * 29].reshape(29, 37, 4)
    assert (out[0, 36] == 0.0).all() and (out[28, 36] == 0.0).all()  # absent stays absent: weight 0 too
    assert (out[..., 3] == 1.0).sum() == 37 * 29 - 4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)], ids=lambda s: "%dx%d" % s)
def test_special_values_on_thin_images(shape, kind):
    inp = cases.inputs(*shape, specials=kind)
    out = run_host(inp, 3)
    assert same_bits(out, cases.reference(*shape, 3, specials=kind))
    check_contained(inp, out)


@pytest.mark.parametrize("specials", [None, "a", "b"])
@pytest.mark.parametrize("flags", [MATCH_OBJECT, DEMODULATE, MATCH_OBJECT | DEMODULATE])
def test_flags_match_the_reference(flags, specials):
    inp = cases.inputs(37, 29, specials=specials)
    out = run_host(inp, 3, flags)
    assert same_bits(out, cases.reference(37, 29, 3, flags, specials=specials))
    check_contained(inp, out)
    assert not same_bits(out, cases.reference(37, 29, 3, 0, specials=specials)), "the flag changed nothing"


def test_demodulate_inputs_straddle_the_floor():
    inp = cases.inputs(37, 29)
    a = inp.albedo_state[:4 * 37 * 29].reshape(-1, 4)
    with np.errstate(all="ignore"):
        mean = np.where(a[:, 3:] != 0, a[:, :3] / a[:, 3:], 0.0)
    assert (mean > N.DENOISE_ALBEDO_FLOOR).any() and ((mean > 0) & (mean <= N.DENOISE_ALBEDO_FLOOR)).any()
    assert (a[:, 3] == 0).any() and (mean == 0).any()


@pytest.mark.parametrize("flags", [0, MATCH_OBJECT | DEMODULATE])
@pytest.mark.parametrize("specials", [None, "a", "b"])
def test_in_place_gives_the_same_bits(specials, flags):
    inp = cases.inputs(37, 29, specials=specials)
    assert same_bits(run_host(inp, 3, flags, in_place=True), cases.reference(37, 29, 3, flags, specials=specials))


def test_python_wrapper_host_form():
    inp = cases.inputs(37, 29)
    fb = FeatureBuffers(inp.features, inp.albedo_state)
    p = params(37, 29, 3, DEMODULATE)
    out = denoise(inp.state, fb, params=p, host=True)
    assert same_bits(out, cases.reference(37, 29, 3, DEMODULATE))
    out = denoise(inp.state, inp.features, params=params(37, 29, 3), host=True)
    assert same_bits(out, cases.reference(37, 29, 3))
    assert denoise(inp.state, fb, host=True).shape == (8 * 37 * 29,)  # the defaults at the records' shape
    with pytest.raises(ValueError):
        denoise(inp.state[:-8], fb, params=p, host=True)


def _forms(p, state, features, albedo, out, workspace):
    """The three entry points with one set of arguments; no call reaches a device when a check fails."""
    L = N.lib()
    ref = C.byref(p) if p is not None else None
    return [("host", L.vr_denoise_host(ref, state, features, albedo, out)),
            ("staged", L.vr_denoise(ref, state, features, albedo, out, 0)),
            ("device", L.vr_denoise_device(ref, state, features, albedo, out, workspace, 0, None)),
            ("stage", L.vr_denoise_stage_device(ref, 0, state, features, albedo, out, workspace, 0, None))]


@pytest.fixture
def arrays():
    n = 16
    a = {"state": np.ones(8 * n), "features": np.zeros(n, dtype=PIXEL_FEATURES_DTYPE), "albedo": np.ones(8 * n),
         "out": np.full(8 * n, GUARD), "workspace": np.full(16 * n, GUARD)}
    return a, {k: v.ctypes.data for k, v in a.items()}


def _expect(code, p, ptr, arrays, **replace):
    args = dict(ptr, **replace)
    for name, rc in _forms(p, args["state"], args["features"], args["albedo"], args["out"], args["workspace"]):
        assert rc == code, (name, rc, N.lib().vr_last_error())
    assert (arrays["out"] == GUARD).all() and (arrays["workspace"] == GUARD).all(), "written before the error"


def test_every_listed_error(arrays):
    a, ptr = arrays
    good = lambda **kw: _set(params(4, 4, 2), **kw)  # noqa: E731
    _expect(INVALID, None, ptr, a)
    for missing in ("state", "features", "out"):
        _expect(INVALID, good(), ptr, a, **{missing: None})
    for it in (0, 9, 1 << 31):
        _expect(INVALID, good(iterations=it), ptr, a)
    for flags in (16, 1 << 31, 4 | 8):
        _expect(INVALID, good(flags=flags), ptr, a)
    _expect(INVALID, good(flags=DEMODULATE), ptr, a, albedo=None)
    for field in ("sigma_colour", "sigma_normal", "sigma_depth"):
        for bad in (0.0, -1.0, math.inf, math.nan):
            _expect(INVALID, good(**{field: bad}), ptr, a)
    _expect(UNSUPPORTED, good(width=1 << 16, height=(1 << 15) + 1), ptr, a)
    _expect(UNSUPPORTED, good(width=1 << 40, height=1 << 40), ptr, a)
    # the device form: a null workspace with n > 0, and alignment
    L = N.lib()
    p = good()
    assert L.vr_denoise_device(C.byref(p), ptr["state"], ptr["features"], None, ptr["out"], None, 0, None) == INVALID
    assert L.vr_denoise_device(C.byref(p), ptr["state"] + 8, ptr["features"], None, ptr["out"], ptr["workspace"], 0,
                               None) == INVALID
    assert L.vr_denoise_stage_device(C.byref(p), 4, ptr["state"], ptr["features"], None, ptr["out"], ptr["workspace"],
                                     0, None) == INVALID
    assert (a["out"] == GUARD).all() and (a["workspace"] == GUARD).all()


def _set(p, **fields):
    for k, v in fields.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("shape", [(0, 4), (4, 0), (0, 0)])
def test_empty_image_is_ok_and_touches_nothing(arrays, shape):
    a, ptr = arrays
    p = params(*shape, 2)
    for name, rc in _forms(p, ptr["state"], ptr["features"], None, ptr["out"], None):
        assert rc == OK, name
    assert (a["out"] == GUARD).all()


def test_region_isolation_with_match_object():
    """A property that does not go through the reference.  With VR_DENOISE_MATCH_OBJECT on a two-region
    image a pixel only ever mixes with pixels of its own region, so every output channel lies within
    [min, max] of the input channel over that region.  The interval is widened by 8 ulp of the larger
    bound: the output is a convex combination of at most 25 terms per iteration, every operation is rounded
    once and the values are positive, so an iteration can leave the interval by a few ulp at most."""
    w, h = 37, 29
    inp = cases.inputs(w, h, seed=2, regions=2)
    state = inp.state.copy()
    rec = state[:4 * w * h].reshape(h, w, 4)
    rec[..., 0] = np.abs(rec[..., 0])  # positive values
    region = inp.features["object"]
    assert sorted(np.unique(region)) == [1, 2]
    rec[..., :3] += np.where(region == 2, 5.0, 0.0)[..., None] * rec[..., 3:]  # the regions' ranges are disjoint
    p = params(w, h, 5, MATCH_OBJECT)
    p.sigma_colour, p.sigma_normal, p.sigma_depth = 50.0, 50.0, 50.0  # nothing else keeps the regions apart
    out = np.zeros(8 * w * h)
    N.check(N.lib().vr_denoise_host(C.byref(p), state.ctypes.data, inp.features.ctypes.data, None, out.ctypes.data))
    mean_in = rec[..., :3] * (1.0 / rec[..., 3:])
    mean_out = out[:4 * w * h].reshape(h, w, 4)[..., :3]
    for r in (1, 2):
        for k in range(3):
            lo, hi = mean_in[region == r, k].min(), mean_in[region == r, k].max()
            slack = 8 * np.spacing(max(abs(lo), abs(hi)))
            got = mean_out[region == r, k]
            assert lo - slack <= got.min() and got.max() <= hi + slack, (r, k)
            assert got.max() - got.min() < 0.5 * (hi - lo)  # and it did smooth
    # without the flag the same sigmas mix the regions
    p.flags = 0
    N.check(N.lib().vr_denoise_host(C.byref(p), state.ctypes.data, inp.features.ctypes.data, None, out.ctypes.data))
    assert out[:4 * w * h].reshape(h, w, 4)[region == 1, 0].max() > mean_in[region == 1, 0].max() + 0.1
