"""The feature-buffer entry points (vr_render_features*, include/vanrijn_amd.h "Feature buffers"): the
record's layout in the header, ctypes and numpy, every argument check -- all of them run before the
first device call, so this passes on a machine without a GPU -- and the FeatureBuffers helpers.  The
pass itself is exercised in tests/test_gpu_features.py."""
import ctypes as C
import re

import numpy as np
import pytest

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE
from vanrijn_amd.render import FeatureBuffers, Tile, render_features, render_features_device

from test_integrate_args import _header, _header_fields, _ptr

OK, INVALID, UNSUPPORTED, HOST_ONLY = 0, -1, -7, -8
FILL = 0x5A
TWO32 = 1 << 32


@pytest.fixture(scope="module")
def host_scene():
    return scenes.bench_scene(scenes.displaced_mesh(6, [], 1, 0, 0.0, (1, 1, 1), (0, 0, 0))).device_scene(
        0, host_only=True)


@pytest.fixture
def outputs():
    """Records and state of a 4x4 tile filled with a guard byte."""
    return np.full(16 * 64, FILL, dtype=np.uint8), np.full(16 * 64, FILL, dtype=np.uint8)


def _params(tile=(0, 4, 0, 4), height=4, width=4, spp=1, accumulate=0, seed=7, first_sample=0):
    return N.RenderParams(N.TileC(*tile), height, width, spp, accumulate, seed, first_sample)


def _calls(scene, params, features, albedo):
    """Both entry points with one set of arguments: (name, return code, vr_last_error())."""
    L = N.lib()
    p = C.byref(params) if params is not None else None
    out = []
    for name, call in (("device", lambda: L.vr_render_features_device(scene, p, features, albedo, None)),
                       ("host", lambda: L.vr_render_features(scene, p, features, albedo))):
        rc = call()
        out.append((name, rc, L.vr_last_error()))
    return out


def _untouched(outputs):
    return all((a == FILL).all() for a in outputs)


def test_header_defines_vr_has_features_and_abi_stays_10():
    text = _header()
    assert re.search(r"^#define\s+VR_HAS_FEATURES\s+1\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_ABI_VERSION\s+10\b", text, flags=re.M)
    assert N.lib().vr_abi_version() == 10
    for fn in ("vr_render_features_device", "vr_render_features"):
        assert re.search(r"^int %s\(" % fn, text, flags=re.M), fn
        assert fn in N.SIGNATURES and hasattr(N.lib(), fn), fn


def test_record_layout_is_the_header():
    want = [("double", "normal_sum[3]"), ("double", "distance_sum"), ("double", "distance_min"), ("uint32_t", "hits"),
            ("uint32_t", "samples"), ("int32_t", "object"), ("int32_t", "reserved"), ("int64_t", "primitive")]
    assert _header_fields("vr_pixel_features") == want
    offsets = {"normal_sum": 0, "distance_sum": 24, "distance_min": 32, "hits": 40, "samples": 44, "object": 48,
               "reserved": 52, "primitive": 56}
    assert C.sizeof(N.PixelFeatures) == PIXEL_FEATURES_DTYPE.itemsize == 64
    ctypes_of = {"double": C.c_double, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64}
    numpy_of = {"double": "<f8", "int32_t": "<i4", "uint32_t": "<u4", "int64_t": "<i8"}
    assert [n for n, _ in N.PixelFeatures._fields_] == list(PIXEL_FEATURES_DTYPE.names) == list(offsets)
    for (ctype, decl), (name, ftype) in zip(want, N.PixelFeatures._fields_):
        assert decl.split("[")[0] == name
        assert ftype == (ctypes_of[ctype] * 3 if decl.endswith("[3]") else ctypes_of[ctype]), name
        assert getattr(N.PixelFeatures, name).offset == PIXEL_FEATURES_DTYPE.fields[name][1] == offsets[name], name
        sub = PIXEL_FEATURES_DTYPE.fields[name][0]
        assert sub.base == np.dtype(numpy_of[ctype]) and sub.shape == ((3,) if decl.endswith("[3]") else ()), name


def test_null_scene_or_params_is_invalid(host_scene, outputs):
    f, a = outputs
    for name, rc, msg in _calls(None, _params(), _ptr(f), _ptr(a)) + _calls(host_scene.handle, None, _ptr(f), _ptr(a)):
        assert rc == INVALID and len(msg) > 0, name
    assert _untouched(outputs)


def test_both_outputs_null_is_invalid(host_scene):
    for name, rc, msg in _calls(host_scene.handle, _params(), None, None):
        assert rc == INVALID and len(msg) > 0, name
    for name, rc, msg in _calls(host_scene.handle, _params(spp=0), None, None):  # before the empty-call rule
        assert rc == INVALID and len(msg) > 0, name


def test_accumulate_must_be_0_or_1(host_scene, outputs):
    f, a = outputs
    for acc in (2, 3, 1 << 31):
        for name, rc, msg in _calls(host_scene.handle, _params(accumulate=acc), _ptr(f), _ptr(a)):
            assert rc == INVALID and len(msg) > 0, (name, acc)
    assert _untouched(outputs)


def test_host_only_scene_is_refused(host_scene, outputs):
    """Valid arguments, either output alone or both, fresh or continuing: VR_ERROR_HOST_ONLY, which comes before
    the checks of the tile and the index space (vr_render_tile_device's order), and nothing is written."""
    f, a = outputs
    for features, albedo in ((_ptr(f), _ptr(a)), (_ptr(f), None), (None, _ptr(a))):
        for params in (_params(), _params(accumulate=1), _params(spp=0), _params(tile=(2, 2, 0, 4)),
                       _params(tile=(0, 5, 0, 4)), _params(first_sample=TWO32), _params(height=TWO32, width=2)):
            for name, rc, msg in _calls(host_scene.handle, params, features, albedo):
                assert rc == HOST_ONLY and len(msg) > 0, name
    assert _untouched(outputs)


def test_python_layer(host_scene):
    with pytest.raises(N.VrError) as e:
        render_features(host_scene, Tile(0, 4, 0, 4), 4, 4, 1, seed=7)
    assert e.value.code == HOST_ONLY
    with pytest.raises(N.VrError) as e:
        render_features_device(host_scene, Tile(0, 4, 0, 4), 4, 4, 1, 7, 0, None, None)
    assert e.value.code == INVALID
    wrong = FeatureBuffers(np.zeros((3, 4), dtype=PIXEL_FEATURES_DTYPE), np.zeros(8 * 12))
    with pytest.raises(ValueError):
        render_features(host_scene, Tile(0, 4, 0, 4), 4, 4, 1, seed=7, accumulate=wrong)
    wrong = FeatureBuffers(np.zeros((4, 4), dtype=PIXEL_FEATURES_DTYPE), np.zeros(8 * 12))
    with pytest.raises(ValueError):
        render_features(host_scene, Tile(0, 4, 0, 4), 4, 4, 1, seed=7, accumulate=wrong)


def test_feature_buffer_helpers():
    """normal() = normal_sum * (1 / hits) and 0 where hits == 0; depth() = distance_sum * (1 / hits);
    alpha() = hits / samples, on a hand-made record array."""
    r = np.zeros((2, 2), dtype=PIXEL_FEATURES_DTYPE)
    r["samples"] = 3
    r[0, 0] = ((0.3, -1.5, 2.7), 7.5, 2.0, 3, 3, 1, 0, 40)
    r[0, 1] = ((0.0, 1.0, 0.0), 4.25, 4.25, 1, 3, 0, 0, 2)
    r[1, 0] = ((np.nan, 0.5, 0.5), 6.0, 3.0, 2, 3, 2, 0, 0)
    r[1, 1] = ((0.0, 0.0, 0.0), 0.0, 0.0, 0, 3, -1, 0, -1)
    fb = FeatureBuffers(r)
    assert fb.albedo_state is None
    third = 1.0 / 3.0
    n = fb.normal()
    assert n.shape == (2, 2, 3)
    assert n[0, 0].tolist() == [0.3 * third, -1.5 * third, 2.7 * third]
    assert n[0, 1].tolist() == [0.0, 1.0, 0.0]
    assert np.isnan(n[1, 0, 0]) and n[1, 0, 1:].tolist() == [0.25, 0.25]
    assert n[1, 1].tolist() == [0.0, 0.0, 0.0]
    d = fb.depth()
    assert d.shape == (2, 2)
    assert d[0, 0] == 7.5 * third and d[0, 1] == 4.25 and d[1, 0] == 3.0 and np.isnan(d[1, 1])
    assert fb.alpha().tolist() == [[1.0, 1.0 / 3.0], [2.0 / 3.0, 0.0]]
