"""The integrate entry points (vr_integrate_rays*, include/vanrijn_amd.h): every argument check runs
before the first device call, so all of this passes on a machine without a GPU.  The integrators
themselves are exercised in tests/test_gpu_integrate.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import PATH_INFO_DTYPE, PHOTON_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, HOST_ONLY = 0, -1, -7, -8


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _header():
    return open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()


def _header_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        out += [(words[0], w) for w in words[1:]]
    return out


@pytest.fixture(scope="module")
def host_scene():
    return scenes.bench_scene(scenes.displaced_mesh(6, [], 1, 0, 0.0, (1, 1, 1), (0, 0, 0))).device_scene(
        0, host_only=True)


@pytest.fixture
def rays():
    o = np.zeros((4, 3))
    d = np.tile([0.0, 0.0, 1.0], (4, 1))
    return o, d, np.full(4, -1.0, dtype=[("wavelength", "<f8"), ("intensity", "<f8")])


def _params(**kw):
    return N.IntegrateParams(kw.get("seed", 7), kw.get("first_stream", 0), kw.get("sample", 0),
                             kw.get("first_draw", 0), kw.get("flags", 0))


def _calls(scene, n, o, d, params, photons, wl=None, ids=None, info=None):
    """Both entry points with one set of arguments: (name, return code)."""
    L = N.lib()
    p = C.byref(params) if params is not None else None
    return [("device", L.vr_integrate_rays_device(scene, n, o, d, wl, ids, p, photons, info, None)),
            ("host", L.vr_integrate_rays(scene, n, o, d, wl, ids, p, photons, info))]


def test_struct_layouts_are_the_header():
    assert C.sizeof(N.Photon) == PHOTON_DTYPE.itemsize == 16
    assert C.sizeof(N.PathInfo) == PATH_INFO_DTYPE.itemsize == 8
    assert C.sizeof(N.IntegrateParams) == 32
    assert (N.Photon.wavelength.offset, N.Photon.intensity.offset) == (0, 8)
    assert (N.PathInfo.bounces.offset, N.PathInfo.flags.offset) == (0, 4)
    assert [getattr(N.IntegrateParams, f).offset for f, _ in N.IntegrateParams._fields_] == [0, 8, 16, 24, 28]
    for name in PHOTON_DTYPE.names:
        assert getattr(N.Photon, name).offset == PHOTON_DTYPE.fields[name][1], name
    for name in PATH_INFO_DTYPE.names:
        assert getattr(N.PathInfo, name).offset == PATH_INFO_DTYPE.fields[name][1], name
    assert _header_fields("vr_photon") == [("double", "wavelength"), ("double", "intensity")]
    assert _header_fields("vr_path_info") == [("int32_t", "bounces"), ("int32_t", "flags")]
    assert _header_fields("vr_integrate_params") == [("uint64_t", "seed"), ("uint64_t", "first_stream"),
                                                     ("uint64_t", "sample"), ("uint32_t", "first_draw"),
                                                     ("uint32_t", "flags")]
    ctypes_of = {"double": C.c_double, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    for struct, cls in (("vr_photon", N.Photon), ("vr_path_info", N.PathInfo),
                        ("vr_integrate_params", N.IntegrateParams)):
        assert [(n, t) for n, t in cls._fields_] == [(n, ctypes_of[t]) for t, n in _header_fields(struct)], struct


def test_header_defines_vr_has_integrate_and_abi_stays_10():
    text = _header()
    assert re.search(r"^#define\s+VR_HAS_INTEGRATE\s+1\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_ABI_VERSION\s+10\b", text, flags=re.M)
    assert N.lib().vr_abi_version() == 10
    for fn in ("vr_integrate_rays_device", "vr_integrate_rays", "vr_accumulate_photons_device",
               "vr_camera_rays_device"):
        assert re.search(r"^int %s\(" % fn, text, flags=re.M), fn
        assert fn in N.SIGNATURES and hasattr(N.lib(), fn), fn


def test_zero_rays_is_ok_and_needs_no_arrays(host_scene):
    for name, rc in _calls(host_scene.handle, 0, None, None, _params(), None):
        assert rc == OK, name


def test_null_scene_or_params_is_invalid(host_scene, rays):
    o, d, ph = rays
    for n in (0, 4):
        for name, rc in _calls(None, n, _ptr(o), _ptr(d), _params(), _ptr(ph)):
            assert rc == INVALID, (name, n)
        for name, rc in _calls(host_scene.handle, n, _ptr(o), _ptr(d), None, _ptr(ph)):
            assert rc == INVALID, (name, n)
    assert len(N.lib().vr_last_error()) > 0


def test_null_required_array_is_invalid(host_scene, rays):
    o, d, ph = rays
    full = (_ptr(o), _ptr(d), _ptr(ph))
    for missing in range(3):
        a = [None if k == missing else p for k, p in enumerate(full)]
        for name, rc in _calls(host_scene.handle, 4, a[0], a[1], _params(), a[2]):
            assert rc == INVALID, (name, missing)
    # the optional arrays may be null: the next check (the host-only scene) answers
    for name, rc in _calls(host_scene.handle, 4, *full[:2], _params(), full[2], None, None, None):
        assert rc == HOST_ONLY, name


def test_unknown_flag_bit_is_invalid(host_scene, rays):
    o, d, ph = rays
    for flags in (N.QUERY_REFERENCE_WALK, 3, 4, 8, 1 << 31, 1 | 4):
        for n in (0, 4):
            for name, rc in _calls(host_scene.handle, n, _ptr(o), _ptr(d), _params(flags=flags), _ptr(ph)):
                assert rc == INVALID, (name, flags, n)


def test_host_only_scene_is_refused(host_scene, rays):
    o, d, ph = rays
    wl = np.full(4, 500.0)
    ids = np.arange(4, dtype=np.uint64)
    info = np.full(4, -1, dtype=PATH_INFO_DTYPE)
    for flags in (0, N.QUERY_NORMALIZE):
        for name, rc in _calls(host_scene.handle, 4, _ptr(o), _ptr(d), _params(flags=flags, first_draw=3), _ptr(ph),
                               _ptr(wl), _ptr(ids), _ptr(info)):
            assert rc == HOST_ONLY, (name, flags)
    assert (ph["wavelength"] == -1.0).all() and (ph["intensity"] == -1.0).all()  # nothing was written
    assert (info["bounces"] == -1).all() and (info["flags"] == -1).all()


def test_index_space_limits(host_scene, rays):
    """first_stream + n > 2^32 or sample >= 2^32: VR_ERROR_UNSUPPORTED, decided without a sum that wraps
    (a wrapped first_stream + n would look small); inside the limits the next check (host-only) answers."""
    o, d, ph = rays
    two32, top = 1 << 32, (1 << 64) - 1
    cases = [(two32 - 4, 0, HOST_ONLY), (two32 - 3, 0, UNSUPPORTED), (two32, 0, UNSUPPORTED),
             (top, 0, UNSUPPORTED), (top - 3, 0, UNSUPPORTED), (top - 2, 0, UNSUPPORTED),
             (0, two32 - 1, HOST_ONLY), (0, two32, UNSUPPORTED), (0, top, UNSUPPORTED),
             (two32 - 4, two32 - 1, HOST_ONLY)]
    for first_stream, sample, want in cases:
        for name, rc in _calls(host_scene.handle, 4, _ptr(o), _ptr(d),
                               _params(first_stream=first_stream, sample=sample), _ptr(ph)):
            assert rc == want, (name, first_stream, sample)
    # n == 0 touches nothing, whatever the indices
    for name, rc in _calls(host_scene.handle, 0, None, None, _params(first_stream=top, sample=top), None):
        assert rc == OK, name
    assert (ph["wavelength"] == -1.0).all()


def test_accumulate_and_camera_rays_argument_checks(host_scene):
    L = N.lib()
    assert L.vr_accumulate_photons_device(None, None, 0, 4, 0, 0, None) == OK  # no pixels: nothing to do
    buf = np.zeros(16)
    assert L.vr_accumulate_photons_device(None, _ptr(buf), 1, 1, 0, 0, None) == INVALID
    assert L.vr_accumulate_photons_device(_ptr(buf), None, 1, 1, 0, 0, None) == INVALID
    p = N.RenderParams(N.TileC(0, 4, 0, 4), 4, 4, 1, 0, 7, 0)
    assert L.vr_camera_rays_device(None, C.byref(p), _ptr(buf), _ptr(buf), _ptr(buf), None) == INVALID
    assert L.vr_camera_rays_device(host_scene.handle, None, _ptr(buf), _ptr(buf), _ptr(buf), None) == INVALID
    assert L.vr_camera_rays_device(host_scene.handle, C.byref(p), _ptr(buf), _ptr(buf), _ptr(buf), None) == HOST_ONLY
    assert not buf.any()


def test_python_layer_raises_host_only(host_scene, rays):
    from vanrijn_amd import integrate_rays
    o, d, _ = rays
    for call in (lambda: integrate_rays(host_scene, o, d, seed=7),
                 lambda: integrate_rays(host_scene, o, d, seed=7, wavelengths=np.full(4, 500.0),
                                        stream_ids=np.arange(4), first_draw=3, normalize=True, info=True)):
        with pytest.raises(N.VrError) as e:
            call()
        assert e.value.code == HOST_ONLY
    with pytest.raises(ValueError):
        integrate_rays(host_scene, o, d, seed=7, wavelengths=np.zeros(3))
