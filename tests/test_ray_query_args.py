"""Ray query entry points (vr_query_*, include/vanrijn_amd.h): every argument check runs before the
first device call, so all of this passes on a machine without a GPU.  The queries themselves are
exercised in tests/test_gpu_ray_query.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import RAY_HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, HOST_ONLY = 0, -1, -8


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host_scene():
    return scenes.bench_scene(scenes.displaced_mesh(6, [], 1, 0, 0.0, (1, 1, 1), (0, 0, 0))).device_scene(
        0, host_only=True)


@pytest.fixture
def rays():
    o = np.zeros((4, 3))
    d = np.tile([0.0, 0.0, 1.0], (4, 1))
    return o, d, np.zeros(4, dtype=RAY_HIT_DTYPE), np.zeros(4, dtype=np.uint8)


def _calls(scene, n, o, d, flags, hits, any_hit):
    """The four entry points with one set of arguments: (name, return code)."""
    L = N.lib()
    return [("closest_device", L.vr_query_closest_device(scene, n, o, d, flags, hits, None, None)),
            ("any_device", L.vr_query_any_device(scene, n, o, d, flags, any_hit, None)),
            ("closest", L.vr_query_closest(scene, n, o, d, flags, hits, None)),
            ("any", L.vr_query_any(scene, n, o, d, flags, any_hit))]


def test_ray_hit_layout_is_the_dtype():
    assert C.sizeof(N.RayHit) == RAY_HIT_DTYPE.itemsize == 32
    for name in ("distance", "primitive", "object", "valid"):
        assert getattr(N.RayHit, name).offset == RAY_HIT_DTYPE.fields[name][1], name
        assert getattr(N.RayHit, name).size == RAY_HIT_DTYPE.fields[name][0].itemsize, name
    assert (N.RayHit.distance.offset, N.RayHit.primitive.offset, N.RayHit.object.offset,
            N.RayHit.valid.offset) == (0, 8, 16, 20)
    # the header's struct, field for field
    text = open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()
    body = re.search(r"typedef struct vr_ray_hit \{(.*?)\} vr_ray_hit;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [tuple(f.split()) for f in body.split(";") if f.strip()]
    assert fields == [("double", "distance"), ("int64_t", "primitive"), ("int32_t", "object"), ("int32_t", "valid"),
                      ("uint64_t", "reserved")]


def test_zero_rays_is_ok_and_needs_no_arrays(host_scene):
    for name, rc in _calls(host_scene.handle, 0, None, None, 0, None, None):
        assert rc == OK, name


def test_null_scene_is_invalid(rays):
    o, d, hits, hit = rays
    for n in (0, 4):
        for name, rc in _calls(None, n, _ptr(o), _ptr(d), 0, _ptr(hits), _ptr(hit)):
            assert rc == INVALID, (name, n)
    assert len(N.lib().vr_last_error()) > 0


def test_null_array_is_invalid(host_scene, rays):
    o, d, hits, hit = rays
    full = (_ptr(o), _ptr(d), _ptr(hits), _ptr(hit))
    for missing in range(4):
        a = [None if k == missing else p for k, p in enumerate(full)]
        for name, rc in _calls(host_scene.handle, 4, a[0], a[1], 0, a[2], a[3]):
            uses = (missing < 2 or (missing == 2) == name.startswith("closest"))
            assert rc == (INVALID if uses else HOST_ONLY), (name, missing)


def test_unknown_flag_bit_is_invalid(host_scene, rays):
    o, d, hits, hit = rays
    for flags in (4, 8, 1 << 31, 3 | 4):
        for n in (0, 4):
            for name, rc in _calls(host_scene.handle, n, _ptr(o), _ptr(d), flags, _ptr(hits), _ptr(hit)):
                assert rc == INVALID, (name, flags, n)


def test_host_only_scene_is_refused_by_all_four(host_scene, rays):
    o, d, hits, hit = rays
    for flags in (0, N.QUERY_NORMALIZE, N.QUERY_REFERENCE_WALK, 3):
        for name, rc in _calls(host_scene.handle, 4, _ptr(o), _ptr(d), flags, _ptr(hits), _ptr(hit)):
            assert rc == HOST_ONLY, (name, flags)
    assert not hits["valid"].any() and not hit.any()  # nothing was written


def test_python_layer_raises_host_only(host_scene, rays):
    from vanrijn_amd.render import query_any, query_closest
    o, d, _, _ = rays
    for call in (lambda: query_closest(host_scene, o, d), lambda: query_any(host_scene, o, d),
                 lambda: query_closest(host_scene, o, d, records=True, normalize=True, reference_walk=True)):
        with pytest.raises(N.VrError) as e:
            call()
        assert e.value.code == HOST_ONLY


def test_header_defines_vr_has_ray_query():
    text = open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()
    assert re.search(r"^#define\s+VR_HAS_RAY_QUERY\s+1\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_QUERY_NORMALIZE\s+1u\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_QUERY_REFERENCE_WALK\s+2u\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_ABI_VERSION\s+10\b", text, flags=re.M)


def test_abi_version_is_still_10():
    assert N.lib().vr_abi_version() == 10
