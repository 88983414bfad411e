"""Film entry points (vr_film_*, include/vanrijn_amd.h): every argument check runs before the first
device call, so all of this passes on a machine without a GPU.  The film itself is exercised in
tests/test_gpu_film.py."""
import ctypes as C
import os
import re

import numpy as np

from vanrijn_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1  # VR_ERROR_INVALID_ARGUMENT


def _invalid(rc):
    assert rc == INVALID, rc
    assert len(N.lib().vr_last_error()) > 0


def _buffer(width, height):
    arrays = [np.zeros(width * height * k) for k in (3, 3, 3, 1, 1)]
    return arrays, N.AccumulationBufferC(width, height, *(a.ctypes.data for a in arrays))


def test_create_rejects_null_out_and_zero_dimensions():
    L = N.lib()
    _invalid(L.vr_film_create(8, 8, 0, None))
    h = C.c_void_p()
    _invalid(L.vr_film_create(0, 8, 0, C.byref(h)))
    assert not h.value
    _invalid(L.vr_film_create(8, 0, 0, C.byref(h)))
    assert not h.value


def test_null_film_is_rejected_by_every_entry_point():
    L = N.lib()
    tile = N.TileC(0, 4, 0, 4)
    m = N.FilmMerge()
    seen = C.c_uint64()
    params = N.RenderParams(tile, 4, 4, 1, 0, 1, 0)
    _, buf = _buffer(4, 4)
    rgb = np.zeros(48, dtype=np.uint8)
    state = np.zeros(16 * 8)  # never read: the film is checked first
    scene = C.c_void_p(0)
    L.vr_film_destroy(None)  # allowed, does nothing
    _invalid(L.vr_film_clear(None))
    _invalid(L.vr_film_partial_render_scene(None, scene, tile, C.byref(m)))
    _invalid(L.vr_film_render_tile(None, scene, C.byref(params), C.byref(m)))
    _invalid(L.vr_film_merge_state(None, tile, state.ctypes.data_as(C.c_void_p), None, C.byref(m)))
    _invalid(L.vr_film_read(None, C.byref(buf), C.byref(seen)))
    _invalid(L.vr_film_to_image_rgb_u8(None, rgb.ctypes.data_as(C.c_void_p), C.byref(seen)))
    _invalid(L.vr_film_to_image_rgb_u8_device(None, rgb.ctypes.data_as(C.c_void_p), None, C.byref(seen)))


def test_abi_version_is_still_10():
    assert N.lib().vr_abi_version() == 10


def test_header_defines_vr_has_film():
    text = open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()
    assert re.search(r"^#define\s+VR_HAS_FILM\s+1\b", text, flags=re.M)
    assert re.search(r"^#define\s+VR_ABI_VERSION\s+10\b", text, flags=re.M)
