"""An independent numpy reference of the denoiser's rule (include/vanrijn_amd.h, "Denoiser").

It works on whole-image arrays: for each iteration and each of the 25 offsets it forms shifted views and
elementwise f64 products and sums in the order of the rule (numpy's elementwise add, subtract, multiply and
divide are single IEEE operations) and applies the skips as masks with np.where.  Its exp is
vanrijn_amd/csrc/vr_exp_table.h itself, compiled with gcc through tests/denoise_exp_shim.c and loaded with
ctypes; that header is existing code held to libm by tests/test_exp_table.py.  Nothing here shares a line
with vanrijn_amd/csrc/vr_denoise.h.
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MATCH_OBJECT, DEMODULATE = 1, 2
ALBEDO_FLOOR = 1.0 / 1024.0
HK = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)

_keep = []  # the temporary directory of the shim, for the life of the process


@functools.lru_cache(maxsize=None)
def _shim():
    d = tempfile.TemporaryDirectory()
    _keep.append(d)
    so = os.path.join(d.name, "denoise_exp_shim.so")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "denoise_exp_shim.c"), "-o", so, "-lm"])
    lib = C.CDLL(so)
    lib.denoise_exp_tab.restype = None
    lib.denoise_exp_tab.argtypes = [C.c_void_p, C.c_void_p, C.c_long]
    return lib


def exp_tab(x):
    """vr_exp_tab elementwise."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    _shim().denoise_exp_tab(x.ctypes.data, out.ctypes.data, x.size)
    return out


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, else `fill`."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


def denoise_reference(width, height, iterations, flags, sigma_colour, sigma_normal, sigma_depth, state, features,
                      albedo_state=None):
    """The output state (flat, 8 f64 per pixel) of the rule on flat state records, [height][width] feature
    records and, with DEMODULATE, the albedo's state records."""
    n = width * height
    sums = np.asarray(state, dtype=np.float64).reshape(-1)[:4 * n].reshape(height, width, 4)
    feat = np.asarray(features).reshape(height, width)
    with np.errstate(all="ignore"):
        weight = sums[..., 3]
        absent = weight == 0.0
        colour = sums[..., :3] * (1.0 / weight)[..., None]
        hits = feat["hits"]
        background = hits == 0
        inv = 1.0 / hits.astype(np.float64)
        normal = feat["normal_sum"] * inv[..., None]
        depth = feat["distance_sum"] * inv
        inv_depth = 1.0 / depth
        obj = feat["object"]
        demodulated = np.zeros((height, width, 3), dtype=bool)
        albedo = np.zeros((height, width, 3))
        if flags & DEMODULATE:
            asums = np.asarray(albedo_state, dtype=np.float64).reshape(-1)[:4 * n].reshape(height, width, 4)
            aw = asums[..., 3]
            albedo = np.where((aw != 0.0)[..., None], asums[..., :3] * (1.0 / aw)[..., None], 0.0)
            demodulated = albedo > ALBEDO_FLOOR
            colour = np.where(demodulated, colour / albedo, colour)
        kc0 = 1.0 / (sigma_colour * sigma_colour)
        kn = 1.0 / (sigma_normal * sigma_normal)
        kz = 1.0 / (sigma_depth * sigma_depth)
        inside = np.ones((height, width), dtype=bool)
        for i in range(iterations):
            step = 1 << i
            kc = kc0 * float(4 ** i)
            total = np.zeros((height, width, 3))
            total_w = np.zeros((height, width))
            centre_taken = np.zeros((height, width), dtype=bool)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    oy, ox = dy * step, dx * step
                    skip = ~_shifted(inside, oy, ox, False)
                    skip |= _shifted(absent, oy, ox, True)
                    bg_q = _shifted(background, oy, ox, False)
                    skip |= background != bg_q
                    if flags & MATCH_OBJECT:
                        skip |= ~background & ~bg_q & (obj != _shifted(obj, oy, ox, 0))
                    cq = _shifted(colour, oy, ox, 0.0)
                    d = cq - colour
                    e_c = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * kc
                    m = _shifted(normal, oy, ox, 0.0) - normal
                    e_n = ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]) * kn
                    t = (_shifted(depth, oy, ox, 0.0) - depth) * inv_depth
                    e_z = (t * t) * kz
                    both_bg = background & bg_q
                    e = (e_c + np.where(both_bg, 0.0, e_n)) + np.where(both_bg, 0.0, e_z)
                    skip |= np.isnan(e)
                    wt = (HK[dy + 2] * HK[dx + 2]) * exp_tab(-e)
                    skip |= ~(wt != 0.0) | np.isnan(wt)
                    total = np.where(skip[..., None], total, total + wt[..., None] * cq)
                    total_w = np.where(skip, total_w, total_w + wt)
                    if dy == 0 and dx == 0:
                        centre_taken = ~skip
            colour = np.where(centre_taken[..., None], total * (1.0 / total_w)[..., None], colour)
        colour = np.where(demodulated, colour * albedo, colour)
    out = np.zeros(8 * n)
    rec = out[:4 * n].reshape(height, width, 4)
    rec[..., :3] = np.where(absent[..., None], 0.0, colour)
    rec[..., 3] = np.where(absent, 0.0, 1.0)
    return out


def same_bits(a, b):
    """Bit for bit, except that a NaN need only be a NaN in the same place; zeros must match in sign."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint64)[~nan_a], b.view(np.uint64)[~nan_b]))
