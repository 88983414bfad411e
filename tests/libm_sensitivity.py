"""Which samples of a render depend on libm's last bits, measured on the reference side alone.

The oracle's Phong sampler calls cos and sin; the device's libm and glibc may round them differently
in the last bit, and a photon made of x^1000 lobes multiplies that by 1000.  To find such samples
without touching the oracle, this module compiles a second, test-only copy of oracle/vr_oracle.c with
tests/libm_nudge.h force-included, in which every cos and sin result is moved by a chosen number of
ulps, and renders with it through a second instance of oracle/oracle_ffi.py.  No device value enters.
"""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# oracle/Makefile's flags: the copy differs from the oracle in the two nudged calls only
CFLAGS = ["-O2", "-std=c11", "-D_POSIX_C_SOURCE=200809L", "-D_DEFAULT_SOURCE", "-ffp-contract=off", "-fno-fast-math",
          "-fPIC", "-shared"]
_nudged = None


def nudged_oracle():
    """The second oracle_ffi module, bound to the nudged copy (built once per process in a temporary
    directory)."""
    global _nudged
    if _nudged is None:
        out = os.path.join(tempfile.mkdtemp(prefix="nudged_oracle_"), "liboracle_nudged.so")
        subprocess.check_call([os.environ.get("CC", "gcc")] + CFLAGS + [
            "-include", os.path.join(ROOT, "tests", "libm_nudge.h"), "-I", os.path.join(ROOT, "oracle"), "-o", out,
            os.path.join(ROOT, "oracle", "vr_oracle.c"), "-lm", "-pthread"])
        spec = importlib.util.spec_from_file_location("oracle_ffi_nudged", os.path.join(ROOT, "oracle", "oracle_ffi.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.LIB_PATH = out
        mod.lib()
        _nudged = mod
    return _nudged


def _set(mod, cos_ulps, sin_ulps):
    C.c_int.in_dll(mod.lib(), "libm_nudge_cos").value = cos_ulps
    C.c_int.in_dll(mod.lib(), "libm_nudge_sin").value = sin_ulps


def photon_moves(spec, tile, height, width, spp, seed):
    """Per sample [tile_h][tile_w][spp]: the largest relative change of the photon's intensity when cos
    and sin move by one ulp (the four sign choices) against the unmoved copy; inf where flags, bounces
    or the wavelength change."""
    mod = nudged_oracle()
    scene = mod.OracleScene(spec)
    _set(mod, 0, 0)
    base = scene.render_samples(tile, height, width, spp, seed, nthreads=8)
    move = np.zeros(base.shape)
    try:
        for c, s in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            _set(mod, c, s)
            r = scene.render_samples(tile, height, width, spp, seed, nthreads=8)
            same = (r["flags"] == base["flags"]) & (r["bounces"] == base["bounces"]) & (
                r["wavelength"] == base["wavelength"])
            with np.errstate(invalid="ignore", divide="ignore"):
                e = np.where(r["intensity"] == base["intensity"], 0.0,
                             np.abs(r["intensity"] - base["intensity"]) / np.abs(base["intensity"]))
            move = np.maximum(move, np.where(same, np.nan_to_num(e, nan=np.inf), np.inf))
    finally:
        _set(mod, 0, 0)
    return move, base
