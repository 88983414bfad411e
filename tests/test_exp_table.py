"""The ordered reduce's table-driven exp (vanrijn_amd/csrc/vr_exp_table.h) against libm exp.

accumulate_kernel evaluates the CIE lobes of ColourXyz::x/y/z (colour_xyz.rs:86-103) with
vr_exp_tab instead of the general exp; the header is plain C99, so gcc builds it unchanged here and
tests/exp_table_check.c measures the largest ulp distance from libm's exp over 10^7 arguments in
[-745, 0], 10^6 small ones and every lobe exponent at 0 nm and 380..740 nm in 1e-4 nm steps.

Below the table's range (-745.2, -746, -1e3, -1e13, -1e60, -1e68, -1e77, -1e296, -DBL_MAX, -inf) the
result must be exactly +0, as libm's and the reference's exp, and NaN must give NaN: a caller's
wavelength may be any double (vr_accumulate_photons_device), and before the range clamp the header
returned inf from about -3.9e68 down and NaN from about -1e160 down and at -inf.
"""
import os
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_ULP = 2
BELOW_RANGE = 10  # arguments below -745 that exp_table_check.c evaluates

needs_gcc = pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")


@pytest.fixture(scope="module")
def check_output():
    """One build and one run of exp_table_check.c: (max ulp, points, below-range results that are
    not +0, whether NaN gave NaN, arguments where vr_exp_tab_near differs from vr_exp_tab)."""
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "exp_check")
        subprocess.check_call(["gcc", "-O2", "-std=c99", "-ffp-contract=off", os.path.join(HERE, "exp_table_check.c"),
                               "-o", exe, "-lm"])
        worst, points, not_zero, nan_kept, near_differs = subprocess.check_output([exe], timeout=120).split()
    return float(worst), int(points), int(not_zero), int(nan_kept), int(near_differs)


@needs_gcc
def test_exp_table_within_two_ulp(check_output):
    worst, points = check_output[:2]
    assert points > 36_000_000
    assert worst <= MAX_ULP


@needs_gcc
def test_exp_table_below_range_is_plus_zero(check_output):
    assert 0 <= check_output[2] <= BELOW_RANGE
    assert check_output[2] == 0  # the failing arguments are on the check's stderr


@needs_gcc
def test_exp_table_keeps_nan(check_output):
    assert check_output[3] == 1


@needs_gcc
def test_exp_table_near_form_is_the_same_function(check_output):
    """vr_exp_tab_near, which the reduce calls after clamping the wavelength, gives vr_exp_tab's bits on
    every argument of the sweep and +0 from -745.2 down to -2^24, the end of its domain."""
    assert check_output[4] == 0
