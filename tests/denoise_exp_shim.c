/* denoise_exp_shim.c -- vr_exp_tab of vanrijn_amd/csrc/vr_exp_table.h, array in and array out, for
 * tests/denoise_reference.py (built with gcc -O2 -std=c99 -ffp-contract=off into a shared object and loaded
 * with ctypes).  The header is held to libm by tests/test_exp_table.py; it is not the code under test. */
#include "../vanrijn_amd/csrc/vr_exp_table.h"

static const double table[64] = VR_EXP_TABLE_INIT;

void denoise_exp_tab(const double* x, double* out, long n) {
    for (long i = 0; i < n; ++i) out[i] = vr_exp_tab(x[i], table);
}
