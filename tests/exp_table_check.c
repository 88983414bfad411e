/* Max ulp distance of vr_exp_tab (vanrijn_amd/csrc/vr_exp_table.h) from libm exp over the reduce's
 * argument range: a deterministic sweep of [-745, 0] plus the CIE lobes' exponents at
 * wavelengths 0 and 380..740 nm, then the arguments below the range (exactly +0) and NaN.  Prints
 * "<max ulp> <points> <below-range results that are not +0> <1 if NaN gave NaN> <arguments where
 * vr_exp_tab_near, the form the reduce calls, differs from vr_exp_tab on its domain>".  Built by
 * tests/test_exp_table.py with gcc -O2 -ffp-contract=off. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../vanrijn_amd/csrc/vr_exp_table.h"

static const double tab[64] = VR_EXP_TABLE_INIT;

static int64_t ord(double v) {
    int64_t i;
    memcpy(&i, &v, 8);
    return i < 0 ? INT64_MIN - i : i;
}

static double worst = 0.0;
static long points = 0;
static long near_differs = 0; /* arguments where vr_exp_tab_near and vr_exp_tab give different bits */

static void check(double x) {
    const double a = vr_exp_tab(x, tab), b = exp(x);
    const double d = fabs((double)(ord(a) - ord(b)));
    if (d > worst) worst = d;
    if (ord(vr_exp_tab_near(x, tab)) != ord(a)) ++near_differs;
    ++points;
}

int main(void) {
    uint64_t s = 0x243F6A8885A308D3ull;
    for (long i = 0; i < 10000000; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        check(-745.0 * (double)(s >> 11) * 0x1.0p-53);
    }
    for (long i = 0; i < 1000000; ++i) {  /* small arguments, where r = x */
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        check(-0.02 * (double)(s >> 11) * 0x1.0p-53);
    }
    /* the reduce's exponents: -(t^2) k for the seven lobes of colour_xyz.rs:86-103 */
    static const double lobes[7][3] = {{599.8, 37.9, 31.0}, {442.0, 16.0, 26.7}, {501.1, 20.4, 26.2},
                                       {568.8, 46.9, 40.5}, {530.9, 16.3, 31.1}, {437.0, 11.8, 36.0},
                                       {459.0, 26.0, 13.8}};
    for (int k = 0; k < 7; ++k)
        for (long i = -1; i <= 3600000; ++i) {
            const double wl = i < 0 ? 0.0 : 380.0 + (double)i * 1e-4;
            const double mu = lobes[k][0], sg = wl < mu ? lobes[k][1] : lobes[k][2];
            const double t = wl - mu;
            check(-(t * t) * (1.0 / (2.0 * (sg * sg))));
        }
    check(0.0);
    check(-0.0);
    check(-745.0);
    /* below the table's range exp is +0 (libm's too); NaN stays NaN.  Third and fourth numbers of
     * the output: how many of these returned something else than +0 (by bits), and whether NaN
     * came back as NaN */
    static const double below[10] = {-745.2, -746.0, -1e3, -1e13, -1e60, -1e68, -1e77, -1e296, -DBL_MAX, -INFINITY};
    int not_zero = 0;
    for (int i = 0; i < 10; ++i) {
        const double a = vr_exp_tab(below[i], tab);
        uint64_t bits;
        memcpy(&bits, &a, 8);
        if (bits != 0) {
            ++not_zero;
            fprintf(stderr, "vr_exp_tab(%g) = %g (bits %016llx), expected +0\n", below[i], a, (unsigned long long)bits);
        }
    }
    const double of_nan = vr_exp_tab(NAN, tab), near_of_nan = vr_exp_tab_near(NAN, tab);
    /* vr_exp_tab_near's own domain below the range, down to the reduce's lowest argument
     * (-(20000 + 599.8)^2 / (2 * 11.8^2) = -1.52e6) and to -2^24: +0 as well */
    for (long i = 0; i <= 1000000; ++i) {
        const double x = i < 1000000 ? -745.2 - 1.6 * (double)i : -0x1.0p+24;
        uint64_t bits;
        const double a = vr_exp_tab_near(x, tab);
        memcpy(&bits, &a, 8);
        if (bits != 0) ++near_differs;
    }
    printf("%.0f %ld %d %d %ld\n", worst, points, not_zero, of_nan != of_nan && near_of_nan != near_of_nan,
           near_differs);
    return 0;
}
