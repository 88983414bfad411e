/* Force-included (gcc -include) in front of oracle/vr_oracle.c by tests/libm_sensitivity.py to build a
 * SECOND, test-only copy of the oracle whose cos and sin results are moved by a number of ulps.  The
 * oracle's source and its library are not touched.  cos and sin are called in one place there, the
 * Phong sampler (CosineWeightedHemisphere); acos is another token and stays. */
#include <math.h>
int libm_nudge_cos = 0, libm_nudge_sin = 0;
static double libm_nudged(double x, int n) {
    for (; n > 0; --n) x = nextafter(x, INFINITY);
    for (; n < 0; ++n) x = nextafter(x, -INFINITY);
    return x;
}
static double libm_nudged_cos(double x) { return libm_nudged(cos(x), libm_nudge_cos); }
static double libm_nudged_sin(double x) { return libm_nudged(sin(x), libm_nudge_sin); }
#define cos libm_nudged_cos
#define sin libm_nudged_sin
