// vr_denoise.h -- the denoiser's rule (include/vanrijn_amd.h, "Denoiser") as inline functions that the
// kernels of vr_denoise.hip and vr_denoise_host (vr_host_denoise.cpp) both compile, as vr_camera.h does for
// the ray rule: the per-pixel preparation, the per-tap rule, the per-pixel fold over the 25 taps and the
// output record.  Every operation is written once, here, in the order the header states; the units are
// compiled with -ffp-contract=off, and the only fused operations are the fma calls inside vr_exp_tab.
//
// The workspace, 128 B per pixel of an image of n pixels, four arrays of 32-B records (two 16-B quads each):
//   [n Colour: ping][n Colour: pong][n Guide][n Extra]
// so a tap costs four 16-B loads (two when the class word already rejects it) instead of reads from three
// differently shaped arrays.  The class word travels with the colour: iteration i reads buffer i & 1 and
// writes the other, copying the centre's class.
#pragma once
#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_exp_table.h"

#ifdef __HIPCC__
#define VR_DN_FN __host__ __device__ inline
#define VR_DN_UNROLL _Pragma("unroll")  // the kernels index hk[] with constants: no array in scratch
#else
#define VR_DN_FN inline
#define VR_DN_UNROLL
#endif

namespace vr {
namespace denoise {

struct alignas(16) D2 {
    double x, y;
};
struct Colour {  // {c0, c1}, {c2, class word}: the class word's bits live in a double that is only moved
    D2 lo, hi;
};
struct Guide {  // {g0, g1}, {g2, z}: mean normal and mean depth; zeros in a background or absent pixel
    D2 lo, hi;
};
struct Extra {  // {iz, a0}, {a1, a2}: 1 / z (the centre's only) and the albedo (0 without VR_DENOISE_DEMODULATE)
    D2 lo, hi;
};
struct alignas(16) FeatureRecord {  // vr_pixel_features, known to be 16-byte aligned
    double normal_sum[3], distance_sum, distance_min;
    uint32_t hits, samples;
    int32_t object, reserved;
    int64_t primitive;
};
static_assert(sizeof(Colour) == 32 && sizeof(Guide) == 32 && sizeof(Extra) == 32, "32-B workspace records");
static_assert(sizeof(FeatureRecord) == sizeof(vr_pixel_features) && sizeof(FeatureRecord) == 64, "the feature record");

// the class word: kind in the high half, vr_pixel_features::object in the low half
constexpr uint32_t kHit = 0, kBackground = 1, kAbsent = 2;
constexpr uint64_t kWorkspacePerPixel = 128;
constexpr uint64_t kMaxPixels = 1ull << 31;

// what the host computes once (vrh::denoise_check)
struct Consts {
    double kc0, kn, kz;
    double hk[5];
    uint64_t width, height, n;
    uint32_t iterations, flags;
};

VR_DN_FN double class_word(uint32_t kind, int32_t object) {
    const uint64_t u = ((uint64_t)kind << 32) | (uint32_t)object;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}
VR_DN_FN uint64_t class_bits(double word) {
    uint64_t u;
    __builtin_memcpy(&u, &word, 8);
    return u;
}

// Inputs per pixel: the state's sums record, the feature record and the albedo's sums record (read only
// when `demodulate`) into the workspace form.
VR_DN_FN void prepare_pixel(const D2 s_lo, const D2 s_hi, const FeatureRecord& f, const D2 a_lo, const D2 a_hi,
                            bool demodulate, Colour* colour, Guide* guide, Extra* extra) {
    double a[3] = {0.0, 0.0, 0.0};
    if (demodulate && a_hi.y != 0.0) {
        const double ia = 1.0 / a_hi.y;
        a[0] = a_lo.x * ia;
        a[1] = a_lo.y * ia;
        a[2] = a_hi.x * ia;
    }
    double g[3] = {0.0, 0.0, 0.0}, z = 0.0, iz = 0.0;
    if (f.hits != 0) {
        const double inv = 1.0 / (double)f.hits;
        g[0] = f.normal_sum[0] * inv;
        g[1] = f.normal_sum[1] * inv;
        g[2] = f.normal_sum[2] * inv;
        z = f.distance_sum * inv;
        iz = 1.0 / z;
    }
    const double w = s_hi.y;
    double c[3] = {0.0, 0.0, 0.0};
    if (w != 0.0) {
        const double iw = 1.0 / w;
        c[0] = s_lo.x * iw;
        c[1] = s_lo.y * iw;
        c[2] = s_hi.x * iw;
        if (demodulate)
            for (int k = 0; k < 3; ++k)
                if (a[k] > VR_DENOISE_ALBEDO_FLOOR) c[k] = c[k] / a[k];
    }
    const uint32_t kind = w == 0.0 ? kAbsent : f.hits == 0 ? kBackground : kHit;
    colour->lo = D2{c[0], c[1]};
    colour->hi = D2{c[2], class_word(kind, kind == kHit ? f.object : 0)};
    guide->lo = D2{g[0], g[1]};
    guide->hi = D2{g[2], z};
    extra->lo = D2{iz, a[0]};
    extra->hi = D2{a[1], a[2]};
}

struct Sums {  // S_k and W of one centre, and whether its own tap was taken
    double s[3], w;
    bool centre;
};

// One tap q of centre p whose class words already passed tap_class: e, w and the sums.
VR_DN_FN void tap(const Colour& cp, const Guide& gp, double izp, const Colour& cq, const Guide& gq, bool background,
                  double hkw, double kc, double kn, double kz, const double* tab, bool is_centre, Sums& acc) {
    const double d0 = cq.lo.x - cp.lo.x, d1 = cq.lo.y - cp.lo.y, d2 = cq.hi.x - cp.hi.x;
    const double e_c = ((d0 * d0 + d1 * d1) + d2 * d2) * kc;
    double e_n = 0.0, e_z = 0.0;
    if (!background) {
        const double m0 = gq.lo.x - gp.lo.x, m1 = gq.lo.y - gp.lo.y, m2 = gq.hi.x - gp.hi.x;
        e_n = ((m0 * m0 + m1 * m1) + m2 * m2) * kn;
        const double t = (gq.hi.y - gp.hi.y) * izp;
        e_z = (t * t) * kz;
    }
    const double e = (e_c + e_n) + e_z;
    if (e != e) return;
    const double w = hkw * vr_exp_tab(-e, tab);
    if (w == 0.0) return;
    acc.s[0] = acc.s[0] + w * cq.lo.x;
    acc.s[1] = acc.s[1] + w * cq.lo.y;
    acc.s[2] = acc.s[2] + w * cq.hi.x;
    acc.w = acc.w + w;
    if (is_centre) acc.centre = true;
}

// The skips that need the class words only: q absent, exactly one of p and q background, another object.
VR_DN_FN bool tap_class(uint64_t class_p, uint64_t class_q, bool match_object) {
    const uint32_t kp = (uint32_t)(class_p >> 32), kq = (uint32_t)(class_q >> 32);
    if (kq == kAbsent) return false;
    if ((kp == kBackground) != (kq == kBackground)) return false;
    if (match_object && kp == kHit && kq == kHit && (uint32_t)class_p != (uint32_t)class_q) return false;
    return true;
}

// One iteration at centre (x, y): the 25 taps, dy outer, dx inner.  `load` gives the records of a pixel
// inside the image -- colour(qx, qy), guide(qx, qy) -- and iz(x, y) of the centre; the centre's own records
// are loaded once.  Returns c' with the centre's class word.
template <class Load>
VR_DN_FN Colour fold_pixel(const Load& load, int64_t x, int64_t y, const Consts& k, int64_t step, double kc,
                           const double* tab) {
    const Colour cp = load.colour(x, y);
    const uint64_t class_p = class_bits(cp.hi.y);
    if ((uint32_t)(class_p >> 32) == kAbsent) return cp;
    const bool bg_p = (uint32_t)(class_p >> 32) == kBackground;
    Guide gp = {D2{0.0, 0.0}, D2{0.0, 0.0}};
    double izp = 0.0;
    if (!bg_p) {
        gp = load.guide(x, y);
        izp = load.iz(x, y);
    }
    const bool match = (k.flags & VR_DENOISE_MATCH_OBJECT) != 0;
    const int64_t width = (int64_t)k.width, height = (int64_t)k.height;
    Sums acc = {{0.0, 0.0, 0.0}, 0.0, false};
VR_DN_UNROLL
    for (int dy = -2; dy <= 2; ++dy) {
        const int64_t qy = y + dy * step;
        if (qy < 0 || qy >= height) continue;
VR_DN_UNROLL
        for (int dx = -2; dx <= 2; ++dx) {
            const int64_t qx = x + dx * step;
            if (qx < 0 || qx >= width) continue;
            const bool is_centre = dx == 0 && dy == 0;
            const double hkw = k.hk[dy + 2] * k.hk[dx + 2];
            if (is_centre) {
                tap(cp, gp, izp, cp, gp, bg_p, hkw, kc, k.kn, k.kz, tab, true, acc);
                continue;
            }
            const Colour cq = load.colour(qx, qy);
            if (!tap_class(class_p, class_bits(cq.hi.y), match)) continue;
            Guide gq = gp;
            if (!bg_p) gq = load.guide(qx, qy);
            tap(cp, gp, izp, cq, gq, bg_p, hkw, kc, k.kn, k.kz, tab, false, acc);
        }
    }
    if (!acc.centre) return cp;
    const double iw = 1.0 / acc.w;
    Colour out;
    out.lo = D2{acc.s[0] * iw, acc.s[1] * iw};
    out.hi = D2{acc.s[2] * iw, cp.hi.y};
    return out;
}

// The output record of a pixel: its sums quads; the bias quads are zero.
VR_DN_FN void finish_pixel(const Colour& c, const Extra& e, bool demodulate, D2* s_lo, D2* s_hi) {
    if ((uint32_t)(class_bits(c.hi.y) >> 32) == kAbsent) {
        *s_lo = D2{0.0, 0.0};
        *s_hi = D2{0.0, 0.0};
        return;
    }
    double v[3] = {c.lo.x, c.lo.y, c.hi.x};
    if (demodulate) {
        const double a[3] = {e.lo.y, e.hi.x, e.hi.y};
        for (int k = 0; k < 3; ++k)
            if (a[k] > VR_DENOISE_ALBEDO_FLOOR) v[k] = v[k] * a[k];
    }
    *s_lo = D2{v[0], v[1]};
    *s_hi = D2{v[2], 1.0};
}

// kc_i = kc_0 * 4^i: a power of two, exact
VR_DN_FN double colour_scale(const Consts& k, uint32_t i) { return k.kc0 * (double)(1ull << (2 * i)); }

}  // namespace denoise
}  // namespace vr

#pragma GCC visibility push(hidden)
namespace vrh {
// vr_host_denoise.cpp: the checks every form shares, in the header's order, and the constants.  VR_OK with
// k->n == 0 is the empty image.  `aligned`: the arrays are device arrays and must be 16-byte aligned.
int denoise_check(const vr_denoise_params* p, const void* state, const void* features, const void* albedo_state,
                  const void* out_state, bool aligned, vr::denoise::Consts* k);
}  // namespace vrh
#pragma GCC visibility pop
