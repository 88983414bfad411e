// vr_reproject.h -- the temporal reprojection's rule (include/vanrijn_amd.h, "Temporal reprojection") as
// inline functions that the kernel of vr_reproject.hip and vr_reproject_host (vr_host_reproject.cpp) both
// compile, as vr_denoise.h does for the denoiser: the per-pixel geometry, the motion row, the projection into
// the previous view, the tap test, the fold over the footprint, the cap and the output record.  Every
// operation is written once, here, in the order the header states; the units are compiled with
// -ffp-contract=off.  The camera ray and the film constants are vr_camera.h's, not restated.
//
// There is no workspace: a pixel reads its own two records, then up to four previous-frame taps.  A tap is
// read quad by quad (16 B) in the order that lets an earlier test spare the later loads: the previous
// state's {S2, W} and {S0, S1}, then of the previous feature record quad 2 (hits), quad 3 (object, only with
// VR_REPROJECT_MATCH_OBJECT), quad 1 (depth) and quad 0 (the rest of the normal).  The order of the skip
// tests does not matter to the result: a tap is kept only if it passes them all.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_camera.h"
#include "vr_denoise.h"  // D2 and FeatureRecord: the 16-B quad and the feature record's layout

#define VR_RP_FN VR_DN_FN

namespace vr {
namespace reproject {

using denoise::D2;
constexpr uint64_t kMaxPixels = denoise::kMaxPixels;

struct Pose {  // vr_camera_pose as the camera functions take it
    double location[3], right[3], up[3], forward[3], film_distance;
};

// what the host computes once (vrh::reproject_check)
struct Consts {
    Pose pose, previous;
    double film[4];              // vr::camera::film_constants(width, height)
    double dt2, nt2, cap;        // the squared tolerances, max_history_weight
    uint64_t width, height, n;
    uint32_t flags, motion_count;
    uint32_t same_pose, reserved;  // 1: the 13 doubles of the two poses compare equal
};

VR_RP_FN uint32_t low_word(double d) {  // the first of the two 32-bit fields that share a double's place
    uint64_t u;
    __builtin_memcpy(&u, &d, 8);
    return (uint32_t)u;
}
VR_RP_FN bool finite(double x) { return !(x - x != 0.0); }

struct Tap {
    int64_t q;  // row * width + column in the previous frame
    double b;
};

struct Centre {  // what steps 2-6 leave for the taps
    double g[3];     // g'
    double z, iz;    // z', iz'
    int32_t object;  // o
    bool any;        // false: no history
    Tap tap[4];      // in tap order; b == 0: skipped unread
};

// Steps 2-6 for pixel (row, column).  `f` gives the current feature record's quads: quad(0..3) as D2;
// `motion` is null or the rows (a host array or device memory, plain f64 loads).
template <class Quads>
VR_RP_FN void centre_pixel(const Consts& k, const Quads& f, const double* motion, int64_t row, int64_t column,
                           Centre* out) {
    out->any = false;
VR_DN_UNROLL
    for (int j = 0; j < 4; ++j) out->tap[j] = Tap{0, 0.0};
    // 2. geometry
    const D2 q2 = f.quad(2);
    const uint32_t hits = low_word(q2.y);
    if (hits == 0) return;
    const D2 q0 = f.quad(0), q1 = f.quad(1);
    const double inv = 1.0 / (double)hits;
    double g[3] = {q0.x * inv, q0.y * inv, q1.x * inv};
    const double z = q1.y * inv;
    if (!(z > 0.0) || !finite(z)) return;
    const camera::Vec d = camera::ray_direction(k.pose.right, k.pose.up, k.pose.forward, k.pose.film_distance,
                                                camera::film_x(k.film, (uint64_t)column, 0.5),
                                                camera::film_y(k.film, k.height, (uint64_t)row, 0.5));
    double P[3] = {k.pose.location[0] + d.x * z, k.pose.location[1] + d.y * z, k.pose.location[2] + d.z * z};
    // 3. motion
    int32_t object = 0;
    bool moved = false;
    if (motion != nullptr || (k.flags & VR_REPROJECT_MATCH_OBJECT)) object = (int32_t)low_word(f.quad(3).x);
    if (motion != nullptr && object >= 0 && (uint32_t)object < k.motion_count) {
        const double* m = motion + 12 * (uint64_t)object;
        double mm[12];
        bool identity = true;
VR_DN_UNROLL
        for (int i = 0; i < 12; ++i) {
            mm[i] = m[i];
            identity = identity && mm[i] == ((i == 0 || i == 5 || i == 10) ? 1.0 : 0.0);
        }
        const double Px = P[0], Py = P[1], Pz = P[2], gx = g[0], gy = g[1], gz = g[2];
VR_DN_UNROLL
        for (int c = 0; c < 3; ++c) {
            P[c] = ((mm[4 * c] * Px + mm[4 * c + 1] * Py) + mm[4 * c + 2] * Pz) + mm[4 * c + 3];
            g[c] = (mm[4 * c] * gx + mm[4 * c + 1] * gy) + mm[4 * c + 2] * gz;
        }
        moved = !identity;
    }
    out->g[0] = g[0];
    out->g[1] = g[1];
    out->g[2] = g[2];
    out->object = object;
    // 4. the same view
    if (k.same_pose && !moved) {
        out->z = z;
        out->iz = 1.0 / z;
        out->tap[0] = Tap{row * (int64_t)k.width + column, 1.0};
        out->any = true;
        return;
    }
    // 5. projection on the previous pose
    const Pose& pp = k.previous;
    const double vx = P[0] - pp.location[0], vy = P[1] - pp.location[1], vz = P[2] - pp.location[2];
    const double a = (vx * pp.right[0] + vy * pp.right[1]) + vz * pp.right[2];
    const double bb = (vx * pp.up[0] + vy * pp.up[1]) + vz * pp.up[2];
    const double c = (vx * pp.forward[0] + vy * pp.forward[1]) + vz * pp.forward[2];
    if (!(c > 0.0)) return;
    const double s = pp.film_distance / c;
    const double xp = a * s, yp = bb * s;
    const double zp = sqrt((vx * vx + vy * vy) + vz * vz);
    out->z = zp;
    out->iz = 1.0 / zp;
    const double fx = (xp + k.film[1]) / k.film[0] - 0.5;
    const double fy = (yp + k.film[3]) / k.film[2] - 0.5;
    const double fr = (double)(k.height - 1) - fy;
    // 6. footprint
    if (!(fx >= -1.0 && fx < (double)k.width && fr >= -1.0 && fr < (double)k.height)) return;
    const double fix = floor(fx), fiy = floor(fr);
    const double tx = fx - fix, ty = fr - fiy;
    const int64_t ix = (int64_t)fix, iy = (int64_t)fiy;
VR_DN_UNROLL
    for (int j = 0; j < 4; ++j) {
        const int dy = j >> 1, dx = j & 1;
        const double b = (dx ? tx : 1.0 - tx) * (dy ? ty : 1.0 - ty);
        const int64_t qx = ix + dx, qy = iy + dy;
        if (b == 0.0 || qx < 0 || qx >= (int64_t)k.width || qy < 0 || qy >= (int64_t)k.height) continue;
        out->tap[j] = Tap{qy * (int64_t)k.width + qx, b};
        out->any = true;
    }
}

struct History {  // B, H_k and Wh of step 8
    double B, h[3], w;
};

// 7 and 8 for one tap.  `prev` gives the previous frame: state(q, 0) = {S0, S1}, state(q, 1) = {S2, W},
// feature(q, quad).
template <class Prev>
VR_RP_FN void fold_tap(const Consts& k, const Prev& prev, const Centre& c, const Tap& t, History& acc) {
    const D2 hi = prev.state(t.q, 1);
    if (!finite(hi.x) || !finite(hi.y) || hi.y == 0.0) return;
    const D2 lo = prev.state(t.q, 0);
    if (!finite(lo.x) || !finite(lo.y)) return;
    const uint32_t hits = low_word(prev.feature(t.q, 2).y);
    if (hits == 0) return;
    if ((k.flags & VR_REPROJECT_MATCH_OBJECT) && (int32_t)low_word(prev.feature(t.q, 3).x) != c.object) return;
    const double invq = 1.0 / (double)hits;
    const D2 f1 = prev.feature(t.q, 1);
    const double zq = f1.y * invq;
    const double dz = (zq - c.z) * c.iz;
    if (!(dz * dz <= k.dt2)) return;
    const D2 f0 = prev.feature(t.q, 0);
    const double m0 = f0.x * invq - c.g[0], m1 = f0.y * invq - c.g[1], m2 = f1.x * invq - c.g[2];
    if (!(((m0 * m0 + m1 * m1) + m2 * m2) <= k.nt2)) return;
    acc.B = acc.B + t.b;
    acc.h[0] = acc.h[0] + t.b * lo.x;
    acc.h[1] = acc.h[1] + t.b * lo.y;
    acc.h[2] = acc.h[2] + t.b * hi.x;
    acc.w = acc.w + t.b * hi.y;
}

// The whole rule for pixel (row, column): its own sums record {s_lo, s_hi} in, the output's sums record out
// (the bias record is zero whatever happens).
template <class Quads, class Prev>
VR_RP_FN void reproject_pixel(const Consts& k, const D2 s_lo, const D2 s_hi, const Quads& f, const Prev& prev,
                              const double* motion, int64_t row, int64_t column, D2* o_lo, D2* o_hi) {
    const double W = s_hi.y;
    if (W == 0.0) {  // 1. absent
        *o_lo = D2{0.0, 0.0};
        *o_hi = D2{0.0, 0.0};
        return;
    }
    *o_lo = s_lo;
    *o_hi = s_hi;
    Centre c;
    centre_pixel(k, f, motion, row, column, &c);
    if (!c.any) return;
    History acc = {0.0, {0.0, 0.0, 0.0}, 0.0};
VR_DN_UNROLL
    for (int j = 0; j < 4; ++j)
        if (c.tap[j].b != 0.0) fold_tap(k, prev, c, c.tap[j], acc);
    if (acc.B == 0.0) return;
    const double r = 1.0 / acc.B;
    double h[3] = {acc.h[0] * r, acc.h[1] * r, acc.h[2] * r}, wh = acc.w * r;
    if (wh > k.cap) {  // 9
        const double fcap = k.cap / wh;
        h[0] = h[0] * fcap;
        h[1] = h[1] * fcap;
        h[2] = h[2] * fcap;
        wh = k.cap;
    }
    *o_lo = D2{s_lo.x + h[0], s_lo.y + h[1]};  // 10
    *o_hi = D2{s_hi.x + h[2], W + wh};
}

}  // namespace reproject
}  // namespace vr

#pragma GCC visibility push(hidden)
namespace vrh {
// vr_host_reproject.cpp: the checks every form shares, in the header's order, and the constants.  VR_OK with
// k->n == 0 is the empty image.  `aligned`: the arrays are device arrays and must be 16-byte aligned.
int reproject_check(const vr_reproject_params* p, const void* state, const void* features, const void* previous_state,
                    const void* previous_features, const void* motion, const void* out_state, bool aligned,
                    vr::reproject::Consts* k);
}  // namespace vrh
#pragma GCC visibility pop
