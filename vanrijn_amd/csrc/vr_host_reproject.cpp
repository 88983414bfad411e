// vr_host_reproject.cpp -- the temporal reprojection's HIP-free half: the defaults, the checks every form
// shares, and vr_reproject_host, the rule of vr_reproject.h in plain C++ on host arrays (the counterpart of
// vr_denoise_host; tools/reproject_host_check.cpp builds this file alone under the host sanitizers).  The
// device forms are in vr_reproject.hip.
#define VR_HOST_NO_HIP
#include "vr_reproject.h"
#include "vr_host.h"

using namespace vrh;
namespace rp = vr::reproject;

namespace {
void copy_pose(const vr_camera_pose& p, rp::Pose* out) {
    const vr_vec3 v[4] = {p.location, p.right, p.up, p.forward};
    double* dst[4] = {out->location, out->right, out->up, out->forward};
    for (int i = 0; i < 4; ++i) {
        dst[i][0] = v[i].x;
        dst[i][1] = v[i].y;
        dst[i][2] = v[i].z;
    }
    out->film_distance = p.film_distance;
}
bool too_many(uint64_t w, uint64_t h) { return w > rp::kMaxPixels || h > rp::kMaxPixels || w * h > rp::kMaxPixels; }
}  // namespace

int vrh::reproject_check(const vr_reproject_params* p, const void* state, const void* features,
                         const void* previous_state, const void* previous_features, const void* motion,
                         const void* out_state, bool aligned, rp::Consts* k) {
    if (!p || !state || !features || !previous_state || !previous_features || !out_state)
        return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: null argument");
    if (!motion && p->motion_count > 0) return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: motion_count without motion rows");
    if (out_state == previous_state)
        return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: out_state may not be previous_state, which is gathered");
    if (p->flags & ~VR_REPROJECT_MATCH_OBJECT) return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: unknown flag");
    for (const double tolerance : {p->depth_tolerance, p->normal_tolerance})
        if (!(tolerance > 0.0) || !std::isfinite(tolerance))
            return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: a tolerance is not finite or not positive");
    if (!(p->max_history_weight > 0.0))  // false for a NaN; +inf passes
        return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: max_history_weight is NaN or not positive");
    for (const vr_camera_pose* pose : {&p->pose, &p->previous_pose})
        if (const char* why = pose_error(*pose)) return fail(VR_ERROR_INVALID_ARGUMENT, std::string("reproject: ") + why);
    if (aligned && (((uintptr_t)state | (uintptr_t)features | (uintptr_t)previous_state | (uintptr_t)previous_features |
                     (uintptr_t)motion | (uintptr_t)out_state) & 15))
        return fail(VR_ERROR_INVALID_ARGUMENT, "reproject: device arrays must be 16-byte aligned");
    const bool empty = p->width == 0 || p->height == 0;
    if (!empty && too_many(p->width, p->height)) return fail(VR_ERROR_UNSUPPORTED, "reproject: more than 2^31 pixels");
    copy_pose(p->pose, &k->pose);
    copy_pose(p->previous_pose, &k->previous);
    const rp::Pose &a = k->pose, &b = k->previous;
    bool same = a.film_distance == b.film_distance;
    for (int i = 0; i < 3; ++i)
        same = same && a.location[i] == b.location[i] && a.right[i] == b.right[i] && a.up[i] == b.up[i] &&
               a.forward[i] == b.forward[i];
    k->same_pose = same ? 1u : 0u;
    k->reserved = 0;
    k->film[0] = k->film[1] = k->film[2] = k->film[3] = 0.0;
    if (!empty) vr::camera::film_constants(p->width, p->height, k->film);
    k->dt2 = p->depth_tolerance * p->depth_tolerance;
    k->nt2 = p->normal_tolerance * p->normal_tolerance;
    k->cap = p->max_history_weight;
    k->width = p->width;
    k->height = p->height;
    k->n = empty ? 0 : p->width * p->height;
    k->flags = p->flags;
    k->motion_count = p->motion_count;
    return VR_OK;
}

int vr_reproject_default_params(uint64_t width, uint64_t height, const vr_camera_pose* pose,
                                const vr_camera_pose* previous_pose, vr_reproject_params* out) {
    if (!pose || !previous_pose || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    out->width = width;
    out->height = height;
    out->pose = *pose;
    out->previous_pose = *previous_pose;
    // tools/reproject_bench.py --sweep ("Temporal reprojection")
    out->depth_tolerance = 0.05;
    out->normal_tolerance = 0.25;
    out->max_history_weight = 64.0;
    out->flags = VR_REPROJECT_MATCH_OBJECT;
    out->motion_count = 0;
    return VR_OK;
}

namespace {
struct HostQuads {  // a feature record of a host array, which need not be 16-byte aligned
    const vr_pixel_features* record;
    rp::D2 quad(int i) const {
        rp::D2 d;
        std::memcpy(&d, (const char*)record + 16 * i, 16);
        return d;
    }
};
struct HostPrev {
    const double* state_;
    const vr_pixel_features* features_;
    rp::D2 state(int64_t q, int half) const { return rp::D2{state_[4 * q + 2 * half], state_[4 * q + 2 * half + 1]}; }
    rp::D2 feature(int64_t q, int i) const { return HostQuads{features_ + q}.quad(i); }
};
}  // namespace

int vr_reproject_host(const vr_reproject_params* p, const double* state, const vr_pixel_features* features,
                      const double* previous_state, const vr_pixel_features* previous_features, const double* motion,
                      double* out_state) {
    rp::Consts k;
    const int rc = reproject_check(p, state, features, previous_state, previous_features, motion, out_state, false, &k);
    if (rc) return rc;
    const HostPrev prev = {previous_state, previous_features};
    const int64_t width = (int64_t)k.width, height = (int64_t)k.height;
    for (int64_t row = 0; row < (k.n ? height : 0); ++row)
        for (int64_t column = 0; column < width; ++column) {
            const uint64_t i = (uint64_t)(row * width + column);
            const double* s = state + 4 * i;
            rp::D2 lo, hi;
            rp::reproject_pixel(k, rp::D2{s[0], s[1]}, rp::D2{s[2], s[3]}, HostQuads{features + i}, prev, motion, row,
                                column, &lo, &hi);
            double* o = out_state + 4 * i;
            o[0] = lo.x;
            o[1] = lo.y;
            o[2] = hi.x;
            o[3] = hi.y;
            for (int j = 0; j < 4; ++j) out_state[4 * k.n + 4 * i + j] = 0.0;
        }
    return VR_OK;
}
