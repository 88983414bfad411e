// vr_host_denoise.cpp -- the denoiser's HIP-free half: the defaults, the workspace size, the checks every
// form shares, and vr_denoise_host, the rule of vr_denoise.h in plain C++ on host arrays (the counterpart
// of the VR_SCENE_HOST_ONLY paths; tools/denoise_host_check.cpp builds this file alone under the host
// sanitizers).  The device forms are in vr_denoise.hip.
#define VR_HOST_NO_HIP
#include <new>

#include "vr_denoise.h"
#include "vr_host.h"

using namespace vrh;
namespace dn = vr::denoise;

int vrh::denoise_check(const vr_denoise_params* p, const void* state, const void* features, const void* albedo_state,
                       const void* out_state, bool aligned, dn::Consts* k) {
    if (!p || !state || !features || !out_state) return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: null argument");
    if (p->iterations < 1 || p->iterations > VR_DENOISE_MAX_ITERATIONS)
        return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: iterations outside 1..8");
    const uint32_t known = VR_DENOISE_MATCH_OBJECT | VR_DENOISE_DEMODULATE | VR_DENOISE_LOADS_DIRECT | VR_DENOISE_LOADS_LDS;
    if (p->flags & ~known) return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: unknown flag");
    if ((p->flags & VR_DENOISE_LOADS_DIRECT) && (p->flags & VR_DENOISE_LOADS_LDS))
        return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: both load forms asked for");
    if ((p->flags & VR_DENOISE_DEMODULATE) && !albedo_state)
        return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: VR_DENOISE_DEMODULATE needs an albedo state");
    for (const double sigma : {p->sigma_colour, p->sigma_normal, p->sigma_depth})
        if (!(sigma > 0.0) || !std::isfinite(sigma))
            return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: a sigma is not finite or not positive");
    if (aligned && (((uintptr_t)state | (uintptr_t)features | (uintptr_t)albedo_state | (uintptr_t)out_state) & 15))
        return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: device arrays must be 16-byte aligned");
    const bool empty = p->width == 0 || p->height == 0;
    if (!empty && (p->width > dn::kMaxPixels || p->height > dn::kMaxPixels || p->width * p->height > dn::kMaxPixels))
        return fail(VR_ERROR_UNSUPPORTED, "denoise: more than 2^31 pixels");
    k->kc0 = 1.0 / (p->sigma_colour * p->sigma_colour);
    k->kn = 1.0 / (p->sigma_normal * p->sigma_normal);
    k->kz = 1.0 / (p->sigma_depth * p->sigma_depth);
    const double hk[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    for (int i = 0; i < 5; ++i) k->hk[i] = hk[i];
    k->width = p->width;
    k->height = p->height;
    k->n = empty ? 0 : p->width * p->height;
    k->iterations = p->iterations;
    k->flags = p->flags;
    return VR_OK;
}

int vr_denoise_default_params(uint64_t width, uint64_t height, vr_denoise_params* out) {
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "null output");
    out->width = width;
    out->height = height;
    out->iterations = 5;
    out->flags = 0;
    out->sigma_colour = 32.0;  // tools/denoise_bench.py --sweep ("Denoiser")
    out->sigma_normal = 0.5;
    out->sigma_depth = 0.1;
    return VR_OK;
}

int vr_denoise_workspace_bytes(const vr_denoise_params* p, uint64_t* out_bytes) {
    if (!p || !out_bytes) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    const bool empty = p->width == 0 || p->height == 0;
    if (!empty && (p->width > dn::kMaxPixels || p->height > dn::kMaxPixels || p->width * p->height > dn::kMaxPixels))
        return fail(VR_ERROR_UNSUPPORTED, "denoise: more than 2^31 pixels");
    *out_bytes = empty ? 0 : p->width * p->height * dn::kWorkspacePerPixel;
    return VR_OK;
}

namespace {
const double kExpTab[64] = VR_EXP_TABLE_INIT;

struct HostLoad {  // the workspace arrays as fold_pixel reads them
    const dn::Colour* colour_;
    const dn::Guide* guide_;
    const dn::Extra* extra_;
    int64_t width;
    dn::Colour colour(int64_t x, int64_t y) const { return colour_[y * width + x]; }
    dn::Guide guide(int64_t x, int64_t y) const { return guide_[y * width + x]; }
    double iz(int64_t x, int64_t y) const { return extra_[y * width + x].lo.x; }
};
}  // namespace

int vr_denoise_host(const vr_denoise_params* p, const double* state, const vr_pixel_features* features,
                    const double* albedo_state, double* out_state) {
    dn::Consts k;
    const int rc = denoise_check(p, state, features, albedo_state, out_state, false, &k);
    if (rc) return rc;
    const uint64_t n = k.n;
    if (n == 0) return VR_OK;
    // the workspace of the device form, 32-B records: [ping][pong][guide][extra]
    dn::Colour* ws = new (std::nothrow) dn::Colour[4 * n];
    if (!ws) return fail(VR_ERROR_OUT_OF_MEMORY, "denoise: workspace allocation failed");
    dn::Colour* buf[2] = {ws, ws + n};
    dn::Guide* guide = reinterpret_cast<dn::Guide*>(ws + 2 * n);
    dn::Extra* extra = reinterpret_cast<dn::Extra*>(ws + 3 * n);
    const bool demodulate = (k.flags & VR_DENOISE_DEMODULATE) != 0;
    for (uint64_t i = 0; i < n; ++i) {
        dn::FeatureRecord f;
        std::memcpy(&f, &features[i], sizeof f);  // a host array need not be 16-byte aligned
        const double* s = state + 4 * i;
        const double* a = demodulate ? albedo_state + 4 * i : s;
        dn::prepare_pixel(dn::D2{s[0], s[1]}, dn::D2{s[2], s[3]}, f, dn::D2{a[0], a[1]}, dn::D2{a[2], a[3]}, demodulate,
                          &buf[0][i], &guide[i], &extra[i]);
    }
    const int64_t width = (int64_t)k.width, height = (int64_t)k.height;
    for (uint32_t it = 0; it < k.iterations; ++it) {
        const HostLoad load = {buf[it & 1], guide, extra, width};
        dn::Colour* out = buf[(it + 1) & 1];
        const double kc = dn::colour_scale(k, it);
        for (int64_t y = 0; y < height; ++y)
            for (int64_t x = 0; x < width; ++x)
                out[y * width + x] = dn::fold_pixel(load, x, y, k, (int64_t)1 << it, kc, kExpTab);
    }
    const dn::Colour* last = buf[k.iterations & 1];
    for (uint64_t i = 0; i < n; ++i) {
        dn::D2 lo, hi;
        dn::finish_pixel(last[i], extra[i], demodulate, &lo, &hi);
        double* o = out_state + 4 * i;
        o[0] = lo.x;
        o[1] = lo.y;
        o[2] = hi.x;
        o[3] = hi.y;
        for (int j = 0; j < 4; ++j) out_state[4 * n + 4 * i + j] = 0.0;
    }
    delete[] ws;
    return VR_OK;
}
