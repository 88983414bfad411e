// denoise_host_check.cpp -- vr_denoise_host as a stand-alone program, for a run under the host sanitizers
// (tools/denoise_asan.sh builds it with vanrijn_amd/csrc/vr_host_denoise.cpp alone, -fsanitize=address,undefined,
// and runs it on the CPU).  A few of the shapes of tests/test_denoise_host.py with the special values in a
// corner and in an interior pixel, every flag, in place and out of place, guard values after the output, and
// the argument errors.  No device call exists in what it links.  Exit status 0: every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../include/vanrijn_amd.h"

// the library's error sink (vr_host_io.cpp), which this program does not link
namespace vrh {
static std::string last;
int fail(int code, const std::string& msg) {
    last = msg;
    return code;
}
}  // namespace vrh

#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, vrh::last.c_str()); \
            return 1;                                                                                    \
        }                                                                                                \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {  // xorshift64*, in [0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * 0x1.0p-53;
}

static const double kGuard = 1234.5;

static int run(uint64_t w, uint64_t h, uint32_t iterations, uint32_t flags, bool in_place) {
    const uint64_t n = w * h;
    std::vector<double> state(8 * n + 4, kGuard), albedo(8 * n), out(8 * n + 4, kGuard);
    std::vector<vr_pixel_features> feat(n);
    for (uint64_t p = 0; p < n; ++p) {
        const uint64_t x = p % w;
        const double wt = 1.0 + std::floor(3.0 * uniform()), aw = std::floor(3.0 * uniform());
        for (int k = 0; k < 3; ++k) {
            state[4 * p + k] = (0.05 + 2.0 * uniform()) * wt;
            albedo[4 * p + k] = (uniform() < 0.2 ? 1e-4 : 0.2 + 0.7 * uniform()) * aw;
        }
        state[4 * p + 3] = wt;
        albedo[4 * p + 3] = aw;
        const uint32_t region = (uint32_t)(x * 3 / w);
        vr_pixel_features& f = feat[p];
        f = vr_pixel_features{};
        f.hits = 1 + (uint32_t)(2.0 * uniform());
        f.samples = f.hits;
        f.normal_sum[region] = (double)f.hits;
        f.distance_sum = (2.0 + 3.0 * region + 0.05 * (double)(p / w)) * f.hits;
        f.object = (int32_t)region;
    }
    // the special values, each in a corner and in an interior pixel (the same pixel on a 1 x 1 image)
    const uint64_t corner[4] = {0, w - 1, (h - 1) * w, n - 1};
    const uint64_t mid = (h / 2) * w + w / 2, inner[4] = {mid, mid ? mid - 1 : 0, mid >= w ? mid - w : 0, mid + 1 < n ? mid + 1 : mid};
    for (int j = 0; j < 2; ++j) {
        const uint64_t* at = j ? inner : corner;
        state[4 * at[0] + 1] = std::numeric_limits<double>::quiet_NaN();
        state[4 * at[1] + 0] = std::numeric_limits<double>::infinity();
        feat[at[2]].normal_sum[0] = std::numeric_limits<double>::quiet_NaN();
        feat[at[3]].distance_sum = 0.0;
    }
    if (n > 8) {
        feat[1].hits = 0;       // background
        state[4 * 2 + 3] = 0.0;  // absent
    }
    vr_denoise_params p;
    CHECK(vr_denoise_default_params(w, h, &p) == 0);
    p.iterations = iterations;
    p.flags = flags;
    double* dst = in_place ? state.data() : out.data();
    CHECK(vr_denoise_host(&p, state.data(), feat.data(), albedo.data(), dst) == 0);
    for (int g = 0; g < 4; ++g) CHECK(dst[8 * n + g] == kGuard);
    for (uint64_t p2 = 0; p2 < n; ++p2) {
        CHECK(dst[4 * p2 + 3] == 1.0 || dst[4 * p2 + 3] == 0.0);
        for (int k = 0; k < 4; ++k) CHECK(dst[4 * n + 4 * p2 + k] == 0.0);
    }
    return 0;
}

int main() {
    const uint64_t shapes[4][2] = {{1, 1}, {1, 7}, {7, 1}, {37, 29}};
    for (const auto& s : shapes)
        for (uint32_t iterations : {1u, 3u, 8u})
            for (uint32_t flags : {0u, VR_DENOISE_MATCH_OBJECT, VR_DENOISE_DEMODULATE, VR_DENOISE_MATCH_OBJECT | VR_DENOISE_DEMODULATE})
                for (bool in_place : {false, true})
                    if (run(s[0], s[1], iterations, flags, in_place)) return 1;
    // the errors, and the empty image
    vr_denoise_params p;
    double one[8] = {1, 1, 1, 1, 0, 0, 0, 0}, o[8] = {kGuard, kGuard, kGuard, kGuard, kGuard, kGuard, kGuard, kGuard};
    vr_pixel_features f{};
    CHECK(vr_denoise_default_params(1, 1, &p) == 0);
    CHECK(vr_denoise_host(nullptr, one, &f, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_denoise_host(&p, nullptr, &f, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.iterations = 9;
    CHECK(vr_denoise_host(&p, one, &f, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.iterations = 1;
    p.flags = VR_DENOISE_DEMODULATE;
    CHECK(vr_denoise_host(&p, one, &f, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.flags = 0;
    p.sigma_depth = std::numeric_limits<double>::quiet_NaN();
    CHECK(vr_denoise_host(&p, one, &f, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.sigma_depth = 0.1;
    p.width = 1ull << 40;
    p.height = 1ull << 40;
    CHECK(vr_denoise_host(&p, one, &f, nullptr, o) == VR_ERROR_UNSUPPORTED);
    p.width = 0;
    CHECK(vr_denoise_host(&p, one, &f, nullptr, o) == VR_OK);
    for (double v : o) CHECK(v == kGuard);
    uint64_t bytes = 0;
    p.width = 3;
    p.height = 5;
    CHECK(vr_denoise_workspace_bytes(&p, &bytes) == VR_OK && bytes == 15 * 128);
    std::puts("denoise_host_check: ok");
    return 0;
}
