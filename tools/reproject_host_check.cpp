// reproject_host_check.cpp -- vr_reproject_host as a stand-alone program, for a run under the host sanitizers
// (tools/reproject_asan.sh builds it with vanrijn_amd/csrc/vr_host_reproject.cpp alone,
// -fsanitize=address,undefined, and runs it on the CPU).  A few of the shapes of tests/test_reproject_host.py on
// a synthetic floor seen from two poses -- identical, a small step, a turn that carries part of the image out
// of frame, a previous camera turned away -- with the special values in a corner and in an interior pixel,
// with and without the flag, every cap, motion rows, in place and out of place, guard values after the
// output, and the argument errors.  No device call exists in what it links.  Exit status 0: every check held.
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
static const double kNaN = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

static vr_camera_pose yawed(double degrees, vr_vec3 location) {
    const double t = degrees * 3.14159265358979323846 / 180.0, c = std::cos(t), s = std::sin(t);
    return vr_camera_pose{location, vr_vec3{c, 0.0, -s}, vr_vec3{0.0, 1.0, 0.0}, vr_vec3{s, 0.0, c}, 1.0};
}

// a floor 1 below the camera: the lower rows hit it at a depth that grows towards the horizon, the upper rows are sky
static void fill_frame(uint64_t w, uint64_t h, std::vector<double>& state, std::vector<vr_pixel_features>& feat) {
    for (uint64_t p = 0; p < w * h; ++p) {
        const uint64_t row = p / w;
        const double wt = 1.0 + std::floor(4.0 * uniform());
        for (int k = 0; k < 3; ++k) state[4 * p + k] = (0.05 + 2.0 * uniform()) * wt;
        state[4 * p + 3] = wt;
        vr_pixel_features& f = feat[p];
        f = vr_pixel_features{};
        f.object = -1;
        f.primitive = -1;
        f.samples = 3;
        if (2 * row >= h || h == 1) {
            f.hits = 1 + (uint32_t)(3.0 * uniform());
            f.normal_sum[1] = (double)f.hits;
            f.distance_sum = (1.5 + 6.0 * (double)(h - row) / (double)h) * f.hits;
            f.distance_min = f.distance_sum / f.hits;
            f.object = (int32_t)(p % 2);
            f.primitive = 0;
        }
    }
}

static int run(uint64_t w, uint64_t h, const vr_camera_pose& pose, const vr_camera_pose& previous, uint32_t flags,
               double cap, bool with_motion, bool in_place) {
    const uint64_t n = w * h;
    std::vector<double> state(8 * n + 4, kGuard), prev(8 * n, 0.5), out(8 * n + 4, kGuard);
    std::vector<vr_pixel_features> feat(n), pfeat(n);
    fill_frame(w, h, state, feat);
    fill_frame(w, h, prev, pfeat);
    // the special values, each in a corner and in an interior pixel (the same pixel on a 1 x 1 image)
    const uint64_t corner[4] = {0, w - 1, (h - 1) * w, n - 1};
    const uint64_t mid = (h * 3 / 4) * w + w / 2, inner[4] = {mid, mid ? mid - 1 : 0, mid >= w ? mid - w : 0, mid + 1 < n ? mid + 1 : mid};
    for (int j = 0; j < 2; ++j) {
        const uint64_t* at = j ? inner : corner;
        prev[4 * at[0] + 1] = kNaN;
        prev[4 * at[1] + 3] = kInf;
        pfeat[at[2]].normal_sum[0] = kNaN;
        feat[at[3]].distance_sum = j ? kNaN : 0.0;
    }
    if (n > 8) {
        feat[n - 2].hits = 0;         // background
        state[4 * (n - 3) + 3] = 0.0;  // absent now
        prev[4 * (n - 4) + 3] = 0.0;   // absent before
        feat[n - 5].normal_sum[2] = kNaN;
    }
    // object 0 slid sideways, object 1 stayed (the identity row), object 2 does not exist
    const double motion[36] = {1, 0, 0, 0.05, 0, 1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0,
                               kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN};
    vr_reproject_params p;
    CHECK(vr_reproject_default_params(w, h, &pose, &previous, &p) == 0);
    p.flags = flags;
    p.max_history_weight = cap;
    p.motion_count = with_motion ? 2 : 0;
    double* dst = in_place ? state.data() : out.data();
    CHECK(vr_reproject_host(&p, state.data(), feat.data(), prev.data(), pfeat.data(), with_motion ? motion : nullptr, dst) == 0);
    for (int g = 0; g < 4; ++g) CHECK(dst[8 * n + g] == kGuard);
    for (uint64_t q = 0; q < n; ++q) {
        for (int k = 0; k < 4; ++k) CHECK(dst[4 * q + k] == dst[4 * q + k]);  // every current sum was finite: no NaN comes out
        for (int k = 0; k < 4; ++k) CHECK(dst[4 * n + 4 * q + k] == 0.0);
    }
    return 0;
}

int main() {
    const uint64_t shapes[5][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 5}, {37, 29}};
    const vr_camera_pose base = yawed(0.0, vr_vec3{0, 0, 0});
    const vr_camera_pose pairs[4][2] = {{base, base},
                                        {yawed(1.0, vr_vec3{0.02, 0.01, -0.01}), base},
                                        {yawed(25.0, vr_vec3{0, 0, 0}), base},
                                        {base, yawed(180.0, vr_vec3{0, 0, 0})}};
    for (const auto& s : shapes)
        for (const auto& pair : pairs)
            for (uint32_t flags : {0u, VR_REPROJECT_MATCH_OBJECT})
                for (double cap : {kInf, 8.0, 0.5})
                    for (int variant = 0; variant < 4; ++variant)
                        if (run(s[0], s[1], pair[0], pair[1], flags, cap, (variant & 1) != 0, (variant & 2) != 0)) return 1;
    // the errors, and the empty image
    vr_reproject_params p;
    double one[8] = {1, 1, 1, 1, 0, 0, 0, 0}, before[8] = {1, 1, 1, 1, 0, 0, 0, 0};
    double o[8] = {kGuard, kGuard, kGuard, kGuard, kGuard, kGuard, kGuard, kGuard};
    vr_pixel_features f{}, pf{};
    CHECK(vr_reproject_default_params(1, 1, &base, &base, &p) == 0);
    CHECK(vr_reproject_default_params(1, 1, nullptr, &base, &p) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_reproject_host(nullptr, one, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_reproject_host(&p, nullptr, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_reproject_host(&p, one, &f, before, nullptr, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_reproject_host(&p, one, &f, o, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.motion_count = 1;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.motion_count = 0;
    p.flags = 2;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.flags = 0;
    p.depth_tolerance = kNaN;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.depth_tolerance = 0.05;
    p.max_history_weight = 0.0;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.max_history_weight = kInf;
    p.previous_pose.up.y = 1.5;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_ERROR_INVALID_ARGUMENT);
    p.previous_pose.up.y = 1.0;
    p.width = 1ull << 40;
    p.height = 1ull << 40;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_ERROR_UNSUPPORTED);
    p.width = 0;
    CHECK(vr_reproject_host(&p, one, &f, before, &pf, nullptr, o) == VR_OK);
    for (double v : o) CHECK(v == kGuard);
    std::puts("reproject_host_check: ok");
    return 0;
}
