// vr_denoise.hip -- the denoiser's device forms (gfx950): vr_denoise_device, vr_denoise_stage_device and the
// staged vr_denoise.  The rule is vr_denoise.h's, the same inline functions vr_denoise_host compiles.
//
// Kernels, one lane per pixel throughout:
//   denoise_prepare_kernel   state, feature records and albedo -> the workspace's 32-B records
//   denoise_direct_kernel    one iteration; a workgroup is 4 rows x 64 columns, a wave owns 64 consecutive
//                            columns of a row, so the taps of a wave are contiguous runs at any step and the
//                            loads coalesce; the 25-fold reuse is left to the caches
//   denoise_lds_kernel       one iteration; a workgroup owns 128 consecutive columns of one row and first
//                            stages its five tap rows (the run plus 2 * step columns of halo on each side)
//                            in LDS as four planes of 16-B quads, so every ds_read_b128 of a wave is one
//                            contiguous run; steps up to VR_DENOISE_LDS_MAX_STEP fit the 64 KiB of a launch
//   denoise_finish_kernel    remodulates and writes the output records
// Compiled with -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>

#include "vr_denoise.h"
#include "vr_host.h"

namespace vr {
namespace dev {

namespace dn = vr::denoise;

__constant__ double c_denoise_exp_tab[64] = VR_EXP_TABLE_INIT;

struct DenoiseArgs {
    dn::Consts k;
    const dn::D2* state;           // the sums half, two quads per pixel
    const dn::FeatureRecord* features;
    const dn::D2* albedo;          // null without VR_DENOISE_DEMODULATE
    dn::D2* out_state;
    dn::Colour* buf[2];
    dn::Guide* guide;
    dn::Extra* extra;
};

__global__ __launch_bounds__(256) void denoise_prepare_kernel(DenoiseArgs A) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.k.n) return;
    const bool demodulate = A.albedo != nullptr;
    const dn::D2 s_lo = A.state[2 * p], s_hi = A.state[2 * p + 1];
    dn::D2 a_lo = s_lo, a_hi = s_hi;
    if (demodulate) {
        a_lo = A.albedo[2 * p];
        a_hi = A.albedo[2 * p + 1];
    }
    dn::Colour c;
    dn::Guide g;
    dn::Extra e;
    dn::prepare_pixel(s_lo, s_hi, A.features[p], a_lo, a_hi, demodulate, &c, &g, &e);
    A.buf[0][p] = c;
    A.guide[p] = g;
    A.extra[p] = e;
}

__global__ __launch_bounds__(256) void denoise_finish_kernel(DenoiseArgs A, int from) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= A.k.n) return;
    const bool demodulate = A.albedo != nullptr;
    dn::D2 lo, hi;
    dn::finish_pixel(A.buf[from][p], demodulate ? A.extra[p] : dn::Extra{{0.0, 0.0}, {0.0, 0.0}}, demodulate, &lo, &hi);
    A.out_state[2 * p] = lo;
    A.out_state[2 * p + 1] = hi;
    A.out_state[2 * A.k.n + 2 * p] = dn::D2{0.0, 0.0};
    A.out_state[2 * A.k.n + 2 * p + 1] = dn::D2{0.0, 0.0};
}

struct DirectLoad {
    const dn::Colour* colour_;
    const dn::Guide* guide_;
    const dn::Extra* extra_;
    int64_t width;
    __device__ dn::Colour colour(int64_t x, int64_t y) const { return colour_[y * width + x]; }
    __device__ dn::Guide guide(int64_t x, int64_t y) const { return guide_[y * width + x]; }
    __device__ double iz(int64_t x, int64_t y) const { return extra_[y * width + x].lo.x; }
};

// blocks_x workgroups of 64 columns across, 4 rows each
__global__ __launch_bounds__(256) void denoise_direct_kernel(DenoiseArgs A, int from, int step, double kc, uint32_t blocks_x) {
    __shared__ double etab[64];  // 2^(j/64) for vr_exp_tab
    const int tid = threadIdx.x;
    if (tid < 64) etab[tid] = c_denoise_exp_tab[tid];
    __syncthreads();
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const int64_t x = (int64_t)bx * 64 + (tid & 63), y = (int64_t)by * 4 + (tid >> 6);
    if (x >= (int64_t)A.k.width || y >= (int64_t)A.k.height) return;
    const DirectLoad load = {A.buf[from], A.guide, A.extra, (int64_t)A.k.width};
    A.buf[from ^ 1][y * (int64_t)A.k.width + x] = dn::fold_pixel(load, x, y, A.k, step, kc, etab);
}

constexpr int kLdsRun = 128;  // columns of a workgroup of the LDS form

struct LdsLoad {
    const dn::D2* plane;  // [4 planes][5 rows][span] quads: colour lo, colour hi, guide lo, guide hi
    const dn::Extra* extra_;
    int64_t width, x_first, y_centre;  // the image column of staged column 0; the workgroup's row
    int step, span;
    __device__ int at(int64_t x, int64_t y) const {
        const int r = (int)((y - y_centre) / step) + 2;
        return r * span + (int)(x - x_first);
    }
    __device__ dn::Colour colour(int64_t x, int64_t y) const {
        const int i = at(x, y);
        return dn::Colour{plane[i], plane[5 * span + i]};
    }
    __device__ dn::Guide guide(int64_t x, int64_t y) const {
        const int i = at(x, y);
        return dn::Guide{plane[10 * span + i], plane[15 * span + i]};
    }
    __device__ double iz(int64_t x, int64_t y) const { return extra_[y * width + x].lo.x; }
};

// blocks_x workgroups of kLdsRun columns across, one row each; dynamic LDS: 20 * span quads, span = kLdsRun + 4 * step
__global__ __launch_bounds__(kLdsRun) void denoise_lds_kernel(DenoiseArgs A, int from, int step, double kc, uint32_t blocks_x) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ double etab[64];
    dn::D2* const plane = reinterpret_cast<dn::D2*>(lds_raw);
    const int tid = threadIdx.x;
    if (tid < 64) etab[tid] = c_denoise_exp_tab[tid];
    const int64_t width = (int64_t)A.k.width, height = (int64_t)A.k.height;
    const int64_t y = blockIdx.x / blocks_x;
    const int64_t x0 = (int64_t)(blockIdx.x - (uint32_t)y * blocks_x) * kLdsRun;
    const int span = kLdsRun + 4 * step;
    const int64_t x_first = x0 - 2 * step;
    const dn::Colour* const in = A.buf[from];
    for (int r = 0; r < 5; ++r) {
        const int64_t qy = y + (int64_t)(r - 2) * step;
        if (qy < 0 || qy >= height) continue;  // never read: fold_pixel skips taps outside the image
        for (int j = tid; j < span; j += kLdsRun) {
            const int64_t qx = x_first + j;
            if (qx < 0 || qx >= width) continue;
            const dn::Colour c = in[qy * width + qx];
            const dn::Guide g = A.guide[qy * width + qx];
            plane[r * span + j] = c.lo;
            plane[5 * span + r * span + j] = c.hi;
            plane[10 * span + r * span + j] = g.lo;
            plane[15 * span + r * span + j] = g.hi;
        }
    }
    __syncthreads();
    const int64_t x = x0 + tid;
    if (x >= width) return;
    const LdsLoad load = {plane, A.extra, width, x_first, y, step, span};
    A.buf[from ^ 1][y * width + x] = dn::fold_pixel(load, x, y, A.k, step, kc, etab);
}

}  // namespace dev
}  // namespace vr

using namespace vrh;
namespace dn = vr::denoise;

namespace {

// Which steps stage their taps in LDS when the caller leaves the choice to the library: none.  Measured on
// one MI355X at 1024 x 1024 (tools/denoise_bench.py, profiles/r14/denoise/denoise_bench.json): the direct form
// takes 0.076-0.088 ms per iteration, the LDS form 0.160-0.217 ms, 2.0-2.5 times as long at every step
// ("Denoiser").
bool lds_wins(uint32_t /*iteration*/) { return false; }

bool takes_lds(uint32_t flags, uint32_t iteration) {
    if ((1u << iteration) > VR_DENOISE_LDS_MAX_STEP) return false;
    if (flags & VR_DENOISE_LOADS_LDS) return true;
    if (flags & VR_DENOISE_LOADS_DIRECT) return false;
    return lds_wins(iteration);
}

// a launch holds fewer than 2^32 lanes, and the direct form spends a 64 x 4 block on every started block
bool too_thin(const dn::Consts& k) { return ((k.width + 63) / 64) * ((k.height + 3) / 4) >= (1ull << 24); }

// stages [first, last] of the call: 0 prepare, 1 .. iterations the iterations, iterations + 1 finish
int enqueue_stages(const dn::Consts& k, uint32_t first, uint32_t last, const double* state,
                   const vr_pixel_features* features, const double* albedo_state, double* out_state, void* workspace,
                   hipStream_t st) {
    vr::dev::DenoiseArgs a;
    a.k = k;
    a.state = reinterpret_cast<const dn::D2*>(state);
    a.features = reinterpret_cast<const dn::FeatureRecord*>(features);
    a.albedo = (k.flags & VR_DENOISE_DEMODULATE) ? reinterpret_cast<const dn::D2*>(albedo_state) : nullptr;
    a.out_state = reinterpret_cast<dn::D2*>(out_state);
    a.buf[0] = reinterpret_cast<dn::Colour*>(workspace);
    a.buf[1] = a.buf[0] + k.n;
    a.guide = reinterpret_cast<dn::Guide*>(a.buf[1] + k.n);
    a.extra = reinterpret_cast<dn::Extra*>(a.guide + k.n);
    const dim3 flat((unsigned)((k.n + 255) / 256));
    for (uint32_t stage = first; stage <= last; ++stage) {
        if (stage == 0) {
            hipLaunchKernelGGL(vr::dev::denoise_prepare_kernel, flat, dim3(256), 0, st, a);
        } else if (stage == k.iterations + 1) {
            hipLaunchKernelGGL(vr::dev::denoise_finish_kernel, flat, dim3(256), 0, st, a, (int)(k.iterations & 1));
        } else {
            const uint32_t it = stage - 1;
            const int step = 1 << it, from = (int)(it & 1);
            const double kc = dn::colour_scale(k, it);
            const uint32_t bx_lds = (uint32_t)((k.width + vr::dev::kLdsRun - 1) / vr::dev::kLdsRun);
            // (a launch holds fewer than 2^32 lanes: a very tall, thin image stays with the direct form)
            if (takes_lds(k.flags, it) && (uint64_t)bx_lds * k.height < (1ull << 25)) {
                const uint32_t bx = bx_lds;
                const size_t lds = (size_t)20 * (vr::dev::kLdsRun + 4 * step) * sizeof(dn::D2);
                hipLaunchKernelGGL(vr::dev::denoise_lds_kernel, dim3((unsigned)(bx * k.height)), dim3(vr::dev::kLdsRun), lds,
                                   st, a, from, step, kc, bx);
            } else {
                const uint32_t bx = (uint32_t)((k.width + 63) / 64);
                const uint64_t rows = (k.height + 3) / 4;
                hipLaunchKernelGGL(vr::dev::denoise_direct_kernel, dim3((unsigned)(bx * rows)), dim3(256), 0, st, a, from,
                                   step, kc, bx);
            }
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return device_fail((int)e, "denoise launch failed");
    }
    return VR_OK;
}

int denoise_stages(const vr_denoise_params* p, bool one, uint32_t stage, const double* state,
                   const vr_pixel_features* features, const double* albedo_state, double* out_state, void* workspace,
                   int32_t device, void* stream) {
    dn::Consts k;
    const int rc = denoise_check(p, state, features, albedo_state, out_state, true, &k);
    if (rc) return rc;
    if (one && stage > k.iterations + 1) return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: no such stage");
    if (k.n == 0) return VR_OK;
    if (too_thin(k)) return fail(VR_ERROR_UNSUPPORTED, "denoise: more than 2^24 - 1 blocks of 64 x 4 pixels");
    if (!workspace) return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: null workspace");
    if ((uintptr_t)workspace & 15) return fail(VR_ERROR_INVALID_ARGUMENT, "denoise: device arrays must be 16-byte aligned");
    VR_HIP(hipSetDevice(device));
    return enqueue_stages(k, one ? stage : 0, one ? stage : k.iterations + 1, state, features, albedo_state, out_state,
                          workspace, (hipStream_t)stream);
}

}  // namespace

int vr_denoise_device(const vr_denoise_params* p, const double* state, const vr_pixel_features* features,
                      const double* albedo_state, double* out_state, void* workspace, int32_t device, void* stream) {
    return denoise_stages(p, false, 0, state, features, albedo_state, out_state, workspace, device, stream);
}

int vr_denoise_stage_device(const vr_denoise_params* p, uint32_t stage, const double* state,
                            const vr_pixel_features* features, const double* albedo_state, double* out_state,
                            void* workspace, int32_t device, void* stream) {
    return denoise_stages(p, true, stage, state, features, albedo_state, out_state, workspace, device, stream);
}

int vr_denoise(const vr_denoise_params* p, const double* state, const vr_pixel_features* features,
               const double* albedo_state, double* out_state, int32_t device) {
    dn::Consts k;
    const int rc = denoise_check(p, state, features, albedo_state, out_state, false, &k);
    if (rc) return rc;
    const uint64_t n = k.n;
    if (n == 0) return VR_OK;
    if (too_thin(k)) return fail(VR_ERROR_UNSUPPORTED, "denoise: more than 2^24 - 1 blocks of 64 x 4 pixels");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(VR_ERROR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(VR_ERROR_INVALID_ARGUMENT, "device out of range");
    VR_HIP(hipSetDevice(device));
    CallScratch cs;
    VR_HIP(hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking));
    // [records: the state's sums half in, the output out | features | the albedo's sums half | workspace]
    const bool demodulate = (k.flags & VR_DENOISE_DEMODULATE) != 0;
    const size_t rec_b = (size_t)n * 64, half_b = (size_t)n * 32, ws_b = (size_t)n * dn::kWorkspacePerPixel;
    VR_HIP(hipMalloc(&cs.ptr, rec_b + rec_b + half_b + ws_b));
    char* base = (char*)cs.ptr;
    double* d_state = (double*)base;
    vr_pixel_features* d_feat = (vr_pixel_features*)(base + rec_b);
    double* d_albedo = (double*)(base + 2 * rec_b);
    void* d_ws = base + 2 * rec_b + half_b;
    VR_HIP(hipMemcpyAsync(d_state, state, half_b, hipMemcpyHostToDevice, cs.stream));
    VR_HIP(hipMemcpyAsync(d_feat, features, rec_b, hipMemcpyHostToDevice, cs.stream));
    if (demodulate) VR_HIP(hipMemcpyAsync(d_albedo, albedo_state, half_b, hipMemcpyHostToDevice, cs.stream));
    const int e = enqueue_stages(k, 0, k.iterations + 1, d_state, d_feat, demodulate ? d_albedo : nullptr, d_state, d_ws,
                                 cs.stream);
    if (e) {
        (void)hipStreamSynchronize(cs.stream);  // the copies read the caller's arrays
        return e;
    }
    VR_HIP(hipMemcpyAsync(out_state, d_state, rec_b, hipMemcpyDeviceToHost, cs.stream));
    VR_HIP(hipStreamSynchronize(cs.stream));
    return VR_OK;
}
