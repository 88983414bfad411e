// vr_reproject.hip -- the temporal reprojection's device forms (gfx950): vr_reproject_device and the staged
// vr_reproject.  The rule is vr_reproject.h's, the same inline functions vr_reproject_host compiles.
//
// One kernel, one lane per pixel: a workgroup is 4 rows x 64 columns and a wave owns 64 consecutive columns of
// a row, like the denoiser's direct form.  A lane reads its own records -- the state's two sums quads and
// the feature record's quads 2, 0, 1 (and 3 when an object id is needed), consecutive across the wave -- and
// then gathers up to four previous-frame taps.  Neighbouring lanes project to neighbouring previous pixels,
// so a wave's tap (0,0) is a run of about 64 consecutive records of a previous row (tap (0,1) the same run
// one record on, taps (1,*) the row below): near-coalesced, the fourfold reuse left to the caches.  Every
// state and feature access is a 16-B load or store; a tap's loads stop at the first test that fails
// (vr_reproject.h).  No LDS, no workspace, no scratch.  Compiled with -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>

#include "vr_reproject.h"
#include "vr_host.h"

namespace vr {
namespace dev {

namespace rp = vr::reproject;

struct ReprojectArgs {
    rp::Consts k;
    const rp::D2* state;              // the sums half, two quads per pixel
    const rp::D2* features;           // four quads per pixel
    const rp::D2* previous_state;
    const rp::D2* previous_features;
    const double* motion;             // null, or k.motion_count rows of 12
    rp::D2* out_state;
};

struct DeviceQuads {
    const rp::D2* record;
    __device__ rp::D2 quad(int i) const { return record[i]; }
};
struct DevicePrev {
    const rp::D2* state_;
    const rp::D2* features_;
    __device__ rp::D2 state(int64_t q, int half) const { return state_[2 * q + half]; }
    __device__ rp::D2 feature(int64_t q, int i) const { return features_[4 * q + i]; }
};

// blocks_x workgroups of 64 columns across, 4 rows each
__global__ __launch_bounds__(256) void reproject_kernel(ReprojectArgs A, uint32_t blocks_x) {
    const int tid = threadIdx.x;
    const uint32_t by = blockIdx.x / blocks_x, bx = blockIdx.x - by * blocks_x;
    const int64_t column = (int64_t)bx * 64 + (tid & 63), row = (int64_t)by * 4 + (tid >> 6);
    if (column >= (int64_t)A.k.width || row >= (int64_t)A.k.height) return;
    const int64_t p = row * (int64_t)A.k.width + column;
    const rp::D2 s_lo = A.state[2 * p], s_hi = A.state[2 * p + 1];
    rp::D2 o_lo, o_hi;
    rp::reproject_pixel(A.k, s_lo, s_hi, DeviceQuads{A.features + 4 * p}, DevicePrev{A.previous_state, A.previous_features},
                        A.motion, row, column, &o_lo, &o_hi);
    const int64_t n = (int64_t)A.k.n;
    A.out_state[2 * p] = o_lo;
    A.out_state[2 * p + 1] = o_hi;
    A.out_state[2 * n + 2 * p] = rp::D2{0.0, 0.0};
    A.out_state[2 * n + 2 * p + 1] = rp::D2{0.0, 0.0};
}

}  // namespace dev
}  // namespace vr

using namespace vrh;
namespace rp = vr::reproject;

namespace {

// a launch holds fewer than 2^32 lanes, and a 64 x 4 block is spent on every started block (as the denoiser)
bool too_thin(const rp::Consts& k) { return ((k.width + 63) / 64) * ((k.height + 3) / 4) >= (1ull << 24); }

int enqueue(const rp::Consts& k, const double* state, const vr_pixel_features* features, const double* previous_state,
            const vr_pixel_features* previous_features, const double* motion, double* out_state, hipStream_t st) {
    vr::dev::ReprojectArgs a;
    a.k = k;
    a.state = reinterpret_cast<const rp::D2*>(state);
    a.features = reinterpret_cast<const rp::D2*>(features);
    a.previous_state = reinterpret_cast<const rp::D2*>(previous_state);
    a.previous_features = reinterpret_cast<const rp::D2*>(previous_features);
    a.motion = motion;
    a.out_state = reinterpret_cast<rp::D2*>(out_state);
    const uint32_t bx = (uint32_t)((k.width + 63) / 64);
    const uint64_t rows = (k.height + 3) / 4;
    hipLaunchKernelGGL(vr::dev::reproject_kernel, dim3((unsigned)(bx * rows)), dim3(256), 0, st, a, bx);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return device_fail((int)e, "reproject launch failed");
    return VR_OK;
}

}  // namespace

int vr_reproject_device(const vr_reproject_params* p, const double* state, const vr_pixel_features* features,
                        const double* previous_state, const vr_pixel_features* previous_features, const double* motion,
                        double* out_state, int32_t device, void* stream) {
    rp::Consts k;
    const int rc = reproject_check(p, state, features, previous_state, previous_features, motion, out_state, true, &k);
    if (rc) return rc;
    if (k.n == 0) return VR_OK;
    if (too_thin(k)) return fail(VR_ERROR_UNSUPPORTED, "reproject: more than 2^24 - 1 blocks of 64 x 4 pixels");
    VR_HIP(hipSetDevice(device));
    return enqueue(k, state, features, previous_state, previous_features, motion, out_state, (hipStream_t)stream);
}

int vr_reproject(const vr_reproject_params* p, const double* state, const vr_pixel_features* features,
                 const double* previous_state, const vr_pixel_features* previous_features, const double* motion,
                 double* out_state, int32_t device) {
    rp::Consts k;
    const int rc = reproject_check(p, state, features, previous_state, previous_features, motion, out_state, false, &k);
    if (rc) return rc;
    const uint64_t n = k.n;
    if (n == 0) return VR_OK;
    if (too_thin(k)) return fail(VR_ERROR_UNSUPPORTED, "reproject: more than 2^24 - 1 blocks of 64 x 4 pixels");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(VR_ERROR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(VR_ERROR_INVALID_ARGUMENT, "device out of range");
    VR_HIP(hipSetDevice(device));
    CallScratch cs;
    VR_HIP(hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking));
    // [records: the state's sums half in, the output out | features | the previous sums half | previous features | motion]
    const size_t rec_b = (size_t)n * 64, half_b = (size_t)n * 32;
    const size_t motion_b = motion ? (size_t)k.motion_count * 96 : 0;
    VR_HIP(hipMalloc(&cs.ptr, 3 * rec_b + half_b + motion_b + 16));
    char* base = (char*)cs.ptr;
    double* d_state = (double*)base;
    vr_pixel_features* d_feat = (vr_pixel_features*)(base + rec_b);
    vr_pixel_features* d_pfeat = (vr_pixel_features*)(base + 2 * rec_b);
    double* d_prev = (double*)(base + 3 * rec_b);
    double* d_motion = (double*)(base + 3 * rec_b + half_b);  // (a non-null place even for zero rows)
    VR_HIP(hipMemcpyAsync(d_state, state, half_b, hipMemcpyHostToDevice, cs.stream));
    VR_HIP(hipMemcpyAsync(d_feat, features, rec_b, hipMemcpyHostToDevice, cs.stream));
    VR_HIP(hipMemcpyAsync(d_pfeat, previous_features, rec_b, hipMemcpyHostToDevice, cs.stream));
    VR_HIP(hipMemcpyAsync(d_prev, previous_state, half_b, hipMemcpyHostToDevice, cs.stream));
    if (motion_b) VR_HIP(hipMemcpyAsync(d_motion, motion, motion_b, hipMemcpyHostToDevice, cs.stream));
    const int e = enqueue(k, d_state, d_feat, d_prev, d_pfeat, motion ? d_motion : nullptr, d_state, cs.stream);
    if (e) {
        (void)hipStreamSynchronize(cs.stream);  // the copies read the caller's arrays
        return e;
    }
    VR_HIP(hipMemcpyAsync(out_state, d_state, rec_b, hipMemcpyDeviceToHost, cs.stream));
    VR_HIP(hipStreamSynchronize(cs.stream));
    return VR_OK;
}
