// vr_reduce.hip -- the ordered reduce (gfx950): each sample's staged photon {wavelength, intensity} to XYZ,
// folded into its pixel in sample order with the reference's Kahan update_pixel.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "rgb_spectrum_tables.h"
#include "vr_layout.h"
#include "vr_exp_table.h"

#include "vr_device.h"

namespace vr {
namespace dev {

#ifndef VR_REDUCE_BATCH  // samples whose colours the ordered reduce computes together
#define VR_REDUCE_BATCH 4
#endif
typedef double d2 __attribute__((ext_vector_type(2)));
// accumulation_buffer.rs:44-60 (update_pixel with weight 1.0), one thread per pixel, samples in
// order: the same Kahan sequence the reference applies call by call.  ANY_WL: the photons are a
// caller's and their wavelengths any doubles (xyz_for_wavelength_tab); false for the render's own.
__constant__ double c_exp_tab[64] = VR_EXP_TABLE_INIT;
template <bool ANY_WL>
__global__ __launch_bounds__(256) void accumulate_kernel(double* state, const double* staging, uint64_t npix,
                                                         uint32_t spp, uint32_t accumulate, const uint8_t* mask,
                                                         uint64_t tile_width, const uint32_t* stage_tag,
                                                         uint32_t stage_gen, int32_t* error_flag) {
    // Debug builds (-DVR_STAGE_GUARD): every staged photon the reduce reads must carry this pass's
    // generation -- a slot the render kernel did not write in this pass is a device error (error
    // word bit 3, VR_ERROR_DEVICE "staging guard").  The invariant it checks: the reduce reads
    // slot (s, p) exactly for the pixels p < npix outside culled blocks and the samples s < spp,
    // and the render kernel's item space covers exactly those (pixel, sample) pairs.
#ifdef VR_STAGE_GUARD
    auto guard = [&](uint32_t s, uint64_t p) {
        if (stage_tag[(uint64_t)s * npix + p] != stage_gen) {
            if (atomicOr(error_flag, 8) == 0)
                printf("vr staging guard: pixel %llu sample %u tag %u, pass generation %u\n", (unsigned long long)p, s,
                       stage_tag[(uint64_t)s * npix + p], stage_gen);
            atomicOr(error_flag, 8);
        }
    };
#define VR_GUARD(s, p) guard(s, p)
#else
#define VR_GUARD(s, p) ((void)stage_tag, (void)stage_gen, (void)error_flag)
#endif
    __shared__ double etab[64];  // 2^(j/64) for the lobes' exp (vr_exp_table.h)
    if (threadIdx.x < 64) etab[threadIdx.x] = c_exp_tab[threadIdx.x];
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= npix) return;
    // records (vr_layout.h): the pixel's sums {X, Y, Z, weight} at state[4p], its Kahan
    // compensations at state[4 npix + 4p] -- 32 B each, one dwordx4 pair per half
    d2* const rs = reinterpret_cast<d2*>(state + 4 * p);
    d2* const rb = reinterpret_cast<d2*>(state + 4 * npix + 4 * p);
    double sum[3] = {0.0, 0.0, 0.0}, bias[3] = {0.0, 0.0, 0.0}, w = 0.0, wb = 0.0;
    if (accumulate) {
        const d2 s0 = rs[0], s1 = rs[1], b0 = rb[0], b1 = rb[1];
        sum[0] = s0.x; sum[1] = s0.y; sum[2] = s1.x; w = s1.y;
        bias[0] = b0.x; bias[1] = b0.y; bias[2] = b1.x; wb = b1.y;
    }
    // update_pixel for one sample (the Kahan chain is sequential in s)
    auto update = [&](const double c[3]) {
        const double wy = 1.0 - wb;
        const double wt = w + wy;
        wb = (wt - w) - wy;
        w = wt;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double y = c[k] * 1.0 - bias[k];
            const double t = sum[k] + y;
            bias[k] = (t - sum[k]) - y;
            sum[k] = t;
        }
    };
    // the colours of kB samples are independent (7 exp() each): computed together, then folded in
    // order -- the same operations as one at a time, with kB-fold instruction-level parallelism
    constexpr uint32_t kB = VR_REDUCE_BATCH;
    uint32_t s = 0;
    if (mask) {
        const uint64_t py = p / tile_width, px = p - py * tile_width;
        if (mask[(py >> 3) * ((tile_width + 7) >> 3) + (px >> 3)]) {
            // a culled block (block_cull_kernel): every sample is the photon {0, 0}, colour +0.
            // From a fresh record the Kahan chain has a closed form: colour y = +0 * 1 - +0 = +0
            // keeps sums and compensations +0, and the weight counts 1, 2, .., spp exactly with
            // compensation (n + 1 - n) - 1 = 0 (spp < 2^32 < 2^53)
            if (!accumulate) {
                w = (double)spp;
                s = spp;
            }
            const double z[3] = {0.0, 0.0, 0.0};
            for (; s < spp; ++s) update(z);
        }
    }
    for (; s + kB <= spp; s += kB) {
        double c[kB][3];
        d2 v[kB];
        uint64_t bits = 0;  // OR of the batch's photon bits: 0 iff all four are {+0, +0}
#pragma unroll
        for (uint32_t j = 0; j < kB; ++j) {
            // final photon {wavelength, intensity}: one 16-B non-temporal load
            VR_GUARD(s + j, p);
            v[j] = __builtin_nontemporal_load(reinterpret_cast<const d2*>(staging) + ((uint64_t)(s + j) * npix + p));
            bits |= (uint64_t)__double_as_longlong(v[j].x) | (uint64_t)__double_as_longlong(v[j].y);
        }
        // the lanes with some nonzero photon bit, as one 64-bit compare into a lane mask.  (Not a
        // compare of a zero-extended bool "dark" with 0: hipcc of ROCm 7.2 folded that into the
        // mask of the dark lanes -- the opposite polarity -- once this loop was split in two, so a
        // wave with ANY dark lane zeroed every lane's colours; DESIGN.md section 8, "the staging
        // invariant")
        if (__builtin_amdgcn_uicmpl(bits, 0ull, 33 /* ne */) == 0) {
            // a missed camera ray's photon {+0, +0} (camera.rs:110-113): every lobe is positive at
            // 0 nm, so its colour is (+0, +0, +0) exactly -- the wave skips the 28 exp when all
            // its photons are such (rows of pixels that see no geometry)
#pragma unroll
            for (uint32_t j = 0; j < kB; ++j) c[j][0] = c[j][1] = c[j][2] = 0.0;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < kB; ++j) {
                const double wl = v[j].x, I = v[j].y;
                const double Is = I * 360.0;                     // photon.rs:26-28, camera.rs:121-126
                const V3 cx = xyz_for_wavelength_tab<ANY_WL>(wl, etab);  // colour_xyz.rs:31-35
                c[j][0] = cx.x * Is;
                c[j][1] = cx.y * Is;
                c[j][2] = cx.z * Is;
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < kB; ++j) update(c[j]);
    }
    for (; s < spp; ++s) {
        VR_GUARD(s, p);
        const d2 v = __builtin_nontemporal_load(reinterpret_cast<const d2*>(staging) + ((uint64_t)s * npix + p));
        const double wl = v.x, I = v.y;
        const double Is = I * 360.0;
        const V3 cx = xyz_for_wavelength_tab<ANY_WL>(wl, etab);
        const double c[3] = {cx.x * Is, cx.y * Is, cx.z * Is};
        update(c);
    }
    rs[0] = d2{sum[0], sum[1]};
    rs[1] = d2{sum[2], w};
    rb[0] = d2{bias[0], bias[1]};
    rb[1] = d2{bias[2], wb};
}
#undef VR_GUARD

}  // namespace dev

// the reduce of a render launch, after its render kernel on the same stream (vr_render_launch.hip launch_render)
hipError_t launch_reduce(const RenderArgs& a, hipStream_t s, hipEvent_t mid) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (mid) {  // between the render kernel and the ordered reduce (timed launches)
        e = hipEventRecord(mid, s);
        if (e != hipSuccess) return e;
    }
    const uint64_t npix = a.tile_width * a.tile_height;
    hipLaunchKernelGGL(dev::accumulate_kernel<false>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, a.state,
                       (const double*)a.staging, npix, a.spp, a.accumulate, a.block_mask, a.tile_width,
                       a.stage_tag, a.stage_gen, a.error_flag);
    return hipGetLastError();
}

// the ordered reduce on its own, for photons a caller staged (vr_accumulate_photons_device): every
// pixel's samples are read, there is no cull mask
int launch_accumulate(double* state, const double* photons, uint64_t npix, uint32_t spp, uint32_t accumulate,
                      void* stream) {
#ifdef VR_STAGE_GUARD  // debug builds: caller-staged photons carry no generation tags
    return (int)hipErrorNotSupported;
#else
    if (npix == 0) return 0;
    hipLaunchKernelGGL(dev::accumulate_kernel<true>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       state, photons, npix, spp, accumulate, (const uint8_t*)nullptr, npix,
                       (const uint32_t*)nullptr, 0u, (int32_t*)nullptr);
    return (int)hipGetLastError();
#endif
}

}  // namespace vr
