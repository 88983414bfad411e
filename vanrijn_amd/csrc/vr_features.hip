// vr_features.hip -- first-hit feature buffers (gfx950): per pixel of a tile, what the camera rays of its
// samples meet first -- summed shading normals and distances, the hit count, the nearest sample's object
// and primitive -- and, optionally, a state array of the first hits' material colours (the albedo).
//
// One lane owns one pixel; a wave covers an 8x8 pixel block of the tile and a workgroup four blocks.
// The lane runs its pixel's samples in order: the camera ray as camera_rays_kernel (vr_integrate.hip)
// and the render form it (vr_camera.h), prepare, vr_walk4.h's per-lane closest-hit walk on the
// workgroup's LDS stack, hit_info, and the fold into registers.  The records are written once, at the
// end: no staging buffer, so no pass split and no atomics, and every sum runs in sample order by
// construction.  The block cull is not used: a ray that misses everything costs its root tests.
//
// The albedo's fold is the ordered reduce's (vr_device.h PixelSums / photon_colour, the operations of
// vr_reduce.hip accumulate_kernel<true>): the array equals vr_accumulate_photons_device of the same
// photons bit for bit.  Compiled with -ffp-contract=off like every other unit.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_layout.h"
#include "vr_exp_table.h"
#include "vr_camera.h"

#include "vr_device.h"
#include "vr_walk4.h"

namespace vr {
namespace dev {

typedef double vrf_d2 __attribute__((ext_vector_type(2)));
typedef uint32_t vrf_u4 __attribute__((ext_vector_type(4)));
static_assert(sizeof(vr_pixel_features) == 64, "vr_pixel_features is four 16-B quads");

__constant__ double c_features_exp_tab[64] = VR_EXP_TABLE_INIT;

// ALBEDO: the albedo state is written (A.albedo_state != nullptr); without it no wavelength is drawn
// and no material row is read.  A.features may be null in an ALBEDO launch.
template <int STACK, bool ALBEDO>
__global__ __launch_bounds__(256) void features_kernel(FeaturesArgs A) {
    __shared__ uint32_t st[2 * STACK * 256];
    __shared__ double etab[ALBEDO ? 64 : 1];  // 2^(j/64) for the lobes' exp (vr_exp_table.h)
    const int tid = threadIdx.x;
    if (ALBEDO) {
        if (tid < 64) etab[tid] = c_features_exp_tab[tid];
        __syncthreads();
    }
    const DeviceScene& S = A.scene;
    // the wave's 8x8 block and the lane's pixel in it; lanes outside the tile idle
    const uint32_t block = blockIdx.x * 4u + ((uint32_t)tid >> 6);
    if (block >= A.block_count) return;
    const uint32_t by = block / A.blocks_per_row, bx = block - by * A.blocks_per_row;
    const uint64_t py = (uint64_t)by * 8 + (((uint32_t)tid >> 3) & 7u), px = (uint64_t)bx * 8 + ((uint32_t)tid & 7u);
    if (py >= A.tile_height || px >= A.tile_width) return;
    const uint64_t npix = A.tile_width * A.tile_height;
    const uint64_t p = py * A.tile_width + px;  // row-major in the tile
    const uint64_t row = A.start_row + py, col = A.start_column + px;
    const uint64_t pixel_id = (row * A.width + col) << 32;

    // the pixel's record (vr_pixel_features, four 16-B quads) and its albedo record, in registers
    vrf_d2* const rec = reinterpret_cast<vrf_d2*>((char*)A.features + 64 * p);
    const bool feat = A.features != nullptr;
    double nsum[3] = {0.0, 0.0, 0.0}, dsum = 0.0, dmin = 0.0;
    uint32_t hits = 0, samples = 0;
    int32_t object = -1;
    int64_t primitive = -1;
    vrf_d2* const rs = reinterpret_cast<vrf_d2*>(A.albedo_state + 4 * p);
    vrf_d2* const rb = reinterpret_cast<vrf_d2*>(A.albedo_state + 4 * npix + 4 * p);
    PixelSums acc;
    acc.clear();
    if (A.accumulate) {
        if (feat) {
            const vrf_d2 q0 = rec[0], q1 = rec[1];
            const vrf_u4 q2 = reinterpret_cast<const vrf_u4*>(rec)[2], q3 = reinterpret_cast<const vrf_u4*>(rec)[3];
            nsum[0] = q0.x; nsum[1] = q0.y; nsum[2] = q1.x; dsum = q1.y;
            dmin = __longlong_as_double((long long)(((uint64_t)q2.y << 32) | q2.x));
            hits = q2.z;
            samples = q2.w;
            object = (int32_t)q3.x;
            primitive = (int64_t)(((uint64_t)q3.w << 32) | q3.z);
        }
        if (ALBEDO) {
            const vrf_d2 s0 = rs[0], s1 = rs[1], b0 = rb[0], b1 = rb[1];
            acc.sum[0] = s0.x; acc.sum[1] = s0.y; acc.sum[2] = s1.x; acc.w = s1.y;
            acc.bias[0] = b0.x; acc.bias[1] = b0.y; acc.bias[2] = b1.x; acc.wb = b1.y;
        }
    }

    for (uint32_t s = 0; s < A.spp; ++s) {
        // ImageSampler::ray_for_pixel (camera.rs:24-66) under the scene's pose and lens: the jitter is
        // draws 0 and 1 of the (pixel, sample) stream, x before y; under a lens draws 2 and 3 feed the
        // lens rule (vr_camera.h), exactly as camera_rays_kernel
        Rng rng;
        rng.reset(mix64(A.seed_key ^ (pixel_id + (A.first_sample + s))));
        const double ux = rng.standard();
        const double uy = rng.standard();
        const double x = camera::film_x(A.film, col, ux);
        const double y = camera::film_y(A.film, A.height, row, uy);
        camera::Vec o, d;
        if (A.lens.lens_radius != 0.0) {
            const double lu = rng.standard();
            const double lv = rng.standard();
            camera::lens_ray(S.camera, A.pose.right, A.pose.up, A.pose.forward, A.pose.film_distance, A.lens.lens_radius,
                             A.lens.focus_distance, x, y, lu, lv, &o, &d);
        } else {
            o.x = S.camera[0];
            o.y = S.camera[1];
            o.z = S.camera[2];
            d = camera::ray_direction(A.pose.right, A.pose.up, A.pose.forward, A.pose.film_distance, x, y);
        }
        Ray ray;
        ray.o = mk(o.x, o.y, o.z);
        ray.d = mk(d.x, d.y, d.z);
        const RayPre pre = prepare(ray);
        Best best;
        const bool hit = walk4<STACK, false>(S, pre, st, tid, best);
        double c[3] = {0.0, 0.0, 0.0};  // a miss: the photon {0, 0} (camera.rs:110-113), whose colour is +0
        if (hit) {
            HitInfo h;
            hit_info(S, best, pre, h);
            if (feat) {
                // the nearest sample: the first hit sample, then only a strictly smaller distance (min_by:
                // a NaN distance never replaces a hit and is never replaced)
                if (hits == 0 || best.d < dmin) {
                    dmin = best.d;
                    object = best.object;
                    primitive = best.kind == kPrim ? S.prims[best.index].position : best.index;
                    if (best.kind == kTri) {
                        for (int b = 0; b < S.bvh_count; ++b)
                            if (S.bvhs[b].object == best.object)
                                primitive = S.tris[best.index].rank - S.bvhs[b].tri_base;  // reference leaf position
                    }
                }
                hits += 1;
                nsum[0] = nsum[0] + h.normal.x;
                nsum[1] = nsum[1] + h.normal.y;
                nsum[2] = nsum[2] + h.normal.z;
                dsum = dsum + best.d;
            }
            if (ALBEDO) {
                // Photon::random_wavelength: the draw the render uses (2, or 4 after the lens draws)
                const double lambda = 380.0 + (740.0 - 380.0) * rng.standard();
                const Material* mat = &S.materials[h.material];
                // the exact Spectrum::intensity_at_wavelength of the hit's material, no strength factor; a
                // dielectric's spectrum is an index of refraction, not a reflectance: 1
                const double a = mat->kind == 3 ? 1.0 : material_colour(mat, lambda);
                photon_colour<true>(lambda, a, etab, c);
            }
        }
        if (ALBEDO) acc.update(c);
    }
    samples += A.spp;

    if (feat) {
        const uint64_t dm = (uint64_t)__double_as_longlong(dmin);
        rec[0] = vrf_d2{nsum[0], nsum[1]};
        rec[1] = vrf_d2{nsum[2], dsum};
        reinterpret_cast<vrf_u4*>(rec)[2] = vrf_u4{(uint32_t)dm, (uint32_t)(dm >> 32), hits, samples};
        reinterpret_cast<vrf_u4*>(rec)[3] =
            vrf_u4{(uint32_t)object, 0u, (uint32_t)(uint64_t)primitive, (uint32_t)((uint64_t)primitive >> 32)};
    }
    if (ALBEDO) {
        rs[0] = vrf_d2{acc.sum[0], acc.sum[1]};
        rs[1] = vrf_d2{acc.sum[2], acc.w};
        rb[0] = vrf_d2{acc.bias[0], acc.bias[1]};
        rb[1] = vrf_d2{acc.bias[2], acc.wb};
    }
}

}  // namespace dev

template <int STACK>
static void launch_features_t(const FeaturesArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    if (a.albedo_state) hipLaunchKernelGGL((dev::features_kernel<STACK, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dev::features_kernel<STACK, false>), grid, block, 0, s, a);
}

int launch_features(const FeaturesArgs& a, int stack_depth, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (a.block_count == 0 || a.spp == 0) return 0;
    if (stack_depth > 48) return -1000;
    const dim3 grid((a.block_count + 3u) / 4u);  // four waves, four 8x8 blocks per workgroup
    // the stack classes as launch_integrate chooses them
    if (stack_depth <= 24) launch_features_t<24>(a, grid, s);
    else if (stack_depth <= 32) launch_features_t<32>(a, grid, s);
    else launch_features_t<48>(a, grid, s);
    return (int)hipGetLastError();
}

}  // namespace vr
