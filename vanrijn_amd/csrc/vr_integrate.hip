// vr_integrate.hip -- the scene's integrator for caller-supplied rays (gfx950): the body of
// partial_render_scene's loop (camera.rs:107-120: sampler.sample(&ray), then integrator.integrate(..)
// or the zero photon) for rays that come from the caller, not from the scene's ImageSampler.
//
// One path per lane.  A path is 0 to kRecursionLimit bounces long, so the kernel's loop runs over path
// steps, not over rays: each lane owns a grid-stride sequence of ray indices, and a lane whose path has
// ended loads its next ray in the same iteration in which its wave-mates go on tracing (lane-level
// regeneration: no atomics, no queue, no scratch allocation).  A wave leaves when all its lanes are
// out of rays.
//
// Traversal is vr_walk4.h's per-lane walk of the 4-wide tree (closest hit for path rays, any hit for
// the Whitted shadow rays, on the same LDS stack).  One shading level is vr_shade.h's, the functions
// render_kernel's `shade` lambda calls too (vr_render_kernel.h), with the general lambda-0 pair (T0, Acc0)
// and every material kind compiled in; the path state and the transitions around a level are that
// kernel's restated for one lane, the same operations in the same order: under -ffp-contract=off the
// photons equal the megakernel's bit for bit.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_layout.h"
#include "vr_exp_table.h"
#include "vr_camera.h"

#include "vr_device.h"
#include "vr_shade.h"
#include "vr_walk4.h"

namespace vr {
namespace dev {

typedef double vri_d2 __attribute__((ext_vector_type(2)));
typedef int32_t vri_i2 __attribute__((ext_vector_type(2)));

template <int STACK, bool WHITTED>
__global__ __launch_bounds__(256) void integrate_kernel(IntegrateArgs A) {
    __shared__ uint32_t st[2 * STACK * 256];
    const int tid = threadIdx.x;
    const DeviceScene& S = A.scene;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint64_t i = (uint64_t)blockIdx.x * 256 + tid;  // the lane's current ray
    bool live = false;                              // a path of ray i is under way
    Ray ray;                                        // the next ray to trace
    Rng rng;
    // the path's state, as render_kernel's: depth -1 = the caller's ray
    int depth = -1, bounces = 0, flags = 0;
    double lambda = 0.0, T = 1.0, Acc = 0.0, T0 = 1.0, Acc0 = 0.0, Wa = 0.0, Wb = 0.0, wo_y = 0.0;
    while (true) {
        if (!live) {
            if (i >= A.n) break;
            ray.o = ldv(A.origins + 3 * i);
            ray.d = ldv(A.directions + 3 * i);
            if (A.flags & VR_QUERY_NORMALIZE) ray.d = normalize(ray.d);  // Ray::new (mod.rs:41-46)
            const uint64_t id = A.stream_ids ? A.stream_ids[i] : (((A.first_stream + i) << 32) + A.sample);
            rng.reset(mix64(A.seed_key ^ id));  // stream_base_keyed with (pixel << 32) + sample = id
            rng.x += A.first_draw * kWeyl32;    // the draws the caller has spent
            depth = -1;
            bounces = 0;
            flags = 0;
            live = true;
        }
        const RayPre pre = prepare(ray);
        Best best;
        walk4<STACK, false>(S, pre, st, tid, best);
        // the ray's closest hit is known (render_kernel's state kTraversed)
        bool go = false, fin = false;
        double fin_wl = 0.0, fin_I = 0.0;
        auto finish = [&](double wl, double I) {
            fin = true;
            fin_wl = wl;
            fin_I = I;
        };
        if (WHITTED && depth >= 0) {
            if (!best.kind) {
                finish(lambda, Acc);  // the continuation missed: photon.scale_intensity(0)
            } else {
                Acc = Acc + Wb;
                T = Wa;
                depth += 1;
                go = true;
            }
        } else if (depth < 0) {
            if (!best.kind) {
                finish(0.0, 0.0);  // the caller's ray missed: photon {0, 0} (camera.rs:110-113)
            } else {
                flags |= 1;
                // Photon::random_wavelength, or the caller's (no draw spent)
                lambda = A.wavelengths ? A.wavelengths[i] : 380.0 + (740.0 - 380.0) * rng.standard();
                T = 1.0; Acc = 0.0; T0 = 1.0; Acc0 = 0.0;
                depth = 0;
                go = true;
            }
        } else if (!best.kind) {
            // simple_random_integrator.rs:43-46; below a cut level (kPathCut) the sky term is discarded too
            finish(lambda, (flags & kPathCut) ? Acc : Acc + T * sky_intensity(wo_y, lambda, &S.materials[S.sky_row]));
        } else {
            depth += 1;
            if (depth == kRecursionLimit) {  // integrate(.., 0) returns {0, 0}: lambda becomes 0
                flags |= 2;
                // the innermost photon's intensity 0 times the lambda-0 throughput: + 0 when finite,
                // NaN when a level's pdf * |cos| was (the reference's 0 * NaN)
                finish(0.0, (flags & kPathCut) ? Acc0 : Acc0 + T0 * 0.0);
            } else {
                go = true;
            }
        }
        // one level of SimpleRandomIntegrator::integrate (simple_random_integrator.rs:20-53) or of
        // WhittedIntegrator::integrate (whitted_integrator.rs:15-87) at the closest hit, forward form:
        // ends the path or leaves the bounce ray in `ray`
        if (go) do {
            HitInfo h;
            hit_info(S, best, pre, h);
            const double det = basis_det(h);
            // try_inverse() == None: the reference panics; the fault_object test hook takes this path
            if (det == 0.0 || best.object == A.fault_object) {
                flags |= 4;
                atomicOr(A.error_flag, 1);
                finish(0.0, 0.0);
                break;
            }
            const V3 w_i = mk(dot(h.tangent, h.retro), dot(h.cotangent, h.retro), dot(h.normal, h.retro));
            const Material* mat = &S.materials[h.material];
            if constexpr (WHITTED) {
                Acc = Acc + T * whitted_direct(S, h, mat, w_i, lambda, [&](const RayPre& sp) {
                    Best unused;
                    return walk4<STACK, true>(S, sp, st, tid, unused);
                });
                if (depth >= kRecursionLimit) {  // recursion_limit 0: the continuation contributes 0
                    flags |= 2;
                    finish(lambda, Acc);
                    break;
                }
            }
            V3 w_o;
            double pdf;
            const int kind = mat->kind;
            Fresnel fr;  // dielectric only
            if (kind == 3) fr = sample_dielectric(mat, w_i, lambda, rng, w_o, pdf);
            else sample_bsdf<3>(kind, w_i, rng, w_o, pdf);
            const V3 wo_world = bsdf_to_world(h, det, w_o);
            const double cosf = fabs(dot(wo_world, h.normal));
            if constexpr (WHITTED) {
                // continuation: bsdf(W retro, dir, L_next) |dir.n|, applied when its ray hits
                double ba, bb;
                bsdf_affine(mat, w_i, w_o, lambda, ba, bb);
                Wa = (T * ba) * cosf;
                Wb = (T * bb) * cosf;
            } else {
                const double c_l = material_intensity(mat, lambda);
                const double c_0 = material_intensity(mat, 0.0);
                double a, a0, bterm;
                bool cut = false;  // this level's bsdf returns the constant 0 whatever comes from below
                if (kind == 3) dielectric_factors<false>(mat, fr, w_i, w_o, pdf, cosf, a, a0, bterm);
                else level_factors<3>(mat, kind, w_i, w_o, pdf, cosf, c_l, c_0, a, a0, bterm, cut);
                // (render_kernel's shade(): levels below a cut one are traced and change nothing)
                if (!(flags & kPathCut)) {
                    Acc = Acc + T * bterm;
                    T = T * a;
                    Acc0 = Acc0 + T0 * bterm;
                    T0 = T0 * a0;
                }
                if (cut) flags |= kPathCut;
                wo_y = wo_world.y;  // the sky term reads the un-normalised direction's y
            }
            ++bounces;
            bounce_ray(h, wo_world, ray.o, ray.d);
        } while (false);
        if (fin) {
            // the caller reads them: plain 16-B and 8-B stores
            reinterpret_cast<vri_d2*>(A.photons)[i] = vri_d2{fin_wl, fin_I};
            if (A.info) reinterpret_cast<vri_i2*>(A.info)[i] = vri_i2{bounces, flags & ~kPathCut};
            live = false;
            i += stride;
        }
    }
}

// ImageSampler::ray_for_pixel (camera.rs:24-66) for entry j = s * (tile pixels) + p: render_kernel's
// camera step (the jitter is draws 0 and 1 of the (pixel, sample) stream, x before y) under the
// scene's pose: vr_camera.h's rule; under a lens the lens rule, with draws 2 and 3, and an origin per entry
__global__ __launch_bounds__(256) void camera_rays_kernel(CameraRaysArgs A) {
    const uint64_t npix = A.tile_width * A.tile_height;
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= npix * A.spp) return;
    const uint64_t s = j / npix, p = j - s * npix;
    const uint64_t py = p / A.tile_width, px = p - py * A.tile_width;
    const uint64_t row = A.start_row + py, col = A.start_column + px;
    const uint64_t id = ((row * A.width + col) << 32) + (A.first_sample + s);
    Rng rng;
    rng.reset(mix64(A.seed_key ^ id));
    const double ux = rng.standard();
    const double uy = rng.standard();
    const double x = camera::film_x(A.film, col, ux);
    const double y = camera::film_y(A.film, A.height, row, uy);
    camera::Vec o, d;
    if (A.lens.lens_radius != 0.0) {  // a lens: draws 2 and 3, then the lens rule (vr_camera.h)
        const double lu = rng.standard();
        const double lv = rng.standard();
        camera::lens_ray(A.camera, A.pose.right, A.pose.up, A.pose.forward, A.pose.film_distance, A.lens.lens_radius,
                         A.lens.focus_distance, x, y, lu, lv, &o, &d);
    } else {
        o.x = A.camera[0];
        o.y = A.camera[1];
        o.z = A.camera[2];
        d = camera::ray_direction(A.pose.right, A.pose.up, A.pose.forward, A.pose.film_distance, x, y);
    }
    A.origins[3 * j] = o.x;
    A.origins[3 * j + 1] = o.y;
    A.origins[3 * j + 2] = o.z;
    A.directions[3 * j] = d.x;
    A.directions[3 * j + 1] = d.y;
    A.directions[3 * j + 2] = d.z;
    A.stream_ids[j] = id;
}

}  // namespace dev

template <int STACK>
static void launch_integrate_t(const IntegrateArgs& a, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    if (a.scene.integrator == 1) hipLaunchKernelGGL((dev::integrate_kernel<STACK, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((dev::integrate_kernel<STACK, false>), grid, block, 0, s, a);
}

int launch_integrate(const IntegrateArgs& a, int stack_depth, int grid_limit, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (a.n == 0) return 0;
    if (stack_depth > 48) return -1000;
    // one workgroup per 256 rays, capped: each lane of a larger batch takes its grid-stride sequence
    const uint64_t want = (a.n + 255) / 256;
    const dim3 grid((unsigned)(want < (uint64_t)grid_limit ? want : (uint64_t)grid_limit));
    if (stack_depth <= 24) launch_integrate_t<24>(a, grid, s);
    else if (stack_depth <= 32) launch_integrate_t<32>(a, grid, s);
    else launch_integrate_t<48>(a, grid, s);
    return (int)hipGetLastError();
}

int launch_camera_rays(const CameraRaysArgs& a, void* stream) {
    const uint64_t n = a.tile_width * a.tile_height * a.spp;
    if (n == 0) return 0;
    hipLaunchKernelGGL(dev::camera_rays_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

}  // namespace vr
