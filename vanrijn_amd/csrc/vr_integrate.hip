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
// the Whitted shadow rays, on the same LDS stack).  Shading is render_kernel's `shade` lambda and the
// transitions around it (vr_render.hip) restated for one lane, the same operations in the same order
// with the general lambda-0 pair (T0, Acc0) and every material kind compiled in: under
// -ffp-contract=off the photons equal the megakernel's bit for bit.
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
            // world_to_bsdf = rows(tangent, cotangent, normal) (algebra_utils.rs:3-5); its
            // determinant via the first-row minors (mat3.rs:106-109)
            const double det = h.tangent.x * (h.cotangent.y * h.normal.z - h.cotangent.z * h.normal.y) -
                               h.tangent.y * (h.cotangent.x * h.normal.z - h.cotangent.z * h.normal.x) +
                               h.tangent.z * (h.cotangent.x * h.normal.y - h.cotangent.y * h.normal.x);
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
                // light terms, in order (fold from the camera photon's intensity 0): a shadow ray per
                // light; blocked -> the ambient spectrum, else bsdf(W retro, W dir, light(lambda) |dir.n|)
                double C = 0.0;
                for (int j = 0; j < S.light_count; ++j) {
                    const V3 ldir = ldv(S.light_dirs + 3 * j);
                    const V3 d1 = normalize(ldir);
                    const RayPre sp = prepare(Ray{add(h.loc, scl(d1, kBounceBias)), normalize_n1(d1)});
                    double term;
                    Best unused;
                    if (walk4<STACK, true>(S, sp, st, tid, unused)) {
                        term = material_intensity(&S.materials[S.light_base], lambda);
                    } else {
                        const V3 wl = mk(dot(h.tangent, ldir), dot(h.cotangent, ldir), dot(h.normal, ldir));
                        const double I = material_intensity(&S.materials[S.light_base + 1 + j], lambda) * fabs(dot(ldir, h.normal));
                        double ba, bb;
                        bsdf_affine(mat, w_i, wl, lambda, ba, bb);
                        term = ba * I + bb;
                    }
                    C = C + term;
                }
                Acc = Acc + T * C;
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
            if (kind == 1) {  // reflective_material.rs:42-47
                w_o = mk(-w_i.x, -w_i.y, w_i.z);
                pdf = 1.0;
            } else if (kind == 2) {  // Phong: Material::sample's default (materials/mod.rs:28-33)
                w_o = cosine_weighted_hemisphere(rng);
                pdf = cosine_weighted_pdf(w_o);
            } else if (kind == 3) {  // smooth_transparent_dialectric.rs:97-114
                fr = dielectric_fresnel(mat, w_i, lambda);
                pdf = 0.5;
                if (fr.T <= 0.0000000001) w_o = fr.rdir;
                else if (fr.R <= 0.0000000001 || rng.boolean()) w_o = fr.tdir;
                else w_o = fr.rdir;
            } else {  // lambertian_material.rs:36-59: rejection sampling on Open01 pairs
                double x = 2.0 * rng.open01() - 1.0;
                double y = 2.0 * rng.open01() - 1.0;
                while (dot(mk(x, y, 0.0), mk(x, y, 0.0)) > 1.0) {
                    x = 2.0 * rng.open01() - 1.0;
                    y = 2.0 * rng.open01() - 1.0;
                }
                const double z = fmax(sqrt(1.0 - x * x - y * y), 0.0);
                const V3 w = mk(x, y, z);
                const double cos_theta = dot(w, mk(0.0, 0.0, 1.0));
                const double sin_theta = sqrt(1.0 - cos_theta * cos_theta);
                w_o = normalize_n1(w);  // |w|^2 = x^2 + y^2 + (1 - x^2 - y^2): 1 within a few spacings
                pdf = (cos_theta * sin_theta) / 3.14159265358979323846;
            }
            // bsdf_to_world = cofactor(M)^T * det (mat3.rs:111-118), applied to w_o by rows
            V3 wo_world;
            {
                const double m00 = h.tangent.x, m01 = h.tangent.y, m02 = h.tangent.z;
                const double m10 = h.cotangent.x, m11 = h.cotangent.y, m12 = h.cotangent.z;
                const double m20 = h.normal.x, m21 = h.normal.y, m22 = h.normal.z;
                const V3 inv0 = mk((1.0 * (m11 * m22 - m12 * m21)) * det, (-1.0 * (m01 * m22 - m02 * m21)) * det,
                                   (1.0 * (m01 * m12 - m02 * m11)) * det);
                wo_world.x = dot(inv0, w_o);
                const V3 inv1 = mk((-1.0 * (m10 * m22 - m12 * m20)) * det, (1.0 * (m00 * m22 - m02 * m20)) * det,
                                   (-1.0 * (m00 * m12 - m02 * m10)) * det);
                wo_world.y = dot(inv1, w_o);
                const V3 inv2 = mk((1.0 * (m10 * m21 - m11 * m20)) * det, (-1.0 * (m00 * m21 - m01 * m20)) * det,
                                   (1.0 * (m00 * m11 - m01 * m10)) * det);
                wo_world.z = dot(inv2, w_o);
            }
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
                if (kind == 1) {  // reflective_material.rs:17-39
                    if (w_i.z <= 0.0 || w_o.z <= 0.0) {
                        a = 0.0; a0 = 0.0; bterm = 0.0; cut = true;
                    } else {
                        const V3 refl = mk(-w_o.x, -w_o.y, w_o.z);
                        double cth = dot(w_i, refl);
                        cth = cth < 0.0 ? 0.0 : (cth > 1.0 ? 1.0 : cth);
                        const double theta = acos(fabs(cth));
                        const double sigma = 0.05, two = 2.0;
                        const double f = mat->reflection * exp(-(pow(theta, two)) / (two * sigma * sigma));
                        a = (((pdf * cosf) * c_l) * mat->diffuse) * (1.0 - f);
                        a0 = (((pdf * cosf) * c_0) * mat->diffuse) * (1.0 - f);
                        bterm = f;
                    }
                } else if (kind == 2) {  // phong_material.rs:17-36: diffuse + specular lobe
                    if (w_i.z < 0.0 || w_o.z < 0.0) {
                        a = 0.0; a0 = 0.0; bterm = 0.0; cut = true;
                    } else {
                        const V3 refl = mk(-w_i.x, -w_i.y, w_i.z);
                        a = ((pdf * cosf) * c_l) * mat->diffuse;
                        a0 = ((pdf * cosf) * c_0) * mat->diffuse;
                        bterm = pow(fabs(dot(w_o, refl)), mat->smoothness) * (mat->reflection / dot(w_i, mk(0.0, 0.0, 1.0)));
                    }
                } else if (kind == 3) {  // smooth_transparent_dialectric.rs:79-95
                    a = (pdf * cosf) * dielectric_strength(fr, w_o);
                    a0 = (pdf * cosf) * dielectric_strength(dielectric_fresnel(mat, w_i, 0.0), w_o);
                    bterm = 0.0;
                } else {  // lambertian_material.rs:27-34
                    a = ((pdf * cosf) * c_l) * mat->diffuse;
                    a0 = ((pdf * cosf) * c_0) * mat->diffuse;
                    bterm = 0.0;
                }
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
            // Ray::new(location, w_o).bias(1e-7): normalise, step, normalise again (mod.rs:41-61)
            const V3 d1 = normalize_n1(wo_world);  // an orthonormal basis applied to a unit vector
            ++bounces;
            ray.o = add(h.loc, scl(d1, kBounceBias));
            ray.d = normalize_n1(d1);
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
