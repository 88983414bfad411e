// vr_shade.h -- one level of the integrators at a closest hit, in pieces (gfx950): what
// render_kernel's `shade` lambda (vr_render_kernel.h) and integrate_kernel (vr_integrate.hip) both do
// between a known hit and the bounce ray, once.  Every function takes and returns values and knows
// nothing of a path's state (flags, T / Acc / T0 / Acc0 / b0, Wa / Wb, the early stop): the two
// kernels keep that bookkeeping around these calls.  Each expression is the reference's, in its
// operation order (-ffp-contract=off), so both kernels compute the same bits.
#pragma once

#include "vr_device.h"

namespace vr {
namespace dev {

// world_to_bsdf = rows(tangent, cotangent, normal) (algebra_utils.rs:3-5); its
// determinant via the first-row minors (mat3.rs:106-109)
__device__ __forceinline__ double basis_det(const HitInfo& h) {
    return h.tangent.x * (h.cotangent.y * h.normal.z - h.cotangent.z * h.normal.y) -
           h.tangent.y * (h.cotangent.x * h.normal.z - h.cotangent.z * h.normal.x) +
           h.tangent.z * (h.cotangent.x * h.normal.y - h.cotangent.y * h.normal.x);
}

// Material::sample for every material kind but the dielectric (the caller's `kind`: compiled in for
// the kinds the scene has, MATS 1: Lambertian only, 2: reflective only, 3: any)
template <int MATS>
__device__ __forceinline__ void sample_bsdf(int kind, V3 w_i, Rng& rng, V3& w_o, double& pdf) {
    if (kind == 1) {  // reflective_material.rs:42-47
        w_o = mk(-w_i.x, -w_i.y, w_i.z);
        pdf = 1.0;
    } else if (MATS == 3 && kind == 2) {  // Phong: Material::sample's default (materials/mod.rs:28-33)
        w_o = cosine_weighted_hemisphere(rng);
        pdf = cosine_weighted_pdf(w_o);
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
}

// The dielectric's sample and factors (kind 3, MATS 3 only) stand apart from the other kinds': its
// Fresnel terms go from the one to the other through the caller, and as an argument of the functions
// of all kinds the partly written struct moved one render_kernel instantiation past 256 VGPRs
// (DESIGN.md section 6, round 16).

// smooth_transparent_dialectric.rs:97-114
__device__ __forceinline__ Fresnel sample_dielectric(const Material* mat, V3 w_i, double lambda, Rng& rng, V3& w_o,
                                                     double& pdf) {
    const Fresnel fr = dielectric_fresnel(mat, w_i, lambda);
    pdf = 0.5;
    if (fr.T <= 0.0000000001) w_o = fr.rdir;
    else if (fr.R <= 0.0000000001 || rng.boolean()) w_o = fr.tdir;
    else w_o = fr.rdir;
    return fr;
}

// smooth_transparent_dialectric.rs:79-95
template <bool DARK0>
__device__ __forceinline__ void dielectric_factors(const Material* mat, const Fresnel& fr, V3 w_i, V3 w_o, double pdf,
                                                   double cosf, double& a, double& a0, double& bterm) {
    a = (pdf * cosf) * dielectric_strength(fr, w_o);
    a0 = DARK0 ? 0.0 : (pdf * cosf) * dielectric_strength(dielectric_fresnel(mat, w_i, 0.0), w_o);
    bterm = 0.0;
}

// bsdf_to_world = cofactor(M)^T * det (mat3.rs:111-118), applied to w_o by rows
__device__ __forceinline__ V3 bsdf_to_world(const HitInfo& h, double det, V3 w_o) {
    V3 wo_world;
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
    return wo_world;
}

// The lobes take the reference's bsdf(w_o, w_i, ..) arguments under its names.  The
// SimpleRandomIntegrator passes (sampled direction, retro), the WhittedIntegrator (retro, direction).

// reflective_material.rs:24-34: the reflection factor of a mirror met from the front
__device__ __forceinline__ double mirror_lobe(const Material* m, V3 w_o, V3 w_i) {
    const V3 refl = mk(-w_o.x, -w_o.y, w_o.z);
    double cth = dot(w_i, refl);
    cth = cth < 0.0 ? 0.0 : (cth > 1.0 ? 1.0 : cth);
    const double theta = acos(fabs(cth));
    const double sigma = 0.05, two = 2.0;
    return m->reflection * exp(-(pow(theta, two)) / (two * sigma * sigma));
}

// phong_material.rs:25-29: the specular term of a Phong surface met from the front
__device__ __forceinline__ double phong_lobe(const Material* m, V3 w_o, V3 w_i) {
    const V3 refl = mk(-w_i.x, -w_i.y, w_i.z);
    return pow(fabs(dot(w_o, refl)), m->smoothness) * (m->reflection / dot(w_i, mk(0.0, 0.0, 1.0)));
}

// One level of SimpleRandomIntegrator::integrate (simple_random_integrator.rs:39-53) as an affine map
// of what comes from below: out = a * I + bterm at the path's wavelength (spectrum value c_l), a0 at
// wavelength 0 (c_0; DARK0: the scene's spectra are 0 there).  cut is set when this level's bsdf
// returns the constant 0 whatever comes from below.  Every kind but the dielectric.
template <int MATS>
__device__ __forceinline__ void level_factors(const Material* mat, int kind, V3 w_i, V3 w_o, double pdf, double cosf,
                                              double c_l, double c_0, double& a, double& a0, double& bterm, bool& cut) {
    if (kind == 1) {  // reflective_material.rs:17-39
        if (w_i.z <= 0.0 || w_o.z <= 0.0) {
            a = 0.0; a0 = 0.0; bterm = 0.0; cut = true;
        } else {
            const double f = mirror_lobe(mat, w_o, w_i);
            a = (((pdf * cosf) * c_l) * mat->diffuse) * (1.0 - f);
            a0 = (((pdf * cosf) * c_0) * mat->diffuse) * (1.0 - f);
            bterm = f;
        }
    } else if (MATS == 3 && kind == 2) {  // phong_material.rs:17-36: diffuse + specular lobe
        if (w_i.z < 0.0 || w_o.z < 0.0) {
            a = 0.0; a0 = 0.0; bterm = 0.0; cut = true;
        } else {
            a = ((pdf * cosf) * c_l) * mat->diffuse;
            a0 = ((pdf * cosf) * c_0) * mat->diffuse;
            bterm = phong_lobe(mat, w_o, w_i);
        }
    } else {  // lambertian_material.rs:27-34
        a = ((pdf * cosf) * c_l) * mat->diffuse;
        a0 = ((pdf * cosf) * c_0) * mat->diffuse;
        bterm = 0.0;
    }
}

// Material::bsdf as an affine map of the incoming intensity: out = a * I + b, for the
// WhittedIntegrator's calls (bsdf(w_o, w_i, photon)); lambertian_material.rs:27-34,
// reflective_material.rs:15-40, phong_material.rs:17-36, smooth_transparent_dialectric.rs:79-95
__device__ __forceinline__ void bsdf_affine(const Material* m, V3 w_o, V3 w_i, double wl, double& a, double& b) {
    b = 0.0;
    if (m->kind == 1) {
        if (w_i.z <= 0.0 || w_o.z <= 0.0) {
            a = 0.0;
            return;
        }
        const double f = mirror_lobe(m, w_o, w_i);
        a = (material_intensity(m, wl) * m->diffuse) * (1.0 - f);
        b = f;
    } else if (m->kind == 2) {
        if (w_i.z < 0.0 || w_o.z < 0.0) {
            a = 0.0;
            return;
        }
        a = material_intensity(m, wl) * m->diffuse;
        b = phong_lobe(m, w_o, w_i);
    } else if (m->kind == 3) {
        a = dielectric_strength(dielectric_fresnel(m, w_i, wl), w_o);
    } else {
        a = material_intensity(m, wl) * m->diffuse;
    }
}

// WhittedIntegrator's light terms, in order (fold from the camera
// photon's intensity 0): a shadow ray per light; blocked -> the ambient spectrum, else
// bsdf(W retro, W dir, light(lambda) |dir.n|).  occluded(RayPre): the caller's any-hit walk.
template <class Occluded>
__device__ __forceinline__ double whitted_direct(const DeviceScene& S, const HitInfo& h, const Material* mat, V3 w_i,
                                                 double lambda, Occluded occluded) {
    double C = 0.0;
    for (int j = 0; j < S.light_count; ++j) {
        const V3 ldir = ldv(S.light_dirs + 3 * j);
        const V3 d1 = normalize(ldir);
        const RayPre sp = prepare(Ray{add(h.loc, scl(d1, kBounceBias)), normalize_n1(d1)});
        double term;
        if (occluded(sp)) {
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
    return C;
}

// Ray::new(location, w_o).bias(1e-7): normalise, step, normalise again (mod.rs:41-61)
__device__ __forceinline__ void bounce_ray(const HitInfo& h, V3 wo_world, V3& o, V3& d) {
    const V3 d1 = normalize_n1(wo_world);  // an orthonormal basis applied to a unit vector
    o = add(h.loc, scl(d1, kBounceBias));
    d = normalize_n1(d1);
}

}  // namespace dev
}  // namespace vr
