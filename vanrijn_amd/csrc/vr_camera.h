// vr_camera.h -- the camera ray rule, and the lens rule below it, shared by the render kernel's camera
// step (vr_render_kernel.h), the block cull (vr_cull.hip), camera_rays_kernel (vr_integrate.hip) and the host's
// vr_camera_ray / vr_camera_lens_ray: one definition, so all four form the same bits.
//
// ImageSampler (camera.rs:24-66) looks down +z from `location` with the film one unit away.  A pose
// {location, right, up, forward, film_distance} turns and zooms that camera: the film point (x, y)
// -- computed as the reference computes it -- leaves along
//     d_c = (x * right_c + y * up_c) + film_distance * forward_c        for each component c,
// in f64, in this order, without contraction (the build's -ffp-contract=off), and the ray is
// Ray::new(location, d): direction d * (1 / |d|) (vec3.rs:103-110).
//
// The default pose -- right (1,0,0), up (0,1,0), forward (0,0,1), film_distance 1 -- gives the
// reference's normalize((x, y, 1)) bit for bit: x and y are differences a - b under
// round-to-nearest, so never -0; every product with a 0 axis entry is +-0, and v + +-0 = v for
// every v that is not -0; the z component is (+-0 + +-0) + 1 * 1 = 1.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace vr {
namespace camera {

struct Vec {
    double x, y, z;
};

// ImageSampler::new's film constants (camera.rs:24-45), the reference's f64 operations: film_w * (1 /
// width), film_w * 0.5, film_h * (1 / height), film_h * 0.5 with the shorter film side 1
__host__ __device__ inline void film_constants(uint64_t width, uint64_t height, double film[4]) {
    const double fw = (double)width, fh = (double)height;
    const double film_w = fw > fh ? fw / fh : 1.0;
    const double film_h = fw > fh ? 1.0 : fw / fh;
    film[0] = film_w * (1.0 / fw);
    film[1] = film_w * 0.5;
    film[2] = film_h * (1.0 / fh);
    film[3] = film_h * 0.5;
}

// the film point of pixel (row, column) with jitter (ux, uy) in [0, 1) (camera.rs:47-66)
__host__ __device__ inline double film_x(const double film[4], uint64_t column, double ux) {
    return ((double)column + ux) * film[0] - film[1];
}
__host__ __device__ inline double film_y(const double film[4], uint64_t height, uint64_t row, double uy) {
    return ((double)(height - (row + 1)) + uy) * film[2] - film[3];
}

// the rule: where the ray through film point (x, y) heads, not normalised (affine in (x, y))
__host__ __device__ inline Vec film_to_world(const double right[3], const double up[3], const double forward[3],
                                             double film_distance, double x, double y) {
    Vec d;
    d.x = (x * right[0] + y * up[0]) + film_distance * forward[0];
    d.y = (x * right[1] + y * up[1]) + film_distance * forward[1];
    d.z = (x * right[2] + y * up[2]) + film_distance * forward[2];
    return d;
}

// Vec3::normalize (vec3.rs:76-82, 103-110): the sum folds from -0.0, then multiply by 1 / norm
__host__ __device__ inline Vec normalize(Vec a) {
    double s = -0.0;
    s = s + a.x * a.x;
    s = s + a.y * a.y;
    s = s + a.z * a.z;
    const double inv = 1.0 / sqrt(s);
    Vec r;
    r.x = a.x * inv;
    r.y = a.y * inv;
    r.z = a.z * inv;
    return r;
}

// the camera ray's direction through film point (x, y)
__host__ __device__ inline Vec ray_direction(const double right[3], const double up[3], const double forward[3],
                                             double film_distance, double x, double y) {
    return normalize(film_to_world(right, up, forward, film_distance, x, y));
}

// ----------------------------------------------------------------------------------------------
// The thin lens (vr_scene_set_camera_lens).  A lens of radius lens_radius lies in the right / up plane
// at `location`, focused on the plane focus_distance along `forward`.  A sample with film point (x, y)
// and lens draws (lu, lv) in [0, 1) leaves the lens point (a, b) = lens_radius * disc(lu, lv) towards the
// point where the pinhole ray through (x, y) meets the focus plane; that line is the pinhole line of the
// film point shifted by -(a, b) k, k = film_distance / focus_distance.  In f64, without contraction, in
// this order:
//     k = film_distance / focus_distance
//     a = lens_radius * disc_x;  b = lens_radius * disc_y
//     origin_c = location_c + (a * right_c + b * up_c)                  for each component c
//     d = film_to_world(right, up, forward, film_distance, x - a * k, y - b * k)
//     direction = normalize(d)
//
// disc is Shirley's concentric map as UnitDisc::value states it (unit_disc.rs:28-40) over the square
// ox = 2 lu - 1, oy = 2 lv - 1:
//     (0, 0) -> (0, 0)
//     |ox| > |oy|:  phi = ((pi / 4) * oy) / ox;   disc = (ox * cos phi, ox * sin phi)
//     otherwise:    phi = ((pi / 4) * ox) / oy;   disc = (oy * sin phi, oy * cos phi)
// (the reference's second angle is pi / 2 - phi, whose cosine and sine are sin phi and cos phi), so
// both branches need sin and cos on [-pi/4, pi/4] only.  They are fixed polynomials, not libm: glibc
// and the device math library need not round alike, and host and kernels must form the same bits
// (as vr_exp_table.h does for exp).  Taylor terms through x^15 and x^16, Horner in z = x * x:
//     sin x = x * (1 + z (s3 + z (s5 + ... + z s15)))       s_n = -+1 / n!
//     cos x =      1 + z (c2 + z (c4 + ... + z c16))        c_n = -+1 / n!
// each step one multiplication then one addition; the truncation is below 5e-17 on the interval and
// both are within 1.2e-16 of the correctly rounded functions there.
// ----------------------------------------------------------------------------------------------
__host__ __device__ inline double lens_sin(double x) {
    const double z = x * x;
    double p = -1.0 / 1307674368000.0;  // 15!
    p = p * z + 1.0 / 6227020800.0;     // 13!
    p = p * z + -1.0 / 39916800.0;      // 11!
    p = p * z + 1.0 / 362880.0;         // 9!
    p = p * z + -1.0 / 5040.0;          // 7!
    p = p * z + 1.0 / 120.0;            // 5!
    p = p * z + -1.0 / 6.0;             // 3!
    p = p * z + 1.0;
    return x * p;
}
__host__ __device__ inline double lens_cos(double x) {
    const double z = x * x;
    double p = 1.0 / 20922789888000.0;  // 16!
    p = p * z + -1.0 / 87178291200.0;   // 14!
    p = p * z + 1.0 / 479001600.0;      // 12!
    p = p * z + -1.0 / 3628800.0;       // 10!
    p = p * z + 1.0 / 40320.0;          // 8!
    p = p * z + -1.0 / 720.0;           // 6!
    p = p * z + 1.0 / 24.0;             // 4!
    p = p * z + -1.0 / 2.0;             // 2!
    p = p * z + 1.0;
    return p;
}

// disc(lu, lv): a point of the unit disc (radius at most 1 + a few ulp)
__host__ __device__ inline void lens_disc(double lu, double lv, double* dx, double* dy) {
    const double ox = 2.0 * lu - 1.0, oy = 2.0 * lv - 1.0;
    if (ox == 0.0 && oy == 0.0) {
        *dx = ox;
        *dy = oy;
    } else if (fabs(ox) > fabs(oy)) {
        const double phi = ((3.14159265358979323846 / 4.0) * oy) / ox;
        *dx = ox * lens_cos(phi);
        *dy = ox * lens_sin(phi);
    } else {
        const double phi = ((3.14159265358979323846 / 4.0) * ox) / oy;
        *dx = oy * lens_sin(phi);
        *dy = oy * lens_cos(phi);
    }
}

// the lens rule: origin and direction of the sample's ray
__host__ __device__ inline void lens_ray(const double location[3], const double right[3], const double up[3],
                                         const double forward[3], double film_distance, double lens_radius,
                                         double focus_distance, double x, double y, double lu, double lv, Vec* origin,
                                         Vec* direction) {
    double dx, dy;
    lens_disc(lu, lv, &dx, &dy);
    const double k = film_distance / focus_distance;
    const double a = lens_radius * dx, b = lens_radius * dy;
    origin->x = location[0] + (a * right[0] + b * up[0]);
    origin->y = location[1] + (a * right[1] + b * up[1]);
    origin->z = location[2] + (a * right[2] + b * up[2]);
    *direction = normalize(film_to_world(right, up, forward, film_distance, x - a * k, y - b * k));
}

}  // namespace camera
}  // namespace vr
