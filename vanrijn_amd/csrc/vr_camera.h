// vr_camera.h -- the camera ray rule, shared by the render kernel's camera step (vr_render.hip), the
// block cull beside it, camera_rays_kernel (vr_integrate.hip) and the host's vr_camera_ray
// (vr_host_rays.cpp): one definition, so all four form the same bits.
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

}  // namespace camera
}  // namespace vr
