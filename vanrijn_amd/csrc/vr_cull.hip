// vr_cull.hip -- the camera-frustum cull of a launch's 8x8 pixel blocks and the compaction of the live
// ones into the render kernel's item space (gfx950).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_layout.h"
#include "vr_exp_table.h"
#include "vr_camera.h"

#include "vr_device.h"

namespace vr {
namespace dev {

// Camera-frustum test of the tile's 8x8 pixel blocks (one thread per block).  The camera rays of a
// block start at the camera and pass through the film rectangle its pixels' sample squares cover
// (camera.rs:24-66: x = (col + u) fw/w - fw/2, y = (h - row - 1 + v) fh/h - fh/2, u, v in [0, 1),
// direction d(x, y) = x right + y up + film_distance forward normalised: vr_camera.h's rule, so
// (x, y, 1) under the default pose).  d is affine in (x, y), so the block's directions are the
// parallelogram spanned by d at the rectangle's four corners, in world space, where every test
// below is made.  A block is culled only when every such line provably misses every object, with
// margins far beyond the f64 rounding of the reference's tests:
//  * a plane (plane.rs:49-75): its t = num / dn is negative for every ray -- num and n . d
//    of opposite signs at all four corners of the rectangle (n . d is affine on the parallelogram:
//    its extremes are at the corners), each by more than 1e-9 of its magnitude scale;
//  * a BVH root box (a ray that misses the box misses every triangle in it) wholly in front of the
//    camera: its corners p - location in camera coordinates (p . right, p . up, p . forward) =: (px,
//    py, pz); the directions that reach the box have (x, y) / film_distance inside the bounding
//    rectangle of the corners' (px / pz, py / pz), which, widened, misses the block's film
//    rectangle divided by film_distance.  The dot products apply the basis' transpose where its
//    inverse is meant.  vr_scene_set_camera_pose admits a basis B = [right up forward] with
//    |B^T B - I| <= 1e-9 per entry, so with w = (x, y, film_distance) the computed triple is
//    t (w + E w), |E w|_i <= 1e-9 (|x| + |y| + film_distance), and px / pz is off x / film_distance
//    by at most 1e-9 s^2 (1 + 1e-9 s), s = 1 + (|x| + |y|) / film_distance: the rectangle is widened
//    by 1e-6 s^2 with s from the computed bounds, a thousand times that and the f64 rounding of the
//    dot products (the front test leaves |px|, |py| <= 1e6 pz, so 1e-9 s stays below 1e-2);
//  * a sphere, or a root box through its bounding sphere: the camera is outside it and the angle
//    between the sphere's centre and the axis of the block's cone of directions exceeds the cone's
//    half-angle (attained at a corner) plus the sphere's angular radius plus 1e-6 rad.  A cone of
//    half-angle below 90 degrees is convex, so holding the four corner directions it holds every
//    positive combination of them: every direction of the block (a wider cone is not used).
// Under a lens (vr_camera.h: the lens rule) a sample's ray leaves the lens point o' = o + a right + b up,
// |(a, b)| <= lens_radius * |disc| with |disc| <= 1 + a few ulp, and its direction is the pinhole
// direction of the film point (x - a k, y - b k), k = film_distance / focus_distance.  With rho =
// lens_radius (1 + 1e-6) -- the disc's excess, the products' rounding and the 1e-9 the basis may be off
// orthonormal (|a right + b up| <= |(a, b)| sqrt(1 + 2e-9)) a hundred times over -- two widenings
// carry every test over, and with lens_radius 0 every number below is what it was:
//  * directions: the block's film rectangle grows by rho k on each side before the corner directions
//    are formed, so the parallelogram and the cone hold every lens ray's direction;
//  * origins: a ray from o' that meets a sphere (c, r) runs within |o' - o| <= rho of the same
//    direction's ray from o, which then meets the sphere (c, r + rho): spheres, and boxes' bounding
//    spheres, are tested from o with their radius inflated by rho.  A plane's num from o' is off its
//    value from o by (o' - o) . n, at most rho |n|: |num| must exceed its tolerance plus rho |n|, and
//    then keeps its sign over the lens.  A box corner seen from o' has camera coordinates (px - a', py
//    - b', pz - c') with |a'|, |b'| <= rho and |c'| <= 1e-6 lens_radius (a right . forward + b up .
//    forward, at most 2e-9 of it): the front test must hold for the smallest pz and the largest |px|,
//    |py|, and the bounding rectangle takes each corner's extremes (px +- rho) / pz over both ends of
//    pz's range (a quotient monotone in pz takes its extremes there).
// A lens so wide that nothing can be proved -- a cone past 90 degrees, corner directions on both sides
// of every plane -- leaves every block live: slower, never wrong.
// Each sample of a culled block is then exactly the missed camera ray's photon {0, 0}, whatever
// its random draws.
__device__ __forceinline__ double vr_angle(V3 a, V3 b) {
    return atan2(sqrt(dot(cross(a, b), cross(a, b))), dot(a, b));
}
__global__ __launch_bounds__(256) void block_cull_kernel(RenderArgs A, const Prim* prims, const Bvh* bvhs,
                                                         uint8_t* mask, PoseArgs pose, LensArgs lens) {
    const uint32_t bw = (uint32_t)((A.tile_width + 7) / 8), bh = (uint32_t)((A.tile_height + 7) / 8);
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= bw * bh) return;
    const uint32_t bx = b % bw, by = b / bw;
    const double c0 = (double)(A.start_column + 8 * (uint64_t)bx);
    const double c1 = (double)(A.start_column + min((uint64_t)8 * bx + 8, A.tile_width));
    const double r0 = (double)(A.start_row + 8 * (uint64_t)by);
    const double r1 = (double)(A.start_row + min((uint64_t)8 * by + 8, A.tile_height));
    const double H = (double)A.height;
    const double xa = c0 * A.film[0] - A.film[1], xb = c1 * A.film[0] - A.film[1];
    const double ya = (H - r1) * A.film[2] - A.film[3], yb = (H - r0) * A.film[2] - A.film[3];
    const double mx = 1e-9 * (fabs(xa) + fabs(xb) + 1.0), my = 1e-9 * (fabs(ya) + fabs(yb) + 1.0);
    const DeviceScene& S = A.scene;
    const double fd = pose.film_distance;
    // the lens: rho bounds the lens point's distance from the location, rho k the film point's shift
    const double rho = lens.lens_radius * (1.0 + 1e-6), dz = 1e-6 * lens.lens_radius;
    const double lw = rho * (fd / lens.focus_distance);
    const double xlo = (fmin(xa, xb) - mx) - lw, xhi = (fmax(xa, xb) + mx) + lw;
    const double ylo = (fmin(ya, yb) - my) - lw, yhi = (fmax(ya, yb) + my) + lw;
    const V3 R = ldv(pose.right), U = ldv(pose.up), F = ldv(pose.forward);
    // the rule at the rectangle's corners: the block's directions in world space, not normalised
    V3 pc[4];
    for (int k = 0; k < 4; ++k) {
        const camera::Vec d =
            camera::film_to_world(pose.right, pose.up, pose.forward, fd, (k & 1) ? xhi : xlo, (k & 2) ? yhi : ylo);
        pc[k] = mk(d.x, d.y, d.z);
    }
    V3 axis = mk(0.0, 0.0, 0.0);
    for (int i = 0; i < 4; ++i) axis = add(axis, normalize(pc[i]));
    axis = normalize(axis);
    double half = 0.0;
    for (int i = 0; i < 4; ++i) half = fmax(half, vr_angle(axis, pc[i]));
    const bool convex = half < 1.5;  // a cone below 90 degrees (1.5708 rad) bounds its corners' hull
    const V3 o = mk(S.camera[0], S.camera[1], S.camera[2]);
    // a sphere (centre c, radius r) every ray of the block misses
    auto sphere_clear = [&](V3 c, double r0) {
        const double r = r0 + rho;  // the lens' origins (above)
        const V3 v = sub(c, o);
        const double dist = sqrt(dot(v, v));
        if (!convex || !(dist > r * (1.0 + 1e-6) + 1e-9)) return false;
        return vr_angle(axis, v) > half + asin(fmin(1.0, r / dist)) + 1e-6;
    };
    bool clear = true;
    for (int i = 0; i < A.scene.prim_count && clear; ++i) {
        const Prim& pr = prims[i];
        const V3 c = ldv(pr.vec);
        if (pr.kind == 0) {
            const V3 q = ldv(pr.pre);
            const double num = dot(sub(q, o), c);
            const double nn = sqrt(dot(c, c));
            const double tol = 1e-9 * nn * (sqrt(dot(q, q)) + sqrt(dot(o, o)) + 1.0);
            if (!(fabs(num) > tol + rho * nn)) {
                clear = false;
                break;
            }
            for (int k = 0; k < 4; ++k) {
                const double dn = dot(pc[k], c);
                const double t = 1e-9 * nn * sqrt(dot(pc[k], pc[k]));
                if (!(num > 0.0 ? dn < -t : dn > t)) clear = false;
            }
        } else {
            clear = sphere_clear(c, pr.scalar);
        }
    }
    for (int i = 0; i < A.scene.bvh_count && clear; ++i) {
        const Bvh& bv = bvhs[i];
        if (bv.root4 == INT32_MIN) continue;  // an empty mesh never hits
        const double* bb = bv.root_box;
        // a box wholly in front of the camera, in camera coordinates: the directions that reach it
        // project (px/pz, py/pz) into the bounding rectangle of its corners' projections; clear
        // when that rectangle, widened, misses the block's film rectangle over film_distance
        double ulo = INFINITY, uhi = -INFINITY, vlo = INFINITY, vhi = -INFINITY;
        bool front = true;
        for (int k = 0; k < 8; ++k) {
            const V3 p = mk(bb[k & 1] - o.x, bb[2 + ((k >> 1) & 1)] - o.y, bb[4 + (k >> 2)] - o.z);
            const double px = dot(p, R), py = dot(p, U), pz = dot(p, F);
            const double pzl = pz - dz, pzh = pz + dz;  // pz over the lens' origins; pz itself without a lens
            front = front && pzl > 1e-6 * ((fabs(px) + rho) + (fabs(py) + rho) + fabs(pz));
            ulo = fmin(ulo, fmin((px - rho) / pzl, (px - rho) / pzh));
            uhi = fmax(uhi, fmax((px + rho) / pzl, (px + rho) / pzh));
            vlo = fmin(vlo, fmin((py - rho) / pzl, (py - rho) / pzh));
            vhi = fmax(vhi, fmax((py + rho) / pzl, (py + rho) / pzh));
        }
        if (front) {
            // the margin: 1e-6 s^2 covers the transpose standing in for the inverse of a basis that
            // is orthonormal to 1e-9 (at most 1e-9 s^2 (1 + 1e-9 s), see above) a thousand times over
            const double s = fmax(fabs(ulo), fabs(uhi)) + fmax(fabs(vlo), fabs(vhi)) + 1.0;
            const double m = 1e-6 * s * s;
            if (uhi + m < xlo / fd || ulo - m > xhi / fd || vhi + m < ylo / fd || vlo - m > yhi / fd) continue;
        }
        const V3 c = mk(0.5 * (bb[0] + bb[1]), 0.5 * (bb[2] + bb[3]), 0.5 * (bb[4] + bb[5]));
        const V3 e = mk(bb[1] - bb[0], bb[3] - bb[2], bb[5] - bb[4]);
        clear = sphere_clear(c, 0.5 * sqrt(dot(e, e)) * (1.0 + 1e-9) + 1e-12);
    }
    mask[b] = clear ? 1 : 0;
}

// The live blocks of a cull mask (one workgroup: each thread counts a contiguous run of the index
// space, an LDS scan gives the runs' offsets, then each thread writes its run's live blocks).  The
// index space is the blocks in row-major order, or (morton) the Z-order curve over the tile's
// blocks padded to a power-of-two square: with block-major work items (RenderArgs::item_order) the
// waves in flight then cover a compact square of the image instead of a strip.
__device__ __forceinline__ uint32_t vr_compact1by1(uint32_t x) {
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}
__global__ __launch_bounds__(1024) void block_compact_kernel(const uint8_t* mask, uint32_t bw, uint32_t bh,
                                                              uint32_t side, uint32_t* live, uint32_t* count) {
    __shared__ uint32_t part[1024];
    const uint32_t n = side ? side * side : bw * bh;  // the index space
    auto block_of = [&](uint32_t i) -> int64_t {    // the live block at index i, or -1
        uint32_t b = i;
        if (side) {
            const uint32_t x = vr_compact1by1(i), y = vr_compact1by1(i >> 1);
            if (x >= bw || y >= bh) return -1;
            b = y * bw + x;
        }
        return mask[b] == 0 ? (int64_t)b : -1;
    };
    const uint32_t tid = threadIdx.x, per = (n + 1023) / 1024;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    uint32_t c = 0;
    for (uint32_t i = lo; i < hi; ++i) c += block_of(i) >= 0;
    part[tid] = c;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive Hillis-Steele scan
        const uint32_t v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint32_t off = part[tid] - c;
    for (uint32_t i = lo; i < hi; ++i) {
        const int64_t b = block_of(i);
        if (b >= 0) live[off++] = (uint32_t)b;
    }
    if (tid == 1023) *count = part[1023];
}

}  // namespace dev

int launch_block_cull(const RenderArgs& a, const PoseArgs& pose, const LensArgs& lens, uint8_t* mask, void* stream) {
    const uint64_t blocks = ((a.tile_width + 7) / 8) * ((a.tile_height + 7) / 8);
    if (blocks == 0) return 0;
    hipLaunchKernelGGL(dev::block_cull_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       a, a.scene.prims, a.scene.bvhs, mask, pose, lens);
    return (int)hipGetLastError();
}

int launch_block_compact(const uint8_t* mask, uint32_t bw, uint32_t bh, bool morton, uint32_t* live, uint32_t* count,
                         void* stream) {
    // Z-order only for near-square block grids (the padded square at most 4x the blocks)
    uint32_t side = 0;
    if (morton) {
        side = 1;
        while (side < bw || side < bh) side <<= 1;
        if ((uint64_t)side * side > 4ull * bw * bh || side > 32768) side = 0;
    }
    hipLaunchKernelGGL(dev::block_compact_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, mask, bw, bh, side, live,
                       count);
    return (int)hipGetLastError();
}

}  // namespace vr
