// vr_refit.h -- the per-record steps of vr_scene_update_mesh, shared by the host refit (vr_host_edit.cpp,
// VR_SCENE_HOST_ONLY scenes) and the device refit (vr_refit.hip): one definition, so both store the
// same bits.  Every step is exact (min / max and outward rounding only), so a refitted tree holds
// what a bottom-up build over the same topology would store.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "vr_layout.h"

namespace vr {
namespace refit {

// what the validation pass reduces (vr_refit.hip validate_kernel; the host loop fills the same)
struct Validation {
    unsigned long long nonfinite;   // vertex coordinates that are NaN or infinite
    unsigned long long max_abs;     // bits of max |coordinate| (non-negative doubles order as integers)
    unsigned long long not_finite;  // triangles failing tri_shading_finite
    unsigned long long pad;
};

__host__ __device__ inline double dmin(double a, double b) { return fmin(a, b); }  // NaN-ignoring, as f64::min
__host__ __device__ inline double dmax(double a, double b) { return fmax(a, b); }

// f32 copies of f64 bounds rounded outward (vr_host_bvh.cpp round_lower / round_upper, the same values)
__host__ __device__ inline float round_lower32(double v) {
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, -INFINITY);
    return f;
}
__host__ __device__ inline float round_upper32(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return f;
}

// BoundingBox::from_points of a triangle's vertices (triangle.rs:101-105), layout order
__host__ __device__ inline void tri_box(const double* v, double box[6]) {
    for (int c = 0; c < 3; ++c) {
        box[2 * c] = dmin(dmin(v[c], v[3 + c]), v[6 + c]);
        box[2 * c + 1] = dmax(dmax(v[c], v[3 + c]), v[6 + c]);
    }
}

// one triangle of vr_host_scene.cpp shading_finite: the same f64 operations in the same order
__host__ __device__ inline bool tri_shading_finite(const double* v, const double* nn) {
    for (int i = 0; i < 9; ++i)
        if (!isfinite(v[i]) || !isfinite(nn[i]) || fabs(v[i]) > 1e100 || fabs(nn[i]) > 1e100) return false;
    const double e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
    const double f[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(fl > 1e-200)) return false;
    double nmax = 0.0, d[3];
    for (int k = 0; k < 3; ++k) {
        const double* n = nn + 3 * k;
        const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        nmax = nmax < len ? len : nmax;
        d[k] = n[0] * f[0] + n[1] * f[1] + n[2] * f[2];
    }
    if (!(nmax > 1e-100)) return false;
    const double m6 = 1e-6 * nmax * fl;
    return (d[0] > m6 && d[1] > m6 && d[2] > m6) || (d[0] < -m6 && d[1] < -m6 && d[2] < -m6);
}

// vr_scene_transform_mesh: the row-major 3x4 matrix [A | t] and the cofactor matrix K of A, which
// the host computes once (vr_host_edit.cpp affine_of)
struct Affine {
    double m[12];
    double k[9];
};

// One triangle of vr_scene_transform_mesh: base vertices / normals (9 f64 each) -> transformed.  The
// order of operations is the header's, with no contraction (the build's -ffp-contract=off), so the
// host form, the kernels and a restatement elsewhere give the same bits.
__host__ __device__ inline void transform_tri(const Affine& a, const double* bv, const double* bn, double* v, double* nn) {
    for (int p = 0; p < 3; ++p) {
        const double x = bv[3 * p], y = bv[3 * p + 1], z = bv[3 * p + 2];
        const double nx = bn[3 * p], ny = bn[3 * p + 1], nz = bn[3 * p + 2];
        for (int c = 0; c < 3; ++c) {
            v[3 * p + c] = ((a.m[4 * c] * x + a.m[4 * c + 1] * y) + a.m[4 * c + 2] * z) + a.m[4 * c + 3];
            nn[3 * p + c] = (a.k[3 * c] * nx + a.k[3 * c + 1] * ny) + a.k[3 * c + 2] * nz;
        }
    }
}

// one triangle's share of a Validation (max_abs as a double; the reductions store its bits)
__host__ __device__ inline void validate_tri(const double* v, const double* nn, unsigned long long& nonfinite,
                                             double& max_abs, unsigned long long& not_finite) {
    for (int i = 0; i < 9; ++i) {
        if (!isfinite(v[i])) ++nonfinite;
        const double a = fabs(v[i]);
        max_abs = max_abs < a ? a : max_abs;  // std::max(extent, |v|): a NaN never replaces it
    }
    if (!tri_shading_finite(v, nn)) ++not_finite;
}

// box[c] of both children of a binary node: a leaf child's triangle box, an interior child's union
__host__ __device__ inline void refit_node(Node* nodes, const TriVerts* tris, int32_t i) {
    Node& n = nodes[i];
    for (int c = 0; c < 2; ++c) {
        const int32_t ch = n.child[c];
        if (ch < 0) {
            tri_box(tris[~ch].v, n.box[c]);
        } else {
            const Node& k = nodes[ch];
            for (int j = 0; j < 6; ++j) n.box[c][j] = (j & 1) ? dmax(k.box[0][j], k.box[1][j]) : dmin(k.box[0][j], k.box[1][j]);
        }
    }
}

// the four slots of a 4-wide node: a leaf slot's triangle box rounded outward, an interior slot's
// union of its child node's slots (fminf / fmaxf skip the NaN bounds of empty slots); empty slots stay
__host__ __device__ inline void refit_node4(Node4* nodes4, const TriVerts* tris, int32_t i) {
    Node4& n = nodes4[i];
    for (int s = 0; s < 4; ++s) {
        const int32_t ch = n.child[s];
        if (ch == kEmptyChild) continue;
        if (ch < 0) {
            double b[6];
            tri_box(tris[~ch].v, b);
            for (int j = 0; j < 6; ++j) n.bound[j][s] = (j & 1) ? round_upper32(b[j]) : round_lower32(b[j]);
        } else {
            const Node4& k = nodes4[ch];
            for (int j = 0; j < 6; ++j) {
                const float* q = k.bound[j];
                n.bound[j][s] = (j & 1) ? fmaxf(fmaxf(q[0], q[1]), fmaxf(q[2], q[3]))
                                        : fminf(fminf(q[0], q[1]), fminf(q[2], q[3]));
            }
        }
    }
}

// Bvh::root_box (the union of everything, read from the refitted binary tree) and root_box32
__host__ __device__ inline void refit_root(Bvh* bvh, const Node* nodes, const TriVerts* tris) {
    if (bvh->root == INT32_MIN) return;  // empty mesh
    if (bvh->root < 0) {
        tri_box(tris[~bvh->root].v, bvh->root_box);
    } else {
        const Node& k = nodes[bvh->root];
        for (int j = 0; j < 6; ++j)
            bvh->root_box[j] = (j & 1) ? dmax(k.box[0][j], k.box[1][j]) : dmin(k.box[0][j], k.box[1][j]);
    }
    for (int j = 0; j < 6; ++j) bvh->root_box32[j] = (j & 1) ? round_upper32(bvh->root_box[j]) : round_lower32(bvh->root_box[j]);
}

}  // namespace refit

}  // namespace vr
