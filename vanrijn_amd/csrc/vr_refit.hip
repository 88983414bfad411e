// vr_refit.hip -- the device stages of vr_scene_update_mesh (include/vanrijn_amd.h): new vertices for
// one mesh of a resident scene, its two trees refitted in place.  Topology, ranks and leaf order stay;
// only triangle records and boxes change.
//
//   validate   one pass over the caller's arrays: non-finite coordinates, max |coordinate| (the scene
//              extent) and the shading_finite predicate (VR_SCENE_INFO_NAN_FREE), reduced into four
//              words the host reads back before anything is modified
//   gather     slot i of the mesh's TriVerts / TriNormals takes input triangle slot_src[i]
//   refit      both trees bottom-up, ONE LAUNCH PER LEVEL, deepest first: a level reads only triangle
//              records and nodes of deeper levels, which earlier launches of the stream wrote.  Kernel
//              boundaries are the only synchronisation: no thread waits for another, and no
//              workgroup consumes what another wrote in the same launch (that would need an
//              agent-scope release / acquire per hand-off, and fail as a silently stale box).
//   root       Bvh::root_box and root_box32 of the mesh's root record
//
// vr_scene_transform_mesh runs the same refit after two passes of its own over the mesh's resident
// base records instead of validate and gather: transform-validate and transform-write.
//
// vr_scene_set_mesh_materials has two kernels here beside the gather, whose slot -> input triangle table
// they share: the largest index of the caller's array (read back before anything is written) and the
// scatter of material + 1 into the last 8 bytes of the normal records.
//
// The per-record arithmetic lives in vr_refit.h, shared with the host refit of VR_SCENE_HOST_ONLY
// scenes: min / max and outward rounding only, so the stored bits do not depend on who computed them.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "vr_layout.h"
#include "vr_refit.h"

namespace vr {
namespace refit {

constexpr int kBlock = 256;

// a workgroup's per-thread shares of a Validation into *out (zeroed before the launch)
__device__ inline void reduce_validation(unsigned long long nonfinite, unsigned long long not_finite, double max_abs,
                                         Validation* out) {
    __shared__ unsigned long long s_bad[kBlock], s_nf[kBlock], s_max[kBlock];
    s_bad[threadIdx.x] = nonfinite;
    s_nf[threadIdx.x] = not_finite;
    s_max[threadIdx.x] = (unsigned long long)__double_as_longlong(max_abs);  // >= 0: ordered as integers
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            s_bad[threadIdx.x] += s_bad[threadIdx.x + w];
            s_nf[threadIdx.x] += s_nf[threadIdx.x + w];
            s_max[threadIdx.x] = s_max[threadIdx.x] < s_max[threadIdx.x + w] ? s_max[threadIdx.x + w] : s_max[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_bad[0]) atomicAdd(&out->nonfinite, s_bad[0]);
        if (s_nf[0]) atomicAdd(&out->not_finite, s_nf[0]);
        atomicMax(&out->max_abs, s_max[0]);
    }
}

__global__ void __launch_bounds__(kBlock) validate_kernel(const double* __restrict__ verts, const double* __restrict__ norms,
                                                          uint64_t n, Validation* out) {
    unsigned long long nonfinite = 0, not_finite = 0;
    double max_abs = 0.0;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kBlock) {
        double v[9], nn[9];
        for (int i = 0; i < 9; ++i) {
            v[i] = verts[9 * t + i];
            nn[i] = norms[9 * t + i];
        }
        for (int i = 0; i < 9; ++i) {
            if (!isfinite(v[i])) ++nonfinite;
            const double a = fabs(v[i]);
            max_abs = max_abs < a ? a : max_abs;  // std::max(extent, |v|): a NaN never replaces it
        }
        if (!tri_shading_finite(v, nn)) ++not_finite;
    }
    reduce_validation(nonfinite, not_finite, max_abs, out);
}

// Destination records are 80 B at 16-B alignment: five dwordx4 stores each.  The last quad of a
// TriVerts holds v[8] and the rank, of a TriNormals n[8] and the triangle's material word (`pad` below):
// both are read and stored back unchanged.  Source rows are 72 B at 8-B alignment (dwordx2 loads).
__global__ void __launch_bounds__(kBlock) gather_kernel(const double* __restrict__ verts, const double* __restrict__ norms,
                                                        const uint32_t* __restrict__ slot_src, uint64_t n,
                                                        TriVerts* tris, TriNormals* normals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = slot_src[i];
    const double* v = verts + 9 * src;
    const double* m = norms + 9 * src;
    double2* tv = reinterpret_cast<double2*>(tris + i);
    double2* tn = reinterpret_cast<double2*>(normals + i);
    const double rank = tv[4].y, pad = tn[4].y;  // bit patterns, moved not computed
    for (int q = 0; q < 4; ++q) {
        tv[q] = make_double2(v[2 * q], v[2 * q + 1]);
        tn[q] = make_double2(m[2 * q], m[2 * q + 1]);
    }
    tv[4] = make_double2(v[8], rank);
    tn[4] = make_double2(m[8], pad);
}

// vr_scene_transform_mesh.  The base is a copy of the mesh's 80-B records in slot order (rank and
// padding included), so both passes read record i with five dwordx4 loads per array and need no gather.
__device__ inline void load_base(const TriVerts* base_tris, const TriNormals* base_normals, uint64_t i, double bv[10],
                                 double bn[10]) {
    const double2* tv = reinterpret_cast<const double2*>(base_tris + i);
    const double2* tn = reinterpret_cast<const double2*>(base_normals + i);
    for (int q = 0; q < 5; ++q) {
        const double2 a = tv[q], b = tn[q];
        bv[2 * q] = a.x;
        bv[2 * q + 1] = a.y;
        bn[2 * q] = b.x;
        bn[2 * q + 1] = b.y;
    }
}

// the Validation of the transformed records, before anything is written
__global__ void __launch_bounds__(kBlock) transform_validate_kernel(const TriVerts* __restrict__ base_tris,
                                                                    const TriNormals* __restrict__ base_normals, uint64_t n,
                                                                    Affine a, Validation* out) {
    unsigned long long nonfinite = 0, not_finite = 0;
    double max_abs = 0.0;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kBlock) {
        double bv[10], bn[10], v[9], nn[9];
        load_base(base_tris, base_normals, t, bv, bn);
        transform_tri(a, bv, bn, v, nn);
        validate_tri(v, nn, nonfinite, max_abs, not_finite);
    }
    reduce_validation(nonfinite, not_finite, max_abs, out);
}

// slot i of the mesh takes the transform of base record i: five dwordx4 stores per array, as
// gather_kernel; the last quads carry the base copy's rank and padding, which are the slot's own
__global__ void __launch_bounds__(kBlock) transform_write_kernel(const TriVerts* __restrict__ base_tris,
                                                                 const TriNormals* __restrict__ base_normals, uint64_t n,
                                                                 Affine a, TriVerts* tris, TriNormals* normals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double bv[10], bn[10], v[9], nn[9];
    load_base(base_tris, base_normals, i, bv, bn);
    transform_tri(a, bv, bn, v, nn);
    double2* tv = reinterpret_cast<double2*>(tris + i);
    double2* tn = reinterpret_cast<double2*>(normals + i);
    for (int q = 0; q < 4; ++q) {
        tv[q] = make_double2(v[2 * q], v[2 * q + 1]);
        tn[q] = make_double2(nn[2 * q], nn[2 * q + 1]);
    }
    tv[4] = make_double2(v[8], bv[9]);  // bit patterns, moved not computed
    tn[4] = make_double2(nn[8], bn[9]);
}

// vr_scene_set_mesh_materials: the largest index of the caller's array, reduced as reduce_validation
// does, so that the host rejects an out-of-range one before anything is written
__global__ void __launch_bounds__(kBlock) materials_max_kernel(const uint32_t* __restrict__ materials, uint64_t n,
                                                               unsigned long long* out) {
    __shared__ uint32_t s_max[kBlock];
    uint32_t m = 0;
    for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (uint64_t)gridDim.x * kBlock)
        m = m < materials[t] ? materials[t] : m;
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            s_max[threadIdx.x] = s_max[threadIdx.x] < s_max[threadIdx.x + w] ? s_max[threadIdx.x + w] : s_max[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(out, (unsigned long long)s_max[0]);
}

// Slot i takes materials[slot_src[i]] + 1 (materials == nullptr: 0, the mesh's own material).  Only the
// last 8 bytes of each 80-B record are written, as one aligned double -- the form the gather moves them
// in; n[0..8] are not touched.  base_normals: the transform's base copy, in the same slot order
__global__ void __launch_bounds__(kBlock) materials_scatter_kernel(const uint32_t* __restrict__ materials,
                                                                   const uint32_t* __restrict__ slot_src, uint64_t n,
                                                                   TriNormals* normals, TriNormals* base_normals) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const long long own = materials ? (long long)materials[slot_src[i]] + 1 : 0;
    const double bits = __longlong_as_double(own);
    reinterpret_cast<double*>(normals + i)[9] = bits;
    if (base_normals) reinterpret_cast<double*>(base_normals + i)[9] = bits;
}

__global__ void __launch_bounds__(kBlock) refit_level_kernel(Node* nodes, const TriVerts* tris, const int32_t* __restrict__ items,
                                                             uint32_t count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < count) refit_node(nodes, tris, items[t]);
}

__global__ void __launch_bounds__(kBlock) refit_level4_kernel(Node4* nodes4, const TriVerts* tris,
                                                              const int32_t* __restrict__ items, uint32_t count) {
    const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
    if (t < count) refit_node4(nodes4, tris, items[t]);
}

__global__ void refit_root_kernel(Bvh* bvh, const Node* nodes, const TriVerts* tris) {
    if (blockIdx.x == 0 && threadIdx.x == 0) refit_root(bvh, nodes, tris);
}

}  // namespace refit

int launch_refit_validate(const double* verts, const double* norms, uint64_t n, unsigned long long* out4, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(out4, 0, sizeof(refit::Validation), st);
    if (e != hipSuccess || n == 0) return (int)e;
    const uint64_t blocks = (n + refit::kBlock - 1) / refit::kBlock;
    refit::validate_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(refit::kBlock), 0, st>>>(
        verts, norms, n, reinterpret_cast<refit::Validation*>(out4));
    return (int)hipGetLastError();
}

int launch_refit_gather(const double* verts, const double* norms, const uint32_t* slot_src, uint64_t n, TriVerts* tris,
                        TriNormals* normals, void* stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + refit::kBlock - 1) / refit::kBlock;
    refit::gather_kernel<<<dim3((unsigned)blocks), dim3(refit::kBlock), 0, (hipStream_t)stream>>>(verts, norms, slot_src, n,
                                                                                                   tris, normals);
    return (int)hipGetLastError();
}

int launch_transform_validate(const TriVerts* base_tris, const TriNormals* base_normals, uint64_t n,
                              const refit::Affine& a, unsigned long long* out4, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(out4, 0, sizeof(refit::Validation), st);
    if (e != hipSuccess || n == 0) return (int)e;
    const uint64_t blocks = (n + refit::kBlock - 1) / refit::kBlock;
    refit::transform_validate_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(refit::kBlock), 0, st>>>(
        base_tris, base_normals, n, a, reinterpret_cast<refit::Validation*>(out4));
    return (int)hipGetLastError();
}

int launch_transform_write(const TriVerts* base_tris, const TriNormals* base_normals, uint64_t n, const refit::Affine& a,
                           TriVerts* tris, TriNormals* normals, void* stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + refit::kBlock - 1) / refit::kBlock;
    refit::transform_write_kernel<<<dim3((unsigned)blocks), dim3(refit::kBlock), 0, (hipStream_t)stream>>>(
        base_tris, base_normals, n, a, tris, normals);
    return (int)hipGetLastError();
}

int launch_materials_max(const uint32_t* materials, uint64_t n, unsigned long long* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(out, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess || n == 0) return (int)e;
    const uint64_t blocks = (n + refit::kBlock - 1) / refit::kBlock;
    refit::materials_max_kernel<<<dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(refit::kBlock), 0, st>>>(materials, n,
                                                                                                                 out);
    return (int)hipGetLastError();
}

int launch_materials_scatter(const uint32_t* materials, const uint32_t* slot_src, uint64_t n, TriNormals* normals,
                             TriNormals* base_normals, void* stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + refit::kBlock - 1) / refit::kBlock;
    refit::materials_scatter_kernel<<<dim3((unsigned)blocks), dim3(refit::kBlock), 0, (hipStream_t)stream>>>(
        materials, slot_src, n, normals, base_normals);
    return (int)hipGetLastError();
}

int launch_refit_levels(Node* nodes, Node4* nodes4,const TriVerts* tris, const int32_t* items, const uint32_t* host_first,
                        uint32_t levels, void* stream) {
    for (uint32_t l = levels; l-- > 0;) {
        const uint32_t count = host_first[l + 1] - host_first[l];
        if (count == 0) continue;
        const unsigned blocks = (count + refit::kBlock - 1) / refit::kBlock;
        if (nodes4)
            refit::refit_level4_kernel<<<dim3(blocks), dim3(refit::kBlock), 0, (hipStream_t)stream>>>(
                nodes4, tris, items + host_first[l], count);
        else
            refit::refit_level_kernel<<<dim3(blocks), dim3(refit::kBlock), 0, (hipStream_t)stream>>>(
                nodes, tris, items + host_first[l], count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

int launch_refit_root(Bvh* bvh, const Node* nodes, const TriVerts* tris, void* stream) {
    refit::refit_root_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(bvh, nodes, tris);
    return (int)hipGetLastError();
}

}  // namespace vr
