// vr_query.hip -- device ray queries (gfx950): Sampler::sample (sampler.rs:9-20) and its
// `.is_some()` form (whitted_integrator.rs:37-38) for caller-supplied rays, one ray per lane, over
// the render kernel's 4-wide f32 tree (vr_layout.h Node4) or, with VR_QUERY_REFERENCE_WALK, over the
// binary f64 tree with vr_device.h's closest_hit / any_hit unchanged.
//
// Compiled with -ffp-contract=off like every other unit: each f64 decision is the reference's, so
// the answers are bit-identical to the oracle and to vr_trace_rays, whichever tree is walked
// (the closest hit does not depend on the tree's shape).
//
// The walk (vr_walk4.h, shared with vr_integrate.hip) restates what render_kernel keeps in lambdas
// (cull thresholds, the ordered quad loads, takes_hit, the exact leaf-box rule, the root-box test) in
// the per-lane form: a leaf met in a node step is tested at once by its own lane, there is no wave
// FIFO and no leaf round.  render_kernel itself is not touched: its lambdas close over the path state
// of a persistent wave.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/vanrijn_amd.h"
#include "vr_layout.h"
#include "vr_exp_table.h"

#include "vr_device.h"
#include "vr_walk4.h"

namespace vr {
namespace dev {

// 256 threads, one ray per lane, grid-stride over n.  REF: the binary f64 tree with closest_hit /
// any_hit of vr_device.h (the parent traversal code: the yardstick for correctness and time).
template <int STACK, bool ANY, bool REF>
__global__ __launch_bounds__(256) void query_kernel(QueryArgs A) {
    __shared__ uint32_t st[(ANY ? 1 : 2) * STACK * 256];
    const int tid = threadIdx.x;
    const DeviceScene& S = A.scene;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + tid; i < A.n; i += stride) {
        Ray r;
        r.o = ldv(A.origins + 3 * i);
        r.d = ldv(A.directions + 3 * i);
        if (A.flags & VR_QUERY_NORMALIZE) r.d = normalize(r.d);  // Ray::new (mod.rs:41-46)
        const RayPre pre = prepare(r);
        Best best;
        bool hit;
        if (REF) {
            if (ANY) {
                hit = any_hit<STACK>(S, pre, st, tid);
            } else {
                Counts cnt = {0, 0, 0, 0, 0, 0, 0, 0};
                best = closest_hit<STACK, false>(S, pre, (int*)st, (float*)(st + STACK * 256), tid, cnt);
                hit = best.kind != kNone;
            }
        } else {
            hit = walk4<STACK, ANY>(S, pre, st, tid, best);
        }
        if (ANY) {
            ((uint8_t*)A.hits)[i] = hit ? 1 : 0;
            continue;
        }
        vr_ray_hit out;
        out.distance = 0.0;
        out.primitive = 0;
        out.object = 0;
        out.reserved = 0;
        out.valid = hit ? 1 : 0;
        if (hit) {
            out.distance = best.d;
            out.object = best.object;
            out.primitive = best.kind == kPrim ? S.prims[best.index].position : best.index;
            if (best.kind == kTri) {
                for (int b = 0; b < S.bvh_count; ++b)
                    if (S.bvhs[b].object == best.object)
                        out.primitive = S.tris[best.index].rank - S.bvhs[b].tri_base;  // reference leaf position
            }
        }
        ((vr_ray_hit*)A.hits)[i] = out;
        if (!A.records) continue;
        vr_hit_record* rec = (vr_hit_record*)A.records + i;
        if (!hit) {  // what vr_trace_rays leaves for a miss
            double* z = (double*)rec;
#pragma unroll
            for (int k = 0; k < (int)(sizeof(vr_hit_record) / 8); ++k) z[k] = 0.0;
            continue;
        }
        HitInfo h;
        hit_info(S, best, pre, h);
        rec->valid = 1;
        rec->object = out.object;
        rec->primitive = out.primitive;
        rec->distance = best.d;
        rec->location[0] = h.loc.x; rec->location[1] = h.loc.y; rec->location[2] = h.loc.z;
        rec->normal[0] = h.normal.x; rec->normal[1] = h.normal.y; rec->normal[2] = h.normal.z;
        rec->tangent[0] = h.tangent.x; rec->tangent[1] = h.tangent.y; rec->tangent[2] = h.tangent.z;
        rec->cotangent[0] = h.cotangent.x; rec->cotangent[1] = h.cotangent.y; rec->cotangent[2] = h.cotangent.z;
        rec->retro[0] = h.retro.x; rec->retro[1] = h.retro.y; rec->retro[2] = h.retro.z;
    }
}

template <int STACK>
__global__ __launch_bounds__(256) void trace_kernel(TraceArgs A) {
    __shared__ int st_node[STACK * 256];
    __shared__ float st_t[STACK * 256];
    const int tid = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + tid;
    if (i >= A.n) return;
    Ray r;
    r.o = ldv(A.origins + 3 * i);
    r.d = ldv(A.directions + 3 * i);
    RayPre pre = prepare(r);
    Counts cnt = {0, 0, 0, 0, 0, 0, 0, 0};
    Best best = closest_hit<STACK, false>(A.scene, pre, st_node, st_t, tid, cnt);
    vr_hit_record* out = (vr_hit_record*)A.out + i;
    out->valid = best.kind != kNone;
    if (!best.kind) return;
    HitInfo h;
    hit_info(A.scene, best, pre, h);
    out->object = best.object;
    out->primitive = best.kind == kPrim ? A.scene.prims[best.index].position : best.index;
    if (best.kind == kTri) {
        for (int b = 0; b < A.scene.bvh_count; ++b)
            if (A.scene.bvhs[b].object == best.object)
                out->primitive = A.scene.tris[best.index].rank - A.scene.bvhs[b].tri_base;  // reference leaf position
    }
    out->distance = best.d;
    out->location[0] = h.loc.x; out->location[1] = h.loc.y; out->location[2] = h.loc.z;
    out->normal[0] = h.normal.x; out->normal[1] = h.normal.y; out->normal[2] = h.normal.z;
    out->tangent[0] = h.tangent.x; out->tangent[1] = h.tangent.y; out->tangent[2] = h.tangent.z;
    out->cotangent[0] = h.cotangent.x; out->cotangent[1] = h.cotangent.y; out->cotangent[2] = h.cotangent.z;
    out->retro[0] = h.retro.x; out->retro[1] = h.retro.y; out->retro[2] = h.retro.z;
}

}  // namespace dev

template <int STACK>
static void launch_query_t(const QueryArgs& a, dim3 grid, hipStream_t s) {
    const bool ref = (a.flags & VR_QUERY_REFERENCE_WALK) != 0;
    const dim3 block(256);
    if (a.any) {
        if (ref) hipLaunchKernelGGL((dev::query_kernel<STACK, true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((dev::query_kernel<STACK, true, false>), grid, block, 0, s, a);
    } else {
        if (ref) hipLaunchKernelGGL((dev::query_kernel<STACK, false, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((dev::query_kernel<STACK, false, false>), grid, block, 0, s, a);
    }
}

int launch_query(const QueryArgs& a, int stack_depth, int grid_limit, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (a.n == 0) return 0;
    if (stack_depth > 48) return -1000;
    // one workgroup per 256 rays, capped: the rest of a larger batch is reached by the grid stride
    const uint64_t want = (a.n + 255) / 256;
    const dim3 grid((unsigned)(want < (uint64_t)grid_limit ? want : (uint64_t)grid_limit));
    if (stack_depth <= 24) launch_query_t<24>(a, grid, s);
    else if (stack_depth <= 32) launch_query_t<32>(a, grid, s);
    else launch_query_t<48>(a, grid, s);
    return (int)hipGetLastError();
}

int launch_trace(const TraceArgs& a, int stack_depth, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (a.n == 0) return 0;
    dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
    if (stack_depth <= 24) hipLaunchKernelGGL(dev::trace_kernel<24>, grid, block, 0, s, a);
    else if (stack_depth <= 32) hipLaunchKernelGGL(dev::trace_kernel<32>, grid, block, 0, s, a);
    else if (stack_depth <= 48) hipLaunchKernelGGL(dev::trace_kernel<48>, grid, block, 0, s, a);
    else return -1000;
    return (int)hipGetLastError();
}

}  // namespace vr
