// vr_walk4.h -- the per-lane walk over the 4-wide f32 tree (vr_layout.h Node4), shared by the units
// that trace caller-supplied rays one per lane: vr_query.hip (Sampler::sample for a batch of rays) and
// vr_integrate.hip (the integrators for a batch of rays).
//
// The walk restates what render_kernel keeps in lambdas (cull thresholds, the ordered quad loads,
// takes_hit, the exact leaf-box rule, the root-box test) in the per-lane form: a leaf met in a node
// step is tested at once by its own lane, there is no wave FIFO and no leaf round.
#pragma once

#include "vr_device.h"

namespace vr {
namespace dev {

typedef int32_t vrq_i4 __attribute__((ext_vector_type(4)));

// element k (0..3, per lane) of four registers, by selects (a runtime-indexed array would live in scratch)
template <class T>
__device__ __forceinline__ T pick4(T a, T b, T c, T d, uint32_t k) {
    return k == 0 ? a : (k == 1 ? b : (k == 2 ? c : d));
}

// The walk over the 4-wide tree.  ANY: Sampler::sample(ray).is_some() -- returns at the first
// accepted primitive or triangle, no ordering, no distance cull, `best` is not written; else the
// closest hit into `best` (kind kNone: a miss).  st: this workgroup's LDS stack, node links in
// st[depth * 256 + tid] and (closest only) the entries' distances in st[(STACK + depth) * 256 + tid].
// A triangle counts only if the exact f64 line test passes on its own box and on its mesh's root
// box; an f32 test that is `sure` stands for the exact one (vr_device.h slab32).
template <int STACK, bool ANY>
__device__ __forceinline__ bool walk4(const DeviceScene& S, const RayPre& pre, uint32_t* st, int tid, Best& best) {
    const Ray32 r32 = prepare32(pre, S.extent);
    const NodeOrder no = node_near_offsets(r32);
    best.kind = kNone;
    best.d = 0.0;
    best.index = -1;
    best.rank = 0;
    best.object = 0x7fffffff;
    // primitive lists first, in object then position order (min_by keeps the first of equals; a NaN
    // distance never replaces a hit and is never replaced)
    for (int i = 0; i < S.prim_count; ++i) {
        const Prim& pr = S.prims[i];
        double d;
        bool ok;
        if (pr.kind == 0) {
            ok = plane_distance(pr, pre, d);
        } else {
            const double a = sphere_a(pre.d);
            d = sphere_distance(pr, pre, a, 1.0 / (2.0 * a));
            ok = d >= 0.0;
        }
        if (!ok) continue;
        if (ANY) return true;
        if (!best.kind || d < best.d) {
            best.d = d;
            best.kind = kPrim;
            best.index = i;
            best.object = pr.object;
        }
    }
    // f32 forms of the cull thresholds, widened by the ray's slab margin E: cull_far >= bound +
    // margin (1 + |bound|) + E, cull_behind <= -behind_margin - E (-inf for rays that may not cull
    // behind); both infinite when E is (exact_only() rays: nothing is culled by f32 values)
    float cull_far = INFINITY;
    auto set_cull_far = [&]() {
        if (ANY) return;
        const double bound = best.kind ? best.d : INFINITY;
        cull_far = round_away_f32(bound + S.margin * (1.0 + fabs(bound)) + margin_of(r32));
    };
    auto culled = [&](double tlo, double thi) {
        if (!ANY) {
            const double bound = best.kind ? best.d : INFINITY;
            if (tlo > bound + S.margin * (1.0 + fabs(bound))) return true;
        }
        return pre.behind_ok() && thi < -S.behind_margin;
    };
    set_cull_far();
    const float cull_behind = pre.behind_ok() ? round_away_f32(-S.behind_margin - margin_of(r32)) : -INFINITY;
    int cur_object = 0;
    // a leaf link: its triangle, bit 31 set when the leaf's f32 box test was too close to call --
    // then the exact line test on the triangle's own box (BoundingBox::from_points, triangle.rs:101-
    // 105: the host build's leaf box bit for bit) decides whether the reference reaches it.
    // Returns whether the triangle is hit (ANY: the answer).
    auto test_tri = [&](int e) -> bool {
        const int tri = e & 0x7fffffff;
        const TriVerts tv = load_tri(S.tris + (uint32_t)tri);
        if (e < 0) {
            double bb[6], lo, hi;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                bb[2 * a] = fmin(fmin(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
                bb[2 * a + 1] = fmax(fmax(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
            }
            if (!slab(bb, pre, lo, hi)) return false;
        }
        double b[3];
        const double d = triangle_distance(tv, pre, b);
        if (d < 0.0) return false;
        if (ANY) return true;
        // closest_intersection / min_by: the smaller distance; at equal distances the later in-order
        // leaf (higher rank) within a BVH, the earlier object across objects
        const uint32_t rk = (uint32_t)tv.rank;
        const bool closer = !best.kind | (d < best.d);
        const bool tie = (d == best.d) & ((best.object == cur_object) ? (rk > best.rank) : (cur_object < best.object));
        if (closer | tie) {
            best.d = d;
            best.kind = kTri;
            best.index = tri;
            best.rank = rk;
            best.object = cur_object;
            set_cull_far();
        }
        return true;
    };
    for (int bi = 0; bi < S.bvh_count; ++bi) {
        const Bvh& bvh = S.bvhs[bi];
        if (bvh.root4 == INT32_MIN) continue;  // empty mesh: the reference's empty leaf never hits
        cur_object = bvh.object;
        {
            float flo, fhi;
            const int rr = slab32(bvh.root_box32, r32, flo, fhi);
            if (rr == 0) continue;
            if (rr == 1) {
                if (flo > cull_far || fhi < cull_behind) continue;
            } else {
                double lo, hi;
                if (!slab(bvh.root_box, pre, lo, hi) || culled(lo, hi)) continue;
            }
        }
        if (bvh.root4 < 0) {  // a one-triangle BVH: its leaf box is the root box
            if (test_tri(~bvh.root4) && ANY) return true;
            continue;
        }
        uint32_t node = (uint32_t)bvh.root4;
        int sp = 0;
        while (true) {
            // the six quads in the ray's order and the four links, one batch of loads at 64-bit
            // addresses (scenes on either side of vr_scene_needs_wide_offsets)
            const char* const p = (const char*)S.nodes4 + ((uint64_t)node << 7);
            vr_f4 q0 = *(const vr_f4*)(p + no.x), q1 = *(const vr_f4*)(p + (no.x ^ 16u));
            vr_f4 q2 = *(const vr_f4*)(p + no.y), q3 = *(const vr_f4*)(p + (no.y ^ 16u));
            vr_f4 q4 = *(const vr_f4*)(p + no.z), q5 = *(const vr_f4*)(p + (no.z ^ 16u));
            vrq_i4 ch = *(const vrq_i4*)(p + 96);
            asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(q4), "+v"(q5), "+v"(ch));
            const vr_f4 tnx = slab32_quad(q0, r32.ix, r32.nx), tfx = slab32_quad(q1, r32.ix, r32.nx);
            const vr_f4 tny = slab32_quad(q2, r32.iy, r32.ny), tfy = slab32_quad(q3, r32.iy, r32.ny);
            const vr_f4 tnz = slab32_quad(q4, r32.iz, r32.nz), tfz = slab32_quad(q5, r32.iz, r32.nz);
            const int c[4] = {ch.x, ch.y, ch.z, ch.w};
            float f[4];
            uint32_t hm = 0, xm = 0;  // per child: taken (hit or too close to call, not culled); too close to call
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float g;
                bool maybe, sure;
                slab32_ordered(tnx[k], tny[k], tnz[k], tfx[k], tfy[k], tfz[k], r32.e2, f[k], g, maybe, sure);
                const bool pass = c[k] != kEmptyChild && maybe && !(f[k] > cull_far || g < cull_behind);
                hm |= pass ? 1u << k : 0u;
                xm |= (pass && !sure) ? 1u << k : 0u;
            }
            // leaf children at once (one copy of the triangle test: the lane's leaves one by one),
            // so their hits tighten the cull before the interior children are ordered
            uint32_t lm = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) lm |= (((hm >> k) & 1u) && c[k] < 0) ? 1u << k : 0u;
            while (lm) {
                const uint32_t k = (uint32_t)__builtin_ctz(lm);
                lm &= lm - 1;
                const int ck = pick4(c[0], c[1], c[2], c[3], k);
                const bool hit = test_tri((~ck) | (((xm >> k) & 1u) ? INT32_MIN : 0));
                if (ANY && hit) return true;
            }
            // interior children: one 32-bit key per child, the entry distance's bits (clamped below
            // at 0: non-negative f32 bits order like the values; negative NaNs clamp to 0 and positive
            // ones keep bit 31 clear, so a taken child is never dropped) over the child's slot in the
            // two low bits; 0xffffffff: not descended.  An interior child too close to call is
            // descended: its box is a superset of its leaves', so that only costs work.
            uint32_t key[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool h = ((hm >> k) & 1u) && c[k] >= 0 && !(f[k] > cull_far);
                key[k] = h ? (((uint32_t)max(__float_as_int(f[k]), 0) & ~3u) | (uint32_t)k) : 0xffffffffu;
            }
            if (!ANY) {  // nearest first: only the visiting order depends on it
                auto cas = [&](int i, int j) {
                    const uint32_t ki = key[i], kj = key[j];
                    key[i] = ki < kj ? ki : kj;
                    key[j] = ki < kj ? kj : ki;
                };
                cas(0, 1);
                cas(2, 3);
                cas(0, 2);
                cas(1, 3);
                cas(1, 2);
            }
            uint32_t next = kEmptyChild;
#pragma unroll
            for (int j = 3; j >= 0; --j) {  // farthest first, so the nearest remaining pops first
                const uint32_t kj = key[j];
                if (kj >= 0x80000000u) continue;
                const uint32_t child = (uint32_t)pick4(c[0], c[1], c[2], c[3], kj & 3u);
                if (ANY ? next == (uint32_t)kEmptyChild : j == 0) {
                    next = child;
                } else {
                    // (at most wide_stack entries are ever live: vr_host_bvh.cpp WideBuilder::stack)
                    st[sp * 256 + tid] = child;
                    // the entry distance rounded down (its two low bits cleared; 0 for a negative one)
                    if (!ANY) st[(STACK + sp) * 256 + tid] = kj & ~3u;
                    ++sp;
                }
            }
            if (next != (uint32_t)kEmptyChild) {
                node = next;
                continue;
            }
            // pop, skipping entries the improved bound has since culled
            bool found = false;
            while (sp > 0) {
                --sp;
                if (!ANY && __uint_as_float(st[(STACK + sp) * 256 + tid]) > cull_far) continue;
                node = st[sp * 256 + tid];
                found = true;
                break;
            }
            if (!found) break;
        }
    }
    return best.kind != kNone;
}

}  // namespace dev
}  // namespace vr
