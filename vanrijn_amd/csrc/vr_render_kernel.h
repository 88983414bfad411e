// vr_render_kernel.h -- the MI355X (gfx950) hot path: camera rays, closest-hit BVH traversal,
// ray-triangle / sphere / plane tests, the SimpleRandomIntegrator path loop, Lambertian and
// reflective BSDFs and the Kahan-compensated CIE-XYZ accumulation, in one kernel.
//
// Compiled with -ffp-contract=off: every f64 expression below is written in the operation order
// of the reference's Rust text (which never contracts a*b+c), so hit/miss decisions and bounce
// directions are bit-identical to the CPU restatement in oracle/ (SURVEY.md F5/F6).  The only
// re-association is the forward (iterative) accumulation of path throughput, which changes
// values by O(1e-16) relative and no decision.
//
// Execution model:
//   * persistent waves (3 per SIMD) pull single-sample work items (pixel, sample) from a global
//     queue, 512 items per atomic into a wave-private slice (8 consecutive 8x8 pixel blocks);
//   * each lane keeps its own path state; the wave alternates a shading phase (BSDF, next ray,
//     end of sample + next camera ray) and a traversal phase that steps BVH nodes for every
//     traversing lane until 56 lanes wait to shade;
//   * traversal: per-lane ordered stack walk (LDS stack [depth][thread], node indices only) over
//     a 4-wide tree of 128-B f32 nodes with outward-rounded boxes; a box test too close to call
//     in f32 is re-run exactly in f64 on the 192-B Node4x; leaf triangles are queued (8 per lane,
//     LDS) and tested in f64 in leaf rounds when 2 lanes stall, so the triangle test runs for many
//     lanes at once;
//   * each sample's final photon {wavelength, intensity} goes to a staging buffer;
//     accumulate_kernel turns it into XYZ and folds the samples of a pixel in sample order with
//     the reference's Kahan update_pixel, so the buffers are bit-identical to sequential calls.
//
// Included by the three camera units (vr_render_cam0.hip, vr_render_cam1.hip, vr_render_cam2.hip): each
// instantiates launch_render_class for one camera mode and with it that mode's render kernels, which
// no other mode shares; vr_render_launch.hip's launch_render picks among them.
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/vanrijn_amd.h"
#include "rgb_spectrum_tables.h"
#include "vr_layout.h"
#include "vr_exp_table.h"
#include "vr_camera.h"

#include "vr_device.h"
#include "vr_shade.h"

namespace vr {
namespace dev {

// ----------------------------------------------------------------------------------------------
// Kernels
// ----------------------------------------------------------------------------------------------
__device__ __forceinline__ Ray ray_new(V3 o, V3 d) { return Ray{o, normalize(d)}; }  // mod.rs:41-46

// ----------------------------------------------------------------------------------------------
// Render kernel: persistent waves, lane-level work queue, traversal and shading interleaved.
//
// Work items are (pixel, `chunk` consecutive samples), numbered chunk-major over 8x8 pixel
// blocks; chunk = 1 by default (a pixel whose paths all run to the 128-bounce limit would
// otherwise hold one lane for chunk x 128 bounces: 6.5x on the reflective bench scene).  Lanes
// refill from a wave-private slice of the queue (`grab` items per atomic; one atomic per refill
// cost 35 %).  With whole 16x16 blocks x 256 spp per workgroup, average workgroup concurrency
// was 43 % of the chip's; with the queue it is 98 %.
//
// Inside a wave, each lane's traversal state (node, LDS stack, closest hit, pending leaves)
// stays alive across iterations: the wave steps BVH nodes for all traversing lanes until at
// least `shade_threshold` lanes have finished, then those lanes shade and rejoin (one-ray-per-
// iteration lock-step measured 25 % traversal lane utilisation; this scheme 58 %).
// ----------------------------------------------------------------------------------------------
// Lane masks straight from one v_cmp into a scalar register pair (llvm.amdgcn.icmp): __ballot of a
// bool that already lives in a lane mask is lowered to v_cndmask + v_cmp (two extra VALU per vote,
// on the phase-B loop's every iteration)
__device__ __forceinline__ uint64_t lanes_ieq(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 32); }
__device__ __forceinline__ uint64_t lanes_ine(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 33); }
__device__ __forceinline__ uint64_t lanes_igt(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 38); }
__device__ __forceinline__ uint64_t lanes_ige(int a, int b) { return __builtin_amdgcn_sicmp(a, b, 39); }
__device__ __forceinline__ uint64_t lanes_uge(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 35); }
__device__ __forceinline__ uint64_t lanes_ugt(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, 34); }
__device__ __forceinline__ uint64_t exec_mask() { return __builtin_amdgcn_read_exec(); }
// set bits of the wave mask m in lanes below this one (two v_mbcnt, no lane-mask registers)
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// Items of one launch: the first spp - tail samples in chunks of `chunk`, then the last `tail`
// samples one per item, so that a path that runs to the recursion limit near the end of the
// launch holds one lane for one path, not for `chunk` of them.
// keeps a wave-uniform 64-bit value in SGPRs
__device__ inline uint64_t uniform64(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

__host__ __device__ inline uint32_t tail_of(const RenderArgs& a) {
    return a.tail_samples < a.spp ? a.tail_samples : a.spp;
}
__host__ __device__ inline uint64_t chunk_rounds(const RenderArgs& a) {
    const uint32_t bulk = a.spp - tail_of(a);
    return (bulk + a.chunk - 1) / a.chunk;
}
__host__ __device__ inline uint64_t render_items(const RenderArgs& a, uint64_t per_chunk) {
    return per_chunk * (chunk_rounds(a) + tail_of(a));
}

// kRayReady: the lane's next ray (pre.o, pre.d) is set and begin_ray runs once for all such
// lanes at the end of phase A (one inlined copy for bounce and camera rays alike)
//
// Wave-level leaf queue: the leaf triangles a wave's lanes meet go to one FIFO per wave, tagged
// with the lane whose ray met them, and a leaf round hands the oldest 64 to the 64 lanes -- each
// tests one against its owner's ray (fetched by cross-lane permute), and the owners merge their
// results through LDS atomics.  The f64 triangle test then runs with every lane busy; with per-lane
// queues a round tested one triangle per lane that had one (17 of 64).
//
// Wave priority by phase (s_setprio; MI355X_MICROARCH.md: VALU issue is arbitrated by priority,
// then age): a wave stepping BVH nodes or testing leaves -- short, latency-bound bursts ending in
// a dependent load -- wins issue over waves in long f64 shading sequences, so its next load
// leaves sooner.  Measured (A/B): traversal 1 / shading 0: main -1.0 %, C5 -2.0 %; the reverse
// +1.1 %, +3.4 %.
//
// Experiments measured and rejected in rounds 2-3 (the f32 sphere skip, the plane-sign skip, lazy
// shear constants, per-lane leaf queues, rotated vertex loads, the hoisted sphere reciprocal, the
// cooperative tail, the partial child sort, plain staging stores) were removed from the source in
// round 4; their code is kept as a patch (profiles/r04/removed_experiments.patch) and their A/B
// numbers in DESIGN.md.
#ifndef VR_PRIO  // phase A, node step, leaf round (A/B builds: -DVR_PRIO=0,2,1 ...)
#define VR_PRIO 0, 1, 1
#endif
constexpr int kPrio[3] = {VR_PRIO};
constexpr int kPrioA = kPrio[0], kPrioNode = kPrio[1], kPrioLeaf = kPrio[2];
#ifndef VR_NODE_STEPS  // node steps per phase-B iteration (round 6: 2)
#define VR_NODE_STEPS 2
#endif
// Round 13's shorter node step and leaf append (DESIGN.md section 6 "Phase-B trims": the leaf votes from one
// compare per child, raw keys on the 16-bit stack, one test for "takes a step") are in the kernels of one
// material kind (MATS 1 and 2: the timed kernels of every scene bench.py renders).  The general-material
// kernels (MATS 3) spill VGPRs to scratch already, and there the same source change only moved the spills,
// up for some of them: they keep the longer form.
template <int MATS> constexpr bool kPhaseBTrim = MATS != 3;
constexpr int kPend = 8;  // FIFO entries per lane of a wave, on average
constexpr int kWaveList = 64 * kPend;
static_assert((kWaveList & (kWaveList - 1)) == 0, "the wave FIFO is a power-of-two ring");
// Room for a node step's leaves: the wave FIFO can take a step of all 64 lanes (4 leaves each), so
// any one lane may queue more than kPend.  Wave-uniform (q_head / q_tail are).
#define VR_ROOM (q_tail - q_head <= (uint32_t)(kWaveList - 256))

// The kernel argument block, re-read through a pointer the compiler cannot prove unchanged: the
// tree and triangle base pointers become scalar loads at their use.  Held in SGPRs for the whole
// kernel they were spilled to VGPR lanes and cost 8 v_readlane per node step (static count
// 245 -> 34; -1.7 % on the main scene, -2 % on the reflective bench scene).
typedef __attribute__((address_space(4))) const RenderArgs* KArgs;
__device__ __forceinline__ KArgs kargs() {
    KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}
#define VR_NODES4 (kargs()->scene.nodes4)
#define VR_TRIS (kargs()->scene.tris)

enum LaneState : int { kNeedRay = 0, kTraversing = 1, kTraversed = 2, kDone = 3, kRayReady = 4 };

#ifdef VR_COOP_PROF
// VR_CP_DUMP (analysis builds): a tail wave's phase sums into words 8..18 of the context's queue
// buffer, and one record per wave that ran for more than 1 ms (vr_host.cpp prints both)
__device__ void coop_prof_dump(unsigned long long* o, bool coop_on, unsigned lane, const uint64_t* cp_t,
                               const uint32_t* cp_n, uint64_t cp_r0, uint64_t cp_s, uint32_t cp_maxlive) {
    if (coop_on && lane == 0) {
        for (int i = 0; i < 4; ++i) atomicAdd(o + i, (unsigned long long)cp_t[i]);
        for (int i = 0; i < 3; ++i) atomicAdd(o + 4 + i, (unsigned long long)cp_n[i]);
        atomicAdd(o + 7, 1ull);
        atomicMax(o + 8, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - cp_r0));
        atomicAdd(o + 10, (unsigned long long)cp_n[3]);
        atomicAdd(o + 9, (unsigned long long)(__builtin_amdgcn_s_memrealtime() - cp_r0));
    }
    const uint64_t now = __builtin_amdgcn_s_memrealtime();
    if (now - cp_s > 100000 && lane == 0) {
        const unsigned long long slot = atomicAdd(o + 11, 1ull);
        if (slot < 1000) {
            unsigned long long* r = o + 16 + 6 * slot;
            r[0] = now - cp_s;
            r[1] = coop_on ? now - cp_r0 : 0;
            r[2] = cp_n[3];
            r[3] = cp_n[2];
            r[4] = cp_maxlive;
            r[5] = cp_s;
        }
    }
}
#endif

// The camera pose of the launch: render_kernel's last argument, which the kernel never names.  The camera
// step reads it from the kernel-argument segment as kargs() above reads the base pointers: ten scalar
// loads per camera ray of a wave.  Read as an ordinary argument its 20 scalar registers stay live through
// the whole kernel, on top of a register file that is full: measured, up to 98 more scalar spills and up
// to 72 B more scratch per instantiation.  It comes last because every other argument then keeps its
// offset: as a member of RenderArgs::scene it moved the scratch of most instantiations, the default
// pose's included, by shifting what follows it (DESIGN.md section 2 "Camera pose").
struct RenderKernargs {  // render_kernel's argument list as the segment holds it (every member 8-aligned)
    RenderArgs args;
    const Prim* prims;
    const Material* materials;
    const Bvh* bvhs;
    PoseArgs pose;
    LensArgs lens;
};
__device__ __forceinline__ camera::Vec posed_direction(double x, double y) {
    typedef __attribute__((address_space(4))) const RenderKernargs* Segment;
    Segment k = (Segment)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    const double r[3] = {k->pose.right[0], k->pose.right[1], k->pose.right[2]};
    const double u[3] = {k->pose.up[0], k->pose.up[1], k->pose.up[2]};
    const double f[3] = {k->pose.forward[0], k->pose.forward[1], k->pose.forward[2]};
    return camera::ray_direction(r, u, f, k->pose.film_distance, x, y);
}
// The lens rule (vr_camera.h) from pose and lens, the kernel's last two arguments, read the same way:
// twelve scalar loads per camera ray of a wave, in the lens instantiations only
__device__ __forceinline__ void lens_camera_ray(const double location[3], double x, double y, double lu, double lv,
                                                camera::Vec* o, camera::Vec* d) {
    typedef __attribute__((address_space(4))) const RenderKernargs* Segment;
    Segment k = (Segment)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));
    const double r[3] = {k->pose.right[0], k->pose.right[1], k->pose.right[2]};
    const double u[3] = {k->pose.up[0], k->pose.up[1], k->pose.up[2]};
    const double f[3] = {k->pose.forward[0], k->pose.forward[1], k->pose.forward[2]};
    camera::lens_ray(location, r, u, f, k->pose.film_distance, k->lens.lens_radius, k->lens.focus_distance, x, y, lu, lv,
                     o, d);
}

// MATS: material kinds present (1 Lambertian, 2 reflective, 3 both); code for absent kinds is
// compiled out, which keeps the reflective BSDF's acos/pow/exp off Lambertian-only scenes.
// WHITTED: the WhittedIntegrator (whitted_integrator.rs:20-87) instead of SimpleRandomIntegrator.
// COOP: the cooperative tail (coop_step below) -- instantiated for the small launches of scenes with
// a reflective material, the only ones whose time is a few trapped paths (vr_host.cpp make_args).
// BIG: 64-bit byte offsets for the node and triangle loads -- scenes whose triangle array reaches 4 GB
// (53.7 M triangles) or whose 4-wide tree has 2^25 nodes (vr_host.cpp needs_big_offsets); every other
// scene's kernels address both arrays with 32-bit offsets from the scalar base (the loads' saddr form)
// S16: 16-bit LDS stack entries (trees below 65,536 wide nodes): half the stack's LDS, so more
// workgroups fit a CU.
// CAM: the camera step's mode (RenderArgs::posed): 0 the default pose, 1 the scene's pose, 2 the scene's
// pose and lens (any pose, the default one included; two more draws per sample).  The default pose keeps
// its own instantiations, whose code is what it was before poses existed: in a kernel whose registers are
// all taken, a pose read in the shared code moved spills and scratch of a dozen instantiations whichever
// way it was loaded (DESIGN.md section 2 "Camera pose"); the lens keeps its own for the same reason, so
// the posed ones are what they were before lenses existed ("Camera lens").
// ONE: the scene has exactly one BVH and its root is a wide node (LaunchChoice::one_bvh; timed kernels
// only): start_bvhs is straight-line code for S.bvhs[0], phase B has no "next BVH" step, and the
// current BVH's object is the wave-uniform S.bvhs[0].object instead of a per-lane cursor and copy.
// With ONE = false the code is what it was before the parameter existed.
template <int STACK, bool COUNT, bool RECORD, bool DARK0, int MATS = 3, int MINW = 3, bool WHITTED = false,
          bool COOP = false, bool BIG = false, bool S16 = false, int CAM = 0, bool ONE = false>
// The scene's small uniform tables (planes / spheres, materials, BVH roots) come in again as
// restrict-qualified arguments: nothing the kernel stores can alias them, so their wave-uniform
// reads compile to scalar loads (the scalar cache) instead of vector loads through L2.
__global__ __launch_bounds__(256, MINW) void render_kernel(RenderArgs A, const Prim* __restrict__ g_prims,
                                                           const Material* __restrict__ g_materials,
                                                           const Bvh* __restrict__ g_bvhs, PoseArgs, LensArgs) {
    typedef typename std::conditional<S16, uint16_t, uint32_t>::type StackT;
    __shared__ StackT st_node[STACK * 256];
    // leaf triangles met during traversal wait for a leaf round, in which every lane tests one: the
    // f64 triangle test then runs for many lanes at once instead of for the few that reached a leaf
    // in this step.  Per wave: the FIFO of queued leaves (triangle | exact-box flag, and the owning
    // lane) and, per owner lane, one leaf round's results: entries tested, min distance bits, and
    // (max rank at that distance, its triangle)
    __shared__ int32_t wl_tri[4 * kWaveList];
    __shared__ uint8_t wl_own[4 * kWaveList];
    __shared__ unsigned long long lr_d[256], lr_key[256];  // key: rank << 32 | triangle
    __shared__ uint32_t lr_cnt[256];
    // COOP: an owner's stack column map (coop_step)
    __shared__ uint32_t coop_map[COOP ? 256 : 1];
    const int wbase = (threadIdx.x >> 6) * kWaveList;
    uint32_t q_head = 0, q_tail = 0;  // wave-uniform FIFO positions (mod kWaveList)
    const int tid = threadIdx.x;
    const unsigned lane = __lane_id();
    lr_d[tid] = ~0ull;  // each lane's result slot is only touched by its own wave
    lr_key[tid] = 0;
    lr_cnt[tid] = 0;
    if (COOP) coop_map[tid] = 0;
    DeviceScene S = A.scene;
    S.prims = g_prims;
    S.materials = g_materials;
    S.bvhs = g_bvhs;
    Counts cnt = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t sec[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t step_hist[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // counting variant: lanes per node step
    uint32_t prim_cnt[3] = {0, 0, 0};  // counting variant: sphere tests, their maybe-lanes, active lanes
#ifdef VR_MARKS  // ISA section markers for tools/isa_sections.py (analysis builds only)
#define VR_MARK(name) asm volatile(";@mark " name)
#else
#define VR_MARK(name)
#endif
#define VR_SEC(i) \
    if (COUNT && first_active_lane()) sec[i]++;
    uint64_t cyc[6] = {0, 0, 0, 0, 0, 0}, tprev = COUNT ? __builtin_amdgcn_s_memtime() : 0;
#define VR_STAMP(i)                                           \
    if (COUNT) {                                              \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();     \
        cyc[i] += t_ - tprev;                                 \
        tprev = t_;                                           \
    }
    uint32_t samples_done = 0;
    // The cooperative tail's profile (analysis builds, -DVR_COOP_PROF: where a tail wave's time goes;
    // vr_host.cpp prints the sums after the launch).  One macro family, empty in every other build:
    //   VR_CP(i)        s_memtime since the last stamp into phase i (0 phase A, 1 coop steps, 2 leaf
    //                   rounds, 3 the rest of phase B), in tail waves;
    //   VR_CPN(i, c)    event count i when c (0 lone-walk iterations, 1 leaf rounds, 2 phase A
    //                   entries, 3 lone walks);
    //   VR_CP_PHASE_A() phase A starts;  VR_CP_TAIL(n) the wave's live paths before its tail and the
    //                   tail's start time;  VR_CP_DUMP() the wave's records at its end
#ifdef VR_COOP_PROF
    uint64_t cp_t[4] = {0, 0, 0, 0}, cp_prev = 0;
    uint32_t cp_n[4] = {0, 0, 0, 0};
    uint64_t cp_r0 = 0;  // s_memrealtime (100 MHz) when the wave's tail began
    const uint64_t cp_s = __builtin_amdgcn_s_memrealtime();
    uint32_t cp_maxlive = 0;
#define VR_CP(i)                                              \
    if (coop_on) {                                            \
        const uint64_t t_ = __builtin_amdgcn_s_memtime();     \
        cp_t[i] += t_ - cp_prev;                              \
        cp_prev = t_;                                         \
    }
#define VR_CPN(i, c) \
    if (c) cp_n[i]++;
#define VR_CP_PHASE_A()                          \
    cp_prev = __builtin_amdgcn_s_memtime();      \
    VR_CPN(2, coop_on)
#define VR_CP_TAIL(n)                                                           \
    if (!coop && (n) > (int)cp_maxlive) cp_maxlive = (n);                      \
    if (coop_on && cp_r0 == 0) cp_r0 = __builtin_amdgcn_s_memrealtime();
#define VR_CP_DUMP() coop_prof_dump((unsigned long long*)A.queue + 8, coop_on, lane, cp_t, cp_n, cp_r0, cp_s, cp_maxlive)
#else
#define VR_CP(i)
#define VR_CPN(i, c)
#define VR_CP_PHASE_A()
#define VR_CP_TAIL(n)
#define VR_CP_DUMP()
#endif
    if (COUNT && A.wg_times && tid == 0) A.wg_times[2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
    const uint32_t bw = (uint32_t)((A.tile_width + 7) / 8), bh = (uint32_t)((A.tile_height + 7) / 8);
    // work items run over the live blocks only (frustum-culled blocks are not in the item space)
    const uint32_t nlive = A.live_blocks ? __builtin_amdgcn_readfirstlane(*A.live_count) : bw * bh;
    const double rcp_live = A.live_blocks ? 1.0 / (double)nlive : A.rcp_blocks;
    const uint64_t per_chunk = (uint64_t)nlive * 64;
    const uint64_t items = render_items(A, per_chunk);
    const uint64_t rounds = chunk_rounds(A);
    const double rcp_R = A.item_order ? 1.0 / (double)(rounds + tail_of(A)) : 0.0;  // block-major decode
    const uint32_t bulk = A.spp - tail_of(A);
    const uint64_t npix = A.tile_width * A.tile_height;
    uint32_t px = 0, py = 0, s_end = 0;
    int state = kNeedRay;  // with s_idx == s_end: needs a work item
    uint32_t s_idx = 0;
    bool coop_on = false;  // COOP: this wave's tail walks its last paths cooperatively (sticky)
    uint64_t w_next = 0, w_end = 0;  // this wave's slice of the queue (grab > 0)
    Rng rng;
    rng.reset(0);
    RayPre pre;
    Ray32 pre32;
    NodeOrder near_off = {0u, 32u, 64u};  // the ray's near-side quads of a Node4 (set with pre32)
    Best best;
    int node = -1, sp = 0, bvh_i = 0, cur_object = 0;  // (ONE: bvh_i and cur_object are never touched)
    // the object of the BVH being walked: the lane's copy, or the only BVH's (a scalar).  An expression,
    // not a lambda: with ONE = false it is `cur_object` to the compiler, and the generic kernels keep
    // their code instruction for instruction
#define VR_WALKED_OBJECT (ONE ? S.bvhs[0].object : cur_object)
    int np = 0;  // this lane's queued leaf triangles not yet tested
    // f32 forms of the cull thresholds, widened by the ray's slab margin E (vr_device.h Ray32):
    // cull_far >= bound + margin + E (rounded up), cull_behind <= -behind_margin - E (rounded down;
    // -inf when behind-culling is off), compared with the slab values lo / hi as computed
    float cull_far = INFINITY, cull_behind = -INFINITY;
    int depth = -1, bounces = 0, flags = 0;
    double lambda = 0.0, T = 1.0, Acc = 0.0, T0 = 1.0, Acc0 = 0.0, b0 = 0.0, wo_y = 0.0;
    double Wa = 0.0, Wb = 0.0;  // Whitted: the pending continuation's throughput and constant
    // PATHWL: the ONE kernels of one material kind look intensities up on the one wavelength grid the scene's
    // material rows share (the host launches them for no other scene: vr_host.cpp launch_choice), read from
    // its wave-uniform copy, row 0, with scalar loads; every other instantiation keeps spectrum_fast on
    // the lane's own row, and its code.
    // CARRY: of these the Lambertian-only ones find the wavelength's segment and ratio on that grid once
    // per path, where lambda is drawn (vr_device.h path_segment), and every intensity lookup of the path --
    // the surface colour in shade, the sky at its end -- blends its two samples with them instead of finding
    // them again (two range compares, the index, two dependent knot loads and an f64 division per lookup).
    // The three registers come from the `flags` word, which these kernels do not have (NOFLAGS): no
    // Lambertian surface cuts a path (kPathCut is a mirror's or a Phong surface's), and bits 1, 2 and 4 are
    // the record kernels'.  The reflective-only ones need the word and spill already: carrying the ratio,
    // alone or with the segment, cost them 8 to 32 B more scratch, so they keep the lookup whole.
    constexpr bool PATHWL = ONE && DARK0 && (MATS == 1 || MATS == 2) && !WHITTED && !COUNT && !RECORD;
    constexpr bool CARRY = PATHWL && MATS == 1, NOFLAGS = CARRY;
#define VR_PATH_CUT (!NOFLAGS && (flags & kPathCut))
    const Material* const grid = S.materials;
    int wl_seg = -1;
    double wl_ratio = 0.0;

    // BVH cull: subtree entirely beyond the closest hit (+margin) or behind the origin
    auto culled = [&](double tlo, double thi) {
        const double bound = best.kind ? best.d : INFINITY;
        if (tlo > bound + S.margin * (1.0 + fabs(bound))) return true;
        return pre.behind_ok() && thi < -S.behind_margin;
    };
    auto set_cull_far = [&]() {
        const double bound = best.kind ? best.d : INFINITY;
        cull_far = round_away_f32(bound + S.margin * (1.0 + fabs(bound)) + margin_of(pre32));
    };
    // closest_intersection's rule for a triangle hit of the current BVH at distance d, reference rank
    // rk: the smaller distance; at equal distances the later in-order leaf (higher rank) within the
    // BVH, the earlier object across objects (sampler.rs min_by).  Branch-free selects on the rank
    // kept in `best` (round 4: the nested branch form with a global load of the best triangle's rank
    // was miscompiled in some builds -- a tie's new triangle index lost to the old one -- and the
    // load was a dependent global access inside a divergent branch anyway)
    // the triangle record of leaf link ~tri
    auto tri_at = [&](int tri) -> const TriVerts* {
        if (BIG) return VR_TRIS + (uint32_t)tri;
        return (const TriVerts*)((const char*)VR_TRIS + (uint32_t)tri * (uint32_t)sizeof(TriVerts));
    };
    // Node n's six quads of bounds in a ray's order (vr_layout.h Node4; no: the ray's near-side byte
    // offsets, each < 96): q = {near x, far x, near y, far y, near z, far z}.  Each load is the scalar
    // base plus a 32-bit per-lane offset (node << 7 | offset; the far side that ^ 16), or the node's
    // 64-bit address plus the offset when BIG.  As in load_tri, the empty asm needs all six values at
    // once, so the six loads are in flight together (left alone they were issued one after another,
    // each waiting for the one before: six memory round trips per step).
    // c: the four child links (offset 96), in the same batch.
    typedef int32_t vr_i4 __attribute__((ext_vector_type(4)));
    auto load_quads = [&](int n, const NodeOrder& no, vr_f4 (&q)[6], int (&c)[4]) {
        const char* const p = BIG ? (const char*)(VR_NODES4 + (uint32_t)n) : (const char*)VR_NODES4;
        const uint32_t b = BIG ? 0u : (uint32_t)n << 7;
        vr_f4 q0 = *(const vr_f4*)(p + (b | no.x)), q1 = *(const vr_f4*)(p + ((b | no.x) ^ 16u));
        vr_f4 q2 = *(const vr_f4*)(p + (b | no.y)), q3 = *(const vr_f4*)(p + ((b | no.y) ^ 16u));
        vr_f4 q4 = *(const vr_f4*)(p + (b | no.z)), q5 = *(const vr_f4*)(p + ((b | no.z) ^ 16u));
        vr_i4 ch = *(const vr_i4*)(p + (size_t)b + 96);  // (the load's immediate offset)
        asm volatile("" : "+v"(q0), "+v"(q1), "+v"(q2), "+v"(q3), "+v"(q4), "+v"(q5), "+v"(ch));
        q[0] = q0; q[1] = q1; q[2] = q2; q[3] = q3; q[4] = q4; q[5] = q5;
        c[0] = ch.x; c[1] = ch.y; c[2] = ch.z; c[3] = ch.w;
    };
    // Child slot k's six bounds {min x, max x, min y, max y, min z, max z} and its link (lone_walk: one
    // child per worker): element k of each quad, seven loads at immediate offsets from one address.
    // Per-lane ordered offsets as in load_quads would cost an address instruction per load on the
    // walk's critical path (C1 +1 % against the pair layout); lone_walk orders the pairs by select
    auto load_bounds = [&](int n, int k, float (&v)[6], int& c) {
        const char* const p = BIG ? (const char*)(VR_NODES4 + (uint32_t)n) : (const char*)VR_NODES4;
        const char* const a = p + (size_t)((BIG ? 0u : (uint32_t)n << 7) | ((uint32_t)k << 2));
        float v0 = *(const float*)(a), v1 = *(const float*)(a + 16);
        float v2 = *(const float*)(a + 32), v3 = *(const float*)(a + 48);
        float v4 = *(const float*)(a + 64), v5 = *(const float*)(a + 80);
        int ch = *(const int32_t*)(a + 96);
        asm volatile("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3), "+v"(v4), "+v"(v5), "+v"(ch));
        v[0] = v0; v[1] = v1; v[2] = v2; v[3] = v3; v[4] = v4; v[5] = v5;
        c = ch;
    };
    auto takes_hit = [&](double d, uint32_t rk) {
        const bool closer = !best.kind | (d < best.d);
        const int co = VR_WALKED_OBJECT;
        const bool tie = (d == best.d) & ((best.object == co) ? (rk > best.rank) : (co < best.object));
        return closer | tie;
    };
    // a queued leaf: its triangle index, bit 31 set when the leaf's f32 box test was too close to
    // call -- then the exact f64 line test on the triangle's own box (BoundingBox::from_points of
    // its vertices, triangle.rs:101-105: per axis fmin / fmax in vertex order, the host build's
    // leaf box bit for bit) decides whether the reference reaches the triangle at all
    auto test_tri = [&](int e) {
        const int tri = e & 0x7fffffff;
        const TriVerts tv = load_tri(tri_at(tri));
        if (e < 0) {
            VR_SEC(2);
            VR_MARK("exact_box");
            if (COUNT) cnt.exact_boxes++;
            double bb[6], lo, hi;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                bb[2 * a] = fmin(fmin(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
                bb[2 * a + 1] = fmax(fmax(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
            }
            if (!slab(bb, pre, lo, hi)) return;
        }
        if (COUNT) cnt.tri_tests++;
        double b[3];
        const double d = triangle_distance(tv, pre, b);
        if (d < 0.0) return;
        const uint32_t rk = (uint32_t)tv.rank;
        if (takes_hit(d, rk)) {
            best.d = d;
            best.kind = kTri;
            best.index = tri;
            best.rank = rk;
            best.object = VR_WALKED_OBJECT;
            set_cull_far();
        }
    };
    // One leaf round over the n (<= 64) oldest entries of the wave FIFO: lane i tests entry i
    // against its owner's ray.  Per owner, the round's candidate is the minimum distance and, among
    // equal distances, the highest reference rank (LDS atomics; one wave's LDS operations execute
    // in order): applied to `best` with test_tri's rule it gives what testing the entries one by
    // one in any order gives (closest_intersection keeps the later leaf on ties, sampler.rs keeps
    // the earlier object).  Called with the whole wave active.
    auto leaf_round = [&](uint32_t n) {
        const bool mine = lane < n;
        int e = 0;
        uint32_t owner = lane;
        if (mine) {
            const uint32_t pos = (q_head + lane) & (kWaveList - 1);
            e = wl_tri[wbase + pos];
            owner = wl_own[wbase + pos];
        }
        RayPre op;  // the owner's ray
        op.o.x = __shfl(pre.o.x, (int)owner);
        op.o.y = __shfl(pre.o.y, (int)owner);
        op.o.z = __shfl(pre.o.z, (int)owner);
        op.sx = __shfl(pre.sx, (int)owner);
        op.sy = __shfl(pre.sy, (int)owner);
        op.pdz = __shfl(pre.pdz, (int)owner);
        op.flags = __shfl(pre.flags, (int)owner);
        const int oslot = (tid & ~63) + (int)owner;
        double d = -1.0;
        uint32_t rank = 0;
        const int tri = e & 0x7fffffff;
        // The exact box test decides only where the triangle test hits: a leaf whose triangle
        // misses adds nothing whichever way its box test goes (bvh.rs:77-120 tests the triangle only
        // inside a hit box), so the reference's box decision is taken after the triangle test and
        // only for hitting entries -- the wave runs the six f64 divisions only when such an entry
        // exists, not whenever an entry's f32 box test was too close to call.  The counting variant
        // tests every flagged box, so its counters stay the reference's.
        TriVerts tv;
        if (mine) {
            tv = load_tri(tri_at(tri));
            double b[3];
            d = triangle_distance(tv, op, b);  // needs the owner's shear constants, not its direction
            rank = (uint32_t)tv.rank;
            if (COUNT && e >= 0) cnt.tri_tests++;
        }
        // lanes with an entry (lane < n) whose box was too close to call (e < 0) and whose triangle
        // hits (d >= 0), as compares into lane masks
        const uint64_t flagged = __builtin_amdgcn_uicmp(lane, n, 36 /* ult */) & lanes_igt(0, e);
        if (COUNT ? flagged : (flagged & __builtin_amdgcn_fcmp(d, 0.0, 3 /* oge */))) {
            op.d.x = __shfl(pre.d.x, (int)owner);
            op.d.y = __shfl(pre.d.y, (int)owner);
            op.d.z = __shfl(pre.d.z, (int)owner);
            if (mine && e < 0 && (COUNT || d >= 0.0)) {  // the leaf's f32 box test was too close to call
                VR_SEC(2);
                VR_MARK("exact_box");
                if (COUNT) cnt.exact_boxes++;
                double bb[6], lo, hi;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    bb[2 * a] = fmin(fmin(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
                    bb[2 * a + 1] = fmax(fmax(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
                }
                const bool reach = slab(bb, op, lo, hi);
                if (COUNT && reach) cnt.tri_tests++;
                if (!reach) d = -1.0;
            }
        }
        if (mine) atomicAdd(&lr_cnt[oslot], 1u);
        const bool hit = mine && d >= 0.0;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
        if (hit) atomicMin(&lr_d[oslot], bits);
        // at the minimum distance the highest rank wins; its triangle rides in the low half
        if (hit && lr_d[oslot] == bits) atomicMax(&lr_key[oslot], ((unsigned long long)rank << 32) | (uint32_t)tri);
        // owners: fold the round's candidate into the closest hit
        const uint32_t got = lr_cnt[tid];
        if (got) {
            np -= (int)got;
            const unsigned long long db = lr_d[tid];
            if (db != ~0ull) {
                const double dd = __longlong_as_double((long long)db);
                const unsigned long long key = lr_key[tid];
                const uint32_t rk = (uint32_t)(key >> 32);
                if (takes_hit(dd, rk)) {
                    best.d = dd;
                    best.kind = kTri;
                    best.index = (int)(uint32_t)key;
                    best.rank = rk;
                    best.object = VR_WALKED_OBJECT;
                    set_cull_far();
                }
            }
            lr_cnt[tid] = 0;
            lr_d[tid] = ~0ull;
            lr_key[tid] = 0;
        }
    };
    // next BVH (from bvh_i) with work; false when the ray is fully traced
    auto start_bvhs = [&]() {
        if constexpr (ONE) {  // the only BVH, a wide root: the same tests, no list to walk
            const Bvh& bvh = S.bvhs[0];
            float flo, fhi;
            const int rr = slab32(bvh.root_box32, pre32, flo, fhi);
            if (rr == 0) return false;
            if (rr == 1) {
                if (flo > cull_far || fhi < cull_behind) return false;
            } else {
                double lo, hi;
                if (!slab(bvh.root_box, pre, lo, hi) || culled(lo, hi)) return false;
            }
            node = bvh.root4;
            sp = 0;
            return true;
        }
        for (; bvh_i < S.bvh_count; ++bvh_i) {
            const Bvh& bvh = S.bvhs[bvh_i];
            if (bvh.root4 == INT32_MIN) continue;
            cur_object = bvh.object;
            if (COUNT) cnt.box_tests++;
            float flo, fhi;
            const int rr = slab32(bvh.root_box32, pre32, flo, fhi);
            if (rr == 0) continue;
            if (rr == 1) {
                if (flo > cull_far || fhi < cull_behind) continue;
            } else {
                double lo, hi;
                if (!slab(bvh.root_box, pre, lo, hi) || culled(lo, hi)) continue;
            }
            if (bvh.root4 < 0) {  // a one-triangle BVH
                test_tri(~bvh.root4);
                continue;
            }
            node = bvh.root4;
            sp = 0;
            return true;
        }
        return false;
    };
    // the lane's next ray, already in pre.o / pre.d (directions normalised; the next ray is kept
    // there, not in registers of its own that would stay live through the traversal phase):
    // primitive lists first, then the BVHs
    auto begin_ray = [&]() {
        pre = prepare(Ray{pre.o, pre.d});
        pre32 = prepare32(pre, S.extent);
        near_off = node_near_offsets(pre32);
        if (COUNT) cnt.rays++;
        best.kind = kNone;
        best.d = 0.0;
        best.index = -1;
        best.rank = 0;
        best.object = 0x7fffffff;
        VR_MARK("br_prims");
        for (int i = 0; i < S.prim_count; ++i) {
            const Prim& pr = S.prims[i];
            double dd;
            bool ok;
            if (pr.kind == 0) {
                VR_MARK("br_plane");
                ok = plane_distance(pr, pre, dd);
            } else {
                VR_MARK("br_sphere");
                // the f64 test is skipped only when, for every lane, the line clearly misses the
                // sphere or the sphere lies behind the origin or beyond the lane's best distance
                // (camera rays of a wave are coherent; so are many bounce rays)
                const uint64_t maybe_lanes = sphere_maybe32_lanes(pr, pre);
                if (maybe_lanes == 0) continue;
                if (COUNT) {
                    const int act = __popcll(exec_mask());
                    if (first_active_lane()) {
                        prim_cnt[0]++;
                        prim_cnt[1] += __popcll(maybe_lanes);
                        prim_cnt[2] += act;
                    }
                }
                {
                    const double a1 = sphere_a(pre.d);
                    dd = sphere_distance(pr, pre, a1, 1.0 / (2.0 * a1));
                }
                ok = dd >= 0.0;
            }
            if (ok && (!best.kind || dd < best.d)) {  // min_by keeps the first of equals
                best.d = dd;
                best.kind = kPrim;
                best.index = i;
                best.object = pr.object;
            }
        }
        VR_MARK("br_bvhs");
        set_cull_far();
        if (pre.behind_ok()) {
            cull_behind = round_away_f32(-S.behind_margin - margin_of(pre32));
        } else {
            cull_behind = -INFINITY;
        }
        if constexpr (!ONE) bvh_i = 0;
        node = -1;
        state = start_bvhs() ? kTraversing : kTraversed;
    };
    // the sample's final photon goes to the staging buffer; accumulate_kernel turns it into XYZ
    // (ColourXyz::from_photon of photon.scale_intensity(360)) and the Kahan sums.  finish() only
    // notes the photon; phase A stores it at one place after shading (store_photon), so a wave whose
    // lanes end their samples in different ways (camera miss, sky, recursion limit, early stop)
    // runs the staging address arithmetic once, not once per way
    bool fin = false;
    double fin_wl = 0.0, fin_I = 0.0;
    auto finish = [&](double wl, double I) {
        fin = true;
        fin_wl = wl;
        fin_I = I;
    };
    auto store_photon = [&](double wl, double I) {
        VR_SEC(6);
        VR_MARK("finish");
        double* out = A.staging + ((uint64_t)s_idx * npix + (uint64_t)py * A.tile_width + px) * 2;
        // streamed once to HBM and read once by the reduce: non-temporal, so the 16 B per sample
        // (4.3 GB per 1024^2 x 256 frame) do not evict the BVH and triangles from L2 and MALL
        __builtin_nontemporal_store(wl, &out[0]);
        __builtin_nontemporal_store(I, &out[1]);
#ifdef VR_STAGE_GUARD  // debug builds: this slot now holds this pass's photon
        A.stage_tag[(uint64_t)s_idx * npix + (uint64_t)py * A.tile_width + px] = A.stage_gen;
#endif
        if (RECORD) {
            const double Is = I * 360.0;
            const V3 c = xyz_for_wavelength(wl);
            vr_sample_record* rec =
                (vr_sample_record*)A.records + (((uint64_t)py * A.tile_width + px) * A.spp + s_idx);  // single pass
            rec->wavelength = wl;
            rec->intensity = I;
            rec->xyz[0] = c.x * Is;
            rec->xyz[1] = c.y * Is;
            rec->xyz[2] = c.z * Is;
            rec->bounces = bounces;
            rec->flags = flags & ~kPathCut;
        }
        if (COUNT) samples_done++;
        ++s_idx;
        state = kNeedRay;
    };
    // one level of SimpleRandomIntegrator::integrate (simple_random_integrator.rs:20-53) at the
    // closest hit, forward form: returns true when a bounce ray was started
    auto shade = [&]() {
        VR_SEC(3);
        VR_MARK("shade");
        HitInfo h;
        hit_info<ONE>(S, best, pre, h);
        if (COUNT && best.kind == kTri) cnt.shaded++;
        const double det = basis_det(h);
        // try_inverse() == None: the reference panics ("Expected matrix to be invertable."); the
        // fault_object test hook takes this path for hits on one object (DESIGN.md "Errors")
        if (det == 0.0 || best.object == A.fault_object) {
            flags |= 4;
            atomicOr(A.error_flag, 1);
            finish(0.0, 0.0);
            return;
        }
        const V3 w_i = mk(dot(h.tangent, h.retro), dot(h.cotangent, h.retro), dot(h.normal, h.retro));
        const Material* mat = &S.materials[h.material];
        if constexpr (WHITTED) {
            Acc = Acc + T * whitted_direct(S, h, mat, w_i, lambda,
                                           [&](const RayPre& sp) { return any_hit<STACK>(S, sp, st_node, tid); });
            if (depth >= kRecursionLimit) {  // recursion_limit 0: the continuation contributes 0
                flags |= 2;
                finish(lambda, Acc);
                return;
            }
        }
        V3 w_o;
        double pdf;
        // material kind: compiled in for the kinds the scene has (MATS 1: Lambertian only,
        // 2: reflective only, 3: any of Lambertian / reflective / Phong / dielectric)
        const int kind = MATS == 1 ? 0 : (MATS == 2 ? 1 : mat->kind);
        Fresnel fr;  // dielectric only
        if (MATS == 3 && kind == 3) fr = sample_dielectric(mat, w_i, lambda, rng, w_o, pdf);
        else sample_bsdf<MATS>(kind, w_i, rng, w_o, pdf);
        const V3 wo_world = bsdf_to_world(h, det, w_o);
        const double cosf = fabs(dot(wo_world, h.normal));
        if constexpr (WHITTED) {
            // continuation: bsdf(W retro, dir, L_next) |dir.n|, applied when its ray hits
            double ba, bb;
            bsdf_affine(mat, w_i, w_o, lambda, ba, bb);
            Wa = (T * ba) * cosf;
            Wb = (T * bb) * cosf;
            ++bounces;
            bounce_ray(h, wo_world, pre.o, pre.d);  // the next ray (state kRayReady)
            state = kRayReady;
            return;
        }
        const double c_l = CARRY    ? material_intensity_path(mat, grid, wl_seg, wl_ratio)
                           : PATHWL ? material_intensity_on(mat, grid, lambda)
                                    : material_intensity(mat, lambda);
        const double c_0 = DARK0 ? 0.0 : material_intensity(mat, 0.0);
        double a, a0, bterm;
        bool cut = false;  // this level's bsdf returns the constant 0 whatever comes from below
        if (MATS == 3 && kind == 3) dielectric_factors<DARK0>(mat, fr, w_i, w_o, pdf, cosf, a, a0, bterm);
        else level_factors<MATS>(mat, kind, w_i, w_o, pdf, cosf, c_l, c_0, a, a0, bterm, cut);
        if (depth == 0) b0 = bterm;
        // A cut level (a mirror or Phong surface met from behind) returns intensity 0 without reading
        // what comes from below (reflective_material.rs:20-24, phong_material.rs:19-21): the recursion
        // still traces the levels below it -- they count bounces, reach the limit, raise the basis
        // error -- but a NaN there (a bounce ray that re-hits its own surface at distance 0, as every
        // trapped path of a scene scaled by 1e20 does) is discarded, where T * a would turn the
        // forward product 0 * NaN.  From the cut on (kPathCut in `flags`, cleared per path and masked
        // out of the record) the products are frozen and the path's end adds nothing.
        if (!VR_PATH_CUT) {
            Acc = Acc + T * bterm;
            T = T * a;
            if (!DARK0) {
                Acc0 = Acc0 + T0 * bterm;
                T0 = T0 * a0;
            }
        }
        if (!NOFLAGS && cut) flags |= kPathCut;
        // A path whose every continuation yields intensity 0 stops here -- only in scenes the host
        // proved NaN-free (A.early_stop: every mesh triangle's shading basis is finite for any
        // barycentric point, no Phong / dielectric): the reference keeps recursing and returns
        // inner x 0, which is NaN when a later bounce is (simple_random_integrator.rs:39-53).
        const bool zero_tail = DARK0 ? (b0 == 0.0) : (T0 == 0.0 && Acc0 == 0.0);
        if (!RECORD && A.early_stop && T == 0.0 && Acc == 0.0 && zero_tail) {
            finish(lambda, 0.0);  // every continuation yields intensity 0
            return;
        }
        wo_y = wo_world.y;
        ++bounces;
        bounce_ray(h, wo_world, pre.o, pre.d);  // the next ray (state kRayReady)
        state = kRayReady;
    };

    // The launch's tail (COOP instantiations): the queue is exhausted and one or two paths are left
    // in the wave -- in a small frame of a scene with mirrors, paths trapped between facets run to
    // the 128-bounce recursion limit and set the frame's time (C1, benches/simple_scene.rs: 25 of
    // its 3,072 waves hold one or two and end at 3.5-6.4 ms, the others by 1.1 ms).  Their walks are
    // spread over the wave's lanes: with one owner every lane works for it, with two the lower half
    // of the lanes works for the lower owner and the upper half for the other.  Each step takes the
    // owner's current node and up to (workers - 1) entries from the top of its stack, one per worker,
    // tests them against the owner's ray, pushes the hit interior children back and queues the hit
    // leaves for the owner.  An owner's stack spans extra lane columns of the wave (the other lanes
    // are done): with one owner from the start, the next columns in turn; once two owners have shared
    // the wave (coop_map, sticky for the rest of the launch), each owner keeps its own column plus the
    // lanes of its half other than the two owners', so the map never changes under an owner whose
    // partner finishes first.  Culling and the order-independent leaf rounds keep the closest hit and
    // its tie rule: only the visiting order changes.  Called with the whole wave
    // active; `live` holds the one or two live lanes.
    // the LDS word of virtual stack entry v of owner o whose column map is om (coop_map)
    auto coop_vaddr = [&](int o, uint32_t om, int v) {
        const int j = v / STACK, og = (int)(om & 3) - 1, op = (int)(om >> 8);
        int col;
        if (j == 0) {
            col = o;
        } else if (og < 0) {
            col = (o + j) & 63;
        } else {  // the (j-1)-th lane of half og that is neither owner
            const int s1 = o < op ? o : op, s2 = o < op ? op : o, lo = og * 32;
            col = lo + j - 1;
            if (s1 >= lo && s1 < lo + 32 && col >= s1) ++col;
            if (s2 >= lo && s2 < lo + 32 && col >= s2) ++col;
        }
        return (v % STACK) * 256 + (tid & ~63) + col;
    };
    auto coop_step = [&](const uint64_t live) {
        uint32_t lmask = 0;
        int32_t lent[4];
        const int oa = (int)__builtin_ctzll(live);         // lower owner
        const int ob = (int)(63 - __builtin_clzll(live));  // upper owner (== oa: one owner)
        const bool two = oa != ob;
        uint32_t* cmap = &coop_map[tid & ~63];  // per lane: 0 (full map), or 1 + half | partner << 8
        if (two && cmap[oa] == 0) {
            if ((int)lane == oa) cmap[oa] = 1u | ((uint32_t)ob << 8);
            if ((int)lane == ob) cmap[ob] = 2u | ((uint32_t)oa << 8);
        }
        // this lane works for its half's owner (two owners) or the one owner
        const bool upper = two && lane >= 32;
        const int owner = upper ? ob : oa;
        const int gbase = upper ? 32 : 0, gsize = two ? 32 : 64;
        const uint64_t gmask = two ? (upper ? 0xFFFFFFFF00000000ull : 0xFFFFFFFFull) : ~0ull;
        const int r = (int)lane - gbase;  // worker rank
        const uint32_t om = cmap[owner];  // the owner's column map
        const int o_sp = __shfl(sp, owner);
        const int o_node = __shfl(node, owner);
        const bool o_trav = __shfl(state == kTraversing ? 1 : 0, owner) != 0;
        const int have = o_trav ? (o_node >= 0 ? 1 : 0) + o_sp : 0;
        // the owner's stack capacity: every column of the wave, or its own plus 30 of its half
        const int cap = ((om & 3) == 0 ? 64 : 31) * STACK;
        // entries taken this step: at most one per worker, and at most what keeps 150 entries of
        // headroom (a step adds at most 3 net per entry taken; a depth-first walk from a near-full
        // stack needs at most 3 per level below)
        int t = have < gsize ? have : gsize;
        const int room = (cap - 150 - have) / 3;
        if (t > room) t = room < 1 ? (have > 0 ? 1 : 0) : room;
        const bool work = t > 0 && VR_ROOM;  // uniform per half
        uint32_t im = 0;                     // hit interior children
        int c[4] = {0, 0, 0, 0};
        int pos = o_sp;
        // the owner's ray and cull bounds, permuted with the whole wave active: `work` differs between
        // the halves, and the upper half's owner may be a lane of the lower half (ds_bpermute reads 0
        // from a source lane outside exec)
        Ray32 ry;
        ry.ox = __shfl(pre32.ox, owner);
        ry.oy = __shfl(pre32.oy, owner);
        ry.oz = __shfl(pre32.oz, owner);
        ry.ix = __shfl(pre32.ix, owner);
        ry.iy = __shfl(pre32.iy, owner);
        ry.iz = __shfl(pre32.iz, owner);
        ry.nx = __shfl(pre32.nx, owner);
        ry.ny = __shfl(pre32.ny, owner);
        ry.nz = __shfl(pre32.nz, owner);
        ry.e2 = __shfl(pre32.e2, owner);
        const float cf = __shfl(cull_far, owner);
        const float cb = __shfl(cull_behind, owner);
        if (work) {
            VR_MARK("coop_step");
            const int first_stack = o_node >= 0 ? 1 : 0;  // worker 0 takes the current node
            int my = -1;
            if (r < t) my = (r < first_stack) ? o_node : (int)st_node[coop_vaddr(owner, om, o_sp - 1 - (r - first_stack))];
            pos = o_sp - (t - first_stack);  // stack entries left below the taken ones
            if (my >= 0) {
                if (COUNT) cnt.node_visits++;
                uint32_t xm = 0;
                // the quads in the OWNER's ray order (the node step's form, vr_device.h slab32_ordered)
                vr_f4 q[6];
                load_quads(my, node_near_offsets(ry), q, c);
                const vr_f4 tnx = slab32_quad(q[0], ry.ix, ry.nx), tfx = slab32_quad(q[1], ry.ix, ry.nx);
                const vr_f4 tny = slab32_quad(q[2], ry.iy, ry.ny), tfy = slab32_quad(q[3], ry.iy, ry.ny);
                const vr_f4 tnz = slab32_quad(q[4], ry.iz, ry.nz), tfz = slab32_quad(q[5], ry.iz, ry.nz);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float f, g;
                    bool maybe, sure;
                    slab32_ordered(tnx[k], tny[k], tnz[k], tfx[k], tfy[k], tfz[k], ry.e2, f, g, maybe, sure);
                    const bool lv = c[k] != kEmptyChild;
                    if (COUNT && lv) cnt.box_tests++;
                    const bool pass = lv && maybe && !(f > cf || g < cb);
                    xm |= (pass && !sure) ? 1u << k : 0u;
                    im |= (pass && c[k] >= 0) ? 1u << k : 0u;
                    lmask |= (pass && c[k] < 0) ? 1u << k : 0u;
                    lent[k] = (~c[k]) | (((xm >> k) & 1u) ? INT32_MIN : 0);
                }
            }
        }
        // interior hits onto the owner's stack, in (child slot, worker) order
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool ih = (im >> k) & 1u;
            const uint64_t m = __ballot(ih) & gmask;
            if (ih) st_node[coop_vaddr(owner, om, pos + (int)lanes_below(m))] = (uint32_t)c[k];
            pos += (int)__popcll(m);
        }
        // each owner takes its next node, the top of its stack: its workers' pos and work flag
        // (uniform over its half) by permute from the half's first lane
        const int lead = (two && (int)lane == ob) ? 32 : 0;
        const int npos = __shfl(pos, lead);
        const bool nwork = __shfl(work ? 1 : 0, lead) != 0;
        const bool is_owner = ((live >> lane) & 1ull) != 0;
        if (is_owner && nwork) {
            sp = npos;
            if (sp > 0) {
                --sp;
                node = (int)st_node[coop_vaddr((int)lane, cmap[lane], sp)];
            } else {
                node = -1;
            }
        }
        // the hit leaves, queued for their owners in (child slot, lane) order
        const uint64_t own_mask = two ? ((int)lane == ob ? 0xFFFFFFFF00000000ull : 0xFFFFFFFFull) : ~0ull;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool lh = (lmask >> k) & 1u;
            const uint64_t m = __ballot(lh);
            if (lh) {
                const uint32_t qp = (q_tail + (uint32_t)lanes_below(m)) & (kWaveList - 1);
                wl_tri[wbase + qp] = lent[k];
                wl_own[wbase + qp] = (uint8_t)owner;
            }
            q_tail += (uint32_t)__popcll(m);
            if (is_owner) np += (int)__popcll(m & own_mask);
        }
        q_tail = __builtin_amdgcn_readfirstlane(q_tail);
    };
    // The cooperative tail's walks with nothing pending (no stack entries, no queued leaves, an empty
    // wave FIFO) for the one to four traversing paths `own` of a wave whose other lanes are done: the
    // whole rest of each path's walk of its current BVH in one call.  With one owner every lane
    // works for it; with two the lower half works for the lower owner and the upper half for the
    // other, with three or four each quarter of the wave for one of them (round 6: C1 frames whose
    // waves kept three trapped mirror paths took 3.9-5.3 ms against ~1.55 ms, profiles/r06/split/
    // c1_frames.json), all walks at once.  An owner's frontier of nodes to visit is a LIFO over its
    // group's columns of the wave's stack words; each iteration pops up to one node per four workers, each
    // worker tests one child box against the owner's ray, the hit interior children are pushed and
    // the hit leaves tested at once, one per worker.  The round's candidate (minimum distance, then the
    // highest reference rank) is merged with takes_hit's rule, as in leaf_round, so each path gets
    // what its per-lane walk finds: only the visiting order differs.  Against coop_step it saves the
    // per-step owner-state permutes and stack remapping and the separate leaf rounds through the FIFO
    // (C1: the trapped mirror paths' last bounces).  Called with the whole wave active.
    auto lone_walk = [&](const uint64_t own) {
        // 1, 2 or up to 4 owners (wave-uniform): the whole wave, its halves or its quarters work for
        // them, group g for the g-th lowest owner lane (with 3 owners the last quarter idles)
        const int nown = __popcll(own);
        const int hshift = nown == 1 ? 6 : (nown == 2 ? 5 : 4), hs = 1 << hshift;
        const int grp = (int)lane >> hshift;
        const int hb = grp << hshift;
        const int r = (int)lane - hb;  // worker rank
        const uint64_t gmask = hs == 64 ? ~0ull : (((1ull << hs) - 1) << hb);
        // this group's owner's ray, cull bounds and closest hit, by cross-lane permute (per-lane
        // copies: uniform copies of the owners' values would need ~40 SGPRs per owner, spilled)
        const uint64_t own1 = own & (own - 1), own2 = own1 & (own1 - 1), own3 = own2 & (own2 - 1);
        const uint64_t mine_o = grp == 0 ? own : (grp == 1 ? own1 : (grp == 2 ? own2 : own3));
        const bool has_owner = mine_o != 0;
        const int ow = has_owner ? (int)__builtin_ctzll(mine_o) : (int)lane;
        auto p64 = [&](double v) { return __shfl(v, ow); };
        auto p32 = [&](float v) { return __shfl(v, ow); };
        auto pi = [&](int v) { return __shfl(v, ow); };
        RayPre op;
        op.o = mk(p64(pre.o.x), p64(pre.o.y), p64(pre.o.z));
        op.d = mk(p64(pre.d.x), p64(pre.d.y), p64(pre.d.z));
        op.sx = p64(pre.sx);
        op.sy = p64(pre.sy);
        op.pdz = p64(pre.pdz);
        op.flags = pi(pre.flags);
        Ray32 ry;
        ry.ox = p32(pre32.ox); ry.oy = p32(pre32.oy); ry.oz = p32(pre32.oz);
        ry.ix = p32(pre32.ix); ry.iy = p32(pre32.iy); ry.iz = p32(pre32.iz);
        ry.nx = p32(pre32.nx); ry.ny = p32(pre32.ny); ry.nz = p32(pre32.nz);
        ry.e2 = p32(pre32.e2);
        // the owner's order of each axis's two bounds: the sign bits of its f32 reciprocals (vr_device.h
        // slab32_ordered)
        const bool neg_x = (__float_as_uint(ry.ix) >> 31) != 0, neg_y = (__float_as_uint(ry.iy) >> 31) != 0,
                   neg_z = (__float_as_uint(ry.iz) >> 31) != 0;
        float cf = p32(cull_far);
        const float cb = p32(cull_behind);
        const int cobj = pi(cur_object);
        int bkind = pi(best.kind), bindex = pi(best.index), bobject = pi(best.object);
        uint32_t brank = (uint32_t)pi((int)best.rank);
        double bd = p64(best.d);
        // frontier entry f of this half: row f / hs, column hb + f % hs of the wave's stack words
        auto fr = [&](int f) -> StackT& {
            return st_node[(f >> hshift) * 256 + (tid & ~63) + hb + (f & (hs - 1))];
        };
        const int cap = hs * STACK;
        // a batch pushes at most 3 net entries per entry taken and stays below `safe`; above it, one
        // entry per iteration is a depth-first walk of one subtree, which needs at most the per-lane
        // walk's stack (< STACK) plus one word per level (it pushes every hit child), < 2 * STACK
        const int safe = cap - 4 * STACK;
        int32_t* const leaves = &wl_tri[wbase + grp * (hs * kPend)];  // <= 1 per worker per step
        static_assert(kPend >= 1, "each group's share of the wave FIFO holds a step's leaves");
        // the owner's current node, permuted with the whole wave active: ds_bpermute reads 0 from a
        // source lane outside exec, so a permute inside `r == 0` (lanes 0 / 32 only) would start
        // the walk at node 0 whenever the owner is another lane
        const int start = pi(node);
        if (r == 0) fr(0) = (uint32_t)start;
        int n = has_owner ? 1 : 0;  // this group's frontier size
        while (true) {
            const bool act = n > 0;
            if (__ballot(act) == 0) break;
            if (!act) continue;
            VR_MARK("lone_step");
            VR_CPN(0, true);  // lone-walk iterations (per half)
            if (n > cap - 4) {  // cannot happen (above); a device error rather than a stray LDS write
                atomicOr(A.error_flag, 1);
                n = 0;
                continue;
            }
            // four workers per node, one child each: a quarter of the per-worker instructions of
            // one worker per node (C1 2.15 -> 1.60 ms, profiles/r05/lone/ab_split_c1.jsonl)
            const int tw = hs >> 2;
            int t = n < tw ? n : tw;
            if (n + 3 * t > safe) t = (safe - n) / 3 > 1 ? (safe - n) / 3 : 1;
            const int slot = r >> 2, k = r & 3;
            const int my = slot < t ? (int)fr(n - 1 - slot) : -1;
            n -= t;
            bool ih = false, lh = false;
            int c = 0;
            int32_t le = 0;
            if (my >= 0) {
                float f, g;
                bool maybe, sure;
                // child k's six bounds, each axis's pair in the owner's ray order
                float v[6];
                load_bounds(my, k, v, c);
                const vr_f2 tx = slab32_pair(neg_x ? v[1] : v[0], neg_x ? v[0] : v[1], ry.ix, ry.nx);
                const vr_f2 ty = slab32_pair(neg_y ? v[3] : v[2], neg_y ? v[2] : v[3], ry.iy, ry.ny);
                const vr_f2 tz = slab32_pair(neg_z ? v[5] : v[4], neg_z ? v[4] : v[5], ry.iz, ry.nz);
                slab32_ordered(tx.x, ty.x, tz.x, tx.y, ty.y, tz.y, ry.e2, f, g, maybe, sure);
                const bool pass = c != kEmptyChild && maybe && !(f > cf || g < cb);
                ih = pass && c >= 0;
                lh = pass && c < 0;
                le = (~c) | ((pass && !sure) ? INT32_MIN : 0);
            }
            int nl = 0;  // hit leaves, in (node, child slot) order
            {
                const uint64_t mi = __ballot(ih) & gmask, ml = __ballot(lh) & gmask;
                if (ih) fr(n + (int)lanes_below(mi)) = (uint32_t)c;
                if (lh) leaves[(int)lanes_below(ml)] = le;
                n += (int)__popcll(mi);
                nl = (int)__popcll(ml);
            }
            for (int b = 0; b < nl; b += hs) {  // nl is uniform per half: the halves branch apart
                VR_MARK("lone_leaf");
                VR_CPN(1, true);  // lone-walk leaf rounds (per half)
                const bool mine = r < nl - b;
                double d = -1.0;
                uint64_t key = 0;
                if (mine) {
                    const int e = leaves[b + r];
                    const int tri = e & 0x7fffffff;
                    const TriVerts tv = load_tri(tri_at(tri));
                    double bb3[3];
                    d = triangle_distance(tv, op, bb3);
                    if (e < 0 && d >= 0.0) {  // the leaf's f32 box test was too close to call
                        double bb[6], lo, hi;
#pragma unroll
                        for (int a = 0; a < 3; ++a) {
                            bb[2 * a] = fmin(fmin(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
                            bb[2 * a + 1] = fmax(fmax(tv.v[a], tv.v[3 + a]), tv.v[6 + a]);
                        }
                        if (!slab(bb, op, lo, hi)) d = -1.0;
                    }
                    key = ((uint64_t)(uint32_t)tv.rank << 32) | (uint32_t)tri;
                }
                const bool hit = mine && d >= 0.0;
                const uint64_t hm = __ballot(hit) & gmask;
                if (hm == 0) continue;
                // the round's candidate over this half: the minimum distance (non-negative, so its
                // bits order as integers), and at it the highest rank (its triangle in the low half);
                // most rounds have one hit, taken by one permute
                const uint64_t db = hit ? (uint64_t)__double_as_longlong(d) : ~0ull;
                uint64_t dmin, kmax;
                if (__popcll(hm) == 1) {
                    const int src = (int)__builtin_ctzll(hm);
                    dmin = __shfl(db, src);
                    kmax = __shfl(key, src);
                } else {
                    dmin = db;
                    for (int sh = hs >> 1; sh >= 1; sh >>= 1) {
                        const uint64_t w = __shfl_xor(dmin, sh);
                        dmin = w < dmin ? w : dmin;
                    }
                    kmax = hit && db == dmin ? key : 0ull;
                    for (int sh = hs >> 1; sh >= 1; sh >>= 1) {
                        const uint64_t w = __shfl_xor(kmax, sh);
                        kmax = w > kmax ? w : kmax;
                    }
                }
                const double dd = __longlong_as_double((long long)dmin);
                const uint32_t rk = (uint32_t)(kmax >> 32);
                // takes_hit for the owner
                const bool closer = !bkind | (dd < bd);
                const bool tie = (dd == bd) & ((bobject == cobj) ? (rk > brank) : (cobj < bobject));
                if (closer | tie) {
                    bd = dd;
                    bkind = kTri;
                    bindex = (int)(uint32_t)kmax;
                    brank = rk;
                    bobject = cobj;
                    cf = round_away_f32(bd + S.margin * (1.0 + fabs(bd)) + margin_of(ry));  // set_cull_far
                }
            }
        }
        // each owner takes its group's results (from the group's first lane: the owners below it
        // count its group)
        const int src = (int)lanes_below(own) << hshift;
        const double rd = __shfl(bd, src);
        const int rkind = __shfl(bkind, src), rindex = __shfl(bindex, src), robject = __shfl(bobject, src);
        const uint32_t rrank = (uint32_t)__shfl((int)brank, src);
        const float rcf = __shfl(cf, src);
        if ((own >> lane) & 1ull) {
            best.d = rd;
            best.kind = rkind;
            best.index = rindex;
            best.rank = rrank;
            best.object = robject;
            cull_far = rcf;
            node = -1;
            sp = 0;
        }
    };
    while (true) {
        // ---------------------------------------------------------------- phase A: shade
        // repeated while some lane's new ray was resolved without BVH work (sky misses, rays
        // that only meet the plane or spheres), so those lanes do not idle through phase B
        VR_CP_PHASE_A();
        for (int rep = 0; rep < A.phase_a_reps; ++rep) {
            VR_MARK("phaseA_top");
            __builtin_amdgcn_s_setprio(kPrioA);
            if (COUNT && first_active_lane()) cnt.outer_slots += 64;
            VR_STAMP(5);
            // shading is deferred while fewer than shade_min lanes have a hit to shade and other
            // lanes still traverse: the deferred lanes wait (state kTraversed) and the next phase
            // A shades them with more lanes busy (misses are finished at once either way)
            bool shade_now = true, finish_now = true;
            if (A.shade_min | A.miss_min) {
                const bool idle = lanes_ieq(state, kTraversing) == 0;
                const uint64_t done_trav = lanes_ieq(state, kTraversed);
                const int nhit = __popcll(done_trav & lanes_ine((int)best.kind, (int)kNone));
                const int nmiss = __popcll(done_trav & lanes_ieq((int)best.kind, (int)kNone));
                shade_now = nhit >= (int)A.shade_min || idle;
                finish_now = nmiss >= (int)A.miss_min || idle;
            }
            if (state == kTraversed && (best.kind == kNone ? finish_now : shade_now)) {
                VR_MARK("traversed");
                // one call site for shade(): two inlined copies would both run whenever a wave
                // holds camera-ray hits and bounce hits at once
                bool go = false;
                fin = false;
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
                        finish(0.0, 0.0);  // camera ray missed: photon {0, 0} (camera.rs:110-113)
                    } else {
                        if (!NOFLAGS) flags |= 1;
                        lambda = 380.0 + (740.0 - 380.0) * rng.standard();  // Photon::random_wavelength
                        if constexpr (CARRY) path_segment(grid, lambda, wl_seg, wl_ratio);
                        T = 1.0; Acc = 0.0; T0 = 1.0; Acc0 = 0.0; b0 = 0.0;
                        depth = 0;
                        go = true;
                    }
                } else if (!best.kind) {
                    // simple_random_integrator.rs:43-46; below a cut level the sky term is discarded too
                    // (CARRY: a sky row on another grid than the materials' keeps its own lookup)
                    finish(lambda, VR_PATH_CUT              ? Acc
                                   : CARRY && A.sky_on_grid ? Acc + T * sky_intensity_path(wo_y, grid, wl_seg, wl_ratio)
                                                            : Acc + T * sky_intensity(wo_y, lambda, &S.materials[S.sky_row]));
                } else {
                    depth += 1;
                    if (depth == kRecursionLimit) {  // integrate(.., 0) returns {0, 0}: lambda becomes 0
                        if (!NOFLAGS) flags |= 2;
                        // the innermost photon's intensity 0 times the lambda-0 throughput: + 0
                        // when finite, NaN when a level's pdf * |cos| was (the reference's 0 * NaN);
                        // DARK0 scenes are NaN-free (host), where every lambda-0 level is 0 * I + b
                        finish(0.0, DARK0 ? b0 : VR_PATH_CUT ? Acc0 : Acc0 + T0 * 0.0);
                    } else {
                        go = true;
                    }
                }
                if (go) shade();
                if (fin) store_photon(fin_wl, fin_I);
            }
            VR_STAMP(0);
            VR_MARK("refill_check");
            // refill: lanes whose item is exhausted take the next items (one atomic per wave)
            while (true) {
                const bool need = state == kNeedRay && s_idx >= s_end;
                const uint64_t m = lanes_ieq(state, kNeedRay) & lanes_uge(s_idx, s_end);
                if (m == 0) break;
                VR_SEC(7);
                VR_MARK("refill");
                const unsigned leader = (unsigned)__builtin_ctzll(m);
                const uint32_t rank = (uint32_t)lanes_below(m);
                unsigned long long base = 0;
                bool take = need;
                if (A.grab == 0) {
                    if (lane == leader) base = atomicAdd(A.queue, (unsigned long long)__popcll(m));
                    base = __shfl(base, (int)leader);
                } else {
                    // wave-private slice of the queue: one atomic per `grab` items
                    if (w_next >= w_end) {
                        if (lane == leader) base = atomicAdd(A.queue, (unsigned long long)A.grab);
                        w_next = uniform64(__shfl(base, (int)leader));
                        w_end = w_next + A.grab;
                    }
                    const uint64_t avail = w_end - w_next;
                    base = w_next;
                    take = need && rank < avail;
                    const uint64_t want = (uint64_t)__popcll(m);
                    w_next = uniform64(w_next + (want < avail ? want : avail));
                }
                if (take) {
                    const uint64_t g = base + rank;
                    if (g >= items) {
                        state = kDone;
                    } else {
                        // g = (chunk_i * blocks + blk) * 64 + l; g >> 6 < 2^32 (the host caps
                        // a launch's items), quotients by f64 reciprocal, corrected by one
                        const uint32_t gb = (uint32_t)(g >> 6), l = (uint32_t)(g & 63);
                        uint32_t chunk_i;
                        int32_t rem;
                        if (A.item_order) {
                            // block-major: g = (blk * R + chunk_i) * 64 + l, R = the items per pixel
                            // -- the waves in flight work on few blocks at a time (see RenderArgs)
                            const uint32_t R = (uint32_t)(rounds + tail_of(A));
                            uint32_t bi = (uint32_t)((double)gb * rcp_R);
                            int32_t c = (int32_t)(gb - bi * R);
                            if (c < 0) { --bi; c += (int32_t)R; }
                            if (c >= (int32_t)R) { ++bi; c -= (int32_t)R; }
                            rem = (int32_t)bi;
                            chunk_i = (uint32_t)c;
                        } else {
                            const uint32_t nblk = (uint32_t)(per_chunk >> 6);
                            chunk_i = (uint32_t)((double)gb * rcp_live);
                            rem = (int32_t)(gb - chunk_i * nblk);
                            if (rem < 0) { --chunk_i; rem += (int32_t)nblk; }
                            if (rem >= (int32_t)nblk) { ++chunk_i; rem -= (int32_t)nblk; }
                        }
                        const uint32_t blk = A.live_blocks ? A.live_blocks[rem] : (uint32_t)rem;
                        uint32_t by = (uint32_t)((double)blk * A.rcp_bw);
                        int32_t bx = (int32_t)(blk - by * bw);
                        if (bx < 0) { --by; bx += (int32_t)bw; }
                        if (bx >= (int32_t)bw) { ++by; bx -= (int32_t)bw; }
                        const uint32_t x = (uint32_t)bx * 8 + (l & 7), y = by * 8 + (l >> 3);
                        // else padding: take another item (blocks whose camera rays all miss every
                        // object are not in the item space; their samples are the photon {0, 0},
                        // applied by the ordered reduce without staged data)
                        if (x < A.tile_width && y < A.tile_height) {
                            px = x;
                            py = y;
                            if (chunk_i < rounds) {
                                s_idx = chunk_i * A.chunk;
                                s_end = min(bulk, s_idx + A.chunk);
                            } else {
                                s_idx = bulk + (uint32_t)(chunk_i - rounds);
                                s_end = s_idx + 1;
                            }
                        }
                    }
                }
            }
            VR_STAMP(1);
            if (state == kNeedRay) {
                const uint64_t row = A.start_row + py, col = A.start_column + px;
                rng.reset(stream_base_keyed(A.seed_key, row * A.width + col, A.first_sample + s_idx));
                // ImageSampler (camera.rs:24-66): film (w/h, 1) or (1, w/h); x's draw first
                VR_SEC(4);
                VR_MARK("camera");
                // film_w * (1 / w), film_w * 0.5, ... are per-launch constants (host: make_args)
                const double ux = rng.standard();
                const double uy = rng.standard();
                const double x = camera::film_x(A.film, col, ux);
                const double y = camera::film_y(A.film, A.height, row, uy);
                depth = -1;
                bounces = 0;
                flags = 0;
                pre.o = mk(S.camera[0], S.camera[1], S.camera[2]);
                if constexpr (CAM == 2) {  // pose and lens (vr_camera.h: the lens rule); draws 2 and 3
                    const double lu = rng.standard();
                    const double lv = rng.standard();
                    camera::Vec co, cd;
                    lens_camera_ray(S.camera, x, y, lu, lv, &co, &cd);
                    pre.o = mk(co.x, co.y, co.z);
                    pre.d = mk(cd.x, cd.y, cd.z);
                } else if constexpr (CAM == 1) {  // the scene's pose (vr_camera.h: the ray rule)
                    const camera::Vec cd = posed_direction(x, y);
                    pre.d = mk(cd.x, cd.y, cd.z);
                } else {  // the default pose: what the rule gives for it, bit for bit (vr_camera.h)
                    pre.d = normalize(mk(x, y, 1.0));
                }
                state = kRayReady;
            }
            if (state == kRayReady) {
                VR_SEC(5);
                VR_MARK("begin_ray");
                begin_ray();
            }
            VR_STAMP(2);

            if (lanes_ieq(state, kTraversed) == 0) break;
        }
        if (lanes_ine(state, kDone) == 0) break;
        const bool tail = lanes_ieq(state, kDone) != 0;  // wave-uniform, fixed through phase B
        (void)tail;
        VR_CP(0);
        // ---------------------------------------------------------------- phase B: traverse
        // The lanes that take a node step are those with node >= 0: it implies state == kTraversing.
        // begin_ray sets node = -1 before start_bvhs gives a lane its root together with kTraversing; a
        // walk ends with node = -1 (the step's last branch) before next_bvh may leave kTraversing; phase A
        // only changes lanes that are kTraversed or beyond, whose node has been -1 since.  So the step
        // guards test node alone.  The COOP kernels keep both tests: their tail hands nodes between lanes.
        constexpr bool kTrim = kPhaseBTrim<MATS>;
        constexpr bool kNodeOnly = kTrim && !COOP;
        auto at_node_lanes = [&]() {
            return kNodeOnly ? lanes_ige(node, 0) : lanes_ieq(state, kTraversing) & lanes_ige(node, 0);
        };
        do {
            if (COUNT && first_active_lane()) cnt.trav_slots += 64;
            VR_STAMP(5);
            VR_MARK("phaseB_top");
            __builtin_amdgcn_s_setprio(kPrioNode);
            // node step (4-wide node), while the wave FIFO has room for four more leaves per lane
            bool lq[4] = {false, false, false, false};  // leaf children this lane queues in this step
            // ... carried out of the step as the hit child's link (0: no hit), so that the append's one
            // compare per child gives the vote's lane mask and the branch alike (a bool merged at the end
            // of the step's branch comes back as a 0 / 1 value that the vote turns into a mask again)
            // (the kernels that keep the longer form get no variable at all: a dead one moves their spills)
            typename std::conditional<kTrim, int32_t, const int32_t>::type lqc[4] = {0, 0, 0, 0};
            typename std::conditional<kTrim, uint64_t, const uint64_t>::type stepm = 0;  // (set per step, below)
            int32_t lent[4];
            bool coop = false;
            if constexpr (COOP) {
                if (A.coop && tail) {  // some lane of the wave is done: the queue is exhausted
                    const uint64_t live = __ballot(state != kDone);
                    const int nlive = __popcll(live);
                    // A.coop: owners served (1 or 2); to start, every live path must have bounced
                    // A.coop_bounces times.  Once on, it stays on for the wave: an owner's stack may
                    // span other lanes' columns, and the live set only shrinks (a live lane may still
                    // start a new path from the wave's slice, with its own empty stack)
                    if (!coop_on)
                        coop_on = nlive >= 1 && nlive <= (int)A.coop &&
                                  (__ballot(state != kDone && bounces >= (int)A.coop_bounces) == live);
                    coop = coop_on && nlive >= 1;
                    VR_CP(3);
                    VR_CP_TAIL(nlive);
                    if (coop) {
                        // the traversing paths' walks of their BVHs at once when nothing is pending
                        const uint64_t busy = lanes_ieq(state, kTraversing);
                        const uint64_t fresh = busy & lanes_ige(node, 0) & lanes_ieq(sp, 0) & lanes_ieq(np, 0);
                        if (A.lone_walk && busy != 0 && fresh == busy && __popcll(busy) <= 4 && q_head == q_tail) {
                            VR_CPN(3, true);
                            lone_walk(busy);
                        } else if (nlive <= 2) {
                            coop_step(live);
                        } else {
                            // 3 or 4 live paths with pending work: per-lane steps until every one of
                            // them is fresh again (each bounce's start), then their whole walks at once
                            coop = false;
                        }
                    }
                    VR_CP(1);
                }
            }
            if (COUNT) {  // how full this iteration's node step is (the headroom of merging waves)
                const int n = VR_ROOM ? __popcll(at_node_lanes()) : 0;
                if (first_active_lane()) step_hist[n == 0 ? 0 : 1 + (n - 1) / 8]++;
            }
            // VR_NODE_STEPS (2) node steps per iteration: the second, with its leaf append, before the
            // leaf-round check, the next-BVH step and the loop condition, for the lanes still at a node
            // while the FIFO has room -- half the iterations' bookkeeping (round 6: C3 38.96 -> 38.13 ms,
            // C5 2048^2 @16 17.16 -> 16.34 ms, C2 -3.6 %; 3 steps: C3 38.24, C5 16.12 ms;
            // profiles/r06/steps/).  The order of node visits and leaf tests changes, the records do not
            // (every step and leaf round is order-independent)
            for (int nst = 0; nst < VR_NODE_STEPS; ++nst) {
                // kTrim: the lanes that take this step as a lane mask -- one compare for the test whether
                // any does and for the step's branch
                if constexpr (kTrim) stepm = (!coop && VR_ROOM) ? at_node_lanes() : 0;
                if (nst > 0) {
                    if constexpr (kTrim) {
                        if (stepm == 0) break;
                    } else {
                        if (coop || (lanes_ieq(state, kTraversing) & lanes_ige(node, 0)) == 0 || !VR_ROOM) break;
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        lq[k] = false;
                        if constexpr (kTrim) lqc[k] = 0;
                    }
                    if (COUNT && first_active_lane()) cnt.trav_slots += 64;
                }
                bool takes;
                if constexpr (kTrim) takes = __builtin_amdgcn_inverse_ballot_w64(stepm);
                else takes = !coop && state == kTraversing && node >= 0 && VR_ROOM;
                if (takes) {
                    VR_MARK("node_step");
                    // 32-bit byte offsets from the scalar base (node < 2^25 unless BIG): the loads' saddr form,
                    // no 64-bit address arithmetic per step (load_quads)
                    if (COUNT) cnt.node_visits++;
                    int c[4];
                    float f[4];
                    // per-child bits: descend / queue (f32 hit or too close to call, not culled), and
                    // too close to call.  An interior child too close to call is descended: its box is
                    // a superset of its leaves' boxes, so walking it only costs work (DESIGN.md section
                    // 5); a leaf child too close to call is queued with bit 31 set and its exact f64 box
                    // test runs in the leaf round, beside the triangle test (the f32 bounds tlo / thi
                    // enclose the exact interval either way, so the f32 cull stays conservative)
                    uint32_t hm = 0, xm = 0;
                    // the six quads in the ray's order (vr_layout.h Node4, vr_device.h slab32_ordered)
                    vr_f4 q[6];
                    load_quads(node, near_off, q, c);
                    const vr_f4 tnx = slab32_quad(q[0], pre32.ix, pre32.nx), tfx = slab32_quad(q[1], pre32.ix, pre32.nx);
                    const vr_f4 tny = slab32_quad(q[2], pre32.iy, pre32.ny), tfy = slab32_quad(q[3], pre32.iy, pre32.ny);
                    const vr_f4 tnz = slab32_quad(q[4], pre32.iz, pre32.nz), tfz = slab32_quad(q[5], pre32.iz, pre32.nz);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float g;
                        bool maybe, sure;
                        slab32_ordered(tnx[k], tny[k], tnz[k], tfx[k], tfy[k], tfz[k], pre32.e2, f[k], g, maybe, sure);
                        const bool live = c[k] != kEmptyChild;
                        if (COUNT && live) cnt.box_tests++;
                        const bool pass = live && maybe && !(f[k] > cull_far || g < cull_behind);
                        hm |= pass ? 1u << k : 0u;
                        xm |= (pass && !sure) ? 1u << k : 0u;
                    }
                    // leaf children: their triangles go to the wave FIFO, appended after the step by all
                    // lanes at once
                    // interior children near-first: one 32-bit key per child, the entry distance's high
                    // bits (clamped below at 0: non-negative f32 bits order like the values) over the
                    // child's node index (A.sort_mask: the low bits, wide enough for every wide node), so
                    // the sorting network is integer min / max and the index rides along; 0xffffffff
                    // (or any key with bit 31 set) marks "not descended".  Only the visiting order depends on the key.
                    // kTrim: the 16-bit-stack kernels keep exactly 16 index bits, whatever sort_mask says
                    // (their trees have fewer than 65,536 wide nodes): a push stores the raw key, whose low
                    // half is the index.
                    constexpr bool kRawKey = S16 && kTrim;
                    const uint32_t smask = kRawKey ? 0xffffu : A.sort_mask;
                    uint32_t key[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const bool h = (hm >> k) & 1u;
                        lent[k] = (~c[k]) | (((xm >> k) & 1u) ? INT32_MIN : 0);
                        if constexpr (kTrim) lqc[k] = h ? c[k] : 0;
                        else lq[k] = h && c[k] < 0;
                        // a leaf or empty child's index is negative: its key has bit 31 set as it is
                        // (negative distances, -0 and negative NaNs clamp to 0 as integers; +inf and
                        // positive NaNs keep bit 31 clear: a hit child is never dropped)
                        uint32_t kb = ((uint32_t)max(__float_as_int(f[k]), 0) & ~smask) | (uint32_t)c[k];
                        asm volatile("" : "+v"(kb));  // computed for every lane: a select, not a branch
                        key[k] = h ? kb : 0xffffffffu;
                    }
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
                    if (key[0] < 0x80000000u) {
                        // farthest first, so the nearest remaining pops first (writes at sp are
                        // unconditional: the stack holds one spare entry)
                        // (sp advances by 1 + (key >> 31 arithmetic): 1 for a descended child, 0 else)
                        int32_t adv[4];
#pragma unroll
                        for (int k = 1; k < 4; ++k) {
                            adv[k] = (int32_t)key[k] >> 31;
                            asm volatile("" : "+v"(adv[k]));  // keeps the shift: LLVM would rebuild it as not + shift
                        }
                        st_node[sp * 256 + tid] = (StackT)(kRawKey ? key[3] : key[3] & smask);
                        sp += 1 + adv[3];
                        st_node[sp * 256 + tid] = (StackT)(kRawKey ? key[2] : key[2] & smask);
                        sp += 1 + adv[2];
                        st_node[sp * 256 + tid] = (StackT)(kRawKey ? key[1] : key[1] & smask);
                        sp += 1 + adv[1];
                        node = (int)(key[0] & smask);
                    } else if (sp > 0) {
                        --sp;
                        node = (int)st_node[sp * 256 + tid];
                    } else {
                        node = -1;  // this BVH is walked; its pending leaves remain
                    }
                }
                VR_STAMP(3);
                VR_MARK("leaf_check");
                __builtin_amdgcn_s_setprio(kPrioLeaf);
                // append this step's leaves to the wave FIFO in (child slot, lane) order (skipped when no
                // lane met a leaf: main -1.3 %, C5 -4.5 %)
                // (a leaf child's link is negative and not the empty slot's INT32_MIN: one unsigned compare,
                // whose lane mask is the vote -- lanes outside the step carry 0)
                uint64_t lqm[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    lqm[k] = kTrim ? lanes_ugt((uint32_t)lqc[k], 0x80000000u) : __ballot(lq[k]);
                    if (kTrim) lq[k] = __builtin_amdgcn_inverse_ballot_w64(lqm[k]);  // the mask itself
                }
                if ((lqm[0] | lqm[1] | lqm[2] | lqm[3]) != 0)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool lh = lq[k];
                    const uint64_t m = lqm[k];
                    if (lh) {
                        const uint32_t pos = (q_tail + (uint32_t)lanes_below(m)) & (kWaveList - 1);
                        wl_tri[wbase + pos] = lent[k];
                        wl_own[wbase + pos] = (uint8_t)lane;
                        if (kTrim) ++np;  // (under the branch's mask: one add, no 0 / 1 select)
                    }
                    q_tail += (uint32_t)__popcll(m);
                    if (!kTrim) np += lh ? 1 : 0;
                }
                q_tail = __builtin_amdgcn_readfirstlane(q_tail);
            }
            // leaf round: leaf_threshold (64) queued leaves -- every lane busy --, or enough lanes (or
            // all) are stalled on theirs
            const uint32_t queued = q_tail - q_head;
            if (queued != 0) {
                // the launch's tail (the queue is exhausted: some lane of the wave is done) with few
                // lanes still traversing (long paths alone in their wave): test their leaves at once,
                // so the hits found tighten the distance cull of the rest of the walk -- waiting for
                // a full round would walk the whole tree unculled
                const uint64_t trav = lanes_ieq(state, kTraversing);
                const bool room = VR_ROOM;  // wave-uniform
                const uint64_t at_node = kNodeOnly ? lanes_ige(node, 0) : trav & lanes_ige(node, 0);
                const uint64_t stalled_m = lanes_igt(np, 0) & (room ? ~lanes_ige(node, 0) : exec_mask());
                const bool few = coop || (tail && __popcll(trav) <= (int)A.leaf_few);
                if (queued >= A.leaf_threshold || few || __popcll(stalled_m) >= (int)A.leaf_stall ||
                    !room || at_node == 0) {
                    VR_SEC(0);
                    VR_MARK("leaf_test");
                    VR_CP(3);
                    VR_CPN(1, coop_on);
                    leaf_round(queued < 64u ? queued : 64u);
                    q_head = __builtin_amdgcn_readfirstlane(q_head + (queued < 64u ? queued : 64u));
                    VR_CP(2);
                }
            }
            VR_STAMP(4);
            if (state == kTraversing && node < 0 && np == 0) {
                VR_SEC(8);
                VR_MARK("next_bvh");
                if constexpr (ONE) {
                    state = kTraversed;  // there is no other BVH
                } else {
                    ++bvh_i;
                    if (!start_bvhs()) state = kTraversed;
                }
            }
            VR_CP(3);
        } while (lanes_ieq(state, kTraversing) != 0 &&
                 __popcll(lanes_ieq(state, kTraversed)) < (int)A.shade_threshold);
    }
    VR_CP_DUMP();
#undef VR_WALKED_OBJECT
#undef VR_CP
#undef VR_CPN
#undef VR_CP_PHASE_A
#undef VR_CP_TAIL
#undef VR_CP_DUMP

    if (COUNT) {
        atomicAdd(&A.counters[kCntBoxTests], (unsigned long long)cnt.box_tests);
        atomicAdd(&A.counters[kCntNodeVisits], (unsigned long long)cnt.node_visits);
        atomicAdd(&A.counters[kCntTriangleTests], (unsigned long long)cnt.tri_tests);
        atomicAdd(&A.counters[kCntRays], (unsigned long long)cnt.rays);
        atomicAdd(&A.counters[kCntShadedTriangles], (unsigned long long)cnt.shaded);
        atomicAdd(&A.counters[kCntSamples], (unsigned long long)samples_done);
        atomicAdd(&A.counters[kCntTraversalSlots], (unsigned long long)cnt.trav_slots);
        atomicAdd(&A.counters[kCntOuterSlots], (unsigned long long)cnt.outer_slots);
        atomicAdd(&A.counters[kCntExactBoxes], (unsigned long long)cnt.exact_boxes);
        VR_STAMP(5);
        if (first_active_lane())
            for (int i = 0; i < 6; ++i) atomicAdd(&A.counters[kCntCycles + i], (unsigned long long)cyc[i]);
        for (int i = 0; i < 3; ++i)
            if (prim_cnt[i]) atomicAdd(&A.counters[kCntPrimTests + i], (unsigned long long)prim_cnt[i]);
        for (int i = 0; i < 9; ++i) {  // each lane counted the executions it led
            if (sec[i]) atomicAdd(&A.counters[kCntSections + i], (unsigned long long)sec[i]);
            if (step_hist[i]) atomicAdd(&A.counters[kCntStepHist + i], (unsigned long long)step_hist[i]);
        }
        if (A.wg_times) {
            __syncthreads();
            if (tid == 0) A.wg_times[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
        }
    }
}

#undef VR_STAMP
#undef VR_SEC

}  // namespace dev

// ----------------------------------------------------------------------------------------------
// Host-side launch wrappers
// ----------------------------------------------------------------------------------------------
// One instantiation of render_kernel, named by field; the defaults are the template's
struct Variant {
    int stack = 0;
    bool count = false, record = false, dark0 = false;
    int mats = 3, minw = 3;
    bool whitted = false, coop = false, big = false, s16 = false;
    int cam = 0;
    bool one = false;
};

// Launches the instantiation that `make`, a captureless constexpr lambda, returns: the one place that
// spells render_kernel's template arguments in their order
template <class Make>
static void launch_variant(Make make, dim3 grid, hipStream_t s, const RenderArgs& a, const PoseArgs& pose,
                           const LensArgs& lens) {
    constexpr Variant v = make();
    hipLaunchKernelGGL((dev::render_kernel<v.stack, v.count, v.record, v.dark0, v.mats, v.minw, v.whitted, v.coop, v.big,
                                           v.s16, v.cam, v.one>),
                       grid, dim3(256), 0, s, a, a.scene.prims, a.scene.materials, a.scene.bvhs, pose, lens);
}

template <int STACK, int CAM>
static hipError_t launch_render_t(const RenderArgs& a, const PoseArgs& pose, const LensArgs& lens, const LaunchChoice& c,
                                  int grid_limit, hipStream_t s) {
    // persistent waves: enough workgroups to fill the chip, each wave loops over work items
    const uint64_t items = dev::render_items(a, ((a.tile_width + 7) / 8) * ((a.tile_height + 7) / 8) * 64);
    const uint64_t want = (items + 255) / 256;
    const dim3 grid((unsigned)(want < (uint64_t)grid_limit ? want : (uint64_t)grid_limit));
    const bool recording = c.recording, counting = c.counting;
    // VR_K(v.field = value, ...): the kernel of this stack class and camera mode with those fields set
#define VR_K(...)                             \
    launch_variant(                           \
        []() constexpr {                      \
            Variant v;                        \
            v.stack = STACK, v.cam = CAM;     \
            __VA_ARGS__;                      \
            return v;                         \
        },                                    \
        grid, s, a, pose, lens)
    // ... its recording, counting or timed kernel, as the launch asks
#define VR_MODES(...)                                          \
    if (recording) VR_K(v.record = true, __VA_ARGS__);         \
    else if (counting) VR_K(v.count = true, __VA_ARGS__);      \
    else VR_K(__VA_ARGS__)
#ifdef VR_TUNING_VARIANTS  // experiment hooks of tuning builds only (tools/variants.py)
    // 1..4 = force that many waves per SIMD (default 3); 5 / 6: 16-bit LDS stack entries (trees below
    // 65,536 wide nodes only) at 4 / 3 waves per SIMD; VR_FORCE_MATS (below): the material specialisation
    const char* ve = getenv("VR_KERNEL_VARIANT");
    const int variant = ve ? atoi(ve) : 0;
#define VR_TUNING_ARMS(...)                                                                  \
    else if (variant == 1) VR_K(v.minw = 1, __VA_ARGS__);                                    \
    else if (variant == 2) VR_K(v.minw = 2, __VA_ARGS__);                                    \
    else if (variant == 4) VR_K(v.minw = 4, __VA_ARGS__);                                    \
    else if (variant == 5 && STACK == 32) VR_K(v.minw = 4, v.s16 = true, __VA_ARGS__);       \
    else if (variant == 6 && STACK == 32) VR_K(v.s16 = true, __VA_ARGS__);
#else
#define VR_TUNING_ARMS(...)
#endif
    // ... where the timed kernel is the one with 16-bit stack entries, the single-BVH one, both or neither
#define VR_TIMED(...)                                                                             \
    if (recording) VR_K(v.record = true, __VA_ARGS__);                                            \
    else if (counting) VR_K(v.count = true, __VA_ARGS__);                                         \
    VR_TUNING_ARMS(__VA_ARGS__)                                                                   \
    else if (s16 && one) VR_K(v.stack = STACK_S16, v.s16 = true, v.one = true, __VA_ARGS__);      \
    else if (s16) VR_K(v.stack = STACK_S16, v.s16 = true, __VA_ARGS__);                           \
    else if (one) VR_K(v.stack = STACK_ONE, v.one = true, __VA_ARGS__);                           \
    else VR_K(__VA_ARGS__)
    const bool whitted = a.scene.integrator == 1;  // WhittedIntegrator: the general-material kernel
    if (c.big) {
        // 64-bit load offsets (scenes past 4 GB of triangles or 2^25 wide nodes): the general
        // kernels only (DARK0 = false and every material kind are always correct, only slower), in
        // the deepest stack class only (launch_render)
        if constexpr (STACK != 48) {
            return hipErrorInvalidValue;
        } else if (whitted) {
            VR_MODES(v.whitted = true, v.big = true);
        } else {
            VR_MODES(v.big = true);
        }
        return hipSuccess;
    }
    if (whitted) {
        VR_MODES(v.dark0 = true, v.whitted = true);
        return hipSuccess;
    }
    // kinds present (bit 0 Lambertian, 1 reflective, 2 Phong or dielectric) -> specialisation:
    // Lambertian-only (1), reflective-only (2) or the general kernel (3)
    int mats = (c.mats == 1 || c.mats == 2) ? c.mats : 3;
    if (!c.dark0) mats = 3;  // the general kernel
#ifdef VR_TUNING_VARIANTS
    if (const char* fm = getenv("VR_FORCE_MATS")) mats = atoi(fm);
#endif
    // the cooperative-tail instantiations: launches the host marks (RenderArgs::coop: small launches
    // of scenes with a reflective material)
#ifndef VR_COOP_MINW  // their waves per SIMD (2: no spills; C1 -9 %)
#define VR_COOP_MINW 2
#endif
    const bool coop = c.coop;
    // 16-bit LDS stack entries (LaunchChoice::s16: trees below 65,536 wide nodes) for the timed
    // kernels of the 24 / 32 stack classes: half the stack's LDS at the same 3 waves per SIMD, C3
    // 39.22 -> 38.71 ms, 1024^2 @64 10.83 -> 10.58 ms, records bit-identical (profiles/r06/occ)
    constexpr int STACK_S16 = STACK <= 32 ? STACK : 32;  // (never launched for the 48 class)
    const bool s16 = c.s16 && STACK <= 32;
    // the single-BVH instantiations (LaunchChoice::one_bvh, round 8) of the timed kernels: with 16-bit
    // stack entries in the 24 and 32 classes, with 32-bit ones in the 32 class only (the host's choice
    // knows: vr_host.cpp takes_one_bvh; the other classes would add a third to this file's build time
    // for kernels no scene here runs)
    constexpr int STACK_ONE = 32;  // (never launched for another class)
    const bool one = c.one_bvh && (s16 || STACK == 32);
    if (!c.dark0) {
        VR_TIMED(v.dark0 = false);
    } else if (mats == 1) {
        VR_TIMED(v.dark0 = true, v.mats = 1);
    } else if (mats == 2) {
        if (coop) VR_K(v.dark0 = true, v.mats = 2, v.minw = VR_COOP_MINW, v.coop = true);
        else VR_TIMED(v.dark0 = true, v.mats = 2);
    } else {
        if (coop) VR_K(v.dark0 = true, v.mats = 3, v.minw = VR_COOP_MINW, v.coop = true);
        else VR_TIMED(v.dark0 = true, v.mats = 3);
    }
#undef VR_TIMED
#undef VR_TUNING_ARMS
#undef VR_MODES
#undef VR_K
    return hipSuccess;
}

// The launcher of one camera mode's kernels: the stack class of the launch.  Only enqueues the render
// kernel; launch_render (vr_render_launch.hip) follows it with the ordered reduce.
template <int CAM>
hipError_t launch_render_class(int depth, const RenderArgs& a, const PoseArgs& pose, const LensArgs& lens,
                               const LaunchChoice& c, int grid_limit, hipStream_t s) {
    if (depth <= 24) return launch_render_t<24, CAM>(a, pose, lens, c, grid_limit, s);
    if (depth <= 32) return launch_render_t<32, CAM>(a, pose, lens, c, grid_limit, s);
    return launch_render_t<48, CAM>(a, pose, lens, c, grid_limit, s);
}

}  // namespace vr
