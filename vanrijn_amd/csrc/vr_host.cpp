// vr_host.cpp -- the core of the host side (the rest: vr_host_*.cpp): the call-context pool, launch arguments, the pass loop, the
// scaffold of the host-buffer calls, the render entry points, launch times and stream errors.
//   partial_render_scene                          src/camera.rs:95-130
//   AccumulationBuffer::{new, update_pixel}       src/accumulation_buffer.rs:14-60
#include "vr_host.h"

#include <chrono>

using namespace vrh;

// launch defaults (A/B builds may override them at compile time)
#ifndef VR_COOP_SAMPLES  // launches of at most this many pixel-samples may take the cooperative tail
#define VR_COOP_SAMPLES (4ull << 20)
#endif
#ifndef VR_COOP_BOUNCES  // ... once every live path of a wave has bounced this often
#define VR_COOP_BOUNCES 0u
#endif
namespace {

// The render kernel addresses the triangle and 4-wide node arrays with 32-bit byte offsets from
// their scalar bases (tri * 80, node << 7); a scene past either limit -- 53.7 M triangles (4 GB of
// TriVerts), 2^25 wide nodes -- runs the kernels with 64-bit offsets (render_kernel<.., BIG>)
static bool needs_big_offsets(uint64_t tri_count, uint64_t wide_count) {
    return tri_count * sizeof(vr::TriVerts) >= (1ull << 32) || wide_count >= (1ull << 25);
}

// The timed render kernels have an instantiation for scenes whose BVH list is one BVH with a wide
// root (render_kernel<.., ONE>: no list walk, no per-lane BVH cursor; round 8).  `root4`: that BVH's
// root (negative: a one-triangle mesh, or INT32_MIN for an empty one).  `other`: VR_CHOICE_* bits of
// what else the launch selected -- the counting, record, Whitted and 64-bit-offset kernels have no such
// instantiation, VR_LAUNCH_MULTI_BVH asks for the generic kernel, a scene of one material kind whose
// rows lie on different wavelength grids runs it too (VR_CHOICE_OWN_GRIDS), and a launch small enough for the
// cooperative tail keeps the kernels it had, with the tail or (VR_LAUNCH_NO_COOP) without it, so that
// flag's A/B still isolates the tail.  It exists with 16-bit stack entries in the 24 and 32 stack classes
// and with 32-bit ones in the 32 class (vr_render_kernel.h launch_render_t).
static bool takes_one_bvh(uint64_t bvh_count, int32_t root4, uint32_t other, int stack_depth, bool s16) {
    if (bvh_count != 1 || root4 < 0 || other != 0) return false;
    return s16 ? stack_depth <= 32 : (stack_depth > 24 && stack_depth <= 32);
}

// the launches that may take the cooperative tail: at most VR_COOP_SAMPLES pixel-samples of a DARK0
// scene with a reflective material (make_args)
static bool coop_gated(const vr_scene* s, uint64_t pixel_samples) {
    return pixel_samples <= VR_COOP_SAMPLES && (s->mats & 2) && s->dark0;
}

// Which render_kernel instantiation a launch of `s` runs.  coop: RenderArgs::coop != 0 (the launch is
// coop_gated and nothing turned the tail off).  Everything is read from the scene now, so an edit that
// changed its meshes, materials or tree is reflected at the next launch.
static vr::LaunchChoice launch_choice(const vr_scene* s, bool coop, bool gated, bool counting, bool recording,
                                      uint32_t launch_flags) {
    vr::LaunchChoice lc;
    // LDS stack entries: the 4-wide walk's, and the binary walk's for Whitted shadow rays
    const int stack = s->dev.integrator == 1 ? std::max(stack_depth(s), wide_stack_depth(s)) : wide_stack_depth(s);
    lc.stack_depth = stack;
    lc.counting = counting;
    lc.recording = recording;
    lc.dark0 = s->dark0;
    lc.mats = s->mats ? s->mats : 3;
    lc.big = s->force_big || needs_big_offsets(s->tri_count, s->wide_count);
    // the cooperative tail's instantiations exist for DARK0 scenes with a reflective material
    lc.coop = coop && !recording && !counting && !lc.big && s->dev.integrator != 1 && s->dark0 && (lc.mats & 2);
    // 16-bit LDS stack entries: every node index of the tree fits (round 6, vr_render_kernel.h
    // launch_render_t; VR_LAUNCH_STACK32 keeps 32-bit entries, the same records bit for bit)
    lc.s16 = !recording && !counting && !lc.big && !lc.coop && s->dev.integrator != 1 && s->wide_count < 65536 &&
             stack <= 32 && !(launch_flags & VR_LAUNCH_STACK32);
    const uint32_t other = (counting ? VR_CHOICE_COUNTING : 0u) | (recording ? VR_CHOICE_RECORD : 0u) |
                           (s->dev.integrator == 1 ? VR_CHOICE_WHITTED : 0u) | (gated || lc.coop ? VR_CHOICE_COOP_GATED : 0u) |
                           (lc.big ? VR_CHOICE_WIDE_OFFSETS : 0u) |
                           ((launch_flags & VR_LAUNCH_MULTI_BVH) ? VR_CHOICE_MULTI_BVH : 0u) |
                           // the single-BVH kernels of one material kind look a path's wavelength up once,
                           // on the one grid every row shares (vr_render_kernel.h PATHWL)
                           (lc.dark0 && (lc.mats == 1 || lc.mats == 2) && !s->grid_shared ? VR_CHOICE_OWN_GRIDS : 0u);
    lc.one_bvh = takes_one_bvh(s->bvhs.size(), s->bvhs.empty() ? INT32_MIN : s->bvhs[0].root4, other, stack, lc.s16);
    return lc;
}

static uint32_t variant_bits(const vr::LaunchChoice& lc) {
    return (lc.coop ? VR_VARIANT_COOP : 0u) | (lc.big ? VR_VARIANT_WIDE_OFFSETS : 0u) |
           (lc.s16 ? VR_VARIANT_STACK16 : 0u) | (lc.one_bvh ? VR_VARIANT_ONE_BVH : 0u);
}

// persistent grid: workgroups per CU of the render kernel (3: 3 waves per SIMD); VR_GRID_PER_CU
// overrides (tuning builds; diagnostic: throughput against occupancy)
int grid_per_cu() {
    const char* g = tuning_env("VR_GRID_PER_CU");
    return g ? std::max(1, atoi(g)) : 3;
}
// ... of the cooperative-tail instantiations.  They run at VR_COOP_MINW = 2 waves per SIMD, so only 2
// workgroups per CU are resident; the third starts as another retires.  Kept on purpose:
// C1 1.558 ms at 3 per CU against 1.572-1.604 at 2 (9 interleaved repetitions each,
// profiles/r06/probe/coopgrid.out) -- a late-starting workgroup takes items the resident ones would
// otherwise have taken in their tails
int coop_grid_per_cu() {
    const char* g = tuning_env("VR_COOP_GRID");
    return g ? std::max(1, atoi(g)) : 3;
}

// Take a context from the scene's pool (a new one when all are in use).  The caller must hand it
// back with ctx_release; work it enqueued may still run (its `done` event orders the next user).
// `want`: the stream the caller will enqueue on (vr_render_tile_device), or none (the host-buffer
// entry points, which use the context's own stream).
int ctx_acquire(vr_scene* s, CallCtx** out, const hipStream_t* want = nullptr) {
    {
        // In order of preference:
        //  1. a free context whose last call's work has finished on the device (its `done` has
        //     completed);
        //  2. a free context whose last call was enqueued on the caller's own stream: stream order
        //     already puts the new call after that work, so the hipStreamWaitEvent on `done` costs
        //     nothing (bench.py's frames queue back to back on one stream and reuse ONE context --
        //     a second one would allocate a second frame-sized staging buffer, 68.7 GB at C4 / C5,
        //     inside the timed region, and its smaller cap could split alternate frames into passes);
        //  3. with none of those and fewer than two contexts, a new one (frame k + 1 on another
        //     stream then renders while frame k's launch drains); beyond two the most recent one is
        //     reused (its `done` orders the new call after it).
        std::lock_guard<std::mutex> g(s->ctx_mutex);
        for (size_t i = s->ctx_free.size(); i-- > 0;) {
            if (hipEventQuery(s->ctx_free[i]->done) == hipSuccess) {
                *out = s->ctx_free[i];
                s->ctx_free.erase(s->ctx_free.begin() + (ptrdiff_t)i);
                return VR_OK;
            }
        }
        if (want) {
            for (size_t i = s->ctx_free.size(); i-- > 0;) {
                if (s->ctx_free[i]->used && s->ctx_free[i]->last_stream == *want) {
                    *out = s->ctx_free[i];
                    s->ctx_free.erase(s->ctx_free.begin() + (ptrdiff_t)i);
                    return VR_OK;
                }
            }
        }
        if (!s->ctx_free.empty() && s->ctx_all.size() >= 2) {
            *out = s->ctx_free.back();
            s->ctx_free.pop_back();
            return VR_OK;
        }
    }
    CallCtx* c = new (std::nothrow) CallCtx();
    if (!c) return fail(VR_ERROR_OUT_OF_MEMORY, "call context allocation failed");
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    // blocking sync: a host-buffer call waits on `done` asleep, not spinning a core (8 spinning
    // callers under a 16-CPU quota throttled the whole process for ~10 ms at a time)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->done, hipEventDisableTiming | hipEventBlockingSync);
#ifdef VR_COOP_PROF  // analysis builds: per-wave records after word 24 (vr_render_kernel.h)
    if (e == hipSuccess) e = hipMalloc(&c->queue, 65536);
    if (e == hipSuccess) e = hipMemsetAsync(c->queue, 0, 65536, c->stream);
#else
    if (e == hipSuccess) e = hipMalloc(&c->queue, 256);
    if (e == hipSuccess) e = hipMemsetAsync(c->queue, 0, 256, c->stream);
#endif
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        ctx_free_all(c);
        return fail(VR_ERROR_DEVICE, std::string("call context: ") + hipGetErrorString(e));
    }
    c->error = (int32_t*)(c->queue + 1);
    std::lock_guard<std::mutex> g(s->ctx_mutex);
    s->ctx_all.push_back(c);
    *out = c;
    return VR_OK;
}

void ctx_release(vr_scene* s, CallCtx* c) {
    std::lock_guard<std::mutex> g(s->ctx_mutex);
    s->ctx_free.push_back(c);
}

// Records the context's `done` on the call's stream when it goes out of scope, so that EVERY exit of
// a call after its first enqueue -- an error return included -- orders the context's next user
// (possibly on another stream) after the work this call left queued on its staging, mask, queue
// counter and scratch.  (The success paths record `done` themselves as well: recording it again
// at the same point of the stream changes nothing.)  enqueue_passes' own guard: it also serves
// vr_render_tile_device, on the caller's stream, where there is no HostCall.
struct DoneOnExit {
    hipEvent_t done;
    hipStream_t st;
    ~DoneOnExit() { (void)hipEventRecord(done, st); }
};

}  // namespace

namespace vrh {

int check_render_params(const vr_scene* s, const vr_render_params* p) {
    if (!s || !p) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or params");
    if (s->host_only) return host_only_error();
    const vr_tile& t = p->tile;
    // Tile and Array2D index asserts in the reference (array2d.rs:58,65) panic; here: an error
    if (t.end_column < t.start_column || t.end_row < t.start_row || t.end_column > p->width ||
        t.end_row > p->height || p->width == 0 || p->height == 0)
        return fail(VR_ERROR_INVALID_ARGUMENT, "tile outside the image");
    // the random stream's base mix64(key ^ (pixel << 32 | sample)) is injective
    // only for pixel and sample indices below 2^32: a larger index would silently carry into the
    // other field and repeat another (pixel, sample)'s stream
    if (p->width > (1ull << 32) || p->height > (1ull << 32) || p->width * p->height > (1ull << 32))
        return fail(VR_ERROR_UNSUPPORTED, "image of more than 2^32 pixels (random stream index space)");
    if ((uint64_t)p->first_sample + p->spp > (1ull << 32) || (uint64_t)p->first_sample >= (1ull << 32))
        return fail(VR_ERROR_UNSUPPORTED, "sample indices past 2^32 (random stream index space)");
    if (stack_depth(s) > 48 || wide_stack_depth(s) > 48)
        return fail(VR_ERROR_UNSUPPORTED, "BVH deeper than the largest traversal stack (48)");
    return VR_OK;
}

uint64_t seed_key_of(uint64_t seed) {  // vr-hash32 v2: the launch-constant key of stream_base_keyed
    uint64_t z = seed ^ 0x76616E52696A6E31ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

vr::RenderArgs make_args(const vr_scene* s, const vr_render_params* p, double* state) {
    vr::RenderArgs a{};
    a.scene = s->dev;
    a.start_column = p->tile.start_column;
    a.start_row = p->tile.start_row;
    a.tile_width = p->tile.end_column - p->tile.start_column;
    a.tile_height = p->tile.end_row - p->tile.start_row;
    a.width = p->width;
    a.height = p->height;
    a.seed = p->seed;
    a.seed_key = seed_key_of(p->seed);
    a.first_sample = p->first_sample;
    a.spp = p->spp;
    a.accumulate = p->accumulate;
    a.state = state;  // (queue, staging, error word, cull mask, records, counters: per call, enqueue_passes)
    a.fault_object = s->fault_object;
    a.sky_on_grid = s->sky_on_grid ? 1u : 0u;
    const char* th = tuning_env("VR_SHADE_THRESHOLD");  // tuning hook (tools/variants.py)
    a.shade_threshold = th ? (uint32_t)atoi(th) : 52u;
    const char* sm = tuning_env("VR_SHADE_MIN");  // tuning hook: defer shading below this many hits
    a.shade_min = sm ? (uint32_t)std::max(0, atoi(sm)) : 16u;
    a.early_stop = s->nan_free ? 1u : 0u;
    if (const char* es = tuning_env("VR_EARLY_STOP")) a.early_stop = atoi(es) != 0 && s->nan_free;  // A/B hook (off only)
    const char* mm = tuning_env("VR_MISS_MIN");  // tuning hook: defer finishing misses
    a.miss_min = mm ? (uint32_t)std::max(0, atoi(mm)) : 8u;
    const char* ch = tuning_env("VR_CHUNK");  // tuning hook: samples per work item
    a.chunk = ch ? (uint32_t)std::max(1, atoi(ch)) : 1u;
    const char* ts = tuning_env("VR_TAIL_SAMPLES");  // tuning hook: single-sample items at the end
    a.tail_samples = ts ? (uint32_t)std::max(0, atoi(ts)) : 0u;
    const char* gr = tuning_env("VR_GRAB");  // tuning hook: items per queue atomic
    if (gr) {
        a.grab = (uint32_t)std::max(0, atoi(gr));
    } else {
        // 512 items per atomic keeps the queue counter cold on full frames; a smaller launch would
        // hand 512 items to a few waves and leave the rest of the chip idle at its end (1 spp of
        // 1024^2: 1.9 ms at 512), so every wave gets about 80 slices, in multiples of 64 (one item
        // per lane), and at least 128: one atomic per 64 items costs more than the tail it saves.
        // Measured (1024^2): 256 spp best at 512 (64: +38 %, 256: +0.3 %), 64 spp at 256 (512:
        // +1.5 %), C5's mesh at 32 spp at 128; 512^2 @64 (C2) 128..384 within 2 % (64: +17 %);
        // 256^2 @16 (C1) flat (profiles/r02/sweeps/sw_grab_*.txt)
        const uint64_t items = ((a.tile_width + 7) / 8) * ((a.tile_height + 7) / 8) * 64 * std::max(1u, p->spp);
        const uint64_t waves = (uint64_t)std::max(1, s->cu_count) * 3 * 4;
        const uint64_t g = items / (waves * 80) / 64 * 64;
        a.grab = (uint32_t)std::min<uint64_t>(512, std::max<uint64_t>(128, g));
    }
    const char* lt = tuning_env("VR_LEAF_THRESHOLD");  // tuning hooks
    a.leaf_threshold = lt ? (uint32_t)std::max(1, atoi(lt)) : 48u;
    const char* ls = tuning_env("VR_LEAF_STALL");
    a.leaf_stall = ls ? (uint32_t)std::max(1, atoi(ls)) : 3u;
    const char* lf = tuning_env("VR_LEAF_FEW");  // tuning hook (0: off)
    a.leaf_few = lf ? (uint32_t)std::max(0, atoi(lf)) : 0u;
    // the cooperative tail (vr_render_kernel.h coop_step, the COOP instantiations): launches of at most
    // 4 M pixel-samples (a small frame's time is its longest paths') of scenes with a reflective
    // material (paths trapped between mirror facets run to the 128-bounce limit: C1,
    // benches/simple_scene.rs).  Scenes without mirrors never take it: on main.rs's Lambertian scene
    // the breadth-first walk of short tail paths cost more than it saved.
    {
        const uint64_t lsamples = a.tile_width * a.tile_height * (uint64_t)p->spp;
        // (a.coop: the most live paths a wave's tail may have to start it: coop_step serves one or
        // two, lone_walk's whole walks up to four)
        a.coop = coop_gated(s, lsamples) ? 4u : 0u;
        if (const char* co = tuning_env("VR_COOP")) a.coop = (uint32_t)std::min(4, std::max(0, atoi(co)));
        a.coop_bounces = VR_COOP_BOUNCES;  // ... once every live path of the wave has bounced this often
        a.lone_walk = 1;
        if (const char* cb = tuning_env("VR_COOP_BOUNCES")) a.coop_bounces = (uint32_t)std::max(0, atoi(cb));
    }
    {
        // the node step's child keys keep the entry distance's high bits above the node index:
        // the fewest low bits whose all-ones value exceeds every wide node index
        uint32_t m = 1;
        while (m < s->wide_count + 1 && m != 0xffffffffu) m = m << 1 | 1;
        a.sort_mask = m;
    }
    // block-major work items over the live blocks in Z-order (round 5): the waves in flight share a
    // compact patch of the image, so their camera rays and first hits walk the same part of the
    // tree -- C3 -4.5 %, C2 -4.5 %, C5 -4.2 %; scenes with a reflective material keep sample-major
    // order (the bench scene +1..4 % block-major: its trapped mirror paths cluster in the same waves)
    // (profiles/r05/order)
    const bool block_major = (s->mats & 2) == 0;
    const char* io = tuning_env("VR_ITEM_ORDER");  // tuning hook: 0 sample-major, 1 block-major
    a.item_order = io ? (uint32_t)(atoi(io) != 0) : (block_major ? 1u : 0u);
    const char* pr = tuning_env("VR_PHASE_A_REPS");  // tuning hook
    a.phase_a_reps = pr ? (uint32_t)std::max(1, atoi(pr)) : 2u;
    // same f64 operations as the reference's ImageSampler::new / film_to_world
    vr::camera::film_constants(a.width, a.height, a.film);
    {
        // by value: an axis entry of -0.0 is a default entry too (its products are +-0 as well)
        const vr::PoseArgs& d = s->pose;
        const double pose[10] = {d.right[0], d.right[1], d.right[2], d.up[0], d.up[1],
                                 d.up[2], d.forward[0], d.forward[1], d.forward[2], d.film_distance};
        const double standard[10] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0};
        a.posed = std::equal(pose, pose + 10, standard) ? 0u : 1u;
        if (s->lens.lens_radius != 0.0) a.posed = 2u;  // a lens: the instantiations that apply pose and lens
    }
    {
        const uint64_t bw = (a.tile_width + 7) / 8, bh = (a.tile_height + 7) / 8;
        a.rcp_blocks = bw * bh ? 1.0 / (double)(bw * bh) : 0.0;
        a.rcp_bw = bw ? 1.0 / (double)bw : 0.0;
    }
    return a;
}

int error_status(int32_t bits) {
    if (bits & 8)  // debug builds (VR_STAGE_GUARD)
        return fail(VR_ERROR_DEVICE, "staging guard: the ordered reduce read a staged photon its pass did not write");
    return fail(VR_ERROR_SINGULAR_BASIS,
                "Normal, tangent and cotangent don't form a valid basis (det == 0); the reference panics here");
}

// Waits for `stream`, then reads and clears one error word (a call's own, or a stream's sticky one).
int read_and_clear_error(int32_t* slot, hipStream_t stream) {
    int32_t flag = 0;
    VR_HIP(hipMemcpyAsync(&flag, slot, sizeof flag, hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    if (flag) {
        VR_HIP(hipMemsetAsync(slot, 0, sizeof flag, stream));
        VR_HIP(hipStreamSynchronize(stream));
        return error_status(flag);
    }
    return VR_OK;
}

// Grow a context buffer to `need` bytes; its previous contents may still be in use by the
// context's last call (on whatever stream), so wait for `done` before freeing it.
int ctx_grow(void** ptr, size_t* have, size_t need, hipEvent_t done) {
    if (need <= *have) return VR_OK;
    VR_HIP(hipEventSynchronize(done));
    if (*ptr) VR_HIP(hipFree(*ptr));
    *ptr = nullptr;
    *have = 0;
    VR_HIP(hipMalloc(ptr, need));
    *have = need;
    return VR_OK;
}

// Grow the context's page-locked host buffer (its previous contents are only read by the host
// within the call that filled it, so no device wait is needed beyond the context's `done`).
int ctx_grow_pinned(CallCtx* c, size_t need) {
    if (need <= c->pinned_bytes) return VR_OK;
    VR_HIP(hipEventSynchronize(c->done));
    if (c->pinned) VR_HIP(hipHostFree(c->pinned));
    c->pinned = nullptr;
    c->pinned_bytes = 0;
    VR_HIP(hipHostMalloc(&c->pinned, need, hipHostMallocDefault));
    c->pinned_bytes = need;
    return VR_OK;
}

void ctx_free_all(CallCtx* c) {
    if (c->done) {
        (void)hipEventSynchronize(c->done);
        (void)hipEventDestroy(c->done);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->staging) (void)hipFree(c->staging);
    if (c->mask) (void)hipFree(c->mask);
    if (c->scratch) (void)hipFree(c->scratch);
    if (c->pinned) (void)hipHostFree(c->pinned);
    if (c->queue) (void)hipFree(c->queue);
    if (c->tags) (void)hipFree(c->tags);
    delete c;
}

// The sticky error word of `stream` (created zeroed on first use, on that stream).
int stream_slot(vr_scene* s, void* stream, int32_t** out) {
    std::lock_guard<std::mutex> g(s->slot_mutex);
    auto it = s->stream_slots.find(stream);
    if (it != s->stream_slots.end()) {
        *out = it->second;
        return VR_OK;
    }
    int32_t* p = nullptr;
    VR_HIP(hipMalloc(&p, 256));
    const hipError_t e = hipMemsetAsync(p, 0, 256, (hipStream_t)stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(VR_ERROR_DEVICE, std::string("error slot: ") + hipGetErrorString(e));
    }
    s->stream_slots.emplace(stream, p);
    *out = p;
    return VR_OK;
}

// Enqueue the render of params `p` into `state` on stream `st`, in passes that fit the context's
// staging buffer (16 B per pixel-sample: the final photon).  `err` is the device word the kernel
// flags a singular shading basis in.  Per-pass events of a timed launch: render kernel
// [start, mid), ordered reduce [mid, end).
struct PassEvents {
    std::vector<hipEvent_t> ev;
    ~PassEvents() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    hipEvent_t add() {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        ev.push_back(e);
        return e;
    }
};

int enqueue_passes(vr_scene* s, CallCtx* c, const vr_render_params* p, double* state, hipStream_t st, int32_t* err,
                   bool counting, bool recording, void* records, unsigned long long* counters,
                   unsigned long long* wg_times, PassEvents* timing, uint32_t launch_flags, uint32_t* variant) {
    launch_flags |= s->debug_launch_flags;
    const bool no_cull = (launch_flags & VR_LAUNCH_NO_CULL) != 0;
    const uint64_t tw = p->tile.end_column - p->tile.start_column, th = p->tile.end_row - p->tile.start_row;
    const uint64_t npix = tw * th;
    if (npix == 0 || p->spp == 0) return VR_OK;
    size_t free_b = 0, total_b = 0;
    VR_HIP(hipMemGetInfo(&free_b, &total_b));
    // staging for a whole frame when half the free HBM holds it (a 288 GB MI355X: C4 / C5's
    // 68.7 GB on one GPU in one launch -- every extra launch adds the tail of the frame's longest
    // paths, ~7 ms on the C5 mesh); vr_scene_set_staging_limit lowers the cap (a GPU shared with
    // other work; the tests of the pass split)
    size_t cap = (free_b + c->staging_bytes) / 2;
    if (s->staging_limit) cap = std::min<size_t>(cap, s->staging_limit);
    uint64_t pass = recording ? p->spp : std::min<uint64_t>(p->spp, std::max<uint64_t>(1, cap / (16 * npix)));
    // the kernel decodes work items with 32-bit block indices: (8x8 blocks) x samples < 2^32
    if (((tw + 7) / 8) * ((th + 7) / 8) * pass >= (1ull << 32))
        return fail(VR_ERROR_UNSUPPORTED, "too many pixel blocks x samples in one launch (2^32)");
    // the context's previous user (possibly on another stream) must be done with its buffers
    VR_HIP(hipStreamWaitEvent(st, c->done, 0));
    DoneOnExit guard{c->done, st};
    c->last_stream = st;
    c->used = true;
    int rc = ctx_grow(&c->staging, &c->staging_bytes, (size_t)(16 * npix * pass), c->done);
    if (rc) return rc;
#ifdef VR_STAGE_GUARD
    if (c->tag_bytes < (size_t)(4 * npix * pass)) {
        rc = ctx_grow(&c->tags, &c->tag_bytes, (size_t)(4 * npix * pass), c->done);
        if (rc) return rc;
        VR_HIP(hipMemsetAsync(c->tags, 0, c->tag_bytes, st));  // generation 0: never written
    }
#endif
    // blocks whose camera rays all miss every object (one small kernel per call; VR_LAUNCH_NO_CULL
    // turns the test off: the records are the same bit for bit, tests/test_gpu_cull.py)
    const bool cull = !no_cull;
    const uint8_t* mask = nullptr;
    const uint32_t *live = nullptr, *live_count = nullptr;
    if (cull && !recording) {  // (the record variant writes every sample's record)
        // mask: 1 B per block; then the live-block list (4 B per block) and its count (16-B aligned)
        const uint64_t nb = ((tw + 7) / 8) * ((th + 7) / 8);
        const size_t list_off = (nb + 15) & ~(uint64_t)15;
        rc = ctx_grow(&c->mask, &c->mask_bytes, (size_t)(list_off + 4 * nb + 16), c->done);
        if (rc) return rc;
        if (nb >= (1ull << 32)) return fail(VR_ERROR_UNSUPPORTED, "too many pixel blocks in one tile (2^32)");
        vr::RenderArgs a = make_args(s, p, state);
        int lc = vr::launch_block_cull(a, s->pose, s->lens, (uint8_t*)c->mask, st);
        uint32_t* lst = (uint32_t*)((char*)c->mask + list_off);
        const char* bm = tuning_env("VR_BLOCK_MORTON");  // tuning hook: live blocks in Z-order
        const bool morton = bm ? atoi(bm) != 0 : (s->mats & 2) == 0;  // with block-major items (make_args)
        if (!lc)
            lc = vr::launch_block_compact((const uint8_t*)c->mask, (uint32_t)((tw + 7) / 8), (uint32_t)((th + 7) / 8),
                                          morton, lst, lst + nb, st);
        if (lc) return fail(VR_ERROR_DEVICE, vr::device_error_string(lc));
        mask = (const uint8_t*)c->mask;
        live = lst;
        live_count = lst + nb;
    }
    for (uint64_t done = 0; done < p->spp; done += pass) {
        vr_render_params q = *p;
        q.spp = (uint32_t)std::min<uint64_t>(pass, p->spp - done);
        q.first_sample = p->first_sample + done;
        q.accumulate = (done > 0 || p->accumulate) ? 1u : 0u;
        vr::RenderArgs a = make_args(s, &q, state);
        a.staging = (double*)c->staging;
        if (launch_flags & VR_LAUNCH_NO_DIST_CULL) {
            // every box the line crosses is walked (culled() / cull_far / cull_behind never prune):
            // the records stay the same bit for bit (tests/test_gpu_launch_variants.py)
            a.scene.margin = INFINITY;
            a.scene.behind_margin = INFINITY;
        }
        if (launch_flags & VR_LAUNCH_NO_COOP) a.coop = 0;
        if (launch_flags & VR_LAUNCH_NO_LONE_WALK) a.lone_walk = 0;
#ifdef VR_STAGE_GUARD
        a.stage_tag = (uint32_t*)c->tags;
        if (++c->gen == 0) c->gen = 1;
        a.stage_gen = c->gen;
#endif
        a.queue = c->queue;
        a.error_flag = err;
        a.block_mask = mask;
        a.live_blocks = live;
        a.live_count = live_count;
        a.records = records;
        a.counters = counters;
        a.wg_times = done == 0 ? wg_times : nullptr;
#ifdef VR_COOP_PROF  // analysis builds: the previous launch's tail-wave sums (vr_render_kernel.h)
        {
            static unsigned long long h[16 + 6000];
            VR_HIP(hipStreamSynchronize(st));
            VR_HIP(hipMemcpy(h, c->queue + 8, sizeof h, hipMemcpyDeviceToHost));
            if (h[7])
                fprintf(stderr, "vrcoop A %llu coop %llu leaf %llu rest %llu iters %llu leafrounds %llu phaseA %llu waves %llu maxwall %llu sumwall %llu lone %llu\n",
                        h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10]);
            for (unsigned long long i = 0; i < h[11] && i < 1000; ++i)
                fprintf(stderr, "vrwave %llu %llu %llu %llu %llu %llu\n", h[16 + 6 * i], h[17 + 6 * i], h[18 + 6 * i],
                        h[19 + 6 * i], h[20 + 6 * i], h[21 + 6 * i]);
            VR_HIP(hipMemset(c->queue + 8, 0, sizeof h));
        }
#endif
        VR_HIP(hipMemsetAsync(c->queue, 0, sizeof(unsigned long long), st));
        hipEvent_t mid = nullptr;
        if (timing) {
            hipEvent_t start = timing->add();
            mid = timing->add();
            if (!start || !mid) return fail(VR_ERROR_DEVICE, "hipEventCreate failed");
            VR_HIP(hipEventRecord(start, st));
        }
        const vr::LaunchChoice lc = launch_choice(s, a.coop != 0, coop_gated(s, a.tile_width * a.tile_height * (uint64_t)q.spp),
                                                  counting, recording, launch_flags);
        if (variant) *variant = variant_bits(lc);
        // the COOP instantiations (2 waves per SIMD) keep 3 workgroups per CU (coop_grid_per_cu)
        const int per_cu = lc.coop ? coop_grid_per_cu() : grid_per_cu();
        int lr = vr::launch_render(a, s->pose, s->lens, lc, std::max(1, s->cu_count) * per_cu, st, mid);
        if (lr) return launch_status(lr);
        if (timing) {
            hipEvent_t end = timing->add();
            if (!end) return fail(VR_ERROR_DEVICE, "hipEventCreate failed");
            VR_HIP(hipEventRecord(end, st));
        }
    }
    VR_HIP(hipEventRecord(c->done, st));
    return VR_OK;
}

int HostCall::begin(const vr_scene* s) {
    VR_HIP(hipSetDevice(s->device));
    scene_ = const_cast<vr_scene*>(s);
    const int rc = ctx_acquire(scene_, &c);
    if (rc) return rc;
    st = c->stream;
    VR_HIP(hipStreamWaitEvent(st, c->done, 0));
    begun_ = true;
    return VR_OK;
}

HostCall::~HostCall() {
    if (begun_) (void)hipEventRecord(c->done, st);
    if (c) ctx_release(scene_, c);
}

}  // namespace vrh

// [start, mid, end] per pass: render kernel [start, mid), ordered reduce [mid, end), summed in the caller's T
template <class T>
static int sum_pass_times(const std::vector<hipEvent_t>& ev, T* kernel_ms, T* reduce_ms) {
    if (!ev.empty()) VR_HIP(hipEventSynchronize(ev.back()));
    for (size_t i = 0; i + 3 <= ev.size(); i += 3) {
        float x = 0.f, y = 0.f;
        VR_HIP(hipEventElapsedTime(&x, ev[i], ev[i + 1]));
        VR_HIP(hipEventElapsedTime(&y, ev[i + 1], ev[i + 2]));
        *kernel_ms += x;
        *reduce_ms += y;
    }
    return VR_OK;
}

int vr_scene_needs_wide_offsets(uint64_t triangle_count, uint64_t wide_node_count) {
    return needs_big_offsets(triangle_count, wide_node_count) ? 1 : 0;
}

int vr_material_grids_shared(const void* rows, uint32_t count) {
    return rows && grids_shared((const vr::Material*)rows, count) ? 1 : 0;
}

int vr_scene_grid_shared(const vr_scene* s) { return s ? (s->grid_shared ? 1 : 0) | (s->sky_on_grid ? 2 : 0) : 0; }

int vr_launch_takes_one_bvh(uint64_t bvh_count, int32_t root4, uint32_t other, int32_t stack_depth, int32_t stack16) {
    return takes_one_bvh(bvh_count, root4, other, stack_depth, stack16 != 0) ? 1 : 0;
}

int vr_scene_launch_variant(const vr_scene* s, uint64_t pixel_samples, uint32_t launch_flags, int32_t recording,
                            uint32_t* variant) {
    if (!s || !variant) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    const bool counting = (launch_flags & VR_LAUNCH_COUNTERS) != 0;
    launch_flags |= s->debug_launch_flags;
    const bool gated = coop_gated(s, pixel_samples);
    *variant = variant_bits(launch_choice(s, gated && !(launch_flags & VR_LAUNCH_NO_COOP), gated, counting, recording != 0,
                                          launch_flags));
    return VR_OK;
}

int vr_render_tile_device(const vr_scene* s, const vr_render_params* p, double* state, void* stream,
                          uint32_t launch_flags, vr_launch_stats* stats) {
    int rc = check_render_params(s, p);
    if (rc) return rc;
    if (!state) return fail(VR_ERROR_INVALID_ARGUMENT, "null state");
    VR_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    vr_scene* ms = const_cast<vr_scene*>(s);
    const bool counting = (launch_flags & VR_LAUNCH_COUNTERS) != 0;
    const bool timed = (launch_flags & VR_LAUNCH_TIMED) != 0 || counting;
    // timed without waiting: the events stay with the scene until vr_collect_launch_times
    const bool defer = timed && !counting && (launch_flags & VR_LAUNCH_DEFER_TIMES) != 0;
    int32_t* slot = nullptr;
    rc = stream_slot(ms, stream, &slot);
    if (rc) return rc;
    if (defer) {  // a caller that defers must collect: the pending events are bounded per stream
        std::lock_guard<std::mutex> g(ms->slot_mutex);
        auto it = ms->deferred.find(stream);
        if (it != ms->deferred.end() && it->second.passes.size() >= vr::kMaxDeferredLaunches)
            return fail(VR_ERROR_INVALID_ARGUMENT,
                        "too many VR_LAUNCH_DEFER_TIMES launches on this stream without vr_collect_launch_times");
    }
    std::unique_lock<std::mutex> lock(ms->counter_mutex, std::defer_lock);
    // diagnostic (tools): with counters, VR_WG_TIMES_PATH receives per-workgroup start/end stamps
    const char* wg_path = counting ? tuning_env("VR_WG_TIMES_PATH") : nullptr;
    CallScratch wg;
    const uint64_t blocks = (uint64_t)std::max(1, s->cu_count) * grid_per_cu();  // persistent grid limit
    unsigned long long* counters = nullptr;
    if (counting) {
        lock.lock();
        VR_HIP(hipMemsetAsync(s->d_counters, 0, sizeof(unsigned long long) * vr::kCntCount, st));
        counters = s->d_counters;
        if (wg_path) VR_HIP(hipMalloc(&wg.ptr, blocks * 2 * sizeof(unsigned long long)));
    }
    PassEvents pe;
    uint32_t variant = 0;
    CallCtx* c = nullptr;
    rc = ctx_acquire(ms, &c, &st);
    if (rc) return rc;
    rc = enqueue_passes(ms, c, p, state, st, slot, counting, false, nullptr, counters, (unsigned long long*)wg.ptr,
                        timed ? &pe : nullptr, launch_flags, &variant);
    ctx_release(ms, c);  // (its `done` orders the next user after the work just queued)
    if (rc) return rc;
    vr_launch_stats out;  // what *stats receives: zero but for what this kind of launch measures
    std::memset(&out, 0, sizeof out);
    out.variant = variant;
    if (!timed) {  // errors of this launch: vr_stream_check_error(scene, stream)
        if (stats) *stats = out;
        return VR_OK;
    }
    if (defer) {
        std::lock_guard<std::mutex> g(ms->slot_mutex);
        vr_scene::Deferred& d = ms->deferred[stream];
        d.ev.insert(d.ev.end(), pe.ev.begin(), pe.ev.end());
        d.passes.push_back((uint32_t)(pe.ev.size() / 3));
        pe.ev.clear();  // owned by the scene now
        out.passes = d.passes.back();
        if (stats) *stats = out;
        return VR_OK;
    }
    float render_ms = 0.f, reduce_ms = 0.f;
    rc = sum_pass_times(pe.ev, &render_ms, &reduce_ms);
    if (rc) return rc;
    out.kernel_ms = render_ms;
    out.reduce_ms = reduce_ms;
    out.passes = (uint32_t)(pe.ev.size() / 3);
    out.timed = 1;
    if (stats) *stats = out;
    if (counting) {
        unsigned long long c[vr::kCntCount];
        VR_HIP(hipMemcpy(c, s->d_counters, sizeof c, hipMemcpyDeviceToHost));
        if (const char* cp = tuning_env("VR_COUNTERS_PATH")) {  // diagnostic: the raw counter array
            if (FILE* f = std::fopen(cp, "wb")) {
                std::fwrite(c, sizeof c, 1, f);
                std::fclose(f);
            }
        }
        if (wg_path && wg.ptr) {
            std::vector<unsigned long long> t(blocks * 2);
            VR_HIP(hipMemcpy(t.data(), wg.ptr, t.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            if (FILE* f = std::fopen(wg_path, "wb")) {
                std::fwrite(t.data(), sizeof(unsigned long long), t.size(), f);
                std::fclose(f);
            }
        }
        if (stats) {
            stats->box_tests = c[vr::kCntBoxTests];
            stats->node_visits = c[vr::kCntNodeVisits];
            stats->triangle_tests = c[vr::kCntTriangleTests];
            stats->rays = c[vr::kCntRays];
            stats->shaded_triangle_hits = c[vr::kCntShadedTriangles];
            stats->samples = c[vr::kCntSamples];
            stats->traversal_slots = c[vr::kCntTraversalSlots];
            stats->path_loop_slots = c[vr::kCntOuterSlots];
            stats->exact_box_tests = c[vr::kCntExactBoxes];
        }
    }
    return read_and_clear_error(slot, st);
}

int vr_collect_launch_times(const vr_scene* s, void* stream, vr_launch_times* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (s->host_only) return host_only_error();
    VR_HIP(hipSetDevice(s->device));
    vr_scene* ms = const_cast<vr_scene*>(s);
    vr_scene::Deferred d;
    int32_t* slot = nullptr;
    {
        std::lock_guard<std::mutex> g(ms->slot_mutex);
        auto it = ms->deferred.find(stream);
        if (it != ms->deferred.end()) {
            d = std::move(it->second);
            ms->deferred.erase(it);
        }
        auto sl = ms->stream_slots.find(stream);
        if (sl != ms->stream_slots.end()) slot = sl->second;
    }
    PassEvents pe;  // destroys the events on every exit
    pe.ev = std::move(d.ev);
    std::memset(out, 0, sizeof *out);
    const int rc = sum_pass_times(pe.ev, &out->kernel_ms, &out->reduce_ms);
    if (rc) return rc;
    out->launches = (uint32_t)d.passes.size();
    for (uint32_t n : d.passes) {
        out->passes += n;
        out->max_passes = std::max(out->max_passes, n);
    }
    // the device errors of those launches, as a timed launch reports its own
    return slot ? read_and_clear_error(slot, (hipStream_t)stream) : VR_OK;
}

int vr_stream_check_error(const vr_scene* s, void* stream) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if (s->host_only) return host_only_error();
    VR_HIP(hipSetDevice(s->device));
    int32_t* slot = nullptr;
    {
        vr_scene* ms = const_cast<vr_scene*>(s);
        std::lock_guard<std::mutex> g(ms->slot_mutex);
        auto it = ms->stream_slots.find(stream);
        if (it != ms->stream_slots.end()) slot = it->second;
    }
    if (!slot) {  // nothing of this scene was ever launched on the stream
        VR_HIP(hipStreamSynchronize((hipStream_t)stream));
        return VR_OK;
    }
    return read_and_clear_error(slot, (hipStream_t)stream);
}

int vr_render_tile(const vr_scene* s, const vr_render_params* p, vr_accumulation_buffer* buf) {
    int rc = check_render_params(s, p);
    if (rc) return rc;
    const uint64_t tw = p->tile.end_column - p->tile.start_column, th = p->tile.end_row - p->tile.start_row;
    if (!buf || buf->width != tw || buf->height != th || !buf->colour || !buf->colour_sum || !buf->colour_bias ||
        !buf->weight || !buf->weight_bias)
        return fail(VR_ERROR_INVALID_ARGUMENT, "accumulation buffer does not match the tile");
    const uint64_t n = tw * th;
    if (n == 0) return VR_OK;
    HostCall call;
    rc = call.begin(s);
    if (rc) return rc;
    CallCtx* c = call.c;
    const hipStream_t st = call.st;
    // device records (64 B per pixel), then the host layout (88 B per pixel: colour, colour_sum,
    // colour_bias, weight, weight_bias back to back)
    const size_t o_state = call.part(n * 64), o_planar = call.part(n * 88);
    rc = call.grow();
    if (rc) return rc;
    double *const state = (double*)call.at(o_state), *const planar = (double*)call.at(o_planar);
    // one sample into a fresh buffer (vr_partial_render_scene, the reference's per-call pattern):
    // only colour_sum comes back (24 B per pixel), the host derives the other four arrays
    const bool fresh1 = !p->accumulate && p->spp == 1;
    const size_t payload = (fresh1 ? 24 : 88) * n;
    rc = ctx_grow_pinned(c, payload + 256);  // + the call's error word
    if (rc) return rc;
    double* host = (double*)c->pinned;  // same layout as `planar`
    const size_t b3 = n * 3 * sizeof(double), b1 = n * sizeof(double);
    if (p->accumulate) {  // continue update_pixel from the caller's buffer
        parallel_copy(host + 3 * n, buf->colour_sum, b3);
        parallel_copy(host + 6 * n, buf->colour_bias, b3);
        parallel_copy(host + 9 * n, buf->weight, b1);
        parallel_copy(host + 10 * n, buf->weight_bias, b1);
        VR_HIP(hipMemcpyAsync(planar + 3 * n, host + 3 * n, 2 * b3 + 2 * b1, hipMemcpyHostToDevice, st));
        const int e = vr::launch_buffer_convert(planar, state, n, 0, st);
        if (e) return device_fail(e, "buffer import");
    } else {  // AccumulationBuffer::new
        VR_HIP(hipMemsetAsync(state, 0, n * 64, st));
    }
    rc = enqueue_passes(const_cast<vr_scene*>(s), c, p, state, st, c->error, false, false, nullptr, nullptr, nullptr);
    if (rc) return rc;
    const int e = vr::launch_buffer_convert(state, planar, n, fresh1 ? 2 : 1, st);
    if (e) return device_fail(e, "buffer export");
    VR_HIP(hipMemcpyAsync(host, planar, fresh1 ? b3 : 3 * b3 + 2 * b1, hipMemcpyDeviceToHost, st));
    volatile int32_t* flag = (volatile int32_t*)((char*)host + payload);  // the error word rides along
    VR_HIP(hipMemcpyAsync((void*)flag, c->error, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(c->done, st));
    static const bool host_timing = tuning_env("VR_HOST_TIMING") != nullptr;  // diagnostic (tools/dropin.py)
    const auto t_enq = std::chrono::steady_clock::now();
    VR_HIP(hipEventSynchronize(c->done));
    if (const int32_t bits = *flag) {
        VR_HIP(hipMemsetAsync(c->error, 0, sizeof(int32_t), st));
        VR_HIP(hipStreamSynchronize(st));
        return error_status(bits);
    }
    const auto t_dev = std::chrono::steady_clock::now();
    struct Report {
        bool on;
        std::chrono::steady_clock::time_point a, b;
        ~Report() {
            if (on)
                std::fprintf(stderr, "vr_render_tile host timing: device wait %.3f ms, host copy-out %.3f ms\n",
                             std::chrono::duration<double, std::milli>(b - a).count(),
                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - b).count());
        }
    } report{host_timing, t_enq, t_dev};
    if (fresh1) {
        // update_pixel (accumulation_buffer.rs:44-60) from zeros with weight 1: weight 1, weight bias
        // (1 - 0) - 1 = 0; colour_sum t = 0 + y with y = c * 1 - 0, so y == t bit for bit except y = -0
        // (t = +0), where the bias (t - 0) - y is +0 either way; colour = t * (1 / 1)
        parallel_range(n, (uint64_t)1 << 14, [&](uint64_t b, uint64_t e) {
            for (uint64_t i = b; i < e; ++i) {
                for (int k = 0; k < 3; ++k) {
                    const double t = host[3 * i + k];
                    buf->colour_sum[3 * i + k] = t;
                    buf->colour_bias[3 * i + k] = (t - 0.0) - t;
                    buf->colour[3 * i + k] = t * (1.0 / 1.0);
                }
                buf->weight[i] = 1.0;
                buf->weight_bias[i] = 0.0;
            }
        });
    } else {
        parallel_copy(buf->colour, host, b3);
        parallel_copy(buf->colour_sum, host + 3 * n, b3);
        parallel_copy(buf->colour_bias, host + 6 * n, b3);
        parallel_copy(buf->weight, host + 9 * n, b1);
        parallel_copy(buf->weight_bias, host + 10 * n, b1);
    }
    return VR_OK;
}

int vr_partial_render_scene(const vr_scene* s, vr_tile tile, uint64_t height, uint64_t width,
                            vr_accumulation_buffer* out) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    vr_render_params p{};
    p.tile = tile;
    p.height = height;
    p.width = width;
    p.spp = 1;
    p.accumulate = 0;
    p.seed = s->partial_seed;
    p.first_sample = const_cast<vr_scene*>(s)->pass_counter.fetch_add(1);
    return vr_render_tile(s, &p, out);
}

int vr_render_samples(const vr_scene* s, const vr_render_params* p, vr_sample_record* out) {
    int rc = check_render_params(s, p);
    if (rc) return rc;
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "null output");
    const uint64_t tw = p->tile.end_column - p->tile.start_column, th = p->tile.end_row - p->tile.start_row;
    const uint64_t n = tw * th;
    if (n == 0 || p->spp == 0) return VR_OK;
    HostCall call;
    rc = call.begin(s);
    if (rc) return rc;
    CallCtx* c = call.c;
    const hipStream_t st = call.st;
    const size_t rec_bytes = n * p->spp * sizeof(vr_sample_record);
    const size_t o_state = call.part(n * 64), o_rec = call.part(rec_bytes);
    rc = call.grow();
    if (rc) return rc;
    double* const state = (double*)call.at(o_state);
    void* const rec = call.at(o_rec);
    VR_HIP(hipMemsetAsync(state, 0, n * 64, st));
    vr_render_params q = *p;
    q.accumulate = 0;
    rc = enqueue_passes(const_cast<vr_scene*>(s), c, &q, state, st, c->error, false, true, rec, nullptr, nullptr);
    if (rc) return rc;
    VR_HIP(hipMemcpyAsync(out, rec, rec_bytes, hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(c->done, st));
    return read_and_clear_error(c->error, st);
}
