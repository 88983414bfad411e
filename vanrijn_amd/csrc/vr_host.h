// vr_host.h -- internal to the host side (vr_host.cpp, vr_host_*.cpp; not installed): what crosses its files.
// Everything declared here has hidden visibility: the library exports include/vanrijn_amd.h only.
// The builder and io files define VR_HOST_NO_HIP first and see the HIP-free top part alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/vanrijn_amd.h"
#include "vr_layout.h"

#pragma GCC visibility push(hidden)
namespace vrh {

int fail(int code, const std::string& msg);  // sets vr_last_error's message (vr_host_io.cpp); returns code

// Environment overrides exist in tuning builds only (python -m vanrijn_amd.build with VR_TUNING=1,
// -DVR_TUNING_VARIANTS: tools/variants.py threshold sweeps, tools/cycles.py diagnostics); a default
// build reads no VR_* variable, so nothing in a user's environment changes rendering or timing.
inline const char* tuning_env(const char* name) {
#ifdef VR_TUNING_VARIANTS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// what vr_scene_set_camera_pose admits (the block cull's margins are sized for these bounds): null, or why
// not.  vr_camera_look_at and the reprojection's argument check (vr_host_reproject.cpp) share it.
inline const char* pose_error(const vr_camera_pose& p) {
    const vr_vec3 axes[3] = {p.right, p.up, p.forward};
    bool finite = std::isfinite(p.location.x) && std::isfinite(p.location.y) && std::isfinite(p.location.z) &&
                  std::isfinite(p.film_distance);
    for (const vr_vec3& a : axes) finite = finite && std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z);
    if (!finite) return "camera pose: an entry is not finite";
    if (!(p.film_distance >= 1e-3 && p.film_distance <= 1e3)) return "camera pose: film_distance outside [1e-3, 1e3]";
    const auto dot = [](vr_vec3 a, vr_vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; };
    for (int i = 0; i < 3; ++i) {
        if (std::fabs(dot(axes[i], axes[i]) - 1.0) > 1e-9) return "camera pose: an axis is not of unit length (1e-9)";
        if (std::fabs(dot(axes[i], axes[(i + 1) % 3])) > 1e-9) return "camera pose: two axes are not orthogonal (1e-9)";
    }
    return nullptr;
}

// host threads (vr_host_io.cpp): fn(begin, end) over [0, n) in pieces of at least `grain`; a parallel memcpy
void parallel_range(uint64_t n, uint64_t grain, const std::function<void(uint64_t, uint64_t)>& fn);
void parallel_copy(void* dst, const void* src, size_t bytes);

// ---- the BVH builders (vr_host_bvh.cpp): plain data in and out, no scene and no HIP ----
float round_lower(double v);  // f32 copies of f64 box bounds, rounded outward
float round_upper(double v);
// root box (vr::Bvh::root_box's layout; the empty box for n == 0) and max |coordinate| of n triangles
void mesh_bounds(const double* vertices, uint64_t n, double root_box[6], double* extent);
// One mesh's host-built trees.  nodes: the traversal tree (binned SAH, or the reference's median split)
// with interior links offset by node_base and leaves ~(tri_base + slot); order[r]: the input triangle
// at reference leaf position r; rank[i]: the reference leaf position of traversal slot i
struct MeshTree {
    std::vector<vr::Node> nodes;
    std::vector<uint64_t> order, rank;
    int32_t root = INT32_MIN;  // an empty mesh; else an interior node, or ~tri_base for one triangle
    int depth = 0;
    double root_box[6], extent = 0.0;
};
MeshTree build_mesh_tree(const double* vertices, uint64_t n, int32_t tri_base, int32_t node_base, bool sah);
// the render kernel's 4-wide tree over every BVH record's binary tree in `nodes`; roots: per record
struct WideTree {
    std::vector<vr::Node4> nodes4;
    std::vector<int32_t> roots;
    int stack = 0;  // deepest traversal stack
};
WideTree collapse_wide(const std::vector<vr::Node>& nodes, const std::vector<vr::Bvh>& bvhs, bool greedy);
// the 4-wide tree of a device-built (median-split) mesh of n >= 2 triangles, planned from n alone:
// appends to desc (vr_build.hip fill_wide_kernel's descriptor), raises stack, returns the root
int32_t shape_wide(uint64_t n, int32_t node_base, int32_t tri_base, std::vector<int32_t>& desc, int& stack);

}  // namespace vrh
#pragma GCC visibility pop

#ifndef VR_HOST_NO_HIP
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <unordered_map>
#include <utility>

#include "vr_camera.h"

#define VR_HIP(call)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(VR_ERROR_DEVICE, std::string(#call " failed: ") + hipGetErrorString(e_)); \
    } while (0)

struct CallCtx;
struct vr_scene {
    int device = -1;
    bool host_only = false;
    double camera[3];
    // the camera pose beside the location (vr_scene_set_camera_pose): the default is the reference's camera
    vr::PoseArgs pose = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}, 1.0};
    // the camera lens (vr_scene_set_camera_lens): radius 0 is no lens
    vr::LensArgs lens = {0.0, 1.0};
    double extent = 0.0;
    std::vector<vr::Material> materials;
    std::vector<vr::Prim> prims;
    std::vector<vr::Bvh> bvhs;
    std::vector<double> light_dirs;  // Whitted: 3 per light
    std::vector<vr::Node> nodes;
    std::vector<vr::Node4> nodes4;  // the render kernel's 4-wide tree (collapse_wide)
    int wide_stack = 0;             // deepest traversal stack of the 4-wide tree
    uint64_t wide_count = 0;        // its node count
    std::vector<vr::TriVerts> tris;
    std::vector<vr::TriNormals> normals;
    std::vector<std::vector<uint64_t>> leaf_order;  // per mesh
    std::vector<int> mesh_tri_base;
    int max_depth = 0;
    uint32_t object_count = 0;
    // VR_SCENE_DEVICE_BVH: the meshes' BVHs are built on the device after upload (host vectors
    // nodes / tris / normals stay empty; the counts below size the device arrays)
    bool device_bvh = false;
    bool device_sah = false;  // VR_SCENE_DEVICE_SAH: the SAH traversal tree too (vr_build.hip)
    bool greedy_collapse = false;  // VR_SCENE_GREEDY_COLLAPSE: the 4-wide tree by largest child area
    bool force_big = false;        // VR_SCENE_WIDE_OFFSETS: the 64-bit-offset kernels for any size
    uint64_t staging_limit = 0;    // vr_scene_set_staging_limit: bytes of staging per call (0: half the free HBM)
    uint64_t node_count = 0, tri_count = 0;
    struct PendingMesh {
        const double* vertices;
        const double* normals;
        uint64_t n;
        int32_t node_base, tri_base;
        uint32_t mesh;
    };
    std::vector<PendingMesh> pending;
    bool dark0 = true;  // every material's colour(0 nm) == 0: the recursion-limit photon needs no lambda-0 chain
    int mats = 0;       // bit 0: a Lambertian material exists, bit 1: a reflective one
    // every continuation of every path yields a finite intensity (shading_finite on each traced
    // mesh, no Phong or dielectric material): then a path with zero throughput may stop early and
    // the recursion-limit lambda-0 chain may be taken as b0 (DARK0); otherwise both are traced so
    // that a later NaN reaches the photon as in the reference (0 * NaN)
    bool nan_free = true;
    // device copies
    void* d_block = nullptr;
    size_t device_bytes = 0;
    vr::DeviceScene dev{};
    unsigned long long* d_counters = nullptr;
    std::mutex counter_mutex;
    std::atomic<uint64_t> pass_counter{0};
    // render-call contexts (stream, staging buffer, work-queue counter, error word, scratch),
    // pooled: concurrent calls each hold their own, so they neither share a staging buffer nor
    // read each other's error word (include/vanrijn_amd.h "Threading")
    std::mutex ctx_mutex;
    std::vector<struct CallCtx*> ctx_all, ctx_free;
    // sticky per-stream error words of the asynchronous entry point (vr_render_tile_device),
    // read and cleared by vr_stream_check_error or a timed launch on that stream
    std::mutex slot_mutex;
    std::unordered_map<void*, int32_t*> stream_slots;
    // deferred launch timings (VR_LAUNCH_DEFER_TIMES), per stream, under slot_mutex: the HIP events
    // of launches not yet read by vr_collect_launch_times -- [start, mid, end] per pass -- and the
    // passes of each launch
    struct Deferred {
        std::vector<hipEvent_t> ev;
        std::vector<uint32_t> passes;
    };
    std::unordered_map<void*, Deferred> deferred;
    int cu_count = 0;
    uint64_t partial_seed = 0x5EED0001ull;
    // test hook (vr_debug_set_fault_object): hits on this object take the singular-basis path,
    // which finite geometry cannot reach (DESIGN.md "Errors")
    int32_t fault_object = -1;
    // test hook (vr_debug_set_launch_flags): launch flags OR'ed into every render of the scene
    uint32_t debug_launch_flags = 0;
    // vr_scene_update_mesh: the parts extent, NAN_FREE and dark0 are put together from
    // (update_scalars), where each mesh's records are, and the per-mesh plans
    double base_extent = 0.0;             // camera and primitives
    std::vector<double> mesh_extent;      // max |coordinate| of each mesh
    std::vector<uint8_t> mesh_finite;     // shading_finite of each mesh (1 where no object traces it)
    bool dark0_materials = true;          // dark0's materials-only part
    // the rows of `materials` lie on one wavelength grid, bit for bit (update_grid_shared): the desc's
    // materials and the Whitted light rows (grid_shared), and the sky row as well (sky_on_grid, never set
    // without grid_shared); materials[0] is the scene's copy of that grid
    bool grid_shared = false, sky_on_grid = false;
    std::vector<int> mesh_object;         // the BVH object a mesh backs, or -1
    std::vector<int> mesh_bvh;            // its record in bvhs, or -1
    std::vector<uint32_t> mesh_material;  // vr_mesh_desc::material (what TriNormals::material1 == 0 stands for)
    std::vector<int32_t> mesh_node_base;  // its first interior node (the root of a mesh of 2 or more triangles)
    std::vector<int32_t> mesh_root4;      // its 4-wide root node, or kEmptyChild
    bool host_stale = false;  // a device update ran: the host copies of trees and triangles are the creation's
    struct UpdatePlan {
        bool built = false;
        std::vector<uint32_t> slot_src;       // per slot of the mesh: the input triangle it holds
        std::vector<int32_t> items2, items4;  // node indices of the binary / 4-wide tree grouped by depth
        std::vector<uint32_t> first2, first4; // items[first[l] .. first[l + 1]): depth l (root 0)
        // device copy: [Validation | slot_src | items2 | items4], and the host form's uploaded arrays
        void* d_plan = nullptr;
        size_t plan_bytes = 0;
        unsigned long long* d_valid = nullptr;
        uint32_t* d_slot_src = nullptr;
        int32_t *d_items2 = nullptr, *d_items4 = nullptr;
        void* d_stage = nullptr;
        size_t stage_bytes = 0;
    };
    std::vector<UpdatePlan> plans;
    // scene edits (vr_scene_set_camera, vr_scene_update_primitives, vr_scene_update_material,
    // vr_scene_set_lights): what of the creation desc they need
    uint32_t desc_materials = 0;                   // vr_scene_desc::material_count (the addressable rows)
    std::vector<std::vector<uint32_t>> prim_rows;  // per vr_scene_desc::primitives entry: its rows in prims
    // vr_scene_transform_mesh: a mesh's base geometry, a copy of its triangle and normal records in slot
    // order (host vectors on VR_SCENE_HOST_ONLY scenes, else d_base = [n TriVerts | n TriNormals]), made
    // at the first transform; a successful vr_scene_update_mesh marks it stale, and the next transform
    // takes it again from the records
    struct MeshBase {
        bool current = false;
        std::vector<vr::TriVerts> tris;
        std::vector<vr::TriNormals> normals;
        void* d_base = nullptr;
    };
    std::vector<MeshBase> bases;
};

// One render call's device resources.  `done` is recorded on the launch stream after the last
// kernel that reads `staging` / `queue`; a later user of the context waits on it first.
struct CallCtx {
    hipStream_t stream = nullptr;  // the host-buffer entry points' own stream
    hipEvent_t done = nullptr;
    void* staging = nullptr;  // 16 B per (pixel, sample) of a pass
    size_t staging_bytes = 0;
    unsigned long long* queue = nullptr;  // work-item counter; error word at queue + 8
    int32_t* error = nullptr;
    void* scratch = nullptr;  // device records + host-layout buffers of the host-buffer calls
    size_t scratch_bytes = 0;
    void* pinned = nullptr;  // page-locked host copy of the host-layout buffers (DMA at full PCIe rate)
    size_t pinned_bytes = 0;
    void* mask = nullptr;  // camera-frustum culled 8x8 blocks of the call's tile (1 B each)
    size_t mask_bytes = 0;
    hipStream_t last_stream = nullptr;  // the stream of the last call's work (enqueue_passes)
    bool used = false;
    // debug builds (-DVR_STAGE_GUARD): a generation tag beside every staging slot, and the last
    // pass generation this context used
    void* tags = nullptr;
    size_t tag_bytes = 0;
    uint32_t gen = 0;
};

#pragma GCC visibility push(hidden)
namespace vrh {

struct CallScratch {  // a stream and a device buffer for the length of one call
    hipStream_t stream = nullptr;
    void* ptr = nullptr;
    ~CallScratch() {
        if (ptr) (void)hipFree(ptr);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

inline int device_fail(int e, const char* what) {  // "what: HIP's message" for a launch wrapper's hipError_t
    return fail(VR_ERROR_DEVICE, std::string(what) + ": " + hipGetErrorString((hipError_t)e));
}
inline int launch_status(int lr) {  // a vr_render / vr_query / vr_integrate launch wrapper's code (-1000: no stack class)
    return fail(lr == -1000 ? VR_ERROR_UNSUPPORTED : VR_ERROR_DEVICE, vr::device_error_string(lr));
}
inline int host_only_error() { return fail(VR_ERROR_HOST_ONLY, "scene was created with VR_SCENE_HOST_ONLY"); }
int error_status(int32_t bits);  // a nonzero device error word as a status and message

inline int stack_depth(const vr_scene* s) { return std::max(1, s->max_depth - 1); }  // binary tree walks
inline int wide_stack_depth(const vr_scene* s) { return s->wide_stack + 1; }  // render kernel (+1: branchless pushes)

// vr_host_scene.cpp: rows of the scene block (a message on a bad description), the scene scalars
const char* material_row(const vr_material_desc& m, vr::Material& dm);
const char* light_rows(const vr_integrator_desc& ig, std::vector<vr::Material>& rows, std::vector<double>& dirs);
const char* prim_row(const vr_primitive_desc& p, int32_t object, int32_t position, vr::Prim& dp);
void update_base_extent(vr_scene* s);
void update_material_scalars(vr_scene* s);
void update_scalars(vr_scene* s);
bool grids_shared(const vr::Material* rows, size_t count);
void update_grid_shared(vr_scene* s);

// vr_host.cpp: the call-context pool and the render path
void ctx_free_all(CallCtx* c);
int ctx_grow(void** ptr, size_t* have, size_t need, hipEvent_t done);
int ctx_grow_pinned(CallCtx* c, size_t need);
int stream_slot(vr_scene* s, void* stream, int32_t** out);
int read_and_clear_error(int32_t* slot, hipStream_t stream);
int check_render_params(const vr_scene* s, const vr_render_params* p);
uint64_t seed_key_of(uint64_t seed);
vr::RenderArgs make_args(const vr_scene* s, const vr_render_params* p, double* state);
struct PassEvents;
int enqueue_passes(vr_scene* s, CallCtx* c, const vr_render_params* p, double* state, hipStream_t st, int32_t* err,
                   bool counting, bool recording, void* records, unsigned long long* counters,
                   unsigned long long* wg_times, PassEvents* timing = nullptr, uint32_t launch_flags = 0,
                   uint32_t* variant = nullptr);

// A host-buffer call: begin() selects the scene's device, takes a context from its pool and makes the
// context's own stream `st` wait for the context's last user.  From then on every exit records `done`
// on `st` -- so the next user, on whatever stream, is ordered after the work this call left queued
// on the context's staging, mask, queue counter and scratch -- and hands the context back.
// The call's device buffers are parts of c->scratch: part() declares them, grow() sizes the scratch
// once, at() gives their addresses.  Every part starts 256-B aligned: the kernels take each part as
// its own pointer and need at most 16 B, so how tightly the parts pack carries no meaning.
struct HostCall {
    CallCtx* c = nullptr;
    hipStream_t st = nullptr;
    int begin(const vr_scene* s);
    ~HostCall();
    size_t part(size_t bytes) { return std::exchange(total_, total_ + ((bytes + 255) & ~size_t(255))); }
    int grow() { return ctx_grow(&c->scratch, &c->scratch_bytes, total_, c->done); }
    char* at(size_t offset) const { return (char*)c->scratch + offset; }

  private:
    vr_scene* scene_ = nullptr;
    bool begun_ = false;
    size_t total_ = 0;
};

}  // namespace vrh
#pragma GCC visibility pop
#endif  // VR_HOST_NO_HIP
