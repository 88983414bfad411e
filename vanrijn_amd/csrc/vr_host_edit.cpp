// vr_host_edit.cpp -- changes to a created scene: vr_scene_update_mesh (new vertices for one mesh,
// both trees refitted in place; vr_refit.h holds the per-record steps, vr_refit.hip the device
// stages), and the scene edits, each in a host form (VR_SCENE_HOST_ONLY) and a device form.
#include "vr_host.h"
#include "vr_refit.h"

using namespace vrh;

namespace {

// The plan of mesh `mi`, built at its first update: which input triangle every slot holds (from the
// ranks in the slots and the leaf order) and both trees' node indices grouped by depth, found by
// walking the child links from the roots.  Device-built scenes keep no host copy of the trees, so
// their links are read back here, once.  Every index is range-checked: the kernels trust the plan.
int build_update_plan(vr_scene* s, uint32_t mi) {
    vr_scene::UpdatePlan& p = s->plans[mi];
    if (p.built) return VR_OK;
    const uint64_t n = s->leaf_order[mi].size(), interior = n ? n - 1 : 0;
    const int64_t tri_base = s->mesh_tri_base[mi], node_base = s->mesh_node_base[mi];
    const bool readback = !s->host_only && s->device_bvh;
    std::vector<vr::TriVerts> tv;
    std::vector<vr::Node> bn;
    std::vector<vr::Node4> wn;
    if (readback) {
        tv.resize(n);
        bn.resize(interior);
        wn.resize(s->wide_count);
        VR_HIP(hipMemcpy(tv.data(), s->dev.tris + tri_base, n * sizeof(vr::TriVerts), hipMemcpyDeviceToHost));
        if (interior)
            VR_HIP(hipMemcpy(bn.data(), s->dev.nodes + node_base, interior * sizeof(vr::Node), hipMemcpyDeviceToHost));
        if (s->wide_count)
            VR_HIP(hipMemcpy(wn.data(), s->dev.nodes4, s->wide_count * sizeof(vr::Node4), hipMemcpyDeviceToHost));
    }
    const vr::TriVerts* tris = readback ? tv.data() : s->tris.data() + tri_base;      // the mesh's slots
    const vr::Node* nodes = readback ? bn.data() : s->nodes.data() + node_base;        // the mesh's nodes
    const vr::Node4* nodes4 = readback ? wn.data() : s->nodes4.data();                 // every wide node
    const uint64_t wide_count = readback ? wn.size() : s->nodes4.size();
    const char* corrupt = "scene update: the tree's links do not form the mesh's tree";
    p.slot_src.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = tris[i].rank - tri_base;
        if (r < 0 || (uint64_t)r >= n || s->leaf_order[mi][(size_t)r] >= n) return fail(VR_ERROR_DEVICE, corrupt);
        p.slot_src[i] = (uint32_t)s->leaf_order[mi][(size_t)r];
    }
    auto leaf_ok = [&](int32_t ch) { return (int64_t)~ch >= tri_base && (uint64_t)((int64_t)~ch - tri_base) < n; };
    // a tree's node indices grouped by depth, walking `fan` child links per node from `root`; `count`
    // nodes from index `base` on may be met (more: a cycle); false where a link leaves the mesh's tree
    auto levels = [&](int32_t root, int fan, auto child, int64_t base, uint64_t count, std::vector<int32_t>& items,
                      std::vector<uint32_t>& first) {
        auto node_ok = [&](int32_t x) { return x >= base && (uint64_t)(x - base) < count; };
        items.clear();
        first.assign(1, 0);
        std::vector<int32_t> frontier, next;
        if (root != vr::kEmptyChild) {
            if (!node_ok(root)) return false;
            frontier.push_back(root);
        }
        while (!frontier.empty()) {
            next.clear();
            for (int32_t x : frontier) {
                items.push_back(x);
                for (int c = 0; c < fan; ++c) {
                    const int32_t ch = child(x, c);
                    if (fan == 4 && ch == vr::kEmptyChild) continue;
                    if (ch >= 0 ? !node_ok(ch) : !leaf_ok(ch)) return false;
                    if (ch >= 0) next.push_back(ch);
                }
            }
            if (items.size() + next.size() > count) return false;
            first.push_back((uint32_t)items.size());
            frontier.swap(next);
        }
        return true;
    };
    if (!levels(n >= 2 ? (int32_t)node_base : vr::kEmptyChild, 2, [&](int32_t x, int c) { return nodes[x - node_base].child[c]; },
                node_base, interior, p.items2, p.first2) ||
        !levels(s->mesh_root4[mi], 4, [&](int32_t x, int c) { return nodes4[x].child[c]; }, 0, wide_count, p.items4, p.first4))
        return fail(VR_ERROR_DEVICE, corrupt);
    if (!s->host_only) {
        auto a16 = [](size_t b) { return (b + 15) & ~size_t(15); };
        const size_t o_src = a16(sizeof(vr::refit::Validation)), o_i2 = o_src + a16(4 * n),
                     o_i4 = o_i2 + a16(4 * p.items2.size()), total = o_i4 + a16(4 * p.items4.size());
        VR_HIP(hipMalloc(&p.d_plan, total));
        p.plan_bytes = total;
        s->device_bytes += total;
        char* b = (char*)p.d_plan;
        p.d_valid = (unsigned long long*)b;
        p.d_slot_src = (uint32_t*)(b + o_src);
        p.d_items2 = (int32_t*)(b + o_i2);
        p.d_items4 = (int32_t*)(b + o_i4);
        if (n) VR_HIP(hipMemcpy(p.d_slot_src, p.slot_src.data(), 4 * n, hipMemcpyHostToDevice));
        if (!p.items2.empty()) VR_HIP(hipMemcpy(p.d_items2, p.items2.data(), 4 * p.items2.size(), hipMemcpyHostToDevice));
        if (!p.items4.empty()) VR_HIP(hipMemcpy(p.d_items4, p.items4.data(), 4 * p.items4.size(), hipMemcpyHostToDevice));
    }
    p.built = true;
    return VR_OK;
}

// both trees, the root record and the scene scalars once the mesh's records hold the new geometry
void refit_host(vr_scene* s, uint32_t mi, double max_abs, const vr::refit::Validation& val) {
    const vr_scene::UpdatePlan& p = s->plans[mi];
    for (size_t l = p.first2.size() - 1; l-- > 0;)
        for (uint32_t k = p.first2[l]; k < p.first2[l + 1]; ++k)
            vr::refit::refit_node(s->nodes.data(), s->tris.data(), p.items2[k]);
    for (size_t l = p.first4.size() - 1; l-- > 0;)
        for (uint32_t k = p.first4[l]; k < p.first4[l + 1]; ++k)
            vr::refit::refit_node4(s->nodes4.data(), s->tris.data(), p.items4[k]);
    if (s->mesh_bvh[mi] >= 0) vr::refit::refit_root(&s->bvhs[s->mesh_bvh[mi]], s->nodes.data(), s->tris.data());
    s->mesh_extent[mi] = max_abs;
    s->mesh_finite[mi] = s->mesh_object[mi] < 0 || val.not_finite == 0;
    update_scalars(s);
}

// the refit in plain C++ on the host arrays (VR_SCENE_HOST_ONLY): the steps of vr_refit.hip in its order
int update_mesh_host(vr_scene* s, uint32_t mi, uint64_t n, const double* verts, const double* norms) {
    vr::refit::Validation val{};
    double max_abs = 0.0;
    for (uint64_t t = 0; t < n; ++t) {
        for (int i = 0; i < 9; ++i) {
            if (!std::isfinite(verts[9 * t + i])) ++val.nonfinite;
            max_abs = std::max(max_abs, std::fabs(verts[9 * t + i]));
        }
        if (!vr::refit::tri_shading_finite(verts + 9 * t, norms + 9 * t)) ++val.not_finite;
    }
    if (val.nonfinite) return fail(VR_ERROR_UNSUPPORTED, "scene update: a vertex coordinate is not finite");
    vr_scene::UpdatePlan& p = s->plans[mi];
    if (const int rc = build_update_plan(s, mi)) return rc;
    const int32_t tri_base = s->mesh_tri_base[mi];
    for (uint64_t i = 0; i < n; ++i) {
        std::memcpy(s->tris[tri_base + i].v, verts + 9 * (uint64_t)p.slot_src[i], 9 * sizeof(double));
        std::memcpy(s->normals[tri_base + i].n, norms + 9 * (uint64_t)p.slot_src[i], 9 * sizeof(double));
    }
    s->bases[mi].current = false;
    refit_host(s, mi, max_abs, val);
    return VR_OK;
}

// both trees, the root record and the scene scalars once the launches that write the mesh's records are
// queued on `st`; blocks until the scene is ready
int refit_device(vr_scene* s, uint32_t mi, const vr::refit::Validation& val, hipStream_t st) {
    const vr_scene::UpdatePlan& p = s->plans[mi];
    vr::TriVerts* tris = const_cast<vr::TriVerts*>(s->dev.tris);
    vr::Node* nodes = const_cast<vr::Node*>(s->dev.nodes);
    int e = vr::launch_refit_levels(nodes, nullptr, tris, p.d_items2, p.first2.data(), (uint32_t)p.first2.size() - 1, st);
    if (e) return device_fail(e, "scene update (binary refit)");
    if (!p.items4.empty()) {
        e = vr::launch_refit_levels(nullptr, const_cast<vr::Node4*>(s->dev.nodes4), tris, p.d_items4, p.first4.data(),
                                    (uint32_t)p.first4.size() - 1, st);
        if (e) return device_fail(e, "scene update (4-wide refit)");
    }
    const int bi = s->mesh_bvh[mi];
    if (bi >= 0) {
        vr::Bvh* rec = const_cast<vr::Bvh*>(s->dev.bvhs) + bi;
        e = vr::launch_refit_root(rec, nodes, tris, st);
        if (e) return device_fail(e, "scene update (root)");
        VR_HIP(hipMemcpyAsync(&s->bvhs[bi], rec, sizeof(vr::Bvh), hipMemcpyDeviceToHost, st));
    }
    VR_HIP(hipStreamSynchronize(st));
    if (!s->device_bvh) s->host_stale = true;
    double max_abs;
    std::memcpy(&max_abs, &val.max_abs, sizeof max_abs);
    s->mesh_extent[mi] = max_abs;
    s->mesh_finite[mi] = s->mesh_object[mi] < 0 || val.not_finite == 0;
    update_scalars(s);
    return VR_OK;
}

// ... and on the device; `device_arrays`: verts / norms are device pointers, else they are uploaded first
int update_mesh_device(vr_scene* s, uint32_t mi, uint64_t n, const double* verts, const double* norms,
                       bool device_arrays, hipStream_t st) {
    VR_HIP(hipSetDevice(s->device));
    vr_scene::UpdatePlan& p = s->plans[mi];
    if (const int rc = build_update_plan(s, mi)) return rc;
    const size_t row_bytes = (size_t)n * 9 * sizeof(double);
    if (!device_arrays) {
        if (p.stage_bytes < 2 * row_bytes) {
            if (p.d_stage) VR_HIP(hipFree(p.d_stage));
            s->device_bytes -= p.stage_bytes;
            p.d_stage = nullptr;
            p.stage_bytes = 0;
            VR_HIP(hipMalloc(&p.d_stage, 2 * row_bytes));
            p.stage_bytes = 2 * row_bytes;
            s->device_bytes += p.stage_bytes;
        }
        VR_HIP(hipMemcpyAsync(p.d_stage, verts, row_bytes, hipMemcpyHostToDevice, st));
        VR_HIP(hipMemcpyAsync((char*)p.d_stage + row_bytes, norms, row_bytes, hipMemcpyHostToDevice, st));
        verts = (const double*)p.d_stage;
        norms = (const double*)((const char*)p.d_stage + row_bytes);
    }
    // errors come before anything is modified: the reduction over the new arrays is read back first
    int e = vr::launch_refit_validate(verts, norms, n, p.d_valid, st);
    if (e) return device_fail(e, "scene update (validate)");
    vr::refit::Validation val{};
    VR_HIP(hipMemcpyAsync(&val, p.d_valid, sizeof val, hipMemcpyDeviceToHost, st));
    VR_HIP(hipStreamSynchronize(st));
    if (val.nonfinite) return fail(VR_ERROR_UNSUPPORTED, "scene update: a vertex coordinate is not finite");
    const int32_t tri_base = s->mesh_tri_base[mi];
    e = vr::launch_refit_gather(verts, norms, p.d_slot_src, n, const_cast<vr::TriVerts*>(s->dev.tris) + tri_base,
                                const_cast<vr::TriNormals*>(s->dev.normals) + tri_base, st);
    if (e) return device_fail(e, "scene update (gather)");
    const int rc = refit_device(s, mi, val, st);
    if (rc == VR_OK) s->bases[mi].current = false;
    return rc;
}

int update_mesh_checked(vr_scene* s, uint32_t mesh, uint64_t n, const double* verts, const double* norms,
                        bool device_arrays, void* stream) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if (mesh >= s->leaf_order.size()) return fail(VR_ERROR_INVALID_ARGUMENT, "scene update: bad mesh index");
    if (n != s->leaf_order[mesh].size())
        return fail(VR_ERROR_INVALID_ARGUMENT, "scene update: triangle_count differs from the mesh's");
    if (n && (!verts || !norms)) return fail(VR_ERROR_INVALID_ARGUMENT, "scene update: null vertex or normal array");
    if (device_arrays && s->host_only) return host_only_error();
    if (n == 0) return VR_OK;  // an empty mesh stays empty
    if (s->host_only) return update_mesh_host(s, mesh, n, verts, norms);
    return update_mesh_device(s, mesh, n, verts, norms, device_arrays, (hipStream_t)stream);
}

}  // namespace

int vr_scene_update_mesh(vr_scene* s, uint32_t mesh, uint64_t triangle_count, const double* vertices,
                         const double* normals) {
    return update_mesh_checked(s, mesh, triangle_count, vertices, normals, false, nullptr);
}

int vr_scene_update_mesh_device(vr_scene* s, uint32_t mesh, uint64_t triangle_count, const double* vertices,
                                const double* normals, void* stream) {
    return update_mesh_checked(s, mesh, triangle_count, vertices, normals, true, stream);
}

// ------------------------------------------------------------------------------------------
// Scene edits: camera, primitives, materials, lights, and a mesh's affine transform from its
// resident base geometry.  Each validates first, then changes the host records and copies the
// changed rows into the scene block (VR_SCENE_HOST_ONLY: host records only, no device call).
// ------------------------------------------------------------------------------------------
namespace {

// rows `first` .. of a device array of the scene block <- the host records (a host-only scene has no block)
int copy_rows(const vr_scene* s, const void* device_array, size_t row_bytes, size_t first, const void* src,
              size_t count) {
    if (s->host_only || count == 0) return VR_OK;
    VR_HIP(hipSetDevice(s->device));
    char* dst = (char*)const_cast<void*>(device_array) + first * row_bytes;
    VR_HIP(hipMemcpy(dst, src, count * row_bytes, hipMemcpyHostToDevice));
    return VR_OK;
}

// [A | t] and the cofactor matrix of A: K[i][j] = A[i+1][j+1] * A[i+2][j+2] - A[i+1][j+2] * A[i+2][j+1],
// indices mod 3, so that (A a) x (A b) = K (a x b)
vr::refit::Affine affine_of(const double m[12]) {
    vr::refit::Affine a;
    std::memcpy(a.m, m, sizeof a.m);
    auto A = [&](int i, int j) { return m[4 * (i % 3) + (j % 3)]; };
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a.k[3 * i + j] = A(i + 1, j + 1) * A(i + 2, j + 2) - A(i + 1, j + 2) * A(i + 2, j + 1);
    return a;
}

const char* kOverflow = "scene transform: a transformed vertex coordinate is not finite";

int transform_mesh_host(vr_scene* s, uint32_t mi, uint64_t n, const vr::refit::Affine& a) {
    vr_scene::MeshBase& b = s->bases[mi];
    const int32_t tri_base = s->mesh_tri_base[mi];
    if (!b.current) {
        b.tris.assign(s->tris.begin() + tri_base, s->tris.begin() + tri_base + n);
        b.normals.assign(s->normals.begin() + tri_base, s->normals.begin() + tri_base + n);
        b.current = true;
    }
    vr::refit::Validation val{};
    double max_abs = 0.0, v[9], nn[9];
    for (uint64_t i = 0; i < n; ++i) {
        vr::refit::transform_tri(a, b.tris[i].v, b.normals[i].n, v, nn);
        vr::refit::validate_tri(v, nn, val.nonfinite, max_abs, val.not_finite);
    }
    if (val.nonfinite) return fail(VR_ERROR_UNSUPPORTED, kOverflow);
    if (const int rc = build_update_plan(s, mi)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        vr::refit::transform_tri(a, b.tris[i].v, b.normals[i].n, s->tris[tri_base + i].v, s->normals[tri_base + i].n);
    refit_host(s, mi, max_abs, val);
    return VR_OK;
}

int transform_mesh_device(vr_scene* s, uint32_t mi, uint64_t n, const vr::refit::Affine& a, hipStream_t st) {
    VR_HIP(hipSetDevice(s->device));
    vr_scene::UpdatePlan& p = s->plans[mi];
    if (const int rc = build_update_plan(s, mi)) return rc;
    vr_scene::MeshBase& b = s->bases[mi];
    const size_t half = (size_t)n * sizeof(vr::TriVerts);
    static_assert(sizeof(vr::TriVerts) == sizeof(vr::TriNormals), "the base holds both arrays, one after the other");
    if (!b.d_base) {
        VR_HIP(hipMalloc(&b.d_base, 2 * half));
        s->device_bytes += 2 * half;
    }
    const int32_t tri_base = s->mesh_tri_base[mi];
    vr::TriVerts* tris = const_cast<vr::TriVerts*>(s->dev.tris) + tri_base;
    vr::TriNormals* normals = const_cast<vr::TriNormals*>(s->dev.normals) + tri_base;
    const vr::TriVerts* base_tris = (const vr::TriVerts*)b.d_base;
    const vr::TriNormals* base_normals = (const vr::TriNormals*)((const char*)b.d_base + half);
    if (!b.current) {
        VR_HIP(hipMemcpyAsync(b.d_base, tris, half, hipMemcpyDeviceToDevice, st));
        VR_HIP(hipMemcpyAsync((char*)b.d_base + half, normals, half, hipMemcpyDeviceToDevice, st));
    }
    // errors come before anything is modified: the reduction over the transformed base is read back first
    int e = vr::launch_transform_validate(base_tris, base_normals, n, a, p.d_valid, st);
    if (e) return device_fail(e, "scene transform (validate)");
    vr::refit::Validation val{};
    VR_HIP(hipMemcpyAsync(&val, p.d_valid, sizeof val, hipMemcpyDeviceToHost, st));
    VR_HIP(hipStreamSynchronize(st));
    b.current = true;  // the copy above has completed
    if (val.nonfinite) return fail(VR_ERROR_UNSUPPORTED, kOverflow);
    e = vr::launch_transform_write(base_tris, base_normals, n, a, tris, normals, st);
    if (e) return device_fail(e, "scene transform (write)");
    return refit_device(s, mi, val, st);
}

}  // namespace

int vr_scene_set_camera(vr_scene* s, vr_vec3 location) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if (!std::isfinite(location.x) || !std::isfinite(location.y) || !std::isfinite(location.z))
        return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: a camera coordinate is not finite");
    s->camera[0] = location.x;
    s->camera[1] = location.y;
    s->camera[2] = location.z;
    std::memcpy(s->dev.camera, s->camera, sizeof s->dev.camera);
    update_base_extent(s);
    update_scalars(s);
    return VR_OK;
}

namespace {

bool finite3(vr_vec3 v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); }
double dot3(vr_vec3 a, vr_vec3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
vr_vec3 cross3(vr_vec3 a, vr_vec3 b) {  // vec3.rs:84-89
    return vr_vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
vr_vec3 normalize3(vr_vec3 a) {
    const vr::camera::Vec n = vr::camera::normalize(vr::camera::Vec{a.x, a.y, a.z});
    return vr_vec3{n.x, n.y, n.z};
}
bool film_distance_ok(double f) { return f >= 1e-3 && f <= 1e3; }  // false for a NaN
// (what vr_scene_set_camera_pose admits: vrh::pose_error, vr_host.h)

}  // namespace

int vr_scene_set_camera_pose(vr_scene* s, const vr_camera_pose* pose) {
    if (!s || !pose) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or pose");
    if (const char* why = pose_error(*pose)) return fail(VR_ERROR_INVALID_ARGUMENT, why);
    vr::PoseArgs& d = s->pose;
    const vr_vec3 axes[3] = {pose->right, pose->up, pose->forward};
    double* dst[3] = {d.right, d.up, d.forward};
    for (int i = 0; i < 3; ++i) {  // stored and used as given
        dst[i][0] = axes[i].x;
        dst[i][1] = axes[i].y;
        dst[i][2] = axes[i].z;
    }
    d.film_distance = pose->film_distance;
    return vr_scene_set_camera(s, pose->location);  // cannot fail: the location is finite
}

int vr_scene_set_camera_lens(vr_scene* s, const vr_camera_lens* lens) {
    if (!s || !lens) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or lens");
    if (!std::isfinite(lens->lens_radius) || !std::isfinite(lens->focus_distance))
        return fail(VR_ERROR_INVALID_ARGUMENT, "camera lens: an entry is not finite");
    if (!(lens->lens_radius >= 0.0 && lens->lens_radius <= 1e3))
        return fail(VR_ERROR_INVALID_ARGUMENT, "camera lens: lens_radius outside [0, 1e3]");
    if (!(lens->focus_distance >= 1e-3 && lens->focus_distance <= 1e6))
        return fail(VR_ERROR_INVALID_ARGUMENT, "camera lens: focus_distance outside [1e-3, 1e6]");
    s->lens.lens_radius = lens->lens_radius;
    s->lens.focus_distance = lens->focus_distance;
    update_base_extent(s);  // the camera's part of the extent carries the radius
    update_scalars(s);
    return VR_OK;
}

int vr_camera_look_at(vr_vec3 eye, vr_vec3 target, vr_vec3 up_hint, double film_distance, vr_camera_pose* out) {
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "null pose");
    if (!finite3(eye) || !finite3(target) || !finite3(up_hint) || !std::isfinite(film_distance))
        return fail(VR_ERROR_INVALID_ARGUMENT, "look_at: an argument is not finite");
    if (!film_distance_ok(film_distance)) return fail(VR_ERROR_INVALID_ARGUMENT, "look_at: film_distance outside [1e-3, 1e3]");
    const vr_vec3 view{target.x - eye.x, target.y - eye.y, target.z - eye.z};
    if (!finite3(view)) return fail(VR_ERROR_INVALID_ARGUMENT, "look_at: target - eye is not finite");
    if (view.x == 0.0 && view.y == 0.0 && view.z == 0.0) return fail(VR_ERROR_INVALID_ARGUMENT, "look_at: eye == target");
    const vr_vec3 forward = normalize3(view);
    const vr_vec3 side = cross3(up_hint, forward);
    if (!finite3(forward) || !(dot3(side, side) > 1e-24 * dot3(up_hint, up_hint)))
        return fail(VR_ERROR_INVALID_ARGUMENT, "look_at: up_hint is parallel to the view direction");
    const vr_vec3 right = normalize3(side);
    const vr_vec3 up = cross3(forward, right);
    vr_camera_pose p{eye, right, up, forward, film_distance};
    if (pose_error(p)) return fail(VR_ERROR_INVALID_ARGUMENT, "look_at: the arguments' magnitudes leave no orthonormal basis");
    *out = p;
    return VR_OK;
}

int vr_camera_ray(const vr_camera_pose* pose, uint64_t width, uint64_t height, uint64_t row, uint64_t column, double ux,
                  double uy, double origin[3], double direction[3]) {
    if (!pose || !origin || !direction) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (width == 0 || height == 0 || row >= height || column >= width)
        return fail(VR_ERROR_INVALID_ARGUMENT, "camera ray: the pixel is outside the image");
    double film[4];
    vr::camera::film_constants(width, height, film);
    const double r[3] = {pose->right.x, pose->right.y, pose->right.z}, u[3] = {pose->up.x, pose->up.y, pose->up.z};
    const double f[3] = {pose->forward.x, pose->forward.y, pose->forward.z};
    const vr::camera::Vec d = vr::camera::ray_direction(r, u, f, pose->film_distance, vr::camera::film_x(film, column, ux),
                                                        vr::camera::film_y(film, height, row, uy));
    origin[0] = pose->location.x;
    origin[1] = pose->location.y;
    origin[2] = pose->location.z;
    direction[0] = d.x;
    direction[1] = d.y;
    direction[2] = d.z;
    return VR_OK;
}

int vr_scene_update_primitives(vr_scene* s, uint32_t first, uint32_t count, const vr_primitive_desc* prims) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if ((uint64_t)first + count > s->prim_rows.size())
        return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: primitive range past primitive_count");
    if (count == 0) return VR_OK;
    if (!prims) return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: null primitive array");
    for (uint32_t k = 0; k < count; ++k) {
        if (prims[k].kind != VR_PRIMITIVE_PLANE && prims[k].kind != VR_PRIMITIVE_SPHERE)
            return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: unknown primitive kind");
        if (prims[k].material >= s->desc_materials)
            return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: primitive material out of range");
    }
    uint32_t lo = UINT32_MAX, hi = 0;  // the rows that change
    for (uint32_t k = 0; k < count; ++k)
        for (uint32_t row : s->prim_rows[first + k]) {
            const vr::Prim old = s->prims[row];
            (void)prim_row(prims[k], old.object, old.position, s->prims[row]);  // the kind was checked above
            lo = std::min(lo, row);
            hi = std::max(hi, row);
        }
    update_base_extent(s);
    update_scalars(s);
    if (lo > hi) return VR_OK;  // entries that no list refers to
    return copy_rows(s, s->dev.prims, sizeof(vr::Prim), lo, &s->prims[lo], (size_t)(hi - lo + 1));
}

int vr_scene_update_material(vr_scene* s, uint32_t index, const vr_material_desc* material) {
    if (!s || !material) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or material");
    if (index >= s->desc_materials) return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: material index out of range");
    vr::Material row;
    if (const char* why = material_row(*material, row)) return fail(VR_ERROR_INVALID_ARGUMENT, why);
    s->materials[index] = row;
    update_material_scalars(s);
    update_grid_shared(s);
    update_scalars(s);
    return copy_rows(s, s->dev.materials, sizeof(vr::Material), index, &s->materials[index], 1);
}

int vr_scene_set_lights(vr_scene* s, const vr_integrator_desc* integrator) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    const int32_t kind = integrator ? integrator->kind : (int32_t)VR_INTEGRATOR_SIMPLE_RANDOM;
    if (kind != s->dev.integrator || (integrator && (int64_t)integrator->light_count != s->dev.light_count))
        return fail(VR_ERROR_INVALID_ARGUMENT, "scene edit: integrator kind or light_count differs from the scene's");
    if (kind != VR_INTEGRATOR_WHITTED) return VR_OK;
    std::vector<vr::Material> rows;
    std::vector<double> dirs;
    if (const char* why = light_rows(*integrator, rows, dirs)) return fail(VR_ERROR_INVALID_ARGUMENT, why);
    std::copy(rows.begin(), rows.end(), s->materials.begin() + s->dev.light_base);
    update_grid_shared(s);
    s->light_dirs = dirs;
    const int rc = copy_rows(s, s->dev.materials, sizeof(vr::Material), (size_t)s->dev.light_base, rows.data(), rows.size());
    return rc ? rc : copy_rows(s, s->dev.light_dirs, sizeof(double), 0, dirs.data(), dirs.size());
}

int vr_scene_transform_mesh(vr_scene* s, uint32_t mesh, const double matrix[12], void* stream) {
    if (!s || !matrix) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or matrix");
    if (mesh >= s->leaf_order.size()) return fail(VR_ERROR_INVALID_ARGUMENT, "scene transform: bad mesh index");
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(matrix[i]))
            return fail(VR_ERROR_INVALID_ARGUMENT, "scene transform: a matrix entry is not finite");
    const uint64_t n = s->leaf_order[mesh].size();
    if (n == 0) return VR_OK;  // an empty mesh stays empty
    const vr::refit::Affine a = affine_of(matrix);
    if (s->host_only) return transform_mesh_host(s, mesh, n, a);
    return transform_mesh_device(s, mesh, n, a, (hipStream_t)stream);
}


// ------------------------------------------------------------------------------------------
// Per-triangle materials: TriNormals::material1 of a mesh's slots (0: the mesh's own material,
// m + 1: material m), scattered through the update plan's slot -> input triangle table.  Nothing
// else of the scene changes; the transform's base copy, where one exists, takes the same values so
// that the next transform carries them.
// ------------------------------------------------------------------------------------------
namespace {

const char* kMaterialRange = "mesh materials: a material index is out of range";

// Bvh::own_materials of the mesh's root record (a mesh that backs no object has none, and no hit)
int set_materials_flag(vr_scene* s, uint32_t mi, bool on) {
    const int bi = s->mesh_bvh[mi];
    if (bi < 0) return VR_OK;
    s->bvhs[bi].own_materials = on ? 1 : 0;
    if (s->host_only) return VR_OK;
    char* field = (char*)(const_cast<vr::Bvh*>(s->dev.bvhs) + bi) + offsetof(vr::Bvh, own_materials);
    VR_HIP(hipMemcpy(field, &s->bvhs[bi].own_materials, sizeof(int32_t), hipMemcpyHostToDevice));
    return VR_OK;
}

void set_materials_records(vr_scene* s, uint32_t mi, uint64_t n, const uint32_t* mats) {
    const vr_scene::UpdatePlan& p = s->plans[mi];
    vr_scene::MeshBase& b = s->bases[mi];
    const int32_t tri_base = s->mesh_tri_base[mi];
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t own = mats ? (int64_t)mats[p.slot_src[i]] + 1 : 0;
        s->normals[tri_base + i].material1 = own;
        if (b.normals.size() == n) b.normals[i].material1 = own;
    }
}

int set_materials_device(vr_scene* s, uint32_t mi, uint64_t n, const uint32_t* mats, bool device_array, hipStream_t st) {
    VR_HIP(hipSetDevice(s->device));
    vr_scene::UpdatePlan& p = s->plans[mi];
    if (const int rc = build_update_plan(s, mi)) return rc;
    const uint32_t* d_mats = mats;
    if (mats && !device_array) {
        const size_t bytes = (size_t)n * sizeof(uint32_t);
        if (p.stage_bytes < bytes) {
            if (p.d_stage) VR_HIP(hipFree(p.d_stage));
            s->device_bytes -= p.stage_bytes;
            p.d_stage = nullptr;
            p.stage_bytes = 0;
            VR_HIP(hipMalloc(&p.d_stage, bytes));
            p.stage_bytes = bytes;
            s->device_bytes += p.stage_bytes;
        }
        VR_HIP(hipMemcpyAsync(p.d_stage, mats, bytes, hipMemcpyHostToDevice, st));
        d_mats = (const uint32_t*)p.d_stage;
    }
    if (d_mats) {  // errors come before anything is modified: the largest index is read back first
        const int e = vr::launch_materials_max(d_mats, n, p.d_valid, st);
        if (e) return device_fail(e, "mesh materials (validate)");
        unsigned long long largest = 0;
        VR_HIP(hipMemcpyAsync(&largest, p.d_valid, sizeof largest, hipMemcpyDeviceToHost, st));
        VR_HIP(hipStreamSynchronize(st));
        if (largest >= s->desc_materials) return fail(VR_ERROR_INVALID_ARGUMENT, kMaterialRange);
    }
    vr_scene::MeshBase& b = s->bases[mi];
    vr::TriNormals* base_normals = b.d_base ? (vr::TriNormals*)((char*)b.d_base + (size_t)n * sizeof(vr::TriVerts)) : nullptr;
    const int e = vr::launch_materials_scatter(d_mats, p.d_slot_src, n,
                                               const_cast<vr::TriNormals*>(s->dev.normals) + s->mesh_tri_base[mi],
                                               base_normals, st);
    if (e) return device_fail(e, "mesh materials (scatter)");
    VR_HIP(hipStreamSynchronize(st));
    // the host copy of a host-built scene follows where it is current and the values are at hand
    if (!s->device_bvh && !s->host_stale && !(mats && device_array))
        set_materials_records(s, mi, n, mats);
    else if (!s->device_bvh)
        s->host_stale = true;
    return set_materials_flag(s, mi, mats != nullptr);
}

int set_materials_checked(vr_scene* s, uint32_t mesh, uint64_t n, const uint32_t* mats, bool device_array, void* stream) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if (mesh >= s->leaf_order.size()) return fail(VR_ERROR_INVALID_ARGUMENT, "mesh materials: bad mesh index");
    if (n != s->leaf_order[mesh].size())
        return fail(VR_ERROR_INVALID_ARGUMENT, "mesh materials: triangle_count differs from the mesh's");
    if (device_array && s->host_only) return host_only_error();
    if (mats && !device_array)
        for (uint64_t t = 0; t < n; ++t)
            if (mats[t] >= s->desc_materials) return fail(VR_ERROR_INVALID_ARGUMENT, kMaterialRange);
    if (n == 0) return VR_OK;  // an empty mesh stays empty
    if (!s->host_only) return set_materials_device(s, mesh, n, mats, device_array, (hipStream_t)stream);
    if (const int rc = build_update_plan(s, mesh)) return rc;
    set_materials_records(s, mesh, n, mats);
    return set_materials_flag(s, mesh, mats != nullptr);
}

}  // namespace

int vr_scene_set_mesh_materials(vr_scene* s, uint32_t mesh, uint64_t triangle_count, const uint32_t* materials) {
    return set_materials_checked(s, mesh, triangle_count, materials, false, nullptr);
}

int vr_scene_set_mesh_materials_device(vr_scene* s, uint32_t mesh, uint64_t triangle_count, const uint32_t* materials_device,
                                       void* stream) {
    return set_materials_checked(s, mesh, triangle_count, materials_device, true, stream);
}
