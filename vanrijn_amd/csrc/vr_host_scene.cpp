// vr_host_scene.cpp -- the scene: its rows (materials, primitives, lights) and scalars, creation
// (copy, the host builders of vr_host_bvh.cpp or the device build, HBM upload) and the dump accessors.
//   Scene { camera_location, objects }            src/scene.rs:5-8
//   Plane::new                                    src/raycasting/plane.rs:18-31
#include "vr_host.h"

#include "rgb_spectrum_tables.h"

using namespace vrh;

namespace {

// Host math in the reference's operation order (Plane::new)
struct H3 {
    double x, y, z;
};
double hdot(H3 a, H3 b) {
    double s = -0.0;  // `Sum for f64` folds from -0.0 (vec3.rs:76-82)
    s = s + a.x * b.x;
    s = s + a.y * b.y;
    s = s + a.z * b.z;
    return s;
}
H3 hcross(H3 a, H3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
H3 hnormalize(H3 a) {
    double inv = 1.0 / std::sqrt(hdot(a, a));
    return {a.x * inv, a.y * inv, a.z * inv};
}

// Whether every hit on this mesh has a finite shading basis, whatever the barycentric point: the
// reference's normal = normalize(sum b_i N_i) (triangle.rs:73-78) is NaN where the interpolated
// normal is zero (mesh.rs:37 gives zero normals to an OBJ without them), and cotangent =
// normalize((V0 - V1) x n) is NaN where n is parallel to that edge.  Sufficient: all three vertex
// normals lie strictly on one side of the triangle's plane, by a relative margin of 1e-6 (then
// n . f >= 1e-6 |N|max |f| sum(b) - O(1e-16), so n is nonzero and not in the plane, where the edge
// lies), with magnitudes far from f64 under- / overflow.  Degenerate triangles fail.  (A sphere's
// basis is NaN only where a hit's x and y equal the centre's exactly, and a retro direction only
// where a hit lies exactly at the ray origin: exact-equality events of measure zero, not excluded.)
bool shading_finite(const vr_mesh_desc& m) {
    for (uint64_t t = 0; t < m.triangle_count; ++t) {
        const double* v = m.vertices + 9 * t;
        const double* nn = m.normals + 9 * t;
        for (int i = 0; i < 9; ++i)
            if (!std::isfinite(v[i]) || !std::isfinite(nn[i]) || std::fabs(v[i]) > 1e100 || std::fabs(nn[i]) > 1e100)
                return false;
        const double e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        const double f[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
        if (!(fl > 1e-200)) return false;
        double nmax = 0.0, d[3];
        for (int k = 0; k < 3; ++k) {
            const double* n = nn + 3 * k;
            nmax = std::max(nmax, std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]));
            d[k] = n[0] * f[0] + n[1] * f[1] + n[2] * f[2];
        }
        if (!(nmax > 1e-100)) return false;
        const double m6 = 1e-6 * nmax * fl;
        if (!((d[0] > m6 && d[1] > m6 && d[2] > m6) || (d[0] < -m6 && d[1] < -m6 && d[2] < -m6))) return false;
    }
    return true;
}

// spectrum.rs:64-79's sample wavelengths as the reference computes them (before / after), and the
// reciprocal step for the device's segment index (intensity only: a neighbouring segment at a knot
// gives the same value to rounding)
void fill_knots(vr::Material& m) {
    const double range = m.longest - m.shortest;
    for (int j = 0; j < m.n; ++j) m.knots[j] = (double)j / (double)(m.n - 1) * range + m.shortest;
    m.inv_step = m.n > 1 && range > 0.0 ? (double)(m.n - 1) / range : 0.0;
}

// The rows of the scene block that vr_scene_create and the scene edits both make: one definition
// each, so an edited scene holds a fresh scene's bits.  Each returns a message on a bad description.
const char* spectrum_row(const vr_spectrum& sp, vr::Material& dm) {
    if (sp.sample_count < 1 || sp.sample_count > VR_MAX_SPECTRUM_SAMPLES || !sp.samples)
        return "spectrum needs 1..64 samples";
    dm = vr::Material{};
    dm.n = (int32_t)sp.sample_count;
    dm.shortest = sp.shortest_wavelength;
    dm.longest = sp.longest_wavelength;
    std::memcpy(dm.samples, sp.samples, sizeof(double) * sp.sample_count);
    fill_knots(dm);
    return nullptr;
}

}  // namespace

namespace vrh {

const char* material_row(const vr_material_desc& m, vr::Material& dm) {
    if (m.kind < VR_MATERIAL_LAMBERTIAN || m.kind > VR_MATERIAL_DIELECTRIC) return "unknown material kind";
    if (spectrum_row(m.colour, dm)) return "material spectrum needs 1..64 samples";
    dm.kind = m.kind;
    dm.diffuse = m.diffuse_strength;
    dm.reflection = m.reflection_strength;
    dm.smoothness = m.smoothness;
    return nullptr;
}

// the Whitted rows: ambient, then one per light; dirs: 3 per light, stored as given
const char* light_rows(const vr_integrator_desc& ig, std::vector<vr::Material>& rows, std::vector<double>& dirs) {
    if (ig.light_count > VR_MAX_LIGHTS || (ig.light_count && !ig.lights)) return "bad light list";
    vr::Material dm;
    if (spectrum_row(ig.ambient_light, dm)) return "ambient light spectrum needs 1..64 samples";
    rows.push_back(dm);
    for (uint32_t j = 0; j < ig.light_count; ++j) {
        if (spectrum_row(ig.lights[j].spectrum, dm)) return "light spectrum needs 1..64 samples";
        rows.push_back(dm);
        const vr_vec3& d = ig.lights[j].direction;
        dirs.insert(dirs.end(), {d.x, d.y, d.z});
    }
    return nullptr;
}

// entry `p` of vr_scene_desc::primitives as the row at `position` of the list of scene object `object`
const char* prim_row(const vr_primitive_desc& p, int32_t object, int32_t position, vr::Prim& dp) {
    dp = vr::Prim{};
    dp.kind = p.kind;
    dp.material = (int32_t)p.material;
    dp.object = object;
    dp.position = position;
    dp.scalar = p.scalar;
    if (p.kind == VR_PRIMITIVE_PLANE) {
        // Plane::new (plane.rs:18-31)
        H3 n = hnormalize({p.vector.x, p.vector.y, p.vector.z});
        double ax = std::fabs(n.x), ay = std::fabs(n.y), az = std::fabs(n.z);
        int k2 = ax < ay ? (ax < az ? 0 : 2) : (ay < az ? 1 : 2);  // smallest_coord
        H3 axis{k2 == 0 ? 1.0 : 0.0, k2 == 1 ? 1.0 : 0.0, k2 == 2 ? 1.0 : 0.0};
        H3 cot = hnormalize(hcross(n, axis));
        H3 tan = hcross(n, cot);
        dp.vec[0] = n.x; dp.vec[1] = n.y; dp.vec[2] = n.z;
        dp.tan[0] = tan.x; dp.tan[1] = tan.y; dp.tan[2] = tan.z;
        dp.cot[0] = cot.x; dp.cot[1] = cot.y; dp.cot[2] = cot.z;
        dp.pre[0] = n.x * p.scalar; dp.pre[1] = n.y * p.scalar; dp.pre[2] = n.z * p.scalar;
    } else if (p.kind == VR_PRIMITIVE_SPHERE) {
        dp.vec[0] = p.vector.x; dp.vec[1] = p.vector.y; dp.vec[2] = p.vector.z;
        dp.pre[0] = p.vector.x * p.vector.x;
        dp.pre[1] = p.vector.y * p.vector.y;
        dp.pre[2] = p.vector.z * p.vector.z;
        dp.scalar2 = p.scalar * p.scalar;
    } else {
        return "unknown primitive kind";
    }
    return nullptr;
}

// The scene scalars that depend on mesh geometry, from their per-mesh parts: at creation, and again
// after vr_scene_update_mesh replaced one mesh's part -- so an updated scene holds a fresh scene's values.
// base_extent: the camera's and every primitive row's share of the extent (a row keeps the entry's
// scalar, and a sphere's centre, as given)
void update_base_extent(vr_scene* s) {
    // the camera's part: every point of the lens disc is within lens_radius of the location
    double extent =
        std::max({std::fabs(s->camera[0]), std::fabs(s->camera[1]), std::fabs(s->camera[2])}) + s->lens.lens_radius;
    for (const vr::Prim& p : s->prims) {
        if (p.kind == VR_PRIMITIVE_PLANE)
            extent = std::max(extent, std::fabs(p.scalar));
        else
            extent = std::max({extent, std::fabs(p.vec[0]) + std::fabs(p.scalar), std::fabs(p.vec[1]) + std::fabs(p.scalar),
                               std::fabs(p.vec[2]) + std::fabs(p.scalar)});
    }
    s->base_extent = extent;
}

// mats and dark0's materials-only part, over the desc's materials (not the light and sky rows)
void update_material_scalars(vr_scene* s) {
    s->mats = 0;
    s->dark0_materials = true;
    for (uint32_t i = 0; i < s->desc_materials; ++i) {
        const vr::Material& m = s->materials[i];
        const vr_spectrum colour{m.shortest, m.longest, (uint32_t)m.n, m.samples};
        if (vr_spectrum_intensity_at_wavelength(&colour, 0.0) != 0.0) s->dark0_materials = false;
        s->mats |= m.kind == VR_MATERIAL_LAMBERTIAN ? 1 : (m.kind == VR_MATERIAL_REFLECTIVE ? 2 : 4);
        // the dielectric's strength at 0 nm is not its eta(0): a path cut at the recursion limit
        // (lambda 0) needs the general lambda-0 chain
        if (m.kind == VR_MATERIAL_DIELECTRIC) s->dark0_materials = false;
    }
}

// The wavelength grid of a row is what the device's intensity lookup reads beside the samples:
// shortest, longest, n, inv_step and knots[0..n).  True when every row's equals the first row's bit
// for bit (compared as bytes: -0.0 is not 0.0, a NaN equals only itself).
bool grids_shared(const vr::Material* rows, size_t count) {
    for (size_t i = 1; i < count; ++i) {
        const vr::Material &a = rows[0], &b = rows[i];
        if (a.n != b.n || a.n < 0 || a.n > vr::kMaxSpectrumSamples) return false;
        if (std::memcmp(&a.shortest, &b.shortest, sizeof(double)) || std::memcmp(&a.longest, &b.longest, sizeof(double)) ||
            std::memcmp(&a.inv_step, &b.inv_step, sizeof(double)) ||
            std::memcmp(a.knots, b.knots, sizeof(double) * (size_t)a.n))
            return false;
    }
    return true;
}

// At creation and after every edit that writes a material or light row (nothing writes the sky row, the
// last one).  The render kernels that find a path's segment and ratio once, on row 0's grid, run only
// while the material and light rows share it (vr_host.cpp launch_choice); a sky row on another grid --
// a scene of two-sample grey materials, say -- keeps its own lookup there (RenderArgs::sky_on_grid).
void update_grid_shared(vr_scene* s) {
    s->grid_shared = grids_shared(s->materials.data(), (size_t)s->dev.sky_row);
    s->sky_on_grid = s->grid_shared && grids_shared(s->materials.data(), s->materials.size());
}

void update_scalars(vr_scene* s) {
    double extent = s->base_extent;
    for (double e : s->mesh_extent) extent = std::max(extent, e);
    s->extent = extent;
    s->dev.margin = 1e-9 * (extent + 1.0);
    s->dev.behind_margin = 1e-6 * (extent + 1.0);
    s->dev.extent = extent;
    // NaN-capable continuations (shading_finite): no early stop, the general lambda-0 chain
    s->nan_free = (s->mats & 4) == 0;
    for (uint8_t f : s->mesh_finite)
        if (!f) s->nan_free = false;
    s->dark0 = s->dark0_materials && s->nan_free;
}

}  // namespace vrh

namespace {

// the render kernel's 4-wide tree over every traversed mesh's binary tree `nodes`
void collapse_scene(vr_scene* s, const std::vector<vr::Node>& nodes) {
    WideTree w = collapse_wide(nodes, s->bvhs, s->greedy_collapse);
    s->nodes4 = std::move(w.nodes4);
    for (size_t i = 0; i < s->bvhs.size(); ++i) s->bvhs[i].root4 = w.roots[i];
    s->wide_stack = w.stack;
    s->wide_count = s->nodes4.size();
}

int upload(vr_scene* s) {
    VR_HIP(hipSetDevice(s->device));
    const size_t sz_nodes = s->node_count * sizeof(vr::Node);
    // the 4-wide tree has at most one node per binary interior node (device builds collapse after
    // the build, so its arrays are sized by that bound)
    const size_t sz_nodes4 = s->node_count * sizeof(vr::Node4);
    const size_t sz_tris = s->tri_count * sizeof(vr::TriVerts);
    const size_t sz_norm = s->tri_count * sizeof(vr::TriNormals);
    const size_t sz_mat = s->materials.size() * sizeof(vr::Material);
    const size_t sz_prim = s->prims.size() * sizeof(vr::Prim);
    const size_t sz_bvh = s->bvhs.size() * sizeof(vr::Bvh);
    size_t off[8], total = 0;
    const size_t sz_misc = 64 + vr::kCntCount * sizeof(unsigned long long);  // error flag, counters
    const size_t sizes[8] = {sz_nodes, sz_tris, sz_norm, sz_mat, sz_prim, sz_bvh,
                             sz_misc + 3 * VR_MAX_LIGHTS * sizeof(double), sz_nodes4};
    for (int i = 0; i < 8; ++i) {
        off[i] = total;
        total += (std::max<size_t>(sizes[i], 1) + 255) & ~size_t(255);
    }
    VR_HIP(hipMalloc(&s->d_block, total));
    s->device_bytes = total;
    VR_HIP(hipDeviceGetAttribute(&s->cu_count, hipDeviceAttributeMultiprocessorCount, s->device));
    char* base = (char*)s->d_block;
    const void* src[6] = {s->nodes.data(), s->tris.data(), s->normals.data(), s->materials.data(), s->prims.data(),
                          s->bvhs.data()};
    for (int i = 0; i < 6; ++i) {
        if (s->device_bvh && (i < 3 || i == 5)) continue;  // filled by the device build below
        if (sizes[i]) VR_HIP(hipMemcpy(base + off[i], src[i], sizes[i], hipMemcpyHostToDevice));
    }
    VR_HIP(hipMemset(base + off[6], 0, sizes[6]));
    s->d_counters = (unsigned long long*)(base + off[6] + 64);
    s->dev.light_dirs = (const double*)(base + off[6] + sz_misc);
    if (!s->light_dirs.empty())
        VR_HIP(hipMemcpy(base + off[6] + sz_misc, s->light_dirs.data(), s->light_dirs.size() * sizeof(double),
                         hipMemcpyHostToDevice));
    vr::DeviceScene& d = s->dev;
    d.nodes = (const vr::Node*)(base + off[0]);
    d.nodes4 = (const vr::Node4*)(base + off[7]);
    d.tris = (const vr::TriVerts*)(base + off[1]);
    d.normals = (const vr::TriNormals*)(base + off[2]);
    d.materials = (const vr::Material*)(base + off[3]);
    d.prims = (const vr::Prim*)(base + off[4]);
    d.bvhs = (const vr::Bvh*)(base + off[5]);
    if (s->device_bvh) {
        // BoundingVolumeHierarchy::build on the device (vr_build.hip): same nodes, same leaf order
        CallScratch cs;
        VR_HIP(hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking));
        vr::Node* nodes = (vr::Node*)(base + off[0]);
        for (const auto& pm : s->pending) {
            double root_box[6];
            int levels = 0;
            const int e = vr::device_build_bvh(pm.vertices, pm.normals, (uint32_t)pm.n, pm.node_base, pm.tri_base,
                                               nodes + pm.node_base, (vr::TriVerts*)(base + off[1]) + pm.tri_base,
                                               (vr::TriNormals*)(base + off[2]) + pm.tri_base,
                                               s->leaf_order[pm.mesh].data(), root_box, &levels, cs.stream);
            if (e) return device_fail(e, "device BVH build failed");
            s->max_depth = std::max(s->max_depth, levels);
        }
        VR_HIP(hipStreamSynchronize(cs.stream));
        if (s->device_sah && s->device_bvh) {
            // the SAH traversal tree over the ranked triangles (replaces the median tree in the
            // binary array; the triangles move into its leaf order), then the 4-wide collapse on
            // the host's binary copy (collapse_wide: depth-first layout, as the host-built scene)
            for (const auto& pm : s->pending) {
                if (pm.n < 2) continue;
                double root_box[6];
                int levels = 0;
                const int e = vr::device_build_sah((vr::TriVerts*)(base + off[1]) + pm.tri_base,
                                                   (vr::TriNormals*)(base + off[2]) + pm.tri_base, (uint32_t)pm.n,
                                                   pm.node_base, pm.tri_base, nodes + pm.node_base, root_box, &levels,
                                                   cs.stream);
                if (e) return device_fail(e, "device SAH build failed");
                s->max_depth = std::max(s->max_depth, levels);
            }
            s->nodes.resize(s->node_count);
            if (s->node_count)
                VR_HIP(hipMemcpy(s->nodes.data(), nodes, s->node_count * sizeof(vr::Node), hipMemcpyDeviceToHost));
            collapse_scene(s, s->nodes);
            s->nodes.clear();
            s->nodes.shrink_to_fit();
        } else {
            // the 4-wide traversal tree: planned from the meshes' sizes (shape_wide), boxes gathered on
            // the device
            std::vector<int32_t> desc;
            for (const auto& pm : s->pending) {
                if (pm.n < 2) continue;  // one-triangle mesh: its root is the leaf
                const int32_t root = shape_wide(pm.n, pm.node_base, pm.tri_base, desc, s->wide_stack);
                s->mesh_root4[pm.mesh] = root;
                for (auto& b : s->bvhs)
                    if (b.tri_base == pm.tri_base && b.root == pm.node_base) b.root4 = root;
            }
            for (auto& b : s->bvhs)
                if (b.root < 0) b.root4 = b.root;
            s->wide_count = desc.size() / 8;
            if (s->wide_count) {
                int32_t* d_desc = nullptr;
                VR_HIP(hipMalloc(&d_desc, desc.size() * sizeof(int32_t)));
                const hipError_t ec = hipMemcpy(d_desc, desc.data(), desc.size() * sizeof(int32_t), hipMemcpyHostToDevice);
                const int e = ec != hipSuccess ? (int)ec
                                               : vr::device_fill_wide(nodes, d_desc, s->wide_count, (vr::Node4*)(base + off[7]),
                                                                      cs.stream);
                const hipError_t es = hipStreamSynchronize(cs.stream);
                (void)hipFree(d_desc);
                if (e || es != hipSuccess) return fail(VR_ERROR_DEVICE, "device wide-tree fill failed");
            }
        }
        s->pending.clear();  // the caller's arrays are not kept
        if (sz_bvh) VR_HIP(hipMemcpy(base + off[5], s->bvhs.data(), sz_bvh, hipMemcpyHostToDevice));
    }
    if (!s->nodes4.empty())
        VR_HIP(hipMemcpy(base + off[7], s->nodes4.data(), s->nodes4.size() * sizeof(vr::Node4), hipMemcpyHostToDevice));
    if (s->device_bvh) {  // a device-built scene keeps no host copy of its trees
        s->nodes4.clear();
        s->nodes4.shrink_to_fit();
    }
    return VR_OK;
}

// whether the host vectors (nodes, nodes4, tris, normals) hold the scene's current state
bool host_copies_current(const vr_scene* s) { return s->host_only || (!s->device_bvh && !s->host_stale); }

// rows of the scene block for an inspector: the host records where they are current, else read back
int dump_rows(const vr_scene* s, bool host_current, const void* device_src, const void* host_src, size_t bytes, void* out) {
    if (bytes == 0 || !out) return VR_OK;
    if (host_current) {
        std::memcpy(out, host_src, bytes);
        return VR_OK;
    }
    VR_HIP(hipSetDevice(s->device));
    VR_HIP(hipMemcpy(out, device_src, bytes, hipMemcpyDeviceToHost));
    return VR_OK;
}

}  // namespace

int vr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vr_scene_create(const vr_scene_desc* desc, int32_t device, uint32_t flags, vr_scene** out) {
    if (!desc || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null desc or out");
    *out = nullptr;
    vr_scene* s = new (std::nothrow) vr_scene();
    if (!s) return fail(VR_ERROR_OUT_OF_MEMORY, "scene allocation failed");
    s->device = device;
    s->host_only = (flags & VR_SCENE_HOST_ONLY) != 0;
    s->greedy_collapse = (flags & VR_SCENE_GREEDY_COLLAPSE) != 0;
    s->force_big = (flags & VR_SCENE_WIDE_OFFSETS) != 0;
    s->camera[0] = desc->camera_location.x;
    s->camera[1] = desc->camera_location.y;
    s->camera[2] = desc->camera_location.z;
    auto bad = [&](const std::string& m) {
        delete s;
        return fail(VR_ERROR_INVALID_ARGUMENT, m);
    };

    for (uint32_t i = 0; i < desc->material_count; ++i) {
        vr::Material dm;
        if (const char* why = material_row(desc->materials[i], dm)) return bad(why);
        s->materials.push_back(dm);
    }
    s->desc_materials = desc->material_count;
    update_material_scalars(s);
    // integrator: Whitted's ambient and light spectra become extra material rows
    if (desc->integrator && desc->integrator->kind == VR_INTEGRATOR_WHITTED) {
        const vr_integrator_desc& ig = *desc->integrator;
        s->dev.integrator = VR_INTEGRATOR_WHITTED;
        s->dev.light_base = (int32_t)s->materials.size();
        s->dev.light_count = (int32_t)ig.light_count;
        if (const char* why = light_rows(ig, s->materials, s->light_dirs)) return bad(why);
    } else if (desc->integrator && desc->integrator->kind != VR_INTEGRATOR_SIMPLE_RANDOM) {
        return bad("unknown integrator kind");
    }
    {  // the sky's lookup row (test_lighting_environment's RGB-basis spectrum: 32 samples)
        vr::Material sky{};
        sky.n = 32;
        sky.shortest = VR_RGBSPEC_SHORTEST;
        sky.longest = VR_RGBSPEC_LONGEST;
        fill_knots(sky);
        s->dev.sky_row = (int32_t)s->materials.size();
        s->materials.push_back(sky);
    }
    update_grid_shared(s);
    // objects: primitive lists keep their order; BVHs are built per mesh
    std::vector<int> mesh_object(desc->mesh_count, -1);
    s->prim_rows.resize(desc->primitive_count);
    for (uint32_t oi = 0; oi < desc->object_count; ++oi) {
        const vr_object_desc& o = desc->objects[oi];
        if (o.kind == VR_OBJECT_PRIMITIVE_LIST) {
            if ((uint64_t)o.first + o.count > desc->primitive_count) return bad("primitive list out of range");
            for (uint32_t k = 0; k < o.count; ++k) {
                const vr_primitive_desc& p = desc->primitives[o.first + k];
                if (p.material >= desc->material_count) return bad("primitive material out of range");
                vr::Prim dp;
                if (const char* why = prim_row(p, (int32_t)oi, (int32_t)k, dp)) return bad(why);
                s->prim_rows[o.first + k].push_back((uint32_t)s->prims.size());
                s->prims.push_back(dp);
            }
        } else if (o.kind == VR_OBJECT_BVH) {
            if (o.first >= desc->mesh_count) return bad("BVH object mesh out of range");
            if (mesh_object[o.first] >= 0) return bad("a mesh can back only one BVH object");
            mesh_object[o.first] = (int)oi;
        } else {
            return bad("unknown object kind");
        }
    }
    s->object_count = desc->object_count;
    // NaN-capable continuations (shading_finite): no early stop, the general lambda-0 chain
    // (one result per mesh, every mesh evaluated: vr_scene_update_mesh replaces one of them)
    s->mesh_finite.assign(desc->mesh_count, 1);
    for (uint32_t mi = 0; mi < desc->mesh_count; ++mi) {
        const vr_mesh_desc& m = desc->meshes[mi];
        if (mesh_object[mi] >= 0 && m.triangle_count && m.vertices && m.normals && !shading_finite(m))
            s->mesh_finite[mi] = 0;
    }
    update_base_extent(s);
    s->mesh_extent.assign(desc->mesh_count, 0.0);
    s->mesh_object = mesh_object;
    s->mesh_bvh.assign(desc->mesh_count, -1);
    s->mesh_node_base.assign(desc->mesh_count, 0);
    s->mesh_root4.assign(desc->mesh_count, vr::kEmptyChild);
    s->plans.resize(desc->mesh_count);
    s->bases.resize(desc->mesh_count);
    s->leaf_order.resize(desc->mesh_count);
    s->mesh_tri_base.assign(desc->mesh_count, 0);
    // device build: requested, a device exists for it, and no NaN coordinate (the reference's
    // sort comparator maps NaN to Equal, which only the host build reproduces)
    s->device_bvh = (flags & (VR_SCENE_DEVICE_BVH | VR_SCENE_DEVICE_SAH)) != 0 && !s->host_only;
    s->device_sah = (flags & VR_SCENE_DEVICE_SAH) != 0 && (flags & VR_SCENE_REFERENCE_BVH) == 0;
    // traversal tree: SAH (default) or the reference's own median-split tree
    const bool sah = (flags & VR_SCENE_REFERENCE_BVH) == 0 && !s->device_bvh;
    for (uint32_t mi = 0; s->device_bvh && mi < desc->mesh_count; ++mi) {
        const vr_mesh_desc& m = desc->meshes[mi];
        if (m.triangle_count && !m.vertices) break;
        for (uint64_t i = 0; i < 9 * m.triangle_count; ++i)
            if (m.vertices[i] != m.vertices[i]) {
                s->device_bvh = false;
                break;
            }
    }
    for (uint32_t mi = 0; mi < desc->mesh_count; ++mi) {
        const vr_mesh_desc& m = desc->meshes[mi];
        const uint64_t n = m.triangle_count;
        if (n && (!m.vertices || !m.normals)) return bad("mesh without vertex or normal arrays");
        if (m.material >= desc->material_count) return bad("mesh material out of range");
        if (s->tri_count + n > (uint64_t)INT32_MAX) return bad("too many triangles (2^31)");
        vr::Bvh bvh{};
        bvh.object = mesh_object[mi];
        bvh.tri_base = (int32_t)s->tri_count;
        bvh.material = (int32_t)m.material;
        s->mesh_tri_base[mi] = bvh.tri_base;
        s->mesh_material.push_back(m.material);
        s->mesh_node_base[mi] = (int32_t)s->node_count;
        if (s->device_bvh) {
            // shape and root box on the host (O(n)); the sort-based build runs after upload
            mesh_bounds(m.vertices, n, bvh.root_box, &s->mesh_extent[mi]);
            bvh.root = n > 1 ? (int32_t)s->node_count : (n ? ~bvh.tri_base : INT32_MIN);
            if (n) {
                s->pending.push_back({m.vertices, m.normals, n, (int32_t)s->node_count, bvh.tri_base, mi});
                s->max_depth = std::max(s->max_depth, 1);
            }
            s->leaf_order[mi].assign(n, 0);
            s->node_count += n ? n - 1 : 0;
            s->tri_count += n;
        } else {
            MeshTree t = build_mesh_tree(m.vertices, n, bvh.tri_base, (int32_t)s->node_count, sah);
            s->mesh_extent[mi] = t.extent;
            std::memcpy(bvh.root_box, t.root_box, sizeof bvh.root_box);
            bvh.root = t.root;
            s->nodes.insert(s->nodes.end(), t.nodes.begin(), t.nodes.end());
            s->max_depth = std::max(s->max_depth, t.depth);
            for (uint64_t i = 0; i < n; ++i) {
                const uint64_t r = t.rank[i];  // reference leaf position of traversal leaf i
                vr::TriVerts tv{};
                vr::TriNormals tn{};
                std::memcpy(tv.v, m.vertices + 9 * t.order[r], 9 * sizeof(double));
                std::memcpy(tn.n, m.normals + 9 * t.order[r], 9 * sizeof(double));
                tv.rank = (int64_t)bvh.tri_base + (int64_t)r;
                s->tris.push_back(tv);
                s->normals.push_back(tn);
            }
            s->leaf_order[mi] = std::move(t.order);
            s->node_count = s->nodes.size();
            s->tri_count = s->tris.size();
        }
        if (mesh_object[mi] >= 0) s->bvhs.push_back(bvh);
    }
    // outward-rounded f32 root boxes (the kernel's pre-test)
    for (auto& b : s->bvhs)
        for (int k = 0; k < 6; ++k) b.root_box32[k] = (k % 2 == 0) ? round_lower(b.root_box[k]) : round_upper(b.root_box[k]);
    // BVH objects in object order (ties across objects depend on it)
    std::sort(s->bvhs.begin(), s->bvhs.end(), [](const vr::Bvh& a, const vr::Bvh& b) { return a.object < b.object; });
    // the render kernel's 4-wide tree (device builds: after the build, in upload)
    if (!s->device_bvh) collapse_scene(s, s->nodes);
    vr::DeviceScene& d = s->dev;
    d.prim_count = (int32_t)s->prims.size();
    d.bvh_count = (int32_t)s->bvhs.size();
    std::memcpy(d.camera, s->camera, sizeof d.camera);
    update_scalars(s);  // extent and the margins, NAN_FREE, dark0
    if (!s->host_only) {
        int rc = upload(s);
        if (rc != VR_OK) {
            const std::string msg = vr_last_error();
            vr_scene_destroy(s);
            return fail(rc, msg);
        }
    }
    for (uint32_t mi = 0; mi < desc->mesh_count; ++mi)
        for (size_t bi = 0; bi < s->bvhs.size(); ++bi)
            if (mesh_object[mi] >= 0 && s->bvhs[bi].object == mesh_object[mi]) {
                s->mesh_bvh[mi] = (int)bi;
                s->mesh_root4[mi] = s->bvhs[bi].root4 >= 0 ? s->bvhs[bi].root4 : vr::kEmptyChild;
            }
    *out = s;
    return VR_OK;
}

void vr_scene_destroy(vr_scene* s) {
    if (!s) return;
    if (s->d_block || !s->ctx_all.empty() || !s->stream_slots.empty()) {
        (void)hipSetDevice(s->device);
        for (CallCtx* c : s->ctx_all) ctx_free_all(c);  // waits for each context's last work
        // (the streams may be gone by now: hipFree waits for the device instead)
        for (auto& kv : s->stream_slots) (void)hipFree(kv.second);
        for (auto& p : s->plans) {
            if (p.d_plan) (void)hipFree(p.d_plan);
            if (p.d_stage) (void)hipFree(p.d_stage);
        }
        for (auto& b : s->bases)
            if (b.d_base) (void)hipFree(b.d_base);
        if (s->d_block) (void)hipFree(s->d_block);
    }
    for (auto& kv : s->deferred)
        for (hipEvent_t e : kv.second.ev) (void)hipEventDestroy(e);
    delete s;
}

int vr_scene_get_info(const vr_scene* s, vr_scene_info* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    out->triangle_count = s->tri_count;
    out->node_count = s->node_count;
    out->max_bvh_depth = (uint32_t)s->max_depth;
    out->object_count = s->object_count;
    out->extent = s->extent;
    out->device_bytes = s->device_bytes;
    out->wide_node_count = s->wide_count;
    out->traversal_stack = (uint32_t)s->wide_stack;
    out->flags = s->nan_free ? VR_SCENE_INFO_NAN_FREE : 0u;
    return VR_OK;
}

int vr_scene_set_staging_limit(vr_scene* s, uint64_t bytes) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    s->staging_limit = bytes;
    return VR_OK;
}

int vr_debug_set_fault_object(vr_scene* s, int32_t object) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    s->fault_object = object < 0 ? -1 : object;
    return VR_OK;
}

int vr_debug_set_launch_flags(vr_scene* s, uint32_t flags) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    const uint32_t allowed =
        VR_LAUNCH_NO_CULL | VR_LAUNCH_NO_DIST_CULL | VR_LAUNCH_NO_COOP | VR_LAUNCH_NO_LONE_WALK | VR_LAUNCH_STACK32 |
        VR_LAUNCH_MULTI_BVH;
    if (flags & ~allowed)
        return fail(VR_ERROR_INVALID_ARGUMENT,
                    "only NO_CULL / NO_DIST_CULL / NO_COOP / NO_LONE_WALK / STACK32 / MULTI_BVH apply to every call");
    s->debug_launch_flags = flags;
    return VR_OK;
}

int vr_scene_bvh_nodes(const vr_scene* s, void* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    return dump_rows(s, !s->device_bvh && !s->host_stale, s->dev.nodes, s->nodes.data(), s->node_count * sizeof(vr::Node), out);
}

int vr_scene_bvh_leaf_order(const vr_scene* s, uint32_t mesh, uint64_t* out) {
    if (!s || !out || mesh >= s->leaf_order.size()) return fail(VR_ERROR_INVALID_ARGUMENT, "bad mesh index");
    std::memcpy(out, s->leaf_order[mesh].data(), sizeof(uint64_t) * s->leaf_order[mesh].size());
    return VR_OK;
}

int vr_scene_primitives(const vr_scene* s, void* out, uint32_t* count) {
    if (!s || (!out && !count)) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (count) *count = (uint32_t)s->prims.size();
    return out ? dump_rows(s, s->host_only, s->dev.prims, s->prims.data(), s->prims.size() * sizeof(vr::Prim), out) : VR_OK;
}

int vr_scene_materials(const vr_scene* s, void* out, uint32_t* count) {
    if (!s || (!out && !count)) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (count) *count = (uint32_t)s->materials.size();
    return out ? dump_rows(s, s->host_only, s->dev.materials, s->materials.data(), s->materials.size() * sizeof(vr::Material), out) : VR_OK;
}

int vr_scene_get_camera(const vr_scene* s, vr_vec3* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    *out = vr_vec3{s->camera[0], s->camera[1], s->camera[2]};
    return VR_OK;
}

int vr_scene_get_camera_pose(const vr_scene* s, vr_camera_pose* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    const vr::PoseArgs& d = s->pose;
    out->location = vr_vec3{s->camera[0], s->camera[1], s->camera[2]};
    out->right = vr_vec3{d.right[0], d.right[1], d.right[2]};
    out->up = vr_vec3{d.up[0], d.up[1], d.up[2]};
    out->forward = vr_vec3{d.forward[0], d.forward[1], d.forward[2]};
    out->film_distance = d.film_distance;
    return VR_OK;
}

int vr_scene_get_camera_lens(const vr_scene* s, vr_camera_lens* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    out->lens_radius = s->lens.lens_radius;
    out->focus_distance = s->lens.focus_distance;
    return VR_OK;
}

int vr_scene_wide_nodes(const vr_scene* s, void* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    return dump_rows(s, host_copies_current(s), s->dev.nodes4, s->nodes4.data(), s->wide_count * sizeof(vr::Node4), out);
}

int vr_scene_triangles(const vr_scene* s, void* out_verts, void* out_normals) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    const size_t bytes = s->tri_count * sizeof(vr::TriVerts);
    const int rc = dump_rows(s, host_copies_current(s), s->dev.tris, s->tris.data(), bytes, out_verts);
    return rc ? rc : dump_rows(s, host_copies_current(s), s->dev.normals, s->normals.data(), bytes, out_normals);
}

int vr_scene_mesh_materials(const vr_scene* s, uint32_t mesh, uint32_t* out) {
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if (mesh >= s->leaf_order.size()) return fail(VR_ERROR_INVALID_ARGUMENT, "mesh materials: bad mesh index");
    const std::vector<uint64_t>& order = s->leaf_order[mesh];
    const uint64_t n = order.size();
    if (n == 0) return VR_OK;
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "mesh materials: null array");
    const int64_t tri_base = s->mesh_tri_base[mesh];
    std::vector<vr::TriVerts> tv;
    std::vector<vr::TriNormals> tn;
    const vr::TriVerts* tris = s->tris.data() + tri_base;
    const vr::TriNormals* normals = s->normals.data() + tri_base;
    if (!host_copies_current(s)) {
        tv.resize(n);
        tn.resize(n);
        VR_HIP(hipSetDevice(s->device));
        VR_HIP(hipMemcpy(tv.data(), s->dev.tris + tri_base, n * sizeof(vr::TriVerts), hipMemcpyDeviceToHost));
        VR_HIP(hipMemcpy(tn.data(), s->dev.normals + tri_base, n * sizeof(vr::TriNormals), hipMemcpyDeviceToHost));
        tris = tv.data();
        normals = tn.data();
    }
    // slot i holds the input triangle at reference leaf position rank - tri_base (build_update_plan's rule)
    for (uint64_t i = 0; i < n; ++i) {
        const int64_t r = tris[i].rank - tri_base;
        if (r < 0 || (uint64_t)r >= n || order[(size_t)r] >= n)
            return fail(VR_ERROR_DEVICE, "mesh materials: the ranks do not form the mesh's leaf order");
        const int64_t own = normals[i].material1;
        out[order[(size_t)r]] = own ? (uint32_t)(own - 1) : s->mesh_material[mesh];
    }
    return VR_OK;
}

int vr_scene_bvh_roots(const vr_scene* s, void* out) {
    if (!s || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    std::memcpy(out, s->bvhs.data(), s->bvhs.size() * sizeof(vr::Bvh));
    return VR_OK;
}
