// mesh_materials_check.cpp -- the host-only path of the per-triangle materials (vr_scene_set_mesh_materials,
// vr_scene_mesh_materials, vr_scene_triangles, vr_load_obj_groups) as a stand-alone program, for a run under
// the host sanitizers (tools/mesh_materials_asan.sh builds it with -fsanitize=address,undefined and runs it
// on the CPU).  A VR_SCENE_HOST_ONLY scene makes no device call.  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/vanrijn_amd.h"

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, vr_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

struct Records {  // vr_scene_triangles' two arrays
    std::vector<unsigned char> verts, normals;
    bool operator==(const Records& o) const { return verts == o.verts && normals == o.normals; }
};

static int records(const vr_scene* s, uint64_t n, Records* out) {
    out->verts.assign(80 * n, 0);
    out->normals.assign(80 * n, 0);
    return vr_scene_triangles(s, out->verts.data(), out->normals.data());
}

int main(int argc, char** argv) {
    const uint64_t n = 5;
    double samples[2] = {0.5, 0.5};
    vr_material_desc mats[3];
    std::memset(mats, 0, sizeof mats);
    for (auto& m : mats) {
        m.kind = VR_MATERIAL_LAMBERTIAN;
        m.colour = vr_spectrum{380.0, 740.0, 2, samples};
        m.diffuse_strength = 0.5;
    }
    std::vector<double> v(9 * n), nn(9 * n, 0.0);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (double)((i * 37) % 11) - 5.0 + 0.1 * (double)(i / 9);
    for (uint64_t t = 0; t < n; ++t)
        for (int c = 0; c < 3; ++c) nn[9 * t + 3 * c + 2] = 1.0;
    vr_mesh_desc mesh;
    std::memset(&mesh, 0, sizeof mesh);
    mesh.triangle_count = n;
    mesh.vertices = v.data();
    mesh.normals = nn.data();
    mesh.material = 1;
    vr_object_desc object;
    std::memset(&object, 0, sizeof object);
    object.kind = VR_OBJECT_BVH;
    object.first = 0;
    object.count = 1;
    vr_scene_desc desc;
    std::memset(&desc, 0, sizeof desc);
    desc.camera_location = vr_vec3{0.0, 0.0, -20.0};
    desc.material_count = 3;
    desc.materials = mats;
    desc.mesh_count = 1;
    desc.meshes = &mesh;
    desc.object_count = 1;
    desc.objects = &object;
    vr_scene* s = nullptr;
    CHECK(vr_scene_create(&desc, 0, VR_SCENE_HOST_ONLY, &s) == VR_OK);

    Records fresh, now;
    CHECK(records(s, n, &fresh) == VR_OK);
    uint32_t got[5];
    CHECK(vr_scene_mesh_materials(s, 0, got) == VR_OK);
    for (uint32_t g : got) CHECK(g == 1);

    // round trip
    const uint32_t ids[5] = {2, 0, 1, 2, 0};
    CHECK(vr_scene_set_mesh_materials(s, 0, n, ids) == VR_OK);
    CHECK(vr_scene_mesh_materials(s, 0, got) == VR_OK);
    CHECK(std::memcmp(got, ids, sizeof ids) == 0);
    unsigned char root[96];  // vr_scene_bvh_roots: int32 own_materials at byte 80
    int32_t flagged = -1;
    CHECK(vr_scene_bvh_roots(s, root) == VR_OK);
    std::memcpy(&flagged, root + 80, 4);
    CHECK(flagged == 1);
    Records set;
    CHECK(records(s, n, &set) == VR_OK);
    CHECK(set.verts == fresh.verts);
    uint64_t leaf_order[5];
    CHECK(vr_scene_bvh_leaf_order(s, 0, leaf_order) == VR_OK);
    for (uint64_t i = 0; i < n; ++i) {
        int64_t rank, word;
        std::memcpy(&rank, &set.verts[80 * i + 72], 8);
        std::memcpy(&word, &set.normals[80 * i + 72], 8);
        CHECK(rank >= 0 && (uint64_t)rank < n);
        CHECK(word == (int64_t)ids[leaf_order[rank]] + 1);
        CHECK(std::memcmp(&set.normals[80 * i], &fresh.normals[80 * i], 72) == 0);
    }

    // every error case, the scene untouched
    const uint32_t bad[5] = {2, 0, 3, 2, 0}, huge[5] = {0xFFFFFFFFu, 0, 0, 0, 0};
    CHECK(vr_scene_set_mesh_materials(nullptr, 0, n, ids) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials(s, 1, n, ids) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials(s, 0, n - 1, ids) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials(s, 0, n + 1, ids) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials(s, 0, 0, nullptr) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials(s, 0, n, bad) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials(s, 0, n, huge) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_set_mesh_materials_device(s, 0, n, ids, nullptr) == VR_ERROR_HOST_ONLY);
    CHECK(vr_scene_mesh_materials(nullptr, 0, got) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(vr_scene_mesh_materials(s, 1, got) == VR_ERROR_INVALID_ARGUMENT);
    CHECK(records(s, n, &now) == VR_OK);
    CHECK(now == set);

    // the assignment survives a transform and an update; a set after the transform reaches its base
    const double shift[12] = {1, 0, 0, 0.5, 0, 1, 0, -0.25, 0, 0, 1, 2.0};
    CHECK(vr_scene_transform_mesh(s, 0, shift, nullptr) == VR_OK);
    CHECK(vr_scene_mesh_materials(s, 0, got) == VR_OK);
    CHECK(std::memcmp(got, ids, sizeof ids) == 0);
    const uint32_t ids2[5] = {0, 1, 2, 0, 1};
    CHECK(vr_scene_set_mesh_materials(s, 0, n, ids2) == VR_OK);
    CHECK(vr_scene_transform_mesh(s, 0, shift, nullptr) == VR_OK);
    CHECK(vr_scene_update_mesh(s, 0, n, v.data(), nn.data()) == VR_OK);
    CHECK(vr_scene_mesh_materials(s, 0, got) == VR_OK);
    CHECK(std::memcmp(got, ids2, sizeof ids2) == 0);

    // the reset: the fresh scene's records again
    CHECK(vr_scene_set_mesh_materials(s, 0, n, nullptr) == VR_OK);
    CHECK(records(s, n, &now) == VR_OK);
    CHECK(now == fresh);
    CHECK(vr_scene_bvh_roots(s, root) == VR_OK);
    std::memcpy(&flagged, root + 80, 4);
    CHECK(flagged == 0);
    vr_scene_destroy(s);

    // the OBJ loader's groups
    const char* path = argc > 1 ? argv[1] : "mesh_materials_check.obj";
    FILE* f = std::fopen(path, "w");
    CHECK(f != nullptr);
    std::fputs("v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3\nusemtl red\nf 1 2 3 4\nusemtl blue  \nf 3 2 1\nusemtl red\nf 4 2 1\n", f);
    std::fclose(f);
    uint64_t tris = 0, plain_tris = 0;
    double *ov = nullptr, *on = nullptr, *pv = nullptr, *pn = nullptr;
    uint32_t *group = nullptr, group_count = 0;
    char* names = nullptr;
    CHECK(vr_load_obj_groups(path, &tris, &ov, &on, &group, &group_count, &names) == VR_OK);
    CHECK(vr_load_obj(path, &plain_tris, &pv, &pn) == VR_OK);
    std::remove(path);
    CHECK(tris == 5 && plain_tris == 5 && group_count == 3);
    CHECK(std::memcmp(ov, pv, 72 * tris) == 0 && std::memcmp(on, pn, 72 * tris) == 0);
    const uint32_t want[5] = {0, 1, 1, 2, 1};
    CHECK(std::memcmp(group, want, sizeof want) == 0);
    const char* name = names;
    CHECK(std::strcmp(name, "") == 0);
    name += std::strlen(name) + 1;
    CHECK(std::strcmp(name, "red") == 0);
    name += std::strlen(name) + 1;
    CHECK(std::strcmp(name, "blue") == 0);
    vr_mesh_free(ov, on);
    vr_mesh_free(pv, pn);
    vr_obj_groups_free(group, names);
    CHECK(vr_load_obj_groups("/nonexistent/none.obj", &tris, &ov, &on, &group, &group_count, &names) == VR_ERROR_IO);
    std::puts("mesh_materials_check: ok");
    return 0;
}
