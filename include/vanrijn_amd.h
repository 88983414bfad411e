/*
 * vanrijn_amd.h -- C ABI of the MI355X (gfx950) path-tracing core.
 *
 * Drop-in boundary for vanrijn's per-pixel hot path.  The reference's boundary is
 *     pub fn partial_render_scene(scene: &Scene, tile: Tile, height: usize, width: usize)
 *         -> AccumulationBuffer                                   (src/camera.rs:95-130)
 * called concurrently from rayon workers in src/main.rs:204 and from benches/simple_scene.rs:45.
 * Every entry point below names the reference interface it replaces.  Plain pointers and sizes
 * only; no HIP or torch types in the signatures (streams are passed as void*).  A Rust binding
 * (extern "C" block) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All floating point is IEEE binary64, as in the reference (everything on the path is f64).
 *   - Return value: VR_OK (0) or a negative vr_status.  The message of the last failure on the
 *     calling thread is in vr_last_error().  Nothing unwinds across the ABI; where the reference
 *     panics (singular shading basis, out-of-range tile) the call returns an error instead.
 *   - A vr_scene changes only through vr_scene_update_mesh (new vertices for one mesh, VR_HAS_SCENE_UPDATE),
 *     the scene edits (camera, primitives, materials, lights and a mesh's affine transform,
 *     VR_HAS_SCENE_EDIT) and the set-before-rendering hooks; between such calls it is immutable and may
 *     be shared by any number of threads.  An update or edit is not thread-safe against any other
 *     call on the same scene, and asynchronous work of the scene still queued on any stream must
 *     have finished first (the caller's to order, as for vr_scene_set_staging_limit).
 *     Render calls are re-entrant.  Each call holds its own stream, staging buffer, work-queue
 *     counter and device error word for its duration (a per-scene pool of call contexts), so
 *     concurrent calls neither serialise on shared scratch nor see each other's errors
 *     (tests/test_gpu_concurrency.py).
 *   - Errors found on the device (the singular shading basis where the reference panics,
 *     simple_random_integrator.rs:26-31) belong to the call that found them: synchronous entry
 *     points return them; the asynchronous vr_render_tile_device records them in a sticky word of
 *     its stream, returned by the next vr_stream_check_error (or timed launch) on that stream.
 *   - The film entry points (vr_film_*, VR_HAS_FILM) were added under ABI 10: they are additions
 *     only, so VR_ABI_VERSION did not move; probe for them with VR_HAS_FILM.
 */
#ifndef VANRIJN_AMD_H
#define VANRIJN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VR_ABI_VERSION 10
#define VR_HAS_FILM 1 /* the vr_film_* entry points below exist (added under ABI 10) */
/* VR_VARIANT_ONE_BVH, VR_LAUNCH_MULTI_BVH, vr_launch_takes_one_bvh and vr_scene_launch_variant exist
 * (additions under ABI 10: no structure or existing value changed) */
#define VR_HAS_ONE_BVH 1
#define VR_MAX_SPECTRUM_SAMPLES 64
#define VR_RECURSION_LIMIT 128 /* camera.rs:69 */

typedef enum vr_status {
    VR_OK = 0,
    VR_ERROR_INVALID_ARGUMENT = -1,
    VR_ERROR_OUT_OF_MEMORY = -2,
    VR_ERROR_DEVICE = -3,          /* a HIP call failed */
    VR_ERROR_NO_DEVICE = -4,       /* no gfx950 device visible */
    VR_ERROR_SINGULAR_BASIS = -5,  /* simple_random_integrator.rs:26-31 would panic ("expect") */
    VR_ERROR_IO = -6,              /* load_obj: std::io::Error (src/mesh.rs:74-77) */
    VR_ERROR_UNSUPPORTED = -7,     /* e.g. BVH deeper than the traversal stack */
    VR_ERROR_HOST_ONLY = -8        /* render call on a scene created with VR_SCENE_HOST_ONLY */
} vr_status;

typedef struct vr_vec3 {
    double x, y, z;
} vr_vec3; /* math::Vec3 (src/math/vec3.rs:8-10) */

/* colour::Spectrum (src/colour/spectrum.rs:5-10): samples linearly interpolated over
 * [shortest_wavelength, longest_wavelength], zero outside. */
typedef struct vr_spectrum {
    double shortest_wavelength;
    double longest_wavelength;
    uint32_t sample_count; /* 2 .. VR_MAX_SPECTRUM_SAMPLES */
    const double* samples;
} vr_spectrum;

typedef enum vr_material_kind {
    VR_MATERIAL_LAMBERTIAN = 0, /* materials/lambertian_material.rs:12-60 */
    VR_MATERIAL_REFLECTIVE = 1, /* materials/reflective_material.rs:8-48 */
    VR_MATERIAL_PHONG = 2,      /* materials/phong_material.rs:8-37 (sample: materials/mod.rs:28-33) */
    VR_MATERIAL_DIELECTRIC = 3  /* materials/smooth_transparent_dialectric.rs:64-115 (colour = eta) */
} vr_material_kind;

typedef struct vr_material_desc {
    int32_t kind;
    uint32_t reserved;
    vr_spectrum colour;         /* the refractive index eta(lambda) for the dielectric */
    double diffuse_strength;    /* Lambertian, reflective, Phong */
    double reflection_strength; /* reflective; Phong's specular_strength */
    double smoothness;          /* Phong only */
} vr_material_desc;

typedef enum vr_primitive_kind {
    VR_PRIMITIVE_PLANE = 0, /* raycasting/plane.rs:18-31: vector = normal (normalised here, as Plane::new), scalar = distance_from_origin */
    VR_PRIMITIVE_SPHERE = 1 /* raycasting/sphere.rs:15-23: vector = centre, scalar = radius */
} vr_primitive_kind;

typedef struct vr_primitive_desc {
    int32_t kind;
    uint32_t material;
    vr_vec3 vector;
    double scalar;
} vr_primitive_desc;

/* A triangle mesh (Vec<Arc<dyn Primitive>> of raycasting::Triangle, src/raycasting/triangle.rs:8-13).
 * vertices/normals: [triangle][corner 0..2][xyz] doubles; copied by vr_scene_create. */
typedef struct vr_mesh_desc {
    uint64_t triangle_count;
    const double* vertices;
    const double* normals;
    uint32_t material;
    uint32_t reserved;
} vr_mesh_desc;

typedef enum vr_object_kind {
    VR_OBJECT_PRIMITIVE_LIST = 0, /* Box<Vec<Box<dyn Primitive>>> (raycasting/vec_aggregate.rs:11-24) */
    VR_OBJECT_BVH = 1             /* Box<BoundingVolumeHierarchy> (raycasting/bounding_volume_hierarchy.rs:49-74) */
} vr_object_kind;

typedef struct vr_object_desc {
    int32_t kind;
    uint32_t first; /* primitive list: first primitive index; BVH: mesh index */
    uint32_t count; /* primitive list: number of primitives; BVH: must be 1 */
    uint32_t reserved;
} vr_object_desc;

/* scene::Scene (src/scene.rs:5-8): camera_location + objects in order (order decides ties,
 * sampler.rs:9-20). */
/* Integrators.  The reference's partial_render_scene always uses SimpleRandomIntegrator
 * (camera.rs:103); WhittedIntegrator (integrators/whitted_integrator.rs:15-87: directional lights
 * with shadow rays, an ambient term, one sampled continuation per hit) is selectable per scene. */
typedef enum vr_integrator_kind {
    VR_INTEGRATOR_SIMPLE_RANDOM = 0,
    VR_INTEGRATOR_WHITTED = 1
} vr_integrator_kind;

typedef struct vr_directional_light { /* whitted_integrator.rs:10-13 */
    vr_vec3 direction;
    vr_spectrum spectrum;
} vr_directional_light;

typedef struct vr_integrator_desc {
    int32_t kind;
    uint32_t light_count;        /* at most VR_MAX_LIGHTS */
    vr_spectrum ambient_light;   /* Whitted */
    const vr_directional_light* lights;
} vr_integrator_desc;
#define VR_MAX_LIGHTS 16

typedef struct vr_scene_desc {
    vr_vec3 camera_location;
    uint32_t material_count;
    uint32_t primitive_count;
    uint32_t mesh_count;
    uint32_t object_count;
    const vr_material_desc* materials;
    const vr_primitive_desc* primitives;
    const vr_mesh_desc* meshes;
    const vr_object_desc* objects;
    const vr_integrator_desc* integrator; /* NULL: SimpleRandomIntegrator */
} vr_scene_desc;

typedef struct vr_scene vr_scene;

#define VR_SCENE_HOST_ONLY 1u /* build + flatten only, no device upload (inspection, CPU tests) */
/* Build the meshes' BVHs on the device (level-synchronous sorts; the same nodes and leaf order as
 * the host build, bounding_volume_hierarchy.rs:38-74).  Meshes with NaN coordinates use the host
 * build.  Ignored with VR_SCENE_HOST_ONLY. */
#define VR_SCENE_DEVICE_BVH 2u
/* Traverse the reference's own median-split tree instead of the default SAH tree.  Results are
 * identical either way (the closest hit does not depend on the tree; ties follow the reference
 * tree's in-order leaf rank); the device build always produces the reference tree. */
#define VR_SCENE_REFERENCE_BVH 4u
/* Build the default traversal tree on the device as well (ABI 5): the reference's median-split
 * build above gives every triangle its in-order rank (the tie-break), then a binned-SAH binary
 * tree (the host build's algorithm, one workgroup per node and level) is built over the ranked
 * triangles and collapsed to the 4-wide render tree.  Renders are bit-identical to the host-built
 * scene's; only the build time differs.  Implies VR_SCENE_DEVICE_BVH; ignored with
 * VR_SCENE_REFERENCE_BVH or VR_SCENE_HOST_ONLY. */
#define VR_SCENE_DEVICE_SAH 8u
/* Collapse the binary traversal tree to the 4-wide render tree greedily (the largest-area interior
 * child expanded first) instead of by the SAH-optimal dynamic programme.
 * Renders are identical either way; for inspection and the collapse's own tests (ABI 7). */
#define VR_SCENE_GREEDY_COLLAPSE 16u
/* Render with the 64-bit-offset kernels whatever the scene's size (ABI 8).  They are chosen
 * automatically for scenes past the 32-bit load offsets of the default kernels -- 4 GB of triangle
 * records (53.7 M triangles) or 2^25 nodes of the 4-wide tree (vr_scene_needs_wide_offsets); this
 * flag exercises them on small scenes (tests).  Renders are identical either way. */
#define VR_SCENE_WIDE_OFFSETS 32u

/* Replaces building `Scene { camera_location, objects }` + BoundingVolumeHierarchy::build.
 * Copies every input; builds one BVH per mesh with the reference's median split
 * (bounding_volume_hierarchy.rs:38-74; ties in the sort broken by input triangle index);
 * flattens it and uploads it to `device` (HIP ordinal). */
int vr_scene_create(const vr_scene_desc* desc, int32_t device, uint32_t flags, vr_scene** out);
void vr_scene_destroy(vr_scene* scene);

typedef struct vr_scene_info {
    uint64_t triangle_count;
    uint64_t node_count;     /* flattened interior nodes over all BVHs */
    uint32_t max_bvh_depth;  /* levels, root = 1 */
    uint32_t object_count;
    double extent;           /* max |coordinate| of camera and geometry */
    uint64_t device_bytes;   /* scene bytes resident in HBM */
    uint64_t wide_node_count;  /* nodes of the render kernel's 4-wide traversal tree (ABI 3) */
    uint32_t traversal_stack;  /* deepest stack of the 4-wide walk, entries (ABI 3) */
    uint32_t flags;            /* VR_SCENE_INFO_* (ABI 5) */
} vr_scene_info;
/* Every continuation of every path is provably finite (each traced mesh triangle's vertex normals
 * lie strictly on one side of its plane, so the shading basis of triangle.rs:73-78 is finite at any
 * barycentric point; no Phong or dielectric material).  Only then does a path whose throughput is
 * exactly 0 end early; otherwise it is traced to the end, so a later NaN (e.g. the zero normals
 * mesh.rs:37 gives an OBJ without normals) reaches the pixel as the reference's 0 * NaN does
 * (simple_random_integrator.rs:39-53). */
#define VR_SCENE_INFO_NAN_FREE 1u
int vr_scene_get_info(const vr_scene* scene, vr_scene_info* out);
/* BVH leaf (in-order) sequence of mesh `mesh`: out[i] = input triangle index of leaf i. */
int vr_scene_bvh_leaf_order(const vr_scene* scene, uint32_t mesh, uint64_t* out);
/* The scene's flattened BVH interior nodes (all meshes, pre-order per mesh, scene-wide links):
 * node_count records of 128 B = { double box[2][6] (child c: min x, max x, min y, max y, min z,
 * max z); int32 child[2] (>= 0 interior node, < 0 leaf holding triangle ~child); 24 B pad }.
 * For inspection and build-parity tests. */
int vr_scene_bvh_nodes(const vr_scene* scene, void* out_nodes);

/* ---------------------------------------------------------------------------------------------
 * Scene updates: move or deform a mesh between frames without vr_scene_destroy + vr_scene_create.
 * Added under ABI 10 (VR_HAS_SCENE_UPDATE).
 *
 * The mesh's triangle and normal records are replaced and both trees (the binary tree of
 *   vr_trace_rays, shadow rays and VR_QUERY_REFERENCE_WALK, and the 4-wide render tree) are refitted
 *   bottom-up and exactly, with the mesh's root box, vr_scene_info::extent (and the cull margins
 *   derived from it) and VR_SCENE_INFO_NAN_FREE (and the early stop and kernel choice that follow
 *   from it).  Topology, ranks, leaf order, node counts, stack depths, the pass counter, the staging
 *   limit, the debug hooks, the pooled call contexts and the scene's device allocation stay.
 * Afterwards every entry point behaves as on a scene created from the new geometry with the same
 *   flags, bit for bit: the closest hit does not depend on the tree's shape, only on each triangle's
 *   own box and its mesh's root box, which a refit stores exactly.  The one exception: exact
 *   distance ties between two triangles of a mesh are broken by the rank in the reference's
 *   median-split tree, and an update keeps the creation-time ranks where a fresh scene would re-rank.
 *   A refitted tree may be slower to traverse than a rebuilt one (tools/update_bench.py reports it).
 * Both calls block: when they return VR_OK the scene is ready and the source arrays may be freed.
 * Errors come before anything is modified (a failed update leaves the scene bit for bit as it was):
 *   a null scene or array, a bad mesh index or a triangle_count that is not the mesh's:
 *   VR_ERROR_INVALID_ARGUMENT; a vertex coordinate that is not finite: VR_ERROR_UNSUPPORTED (normals
 *   may be anything; zero normals clear NAN_FREE); the device form on a VR_SCENE_HOST_ONLY scene:
 *   VR_ERROR_HOST_ONLY.  triangle_count == 0 on an empty mesh is VR_OK.  A mesh that backs no object
 *   is updated like any other.
 * On a VR_SCENE_HOST_ONLY scene the host form runs the same refit in plain C++ on the host arrays,
 *   with no device call.
 * The first update of a mesh builds its plan (slot -> input triangle, both trees' nodes by depth),
 *   kept in the scene; its bytes are added to vr_scene_info::device_bytes.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_SCENE_UPDATE 1
/* new vertices / normals for mesh `mesh` (index into vr_scene_desc::meshes), [triangle][corner][xyz] f64 as
 * vr_mesh_desc; triangle_count must equal the mesh's.  Host arrays. */
int vr_scene_update_mesh(vr_scene* scene, uint32_t mesh, uint64_t triangle_count, const double* vertices,
                         const double* normals);
/* the same from device arrays on the scene's GPU, ordered after earlier work on `stream` (NULL = the null stream) */
int vr_scene_update_mesh_device(vr_scene* scene, uint32_t mesh, uint64_t triangle_count, const double* vertices,
                                const double* normals, void* stream);
/* Inspection, beside vr_scene_bvh_nodes (all four: always the current state; device scenes read back).
 * vr_scene_wide_nodes: wide_node_count records of 128 B = { float bound[6][4] (min x, max x, min y,
 *   max y, min z, max z of the four child slots; NaN: empty); int32 child[4] (>= 0 wide node, INT32_MIN
 *   empty, else leaf holding triangle slot ~child); 16 B pad }.
 * vr_scene_triangles: triangle_count records of 80 B each, in slot (traversal leaf) order:
 *   { double v[9]; int64 rank } and { double n[9]; int64 material: 0 the owning mesh's, m + 1 material m
 *   (vr_scene_set_mesh_materials below) }; a NULL array is skipped.
 * vr_scene_bvh_roots: one 96-B record per BVH object, in object order = { double root_box[6];
 *   float root_box32[6]; int32 root, root4, own_materials (1: the mesh's triangles carry materials of their
 *   own, vr_scene_set_mesh_materials below; else 0), object, tri_base, material }. */
int vr_scene_wide_nodes(const vr_scene* scene, void* out);
int vr_scene_triangles(const vr_scene* scene, void* out_verts, void* out_normals);
int vr_scene_bvh_roots(const vr_scene* scene, void* out);

/* ---------------------------------------------------------------------------------------------
 * Scene edits: everything else a caller moves between frames -- the camera, the plane and the
 * spheres, a material, the Whitted lights -- and a mesh placed by an affine matrix, without
 * vr_scene_destroy + vr_scene_create.  Added under ABI 10 (VR_HAS_SCENE_EDIT).
 *
 * For every call below, as for vr_scene_update_mesh:
 * The call blocks: when it returns VR_OK the scene is ready and the arguments may be freed.
 * It is not thread-safe against any other call on the scene, and the scene's queued asynchronous work
 *   must have finished first.
 * Errors come before anything is modified: a failed call leaves the scene bit for bit as it was.
 * Afterwards every entry point (renders, films, samples, traces, queries, integrate, camera rays, the
 *   block cull, vr_scene_get_info) answers as on a scene created from the edited description with the
 *   same flags, bit for bit.  Topology, ranks, node counts, stack depths, the pass counter, the staging
 *   limit, the debug hooks, the pooled call contexts and the scene's device allocation stay.
 * On a VR_SCENE_HOST_ONLY scene each call changes the host records only, with no device call.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_SCENE_EDIT 1
/* vr_scene_desc::camera_location.  A coordinate that is not finite: VR_ERROR_INVALID_ARGUMENT.
 * vr_scene_info::extent and the cull margins follow.  The camera is a launch argument, not in HBM:
 * this call makes no device call at all, on any scene.  It changes the location only: the basis and
 * the film distance of the scene's pose (vr_scene_set_camera_pose below) stay. */
int vr_scene_set_camera(vr_scene* scene, vr_vec3 location);
/* Entries first .. first + count - 1 of vr_scene_desc::primitives; kind, material, vector and scalar may
 * all change.  Every row a primitive list made from such an entry is rebuilt as vr_scene_create builds it
 * (an entry in several overlapping lists has several rows, one in none has none); extent follows.
 * VR_ERROR_INVALID_ARGUMENT: a range past primitive_count, a null array with count > 0, an unknown
 * kind, a material index >= the creation desc's material_count.  count == 0 is VR_OK. */
int vr_scene_update_primitives(vr_scene* scene, uint32_t first, uint32_t count, const vr_primitive_desc* primitives);
/* Material `index` of vr_scene_desc::materials, validated as at creation (kind, 1..64 samples, non-null
 * samples).  VR_SCENE_INFO_NAN_FREE, the early stop and the kernel choice follow the new set of
 * materials as on a fresh scene (a Phong or dielectric material clears NAN_FREE). */
int vr_scene_update_material(vr_scene* scene, uint32_t index, const vr_material_desc* material);
/* The Whitted integrator's ambient spectrum, light spectra and directions (stored as given).  kind and
 * light_count must equal the scene's, else VR_ERROR_INVALID_ARGUMENT; spectra are validated as at
 * creation.  NULL means SimpleRandomIntegrator, which must then be the scene's: on such a scene the call
 * validates and changes nothing. */
int vr_scene_set_lights(vr_scene* scene, const vr_integrator_desc* integrator);
/* Mesh `mesh` becomes the affine image of its BASE geometry: the vertices and normals given at creation
 * or by the latest successful vr_scene_update_mesh[_device].  Transforms do not compound: a turntable
 * passes the absolute pose each frame and never drifts.  matrix: row-major 3 x 4, m = [A | t].  In f64,
 * without contraction, in exactly this order:
 *   vertex component c:  ((m[4c] * x + m[4c + 1] * y) + m[4c + 2] * z) + m[4c + 3]
 *   normal component c:  (K[c][0] * nx + K[c][1] * ny) + K[c][2] * nz
 *   K, the cofactor matrix of A, once per call: K[i][j] = A[i+1][j+1] * A[i+2][j+2] - A[i+1][j+2] * A[i+2][j+1],
 *   indices mod 3 -- the exact rule (A a) x (A b) = K (a x b), so shading normals stay on their
 *   triangle's side for any A, reflections included.  Normals are not normalised (the reference
 *   normalises the interpolated normal at the hit).
 * The identity matrix reproduces the base, except that -0.0 coordinates become +0.0 (x + 0.0).
 * Then both trees are refitted as by vr_scene_update_mesh, whose description applies, the tie caveat
 *   included: exact distance ties between two triangles of the mesh keep the creation-time ranks where
 *   a fresh scene would re-rank.  The `primitive` a hit on the mesh reports (vr_hit_record, vr_ray_hit) is
 *   that creation-time leaf position too; vr_scene_bvh_leaf_order maps it to the input triangle, which is
 *   the one a fresh scene hits.
 * The base is a copy of the mesh's triangle and normal records, 160 B per triangle, allocated at the
 *   mesh's first transform and added to vr_scene_info::device_bytes (beside the update plan); it follows
 *   every later vr_scene_update_mesh.  On the device the call reads only resident records: nothing
 *   per triangle is uploaded.
 * stream: the call is ordered after earlier work on it (NULL = the null stream), as
 *   vr_scene_update_mesh_device; ignored on VR_SCENE_HOST_ONLY scenes.
 * VR_ERROR_INVALID_ARGUMENT: a null scene or matrix, a bad mesh index, a matrix entry that is not finite.
 * VR_ERROR_UNSUPPORTED: a transformed vertex coordinate that is not finite (overflow); the scene and the
 *   base stay as they were.  A singular A is allowed: its degenerate triangles clear NAN_FREE, as the
 *   same arrays through vr_scene_update_mesh would.  An empty mesh: VR_OK after the matrix check.  A mesh
 *   that backs no object is transformed like any other. */
int vr_scene_transform_mesh(vr_scene* scene, uint32_t mesh, const double matrix[12], void* stream);
/* Inspection of what the edits change (always the current state; device scenes read back).  *count
 * receives the number of records; out == NULL returns only the count.
 * vr_scene_primitives: one 128-B record per primitive of every primitive list, in kernel order (object
 *   order, then list position) = { int32 kind, material, object, position; double vec[3] (plane normal /
 *   sphere centre), tan[3], cot[3] (plane basis), scalar (plane distance / sphere radius), pre[3] (plane:
 *   normal * distance; sphere: centre^2 per component), scalar2 (sphere: radius^2) }.
 * vr_scene_materials: one 1,080-B record per material row: the desc's materials, then for a Whitted scene
 *   the ambient row and one row per light, then the sky's lookup row = { int32 kind, n (samples);
 *   double shortest, longest, diffuse, reflection, smoothness, samples[64], knots[64] (the sample
 *   wavelengths), inv_step }. */
int vr_scene_primitives(const vr_scene* scene, void* out, uint32_t* count);
int vr_scene_materials(const vr_scene* scene, void* out, uint32_t* count);
int vr_scene_get_camera(const vr_scene* scene, vr_vec3* out);

/* ---------------------------------------------------------------------------------------------
 * Per-triangle materials: one mesh, one tree, many materials -- an OBJ's usemtl groups rendered
 * without cutting the model into one mesh per material.  Added under ABI 10 (VR_HAS_MESH_MATERIALS);
 * no structure and no existing value changes.
 *
 * Both setters are scene edits: the contract of "Scene edits" above applies word for word (blocking,
 *   not thread-safe against other calls on the scene, errors before anything is modified, host
 *   records only on a VR_SCENE_HOST_ONLY scene, where the device form returns VR_ERROR_HOST_ONLY).
 * materials[i] is the vr_scene_desc::materials index of INPUT triangle i of mesh `mesh` (the order of
 *   vr_mesh_desc / vr_scene_update_mesh); NULL goes back to the mesh's single material
 *   (vr_mesh_desc::material).  Afterwards every entry point (renders, films, samples, vr_integrate_rays*,
 *   the Whitted shading) answers as though each triangle's material were the given one.
 * The record: the last 8 bytes of a triangle's 80-B normal record (vr_scene_triangles) are an int64:
 *   0 means the owning mesh's material -- every record of a scene on which no set call was made, so
 *   such scenes are unchanged bit for bit -- and m + 1 means material m.  A hit reads the word only where
 *   the mesh's root record (vr_scene_bvh_roots) has own_materials set, which a set call with an array does
 *   and the NULL form clears.  Nothing else is written: topology, ranks, trees, extent, VR_SCENE_INFO_NAN_FREE, the kernel choice and the launch variant
 *   stay.  (The kernel choice and the early stop are derived from ALL of the desc's materials, whichever
 *   triangle uses which.)
 * The assignment survives vr_scene_update_mesh[_device] and vr_scene_transform_mesh, the transform's
 *   base copy included.
 * VR_ERROR_INVALID_ARGUMENT: a null scene, a bad mesh index, a triangle_count that is not the mesh's, an
 *   index >= the creation desc's material_count (the device form finds it with a reduction kernel and
 *   one blocking read-back before it writes).  A NULL array with the mesh's count -- 0 on an empty
 *   mesh -- is VR_OK.
 * The device form is ordered after earlier work on `stream` (NULL = the null stream); the host form
 *   uploads its array and runs the same two kernels.  A mesh's first set call builds its update plan
 *   (vr_scene_update_mesh above) where it has none; its bytes, and the 4 bytes per triangle the host
 *   form stages, are added to vr_scene_info::device_bytes.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_MESH_MATERIALS 1
int vr_scene_set_mesh_materials(vr_scene* scene, uint32_t mesh, uint64_t triangle_count, const uint32_t* materials);
int vr_scene_set_mesh_materials_device(vr_scene* scene, uint32_t mesh, uint64_t triangle_count,
                                       const uint32_t* materials_device, void* stream);
/* the current assignment in input-triangle order (the mesh's own material where none is set); `out`
 * holds the mesh's triangle count */
int vr_scene_mesh_materials(const vr_scene* scene, uint32_t mesh, uint32_t* out);

/* ---------------------------------------------------------------------------------------------
 * Camera pose: where the camera looks and how wide.  The reference's ImageSampler (camera.rs:24-66)
 * looks down +z from camera_location with the film one unit away; a pose turns and zooms it.  Added
 * under ABI 10 (VR_HAS_CAMERA_POSE).
 *
 * The ray rule.  x and y are the reference's film coordinates of the sample (the film is width / height
 * by 1 when width > height, else 1 by width / height: the image's shorter side spans a film length of 1;
 * the jitter is draws 0 and 1 of the pixel-sample stream, x first).  For each component c, in f64, without contraction, in this order:
 *     d_c = (x * right_c + y * up_c) + film_distance * forward_c
 * and the ray is Ray::new(location, d): origin `location`, direction d * (1 / |d|).
 * The default pose -- right (1,0,0), up (0,1,0), forward (0,0,1), film_distance 1.0, which every scene
 * has from vr_scene_create on -- gives the reference's rays bit for bit.
 * Field of view: across the image's shorter side, whose film length is 1, it is
 * 2 * atan(0.5 / film_distance) (53.13 degrees at 1.0); across the other side, of film length
 * width / height, 2 * atan(0.5 * (width / height) / film_distance).
 * Every entry point that forms camera rays reads the scene's pose: vr_render_tile*,
 * vr_partial_render_scene, vr_film_*, vr_render_samples, vr_camera_rays_device and the block cull,
 * which stays conservative under any admitted pose.  No entry point takes a new parameter.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_CAMERA_POSE 1
typedef struct vr_camera_pose {
    vr_vec3 location, right, up, forward;
    double film_distance;
} vr_camera_pose;
/* A scene edit: the contract above applies word for word (blocking; not thread-safe against other calls
 * on the scene; errors before anything is modified; works on VR_SCENE_HOST_ONLY scenes).  Like
 * vr_scene_set_camera it makes no device call: the pose is a launch argument.  vr_scene_info::extent and
 * the cull margins follow the location.  The axes are stored and used as given; either handedness is
 * allowed (a right-handed basis renders the mirrored view).
 * VR_ERROR_INVALID_ARGUMENT: a null argument; an entry that is not finite; two axes with |a . b| > 1e-9;
 * an axis with | |a|^2 - 1 | > 1e-9; film_distance outside [1e-3, 1e3]. */
int vr_scene_set_camera_pose(vr_scene* scene, const vr_camera_pose* pose);
int vr_scene_get_camera_pose(const vr_scene* scene, vr_camera_pose* out);
/* Host helper, no scene: the left-handed basis (x right, y up, z forward, as the reference's) of a camera
 * at `eye` looking at `target`, in this fixed arithmetic (normalize as the rule's; cross as vec3.rs:84-89):
 *     forward = normalize(target - eye);  right = normalize(cross(up_hint, forward));  up = cross(forward, right)
 * eye 0, target (0,0,1), up_hint (0,1,0), film_distance 1.0 returns the default pose exactly.
 * VR_ERROR_INVALID_ARGUMENT: a null out; an input that is not finite; eye == target; up_hint parallel to
 * the view direction (|cross(up_hint, forward)|^2 <= 1e-24 |up_hint|^2); film_distance outside [1e-3, 1e3];
 * inputs so large or small that the result would not pass vr_scene_set_camera_pose.  *out is written on
 * VR_OK only. */
int vr_camera_look_at(vr_vec3 eye, vr_vec3 target, vr_vec3 up_hint, double film_distance, vr_camera_pose* out);
/* The ray rule on the host, from the same inline function the kernels compile: the camera ray of pixel
 * (row, column) of a width x height image with jitter (ux, uy).  The pose is used as given (not
 * validated).  VR_ERROR_INVALID_ARGUMENT: a null argument, an empty image, a pixel outside it. */
int vr_camera_ray(const vr_camera_pose* pose, uint64_t width, uint64_t height, uint64_t row, uint64_t column,
                  double ux, double uy, double origin[3], double direction[3]);

/* ---------------------------------------------------------------------------------------------
 * Camera lens: aperture and focus distance (depth of field).  Added under ABI 10
 * (VR_HAS_CAMERA_LENS).  A thin lens of radius lens_radius lies in the pose's right / up plane at
 * `location`, focused on the plane focus_distance along `forward`: a point of that plane is sharp, and
 * the blur of any other grows with lens_radius.  lens_radius == 0 is no lens -- the pinhole of the
 * section above, bit for bit, with no draw spent -- and every scene has {0, 1} from vr_scene_create on.
 *
 * The lens rule.  (x, y) is the sample's film point as above, (lu, lv) in [0, 1) its lens draws.
 *     (dx, dy) = disc(lu, lv)   Shirley's concentric map (unit_disc.rs:28-40) of ox = 2 lu - 1,
 *                               oy = 2 lv - 1:  (0, 0) -> (0, 0);
 *                               |ox| > |oy|:  phi = ((pi / 4) * oy) / ox,  (ox cos phi, ox sin phi);
 *                               otherwise:    phi = ((pi / 4) * ox) / oy,  (oy sin phi, oy cos phi)
 *                               with sin and cos the fixed polynomials of vr_camera.h (Taylor through
 *                               x^15 / x^16, Horner in x^2), within 1.2e-16 of libm's on [-pi/4, pi/4]
 *     k = film_distance / focus_distance;  a = lens_radius * dx;  b = lens_radius * dy
 *     origin_c = location_c + (a * right_c + b * up_c)
 *     d_c = ((x - a * k) * right_c + (y - b * k) * up_c) + film_distance * forward_c
 * and the ray is origin, d * (1 / |d|): the line from the lens point through the point where the
 * pinhole ray of (x, y) meets the focus plane.  In f64, in this order, without contraction.
 * Draws.  In a scene with a lens lu and lv are draws 2 and 3 of the (pixel, sample) stream, Standard
 * like the jitter, lu first, taken for every sample; the wavelength is draw 4 and the material draws
 * start at 5, so vr_integrate_params::first_draw = 4 (5 with given wavelengths) replays a lens render.
 * A scene without a lens keeps its numbering (wavelength 2, materials from 3).
 * Read by vr_render_tile*, vr_partial_render_scene, vr_film_*, vr_render_samples,
 * vr_camera_rays_device (whose origins then vary per entry) and the block cull, which stays
 * conservative under any admitted lens.  No entry point takes a new parameter.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_CAMERA_LENS 1
typedef struct vr_camera_lens {
    double lens_radius, focus_distance;
} vr_camera_lens;
/* A scene edit: the contract above applies word for word (blocking; not thread-safe against other calls
 * on the scene; errors before anything is modified; works on VR_SCENE_HOST_ONLY scenes).  It makes no
 * device call: the lens is a launch argument.  vr_scene_info::extent and the margins derived from it take
 * the camera's part as max |location_c| + lens_radius.  vr_scene_set_camera and
 * vr_scene_set_camera_pose leave the lens alone, and this call leaves the pose alone.
 * VR_ERROR_INVALID_ARGUMENT: a null argument; an entry that is not finite; lens_radius outside [0, 1e3];
 * focus_distance outside [1e-3, 1e6]. */
int vr_scene_set_camera_lens(vr_scene* scene, const vr_camera_lens* lens);
int vr_scene_get_camera_lens(const vr_scene* scene, vr_camera_lens* out);
/* disc(lu, lv) on the host, unit radius, from the inline function the kernels compile.
 * VR_ERROR_INVALID_ARGUMENT: a null out. */
int vr_camera_lens_point(double lu, double lv, double out[2]);
/* The lens rule on the host, from the same inline functions: the ray of pixel (row, column) with jitter
 * (ux, uy) and lens draws (lu, lv).  Pose and lens are used as given (not validated); lens_radius == 0
 * returns vr_camera_ray's bits.  VR_ERROR_INVALID_ARGUMENT: as vr_camera_ray. */
int vr_camera_lens_ray(const vr_camera_pose* pose, const vr_camera_lens* lens, uint64_t width, uint64_t height,
                       uint64_t row, uint64_t column, double ux, double uy, double lu, double lv, double origin[3],
                       double direction[3]);

/* util::Tile (src/util/tile_iterator.rs:1-7): half-open row/column ranges of the full image. */
typedef struct vr_tile {
    uint64_t start_column, end_column, start_row, end_row;
} vr_tile;

/* AccumulationBuffer (src/accumulation_buffer.rs:6-12), row-major over the tile:
 * colour/colour_sum/colour_bias: [height][width][3] XYZ; weight/weight_bias: [height][width].
 * colour is the running mean (sum * (1/weight)); the *_bias arrays are the Kahan compensation. */
typedef struct vr_accumulation_buffer {
    uint64_t width, height;
    double* colour;
    double* colour_sum;
    double* colour_bias;
    double* weight;
    double* weight_bias;
} vr_accumulation_buffer;

/* Sampling parameters.  Each (pixel, sample) draws its random numbers from the counter-based
 * stream (seed, row*width+column, first_sample + s) ("vr-hash32 v2"), so results do
 * not depend on tiling, launch split or device count.  The stream's index space is 2^32 pixels x 2^32
 * samples: width*height > 2^32 or first_sample + spp > 2^32 returns VR_ERROR_UNSUPPORTED.  Each 64-bit
 * draw is two 32-bit hashes of one 32-bit counter word, so it carries 32 bits of state (a Standard
 * f64 takes one of at most 2^32 values). */
typedef struct vr_render_params {
    vr_tile tile;
    uint64_t height, width; /* full image, as partial_render_scene's height/width */
    uint32_t spp;           /* samples per pixel in this call (partial_render_scene == 1) */
    uint32_t accumulate;    /* 0: start from AccumulationBuffer::new(); 1: continue update_pixel */
    uint64_t seed;
    uint64_t first_sample;
} vr_render_params;

/* Replaces partial_render_scene (camera.rs:95-130) one-for-one: one sample per pixel into a
 * fresh tile buffer (`out` arrays are caller-allocated host memory, tile-sized).  The sample
 * index comes from a per-scene atomic pass counter starting at 0 (seed 0x5EED0001), so concurrent
 * callers get distinct random streams like the reference's thread_rng.  Thread-safe. */
int vr_partial_render_scene(const vr_scene* scene, vr_tile tile, uint64_t height, uint64_t width,
                            vr_accumulation_buffer* out);

/* Generalised form: spp samples per pixel, explicit seed / sample range, host buffers; `buf`
 * is read first when params->accumulate is 1 (update_pixel continuation). */
int vr_render_tile(const vr_scene* scene, const vr_render_params* params, vr_accumulation_buffer* buf);

/* Device-resident form for the multi-GPU path: `state` is a device pointer to the tile's records
 * (ABI 7) -- 8 doubles per pixel in two halves, for the n = tile_width*tile_height pixels in
 * row-major order:
 *     state[4p .. 4p+3]           = {sum X, sum Y, sum Z, weight}        (colour_sum, weight)
 *     state[4n + 4p .. 4n + 4p+3] = {bias X, bias Y, bias Z, weight_bias} (Kahan compensations)
 * The first half is the merge-exact part: records of disjoint sample sets (one per GPU) merge by
 * adding it, in place, with one collective over 32 B per pixel.  `stream` is a hipStream_t (NULL =
 * the null stream) and the call only enqueues work (no host synchronisation). */
typedef struct vr_launch_stats {
    float kernel_ms;          /* HIP-event time of the render kernel launch(es), valid when timed != 0 */
    uint32_t timed;
    uint64_t box_tests;       /* filled only when counters were requested */
    uint64_t node_visits;
    uint64_t triangle_tests;
    uint64_t rays;
    uint64_t shaded_triangle_hits;
    uint64_t samples;
    uint64_t traversal_slots;  /* 64 x wave-level traversal-loop iterations (lane utilisation) */
    uint64_t path_loop_slots;  /* 64 x wave-level path-loop iterations */
    uint64_t exact_box_tests;  /* f32 box tests too close to call, re-run exactly in f64 */
    float reduce_ms;           /* HIP-event time of the ordered per-pixel Kahan reduce(s) (timed) */
    uint32_t passes;           /* render + reduce launches (the staging buffer bounds a launch) */
    uint32_t variant;          /* VR_VARIANT_* bits of the render kernel that ran (ABI 8) */
    uint32_t reserved;
} vr_launch_stats;
#define VR_VARIANT_COOP 1u         /* the cooperative-tail instantiation (small launches, mirror scenes) */
#define VR_VARIANT_WIDE_OFFSETS 2u /* the 64-bit-offset kernels (VR_SCENE_WIDE_OFFSETS) */
#define VR_VARIANT_STACK16 4u      /* 16-bit traversal-stack entries (trees below 65,536 wide nodes; ABI 10) */
#define VR_VARIANT_ONE_BVH 8u      /* the single-BVH instantiation (one mesh with a wide root; VR_HAS_ONE_BVH) */

#define VR_LAUNCH_TIMED 1u    /* bracket the kernel with HIP events and synchronise at the end */
#define VR_LAUNCH_COUNTERS 2u /* counting build of the kernel (slower), fills the counters */
/* with VR_LAUNCH_TIMED: record the HIP events but return without waiting (stats: passes only); the
 * times are read later by vr_collect_launch_times, so back-to-back timed frames leave the GPU no
 * idle gap for a host round trip (ABI 6).  The caller must collect: a stream holds at most 4096
 * uncollected deferred launches, beyond which the call fails with VR_ERROR_INVALID_ARGUMENT. */
#define VR_LAUNCH_DEFER_TIMES 4u
/* skip the camera-frustum culling of 8x8 pixel blocks (every sample traced): the records are the
 * same bit for bit (tests/test_gpu_cull.py); for tests and A/B measurements (ABI 7) */
#define VR_LAUNCH_NO_CULL 8u
/* no BVH distance culling: every box the ray's line crosses is walked (the reference's exhaustive
 * traversal, bounding_volume_hierarchy.rs:94-120), with the same records bit for bit -- the check
 * that the tie rule does not lean on the culling order (tests/test_gpu_launch_variants.py; ABI 8) */
#define VR_LAUNCH_NO_DIST_CULL 16u
/* no cooperative tail (small launches of scenes with a reflective material otherwise spread a
 * wave's last one or two paths over its lanes): the same records bit for bit (ABI 8) */
#define VR_LAUNCH_NO_COOP 32u
/* cooperative tail without its whole-walk form (the one or two live paths' walks run in coop_step's
 * per-step form only): the same records bit for bit; for tests and A/B measurements (ABI 9) */
#define VR_LAUNCH_NO_LONE_WALK 64u
/* keep 32-bit traversal-stack entries where the tree would allow 16-bit ones: the same records bit for
 * bit; for tests and A/B measurements (ABI 10) */
#define VR_LAUNCH_STACK32 128u
/* run the generic kernel (a list of BVHs) where the scene's single BVH would allow the single-BVH
 * instantiation: the same records bit for bit; for tests and A/B measurements (VR_HAS_ONE_BVH) */
#define VR_LAUNCH_MULTI_BVH 256u

int vr_render_tile_device(const vr_scene* scene, const vr_render_params* params, double* state, void* stream,
                          uint32_t launch_flags, vr_launch_stats* stats);
/* Waits for `stream` and returns the first device error (VR_ERROR_SINGULAR_BASIS) of any
 * vr_render_tile_device launch of `scene` on that stream since the last check, then clears it
 * (ABI 4).  A VR_LAUNCH_TIMED launch performs this check itself. */
int vr_stream_check_error(const vr_scene* scene, void* stream);
/* Waits for the VR_LAUNCH_DEFER_TIMES launches of `scene` on `stream` since the last collection
 * and returns their summed HIP-event times, then forgets them; reports their device errors like
 * vr_stream_check_error (ABI 6). */
typedef struct vr_launch_times {
    double kernel_ms;    /* render kernel, summed over the launches' passes */
    double reduce_ms;    /* ordered per-pixel Kahan reduce, summed */
    uint32_t launches;   /* vr_render_tile_device calls collected */
    uint32_t passes;     /* render + reduce launches in them */
    uint32_t max_passes; /* the most passes of one call */
    uint32_t reserved;
} vr_launch_times;
int vr_collect_launch_times(const vr_scene* scene, void* stream, vr_launch_times* out);
/* Mean XYZ of host-side state records (the layout of vr_render_tile_device; only the sums half is
 * read): colour = colour_sum * (1 / weight) (accumulation_buffer.rs:59).  States of disjoint sample
 * sets (e.g. one per GPU) merge by element-wise addition of the sums half (the cross-GPU reduce),
 * which is what AccumulationBuffer::merge_tile's weighted blend (accumulation_buffer.rs:62-85)
 * computes. */
int vr_resolve_state(const double* state_host, uint64_t pixel_count, double* colour_out);
/* AccumulationBuffer::merge_tile (accumulation_buffer.rs:62-85, the host side of main.rs:214-216):
 * for every pixel of `tile` (full-image coordinates in `dst`), dst colour = blend(dst colour, dst
 * weight, src colour, src weight) = (c1 * w1 + c2 * w2) * (1 / (w1 + w2)); dst weight += src
 * weight.  dst's colour_sum / bias buffers are not touched (as in the reference).  Host only (ABI 4). */
int vr_merge_tile(vr_accumulation_buffer* dst, vr_tile tile, const vr_accumulation_buffer* src);

/* ---------------------------------------------------------------------------------------------
 * Film: the reference's full-image AccumulationBuffer (accumulation_buffer.rs:6-12) as a device
 * object, for main.rs's call pattern (main.rs:197-243): workers render 1-spp tiles, every tile is
 * folded into the image with merge_tile, the image goes through to_image_rgb_u8 for display.  With
 * a film the tile buffer never leaves the GPU, merge_tile runs there, and the display side reads
 * back 3 bytes per pixel.  Added under ABI 10 (VR_HAS_FILM).
 *
 * Arithmetic is that of vr_render_tile followed by vr_merge_tile, bit for bit.  merge_tile is not
 * commutative in floating point, so the merges of one film are serialised: each call is given a
 * merge_index (consecutive from 0, in the order the calls pass the film's lock) and the film is
 * what merging in that order gives.  A failed call may consume an index but leaves the film
 * unchanged bit for bit.  A snapshot (read, to_image_*) contains exactly the successful merges
 * with index < *merges_seen; later merges wait for it.  Rendering itself is not serialised: every
 * call renders on its own call context, only merges and snapshots are ordered.
 * --------------------------------------------------------------------------------------------- */
typedef struct vr_film vr_film;

/* AccumulationBuffer::new (accumulation_buffer.rs:14-28) on `device`: 32 B per pixel {colour X, Y, Z,
 * weight}, plus as much again for snapshots.  More than 2^32 pixels: VR_ERROR_UNSUPPORTED. */
int vr_film_create(uint64_t width, uint64_t height, int32_t device, vr_film** out);
/* Waits for the film's queued merges; NULL is allowed. */
void vr_film_destroy(vr_film* film);
/* Back to AccumulationBuffer::new; the merge index restarts at 0. */
int vr_film_clear(vr_film* film);

typedef struct vr_film_merge {
    uint64_t merge_index;  /* position of this call's merge_tile in the film's merge order */
    uint64_t first_sample; /* sample index the call rendered (the scene's pass counter for the drop-in form) */
} vr_film_merge;

/* partial_render_scene + merge_tile (main.rs:204,214-216) in one call: one sample per pixel of `tile`
 * (full-image coordinates; height/width are the film's), seed 0x5EED0001, the sample index from the
 * scene's pass counter exactly as vr_partial_render_scene draws it; the tile buffer never leaves the
 * device.  Returns once the merge has run, with the call's device error if any (the film is then
 * untouched).  Thread-safe.  `info` may be NULL. */
int vr_film_partial_render_scene(vr_film* film, const vr_scene* scene, vr_tile tile, vr_film_merge* info);
/* Generalised: params->spp samples, explicit seed / first_sample.  params->height / width must equal
 * the film's and params->accumulate must be 0 (the tile buffer is always fresh, as in the reference). */
int vr_film_render_tile(vr_film* film, const vr_scene* scene, const vr_render_params* params, vr_film_merge* info);
/* merge_tile of caller-owned device records of `tile` (the layout of vr_render_tile_device; only the
 * sums half is read: source colour = sum * (1 / weight), 0 where the weight is 0), e.g. the result of
 * the cross-GPU reduce.  `stream` is the stream that produced them (NULL = the null stream); the call
 * only enqueues work on it.  state_device must be 16-byte aligned (any hipMalloc or torch allocation is).
 * info->first_sample is 0: the call renders nothing. */
int vr_film_merge_state(vr_film* film, vr_tile tile, const double* state_device, void* stream, vr_film_merge* info);

/* Snapshot: the five host arrays of a full-image AccumulationBuffer (out->width / height must be the
 * film's).  colour and weight are the film; colour_sum / colour_bias / weight_bias are 0 because
 * merge_tile never touches them (accumulation_buffer.rs:62-85).  *merges_seen = number of merge
 * indices the snapshot contains (NULL allowed). */
int vr_film_read(vr_film* film, vr_accumulation_buffer* out, uint64_t* merges_seen);
/* to_image_rgb_u8(&ClampingToneMapper) of a snapshot (the bytes of vr_tone_map of its colours):
 * 3 bytes per pixel, row-major, into host memory, or into device memory enqueued on `stream`. */
int vr_film_to_image_rgb_u8(vr_film* film, uint8_t* rgb_host, uint64_t* merges_seen);
int vr_film_to_image_rgb_u8_device(vr_film* film, uint8_t* rgb_device, void* stream, uint64_t* merges_seen);

/* Per-(pixel, sample) records, for decision-identity checks against the oracle. */
typedef struct vr_sample_record {
    double wavelength; /* final photon wavelength (0 on camera miss / recursion limit) */
    double intensity;  /* final photon intensity before the x360 pdf scale */
    double xyz[3];     /* ColourXyz::from_photon of the scaled photon */
    int32_t bounces;   /* bounce rays traced */
    int32_t flags;     /* bit0 camera ray hit, bit1 recursion limit reached, bit2 singular basis */
} vr_sample_record;
int vr_render_samples(const vr_scene* scene, const vr_render_params* params, vr_sample_record* out);

/* Sampler::sample (src/sampler.rs:9-20) for a batch of rays (origins/directions: [n][3], the
 * directions are used as given, as Ray's fields).  Host arrays. */
typedef struct vr_hit_record {
    int32_t valid;
    int32_t object;
    int64_t primitive; /* primitive-list position, or BVH leaf position */
    double distance;
    double location[3];
    double normal[3];
    double tangent[3];
    double cotangent[3];
    double retro[3];
} vr_hit_record;
int vr_trace_rays(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                  vr_hit_record* out);

/* ---------------------------------------------------------------------------------------------
 * Ray queries: Sampler::sample(&Ray) -> Option<IntersectionInfo> (sampler.rs:9-20) and its
 * `.is_some()` form (the Whitted shadow rays, whitted_integrator.rs:37-38) for a batch of caller-
 * supplied rays, walked over the render kernel's 4-wide tree.  Added under ABI 10 (VR_HAS_RAY_QUERY).
 *
 * Directions are unit length, as Ray's fields always are: the distance cull compares the ray
 *   parameter with Euclidean distances and the f32 box tests' error bound assumes |d| = 1.
 *   VR_QUERY_NORMALIZE makes them so on the device with the reference's normalize (d * (1 / |d|)).
 *   Without the flag a direction that is not unit length gives unspecified hits, never an
 *   out-of-bounds access.  Origins may lie anywhere (the error bound carries |o|).
 * Results are the reference's Sampler::sample: among objects the earlier one wins distance ties,
 *   inside a BVH the later in-order leaf; boxes are tested as lines (no t >= 0 clamp); a triangle
 *   counts only if the exact f64 line test passes on its own leaf box and on its mesh's root box.
 * Errors: n == 0 returns VR_OK and touches nothing; a null scene, a null array with n > 0 or an
 *   unknown flag bit: VR_ERROR_INVALID_ARGUMENT; a VR_SCENE_HOST_ONLY scene: VR_ERROR_HOST_ONLY; a
 *   tree deeper than the largest traversal stack (48): VR_ERROR_UNSUPPORTED.
 * Outputs are written for indices < n only, every field of them (a miss: zeros).
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_RAY_QUERY 1

typedef struct vr_ray_hit { /* 32 B: the compact answer of Sampler::sample */
    double distance;        /* IntersectionInfo::distance; 0 when valid == 0 */
    int64_t primitive;      /* as vr_hit_record::primitive (list position / reference leaf position) */
    int32_t object;         /* scene object index */
    int32_t valid;
    uint64_t reserved;      /* written as 0: pads the record to 32 B, two aligned 16-B stores per ray */
} vr_ray_hit;

#define VR_QUERY_NORMALIZE 1u      /* apply Ray::new (mod.rs:41-46, d * (1/|d|)) to each direction first */
/* walk the binary f64 tree (the walk of vr_trace_rays) instead of the 4-wide tree: the same answers
 * bit for bit; for tests and A/B timing */
#define VR_QUERY_REFERENCE_WALK 2u

/* Sampler::sample for n rays.  origins / directions: device [n][3] f64; hits: device [n]; records:
 * NULL, or device [n] vr_hit_record (location, normal, tangent, cotangent, retro as well: the bits
 * of vr_trace_rays).  Only enqueues on `stream` (NULL = the null stream) of the scene's device; no
 * host synchronisation. */
int vr_query_closest_device(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                            uint32_t flags, vr_ray_hit* hits, vr_hit_record* records, void* stream);
/* Sampler::sample(ray).is_some(): hit[i] = 1 or 0, device [n] bytes.  Only enqueues. */
int vr_query_any_device(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                        uint32_t flags, uint8_t* hit, void* stream);
/* Host-array forms: staged through a call context exactly as vr_trace_rays.  Thread-safe,
 * re-entrant, return when done. */
int vr_query_closest(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                     uint32_t flags, vr_ray_hit* hits, vr_hit_record* records);
int vr_query_any(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                 uint32_t flags, uint8_t* hit);

/* ---------------------------------------------------------------------------------------------
 * The integrators for caller-supplied rays: the body of partial_render_scene's loop (camera.rs:107-
 * 120: sampler.sample(&ray), then integrator.integrate(..) or the zero photon) for a batch of rays
 * that come from the caller instead of the scene's ImageSampler -- another camera, light probes,
 * bounce rays of the caller's own.  Added under ABI 10 (VR_HAS_INTEGRATE).
 *
 * Per ray i: the closest hit is found with the rules of vr_query_closest (unit directions;
 *   VR_QUERY_NORMALIZE applies Ray::new's normalisation on the device).  A miss gives the photon
 *   {0, 0} with flags 0 and bounces 0 (camera.rs:110-113; the sky is not sampled for a primary miss,
 *   as in the reference).  A hit sets flags bit 0; the wavelength is Photon::random_wavelength
 *   (380 + 360 x Standard), the call's first draw of the ray's stream, when `wavelengths` is NULL,
 *   else wavelengths[i] and no draw is spent.  Then the scene's integrator runs exactly as in the
 *   render: SimpleRandomIntegrator, or Whitted where the scene selects it, all four material kinds,
 *   VR_RECURSION_LIMIT.  `intensity` is the photon's intensity before the x360 pdf scale
 *   (vr_sample_record::intensity, what vr_accumulate_photons_device reads); wavelength, bounces and
 *   flags are vr_sample_record's bit for bit: wavelength 0 with flags bit 1 after the recursion limit,
 *   flags bit 2 and photon {0, 0} for a singular shading basis.  No path stops early.
 * Random stream ("vr-hash32 v2"): ray i draws from the stream whose
 *   (pixel << 32) + sample is stream_ids[i], or ((first_stream + i) << 32) + sample when stream_ids is
 *   NULL, under `seed`; the stream's first `first_draw` draws are skipped.  first_draw = 2 with drawn
 *   wavelengths (3 with given ones) replays the material draws of pixel row * width + col of a render
 *   with that seed, whose draws 0 and 1 are the camera jitter.  first_stream + n > 2^32 or
 *   sample >= 2^32: VR_ERROR_UNSUPPORTED.
 * Errors: n == 0 returns VR_OK and touches nothing; a null scene or params, a null origins /
 *   directions / photons with n > 0 or a flag bit other than VR_QUERY_NORMALIZE:
 *   VR_ERROR_INVALID_ARGUMENT; a VR_SCENE_HOST_ONLY scene: VR_ERROR_HOST_ONLY; a tree deeper than the
 *   largest traversal stack (48): VR_ERROR_UNSUPPORTED -- all before the first device call.
 *   VR_ERROR_SINGULAR_BASIS: returned by the host form; the device form records it in the stream's
 *   sticky error word, read by vr_stream_check_error(scene, stream), as vr_render_tile_device does.
 *   vr_debug_set_fault_object is honoured.
 * Outputs are written for indices < n only.  photons must be 16-byte aligned, info 8-byte aligned
 *   (any hipMalloc or torch allocation is).
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_INTEGRATE 1

typedef struct vr_photon { /* 16 B: Photon (photon.rs) */
    double wavelength;
    double intensity;
} vr_photon;

typedef struct vr_path_info { /* 8 B */
    int32_t bounces; /* as vr_sample_record::bounces */
    int32_t flags;   /* as vr_sample_record::flags */
} vr_path_info;

typedef struct vr_integrate_params {
    uint64_t seed;         /* as vr_render_params::seed */
    uint64_t first_stream; /* stream_ids == NULL: ray i draws from stream (seed, first_stream + i, sample) */
    uint64_t sample;
    uint32_t first_draw;   /* draws of the stream skipped before the first one this call takes */
    uint32_t flags;        /* VR_QUERY_NORMALIZE only */
} vr_integrate_params;

/* origins / directions: device [n][3] f64; wavelengths: NULL or device [n] f64; stream_ids: NULL or
 * device [n] u64; photons: device [n]; info: NULL or device [n].  Only enqueues on `stream` (NULL = the
 * null stream) of the scene's device; no host synchronisation. */
int vr_integrate_rays_device(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                             const double* wavelengths, const uint64_t* stream_ids,
                             const vr_integrate_params* params, vr_photon* photons, vr_path_info* info, void* stream);
/* Host-array form: staged through a call context as vr_query_closest.  Thread-safe, re-entrant,
 * returns when done. */
int vr_integrate_rays(const vr_scene* scene, uint64_t n, const double* origins, const double* directions,
                      const double* wavelengths, const uint64_t* stream_ids, const vr_integrate_params* params,
                      vr_photon* photons, vr_path_info* info);
/* update_pixel (accumulation_buffer.rs:44-60, weight 1) of photons[s * pixel_count + p], s = 0 ..
 * spp - 1 in order, into pixel p's record at `state` (the layout of vr_render_tile_device; accumulate
 * 0: from a fresh record, 1: continuing the records there): the render's ordered reduce on its own.
 * Device pointers on `device`, 16-byte aligned; only enqueues on `stream`.
 * Every double is accepted as a wavelength: beyond +-20000 nm, the infinities included, all seven CIE
 * lobes are +0 as the reference's exp gives them, so the colour is 0 * intensity; a NaN wavelength or
 * intensity gives NaN in that pixel's sums, as update_pixel does. */
int vr_accumulate_photons_device(double* state, const vr_photon* photons, uint64_t pixel_count, uint32_t spp,
                                 uint32_t accumulate, int32_t device, void* stream);
/* ImageSampler::ray_for_pixel (camera.rs:24-66) of the scene's camera for every (sample, pixel) of
 * params->tile: entry s * (tile pixels) + p (p row-major in the tile) holds sample
 * params->first_sample + s of pixel p -- its origin, its direction (normalised once, as Ray::new) and
 * its stream id ((row * width + col) << 32) + sample; the jitter is draws 0 and 1 of that stream, x
 * before y.  Device arrays of spp * (tile pixels) entries; only enqueues on `stream`.  The way to feed
 * the scene's own camera through vr_integrate_rays_device, and the model for a caller's camera. */
int vr_camera_rays_device(const vr_scene* scene, const vr_render_params* params, double* origins,
                          double* directions, uint64_t* stream_ids, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Feature buffers: what the camera rays of a pixel's samples meet first -- normal, depth, coverage,
 * the object and primitive under the pixel, and the first hit's material colour (albedo) -- for
 * denoisers, compositing and picking.  Added under ABI 10 (VR_HAS_FEATURES); additions only.
 *
 * The rule.  For each pixel of params->tile and each sample first_sample .. first_sample + spp - 1, in
 *   this order: the sample's camera ray is formed exactly as vr_camera_rays_device and the render form
 *   it (the scene's pose and lens), its closest hit is found with the rules of vr_query_closest (the
 *   same walk of the 4-wide tree, scenes on either side of vr_scene_needs_wide_offsets), and the
 *   sample is folded into the pixel's record with plain f64 additions.  No shading runs and no bounce
 *   ray is traced.  One GPU lane owns one pixel, so the order of every sum is the sample order whatever
 *   the tile, the tiling or the split of the samples over calls: spp = 2 followed by spp = 1,
 *   first_sample = 2, accumulate = 1 gives the bits of spp = 3.
 * The draws.  The jitter is draws 0 and 1 of stream (seed, row * width + column, sample), x first; in a
 *   scene with a lens draws 2 and 3 are the lens draws.  Only when the albedo is asked for, a sample that
 *   hits draws its wavelength next (draw 2, or 4 with a lens): the draw the render takes for it.
 * The record, 64 B per pixel, row-major in the tile (vr_pixel_features below):
 *   normal_sum / distance_sum: IntersectionInfo::normal and ::distance summed over the samples that hit.
 *     NaN normals reach the sums as they reach the pixel in a render (the zero normals mesh.rs:37 gives
 *     an OBJ without normals are the usual source).  Mean normal = normal_sum * (1 / hits), mean
 *     depth = distance_sum * (1 / hits), coverage = hits / samples.
 *   distance_min, object, primitive: of the nearest sample -- the first sample that hit, replaced by a
 *     later one only if its distance is strictly less (the reference's min_by rule: a NaN distance
 *     never replaces a hit and is never replaced).  0, -1, -1 while hits == 0.
 * The albedo (albedo_state, optional): a state array of exactly vr_render_tile_device's layout, 8 doubles
 *   per pixel, holding update_pixel (weight 1) of one photon per sample in sample order: {0, 0} for a
 *   miss (camera.rs:110-113); for a hit {lambda, a} with lambda = Photon::random_wavelength from the draw
 *   above and a = Spectrum::intensity_at_wavelength(lambda) of the hit's material colour (exact; the
 *   strength factors are not applied; a triangle's own material, vr_scene_set_mesh_materials, is
 *   honoured), or 1.0 for a dielectric, whose spectrum is an index of refraction.  The x360 pdf scale
 *   and the CIE conversion are update_pixel's: the array equals vr_accumulate_photons_device of those
 *   photons bit for bit, so vr_tone_map_device, vr_resolve_state and vr_film_merge_state take it as it
 *   is.  It converges to the scene's reflectance under flat white light; at low spp it carries the same
 *   wavelength noise as the beauty image.
 * accumulate == 1 continues from the records already in both arrays (sums, counts, the nearest sample,
 *   the Kahan state); 0 starts fresh.
 * Errors, all before the first device call: a null scene or params, both outputs NULL, or accumulate
 *   not 0 or 1: VR_ERROR_INVALID_ARGUMENT; a VR_SCENE_HOST_ONLY scene: VR_ERROR_HOST_ONLY; then params
 *   as vr_render_tile_device checks them (a tile outside the image: VR_ERROR_INVALID_ARGUMENT; an image
 *   of more than 2^32 pixels or first_sample + spp > 2^32: VR_ERROR_UNSUPPORTED); a tree deeper than
 *   the largest traversal stack (48): VR_ERROR_UNSUPPORTED.  An empty tile or spp == 0 returns VR_OK
 *   and touches nothing, as a render.  There is no singular-basis error (nothing is shaded), and
 *   vr_debug_set_fault_object and vr_debug_set_launch_flags are ignored.
 * Either output may be NULL; with albedo_state == NULL no wavelength is drawn and no material is read.
 *   Records are written for the tile's pixels only.  Both arrays must be 16-byte aligned (any hipMalloc
 *   or torch allocation is).
 * Limits.  Parallelism is one lane per pixel: a tiny tile at a very large spp runs on few lanes
 *   (splitting a pixel's samples over lanes would change the order of the sums).  The block cull of the
 *   render is not used: a ray that misses everything costs its root tests.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_FEATURES 1

typedef struct vr_pixel_features { /* 64 B, four 16-B quads */
    double normal_sum[3];  /* sum of IntersectionInfo::normal over the hit samples, in sample order */
    double distance_sum;   /* sum of IntersectionInfo::distance over the hit samples, in sample order */
    double distance_min;   /* distance of the nearest hit sample; 0 while hits == 0 */
    uint32_t hits;         /* samples whose camera ray hit */
    uint32_t samples;      /* samples folded in */
    int32_t object;        /* scene object of the nearest sample; -1 while hits == 0 */
    int32_t reserved;      /* 0 */
    int64_t primitive;     /* as vr_ray_hit::primitive of the nearest sample; -1 while hits == 0 */
} vr_pixel_features;

/* features: NULL or device [tile pixels]; albedo_state: NULL or device, 8 doubles per tile pixel.  Only
 * enqueues on `stream` (NULL = the null stream) of the scene's device; no host synchronisation. */
int vr_render_features_device(const vr_scene* scene, const vr_render_params* params, vr_pixel_features* features,
                              double* albedo_state, void* stream);
/* Host-array form: staged through a call context as vr_query_closest (with accumulate == 1 the arrays are
 * uploaded first).  Thread-safe, re-entrant, returns when done. */
int vr_render_features(const vr_scene* scene, const vr_render_params* params, vr_pixel_features* features,
                       double* albedo_state);

/* ---------------------------------------------------------------------------------------------
 * Denoiser: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; the spatial filter of SVGF)
 * over a noisy state array, guided by the feature records and, optionally, the albedo state of
 * vr_render_features*.  A pure function of its arrays: no scene, no tree, no random stream.  Added
 * under ABI 10 (VR_HAS_DENOISE); additions only.
 *
 * The rule.  All arithmetic is IEEE binary64, in exactly the order written, with no contraction; the
 *   host form and the device form give the same bits.  n = width * height, pixels row-major.
 * Inputs per pixel p.
 *   Presence: w_p = state[4p + 3].  A pixel with w_p == 0 is absent: as a tap it is skipped, as a centre
 *     it produces the all-zero output record (8 zeros).
 *   Colour: c_p[k] = state[4p + k] * (1 / w_p), k = 0..2 (only the sums half of the state is read; the
 *     layout is vr_render_tile_device's).
 *   Guide: h = features[p].hits.  h == 0: the pixel is background.  Otherwise inv = 1 / (double)h,
 *     g_p = normal_sum * inv (three products), z_p = distance_sum * inv, iz_p = 1 / z_p,
 *     o_p = features[p].object.
 *   Albedo (only with VR_DENOISE_DEMODULATE, which requires albedo_state): a_p[k] is formed from
 *     albedo_state exactly as c_p from state, and is 0 where the albedo weight is 0.  Channel k of pixel
 *     p is demodulated when a_p[k] > VR_DENOISE_ALBEDO_FLOOR; then c_p[k] = c_p[k] / a_p[k] before the
 *     first iteration.
 * Constants, computed once on the host and passed to the kernels: kc_0 = 1 / (sigma_colour *
 *   sigma_colour); kc_i = kc_0 * 4^i (an exact scaling: the colour sigma halves per iteration);
 *   kn = 1 / (sigma_normal * sigma_normal); kz = 1 / (sigma_depth * sigma_depth);
 *   hk[5] = {1/16, 1/4, 3/8, 1/4, 1/16}.
 * Iteration i = 0 .. iterations - 1, step s = 2^i, reads colours c and writes c'; the guides never
 *   change.  For centre p = (x, y), visit the taps q = (x + dx*s, y + dy*s) with dy = -2..2 in the outer
 *   loop and dx = -2..2 in the inner loop; the centre tap is visited in its place.  A tap is skipped if
 *   q lies outside the image; q is absent; exactly one of p and q is background;
 *   VR_DENOISE_MATCH_OBJECT is set, both hit, and o_p != o_q; e (below) is NaN; or w (below) is 0.
 *   For a tap that is not skipped earlier:
 *     d = c_q - c_p, e_c = ((d0*d0 + d1*d1) + d2*d2) * kc_i.
 *     If both p and q are background, e_n = e_z = 0.  Otherwise m = g_q - g_p,
 *     e_n = ((m0*m0 + m1*m1) + m2*m2) * kn, t = (z_q - z_p) * iz_p, e_z = (t * t) * kz.
 *     e = (e_c + e_n) + e_z.
 *     w = (hk[dy+2] * hk[dx+2]) * vr_exp_tab(-e)   (the table-driven exp of the ordered reduce, on
 *     host and device alike).
 *     S_k = S_k + w * c_q[k] and W = W + w, both starting from +0.0.
 *   The result is c'_p[k] = S_k * (1 / W).  If the centre tap itself was skipped, c'_p = c_p instead: a
 *   NaN or infinite colour, NaN normals or a mean depth of 0 make the pixel pass through unchanged, and
 *   it poisons no neighbour.  An absent centre stays absent.
 * Output.  Demodulated channels are multiplied back, c[k] * a_p[k].  out_state[4p .. 4p+3] =
 *   {c0, c1, c2, 1.0} and out_state[4n + 4p .. 4n + 4p+3] = 0, so vr_tone_map_device, vr_resolve_state
 *   and vr_film_merge_state take the output as it is (X * (1 / 1.0) is X).  Records are written for the
 *   n pixels only.  out_state may be the same array as state: everything the filter needs is copied
 *   into the workspace first.
 * Errors, all before anything is written or enqueued.  VR_ERROR_INVALID_ARGUMENT: a null params, state,
 *   features or out_state; a null workspace with n > 0 (device form); iterations outside 1..8; an
 *   unknown flag (or both VR_DENOISE_LOADS_* at once); VR_DENOISE_DEMODULATE without an albedo; a sigma
 *   that is not finite or is <= 0; a device array that is not 16-byte aligned.  VR_ERROR_UNSUPPORTED:
 *   more than 2^31 pixels; in the device forms also an image of 2^24 or more blocks of 64 x 4 pixels
 *   (started blocks count whole: an image one pixel wide and 2^26 high is one).  width * height == 0
 *   returns VR_OK and touches nothing.
 * Limits.  No variance estimate (the state carries no second moment): the colour weight compares noisy
 *   means, so sigma_colour trades noise left against detail lost.  Temporal accumulation is a stage of
 *   its own that runs before this one ("Temporal reprojection" below).  vr_denoise_host runs on one thread.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_DENOISE 1

#define VR_DENOISE_MATCH_OBJECT 1u /* a tap of another object (vr_pixel_features::object) is skipped */
#define VR_DENOISE_DEMODULATE 2u   /* filter colour / albedo, multiply the albedo back at the end */
/* How an iteration's taps are loaded; the result's bits are the same.  Neither: the library's own choice
 * per step ("Denoiser").  For measurement and the tests. */
#define VR_DENOISE_LOADS_DIRECT 4u /* every step reads the workspace directly */
#define VR_DENOISE_LOADS_LDS 8u    /* every step up to VR_DENOISE_LDS_MAX_STEP stages its tap rows in LDS */
#define VR_DENOISE_LDS_MAX_STEP 16u
#define VR_DENOISE_ALBEDO_FLOOR (1.0 / 1024.0)
#define VR_DENOISE_MAX_ITERATIONS 8u

typedef struct vr_denoise_params {
    uint64_t width, height;
    uint32_t iterations; /* 1..8; iteration i has tap spacing 2^i */
    uint32_t flags;      /* VR_DENOISE_* */
    double sigma_colour, sigma_normal, sigma_depth; /* of XYZ colour, of the mean normal, of relative depth */
} vr_denoise_params;

/* iterations 5, no flags, sigma_colour 32 (the least XYZ RMSE of the sweep in DESIGN.md section 2, "Denoiser"),
 * sigma_normal 0.5, sigma_depth 0.1. */
int vr_denoise_default_params(uint64_t width, uint64_t height, vr_denoise_params* out);
/* The device form's workspace: 128 B per pixel (two colour buffers, the guides, the albedo). */
int vr_denoise_workspace_bytes(const vr_denoise_params* params, uint64_t* out_bytes);
/* state, features, albedo_state (NULL allowed), out_state and workspace are device pointers, 16-byte
 * aligned.  Only enqueues on `stream` (NULL = the null stream) of `device`: no host synchronisation and
 * no allocation. */
int vr_denoise_device(const vr_denoise_params* params, const double* state, const vr_pixel_features* features,
                      const double* albedo_state, double* out_state, void* workspace, int32_t device, void* stream);
/* Measurement hook: enqueues one stage of vr_denoise_device with its checks -- stage 0 the prepare kernel,
 * 1 .. iterations the iteration stage - 1, iterations + 1 the finish kernel; another stage is
 * VR_ERROR_INVALID_ARGUMENT.  The stages in order are vr_denoise_device. */
int vr_denoise_stage_device(const vr_denoise_params* params, uint32_t stage, const double* state,
                            const vr_pixel_features* features, const double* albedo_state, double* out_state,
                            void* workspace, int32_t device, void* stream);
/* Host arrays, staged through the device; returns when done. */
int vr_denoise(const vr_denoise_params* params, const double* state, const vr_pixel_features* features,
               const double* albedo_state, double* out_state, int32_t device);
/* The same rule in plain C++ on host arrays, with no device call at all: the counterpart of the
 * VR_SCENE_HOST_ONLY paths, for a machine with no GPU. */
int vr_denoise_host(const vr_denoise_params* params, const double* state, const vr_pixel_features* features,
                    const double* albedo_state, double* out_state);

/* ---------------------------------------------------------------------------------------------
 * Temporal reprojection: carries an accumulated image across a camera move (or a rigid motion of scene
 * objects).  The previous accumulation is reprojected into the new view through the feature records of
 * both frames, validated against the geometry, and the new frame's sums are added to it; the result is a
 * state array again, the denoiser's input.  A pure function of its arrays: no scene, no tree, no random
 * stream.  Added under ABI 10 (VR_HAS_REPROJECT); additions only.
 *
 * Arguments.  state, features: the current frame -- a vr_render_tile_device state and the records of
 *   vr_render_features* of the same full width x height image.  previous_state: the history -- the
 *   previous call's out_state, or the previous frame's state at start-up; previous_features: the previous
 *   frame's records.  Both frames describe the same width x height image.  motion: NULL, or motion_count
 *   rows of 12 doubles; row o is a row-major 3x4 matrix [A | t] that maps a current-frame world position
 *   on scene object o (vr_pixel_features::object) to where that point was in the previous frame -- for a
 *   mesh placed by vr_scene_transform_mesh, M_prev * M_cur^-1.  Objects >= motion_count did not move.  The
 *   rows are meant for rigid motions: the mean normal goes through A itself, not through its cofactors.
 *   out_state: a state array; it may be `state` (a pixel reads only its own current record), it may not
 *   be previous_state, which is gathered.
 *
 * The rule.  All arithmetic is IEEE binary64, in exactly the order written, with no contraction; the
 *   three forms give the same bits.  n = width * height, pixels row-major, p = row * width + column.  The
 *   lens is ignored: geometry uses the pinhole ray through the pixel centre.  dt2 = depth_tolerance *
 *   depth_tolerance and nt2 = normal_tolerance * normal_tolerance are formed once on the host.  A step
 *   that says "no history" leaves the record of step 1 as the output's sums record.
 *   1. Current record.  W = state[4p+3].  W == 0: the output record is 8 zeros (absent, as in the
 *      denoiser).  Otherwise the record starts as {state[4p], state[4p+1], state[4p+2], W}.
 *   2. Geometry.  h = features[p].hits; h == 0: no history.  inv = 1 / (double)h, g = normal_sum * inv
 *      (three products), z = distance_sum * inv.  Not (z > 0), or z infinite: no history.
 *      d = the camera ray rule's direction (above, "Camera pose") of `pose` at the film point of the
 *      pixel centre, jitter (0.5, 0.5).  P_c = location_c + d_c * z for each component c.
 *   3. Motion.  o = features[p].object.  If motion != NULL and 0 <= o < motion_count, with m = row o:
 *      P'_c = ((m[4c] * P_x + m[4c+1] * P_y) + m[4c+2] * P_z) + m[4c+3]   (vr_scene_transform_mesh's order)
 *      g'_c = (m[4c] * g_x + m[4c+1] * g_y) + m[4c+2] * g_z.   Otherwise P' = P and g' = g.
 *   4. Same-view shortcut.  If pose and previous_pose are equal field by field (== on all 13 doubles) and
 *      the pixel has no motion row or its row equals the identity entry by entry: the footprint is the
 *      single tap q = p with b = 1, and z' = z, iz' = 1 / z; go to step 7.  (Progressive accumulation of
 *      a still view is exact: the output's sums are state + previous_state element by element.)
 *   5. Projection, on previous_pose.  v = P' - location.  a = (v_x * right_x + v_y * right_y) + v_z *
 *      right_z; bb with up and c with forward the same way.  Not (c > 0): no history.
 *      s = film_distance / c, x' = a * s, y' = bb * s.  z' = sqrt((v_x * v_x + v_y * v_y) + v_z * v_z),
 *      iz' = 1 / z'.  With film[4] the film constants of width x height (film_w / width, film_w / 2,
 *      film_h / height, film_h / 2 as the ray rule forms them):
 *      fx = (x' + film[1]) / film[0] - 0.5,  fy = (y' + film[3]) / film[2] - 0.5,
 *      fr = (double)(height - 1) - fy.
 *   6. Footprint.  Not (fx >= -1 && fx < (double)width && fr >= -1 && fr < (double)height): no history
 *      (tested before any conversion to an integer: NaN and overflow end here).  ix = floor(fx),
 *      tx = fx - ix; iy = floor(fr), ty = fr - iy.  Taps in the order (dy, dx) = (0,0), (0,1), (1,0),
 *      (1,1) at q = (row iy + dy, column ix + dx) with b = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty).  A
 *      tap with b == 0, or outside the image, is skipped unread.
 *   7. Tap test.  S_q[0..2] = previous_state[4q .. 4q+2], W_q = previous_state[4q+3].  The tap is skipped
 *      if any of the four is not finite (x - x != 0); W_q == 0; previous_features[q].hits == 0;
 *      VR_REPROJECT_MATCH_OBJECT is set and previous_features[q].object != o; with invq = 1 /
 *      (double)hits_q, z_q = distance_sum_q * invq and t = (z_q - z') * iz', not (t * t <= dt2); with
 *      m = normal_sum_q * invq - g' (three products, three differences), not (((m0 * m0 + m1 * m1) +
 *      m2 * m2) <= nt2).  A NaN fails either comparison, so a NaN guide poisons nothing.
 *   8. Fold.  From +0.0, for each tap kept, in tap order: B = B + b, H_k = H_k + b * S_q[k],
 *      Wh = Wh + b * W_q.  B == 0: no history.  Otherwise r = 1 / B, H_k = H_k * r, Wh = Wh * r (the
 *      footprint is renormalised over its valid taps).
 *   9. Cap.  If Wh > max_history_weight: f = max_history_weight / Wh, H_k = H_k * f, Wh =
 *      max_history_weight.  A finite cap is the usual exponential moving average: the new frame's share
 *      never falls below W / (cap + W).
 *   10. Output.  out_state[4p+k] = state[4p+k] + H_k, out_state[4p+3] = W + Wh, and
 *      out_state[4n+4p .. 4n+4p+3] = 0 (the bias half), so vr_tone_map_device, vr_resolve_state,
 *      vr_film_merge_state and the denoiser take the output as it is.  Records are written for the n
 *      pixels only.
 * Errors, all before anything is written or enqueued.  VR_ERROR_INVALID_ARGUMENT: a null params, state,
 *   features, previous_state, previous_features or out_state; motion == NULL with motion_count > 0;
 *   out_state == previous_state; an unknown flag; a tolerance that is not finite or is <= 0;
 *   max_history_weight NaN or <= 0 (+inf is allowed: no cap); a pose that vr_scene_set_camera_pose would
 *   refuse; a device array that is not 16-byte aligned.  VR_ERROR_UNSUPPORTED: more than 2^31 pixels; in
 *   the device forms also an image of 2^24 or more blocks of 64 x 4 pixels, as the denoiser.
 *   width * height == 0 returns VR_OK and touches nothing.
 * Limits.  No lens-aware reprojection, no motion-vector output, no variance estimate.  A deforming mesh
 *   (vr_scene_update_mesh) has no motion row: its history survives only where the validity tests pass.
 *   vr_reproject_host runs on one thread.
 * --------------------------------------------------------------------------------------------- */
#define VR_HAS_REPROJECT 1

#define VR_REPROJECT_MATCH_OBJECT 1u /* a previous-frame tap of another object is skipped */

typedef struct vr_reproject_params { /* 256 B */
    uint64_t width, height;
    vr_camera_pose pose, previous_pose; /* of the current frame and of the frame `previous_*` was rendered from */
    double depth_tolerance;             /* relative, > 0 */
    double normal_tolerance;            /* of the mean normal's difference, > 0 */
    double max_history_weight;          /* > 0, +inf allowed: caps the weight the history brings */
    uint32_t flags, motion_count;       /* VR_REPROJECT_*; rows of `motion` */
} vr_reproject_params;

/* depth_tolerance 0.05, normal_tolerance 0.25, max_history_weight 64, VR_REPROJECT_MATCH_OBJECT,
 * motion_count 0 ("Temporal reprojection").  The poses are copied, not validated. */
int vr_reproject_default_params(uint64_t width, uint64_t height, const vr_camera_pose* pose,
                                const vr_camera_pose* previous_pose, vr_reproject_params* out);
/* Every array is a device pointer, 16-byte aligned (motion too, where given).  Only enqueues on `stream`
 * (NULL = the null stream) of `device`: no host synchronisation, no allocation, no workspace. */
int vr_reproject_device(const vr_reproject_params* params, const double* state, const vr_pixel_features* features,
                        const double* previous_state, const vr_pixel_features* previous_features,
                        const double* motion, double* out_state, int32_t device, void* stream);
/* Host arrays, staged through the device; returns when done. */
int vr_reproject(const vr_reproject_params* params, const double* state, const vr_pixel_features* features,
                 const double* previous_state, const vr_pixel_features* previous_features, const double* motion,
                 double* out_state, int32_t device);
/* The same rule in plain C++ on host arrays, with no device call at all. */
int vr_reproject_host(const vr_reproject_params* params, const double* state, const vr_pixel_features* features,
                      const double* previous_state, const vr_pixel_features* previous_features,
                      const double* motion, double* out_state);

/* Host helpers (scene setup; no device work). */
/* Spectrum::reflection_from_linear_rgb (spectrum.rs:81-165): 32 samples over [380, 720] nm. */
int vr_spectrum_reflection_from_linear_rgb(double red, double green, double blue, double out[32]);
/* Spectrum::intensity_at_wavelength (spectrum.rs:64-79). */
double vr_spectrum_intensity_at_wavelength(const vr_spectrum* spectrum, double wavelength);
/* ColourXyz::for_wavelength (colour_xyz.rs:22-29). */
void vr_colour_xyz_for_wavelength(double wavelength, double out[3]);
/* mesh::load_obj (src/mesh.rs:74-88): positions/normals parsed as f32 then widened, polygons
 * fan-triangulated; missing normals are zero.  Returns a malloc'ed [n][3][3] pair; free with
 * vr_mesh_free. */
int vr_load_obj(const char* path, uint64_t* triangle_count, double** vertices, double** normals);
void vr_mesh_free(double* vertices, double* normals);
/* vr_load_obj with the file's usemtl groups (VR_HAS_MESH_MATERIALS): triangles, vertices and normals are
 * exactly vr_load_obj's (the same parse, order and bits); group[t] is the number of the usemtl name in
 * force at triangle t's face.  Names are numbered in order of first appearance; a repeated name reuses
 * its number; faces before any usemtl belong to the empty name "", which is in the list only if such
 * faces exist.  names: one malloc'ed block of group_count NUL-terminated strings, one after the other.
 * No .mtl file is read: the caller maps names to its own materials (vr_scene_set_mesh_materials).
 * Free the geometry with vr_mesh_free, group and names with vr_obj_groups_free. */
int vr_load_obj_groups(const char* path, uint64_t* triangle_count, double** vertices, double** normals,
                       uint32_t** group, uint32_t* group_count, char** names);
void vr_obj_groups_free(uint32_t* group, char* names);

/* AccumulationBuffer::to_image_rgb_u8(&ClampingToneMapper) (accumulation_buffer.rs:38-42,
 * image.rs:166-187, colour_xyz.rs:49-84): XYZ -> linear sRGB (the reference's matrix) ->
 * srgb_gamma (its constants 12.98 / 1.005) -> clamp to [0, 1] -> (v * 255) truncated (NaN -> 0).
 * vr_tone_map_device: `state` = device records (as vr_render_tile_device writes them; only the
 * sums half is read; colour = colour_sum * (1 / weight), 0 where weight is 0), `rgb_out` = device memory
 * (3 bytes per pixel, row-major); enqueued on `stream` (NULL = the null stream) of `device`.
 * vr_tone_map: host XYZ colour buffer (3 f64 per pixel) -> host RGB bytes. */
int vr_tone_map_device(const double* state, uint64_t pixel_count, uint8_t* rgb_out, int device, void* stream);
int vr_tone_map(const double* colour_xyz, uint64_t pixel_count, uint8_t* rgb_out, int device);
/* ImageRgbU8::write_png (image.rs:52-66): 8-bit RGB PNG of `height` rows of `width` pixels
 * (row 0 first).  Host only. */
int vr_write_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height);

/* Upper bound on the staging memory one render call may use (16 B per pixel-sample of a launch;
 * 0 = the default, half of the free HBM).  A call whose tile x spp needs more runs in several
 * launches that continue update_pixel in sample order (bit-identical records).  For a GPU shared
 * with other work, and the tests of the pass split.  Not thread-safe against concurrent render
 * calls on the same scene: set it before rendering (ABI 7). */
int vr_scene_set_staging_limit(vr_scene* scene, uint64_t bytes);

/* Test hook (no reference counterpart): every hit on scene object `object` takes the singular-
 * shading-basis path (VR_ERROR_SINGULAR_BASIS, where simple_random_integrator.rs:26-31 panics),
 * which finite geometry cannot reach; -1 turns it off.  Not thread-safe against concurrent render
 * calls on the same scene: set it before rendering (tests/test_gpu_concurrency.py).  ABI 5. */
int vr_debug_set_fault_object(vr_scene* scene, int32_t object);

/* Test hook: launch flags (VR_LAUNCH_NO_CULL / _NO_DIST_CULL / _NO_COOP / _NO_LONE_WALK only) applied to every render
 * call of the scene, including the host-buffer and per-sample record entry points that take no launch
 * flags of their own; 0 turns them off.  Set before rendering, like the fault object (ABI 8). */
int vr_debug_set_launch_flags(vr_scene* scene, uint32_t flags);
/* 1 when a scene with this many triangles and 4-wide nodes renders with the 64-bit-offset kernels
 * (VR_SCENE_WIDE_OFFSETS), else 0.  Host only, no device (ABI 8). */
int vr_scene_needs_wide_offsets(uint64_t triangle_count, uint64_t wide_node_count);
/* 1 when a launch runs the single-BVH instantiation of the render kernel (VR_VARIANT_ONE_BVH): the
 * scene's BVH list is one BVH whose 4-wide root `root4` is a node (>= 0: not a one-triangle mesh, not an
 * empty one), nothing in `other` (VR_CHOICE_* bits of what else the launch selected) excludes it, and
 * the instantiation exists for the stack class of `stack_depth` entries (16-bit entries: the 24 and 32
 * classes; 32-bit ones: the 32 class).  The library's own choice, exported for the tests. */
#define VR_CHOICE_COUNTING 1u     /* VR_LAUNCH_COUNTERS */
#define VR_CHOICE_RECORD 2u       /* the per-sample record variant (vr_render_samples) */
#define VR_CHOICE_WHITTED 4u      /* the Whitted integrator's kernel */
#define VR_CHOICE_COOP_GATED 8u   /* small enough for the cooperative tail, with or without VR_LAUNCH_NO_COOP */
#define VR_CHOICE_WIDE_OFFSETS 16u /* the 64-bit-offset kernels */
#define VR_CHOICE_MULTI_BVH 32u   /* VR_LAUNCH_MULTI_BVH */
#define VR_CHOICE_OWN_GRIDS 64u   /* one material kind, and the rows' wavelength grids differ (vr_scene_grid_shared bit 0 clear) */
int vr_launch_takes_one_bvh(uint64_t bvh_count, int32_t root4, uint32_t other, int32_t stack_depth, int32_t stack16);
/* 1 when the `count` material rows at `rows` (vr_scene_materials' records) lie on one wavelength grid:
 * shortest, longest, n, inv_step and knots[0..n) equal bit for bit.  vr_scene_grid_shared: the same of
 * the rows of `scene`, kept up to date by the edits: bit 0, its materials and Whitted light rows share a
 * grid; bit 1 (never without bit 0), the sky row lies on it too.  The single-BVH kernels of one material
 * kind, which look a path's wavelength up once, need bit 0 and use bit 1.  Host only (additions under
 * ABI 10). */
int vr_material_grids_shared(const void* rows, uint32_t count);
int vr_scene_grid_shared(const vr_scene* scene);
/* The VR_VARIANT_* bits a render of `pixel_samples` (tile pixels x spp) of `scene` with `launch_flags`
 * would report now (recording: the per-sample record variant).  Launches nothing; host-only scenes too. */
int vr_scene_launch_variant(const vr_scene* scene, uint64_t pixel_samples, uint32_t launch_flags, int32_t recording,
                            uint32_t* variant);

int vr_device_count(void);
const char* vr_last_error(void);
uint32_t vr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VANRIJN_AMD_H */
