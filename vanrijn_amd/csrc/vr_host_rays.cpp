// vr_host_rays.cpp -- the entry points for caller-supplied rays: vr_trace_rays, the ray queries
// (vr_query.hip), the integrators (vr_integrate.hip), camera rays, photon accumulation and the first-hit
// feature buffers (vr_features.hip).
#include "vr_host.h"

using namespace vrh;

int vr_trace_rays(const vr_scene* s, uint64_t n, const double* origins, const double* directions,
                  vr_hit_record* out) {
    if (!s || (n && (!origins || !directions || !out))) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (s->host_only) return host_only_error();
    if (n == 0) return VR_OK;
    HostCall call;
    int rc = call.begin(s);
    if (rc) return rc;
    const hipStream_t st = call.st;
    const size_t in_bytes = n * 3 * sizeof(double), out_bytes = n * sizeof(vr_hit_record);
    const size_t o_o = call.part(in_bytes), o_d = call.part(in_bytes), o_out = call.part(out_bytes);
    rc = call.grow();
    if (rc) return rc;
    char *const d_o = call.at(o_o), *const d_d = call.at(o_d), *const d_out = call.at(o_out);
    VR_HIP(hipMemcpyAsync(d_o, origins, in_bytes, hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(d_d, directions, in_bytes, hipMemcpyHostToDevice, st));
    VR_HIP(hipMemsetAsync(d_out, 0, out_bytes, st));
    vr::TraceArgs a{};
    a.scene = s->dev;
    a.n = n;
    a.origins = (const double*)d_o;
    a.directions = (const double*)d_d;
    a.out = d_out;
    int lr = vr::launch_trace(a, stack_depth(s), st);
    if (lr) return launch_status(lr);
    VR_HIP(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(call.c->done, st));
    VR_HIP(hipStreamSynchronize(st));
    return VR_OK;
}

// ---- ray queries (vr_query.hip) ----
namespace {

// the checks every query entry point makes before its first device call; *go: there is work to do
int query_check(const vr_scene* s, uint64_t n, const void* origins, const void* directions, uint32_t flags,
                const void* out, bool* go) {
    *go = false;
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    if (flags & ~(VR_QUERY_NORMALIZE | VR_QUERY_REFERENCE_WALK))
        return fail(VR_ERROR_INVALID_ARGUMENT, "unknown query flag");
    if (n == 0) return VR_OK;
    if (!origins || !directions || !out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (s->host_only) return host_only_error();
    if (n > UINT64_MAX / sizeof(vr_hit_record)) return fail(VR_ERROR_INVALID_ARGUMENT, "ray count overflows");
    const int depth = (flags & VR_QUERY_REFERENCE_WALK) ? stack_depth(s) : wide_stack_depth(s);
    if (depth > 48) return fail(VR_ERROR_UNSUPPORTED, "BVH deeper than the largest traversal stack (48)");
    *go = true;
    return VR_OK;
}

// enqueue one query launch on `st` (device pointers)
int query_enqueue(const vr_scene* s, uint64_t n, const double* origins, const double* directions, uint32_t flags,
                  bool any, void* hits, void* records, hipStream_t st) {
    vr::QueryArgs a{};
    a.scene = s->dev;
    a.n = n;
    a.origins = origins;
    a.directions = directions;
    a.hits = hits;
    a.records = records;
    a.flags = flags;
    a.any = any ? 1u : 0u;
    const int depth = (flags & VR_QUERY_REFERENCE_WALK) ? stack_depth(s) : wide_stack_depth(s);
    // enough workgroups for every CU's LDS several times over; larger batches take the grid stride
    const int lr = vr::launch_query(a, depth, std::max(1, s->cu_count) * 32, st);
    if (lr) return launch_status(lr);
    return VR_OK;
}

// the host-array forms: inputs and outputs staged through a call context, as vr_trace_rays
int query_host(const vr_scene* s, uint64_t n, const double* origins, const double* directions, uint32_t flags,
               bool any, void* hits, vr_hit_record* records) {
    bool go;
    int rc = query_check(s, n, origins, directions, flags, hits, &go);
    if (rc || !go) return rc;
    HostCall call;
    rc = call.begin(s);
    if (rc) return rc;
    const hipStream_t st = call.st;
    const size_t in_bytes = n * 3 * sizeof(double);
    // (the any-hit bytes: n rounded up to 16; n are copied back)
    const size_t hit_bytes = any ? (size_t)((n + 15) & ~(uint64_t)15) : n * sizeof(vr_ray_hit);
    const size_t rec_bytes = records ? n * sizeof(vr_hit_record) : 0;
    const size_t o_o = call.part(in_bytes), o_d = call.part(in_bytes), o_hits = call.part(hit_bytes),
                 o_rec = call.part(rec_bytes);
    rc = call.grow();
    if (rc) return rc;
    char *const d_o = call.at(o_o), *const d_d = call.at(o_d), *const d_hits = call.at(o_hits);
    char* const d_rec = records ? call.at(o_rec) : nullptr;
    VR_HIP(hipMemcpyAsync(d_o, origins, in_bytes, hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(d_d, directions, in_bytes, hipMemcpyHostToDevice, st));
    rc = query_enqueue(s, n, (const double*)d_o, (const double*)d_d, flags, any, d_hits, d_rec, st);
    if (rc) return rc;
    VR_HIP(hipMemcpyAsync(hits, d_hits, any ? (size_t)n : hit_bytes, hipMemcpyDeviceToHost, st));
    if (records) VR_HIP(hipMemcpyAsync(records, d_rec, rec_bytes, hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(call.c->done, st));
    VR_HIP(hipStreamSynchronize(st));
    return VR_OK;
}

}  // namespace

int vr_query_closest_device(const vr_scene* s, uint64_t n, const double* origins, const double* directions,
                            uint32_t flags, vr_ray_hit* hits, vr_hit_record* records, void* stream) {
    bool go;
    const int rc = query_check(s, n, origins, directions, flags, hits, &go);
    if (rc || !go) return rc;
    VR_HIP(hipSetDevice(s->device));
    return query_enqueue(s, n, origins, directions, flags, false, hits, records, (hipStream_t)stream);
}

int vr_query_any_device(const vr_scene* s, uint64_t n, const double* origins, const double* directions,
                        uint32_t flags, uint8_t* hit, void* stream) {
    bool go;
    const int rc = query_check(s, n, origins, directions, flags, hit, &go);
    if (rc || !go) return rc;
    VR_HIP(hipSetDevice(s->device));
    return query_enqueue(s, n, origins, directions, flags, true, hit, nullptr, (hipStream_t)stream);
}

int vr_query_closest(const vr_scene* s, uint64_t n, const double* origins, const double* directions, uint32_t flags,
                     vr_ray_hit* hits, vr_hit_record* records) {
    return query_host(s, n, origins, directions, flags, false, hits, records);
}

int vr_query_any(const vr_scene* s, uint64_t n, const double* origins, const double* directions, uint32_t flags,
                 uint8_t* hit) {
    return query_host(s, n, origins, directions, flags, true, hit, nullptr);
}

// ---- the integrators for caller-supplied rays (vr_integrate.hip) ----
namespace {

// the checks both integrate entry points make before their first device call; *go: there is work to do
int integrate_check(const vr_scene* s, uint64_t n, const void* origins, const void* directions,
                    const vr_integrate_params* p, const void* photons, bool* go) {
    *go = false;
    if (!s || !p) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or params");
    if (p->flags & ~VR_QUERY_NORMALIZE) return fail(VR_ERROR_INVALID_ARGUMENT, "unknown integrate flag");
    if (n == 0) return VR_OK;
    if (!origins || !directions || !photons) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    // the stream's index space, as check_render_params: (pixel << 32) + sample must not carry.  Compared
    // without forming first_stream + n (it may wrap)
    const uint64_t lim = 1ull << 32;
    if (n > lim || p->first_stream > lim - n)
        return fail(VR_ERROR_UNSUPPORTED, "stream indices past 2^32 (random stream index space)");
    if (p->sample >= lim) return fail(VR_ERROR_UNSUPPORTED, "sample index past 2^32 (random stream index space)");
    if (s->host_only) return host_only_error();
    if (wide_stack_depth(s) > 48) return fail(VR_ERROR_UNSUPPORTED, "BVH deeper than the largest traversal stack (48)");
    *go = true;
    return VR_OK;
}

// enqueue one integrate launch on `st` (device pointers); err: the error word a singular basis sets
int integrate_enqueue(const vr_scene* s, uint64_t n, const double* origins, const double* directions,
                      const double* wavelengths, const uint64_t* stream_ids, const vr_integrate_params* p,
                      vr_photon* photons, vr_path_info* info, int32_t* err, hipStream_t st) {
    vr::IntegrateArgs a{};
    a.scene = s->dev;
    a.n = n;
    a.origins = origins;
    a.directions = directions;
    a.wavelengths = wavelengths;
    a.stream_ids = stream_ids;
    a.seed_key = seed_key_of(p->seed);
    a.first_stream = p->first_stream;
    a.sample = p->sample;
    a.first_draw = p->first_draw;
    a.flags = p->flags;
    a.fault_object = s->fault_object;
    a.error_flag = err;
    a.photons = photons;
    a.info = info;
    const char* g = tuning_env("VR_INTEGRATE_GRID");  // tuning hook: workgroups per CU
    const int per_cu = g ? std::max(1, atoi(g)) : 32;
    const int lr = vr::launch_integrate(a, wide_stack_depth(s), std::max(1, s->cu_count) * per_cu, st);
    if (lr) return launch_status(lr);
    return VR_OK;
}

}  // namespace

int vr_integrate_rays_device(const vr_scene* s, uint64_t n, const double* origins, const double* directions,
                             const double* wavelengths, const uint64_t* stream_ids, const vr_integrate_params* p,
                             vr_photon* photons, vr_path_info* info, void* stream) {
    bool go;
    int rc = integrate_check(s, n, origins, directions, p, photons, &go);
    if (rc || !go) return rc;
    VR_HIP(hipSetDevice(s->device));
    int32_t* slot = nullptr;
    rc = stream_slot(const_cast<vr_scene*>(s), stream, &slot);
    if (rc) return rc;
    return integrate_enqueue(s, n, origins, directions, wavelengths, stream_ids, p, photons, info, slot,
                             (hipStream_t)stream);
}

int vr_integrate_rays(const vr_scene* s, uint64_t n, const double* origins, const double* directions,
                      const double* wavelengths, const uint64_t* stream_ids, const vr_integrate_params* p,
                      vr_photon* photons, vr_path_info* info) {
    bool go;
    int rc = integrate_check(s, n, origins, directions, p, photons, &go);
    if (rc || !go) return rc;
    HostCall call;
    rc = call.begin(s);
    if (rc) return rc;
    CallCtx* c = call.c;
    const hipStream_t st = call.st;
    const size_t in_bytes = n * 3 * sizeof(double), ph_bytes = n * sizeof(vr_photon);
    const size_t o_o = call.part(in_bytes), o_d = call.part(in_bytes), o_ph = call.part(ph_bytes),
                 o_wl = call.part(wavelengths ? n * 8 : 0), o_id = call.part(stream_ids ? n * 8 : 0),
                 o_info = call.part(info ? n * 8 : 0);
    rc = call.grow();
    if (rc) return rc;
    char *const d_o = call.at(o_o), *const d_d = call.at(o_d), *const d_ph = call.at(o_ph), *const d_wl = call.at(o_wl),
               *const d_id = call.at(o_id), *const d_info = call.at(o_info);
    VR_HIP(hipMemcpyAsync(d_o, origins, in_bytes, hipMemcpyHostToDevice, st));
    VR_HIP(hipMemcpyAsync(d_d, directions, in_bytes, hipMemcpyHostToDevice, st));
    if (wavelengths) VR_HIP(hipMemcpyAsync(d_wl, wavelengths, n * 8, hipMemcpyHostToDevice, st));
    if (stream_ids) VR_HIP(hipMemcpyAsync(d_id, stream_ids, n * 8, hipMemcpyHostToDevice, st));
    rc = integrate_enqueue(s, n, (const double*)d_o, (const double*)d_d, wavelengths ? (const double*)d_wl : nullptr,
                           stream_ids ? (const uint64_t*)d_id : nullptr, p, (vr_photon*)d_ph,
                           info ? (vr_path_info*)d_info : nullptr, c->error, st);
    if (rc) return rc;
    VR_HIP(hipMemcpyAsync(photons, d_ph, ph_bytes, hipMemcpyDeviceToHost, st));
    if (info) VR_HIP(hipMemcpyAsync(info, d_info, n * 8, hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(c->done, st));
    return read_and_clear_error(c->error, st);
}

int vr_accumulate_photons_device(double* state, const vr_photon* photons, uint64_t pixel_count, uint32_t spp,
                                 uint32_t accumulate, int32_t device, void* stream) {
    if (pixel_count == 0) return VR_OK;
    if (!state || !photons) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (pixel_count > (1ull << 32)) return fail(VR_ERROR_UNSUPPORTED, "more than 2^32 pixels in one call");
    VR_HIP(hipSetDevice(device));
    const int lr = vr::launch_accumulate(state, (const double*)photons, pixel_count, spp, accumulate, stream);
    if (lr) return fail(VR_ERROR_DEVICE, vr::device_error_string(lr));
    return VR_OK;
}

int vr_camera_rays_device(const vr_scene* s, const vr_render_params* p, double* origins, double* directions,
                          uint64_t* stream_ids, void* stream) {
    int rc = check_render_params(s, p);
    if (rc) return rc;
    const uint64_t tw = p->tile.end_column - p->tile.start_column, th = p->tile.end_row - p->tile.start_row;
    if (tw * th == 0 || p->spp == 0) return VR_OK;
    if (!origins || !directions || !stream_ids) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (tw * th > (1ull << 38) / p->spp) return fail(VR_ERROR_UNSUPPORTED, "too many rays in one call (2^38)");
    VR_HIP(hipSetDevice(s->device));
    const vr::RenderArgs r = make_args(s, p, nullptr);
    vr::CameraRaysArgs a{};
    for (int k = 0; k < 3; ++k) a.camera[k] = s->dev.camera[k];
    a.pose = s->pose;
    a.lens = s->lens;
    a.start_column = r.start_column;
    a.start_row = r.start_row;
    a.tile_width = r.tile_width;
    a.tile_height = r.tile_height;
    a.width = r.width;
    a.height = r.height;
    a.seed_key = r.seed_key;
    a.first_sample = r.first_sample;
    a.spp = r.spp;
    for (int k = 0; k < 4; ++k) a.film[k] = r.film[k];
    a.origins = origins;
    a.directions = directions;
    a.stream_ids = stream_ids;
    const int lr = vr::launch_camera_rays(a, stream);
    if (lr) return fail(VR_ERROR_DEVICE, vr::device_error_string(lr));
    return VR_OK;
}

// ---- feature buffers (vr_features.hip) ----
namespace {

// the checks both feature entry points make before their first device call; *go: there is work to do
int features_check(const vr_scene* s, const vr_render_params* p, const void* features, const void* albedo, bool* go) {
    *go = false;
    if (!s || !p) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene or params");
    if (!features && !albedo) return fail(VR_ERROR_INVALID_ARGUMENT, "both feature outputs are null");
    if (p->accumulate > 1) return fail(VR_ERROR_INVALID_ARGUMENT, "accumulate must be 0 or 1");
    const int rc = check_render_params(s, p);  // host-only, the tile, the 2^32 limits, the stack depth
    if (rc) return rc;
    const uint64_t tw = p->tile.end_column - p->tile.start_column, th = p->tile.end_row - p->tile.start_row;
    if (tw * th == 0 || p->spp == 0) return VR_OK;
    // one wave per 8x8 block, four per workgroup: the block index is 32-bit
    if (((tw + 7) / 8) * ((th + 7) / 8) >= (1ull << 31))
        return fail(VR_ERROR_UNSUPPORTED, "too many pixel blocks in one launch (2^31)");
    *go = true;
    return VR_OK;
}

// enqueue the feature pass on `st` (device pointers)
int features_enqueue(const vr_scene* s, const vr_render_params* p, void* features, double* albedo, hipStream_t st) {
    const vr::RenderArgs r = make_args(s, p, nullptr);
    vr::FeaturesArgs a{};
    a.scene = s->dev;
    a.pose = s->pose;
    a.lens = s->lens;
    a.start_column = r.start_column;
    a.start_row = r.start_row;
    a.tile_width = r.tile_width;
    a.tile_height = r.tile_height;
    a.width = r.width;
    a.height = r.height;
    a.seed_key = r.seed_key;
    a.first_sample = r.first_sample;
    a.spp = r.spp;
    a.accumulate = r.accumulate;
    a.blocks_per_row = (uint32_t)((r.tile_width + 7) / 8);
    a.block_count = (uint32_t)(((r.tile_width + 7) / 8) * ((r.tile_height + 7) / 8));
    for (int k = 0; k < 4; ++k) a.film[k] = r.film[k];
    a.features = features;
    a.albedo_state = albedo;
    const int lr = vr::launch_features(a, wide_stack_depth(s), st);
    if (lr) return launch_status(lr);
    return VR_OK;
}

}  // namespace

int vr_render_features_device(const vr_scene* s, const vr_render_params* p, vr_pixel_features* features,
                              double* albedo_state, void* stream) {
    bool go;
    const int rc = features_check(s, p, features, albedo_state, &go);
    if (rc || !go) return rc;
    VR_HIP(hipSetDevice(s->device));
    return features_enqueue(s, p, features, albedo_state, (hipStream_t)stream);
}

int vr_render_features(const vr_scene* s, const vr_render_params* p, vr_pixel_features* features, double* albedo_state) {
    bool go;
    int rc = features_check(s, p, features, albedo_state, &go);
    if (rc || !go) return rc;
    HostCall call;
    rc = call.begin(s);
    if (rc) return rc;
    const hipStream_t st = call.st;
    const uint64_t npix = (p->tile.end_column - p->tile.start_column) * (p->tile.end_row - p->tile.start_row);
    const size_t f_bytes = features ? npix * sizeof(vr_pixel_features) : 0, a_bytes = albedo_state ? npix * 64 : 0;
    const size_t o_f = call.part(f_bytes), o_a = call.part(a_bytes);
    rc = call.grow();
    if (rc) return rc;
    char* const d_f = features ? call.at(o_f) : nullptr;
    char* const d_a = albedo_state ? call.at(o_a) : nullptr;
    if (p->accumulate) {  // continue from the caller's records
        if (features) VR_HIP(hipMemcpyAsync(d_f, features, f_bytes, hipMemcpyHostToDevice, st));
        if (albedo_state) VR_HIP(hipMemcpyAsync(d_a, albedo_state, a_bytes, hipMemcpyHostToDevice, st));
    }
    rc = features_enqueue(s, p, d_f, (double*)d_a, st);
    if (rc) return rc;
    if (features) VR_HIP(hipMemcpyAsync(features, d_f, f_bytes, hipMemcpyDeviceToHost, st));
    if (albedo_state) VR_HIP(hipMemcpyAsync(albedo_state, d_a, a_bytes, hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(call.c->done, st));
    VR_HIP(hipStreamSynchronize(st));
    return VR_OK;
}

int vr_camera_lens_point(double lu, double lv, double out[2]) {
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    vr::camera::lens_disc(lu, lv, &out[0], &out[1]);
    return VR_OK;
}

int vr_camera_lens_ray(const vr_camera_pose* pose, const vr_camera_lens* lens, uint64_t width, uint64_t height, uint64_t row,
                       uint64_t column, double ux, double uy, double lu, double lv, double origin[3], double direction[3]) {
    if (!pose || !lens || !origin || !direction) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    // no lens: the pinhole ray, whose origin is the location's bits
    if (lens->lens_radius == 0.0) return vr_camera_ray(pose, width, height, row, column, ux, uy, origin, direction);
    if (width == 0 || height == 0 || row >= height || column >= width)
        return fail(VR_ERROR_INVALID_ARGUMENT, "camera ray: the pixel is outside the image");
    double film[4];
    vr::camera::film_constants(width, height, film);
    const double l[3] = {pose->location.x, pose->location.y, pose->location.z};
    const double r[3] = {pose->right.x, pose->right.y, pose->right.z}, u[3] = {pose->up.x, pose->up.y, pose->up.z};
    const double f[3] = {pose->forward.x, pose->forward.y, pose->forward.z};
    vr::camera::Vec o, d;
    vr::camera::lens_ray(l, r, u, f, pose->film_distance, lens->lens_radius, lens->focus_distance,
                         vr::camera::film_x(film, column, ux), vr::camera::film_y(film, height, row, uy), lu, lv, &o, &d);
    origin[0] = o.x;
    origin[1] = o.y;
    origin[2] = o.z;
    direction[0] = d.x;
    direction[1] = d.y;
    direction[2] = d.z;
    return VR_OK;
}
