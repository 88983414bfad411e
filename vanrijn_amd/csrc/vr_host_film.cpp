// vr_host_film.cpp -- the display end and the film: merge_tile on the host and as a device-resident
// AccumulationBuffer, the tone map, vr_resolve_state.
//   AccumulationBuffer::merge_tile                src/accumulation_buffer.rs:62-91 (host, and the device film)
#include "vr_host.h"

using namespace vrh;

int vr_merge_tile(vr_accumulation_buffer* dst, vr_tile t, const vr_accumulation_buffer* src) {
    if (!dst || !src || !dst->colour || !dst->weight || !src->colour || !src->weight)
        return fail(VR_ERROR_INVALID_ARGUMENT, "null buffer");
    // accumulation_buffer.rs:63-64 assert the tile size; Array2D indexing asserts the bounds
    if (t.end_column < t.start_column || t.end_row < t.start_row || t.end_column > dst->width ||
        t.end_row > dst->height || src->width != t.end_column - t.start_column ||
        src->height != t.end_row - t.start_row)
        return fail(VR_ERROR_INVALID_ARGUMENT, "merge_tile: tile does not match the buffers");
    // blend (accumulation_buffer.rs:87-91) per pixel; rows are independent, so a large tile is
    // split into row bands over host threads (96 B of memory traffic per pixel: one core merged
    // a 1024^2 frame in ~5 ms, the bottleneck of main.rs's one merging thread)
    auto rows = [&](uint64_t r0, uint64_t r1) {
        for (uint64_t i = r0; i < r1; ++i) {
            for (uint64_t j = 0; j < src->width; ++j) {
                const uint64_t d = (t.start_row + i) * dst->width + (t.start_column + j), q = i * src->width + j;
                const double w1 = dst->weight[d], w2 = src->weight[q];
                const double inv = 1.0 / (w1 + w2);
                for (int k = 0; k < 3; ++k)
                    dst->colour[3 * d + k] = (dst->colour[3 * d + k] * w1 + src->colour[3 * q + k] * w2) * inv;
                dst->weight[d] = w1 + w2;
            }
        }
    };
    parallel_range(src->height, std::max<uint64_t>(1, ((uint64_t)1 << 16) / std::max<uint64_t>(1, src->width)), rows);
    return VR_OK;
}

int vr_resolve_state(const double* state, uint64_t pixel_count, double* colour) {
    if (!state || !colour) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    for (uint64_t i = 0; i < pixel_count; ++i) {  // the sums half of the records (vr_layout.h)
        const double w = state[4 * i + 3];
        const double inv = 1.0 / w;
        for (int k = 0; k < 3; ++k) colour[3 * i + k] = w != 0.0 ? state[4 * i + k] * inv : 0.0;
    }
    return VR_OK;
}

// ---------------------------------------------------------------------------------------------
// Display end: ClampingToneMapper over ColourXyz::to_srgb (image.rs:166-187,
// colour_xyz.rs:49-84) on the device, ImageRgbU8::write_png (image.rs:52-66) on the host.
// ---------------------------------------------------------------------------------------------
int vr_tone_map_device(const double* state, uint64_t pixel_count, uint8_t* rgb_out, int device, void* stream) {
    if (!state || !rgb_out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    VR_HIP(hipSetDevice(device));
    const int e = vr::launch_tonemap(state, 1, pixel_count, rgb_out, stream);
    if (e) return device_fail(e, "tonemap launch failed");
    return VR_OK;
}

int vr_tone_map(const double* colour, uint64_t pixel_count, uint8_t* rgb_out, int device) {
    if (!colour || !rgb_out) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (pixel_count == 0) return VR_OK;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(VR_ERROR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= n) return fail(VR_ERROR_INVALID_ARGUMENT, "device out of range");
    VR_HIP(hipSetDevice(device));
    CallScratch cs;
    VR_HIP(hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking));
    const size_t in_b = (size_t)pixel_count * 3 * sizeof(double), out_b = (size_t)pixel_count * 3;
    VR_HIP(hipMalloc(&cs.ptr, in_b + out_b));
    double* d_in = (double*)cs.ptr;
    uint8_t* d_out = (uint8_t*)cs.ptr + in_b;
    VR_HIP(hipMemcpyAsync(d_in, colour, in_b, hipMemcpyHostToDevice, cs.stream));
    const int e = vr::launch_tonemap(d_in, 0, pixel_count, d_out, cs.stream);
    if (e) return device_fail(e, "tonemap launch failed");
    VR_HIP(hipMemcpyAsync(rgb_out, d_out, out_b, hipMemcpyDeviceToHost, cs.stream));
    VR_HIP(hipStreamSynchronize(cs.stream));
    return VR_OK;
}

// ---------------------------------------------------------------------------------------------
// Film: the reference's full-image AccumulationBuffer (accumulation_buffer.rs:6-12) as a device
// object -- main.rs:197-243's pattern (workers render 1-spp tiles, merge_tile folds each into the
// image, to_image_rgb_u8 displays it) without a host buffer ("Film").
//
// Order rule: merge_tile is not commutative in floating point, so the film's merges and snapshots
// are serialised in the order their calls pass `mutex`.  Under it a step takes its index, makes its
// stream wait on `order` (the event recorded after the previous step), enqueues its kernel and
// re-records `order` on its stream; the lock is held for those three enqueues only.  Renders are
// not ordered: every call renders on its own call context before it takes the lock.
// ---------------------------------------------------------------------------------------------
struct vr_film {
    int device = -1;
    uint64_t width = 0, height = 0;
    double* pixels = nullptr;      // 32 B per pixel {colour X, Y, Z, weight}, row-major
    void* snap = nullptr;          // a host snapshot's staging (32 B per pixel): planar colour | weight, or RGB bytes
    hipStream_t stream = nullptr;  // snapshots to the host, clear
    hipEvent_t order = nullptr;    // recorded after the last merge or snapshot kernel enqueued
    std::mutex mutex;              // the merge order: index, wait on `order`, enqueue, re-record
    std::mutex snap_mutex;         // one host snapshot at a time (they share `snap`); taken before `mutex`
    uint64_t next_index = 0;
};

namespace {
// One ordered step of the film on stream `st`; the caller holds f->mutex.  Whatever `launch` enqueued
// is ordered before the next step even when it failed half-way (`order` is re-recorded regardless).
int film_step(vr_film* f, hipStream_t st, const char* what, const std::function<int()>& launch) {
    VR_HIP(hipStreamWaitEvent(st, f->order, 0));
    const int e = launch();
    const hipError_t r = hipEventRecord(f->order, st);
    if (e || r != hipSuccess) return device_fail(e ? e : (int)r, what);
    return VR_OK;
}

int film_tile_check(const vr_film* f, const vr_tile& t) {
    // as vr_merge_tile: inverted ranges and tiles outside the image are errors, empty ones merge nothing
    if (t.end_column < t.start_column || t.end_row < t.start_row || t.end_column > f->width || t.end_row > f->height)
        return fail(VR_ERROR_INVALID_ARGUMENT, "film: tile outside the film");
    return VR_OK;
}

void film_free(vr_film* f) {
    if (f->order) (void)hipEventDestroy(f->order);
    if (f->stream) (void)hipStreamDestroy(f->stream);
    if (f->pixels) (void)hipFree(f->pixels);
    if (f->snap) (void)hipFree(f->snap);
    delete f;
}

}  // namespace

int vr_film_create(uint64_t width, uint64_t height, int32_t device, vr_film** out) {
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "null output");
    *out = nullptr;
    if (width == 0 || height == 0) return fail(VR_ERROR_INVALID_ARGUMENT, "film: zero width or height");
    if (width > (1ull << 32) || height > (1ull << 32) || width * height > (1ull << 32))
        return fail(VR_ERROR_UNSUPPORTED, "film of more than 2^32 pixels (random stream index space)");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(VR_ERROR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(VR_ERROR_INVALID_ARGUMENT, "device out of range");
    VR_HIP(hipSetDevice(device));
    vr_film* f = new (std::nothrow) vr_film();
    if (!f) return fail(VR_ERROR_OUT_OF_MEMORY, "film allocation failed");
    f->device = device;
    f->width = width;
    f->height = height;
    const size_t bytes = (size_t)(width * height) * 32;
    hipError_t e = hipMalloc((void**)&f->pixels, bytes);
    if (e == hipSuccess) e = hipMalloc(&f->snap, bytes);
    if (e != hipSuccess) {
        film_free(f);
        return fail(VR_ERROR_OUT_OF_MEMORY, std::string("film: ") + hipGetErrorString(e));
    }
    e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&f->order, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMemsetAsync(f->pixels, 0, bytes, f->stream);  // AccumulationBuffer::new
    if (e == hipSuccess) e = hipEventRecord(f->order, f->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
    if (e != hipSuccess) {
        film_free(f);
        return fail(VR_ERROR_DEVICE, std::string("film: ") + hipGetErrorString(e));
    }
    *out = f;
    return VR_OK;
}

void vr_film_destroy(vr_film* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    (void)hipEventSynchronize(f->order);  // the last merge or snapshot, on whatever stream
    (void)hipStreamSynchronize(f->stream);
    film_free(f);
}

int vr_film_clear(vr_film* f) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    VR_HIP(hipSetDevice(f->device));
    std::lock_guard<std::mutex> g(f->mutex);
    f->next_index = 0;
    return film_step(f, f->stream, "film clear", [&] {
        return (int)hipMemsetAsync(f->pixels, 0, (size_t)(f->width * f->height) * 32, f->stream);
    });
}

// vr_render_tile with the film as its destination: render into the call context's records, then
// merge_tile on the device.  No host round trip lies between the two: the merge kernel reads the
// call's error word and leaves the film alone when the render set it.
int vr_film_render_tile(vr_film* f, const vr_scene* s, const vr_render_params* p, vr_film_merge* info) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    int rc = check_render_params(s, p);
    if (rc) return rc;
    if (p->width != f->width || p->height != f->height)
        return fail(VR_ERROR_INVALID_ARGUMENT, "film: params height / width differ from the film's");
    if (p->accumulate) return fail(VR_ERROR_INVALID_ARGUMENT, "film: accumulate must be 0 (the tile buffer is always fresh)");
    if (s->device != f->device) return fail(VR_ERROR_INVALID_ARGUMENT, "film and scene are on different devices");
    const uint64_t tw = p->tile.end_column - p->tile.start_column, th = p->tile.end_row - p->tile.start_row;
    const uint64_t n = tw * th;
    if (info) info->first_sample = p->first_sample;
    if (n == 0) {  // a merge of no pixels
        std::lock_guard<std::mutex> g(f->mutex);
        if (info) info->merge_index = f->next_index;
        ++f->next_index;
        return VR_OK;
    }
    // (the film's device is the scene's); `done` is recorded after the merge, the last reader of the
    // context's records, on every exit
    HostCall call;
    rc = call.begin(s);
    if (rc) return rc;
    CallCtx* c = call.c;
    const hipStream_t st = call.st;
    const size_t o_state = call.part((size_t)n * 64);
    rc = call.grow();
    if (rc) return rc;
    rc = ctx_grow_pinned(c, 256);  // the call's error word
    if (rc) return rc;
    double* state = (double*)call.at(o_state);
    VR_HIP(hipMemsetAsync(state, 0, n * 64, st));  // AccumulationBuffer::new
    rc = enqueue_passes(const_cast<vr_scene*>(s), c, p, state, st, c->error, false, false, nullptr, nullptr, nullptr);
    if (rc) return rc;
    {
        std::lock_guard<std::mutex> g(f->mutex);
        if (info) info->merge_index = f->next_index;
        ++f->next_index;
        rc = film_step(f, st, "film merge", [&] {
            return vr::launch_film_merge(f->pixels, f->width, p->tile.start_column, p->tile.start_row, tw, th, state,
                                         c->error, st);
        });
    }
    if (rc) return rc;
    volatile int32_t* flag = (volatile int32_t*)c->pinned;
    VR_HIP(hipMemcpyAsync((void*)flag, c->error, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    VR_HIP(hipEventRecord(c->done, st));
    VR_HIP(hipEventSynchronize(c->done));
    if (*flag) {  // the merge kernel saw the same word and returned early
        const int32_t bits = *flag;
        VR_HIP(hipMemsetAsync(c->error, 0, sizeof(int32_t), st));
        VR_HIP(hipStreamSynchronize(st));
        return error_status(bits);
    }
    return VR_OK;
}

int vr_film_partial_render_scene(vr_film* f, const vr_scene* s, vr_tile tile, vr_film_merge* info) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    if (!s) return fail(VR_ERROR_INVALID_ARGUMENT, "null scene");
    vr_render_params p{};
    p.tile = tile;
    p.height = f->height;
    p.width = f->width;
    p.spp = 1;
    p.accumulate = 0;
    p.seed = s->partial_seed;
    p.first_sample = const_cast<vr_scene*>(s)->pass_counter.fetch_add(1);  // as vr_partial_render_scene
    return vr_film_render_tile(f, s, &p, info);
}

int vr_film_merge_state(vr_film* f, vr_tile t, const double* state, void* stream, vr_film_merge* info) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    if (!state) return fail(VR_ERROR_INVALID_ARGUMENT, "null state");
    if ((uintptr_t)state & 15) return fail(VR_ERROR_INVALID_ARGUMENT, "film: state records must be 16-byte aligned");
    const int rc = film_tile_check(f, t);
    if (rc) return rc;
    if (info) info->first_sample = 0;
    const uint64_t tw = t.end_column - t.start_column, th = t.end_row - t.start_row;
    if (tw * th) VR_HIP(hipSetDevice(f->device));
    std::lock_guard<std::mutex> g(f->mutex);
    if (info) info->merge_index = f->next_index;
    ++f->next_index;
    if (tw * th == 0) return VR_OK;
    return film_step(f, (hipStream_t)stream, "film merge", [&] {
        return vr::launch_film_merge(f->pixels, f->width, t.start_column, t.start_row, tw, th, state, nullptr, stream);
    });
}

int vr_film_read(vr_film* f, vr_accumulation_buffer* out, uint64_t* merges_seen) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    if (!out || !out->colour || !out->colour_sum || !out->colour_bias || !out->weight || !out->weight_bias)
        return fail(VR_ERROR_INVALID_ARGUMENT, "null accumulation buffer");
    if (out->width != f->width || out->height != f->height)
        return fail(VR_ERROR_INVALID_ARGUMENT, "accumulation buffer does not match the film");
    VR_HIP(hipSetDevice(f->device));
    const uint64_t n = f->width * f->height;
    double* planar = (double*)f->snap;
    std::lock_guard<std::mutex> sg(f->snap_mutex);
    {
        std::lock_guard<std::mutex> g(f->mutex);
        if (merges_seen) *merges_seen = f->next_index;
        const int rc = film_step(f, f->stream, "film export",
                                 [&] { return vr::launch_film_export(f->pixels, n, planar, f->stream); });
        if (rc) return rc;
    }
    // later merges wait for the export kernel only; the copies read the staging, not the film
    VR_HIP(hipMemcpyAsync(out->colour, planar, n * 3 * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    VR_HIP(hipMemcpyAsync(out->weight, planar + 3 * n, n * sizeof(double), hipMemcpyDeviceToHost, f->stream));
    // merge_tile never touches these three (accumulation_buffer.rs:62-85)
    std::memset(out->colour_sum, 0, n * 3 * sizeof(double));
    std::memset(out->colour_bias, 0, n * 3 * sizeof(double));
    std::memset(out->weight_bias, 0, n * sizeof(double));
    VR_HIP(hipStreamSynchronize(f->stream));
    return VR_OK;
}

int vr_film_to_image_rgb_u8(vr_film* f, uint8_t* rgb, uint64_t* merges_seen) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    if (!rgb) return fail(VR_ERROR_INVALID_ARGUMENT, "null output");
    VR_HIP(hipSetDevice(f->device));
    const uint64_t n = f->width * f->height;
    uint8_t* bytes = (uint8_t*)f->snap;
    std::lock_guard<std::mutex> sg(f->snap_mutex);
    {
        std::lock_guard<std::mutex> g(f->mutex);
        if (merges_seen) *merges_seen = f->next_index;
        const int rc = film_step(f, f->stream, "film tone map",
                                 [&] { return vr::launch_tonemap(f->pixels, 2, n, bytes, f->stream); });
        if (rc) return rc;
    }
    VR_HIP(hipMemcpyAsync(rgb, bytes, n * 3, hipMemcpyDeviceToHost, f->stream));
    VR_HIP(hipStreamSynchronize(f->stream));
    return VR_OK;
}

int vr_film_to_image_rgb_u8_device(vr_film* f, uint8_t* rgb, void* stream, uint64_t* merges_seen) {
    if (!f) return fail(VR_ERROR_INVALID_ARGUMENT, "null film");
    if (!rgb) return fail(VR_ERROR_INVALID_ARGUMENT, "null output");
    VR_HIP(hipSetDevice(f->device));
    std::lock_guard<std::mutex> g(f->mutex);
    if (merges_seen) *merges_seen = f->next_index;
    return film_step(f, (hipStream_t)stream, "film tone map",
                     [&] { return vr::launch_tonemap(f->pixels, 2, f->width * f->height, rgb, stream); });
}

