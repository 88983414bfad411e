// vr_host_io.cpp -- the HIP-free entry points: the last error, the ABI version, the reference's
// colour functions, its host threads (parallel_range / parallel_copy), load_obj and write_png.
//   Spectrum::reflection_from_linear_rgb / intensity_at_wavelength   src/colour/spectrum.rs:64-165
//   ColourXyz::for_wavelength                     src/colour/colour_xyz.rs:22-29, 86-103
//   load_obj                                      src/mesh.rs:13-88
#define VR_HOST_NO_HIP
#include "vr_host.h"

#include <sched.h>
#include <zlib.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

#include "rgb_spectrum_tables.h"

using namespace vrh;

static thread_local std::string g_last_error;

int vrh::fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

// ---------------------------------------------------------------------------------------------
// Host threads for the host-buffer entry points: copying the AccumulationBuffer arrays between
// page-locked staging and the caller's memory, and vr_merge_tile.  88 B per pixel of host memory
// traffic is ~5 ms per 1024^2 frame on one core -- more than the GPU's share of a 1-spp render.
// ---------------------------------------------------------------------------------------------
// the CPUs this process may run on (sched affinity), at most 16 (VR_HOST_THREADS overrides in
// tuning builds)
static unsigned host_threads() {
    static const unsigned n = [] {
        unsigned c = 0;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof set, &set) == 0) c = (unsigned)CPU_COUNT(&set);
        if (c == 0) c = std::thread::hardware_concurrency();
        if (const char* e = tuning_env("VR_HOST_THREADS")) c = (unsigned)atoi(e);
        return std::max(1u, std::min(c, 16u));
    }();
    return n;
}

// A persistent pool: run(parts, fn) calls fn(0..parts-1) on the pool's threads and the caller's,
// and returns when all parts are done.  Concurrent callers share the pool (jobs queue FIFO; each
// caller also works on its own job, so a busy pool never blocks progress).
class HostPool {
  public:
    static HostPool& get() {
        static HostPool* p = new HostPool(host_threads() - 1);  // never destroyed: threads idle at exit
        return *p;
    }
    void run(unsigned parts, const std::function<void(unsigned)>& fn) {
        if (parts == 0) return;
        Job j;
        j.fn = &fn;
        j.parts = parts;
        if (parts > 1 && !threads_.empty()) {
            std::lock_guard<std::mutex> g(m_);
            jobs_.push_back(&j);
            cv_.notify_all();
        }
        for (unsigned i; (i = j.next.fetch_add(1)) < parts;) {
            fn(i);
            j.done.fetch_add(1);
        }
        std::unique_lock<std::mutex> l(m_);
        for (auto it = jobs_.begin(); it != jobs_.end(); ++it)
            if (*it == &j) {
                jobs_.erase(it);
                break;
            }
        done_cv_.wait(l, [&] { return j.done.load() == parts; });
    }

  private:
    struct Job {
        const std::function<void(unsigned)>* fn = nullptr;
        unsigned parts = 0;
        std::atomic<unsigned> next{0}, done{0};
    };
    explicit HostPool(unsigned n) {
        for (unsigned i = 0; i < n; ++i) threads_.emplace_back([this] { work(); });
    }
    void work() {
        std::unique_lock<std::mutex> l(m_);
        while (true) {
            cv_.wait(l, [&] { return !jobs_.empty(); });
            Job* j = jobs_.front();
            const unsigned i = j->next.fetch_add(1);
            if (i >= j->parts) {  // every part taken: the job leaves the queue
                jobs_.pop_front();
                continue;
            }
            l.unlock();
            (*j->fn)(i);
            const bool last = j->done.fetch_add(1) + 1 == j->parts;
            l.lock();
            if (last) done_cv_.notify_all();
        }
    }
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::deque<Job*> jobs_;
    std::vector<std::thread> threads_;
};

// fn(begin, end) over [0, n) in about `host_threads()` pieces of at least `grain`
void vrh::parallel_range(uint64_t n, uint64_t grain, const std::function<void(uint64_t, uint64_t)>& fn) {
    const uint64_t pieces = std::max<uint64_t>(1, std::min<uint64_t>(host_threads(), n / std::max<uint64_t>(1, grain)));
    if (pieces <= 1) {
        fn(0, n);
        return;
    }
    const uint64_t step = (n + pieces - 1) / pieces;
    HostPool::get().run((unsigned)pieces, [&](unsigned i) {
        const uint64_t b = std::min(n, (uint64_t)i * step), e = std::min(n, b + step);
        if (b < e) fn(b, e);
    });
}

// copy `bytes` in parallel (host memory bandwidth, not one core's)
void vrh::parallel_copy(void* dst, const void* src, size_t bytes) {
    parallel_range(bytes, (size_t)1 << 20, [&](uint64_t b, uint64_t e) {
        std::memcpy((char*)dst + b, (const char*)src + b, e - b);
    });
}

extern "C" {

uint32_t vr_abi_version(void) { return VR_ABI_VERSION; }

const char* vr_last_error(void) { return g_last_error.c_str(); }

int vr_spectrum_reflection_from_linear_rgb(double red, double green, double blue, double out[32]) {
    if (!out) return fail(VR_ERROR_INVALID_ARGUMENT, "null output");
    const double r = red, g = green, b = blue;
    double c0, c1, c2;
    int kx, ky;
    if (r <= g && r <= b) {
        if (g <= b) { c0 = r; c1 = g - r; c2 = b - g; kx = VR_RGBSPEC_CYAN; ky = VR_RGBSPEC_BLUE; }
        else { c0 = r; c1 = b - r; c2 = g - b; kx = VR_RGBSPEC_CYAN; ky = VR_RGBSPEC_GREEN; }
    } else if (g <= r && g < b) {
        if (r <= b) { c0 = g; c1 = r - g; c2 = b - r; kx = VR_RGBSPEC_MAGENTA; ky = VR_RGBSPEC_BLUE; }
        else { c0 = g; c1 = b - g; c2 = r - b; kx = VR_RGBSPEC_MAGENTA; ky = VR_RGBSPEC_RED; }
    } else {
        if (r <= g) { c0 = b; c1 = r - b; c2 = g - r; kx = VR_RGBSPEC_YELLOW; ky = VR_RGBSPEC_GREEN; }
        else { c0 = b; c1 = g - b; c2 = r - g; kx = VR_RGBSPEC_YELLOW; ky = VR_RGBSPEC_RED; }
    }
    for (int i = 0; i < 32; ++i)
        out[i] = c0 * vr_rgbspec_basis[VR_RGBSPEC_WHITE][i] + c1 * vr_rgbspec_basis[kx][i] +
                 c2 * vr_rgbspec_basis[ky][i];
    return VR_OK;
}

double vr_spectrum_intensity_at_wavelength(const vr_spectrum* sp, double wl) {
    if (!sp || sp->sample_count < 1) return 0.0;
    if (wl < sp->shortest_wavelength || wl > sp->longest_wavelength) return 0.0;
    const int n = (int)sp->sample_count;
    const double range = sp->longest_wavelength - sp->shortest_wavelength;
    const size_t i = (size_t)((double)(n - 1) * ((wl - sp->shortest_wavelength) / range));
    const double before = (double)i / (double)(n - 1) * range + sp->shortest_wavelength;
    if (i == (size_t)(n - 1)) return sp->samples[i];
    const double after = (double)(i + 1) / (double)(n - 1) * range + sp->shortest_wavelength;
    const double delta = after - before;
    const double ratio = (wl - before) / delta;
    return sp->samples[i] * (1.0 - ratio) + sp->samples[i + 1] * ratio;
}

static double gaussian_h(double wl, double alpha, double mu, double s1, double s2) {
    double s = wl < mu ? s1 : s2;
    double denominator = 2.0 * (s * s);
    double t = wl - mu;
    return alpha * std::exp(-(t * t) / denominator);
}

void vr_colour_xyz_for_wavelength(double wl, double out[3]) {
    out[0] = gaussian_h(wl, 1.056, 599.8, 37.9, 31.0) + gaussian_h(wl, 0.362, 442.0, 16.0, 26.7) +
             gaussian_h(wl, -0.065, 501.1, 20.4, 26.2);
    out[1] = gaussian_h(wl, 0.821, 568.8, 46.9, 40.5) + gaussian_h(wl, 0.286, 530.9, 16.3, 31.1);
    out[2] = gaussian_h(wl, 1.217, 437.0, 11.8, 36.0) + gaussian_h(wl, 0.681, 459.0, 26.0, 13.8);
}

// mesh::load_obj (src/mesh.rs:13-88) over the obj 0.9 crate's parsing: "v x y z" and
// "vn x y z" as f32 (correctly rounded strtof) widened to f64, "f a b c ..." with a, a/t,
// a//n or a/t/n corners (1-based, negative = relative), fan triangles (v0, v_i, v_{i+1}).
// groups != nullptr (vr_load_obj_groups): per triangle the number of the usemtl name in force at its
// face, names in order of first appearance ("" for faces before any usemtl, listed only if there are any)
static int load_obj_impl(const char* path, uint64_t* triangle_count, double** vertices, double** normals,
                         std::vector<uint32_t>* groups, std::vector<std::string>* names) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(VR_ERROR_IO, std::string("cannot open ") + path);
    std::vector<float> pos, nrm;
    size_t tex_count = 0;
    struct Corner {
        int64_t v, n;
    };
    std::vector<double> vout, nout;
    std::vector<Corner> poly;
    char* line = nullptr;
    size_t cap = 0;
    int64_t lineno = 0;
    int64_t current = -1;  // the group of the faces that follow; -1: the name in force is not numbered yet
    std::string in_force;  // "" before any usemtl
    // obj 0.9: 1-based indices, negative = relative to the elements read so far, 0 invalid
    auto resolve = [](long long idx, size_t count) -> int64_t {
        if (idx > 0) return (int64_t)idx - 1;
        if (idx < 0) return (int64_t)count + idx;
        return -1;
    };
    auto is_space = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\f' || c == '\v'; };
    // exactly `n` f32 fields (Rust's correctly rounded str::parse::<f32>, here strtof), then an
    // optional extra field (the w of "v x y z w") and the end of the line
    auto floats = [&](char* e, float* out, int n, int max_fields) -> bool {
        int got = 0;
        while (true) {
            while (*e && is_space(*e)) ++e;
            if (*e == '\0' || *e == '#') break;
            char* q;
            const float v = std::strtof(e, &q);
            if (q == e || (*q && !is_space(*q) && *q != '#')) return false;
            if (got < n) out[got] = v;
            ++got;
            e = q;
        }
        return got >= n && got <= max_fields;
    };
    int status = VR_OK;
    std::string err;
    while (getline(&line, &cap, f) != -1) {
        ++lineno;
        char* s = line;
        while (*s == ' ' || *s == '\t') ++s;
        if (s[0] == 'v' && is_space(s[1])) {
            float xyz[3];
            if (!floats(s + 1, xyz, 3, 4)) {
                status = VR_ERROR_IO;
                err = "malformed vertex at line " + std::to_string(lineno);
                break;
            }
            pos.insert(pos.end(), xyz, xyz + 3);
        } else if (s[0] == 'v' && s[1] == 'n' && is_space(s[2])) {
            float xyz[3];
            if (!floats(s + 2, xyz, 3, 3)) {
                status = VR_ERROR_IO;
                err = "malformed normal at line " + std::to_string(lineno);
                break;
            }
            nrm.insert(nrm.end(), xyz, xyz + 3);
        } else if (s[0] == 'v' && s[1] == 't' && is_space(s[2])) {
            ++tex_count;  // texture coordinates: only counted, for index validation (mesh.rs:19)
        } else if (s[0] == 'f' && is_space(s[1])) {
            poly.clear();
            char* e = s + 1;
            while (true) {
                while (*e && is_space(*e)) ++e;
                if (*e == '\0' || *e == '#') break;
                char* q;
                const long long vi = std::strtoll(e, &q, 10);
                bool ok = q != e;
                e = q;
                long long ti = 0, ni = 0;
                if (ok && *e == '/') {
                    ++e;
                    if (*e != '/') {
                        ti = std::strtoll(e, &q, 10);
                        ok = q != e;
                        e = q;
                    }
                    if (ok && *e == '/') {
                        ++e;
                        ni = std::strtoll(e, &q, 10);
                        ok = q != e;
                        e = q;
                    }
                }
                if (!ok || (*e && !is_space(*e) && *e != '#')) {
                    status = VR_ERROR_IO;
                    err = "malformed face at line " + std::to_string(lineno);
                    break;
                }
                const Corner c{resolve(vi, pos.size() / 3), ni ? resolve(ni, nrm.size() / 3) : -1};
                const int64_t t = ti ? resolve(ti, tex_count) : 0;
                if (c.v < 0 || (size_t)c.v >= pos.size() / 3 || (ni && (c.n < 0 || (size_t)c.n >= nrm.size() / 3)) ||
                    (ti && (t < 0 || (size_t)t >= tex_count))) {
                    status = VR_ERROR_IO;
                    err = "face index out of range at line " + std::to_string(lineno);
                    break;
                }
                poly.push_back(c);
            }
            if (status != VR_OK) break;
            // get_triangles (mesh.rs:43-72): fan (v0, v_i, v_{i+1}); fewer than 3 corners: none
            for (size_t i = 1; i + 1 < poly.size(); ++i) {
                const Corner cs3[3] = {poly[0], poly[i], poly[i + 1]};
                for (const Corner& c : cs3) {
                    for (int k = 0; k < 3; ++k) vout.push_back((double)pos[3 * c.v + k]);
                    for (int k = 0; k < 3; ++k) nout.push_back(c.n >= 0 ? (double)nrm[3 * c.n + k] : 0.0);
                }
                if (groups) {
                    if (current < 0) {  // a name is numbered when its first triangle appears
                        size_t k = 0;
                        while (k < names->size() && (*names)[k] != in_force) ++k;
                        if (k == names->size()) names->push_back(in_force);
                        current = (int64_t)k;
                    }
                    groups->push_back((uint32_t)current);
                }
            }
        } else if (groups && std::strncmp(s, "usemtl", 6) == 0 && (is_space(s[6]) || s[6] == '\0')) {
            const char* b = s + 6;
            while (*b && is_space(*b)) ++b;
            const char* e = b + std::strlen(b);
            while (e > b && is_space(e[-1])) --e;
            in_force.assign(b, e);
            current = -1;
        }
        // everything else (comments, o, g, s, usemtl, mtllib, l, p, blank lines) carries no
        // geometry for load_obj: objects and groups are flattened in file order (mesh.rs:82-85)
    }
    std::free(line);
    std::fclose(f);
    if (status != VR_OK) return fail(status, err);
    const uint64_t n = vout.size() / 9;
    double* v = (double*)std::malloc(sizeof(double) * std::max<size_t>(vout.size(), 1));
    double* nn = (double*)std::malloc(sizeof(double) * std::max<size_t>(nout.size(), 1));
    if (!v || !nn) {
        std::free(v);
        std::free(nn);
        return fail(VR_ERROR_OUT_OF_MEMORY, "mesh allocation failed");
    }
    std::memcpy(v, vout.data(), sizeof(double) * vout.size());
    std::memcpy(nn, nout.data(), sizeof(double) * nout.size());
    *triangle_count = n;
    *vertices = v;
    *normals = nn;
    return VR_OK;
}

int vr_load_obj(const char* path, uint64_t* triangle_count, double** vertices, double** normals) {
    if (!path || !triangle_count || !vertices || !normals) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    return load_obj_impl(path, triangle_count, vertices, normals, nullptr, nullptr);
}

int vr_load_obj_groups(const char* path, uint64_t* triangle_count, double** vertices, double** normals, uint32_t** group,
                       uint32_t* group_count, char** names) {
    if (!path || !triangle_count || !vertices || !normals || !group || !group_count || !names)
        return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    std::vector<uint32_t> groups;
    std::vector<std::string> list;
    const int rc = load_obj_impl(path, triangle_count, vertices, normals, &groups, &list);
    if (rc != VR_OK) return rc;
    if (list.empty()) list.push_back("");  // no triangle at all: still one (empty) name
    size_t bytes = 0;
    for (const std::string& n : list) bytes += n.size() + 1;
    uint32_t* g = (uint32_t*)std::malloc(sizeof(uint32_t) * std::max<size_t>(groups.size(), 1));
    char* block = (char*)std::malloc(bytes);
    if (!g || !block) {
        std::free(g);
        std::free(block);
        vr_mesh_free(*vertices, *normals);
        *vertices = *normals = nullptr;
        return fail(VR_ERROR_OUT_OF_MEMORY, "group allocation failed");
    }
    if (!groups.empty()) std::memcpy(g, groups.data(), sizeof(uint32_t) * groups.size());
    char* at = block;
    for (const std::string& n : list) {
        std::memcpy(at, n.c_str(), n.size() + 1);
        at += n.size() + 1;
    }
    *group = g;
    *group_count = (uint32_t)list.size();
    *names = block;
    return VR_OK;
}

void vr_obj_groups_free(uint32_t* group, char* names) {
    std::free(group);
    std::free(names);
}

void vr_mesh_free(double* vertices, double* normals) {
    std::free(vertices);
    std::free(normals);
}

static void png_chunk(std::vector<uint8_t>& out, const char type[4], const uint8_t* data, size_t n) {
    const uint8_t len[4] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n};
    out.insert(out.end(), len, len + 4);
    const size_t at = out.size();
    out.insert(out.end(), type, type + 4);
    if (n) out.insert(out.end(), data, data + n);
    const uLong crc = crc32(0L, out.data() + at, (uInt)(4 + n));
    const uint8_t c[4] = {(uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc};
    out.insert(out.end(), c, c + 4);
}

int vr_write_png(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height) {
    if (!path || (!rgb && width && height)) return fail(VR_ERROR_INVALID_ARGUMENT, "null argument");
    if (width == 0 || height == 0) return fail(VR_ERROR_INVALID_ARGUMENT, "empty image");
    // 8-bit RGB, no interlace; every scanline carries filter type 0 (the pixels are what the
    // reference's png encoder stores -- its filter choice and compressed bytes may differ)
    const size_t row = (size_t)width * 3;
    std::vector<uint8_t> raw((row + 1) * height);
    for (uint32_t y = 0; y < height; ++y) {
        raw[y * (row + 1)] = 0;
        std::memcpy(&raw[y * (row + 1) + 1], rgb + (size_t)y * row, row);
    }
    uLongf zn = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zn);
    if (compress2(z.data(), &zn, raw.data(), (uLong)raw.size(), 6) != Z_OK) return fail(VR_ERROR_IO, "deflate failed");
    std::vector<uint8_t> out = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    const uint8_t ihdr[13] = {(uint8_t)(width >> 24), (uint8_t)(width >> 16), (uint8_t)(width >> 8), (uint8_t)width,
                              (uint8_t)(height >> 24), (uint8_t)(height >> 16), (uint8_t)(height >> 8), (uint8_t)height,
                              8, 2, 0, 0, 0};
    png_chunk(out, "IHDR", ihdr, 13);
    png_chunk(out, "IDAT", z.data(), zn);
    png_chunk(out, "IEND", nullptr, 0);
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(VR_ERROR_IO, std::string("cannot create ") + path);
    const size_t w = std::fwrite(out.data(), 1, out.size(), f);
    const int c = std::fclose(f);
    if (w != out.size() || c != 0) return fail(VR_ERROR_IO, std::string("write failed: ") + path);
    return VR_OK;
}
}  // extern "C"
