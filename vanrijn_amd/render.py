"""Render API mirroring the reference (camera.rs, accumulation_buffer.rs, util/tile_iterator.rs).

    partial_render_scene(scene, tile, height, width) -> AccumulationBuffer   camera.rs:95-130
    AccumulationBuffer::{new, update_pixel, merge_tile}                     accumulation_buffer.rs:14-85
    Tile / TileIterator                                                     util/tile_iterator.rs:1-67
    AccumulationBuffer::to_image_rgb_u8(&ClampingToneMapper)               accumulation_buffer.rs:38-42
    ImageRgbU8 (get_colour, get_pixel_data, write_png)                      image.rs:8-66
    Film: the full-image AccumulationBuffer of main.rs:197-243 on the GPU   (vr_film_*)

Every render call goes through the C ABI into the gfx950 kernels; nothing here computes a pixel.
"""
import ctypes as C
import sys
import threading
from dataclasses import dataclass

import numpy as np

from . import _native as N
from . import records as R

RECURSION_LIMIT = 128  # camera.rs:69
SAMPLE_RECORD_DTYPE = np.dtype([("wavelength", "<f8"), ("intensity", "<f8"), ("xyz", "<f8", (3,)),
                                ("bounces", "<i4"), ("flags", "<i4")])
HIT_RECORD_DTYPE = np.dtype([("valid", "<i4"), ("object", "<i4"), ("primitive", "<i8"), ("distance", "<f8"),
                             ("location", "<f8", (3,)), ("normal", "<f8", (3,)), ("tangent", "<f8", (3,)),
                             ("cotangent", "<f8", (3,)), ("retro", "<f8", (3,))])
RAY_HIT_DTYPE = np.dtype([("distance", "<f8"), ("primitive", "<i8"), ("object", "<i4"), ("valid", "<i4"),
                          ("reserved", "<u8")])
PHOTON_DTYPE = np.dtype([("wavelength", "<f8"), ("intensity", "<f8")])
PATH_INFO_DTYPE = np.dtype([("bounces", "<i4"), ("flags", "<i4")])
assert RAY_HIT_DTYPE.itemsize == C.sizeof(N.RayHit) == 32
assert PHOTON_DTYPE.itemsize == C.sizeof(N.Photon) == 16 and PATH_INFO_DTYPE.itemsize == C.sizeof(N.PathInfo) == 8
assert SAMPLE_RECORD_DTYPE.itemsize == C.sizeof(N.SampleRecord)
assert HIT_RECORD_DTYPE.itemsize == C.sizeof(N.HitRecord)


@dataclass(frozen=True)
class Tile:
    start_column: int
    end_column: int
    start_row: int
    end_row: int

    def width(self):
        return self.end_column - self.start_column

    def height(self):
        return self.end_row - self.start_row

    def _c(self):
        return N.TileC(self.start_column, self.end_column, self.start_row, self.end_row)


class TileIterator:
    """Row-major tiles of at most tile_size x tile_size covering the image exactly once."""

    def __init__(self, total_width, total_height, tile_size):
        assert tile_size > 0
        self.w, self.h, self.s = total_width, total_height, tile_size

    def __iter__(self):
        row = 0
        while row < self.h:
            col = 0
            while col < self.w:
                yield Tile(col, min(self.w, col + self.s), row, min(self.h, row + self.s))
                col += self.s
            row += self.s


class _OutputPool:
    """Backing stores for output AccumulationBuffers (11 f64 per pixel).  A store is handed out
    again only when nothing but the pool refers to it: every numpy view derived from a store --
    the five arrays of a buffer, and any slice or reshape a caller makes of them -- holds the store
    itself as its `.base`, so the store's reference count says whether any such view is alive."""

    def __init__(self, keep=32):
        self.keep = keep
        self.lock = threading.Lock()
        self.stores = []  # backing arrays
        # the reference count of a store nothing but the pool refers to, measured on this
        # interpreter (how many temporaries getrefcount itself sees differs between versions)
        probe = [np.empty(1)]
        self._free_refs = sys.getrefcount(probe[0])

    @staticmethod
    def _split(store, width, height):
        n = width * height
        return (store[0:3 * n].reshape(height, width, 3), store[3 * n:6 * n].reshape(height, width, 3),
                store[6 * n:9 * n].reshape(height, width, 3), store[9 * n:10 * n].reshape(height, width),
                store[10 * n:11 * n].reshape(height, width))

    def _free(self, i):
        # references: the pool's list (and getrefcount's own); any live view adds its .base
        return sys.getrefcount(self.stores[i]) <= self._free_refs

    def views(self, width, height):
        size = 11 * width * height
        with self.lock:
            for i in range(len(self.stores)):
                if self.stores[i].size == size and self._free(i):
                    return self._split(self.stores[i], width, height)
            store = np.empty(size)
            self.stores.append(store)
            if len(self.stores) > self.keep:  # forget a free store (or the oldest: its views keep it alive)
                for i in range(len(self.stores)):
                    if self._free(i):
                        del self.stores[i]
                        break
                else:
                    del self.stores[0]
            return self._split(store, width, height)


_OUTPUT_POOL = _OutputPool()


class AccumulationBuffer:
    """Per-pixel Kahan-compensated XYZ sums and weights; `colour` is the running mean.

    Arrays are [height][width][3] (XYZ) and [height][width] (weights), row-major like Array2D.
    The reference's `new(a, b)` names its parameters (height, width) but yields width = a,
    height = b (accumulation_buffer.rs:15-28 via array2d.rs:13-19); `new(width, height)` here.
    """

    def __init__(self, width, height):
        self.colour_buffer = np.zeros((height, width, 3))
        self.colour_sum_buffer = np.zeros((height, width, 3))
        self.colour_bias_buffer = np.zeros((height, width, 3))
        self.weight_buffer = np.zeros((height, width))
        self.weight_bias_buffer = np.zeros((height, width))

    @staticmethod
    def new(width, height):
        return AccumulationBuffer(width, height)

    @classmethod
    def _for_output(cls, width, height):
        """A buffer the library overwrites completely (all five arrays): no zeroing pass, and its
        memory recycled from buffers nobody references any more (_OutputPool) -- fresh pages cost
        a page fault per 4 KB on first write, as much host time as a 1-spp render itself."""
        b = cls.__new__(cls)
        (b.colour_buffer, b.colour_sum_buffer, b.colour_bias_buffer, b.weight_buffer,
         b.weight_bias_buffer) = _OUTPUT_POOL.views(width, height)
        return b

    def width(self):
        return self.colour_buffer.shape[1]

    def height(self):
        return self.colour_buffer.shape[0]

    def _c(self):
        for a in (self.colour_buffer, self.colour_sum_buffer, self.colour_bias_buffer, self.weight_buffer,
                  self.weight_bias_buffer):
            assert a.flags.c_contiguous and a.dtype == np.float64
        return N.AccumulationBufferC(self.width(), self.height(), self.colour_buffer.ctypes.data,
                                     self.colour_sum_buffer.ctypes.data, self.colour_bias_buffer.ctypes.data,
                                     self.weight_buffer.ctypes.data, self.weight_bias_buffer.ctypes.data)

    def merge_tile(self, tile: Tile, src: "AccumulationBuffer"):
        """accumulation_buffer.rs:62-85: weighted blend of the means; weights add (vr_merge_tile,
        host code in the library; the size asserts become VrError)."""
        dc, sc = self._c(), src._c()
        N.check(N.lib().vr_merge_tile(C.byref(dc), tile._c(), C.byref(sc)))

    def to_image_rgb_u8(self, device=0) -> "ImageRgbU8":
        """ClampingToneMapper over the XYZ colour buffer (image.rs:166-187), on the GPU."""
        c = np.ascontiguousarray(self.colour_buffer)
        out = np.zeros(c.shape, dtype=np.uint8)
        N.check(N.lib().vr_tone_map(c.ctypes.data_as(C.c_void_p), c.size // 3, out.ctypes.data_as(C.c_void_p),
                                    device))
        return ImageRgbU8(out)

    @staticmethod
    def from_state(state, width=None, height=None):
        """Build from a tile's state records (vanrijn_amd/records.py layout, ABI 7: a flat array of
        8 f64 per pixel, the sums half then the compensations half).  `width` / `height` may be left
        out for a [height][width][8] array, whose shape gives them; such an array must hold the flat
        layout reshaped, not the interleaved per-pixel records of ABI <= 6 -- a shape that does not
        fit raises ValueError instead of misreading the data."""
        a = np.asarray(state.cpu() if hasattr(state, "cpu") else state, dtype=np.float64)
        if width is None or height is None:
            if a.ndim != 3 or a.shape[2] != 8:
                raise ValueError("from_state: pass width and height, or a [height][width][8] array")
            height, width = a.shape[0], a.shape[1]
        if a.size != 8 * width * height:
            raise ValueError(f"from_state: {a.size} values for a {width}x{height} tile (8 f64 per pixel expected)")
        f = R.fields(a.reshape(-1), (height, width))
        b = AccumulationBuffer(width, height)
        b.colour_sum_buffer[...] = f["colour_sum"]
        b.colour_bias_buffer[...] = f["colour_bias"]
        b.weight_buffer[...] = f["weight"]
        b.weight_bias_buffer[...] = f["weight_bias"]
        wgt = f["weight"][..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            b.colour_buffer[...] = np.where(wgt != 0.0, f["colour_sum"] * (1.0 / wgt), 0.0)
        return b


def _scene_handle(scene, device):
    from .scene import DeviceScene, Scene
    if isinstance(scene, DeviceScene):
        return scene
    if isinstance(scene, Scene):
        return scene.device_scene(device)
    raise TypeError("expected Scene or DeviceScene")


def _params(tile, height, width, spp, seed, first_sample, accumulate):
    return N.RenderParams(tile._c(), height, width, spp, 1 if accumulate else 0, seed, first_sample)


def partial_render_scene(scene, tile: Tile, height: int, width: int, device=0) -> AccumulationBuffer:
    """camera.rs:95-130: one sample per pixel of `tile` into a fresh tile AccumulationBuffer."""
    ds = _scene_handle(scene, device)
    out = AccumulationBuffer._for_output(tile.width(), tile.height())
    oc = out._c()
    N.check(N.lib().vr_partial_render_scene(ds.handle, tile._c(), height, width, C.byref(oc)))
    return out


def render_tile(scene, tile: Tile, height, width, spp, seed, first_sample=0, accumulate: AccumulationBuffer = None,
                device=0) -> AccumulationBuffer:
    """spp samples per pixel with explicit seed / sample range (update_pixel semantics)."""
    ds = _scene_handle(scene, device)
    buf = accumulate if accumulate is not None else AccumulationBuffer._for_output(tile.width(), tile.height())
    bc = buf._c()
    p = _params(tile, height, width, spp, seed, first_sample, accumulate is not None)
    N.check(N.lib().vr_render_tile(ds.handle, C.byref(p), C.byref(bc)))
    return buf


def render_samples(scene, tile: Tile, height, width, spp, seed, first_sample=0, device=0):
    """Per-(pixel, sample) records [tile_h][tile_w][spp] (decision-identity checks)."""
    ds = _scene_handle(scene, device)
    out = np.zeros(tile.width() * tile.height() * spp, dtype=SAMPLE_RECORD_DTYPE)
    p = _params(tile, height, width, spp, seed, first_sample, False)
    N.check(N.lib().vr_render_samples(ds.handle, C.byref(p), out.ctypes.data_as(C.c_void_p)))
    return out.reshape(tile.height(), tile.width(), spp)


def trace_rays(scene, origins, directions, device=0):
    """Sampler::sample for a batch of rays (directions used as given)."""
    ds = _scene_handle(scene, device)
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(len(o), dtype=HIT_RECORD_DTYPE)
    N.check(N.lib().vr_trace_rays(ds.handle, len(o), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                  out.ctypes.data_as(C.c_void_p)))
    return out


def _query_flags(normalize, reference_walk):
    return (N.QUERY_NORMALIZE if normalize else 0) | (N.QUERY_REFERENCE_WALK if reference_walk else 0)


def _rays(origins, directions):
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float64).reshape(-1, 3)
    if len(o) != len(d):
        raise ValueError("origins and directions differ in length")
    return o, d


def query_closest(scene, origins, directions, normalize=False, records=False, reference_walk=False, device=0):
    """Sampler::sample for a batch of host rays over the 4-wide tree (vr_query_closest): the hits as
    a RAY_HIT_DTYPE array, or (hits, HIT_RECORD_DTYPE records) with `records`.  Directions are unit
    length unless `normalize` (Ray::new on the device); `reference_walk`: the binary f64 tree, the
    same answers bit for bit."""
    ds = _scene_handle(scene, device)
    o, d = _rays(origins, directions)
    hits = np.zeros(len(o), dtype=RAY_HIT_DTYPE)
    rec = np.zeros(len(o), dtype=HIT_RECORD_DTYPE) if records else None
    N.check(N.lib().vr_query_closest(ds.handle, len(o), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                     _query_flags(normalize, reference_walk), hits.ctypes.data_as(C.c_void_p),
                                     rec.ctypes.data_as(C.c_void_p) if records else None))
    return (hits, rec) if records else hits


def query_any(scene, origins, directions, normalize=False, reference_walk=False, device=0):
    """Sampler::sample(ray).is_some() for a batch of host rays (vr_query_any): a bool array."""
    ds = _scene_handle(scene, device)
    o, d = _rays(origins, directions)
    hit = np.zeros(len(o), dtype=np.uint8)
    N.check(N.lib().vr_query_any(ds.handle, len(o), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                 _query_flags(normalize, reference_walk), hit.ctypes.data_as(C.c_void_p)))
    return hit.astype(bool)


def query_closest_device(scene, n, origins_ptr, directions_ptr, hits_ptr, records_ptr=None, stream_ptr=None,
                         normalize=False, reference_walk=False, device=0):
    """Enqueue Sampler::sample for n rays in device memory ([n][3] f64 each) into device vr_ray_hit
    records at `hits_ptr` (and vr_hit_record at `records_ptr`) on a stream; no synchronisation."""
    ds = _scene_handle(scene, device)
    N.check(N.lib().vr_query_closest_device(ds.handle, n, C.c_void_p(origins_ptr), C.c_void_p(directions_ptr),
                                            _query_flags(normalize, reference_walk), C.c_void_p(hits_ptr),
                                            C.c_void_p(records_ptr or 0), C.c_void_p(stream_ptr or 0)))


def query_any_device(scene, n, origins_ptr, directions_ptr, hit_ptr, stream_ptr=None, normalize=False,
                     reference_walk=False, device=0):
    """Enqueue the any-hit query for n device rays into n device bytes (1 / 0) on a stream."""
    ds = _scene_handle(scene, device)
    N.check(N.lib().vr_query_any_device(ds.handle, n, C.c_void_p(origins_ptr), C.c_void_p(directions_ptr),
                                        _query_flags(normalize, reference_walk), C.c_void_p(hit_ptr),
                                        C.c_void_p(stream_ptr or 0)))


def _integrate_params(seed, first_stream, sample, first_draw, normalize):
    return N.IntegrateParams(seed, first_stream, sample, first_draw, N.QUERY_NORMALIZE if normalize else 0)


def integrate_rays(scene, origins, directions, seed, wavelengths=None, stream_ids=None, first_stream=0, sample=0,
                   first_draw=0, normalize=False, info=False, device=0):
    """The scene's integrator for a batch of host rays (vr_integrate_rays): one photon per ray as a
    PHOTON_DTYPE array, or (photons, PATH_INFO_DTYPE info) with `info`.  `wavelengths`: one per ray, or
    None to draw Photon::random_wavelength from the ray's stream; ray i draws from the stream
    stream_ids[i] = (pixel << 32) + sample, or ((first_stream + i) << 32) + sample, skipping its first
    `first_draw` draws.  Raises VrError(VR_ERROR_SINGULAR_BASIS) like a render."""
    ds = _scene_handle(scene, device)
    o, d = _rays(origins, directions)
    n = len(o)
    wl = ids = None
    if wavelengths is not None:
        wl = np.ascontiguousarray(wavelengths, dtype=np.float64).reshape(-1)
        if len(wl) != n:
            raise ValueError("wavelengths and rays differ in length")
    if stream_ids is not None:
        ids = np.ascontiguousarray(stream_ids, dtype=np.uint64).reshape(-1)
        if len(ids) != n:
            raise ValueError("stream_ids and rays differ in length")
    photons = np.zeros(n, dtype=PHOTON_DTYPE)
    inf = np.zeros(n, dtype=PATH_INFO_DTYPE) if info else None
    p = _integrate_params(seed, first_stream, sample, first_draw, normalize)
    N.check(N.lib().vr_integrate_rays(ds.handle, n, o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                      wl.ctypes.data_as(C.c_void_p) if wl is not None else None,
                                      ids.ctypes.data_as(C.c_void_p) if ids is not None else None, C.byref(p),
                                      photons.ctypes.data_as(C.c_void_p),
                                      inf.ctypes.data_as(C.c_void_p) if info else None))
    return (photons, inf) if info else photons


def integrate_rays_device(scene, n, origins_ptr, directions_ptr, photons_ptr, seed, wavelengths_ptr=None,
                          stream_ids_ptr=None, info_ptr=None, first_stream=0, sample=0, first_draw=0, normalize=False,
                          stream_ptr=None, device=0):
    """Enqueue the scene's integrator for n rays in device memory ([n][3] f64 each) into device
    vr_photon records at `photons_ptr` (and vr_path_info at `info_ptr`) on a stream; no
    synchronisation.  A singular shading basis is reported by stream_check_error on that stream."""
    ds = _scene_handle(scene, device)
    p = _integrate_params(seed, first_stream, sample, first_draw, normalize)
    N.check(N.lib().vr_integrate_rays_device(ds.handle, n, C.c_void_p(origins_ptr), C.c_void_p(directions_ptr),
                                             C.c_void_p(wavelengths_ptr or 0), C.c_void_p(stream_ids_ptr or 0),
                                             C.byref(p), C.c_void_p(photons_ptr), C.c_void_p(info_ptr or 0),
                                             C.c_void_p(stream_ptr or 0)))


def accumulate_photons_device(state_ptr, photons_ptr, pixel_count, spp, accumulate=False, stream_ptr=None, device=0):
    """Enqueue update_pixel of device photons [spp][pixel_count] (sample-major, the staging layout) into
    device state records at `state_ptr` (render_tile_device's layout): the render's ordered reduce alone."""
    N.check(N.lib().vr_accumulate_photons_device(C.c_void_p(state_ptr), C.c_void_p(photons_ptr), pixel_count, spp,
                                                 1 if accumulate else 0, device, C.c_void_p(stream_ptr or 0)))


def camera_rays_device(scene, tile: Tile, height, width, spp, seed, first_sample, origins_ptr, directions_ptr,
                       stream_ids_ptr, stream_ptr=None, device=0):
    """Enqueue ImageSampler::ray_for_pixel of the scene's camera for every (sample, pixel) of `tile`
    into device arrays of spp * tile pixels entries ([s][p] order): origins and directions ([.][3] f64)
    and the samples' stream ids (u64), as integrate_rays_device takes them (first_draw=2)."""
    ds = _scene_handle(scene, device)
    p = _params(tile, height, width, spp, seed, first_sample, False)
    N.check(N.lib().vr_camera_rays_device(ds.handle, C.byref(p), C.c_void_p(origins_ptr), C.c_void_p(directions_ptr),
                                          C.c_void_p(stream_ids_ptr), C.c_void_p(stream_ptr or 0)))


class FeatureBuffers:
    """First-hit feature buffers of a tile (vr_render_features): `records`, a [tile height][tile width]
    array of records.PIXEL_FEATURES_DTYPE, and `albedo_state`, flat state records of render_tile_device's
    layout (8 f64 per pixel; resolve_state, AccumulationBuffer.from_state and tone mapping take it as it
    is), or None where the albedo was not asked for."""

    def __init__(self, records, albedo_state=None):
        self.records = records
        self.albedo_state = albedo_state

    def _inverse_hits(self):
        with np.errstate(divide="ignore"):
            return 1.0 / self.records["hits"].astype(np.float64)

    def normal(self):
        """Mean shading normal [.., 3]: normal_sum * (1 / hits), 0 where no sample hit (not normalised)."""
        with np.errstate(invalid="ignore"):
            mean = self.records["normal_sum"] * self._inverse_hits()[..., None]
        return np.where(self.records["hits"][..., None] != 0, mean, 0.0)

    def depth(self):
        """Mean first-hit distance: distance_sum * (1 / hits); NaN (0 * inf) where no sample hit: there is
        no depth there, and alpha() says so."""
        with np.errstate(invalid="ignore"):
            return self.records["distance_sum"] * self._inverse_hits()

    def alpha(self):
        """Coverage: hits / samples (NaN where no sample was folded in)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.records["hits"].astype(np.float64) / self.records["samples"].astype(np.float64)


def render_features(scene, tile: Tile, height, width, spp, seed, first_sample=0, albedo=True,
                    accumulate: FeatureBuffers = None, device=0) -> FeatureBuffers:
    """First-hit features of spp samples per pixel of `tile` (vr_render_features): per pixel the summed
    normals and distances, the hit count and the nearest sample's object and primitive, and with `albedo`
    a state array of the first hits' material colours.  `accumulate`: a FeatureBuffers of the same tile to
    continue in place (its albedo_state decides whether the albedo is continued)."""
    ds = _scene_handle(scene, device)
    n = tile.width() * tile.height()
    if accumulate is not None:
        out = accumulate
        if out.records.shape != (tile.height(), tile.width()) or out.records.dtype != R.PIXEL_FEATURES_DTYPE or \
                not out.records.flags.c_contiguous:
            raise ValueError("accumulate: records of another tile")
        if out.albedo_state is not None and (out.albedo_state.size != R.RECORD * n or
                                             out.albedo_state.dtype != np.float64 or
                                             not out.albedo_state.flags.c_contiguous):
            raise ValueError("accumulate: albedo state of another tile")
    else:
        out = FeatureBuffers(np.zeros((tile.height(), tile.width()), dtype=R.PIXEL_FEATURES_DTYPE),
                             np.zeros(R.RECORD * n) if albedo else None)
    p = _params(tile, height, width, spp, seed, first_sample, accumulate is not None)
    N.check(N.lib().vr_render_features(ds.handle, C.byref(p), out.records.ctypes.data_as(C.c_void_p),
                                       out.albedo_state.ctypes.data_as(C.c_void_p)
                                       if out.albedo_state is not None else None))
    return out


def render_features_device(scene, tile: Tile, height, width, spp, seed, first_sample, features_ptr, albedo_state_ptr,
                           stream_ptr=None, accumulate=False, device=0):
    """Enqueue the feature pass into device memory on a stream, no synchronisation
    (vr_render_features_device): vr_pixel_features records at `features_ptr` and / or state records at
    `albedo_state_ptr` (either may be None, not both)."""
    ds = _scene_handle(scene, device)
    p = _params(tile, height, width, spp, seed, first_sample, accumulate)
    N.check(N.lib().vr_render_features_device(ds.handle, C.byref(p), C.c_void_p(features_ptr or 0),
                                              C.c_void_p(albedo_state_ptr or 0), C.c_void_p(stream_ptr or 0)))


class DenoiseParams(N.DenoiseParams):
    """vr_denoise_params (its fields are this object's): the image size, the iterations (1..8, tap spacing
    2^i), the flags and the three sigmas; the library's defaults where an argument is None.  `loads`: None
    (the library's choice per step), "direct" or "lds" -- how the device form reads its taps; the bits are
    the same."""

    def __init__(self, width, height, iterations=None, sigma_colour=None, sigma_normal=None, sigma_depth=None,
                 match_object=False, demodulate=False, loads=None):
        super().__init__()
        N.check(N.lib().vr_denoise_default_params(width, height, C.byref(self)))
        for name, value in (("iterations", iterations), ("sigma_colour", sigma_colour), ("sigma_normal", sigma_normal),
                            ("sigma_depth", sigma_depth)):
            if value is not None:
                setattr(self, name, value)
        self.flags = (N.DENOISE_MATCH_OBJECT if match_object else 0) | (N.DENOISE_DEMODULATE if demodulate else 0) | \
            {None: 0, "direct": N.DENOISE_LOADS_DIRECT, "lds": N.DENOISE_LOADS_LDS}[loads]

    def __repr__(self):
        return "DenoiseParams(%s)" % ", ".join(f"{n}={getattr(self, n)!r}" for n, _ in self._fields_)


def denoise_workspace_bytes(params: DenoiseParams) -> int:
    """Bytes of device workspace denoise_device needs (vr_denoise_workspace_bytes): 128 per pixel."""
    out = C.c_uint64()
    N.check(N.lib().vr_denoise_workspace_bytes(C.byref(params), C.byref(out)))
    return out.value


def denoise(state, features, albedo_state=None, params: DenoiseParams = None, device=0, host=False):
    """The edge-avoiding a-trous filter of include/vanrijn_amd.h ("Denoiser") on host arrays: `state`, flat
    state records (8 f64 per pixel); `features`, a FeatureBuffers or a [height][width] array of
    records.PIXEL_FEATURES_DTYPE; `albedo_state`, state records of the albedo (default: the FeatureBuffers'
    own, used only when params asks to demodulate).  Returns a new state array that resolve_state, tone
    mapping and Film.merge_state take as it is.  `params` None: the defaults at the features' shape.
    `host`: vr_denoise_host, the same rule and bits in plain C++ with no device call; otherwise the arrays
    are staged through the device (vr_denoise)."""
    if isinstance(features, FeatureBuffers):
        if albedo_state is None:
            albedo_state = features.albedo_state
        features = features.records
    rec = np.ascontiguousarray(features, dtype=R.PIXEL_FEATURES_DTYPE)
    if params is None:
        if rec.ndim != 2:
            raise ValueError("denoise: params=None needs [height][width] feature records")
        params = DenoiseParams(rec.shape[1], rec.shape[0])
    n = params.width * params.height
    s = np.ascontiguousarray(np.asarray(state, dtype=np.float64).reshape(-1))
    if s.size != R.RECORD * n or rec.size != n:
        raise ValueError("denoise: state or features of another image size")
    a = None
    if albedo_state is not None:
        a = np.ascontiguousarray(np.asarray(albedo_state, dtype=np.float64).reshape(-1))
        if a.size != R.RECORD * n:
            raise ValueError("denoise: albedo state of another image size")
    out = np.zeros(R.RECORD * n)
    args = (C.byref(params), s.ctypes.data_as(C.c_void_p), rec.ctypes.data_as(C.c_void_p),
            a.ctypes.data_as(C.c_void_p) if a is not None else None, out.ctypes.data_as(C.c_void_p))
    N.check(N.lib().vr_denoise_host(*args) if host else N.lib().vr_denoise(*args, device))
    return out


def denoise_device(params: DenoiseParams, state_ptr, features_ptr, albedo_ptr, out_ptr, workspace_ptr, stream_ptr=None,
                   device=0, stage=None):
    """Enqueue the filter on device arrays on a stream, no synchronisation and no allocation
    (vr_denoise_device): state records at `state_ptr`, vr_pixel_features at `features_ptr`, the albedo's
    state records at `albedo_ptr` (or None), the output records at `out_ptr` (may be `state_ptr`) and
    denoise_workspace_bytes(params) bytes at `workspace_ptr`.  `stage`: only that stage
    (vr_denoise_stage_device: 0 prepare, 1..iterations an iteration, iterations + 1 finish)."""
    common = (C.c_void_p(state_ptr or 0), C.c_void_p(features_ptr or 0), C.c_void_p(albedo_ptr or 0),
              C.c_void_p(out_ptr or 0), C.c_void_p(workspace_ptr or 0), device, C.c_void_p(stream_ptr or 0))
    if stage is None:
        N.check(N.lib().vr_denoise_device(C.byref(params), *common))
    else:
        N.check(N.lib().vr_denoise_stage_device(C.byref(params), stage, *common))


class ReprojectParams(N.ReprojectParams):
    """vr_reproject_params (its fields are this object's): the image size, the pose of the current frame and
    of the frame the history was rendered from (scene.CameraPose, or the ctypes struct), the two tolerances,
    the cap on the history's weight (math.inf: none), the flags and the number of motion rows; the library's
    defaults where an argument is None."""

    def __init__(self, width, height, pose, previous_pose, depth_tolerance=None, normal_tolerance=None,
                 max_history_weight=None, match_object=None, motion_count=0):
        super().__init__()
        a, b = (p._c() if hasattr(p, "_c") else p for p in (pose, previous_pose))
        N.check(N.lib().vr_reproject_default_params(width, height, C.byref(a), C.byref(b), C.byref(self)))
        for name, value in (("depth_tolerance", depth_tolerance), ("normal_tolerance", normal_tolerance),
                            ("max_history_weight", max_history_weight)):
            if value is not None:
                setattr(self, name, value)
        if match_object is not None:
            self.flags = N.REPROJECT_MATCH_OBJECT if match_object else 0
        self.motion_count = motion_count

    def __repr__(self):
        return "ReprojectParams(%s)" % ", ".join(
            f"{n}={getattr(self, n)!r}" for n, _ in self._fields_ if n not in ("pose", "previous_pose"))


def motion_rows(previous_matrices, current_matrices):
    """The `motion` rows of reproject for objects placed by transform_mesh: for each object the row-major 3x4
    matrix M_prev * M_cur^-1, which takes a current-frame world position on the object to where that point
    was in the previous frame.  Both arguments: [objects] matrices of 12 or 3x4 values ([A | t]); an object
    that did not move has the same matrix in both.  Returns float64 [objects, 12]."""
    prev = np.asarray(previous_matrices, dtype=np.float64).reshape(-1, 3, 4)
    cur = np.asarray(current_matrices, dtype=np.float64).reshape(-1, 3, 4)
    if prev.shape != cur.shape:
        raise ValueError("motion_rows: as many previous as current matrices")
    out = np.zeros((len(prev), 3, 4))
    for i, (mp, mc) in enumerate(zip(prev, cur)):
        if np.array_equal(mp, mc):
            out[i] = np.eye(3, 4)  # exactly: the same-view shortcut asks for the identity entry by entry
            continue
        inv = np.linalg.inv(mc[:, :3])
        out[i, :, :3] = mp[:, :3] @ inv
        out[i, :, 3] = mp[:, 3] - out[i, :, :3] @ mc[:, 3]
    return out.reshape(-1, 12)


def reproject(state, features, previous_state, previous_features, params: ReprojectParams, motion=None, device=0,
              host=False):
    """Temporal reprojection (include/vanrijn_amd.h, "Temporal reprojection") on host arrays: the current
    frame's flat state records and feature records (a FeatureBuffers or a record array), the history's state
    records and the previous frame's feature records, and optionally `motion`, [rows, 12] (motion_rows).
    Returns a new state array -- the history's contribution plus the current sums -- that resolve_state, tone
    mapping, Film.merge_state and denoise take as it is, and that is the next call's previous_state.
    `host`: vr_reproject_host, the same rule and bits in plain C++ with no device call; otherwise the arrays
    are staged through the device (vr_reproject)."""
    n = params.width * params.height
    rec = []
    for f in (features, previous_features):
        f = f.records if isinstance(f, FeatureBuffers) else f
        rec.append(np.ascontiguousarray(f, dtype=R.PIXEL_FEATURES_DTYPE))
    st = [np.ascontiguousarray(np.asarray(s, dtype=np.float64).reshape(-1)) for s in (state, previous_state)]
    if any(s.size != R.RECORD * n for s in st) or any(r.size != n for r in rec):
        raise ValueError("reproject: state or features of another image size")
    p = params
    m = None
    if motion is not None:
        m = np.ascontiguousarray(np.asarray(motion, dtype=np.float64).reshape(-1, 12))
        p = N.ReprojectParams.from_buffer_copy(params)  # the caller's params stay as they are
        p.motion_count = len(m)
    out = np.zeros(R.RECORD * n)
    args = (C.byref(p), st[0].ctypes.data_as(C.c_void_p), rec[0].ctypes.data_as(C.c_void_p),
            st[1].ctypes.data_as(C.c_void_p), rec[1].ctypes.data_as(C.c_void_p),
            m.ctypes.data_as(C.c_void_p) if m is not None else None, out.ctypes.data_as(C.c_void_p))
    N.check(N.lib().vr_reproject_host(*args) if host else N.lib().vr_reproject(*args, device))
    return out


def reproject_device(params: ReprojectParams, state_ptr, features_ptr, previous_state_ptr, previous_features_ptr, out_ptr,
                     motion_ptr=None, stream_ptr=None, device=0):
    """Enqueue the reprojection on device arrays on a stream, no synchronisation, no allocation and no
    workspace (vr_reproject_device): the current state and feature records, the history's state and the
    previous frame's feature records, the output records at `out_ptr` (may be `state_ptr`, not
    `previous_state_ptr`) and params.motion_count rows of 12 doubles at `motion_ptr` (or None)."""
    N.check(N.lib().vr_reproject_device(C.byref(params), C.c_void_p(state_ptr or 0), C.c_void_p(features_ptr or 0),
                                        C.c_void_p(previous_state_ptr or 0), C.c_void_p(previous_features_ptr or 0),
                                        C.c_void_p(motion_ptr or 0), C.c_void_p(out_ptr or 0), device,
                                        C.c_void_p(stream_ptr or 0)))


def render_tile_device(scene, tile: Tile, height, width, spp, seed, first_sample, state_ptr, stream_ptr=None,
                       accumulate=False, timed=False, counters=False, device=0, defer_times=False, cull=True,
                       dist_cull=True, coop=True, lone_walk=True, stack16=True, one_bvh=True):
    """Enqueue a render into device state records (8 f64 per pixel, vanrijn_amd/records.py) at
    `state_ptr` (a device pointer, e.g. torch.Tensor.data_ptr()).  Returns launch stats (kernel
    time when timed; `variant`: the VR_VARIANT_* bits of the kernel that ran; `defer_times`: the
    events are recorded without waiting, read by collect_launch_times; `cull=False`: every sample
    traced, VR_LAUNCH_NO_CULL; `dist_cull=False`: no BVH distance culling, VR_LAUNCH_NO_DIST_CULL;
    `coop=False`: no cooperative tail, VR_LAUNCH_NO_COOP; `lone_walk=False`: the tail's walks in
    coop_step's per-step form only, VR_LAUNCH_NO_LONE_WALK; `stack16=False`: 32-bit traversal-stack
    entries where 16-bit ones would do, VR_LAUNCH_STACK32; `one_bvh=False`: the generic kernel where the
    single-BVH one would do, VR_LAUNCH_MULTI_BVH -- all six leave the records bit-identical)."""
    ds = _scene_handle(scene, device)
    p = _params(tile, height, width, spp, seed, first_sample, accumulate)
    st = N.LaunchStats()
    flags = (N.LAUNCH_TIMED if timed or defer_times else 0) | (N.LAUNCH_COUNTERS if counters else 0) | \
        (N.LAUNCH_DEFER_TIMES if defer_times else 0) | (0 if cull else N.LAUNCH_NO_CULL) | \
        (0 if dist_cull else N.LAUNCH_NO_DIST_CULL) | (0 if coop else N.LAUNCH_NO_COOP) | \
        (0 if lone_walk else N.LAUNCH_NO_LONE_WALK) | (0 if stack16 else N.LAUNCH_STACK32) | \
        (0 if one_bvh else N.LAUNCH_MULTI_BVH)
    N.check(N.lib().vr_render_tile_device(ds.handle, C.byref(p), C.c_void_p(state_ptr),
                                          C.c_void_p(stream_ptr or 0), flags, C.byref(st)))
    return st.as_dict()


def collect_launch_times(scene, stream_ptr=None, device=0):
    """Waits for the defer_times launches of `scene` on the stream since the last collection:
    {kernel_ms, reduce_ms (sums), launches, passes, max_passes} (vr_collect_launch_times); raises
    their device errors like stream_check_error."""
    ds = _scene_handle(scene, device)
    t = N.LaunchTimes()
    N.check(N.lib().vr_collect_launch_times(ds.handle, C.c_void_p(stream_ptr or 0), C.byref(t)))
    return t.as_dict()


def stream_check_error(scene, stream_ptr=None, device=0):
    """Errors of earlier asynchronous launches of `scene` on a stream (vr_stream_check_error):
    raises VrError(VR_ERROR_SINGULAR_BASIS) once, then the stream is clean again."""
    ds = _scene_handle(scene, device)
    N.check(N.lib().vr_stream_check_error(ds.handle, C.c_void_p(stream_ptr or 0)))


def resolve_state(state):
    """Mean XYZ [pixels, 3] of flat state records (accumulation_buffer.rs:59)."""
    s = np.ascontiguousarray(np.asarray(state, dtype=np.float64).reshape(-1))
    n = R.pixels(s)
    out = np.zeros((n, 3))
    N.check(N.lib().vr_resolve_state(s.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
    return out


class ImageRgbU8:
    """image.rs:8-66: 8-bit RGB pixels, row-major [height][width][3]."""

    def __init__(self, data):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        assert self.data.ndim == 3 and self.data.shape[2] == 3

    @staticmethod
    def new(width, height):
        return ImageRgbU8(np.zeros((height, width, 3), dtype=np.uint8))

    def get_width(self):
        return self.data.shape[1]

    def get_height(self):
        return self.data.shape[0]

    def get_colour(self, row, column):
        return tuple(int(v) for v in self.data[row, column])

    def get_pixel_data(self):
        return self.data.tobytes()

    def write_png(self, path):
        N.check(N.lib().vr_write_png(str(path).encode(), self.data.ctypes.data_as(C.c_void_p), self.get_width(),
                                     self.get_height()))


class Film:
    """The reference's full-image AccumulationBuffer resident on one GPU (vr_film): main.rs:197-243's
    pattern -- workers render 1-spp tiles, merge_tile folds each into the image, to_image_rgb_u8
    displays it -- without the tile buffer leaving the device.  The film's merges are serialised; every
    call reports its place in that order (merge_index), and a snapshot says how many it contains."""

    def __init__(self, width, height, device=0):
        self.width, self.height, self.device = width, height, device
        self.merges_seen = 0  # of the last snapshot taken through this object
        self.handle = None
        h = C.c_void_p()
        N.check(N.lib().vr_film_create(width, height, device, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle is not None:
            N.lib().vr_film_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def clear(self):
        """Back to AccumulationBuffer.new; the merge index restarts at 0."""
        N.check(N.lib().vr_film_clear(self.handle))

    def partial_render_scene(self, scene, tile: Tile):
        """partial_render_scene + merge_tile (main.rs:204,214-216): one sample per pixel of `tile`, the
        sample index from the scene's pass counter.  Returns (merge_index, first_sample)."""
        ds = _scene_handle(scene, self.device)
        m = N.FilmMerge()
        N.check(N.lib().vr_film_partial_render_scene(self.handle, ds.handle, tile._c(), C.byref(m)))
        return m.merge_index, m.first_sample

    def render_tile(self, scene, tile: Tile, spp, seed, first_sample=0):
        """spp samples per pixel of `tile` with an explicit seed / sample range into a fresh tile buffer,
        merged into the film.  Returns (merge_index, first_sample)."""
        ds = _scene_handle(scene, self.device)
        p = _params(tile, self.height, self.width, spp, seed, first_sample, False)
        m = N.FilmMerge()
        N.check(N.lib().vr_film_render_tile(self.handle, ds.handle, C.byref(p), C.byref(m)))
        return m.merge_index, m.first_sample

    def merge_state(self, tile: Tile, state_ptr, stream_ptr=None):
        """merge_tile of device records of `tile` (render_tile_device's layout) produced on the stream;
        only enqueues.  Returns the merge_index."""
        m = N.FilmMerge()
        N.check(N.lib().vr_film_merge_state(self.handle, tile._c(), C.c_void_p(state_ptr),
                                            C.c_void_p(stream_ptr or 0), C.byref(m)))
        return m.merge_index

    def read(self):
        """Snapshot -> (AccumulationBuffer, merges_seen): the buffer holds exactly the successful merges
        with index < merges_seen."""
        out = AccumulationBuffer._for_output(self.width, self.height)
        oc = out._c()
        seen = C.c_uint64()
        N.check(N.lib().vr_film_read(self.handle, C.byref(oc), C.byref(seen)))
        self.merges_seen = seen.value
        return out, seen.value

    def to_image_rgb_u8(self) -> "ImageRgbU8":
        """to_image_rgb_u8(&ClampingToneMapper) of a snapshot (3 bytes per pixel cross PCIe);
        `merges_seen` of this object says which merges it shows."""
        out = np.empty((self.height, self.width, 3), dtype=np.uint8)
        seen = C.c_uint64()
        N.check(N.lib().vr_film_to_image_rgb_u8(self.handle, out.ctypes.data_as(C.c_void_p), C.byref(seen)))
        self.merges_seen = seen.value
        return ImageRgbU8(out)

    def to_image_rgb_u8_device(self, rgb_ptr, stream_ptr=None):
        """The same bytes into device memory (3 per pixel), enqueued on a stream.  Returns merges_seen."""
        seen = C.c_uint64()
        N.check(N.lib().vr_film_to_image_rgb_u8_device(self.handle, C.c_void_p(rgb_ptr), C.c_void_p(stream_ptr or 0),
                                                       C.byref(seen)))
        self.merges_seen = seen.value
        return seen.value


def tone_map_device(state_ptr, pixel_count, rgb_ptr, stream_ptr=None, device=0):
    """Device records (vanrijn_amd/records.py) -> device RGB bytes (3 per pixel), on a stream."""
    N.check(N.lib().vr_tone_map_device(C.c_void_p(state_ptr), pixel_count, C.c_void_p(rgb_ptr), device,
                                       C.c_void_p(stream_ptr or 0)))
