"""Host-side mirror of the reference's scene API (names and argument meaning as in vanrijn).

    colour::ColourRgbF / NamedColour      src/colour/colour_rgb.rs:5-105
    colour::Spectrum                      src/colour/spectrum.rs:5-175
    materials::LambertianMaterial         src/materials/lambertian_material.rs:12-25
    materials::ReflectiveMaterial         src/materials/reflective_material.rs:8-13
    raycasting::{Plane, Sphere}           src/raycasting/plane.rs:18-31, sphere.rs:15-23
    raycasting::BoundingVolumeHierarchy   src/raycasting/bounding_volume_hierarchy.rs:49-51
    mesh::load_obj                        src/mesh.rs:74-88
    scene::Scene                          src/scene.rs:5-8

A `Scene` lowers to a plain-data `SceneSpec` (numbers only) which the C ABI consumes
(`vr_scene_create`) -- and which the test oracle consumes too, so both see identical inputs.
"""
from dataclasses import dataclass, field
import atexit
import ctypes as C
from enum import Enum
from typing import List
import weakref

import numpy as np

from . import _native as N

# every DeviceScene not yet released: destroyed at interpreter exit while the library and the HIP
# runtime are still loaded (module teardown order would otherwise decide)
_LIVE = weakref.WeakSet()


@atexit.register
def _release_live_scenes():
    for s in list(_LIVE):
        s.release()

SHORTEST_VISIBLE_WAVELENGTH = 380.0  # src/colour/mod.rs:13
LONGEST_VISIBLE_WAVELENGTH = 740.0   # src/colour/mod.rs:14


# ------------------------------------------------------------------------------ colours / spectra
class NamedColour(Enum):
    Black = (0.0, 0.0, 0.0)
    White = (1.0, 1.0, 1.0)
    Red = (1.0, 0.0, 0.0)
    Lime = (0.0, 1.0, 0.0)
    Blue = (0.0, 0.0, 1.0)
    Yellow = (1.0, 1.0, 0.0)
    Cyan = (0.0, 1.0, 1.0)
    Magenta = (1.0, 0.0, 1.0)
    Gray = (0.5, 0.5, 0.5)
    Maroon = (0.5, 0.0, 0.0)
    Olive = (0.5, 0.5, 0.0)
    Green = (0.0, 0.5, 0.0)
    Purple = (0.5, 0.0, 0.5)
    Teal = (0.0, 0.5, 0.5)
    Navy = (0.0, 0.0, 0.5)


@dataclass(frozen=True)
class ColourRgbF:
    red: float
    green: float
    blue: float

    @staticmethod
    def new(r, g, b):
        return ColourRgbF(float(r), float(g), float(b))

    @staticmethod
    def from_named(name: NamedColour):
        return ColourRgbF(*name.value)


@dataclass
class Spectrum:
    shortest_wavelength: float
    longest_wavelength: float
    samples: np.ndarray

    @staticmethod
    def black():
        return Spectrum(SHORTEST_VISIBLE_WAVELENGTH, LONGEST_VISIBLE_WAVELENGTH, np.zeros(2))

    @staticmethod
    def grey(brightness):
        return Spectrum(SHORTEST_VISIBLE_WAVELENGTH, LONGEST_VISIBLE_WAVELENGTH, np.full(2, float(brightness)))

    @staticmethod
    def reflection_from_linear_rgb(colour: ColourRgbF):
        out = np.zeros(32)
        N.check(N.lib().vr_spectrum_reflection_from_linear_rgb(colour.red, colour.green, colour.blue,
                                                                out.ctypes.data_as(C.c_void_p)))
        return Spectrum(380.0, 720.0, out)

    def intensity_at_wavelength(self, wavelength):
        s = np.ascontiguousarray(self.samples, dtype=np.float64)
        sp = N.Spectrum(self.shortest_wavelength, self.longest_wavelength, s.size,
                        s.ctypes.data_as(C.POINTER(C.c_double)))
        return N.lib().vr_spectrum_intensity_at_wavelength(C.byref(sp), float(wavelength))


# ------------------------------------------------------------------------------ materials
@dataclass
class LambertianMaterial:
    colour: Spectrum
    diffuse_strength: float

    @staticmethod
    def new_dummy():  # lambertian_material.rs:19-24
        return LambertianMaterial(Spectrum.black(), 1.0)


@dataclass
class ReflectiveMaterial:
    colour: Spectrum
    diffuse_strength: float
    reflection_strength: float


@dataclass
class PhongMaterial:
    """materials/phong_material.rs:8-37; sampled by CosineWeightedHemisphere (materials/mod.rs:28-33)."""
    colour: Spectrum
    diffuse_strength: float
    specular_strength: float
    smoothness: float


@dataclass
class SmoothTransparentDialectric:
    """materials/smooth_transparent_dialectric.rs:64-115 (the reference's spelling): refractive index
    eta(lambda) as a Spectrum."""
    eta: Spectrum

    @staticmethod
    def new(eta):
        return SmoothTransparentDialectric(eta)


# ------------------------------------------------------------------------------ integrators
@dataclass
class DirectionalLight:
    """integrators/whitted_integrator.rs:10-13."""
    direction: tuple
    spectrum: Spectrum


@dataclass
class WhittedIntegrator:
    """integrators/whitted_integrator.rs:15-87.  The reference's partial_render_scene always uses
    SimpleRandomIntegrator (camera.rs:103); here a Scene may carry this one instead."""
    ambient_light: Spectrum
    lights: list


# ------------------------------------------------------------------------------ geometry
@dataclass
class Plane:
    normal: tuple
    distance_from_origin: float
    material: object


@dataclass
class Sphere:
    centre: tuple
    radius: float
    material: object


@dataclass
class Mesh:
    """A triangle mesh: vertices/normals float64 [n][3][3] (Vec<Triangle>, triangle.rs:8-13)."""
    vertices: np.ndarray
    normals: np.ndarray
    material: object
    # per-triangle materials, or None: (palette, ids) -- a list of material objects and a uint32 [n]
    # array of indices into it, in the order of `vertices` (vr_scene_set_mesh_materials)
    triangle_materials: object = None

    def __len__(self):
        return len(self.vertices)


class BoundingVolumeHierarchy:
    """BoundingVolumeHierarchy::build over a mesh.  The tree is built (with the reference's median
    split) by the native library when the scene is created."""

    def __init__(self, mesh: Mesh):
        self.mesh = mesh

    @staticmethod
    def build(mesh: Mesh):
        return BoundingVolumeHierarchy(mesh)


def load_obj(path, material):
    """mesh::load_obj: OBJ positions/normals as f32 widened to f64, fan-triangulated polygons."""
    L = N.lib()
    n = C.c_uint64()
    v = C.POINTER(C.c_double)()
    nn = C.POINTER(C.c_double)()
    N.check(L.vr_load_obj(str(path).encode(), C.byref(n), C.byref(v), C.byref(nn)))
    try:
        cnt = int(n.value) * 9
        verts = np.ctypeslib.as_array(v, shape=(max(cnt, 1),))[:cnt].copy().reshape(-1, 3, 3)
        norms = np.ctypeslib.as_array(nn, shape=(max(cnt, 1),))[:cnt].copy().reshape(-1, 3, 3)
    finally:
        L.vr_mesh_free(v, nn)
    return Mesh(verts, norms, material)


def load_obj_groups(path):
    """vr_load_obj_groups: load_obj's geometry (the same bits) with the file's usemtl groups:
    (vertices, normals, group, names) -- group a uint32 [n] array of indices into the list `names`, in
    order of first appearance; faces before any usemtl belong to the name "".  No .mtl file is read:
    Mesh(vertices, normals, material, triangle_materials=([materials by name], group)) renders it."""
    L = N.lib()
    n, k = C.c_uint64(), C.c_uint32()
    v = C.POINTER(C.c_double)()
    nn = C.POINTER(C.c_double)()
    g = C.POINTER(C.c_uint32)()
    names = C.c_void_p()
    N.check(L.vr_load_obj_groups(str(path).encode(), C.byref(n), C.byref(v), C.byref(nn), C.byref(g), C.byref(k),
                                 C.byref(names)))
    try:
        tri = int(n.value)
        verts = np.ctypeslib.as_array(v, shape=(max(tri * 9, 1),))[:tri * 9].copy().reshape(-1, 3, 3)
        norms = np.ctypeslib.as_array(nn, shape=(max(tri * 9, 1),))[:tri * 9].copy().reshape(-1, 3, 3)
        group = np.ctypeslib.as_array(g, shape=(max(tri, 1),))[:tri].copy()
        out, at = [], names.value
        for _ in range(k.value):
            name = C.string_at(at)
            out.append(name.decode())
            at += len(name) + 1
    finally:
        L.vr_mesh_free(v, nn)
        L.vr_obj_groups_free(g, names)
    return verts, norms, group, out


# ------------------------------------------------------------------------------ plain-data spec
@dataclass
class MaterialSpec:
    kind: int
    colour: Spectrum
    diffuse_strength: float
    reflection_strength: float = 0.0  # reflective; Phong's specular strength
    smoothness: float = 0.0           # Phong


@dataclass
class PrimitiveSpec:
    kind: int
    material: int
    vector: tuple
    scalar: float


@dataclass
class MeshSpec:
    vertices: np.ndarray
    normals: np.ndarray
    material: int
    triangle_materials: object = None  # uint32 [n] indices into SceneSpec.materials, or None


@dataclass
class ObjectSpec:
    kind: str  # "primitives" | "bvh"
    primitives: List[PrimitiveSpec] = field(default_factory=list)
    mesh: int = -1


@dataclass
class SceneSpec:
    camera_location: tuple
    materials: List[MaterialSpec]
    meshes: List[MeshSpec]
    objects: List[ObjectSpec]
    integrator: object = None  # None (SimpleRandomIntegrator) or WhittedIntegrator


@dataclass(frozen=True)
class CameraPose:
    """vr_camera_pose: where the camera is, its orthonormal basis (used as given) and the film's
    distance along `forward`.  The default is the reference's camera: looking down +z, film at 1.
    The field of view across the shorter film side is 2 * atan(0.5 / film_distance)."""
    location: tuple = (0.0, 0.0, 0.0)
    right: tuple = (1.0, 0.0, 0.0)
    up: tuple = (0.0, 1.0, 0.0)
    forward: tuple = (0.0, 0.0, 1.0)
    film_distance: float = 1.0

    def _c(self):
        vec = [N.Vec3(*(float(c) for c in v)) for v in (self.location, self.right, self.up, self.forward)]
        return N.CameraPose(*vec, float(self.film_distance))

    @staticmethod
    def _from_c(p):
        return CameraPose(*((v.x, v.y, v.z) for v in (p.location, p.right, p.up, p.forward)), p.film_distance)

    def ray(self, width, height, row, column, ux, uy, lens=None, lu=0.5, lv=0.5):
        """vr_camera_ray: the camera ray of pixel (row, column) with jitter (ux, uy), on the host from
        the function the kernels compile: (origin, direction), float64 [3] each.  With a CameraLens,
        vr_camera_lens_ray: the ray through the lens point of draws (lu, lv); (0.5, 0.5) is the
        lens' centre, and a lens of radius 0 gives the pinhole ray."""
        o, d = np.zeros(3), np.zeros(3)
        p = self._c()
        if lens is not None:
            cl = lens._c()
            N.check(N.lib().vr_camera_lens_ray(C.byref(p), C.byref(cl), int(width), int(height), int(row), int(column),
                                               float(ux), float(uy), float(lu), float(lv),
                                               o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)))
            return o, d
        N.check(N.lib().vr_camera_ray(C.byref(p), int(width), int(height), int(row), int(column), float(ux),
                                      float(uy), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)))
        return o, d


@dataclass(frozen=True)
class CameraLens:
    """vr_camera_lens: a thin lens of radius `lens_radius` ([0, 1e3]; 0 is no lens, the pinhole) in the
    pose's right / up plane, focused on the plane `focus_distance` ([1e-3, 1e6]) along `forward`."""
    lens_radius: float = 0.0
    focus_distance: float = 1.0

    def _c(self):
        return N.CameraLens(float(self.lens_radius), float(self.focus_distance))


def lens_point(lu, lv):
    """vr_camera_lens_point: the point of the unit disc that lens draws (lu, lv) in [0, 1) map to
    (Shirley's concentric map with the kernels' fixed sine and cosine): float64 [2]."""
    out = np.zeros(2)
    N.check(N.lib().vr_camera_lens_point(float(lu), float(lv), out.ctypes.data_as(C.c_void_p)))
    return out


def look_at(eye, target, up=(0.0, 1.0, 0.0), film_distance=1.0) -> CameraPose:
    """vr_camera_look_at: the left-handed pose (x right, y up, z forward) of a camera at `eye` looking
    at `target`; `up` must not be parallel to the view direction."""
    out = N.CameraPose()
    e, t, u = (N.Vec3(*(float(c) for c in v)) for v in (eye, target, up))
    N.check(N.lib().vr_camera_look_at(e, t, u, float(film_distance), C.byref(out)))
    return CameraPose._from_c(out)


class Scene:
    """scene::Scene { camera_location, objects } (src/scene.rs:5-8).

    objects: list whose items are either a list of Plane/Sphere (a Vec<Box<dyn Primitive>>
    aggregate) or a BoundingVolumeHierarchy."""

    def __init__(self, camera_location, objects, integrator=None):
        self.camera_location = tuple(float(c) for c in camera_location)
        self.objects = list(objects)
        self.integrator = integrator
        self._spec = None
        self._device_scenes = {}

    def spec(self) -> SceneSpec:
        if self._spec is None:
            mats, mat_ids = [], {}

            def mid(m):
                if id(m) not in mat_ids:
                    mat_ids[id(m)] = len(mats)
                    if isinstance(m, ReflectiveMaterial):
                        mats.append(MaterialSpec(N.MATERIAL_REFLECTIVE, m.colour, m.diffuse_strength,
                                                 m.reflection_strength))
                    elif isinstance(m, LambertianMaterial):
                        mats.append(MaterialSpec(N.MATERIAL_LAMBERTIAN, m.colour, m.diffuse_strength, 0.0))
                    elif isinstance(m, PhongMaterial):
                        mats.append(MaterialSpec(N.MATERIAL_PHONG, m.colour, m.diffuse_strength, m.specular_strength,
                                                 m.smoothness))
                    elif isinstance(m, SmoothTransparentDialectric):
                        mats.append(MaterialSpec(N.MATERIAL_DIELECTRIC, m.eta, 0.0, 0.0))
                    else:
                        raise TypeError(f"unsupported material {type(m).__name__}")
                return mat_ids[id(m)]

            meshes, objs = [], []
            for o in self.objects:
                if isinstance(o, BoundingVolumeHierarchy):
                    meshes.append(MeshSpec(np.ascontiguousarray(o.mesh.vertices, dtype=np.float64),
                                           np.ascontiguousarray(o.mesh.normals, dtype=np.float64),
                                           mid(o.mesh.material)))
                    if o.mesh.triangle_materials is not None:
                        palette, ids = o.mesh.triangle_materials
                        ids = np.asarray(ids)
                        if ids.shape != (len(o.mesh.vertices),) or (ids.size and not 0 <= ids.min() <= ids.max() < len(palette)):
                            raise ValueError("triangle_materials: one palette index per triangle")
                        scene_ids = np.array([mid(m) for m in palette], dtype=np.uint32)
                        meshes[-1].triangle_materials = scene_ids[ids.astype(np.int64)] if ids.size else ids.astype(np.uint32)
                    objs.append(ObjectSpec("bvh", mesh=len(meshes) - 1))
                else:
                    prims = []
                    for p in o:
                        if isinstance(p, Plane):
                            prims.append(PrimitiveSpec(N.PRIMITIVE_PLANE, mid(p.material), tuple(p.normal),
                                                       float(p.distance_from_origin)))
                        elif isinstance(p, Sphere):
                            prims.append(PrimitiveSpec(N.PRIMITIVE_SPHERE, mid(p.material), tuple(p.centre),
                                                       float(p.radius)))
                        else:
                            raise TypeError(f"unsupported primitive {type(p).__name__}")
                    objs.append(ObjectSpec("primitives", prims))
            self._spec = SceneSpec(self.camera_location, mats, meshes, objs, self.integrator)
        return self._spec

    def device_scene(self, device=0, host_only=False, device_bvh=False, reference_bvh=False, device_sah=False,
                     wide_offsets=False):
        key = (device, host_only, device_bvh, reference_bvh, device_sah, wide_offsets)
        if key not in self._device_scenes:
            self._device_scenes[key] = DeviceScene(self.spec(), device, host_only, device_bvh, reference_bvh,
                                                   device_sah, wide_offsets=wide_offsets)
        return self._device_scenes[key]


def _c_spectrum(sp, keep):
    a = np.ascontiguousarray(sp.samples, dtype=np.float64)
    keep.append(a)
    return N.Spectrum(sp.shortest_wavelength, sp.longest_wavelength, a.size, a.ctypes.data_as(C.POINTER(C.c_double)))


def _c_material(m: MaterialSpec, keep):
    return N.MaterialDesc(m.kind, 0, _c_spectrum(m.colour, keep), m.diffuse_strength, m.reflection_strength,
                          m.smoothness)


def _c_integrator(integrator: WhittedIntegrator, keep):
    lights = (N.DirectionalLightC * max(len(integrator.lights), 1))()
    for j, li in enumerate(integrator.lights):
        lights[j] = N.DirectionalLightC(N.Vec3(*li.direction), _c_spectrum(li.spectrum, keep))
    keep.append(lights)
    return N.IntegratorDesc(N.INTEGRATOR_WHITTED, len(integrator.lights), _c_spectrum(integrator.ambient_light, keep),
                            lights)


def _c_primitive(p):
    """A PrimitiveSpec, or a Plane / Sphere whose `material` is a material index."""
    if isinstance(p, Plane):
        p = PrimitiveSpec(N.PRIMITIVE_PLANE, p.material, tuple(p.normal), float(p.distance_from_origin))
    elif isinstance(p, Sphere):
        p = PrimitiveSpec(N.PRIMITIVE_SPHERE, p.material, tuple(p.centre), float(p.radius))
    return N.PrimitiveDesc(p.kind, int(p.material), N.Vec3(*p.vector), p.scalar)


class DeviceScene:
    """Owner of a `vr_scene*` (flattened BVH resident in one GPU's HBM)."""

    def __init__(self, spec: SceneSpec, device=0, host_only=False, device_bvh=False, reference_bvh=False,
                 device_sah=False, greedy_collapse=False, wide_offsets=False):
        """device_bvh: build the BVHs on the GPU (VR_SCENE_DEVICE_BVH: the reference's tree);
        reference_bvh: traverse the reference's median-split tree instead of the SAH tree;
        device_sah: build the SAH traversal tree on the GPU too (VR_SCENE_DEVICE_SAH);
        greedy_collapse: the greedy 4-wide collapse instead of the SAH-optimal one (inspection);
        wide_offsets: render with the 64-bit-offset kernels that scenes past 53.7 M triangles or 2^25
        wide nodes take automatically (VR_SCENE_WIDE_OFFSETS; identical renders)."""
        L = N.lib()
        self.spec = spec
        keep = []  # keep ctypes buffers alive during vr_scene_create
        mats = (N.MaterialDesc * max(len(spec.materials), 1))()
        for i, m in enumerate(spec.materials):
            mats[i] = _c_material(m, keep)
        prims, objs, meshes = [], [], []
        for o in spec.objects:
            if o.kind == "primitives":
                objs.append(N.ObjectDesc(N.OBJECT_PRIMITIVE_LIST, len(prims), len(o.primitives), 0))
                prims += [_c_primitive(p) for p in o.primitives]
            else:
                objs.append(N.ObjectDesc(N.OBJECT_BVH, o.mesh, 1, 0))
        for m in spec.meshes:
            v = np.ascontiguousarray(m.vertices, dtype=np.float64).reshape(-1)
            nn = np.ascontiguousarray(m.normals, dtype=np.float64).reshape(-1)
            assert v.size == nn.size and v.size % 9 == 0
            keep += [v, nn]
            meshes.append(N.MeshDesc(v.size // 9, v.ctypes.data_as(C.POINTER(C.c_double)),
                                     nn.ctypes.data_as(C.POINTER(C.c_double)), m.material, 0))
        prim_arr = (N.PrimitiveDesc * max(len(prims), 1))(*prims)
        obj_arr = (N.ObjectDesc * max(len(objs), 1))(*objs)
        mesh_arr = (N.MeshDesc * max(len(meshes), 1))(*meshes)
        ig = _c_integrator(spec.integrator, keep) if spec.integrator is not None else None
        desc = N.SceneDesc(N.Vec3(*spec.camera_location), len(spec.materials), len(prims), len(meshes), len(objs),
                           mats, prim_arr, mesh_arr, obj_arr, C.pointer(ig) if ig is not None else None)
        h = C.c_void_p()
        flags = ((N.SCENE_HOST_ONLY if host_only else 0) | (N.SCENE_DEVICE_BVH if device_bvh else 0) |
                 (N.SCENE_REFERENCE_BVH if reference_bvh else 0) | (N.SCENE_DEVICE_SAH if device_sah else 0) |
                 (N.SCENE_GREEDY_COLLAPSE if greedy_collapse else 0) | (N.SCENE_WIDE_OFFSETS if wide_offsets else 0))
        N.check(L.vr_scene_create(C.byref(desc), device, flags, C.byref(h)))
        self.handle = h
        self.device = device
        self.host_only = host_only
        # bound now: at interpreter exit module globals (N, N.lib) may already be torn down when
        # __del__ runs; scenes still alive then are released by _release_live_scenes (atexit)
        self._destroy = L.vr_scene_destroy
        _LIVE.add(self)
        for i, m in enumerate(spec.meshes):  # a MeshSpec from before the field existed has none
            if getattr(m, "triangle_materials", None) is not None:
                self.set_mesh_materials(i, m.triangle_materials)

    def release(self):
        """vr_scene_destroy now (waits for the scene's queued work); idempotent."""
        h = getattr(self, "handle", None)
        if h:
            self.handle = None
            self._destroy(h)

    def __del__(self):
        self.release()

    def set_staging_limit(self, nbytes):
        """vr_scene_set_staging_limit: cap one call's staging memory (0: half the free HBM); larger
        frames run in several launches with bit-identical records."""
        N.check(N.lib().vr_scene_set_staging_limit(self.handle, int(nbytes)))

    def info(self):
        i = N.SceneInfo()
        N.check(N.lib().vr_scene_get_info(self.handle, C.byref(i)))
        d = {n: getattr(i, n) for n, _ in i._fields_}
        d["nan_free"] = bool(d["flags"] & N.SCENE_INFO_NAN_FREE)
        return d

    def launch_variant(self, pixel_samples, launch_flags=0, recording=False):
        """vr_scene_launch_variant: the VARIANT_* bits a render of `pixel_samples` (tile pixels x spp)
        would report now; launches nothing (host-only scenes too)."""
        v = C.c_uint32(0)
        N.check(N.lib().vr_scene_launch_variant(self.handle, int(pixel_samples), int(launch_flags), int(bool(recording)),
                                                C.byref(v)))
        return v.value

    def grid_shared(self):
        """vr_scene_grid_shared: bit 0, the material and Whitted light rows lie on one wavelength grid bit
        for bit; bit 1 (never without bit 0), the sky row lies on it too."""
        return int(N.lib().vr_scene_grid_shared(self.handle))

    @classmethod
    def grids_shared(cls, rows):
        """vr_material_grids_shared of material rows (materials()' structured array)."""
        rows = np.ascontiguousarray(rows, dtype=cls.MATERIAL_DTYPE)
        return bool(N.lib().vr_material_grids_shared(rows.ctypes.data_as(C.c_void_p), len(rows)))

    def set_fault_object(self, obj):
        """Test hook (vr_debug_set_fault_object): hits on scene object `obj` report the singular
        shading basis (VR_ERROR_SINGULAR_BASIS); -1 turns it off."""
        N.check(N.lib().vr_debug_set_fault_object(self.handle, obj))

    def set_launch_flags(self, no_cull=False, no_dist_cull=False, no_coop=False, no_lone_walk=False, stack32=False,
                         multi_bvh=False):
        """Test hook (vr_debug_set_launch_flags): every later render of this scene -- per-sample
        records and host buffers included -- skips the frustum culling, the BVH distance culling or
        the cooperative tail or its whole-walk form, keeps 32-bit traversal-stack entries, or runs the
        generic kernel where the single-BVH one would do (each leaves the records bit-identical)."""
        flags = ((N.LAUNCH_NO_CULL if no_cull else 0) | (N.LAUNCH_NO_DIST_CULL if no_dist_cull else 0) |
                 (N.LAUNCH_NO_COOP if no_coop else 0) | (N.LAUNCH_NO_LONE_WALK if no_lone_walk else 0) |
                 (N.LAUNCH_STACK32 if stack32 else 0) | (N.LAUNCH_MULTI_BVH if multi_bvh else 0))
        N.check(N.lib().vr_debug_set_launch_flags(self.handle, flags))

    NODE_DTYPE = np.dtype([("box", "<f8", (2, 6)), ("child", "<i4", (2,)), ("pad", "<i4", (6,))])

    def bvh_nodes(self):
        """The flattened interior nodes (vr_scene_bvh_nodes), a structured array."""
        out = np.zeros(self.info()["node_count"], dtype=self.NODE_DTYPE)
        if out.size:
            N.check(N.lib().vr_scene_bvh_nodes(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def leaf_order(self, mesh):
        out = np.zeros(len(self.spec.meshes[mesh].vertices), dtype=np.uint64)
        N.check(N.lib().vr_scene_bvh_leaf_order(self.handle, mesh, out.ctypes.data_as(C.c_void_p)))
        return out

    WIDE_NODE_DTYPE = np.dtype([("bound", "<f4", (6, 4)), ("child", "<i4", (4,)), ("pad", "<i4", (4,))])
    TRI_VERTS_DTYPE = np.dtype([("v", "<f8", (3, 3)), ("rank", "<i8")])
    TRI_NORMALS_DTYPE = np.dtype([("n", "<f8", (3, 3)), ("pad", "<f8")])
    BVH_ROOT_DTYPE = np.dtype([("root_box", "<f8", (6,)), ("root_box32", "<f4", (6,)), ("root", "<i4"),
                               ("root4", "<i4"), ("pad", "<i4"), ("object", "<i4"), ("tri_base", "<i4"),
                               ("material", "<i4")])
    EMPTY_CHILD = -2 ** 31  # an unused slot of a 4-wide node (its six bounds are NaN)

    def wide_nodes(self):
        """The render kernel's 4-wide tree (vr_scene_wide_nodes), a structured array: bound[j][slot],
        j = min x, max x, min y, max y, min z, max z; child >= 0 a wide node, EMPTY_CHILD, else leaf
        holding triangle slot ~child."""
        out = np.zeros(self.info()["wide_node_count"], dtype=self.WIDE_NODE_DTYPE)
        if out.size:
            N.check(N.lib().vr_scene_wide_nodes(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def triangles(self):
        """The triangle and normal records in slot (traversal leaf) order (vr_scene_triangles): two
        structured arrays; `rank` is the scene-wide leaf position in the reference tree, and the bytes
        of the normal records' `pad`, viewed as int64, the triangle's own material: 0 the mesh's, m + 1
        material m (set_mesh_materials)."""
        n = self.info()["triangle_count"]
        v = np.zeros(n, dtype=self.TRI_VERTS_DTYPE)
        nn = np.zeros(n, dtype=self.TRI_NORMALS_DTYPE)
        if n:
            N.check(N.lib().vr_scene_triangles(self.handle, v.ctypes.data_as(C.c_void_p),
                                               nn.ctypes.data_as(C.c_void_p)))
        return v, nn

    def bvh_roots(self):
        """One record per BVH object in object order (vr_scene_bvh_roots); `pad` is 1 where the mesh's
        triangles carry materials of their own (set_mesh_materials), else 0."""
        n = sum(1 for o in self.spec.objects if o.kind == "bvh")
        out = np.zeros(n, dtype=self.BVH_ROOT_DTYPE)
        if n:
            N.check(N.lib().vr_scene_bvh_roots(self.handle, out.ctypes.data_as(C.c_void_p)))
        return out

    def update_mesh(self, mesh, vertices, normals):
        """vr_scene_update_mesh: new vertices / normals ([n][3][3] float64, n the mesh's triangle
        count) for mesh `mesh` of THIS device scene; both trees are refitted in place and every later
        call behaves as on a scene created from the new geometry (bit for bit, except that exact
        distance ties keep the creation-time ranks).  Blocks until the scene is ready.  Not
        thread-safe against other calls on this scene; its queued asynchronous work must be done.

        The owning Scene / SceneSpec are not touched: other cached DeviceScenes of the same Scene,
        and scenes created from it later, keep the old geometry."""
        v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1)
        nn = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1)
        if v.size != nn.size or v.size % 9:
            raise ValueError("vertices and normals must both be [n][3][3]")
        N.check(N.lib().vr_scene_update_mesh(self.handle, mesh, v.size // 9, v.ctypes.data_as(C.c_void_p),
                                             nn.ctypes.data_as(C.c_void_p)))

    def update_mesh_device(self, mesh, vertices_ptr, normals_ptr, stream_ptr=None):
        """vr_scene_update_mesh_device: as update_mesh, from device arrays of the scene's GPU (raw
        pointers to [n][3][3] float64, n the mesh's triangle count, e.g. tensor.data_ptr()), ordered
        after earlier work on `stream_ptr` (None: the null stream).  Blocks until the scene is ready;
        the arrays are not read afterwards."""
        n = len(self.spec.meshes[mesh].vertices) if 0 <= mesh < len(self.spec.meshes) else 0
        N.check(N.lib().vr_scene_update_mesh_device(self.handle, mesh, n, C.c_void_p(vertices_ptr),
                                                    C.c_void_p(normals_ptr), C.c_void_p(stream_ptr or 0)))

    # ------------------------------------------------------------------ per-triangle materials
    def set_mesh_materials(self, mesh, ids):
        """vr_scene_set_mesh_materials: ids[i] is the index into the spec's materials of INPUT triangle
        i of mesh `mesh` (uint32 [n], n the mesh's triangle count); None goes back to the mesh's single
        material.  A scene edit: blocks, changes THIS device scene only, and leaves trees, ranks, info()
        and the launch variant as they are.  The assignment survives update_mesh and transform_mesh."""
        n = len(self.spec.meshes[mesh].vertices) if 0 <= mesh < len(self.spec.meshes) else 0
        if ids is None:
            N.check(N.lib().vr_scene_set_mesh_materials(self.handle, int(mesh), n, None))
            return
        a = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        N.check(N.lib().vr_scene_set_mesh_materials(self.handle, int(mesh), a.size, a.ctypes.data_as(C.c_void_p)))

    def set_mesh_materials_device(self, mesh, ptr, stream_ptr=None):
        """vr_scene_set_mesh_materials_device: as set_mesh_materials, from a device array of the scene's
        GPU (a raw pointer to n 32-bit indices, e.g. an int32 tensor's data_ptr()), ordered after earlier
        work on `stream_ptr` (None: the null stream).  An index out of range is found on the device
        before anything is written."""
        n = len(self.spec.meshes[mesh].vertices) if 0 <= mesh < len(self.spec.meshes) else 0
        N.check(N.lib().vr_scene_set_mesh_materials_device(self.handle, int(mesh), n, C.c_void_p(ptr),
                                                           C.c_void_p(stream_ptr or 0)))

    def mesh_materials(self, mesh):
        """vr_scene_mesh_materials: the material index of every input triangle of mesh `mesh` now
        (uint32 [n]; the mesh's own material where none is set)."""
        n = len(self.spec.meshes[mesh].vertices) if 0 <= mesh < len(self.spec.meshes) else 0
        out = np.zeros(n, dtype=np.uint32)
        N.check(N.lib().vr_scene_mesh_materials(self.handle, int(mesh), out.ctypes.data_as(C.c_void_p)))
        return out

    # ------------------------------------------------------------------ scene edits (VR_HAS_SCENE_EDIT)
    # Each changes THIS device scene only and blocks until it is ready; afterwards every call answers
    # as on a scene created from the edited description, bit for bit.  Not thread-safe against other
    # calls on this scene; its queued asynchronous work must be done.  As with update_mesh, the owning
    # Scene / SceneSpec are not touched: other cached DeviceScenes of the same Scene, and scenes created
    # from it later, keep the old description.
    def set_camera(self, xyz):
        """vr_scene_set_camera: the camera location (three finite floats).  The owning Scene /
        SceneSpec are not touched."""
        x, y, z = (float(c) for c in xyz)
        N.check(N.lib().vr_scene_set_camera(self.handle, N.Vec3(x, y, z)))

    def set_camera_pose(self, pose: CameraPose):
        """vr_scene_set_camera_pose: location, orthonormal basis (1e-9; either handedness) and film
        distance ([1e-3, 1e3]) of the camera every render, film, sample and camera-ray call of this
        scene uses.  set_camera afterwards moves the location alone.  The owning Scene / SceneSpec are
        not touched."""
        p = pose._c()
        N.check(N.lib().vr_scene_set_camera_pose(self.handle, C.byref(p)))

    def camera_pose(self) -> CameraPose:
        """The scene's pose (vr_scene_get_camera_pose); the default one until set_camera_pose."""
        p = N.CameraPose()
        N.check(N.lib().vr_scene_get_camera_pose(self.handle, C.byref(p)))
        return CameraPose._from_c(p)

    def set_camera_lens(self, lens: CameraLens):
        """vr_scene_set_camera_lens: aperture and focus distance of the camera every render, film, sample
        and camera-ray call of this scene uses; a radius of 0 turns the lens off.  A lens scene spends
        draws 2 and 3 of each (pixel, sample) stream on the lens point, so its wavelength is draw 4.
        The pose is not touched, and set_camera / set_camera_pose leave the lens alone."""
        cl = lens._c()
        N.check(N.lib().vr_scene_set_camera_lens(self.handle, C.byref(cl)))

    def camera_lens(self) -> CameraLens:
        """The scene's lens (vr_scene_get_camera_lens); CameraLens(0, 1) until set_camera_lens."""
        cl = N.CameraLens()
        N.check(N.lib().vr_scene_get_camera_lens(self.handle, C.byref(cl)))
        return CameraLens(cl.lens_radius, cl.focus_distance)

    def update_primitives(self, first, prims):
        """vr_scene_update_primitives: replace entries first .. first + len(prims) - 1 of the scene's
        primitives (numbered through all primitive lists in object order) by `prims`: PrimitiveSpec, or
        Plane / Sphere whose `material` is a material index.  The owning Scene / SceneSpec are not
        touched."""
        arr = (N.PrimitiveDesc * max(len(prims), 1))(*[_c_primitive(p) for p in prims])
        N.check(N.lib().vr_scene_update_primitives(self.handle, int(first), len(prims), arr))

    def update_material(self, index, material: MaterialSpec):
        """vr_scene_update_material: replace material `index` of the spec's materials; nan_free and the
        kernel choice follow as on a fresh scene.  The owning Scene / SceneSpec are not touched."""
        keep = []
        m = _c_material(material, keep)
        N.check(N.lib().vr_scene_update_material(self.handle, int(index), C.byref(m)))

    def set_lights(self, integrator):
        """vr_scene_set_lights: a WhittedIntegrator with as many lights as the scene's (new ambient
        spectrum, light spectra and directions), or None on a SimpleRandomIntegrator scene (nothing
        changes).  The owning Scene / SceneSpec are not touched."""
        keep = []
        ig = _c_integrator(integrator, keep) if integrator is not None else None
        N.check(N.lib().vr_scene_set_lights(self.handle, C.byref(ig) if ig is not None else None))

    def transform_mesh(self, mesh, matrix, stream_ptr=None):
        """vr_scene_transform_mesh: mesh `mesh` becomes the image of its base geometry (creation's, or
        the latest update_mesh's) under the row-major 3x4 matrix [A | t] (any array-like of 12 or 3x4
        values); normals go through A's cofactor matrix.  Transforms do not compound.  Runs on the
        device from resident records, ordered after earlier work on `stream_ptr` (None: the null
        stream).  The owning Scene / SceneSpec are not touched."""
        m = np.ascontiguousarray(matrix, dtype=np.float64).reshape(-1)
        if m.size != 12:
            raise ValueError("matrix must hold 12 values (3x4, row-major)")
        N.check(N.lib().vr_scene_transform_mesh(self.handle, int(mesh), m.ctypes.data_as(C.c_void_p),
                                                C.c_void_p(stream_ptr or 0)))

    PRIM_DTYPE = np.dtype([("kind", "<i4"), ("material", "<i4"), ("object", "<i4"), ("position", "<i4"),
                           ("vec", "<f8", (3,)), ("tan", "<f8", (3,)), ("cot", "<f8", (3,)), ("scalar", "<f8"),
                           ("pre", "<f8", (3,)), ("scalar2", "<f8")])
    MATERIAL_DTYPE = np.dtype([("kind", "<i4"), ("n", "<i4"), ("shortest", "<f8"), ("longest", "<f8"),
                               ("diffuse", "<f8"), ("reflection", "<f8"), ("smoothness", "<f8"),
                               ("samples", "<f8", (64,)), ("knots", "<f8", (64,)), ("inv_step", "<f8")])

    def _rows(self, fn, dtype):
        n = C.c_uint32()
        N.check(fn(self.handle, None, C.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        if out.size:
            N.check(fn(self.handle, out.ctypes.data_as(C.c_void_p), C.byref(n)))
        return out

    def primitives(self):
        """The primitive rows in kernel order (vr_scene_primitives), a structured array."""
        return self._rows(N.lib().vr_scene_primitives, self.PRIM_DTYPE)

    def materials(self):
        """Every material row, the light and sky rows included (vr_scene_materials)."""
        return self._rows(N.lib().vr_scene_materials, self.MATERIAL_DTYPE)

    def camera(self):
        """The camera location (vr_scene_get_camera), float64 [3]."""
        v = N.Vec3()
        N.check(N.lib().vr_scene_get_camera(self.handle, C.byref(v)))
        return np.array([v.x, v.y, v.z])
