"""One scene description at many magnitudes, and ray families that sit on the f32 pre-tests' margins.

The renderer decides most box tests and every sphere skip in f32, with error margins that depend on
the scene's magnitude (vr_device.h prepare32, sphere_maybe32_lanes; the distance-cull margins of
vr_host_scene.cpp update_scalars).  `scaled_scene(S, T)` maps one fixed unit description through
x -> S x + T (T added to every coordinate), so the same geometry is seen where f32 resolves it
(the control), where it resolves part of it (T = 1e3 .. 1e5), where it cannot tell two vertices
apart (T = 2^24 + 1), where the `+ 1` of the margins dominates (S = 1e-6), where the f32 squares
underflow (S = 1e-21) or overflow (S = 1e20) and where the per-ray margin becomes infinite
(S = 3e34: per ray, by max |1/d|; S = 1e36: always).

Nothing here needs a GPU; everything a test compares against comes from the scene description and
the oracle.  The one family that reads a dump of the library (`wide_corner_rays`) reads it only to
aim rays.
"""
import numpy as np

from vanrijn_amd.scene import (BoundingVolumeHierarchy, LambertianMaterial, Mesh, Plane, ReflectiveMaterial, Scene,
                               Sphere, Spectrum)

# (S, T): the slab emulation's regimes (tests/test_slab_bound.py) and the two where the sphere
# pre-test's f32 squares leave the normal range
REGIMES = (
    (1.0, 0.0),                 # control
    (1.0, 1e3),                 # a few box tests fall back to f64
    (1.0, 3e4),                 # some do
    (1.0, 1e5),                 # many do, none is sure
    (1.0, 2.0 ** 24 + 1.0),     # f32 cannot tell the vertices apart: every box test is the f64 one
    (1e-3, 30.0),               # a small scene far from the origin
    (1e-6, 0.0),                # the `+ 1` in X = max(extent, |o|) + 1 dominates: every test falls back
    (1e6, 0.0),                 # as the control: the margins are relative
    (3e34, 0.0),                # ek around 1e30: E finite or infinite per ray
    (1e36, 0.0),                # E = inf for every ray
    (1e-21, 0.0),               # f32 squares of the sphere pre-test are denormal
    (1e20, 0.0),                # and here they overflow
)
CONTROL = REGIMES[0]

# For the builders and the refit alone (dumps against tests/scene_update_checks.py's exact refit;
# nothing is traced or rendered at the last three, where the oracle was not checked): bounds f32 does
# not resolve, bounds in the f32 denormal range, bounds beyond FLT_MAX (the outward rounding's +-inf),
# and for the refit bounds that all round to 0 or the smallest denormal.
BUILD_REGIMES = ((1.0, 1e5), (1.0, 2.0 ** 24 + 1.0), (1e-3, 30.0), (1e-42, 0.0), (1e39, 0.0))
REFIT_REGIMES = BUILD_REGIMES + ((1e-46, 0.0),)
RENDERED = {(1.0, 1e5), (1.0, 2.0 ** 24 + 1.0), (1e-3, 30.0)}


def map_matrix(S, T):
    """x -> S x + T as vr_scene_transform_mesh's row-major 3x4 matrix"""
    return [S, 0.0, 0.0, T, 0.0, S, 0.0, T, 0.0, 0.0, S, T]


def regime_id(regime):
    S, T = regime
    t = "2p24+1" if T == 2.0 ** 24 + 1.0 else f"{T:g}"
    return f"S{S:g}_T{t}"


REGIME_IDS = tuple(regime_id(r) for r in REGIMES)

CAMERA = np.array([0.1, 0.2, -4.0])
BOX_LO = np.array([-1.5, -1.0, -0.6])  # the 3 x 2 x 1.2 volume of the large mesh
BOX_HI = np.array([1.5, 1.0, 0.6])
FLOOR = -1.5
MIRROR_SPHERE = ((-2.0, 1.15, 0.3), 0.9)
GREY_SPHERE = ((2.05, -0.65, 0.1), 0.85)


def unit_description():
    """The unit scene: (large mesh vertices, normals), (small mesh vertices, normals); fixed."""
    g = np.random.default_rng(0x3A6)
    centre = g.uniform(BOX_LO + 0.15, BOX_HI - 0.15, (300, 1, 3))
    va = np.clip(centre + g.normal(scale=0.12, size=(300, 3, 3)), BOX_LO, BOX_HI)
    na = g.normal(size=(300, 3, 3)) + np.array([0.0, 0.0, -1.5])
    centre = g.uniform([0.2, 1.2, -0.3], [1.4, 1.8, 0.5], (40, 1, 3))
    vb = centre + g.normal(scale=0.15, size=(40, 3, 3))
    nb = g.normal(size=(40, 3, 3)) + np.array([0.0, 0.0, -1.5])
    return (va, na), (vb, nb)


def mapped(x, S, T):
    return np.asarray(x, dtype=np.float64) * S + T


def scaled_meshes(S, T):
    (va, na), (vb, nb) = unit_description()
    return (mapped(va, S, T), na), (mapped(vb, S, T), nb)


def scaled_scene(S, T, spheres=True):
    """The unit description through x -> S x + T: two meshes (two BVH roots), a floor plane, a mirror
    sphere and a Lambertian sphere; plane distance and radii mapped too.  Object 0 is the primitive
    list, objects 1 and 2 the meshes."""
    (va, na), (vb, nb) = scaled_meshes(S, T)
    grey = LambertianMaterial(Spectrum.grey(0.6), 0.5)
    prims = [Plane((0.0, 1.0, 0.0), FLOOR * S + T, LambertianMaterial(Spectrum.grey(0.5), 0.5))]
    if spheres:
        prims.append(Sphere(tuple(mapped(MIRROR_SPHERE[0], S, T)), MIRROR_SPHERE[1] * S,
                            ReflectiveMaterial(Spectrum.grey(0.8), 0.05, 0.9)))
        prims.append(Sphere(tuple(mapped(GREY_SPHERE[0], S, T)), GREY_SPHERE[1] * S, grey))
    first = BoundingVolumeHierarchy.build(Mesh(va, na, LambertianMaterial(Spectrum.grey(0.7), 0.6)))
    second = BoundingVolumeHierarchy.build(Mesh(vb, nb, ReflectiveMaterial(Spectrum.grey(0.7), 0.1, 0.8)))
    return Scene(tuple(mapped(CAMERA, S, T)), [prims, first, second])


def sphere_field_scene(S, T):
    """Many small spheres in front of the camera, so that a frame's camera rays graze limbs by the
    hundred: a 12 x 10 lattice (pitch 0.4, radii 0.05 .. 0.19, alternately mirror and Lambertian,
    jittered in depth) over the floor plane, through x -> S x + T.  The large spheres of scaled_scene
    leave the sphere pre-test's margin a band of a thousandth of the radius at S = 1e-21; here r^2
    is a few dozen denormal steps and the band is several per cent."""
    g = np.random.default_rng(0x5F1E1D)
    grey = LambertianMaterial(Spectrum.grey(0.6), 0.5)
    mirror = ReflectiveMaterial(Spectrum.grey(0.8), 0.05, 0.9)
    prims = [Plane((0.0, 1.0, 0.0), -2.2 * S + T, LambertianMaterial(Spectrum.grey(0.5), 0.5))]
    for j in range(10):
        for i in range(12):
            centre = np.array([-2.2 + 0.4 * i, -1.8 + 0.4 * j, g.uniform(-0.5, 0.5)]) + g.uniform(-0.03, 0.03, 3)
            prims.append(Sphere(tuple(mapped(centre, S, T)), g.uniform(0.05, 0.19) * S, mirror if (i + j) % 2 else grey))
    return Scene(tuple(mapped((0.0, 0.0, -4.0), S, T)), [prims])


def tied_scene(seed, S, T):
    """tests/test_gpu_ties.py's _tied_scene (the same draws) through x -> S x + T: every triangle two
    or three times at exactly the same place, a second BVH object repeating 300 of them, and a plane."""
    from vanrijn_amd.scene import ColourRgbF
    g = np.random.default_rng(seed)
    n = 600
    centre = g.uniform([-1.2, -0.8, -0.6], [1.2, 0.8, 0.6], (n, 1, 3))
    verts = mapped(centre + g.normal(scale=0.18, size=(n, 3, 3)), S, T)
    reps = g.integers(2, 4, n)
    v_all, n_all = [], []
    for i in range(n):
        for _ in range(reps[i]):
            v_all.append(verts[i])
            n_all.append(g.normal(size=(3, 3)) + np.array([0.0, 0.0, -1.5]))
    order = g.permutation(len(v_all))
    v_all = np.array(v_all)[order]
    n_all = np.array(n_all)[order]
    a = LambertianMaterial(Spectrum.grey(0.7), 0.6)
    b = LambertianMaterial(Spectrum.reflection_from_linear_rgb(ColourRgbF(0.2, 0.9, 0.4)), 0.8)
    floor = LambertianMaterial(Spectrum.grey(0.5), 0.5)
    first = BoundingVolumeHierarchy.build(Mesh(v_all, n_all, a))
    second = BoundingVolumeHierarchy.build(Mesh(v_all[:300].copy(), n_all[:300][:, ::-1].copy(), b))
    return Scene(tuple(mapped((0.0, 0.0, -4.0), S, T)), [[Plane((0.0, 1.0, 0.0), -1.5 * S + T, floor)], first, second])


def triangle_boxes(v):
    """BoundingBox::from_points of each triangle: [n][6] {min x, max x, min y, max y, min z, max z}."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    out = np.empty((len(v), 6))
    out[:, 0::2] = v.min(axis=1)
    out[:, 1::2] = v.max(axis=1)
    return out


def leaf_boxes(S, T):
    (va, _), (vb, _) = scaled_meshes(S, T)
    return np.concatenate([triangle_boxes(va), triangle_boxes(vb)])


def scene_extent(S, T):
    """max |coordinate| of camera and geometry, as the library keeps it (vr_host_scene.cpp)"""
    (va, _), (vb, _) = scaled_meshes(S, T)
    e = max(np.abs(va).max(), np.abs(vb).max(), np.abs(mapped(CAMERA, S, T)).max(), abs(FLOOR * S + T))
    for c, r in (MIRROR_SPHERE, GREY_SPHERE):
        e = max(e, (np.abs(mapped(c, S, T)) + r * S).max())
    return float(e)


# ----------------------------------------------------------------------------------- ray families
def _unit(v):
    with np.errstate(over="ignore"):
        n = np.sqrt((v * v).sum(axis=1, keepdims=True))
    bad = ~np.isfinite(n[:, 0]) | (n[:, 0] == 0.0)
    if bad.any():  # differences near DBL_MAX / DBL_MIN: scale first
        v = v.copy()
        v[bad] = v[bad] / np.abs(v[bad]).max(axis=1, keepdims=True)
        n = np.sqrt((v * v).sum(axis=1, keepdims=True))
    return v / n


def camera_rays(S, T, n, seed):
    g = np.random.default_rng(seed)
    cam = mapped(CAMERA, S, T)
    target = mapped(g.uniform(BOX_LO - [1.2, 0.6, 0.4], BOX_HI + [1.2, 0.9, 0.6], (n, 3)), S, T)
    return np.repeat(cam[None], n, 0), _unit(target - cam)


def inside_rays(S, T, n, seed):
    g = np.random.default_rng(seed)
    o = mapped(g.uniform(BOX_LO - 0.3, BOX_HI + 0.3, (n, 3)), S, T)
    return o, _unit(g.normal(size=(n, 3)))


def bounce_rays(S, points, seed):
    """From surface points (oracle hit locations): the point plus 1e-7 S d, d random"""
    g = np.random.default_rng(seed)
    d = _unit(g.normal(size=points.shape))
    return points + d * (1e-7 * S), d


def _outside_origins(g, S, T, n, far=False):
    """Origins 3 to 6 units from the volume's centre, above the floor; `far`: every other one ten
    times as far (at T = 2^24 + 1 one f64 ulp of a coordinate is 7e-10 of a ray parameter of 5, so
    only the far origins keep a nudged corner within 1e-9 relative)."""
    away = _unit(g.normal(size=(n, 3)))
    away[:, 1] = np.abs(away[:, 1]) * 0.8  # above the floor
    radius = g.uniform(3.0, 6.0, (n, 1))
    if far:
        radius[1::2] *= 10.0
    return mapped(_unit(away) * radius, S, T)


def vertex_rays(S, T, n, seed):
    g = np.random.default_rng(seed)
    (va, _), (vb, _) = scaled_meshes(S, T)
    verts = np.concatenate([va.reshape(-1, 3), vb.reshape(-1, 3)])
    o = _outside_origins(g, S, T, n)
    return o, _unit(verts[g.integers(len(verts), size=n)] - o)


def corner_rays(boxes, S, T, n, seed):
    """Rays from outside origins at corners of `boxes` ([m][6] f64), each corner coordinate nudged by an
    integer -3 .. 3 ulp: the three slabs' entry or exit parameters meet there, so the f64 interval of
    the aimed box is empty or not by a few ulp.  Returns origins, directions and the aimed box's index."""
    g = np.random.default_rng(seed)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    which = g.integers(len(boxes), size=n)
    side = g.integers(2, size=(n, 3))
    corner = boxes[which][np.arange(n)[:, None], 2 * np.arange(3)[None, :] + side]
    corner = corner + g.integers(-3, 4, size=(n, 3)) * np.spacing(np.abs(corner))
    o = _outside_origins(g, S, T, n, far=True)
    return o, _unit(corner - o), which


def wide_corner_boxes(wide_nodes, empty_child):
    """The interior slots' boxes of a 4-wide tree dump (DeviceScene.wide_nodes()), f32 widened to f64"""
    live = (wide_nodes["child"] >= 0) & (wide_nodes["child"] != empty_child)
    b = np.transpose(wide_nodes["bound"], (0, 2, 1))[live]  # [slot][6]
    return b.astype(np.float64)


def slab_interval(boxes, o, d):
    """The reference's line interval per (box, ray) pair, vectorised ([n][6], [n][3], [n][3]): lo, hi
    with NaN-ignoring max / min (axis_aligned_bounding_box.rs:9-27, as test_slab_bound.f64_slab)."""
    lo = np.full(len(o), -np.inf)
    hi = np.full(len(o), np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            x = (boxes[:, 2 * a] - o[:, a]) / d[:, a]
            y = (boxes[:, 2 * a + 1] - o[:, a]) / d[:, a]
            swap = x > y
            mn, mx = np.where(swap, y, x), np.where(swap, x, y)
            lo = np.fmax(lo, mn)
            hi = np.fmin(hi, mx)
    return lo, hi


def near_ties(boxes, o, d, rel=1e-9):
    """Of the (box, ray) pairs, those whose f64 interval has |hi - lo| <= rel max(|lo|, |hi|), and the
    f64 verdict of each (test_slab_bound.f64_slab): (mask, verdict)."""
    from test_slab_bound import f64_slab
    lo, hi = slab_interval(boxes, o, d)
    with np.errstate(invalid="ignore"):
        mask = np.abs(hi - lo) <= rel * np.maximum(np.abs(lo), np.abs(hi))
    verdict = np.array([f64_slab(boxes[k], o[k], d[k]) for k in range(len(o))], dtype=bool)
    return mask, verdict


# the counts of one regime's batch: 8002 rays at the most
N_CAMERA, N_INSIDE, N_BOUNCE, N_VERTEX, N_TRI_CORNER, N_WIDE_CORNER = 1000, 1000, 1500, 1000, 2000, 1500
MAX_RAYS = 8002


def ray_batch(regime, orc, oracle, wide_boxes=None):
    """One regime's rays: camera-like, inside, bounce-like (from the oracle's hits on the first two),
    vertex-aimed, aimed at triangle-box corners and, with `wide_boxes`, at interior-slot corners.
    Returns (origins, directions, family index per ray, (aimed leaf box index or -1) per ray)."""
    S, T = regime
    oc, dc = camera_rays(S, T, N_CAMERA, 1)
    oi, di = inside_rays(S, T, N_INSIDE, 2)
    first, _ = orc.trace(np.concatenate([oc, oi]), np.concatenate([dc, di]), oracle.MODE_REFERENCE)
    pts = np.array([list(h.location) for h in first if h.valid]).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(axis=1)][:N_BOUNCE]
    ob, db = bounce_rays(S, pts, 3)
    ov, dv = vertex_rays(S, T, N_VERTEX, 4)
    ot, dt, which = corner_rays(leaf_boxes(S, T), S, T, N_TRI_CORNER, 5)
    parts = [(oc, dc), (oi, di), (ob, db), (ov, dv), (ot, dt)]
    if wide_boxes is not None and len(wide_boxes):
        ow, dw, _ = corner_rays(wide_boxes, S, T, N_WIDE_CORNER, 6)
        parts.append((ow, dw))
    o = np.concatenate([p[0] for p in parts])
    d = np.concatenate([p[1] for p in parts])
    family = np.concatenate([np.full(len(p[0]), k) for k, p in enumerate(parts)])
    aimed = np.full(len(o), -1)
    start = sum(len(p[0]) for p in parts[:4])
    aimed[start:start + len(which)] = which
    assert len(o) <= MAX_RAYS
    return np.ascontiguousarray(o), np.ascontiguousarray(d), family, aimed
