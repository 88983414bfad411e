"""The camera pose (VR_HAS_CAMERA_POSE) without a GPU: the pose of VR_SCENE_HOST_ONLY scenes, its
validation, and the fixed arithmetic of vr_camera_ray (the ray rule, from the inline function the kernels
compile) and vr_camera_look_at against restatements (tests/camera_pose_checks.py) and the oracle's
ImageSampler, bit for bit.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from camera_pose_checks import film_xy, look_at_restated, mirrored, pose_bits, poses, rule_ray
from vanrijn_amd import _native as N
from vanrijn_amd.scene import (BoundingVolumeHierarchy, CameraPose, DeviceScene, LambertianMaterial, Mesh, Plane, Scene,
                               Sphere, Spectrum, look_at)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = CameraPose()
PROTOTYPES = {
    "vr_scene_set_camera_pose": r"int vr_scene_set_camera_pose\(vr_scene\* \w+, const vr_camera_pose\* \w+\);",
    "vr_scene_get_camera_pose": r"int vr_scene_get_camera_pose\(const vr_scene\* \w+, vr_camera_pose\* \w+\);",
    "vr_camera_look_at":
        r"int vr_camera_look_at\(vr_vec3 eye, vr_vec3 target, vr_vec3 up_hint, double film_distance, vr_camera_pose\* out\);",
    "vr_camera_ray": r"int vr_camera_ray\(const vr_camera_pose\* \w+, uint64_t width, uint64_t height, uint64_t row, "
                     r"uint64_t column, double ux, double uy, double origin\[3\], double direction\[3\]\);",
}


def _scene():
    v = np.random.default_rng(3).normal(size=(17, 3, 3))
    n = np.zeros_like(v)
    n[..., 2] = 1.0
    grey = [LambertianMaterial(Spectrum.grey(g), 0.1) for g in (0.2, 0.4, 0.6)]
    return Scene((-2.0, 1.0, -5.0), [[Plane((0.0, 1.0, 0.0), -2.0, grey[0]), Sphere((-6.25, -0.5, 1.0), 1.25, grey[1])],
                                     BoundingVolumeHierarchy.build(Mesh(v, n, grey[2]))])


def _host():
    return DeviceScene(_scene().spec(), 0, host_only=True)


def _code(call):
    try:
        call()
    except N.VrError as e:
        return e.code
    return 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_header_and_symbols():
    text = open(os.path.join(ROOT, "include", "vanrijn_amd.h")).read()
    assert re.search(r"^#define VR_HAS_CAMERA_POSE 1\b", text, flags=re.M)
    assert re.search(r"^#define VR_ABI_VERSION 10\b", text, flags=re.M)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert re.search(r"typedef struct vr_camera_pose \{ vr_vec3 location, right, up, forward; double film_distance; \} "
                     r"vr_camera_pose;", flat)
    for name, prototype in PROTOTYPES.items():
        assert re.search(prototype, flat), name
        assert hasattr(N.lib(), name) and name in N.SIGNATURES, name
    assert C.sizeof(N.CameraPose) == 104


# ------------------------------------------------------------------ round trip and defaults
def test_default_round_trip_and_set_camera():
    ds = _host()
    fresh = ds.camera_pose()
    assert pose_bits(fresh) == pose_bits(CameraPose(location=(-2.0, 1.0, -5.0)))  # +0.0 in every 0 entry
    extent = ds.info()["extent"]
    for name, p in poses().items():
        ds.set_camera_pose(p)
        assert pose_bits(ds.camera_pose()) == pose_bits(p), name
        assert ds.camera().tobytes() == _bits(p.location)  # vr_scene_get_camera: the location, as before
    # an entry of -0.0 and axes off the unit sphere by less than 1e-9 are stored as given
    odd = CameraPose((50.0, -0.0, 3.0), (1.0 + 4e-10, -0.0, 0.0), (0.0, 1.0 - 4e-10, 4e-10), (0.0, -4e-10, 1.0), 1e3)
    ds.set_camera_pose(odd)
    assert pose_bits(ds.camera_pose()) == pose_bits(odd)
    assert ds.info()["extent"] == 50.0 and extent < 50.0  # extent follows the location
    # vr_scene_set_camera afterwards: the location alone
    ds.set_camera((1.0, 2.0, 3.0))
    got = ds.camera_pose()
    assert pose_bits(got) == pose_bits(CameraPose((1.0, 2.0, 3.0), odd.right, odd.up, odd.forward, odd.film_distance))
    assert ds.info()["extent"] == extent


# ------------------------------------------------------------------ validation
def _bad_poses():
    good = poses()["look_at"]
    fields = ("location", "right", "up", "forward")
    for f in fields:
        for axis in range(3):
            for bad in (np.nan, np.inf, -np.inf):
                v = list(getattr(good, f))
                v[axis] = bad
                yield f"{f}[{axis}]={bad}", CameraPose(**{**good.__dict__, f: tuple(v)})
    for bad in (np.nan, np.inf, 0.0, -1.0, 0.999e-3, 1.001e3):
        yield f"film_distance={bad}", CameraPose(**{**good.__dict__, "film_distance": bad})
    d = DEFAULT
    yield "right . up", CameraPose(d.location, (1.0, 2e-9, 0.0), d.up, d.forward, 1.0)
    yield "up . forward", CameraPose(d.location, d.right, (0.0, 1.0, -2e-9), d.forward, 1.0)
    yield "forward . right", CameraPose(d.location, d.right, d.up, (2e-9, 0.0, 1.0), 1.0)
    for i, f in enumerate(("right", "up", "forward")):
        for scale in (1.0 + 1e-9, 1.0 - 1e-9, 0.0, 2.0):  # |a|^2 off 1 by 2e-9, a zero axis, a long one
            v = tuple(scale * c for c in getattr(d, f))
            yield f"|{f}| = {scale}", CameraPose(**{**d.__dict__, f: v})


def test_every_error_case_leaves_the_pose_untouched():
    ds = _host()
    L = N.lib()
    kept = poses()["mirrored"]
    ds.set_camera_pose(kept)
    info = ds.info()
    cases = list(_bad_poses())
    assert len(cases) == 36 + 6 + 3 + 12
    for what, bad in cases:
        assert _code(lambda: ds.set_camera_pose(bad)) == -1, what
        assert pose_bits(ds.camera_pose()) == pose_bits(kept), what
    assert ds.info() == info
    p = kept._c()
    assert L.vr_scene_set_camera_pose(None, C.byref(p)) == -1
    assert L.vr_scene_set_camera_pose(ds.handle, None) == -1
    assert L.vr_scene_get_camera_pose(None, C.byref(p)) == -1
    assert L.vr_scene_get_camera_pose(ds.handle, None) == -1
    assert pose_bits(ds.camera_pose()) == pose_bits(kept)


def test_mirrored_basis_is_accepted():
    ds = _host()
    p = mirrored(DEFAULT)
    r, u, f = (np.array(v) for v in (p.right, p.up, p.forward))
    assert np.dot(np.cross(r, u), f) == -1.0  # right-handed
    ds.set_camera_pose(p)
    assert pose_bits(ds.camera_pose()) == pose_bits(p)
    o, d = p.ray(40, 24, 3, 5, 0.25, 0.5)
    o2, d2 = DEFAULT.ray(40, 24, 3, 5, 0.25, 0.5)
    assert np.array_equal(d * [-1.0, 1.0, 1.0], d2)


# ------------------------------------------------------------------ the rule on the host
def _pixels(width, height, n, seed):
    """(row, column, ux, uy): the corners, the pixels whose x or y is exactly 0 with jitter 0, then random ones."""
    g = np.random.default_rng(seed)
    fixed = [(0, 0, 0.0, 0.0), (height - 1, width - 1, 0.0, 0.0), (0, width - 1, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -53),
             (height // 2 - 1, width // 2, 0.0, 0.0), (height // 2 - 1, 0, 0.0, 0.5), (0, width // 2, 0.5, 0.0)]
    rows, cols = g.integers(0, height, n), g.integers(0, width, n)
    u = g.random((n, 2))
    return fixed + [(int(r), int(c), float(a), float(b)) for r, c, (a, b) in zip(rows, cols, u)]


@pytest.mark.parametrize("width,height", [(40, 24), (24, 40)])
def test_default_pose_rays_equal_the_oracle(width, height, oracle):
    cam = (-2.0, 1.0, -5.0)
    pose = CameraPose(location=cam)
    pixels = _pixels(width, height, 300, width)
    x0, y0 = film_xy(width, height, height // 2 - 1, width // 2, 0.0, 0.0)
    assert x0 == 0.0 or y0 == 0.0  # a film coordinate of exactly 0 is among them
    for row, col, ux, uy in pixels:
        o, d = pose.ray(width, height, row, col, ux, uy)
        ro, rd = oracle.ray_for_pixel(cam, width, height, row, col, ux, uy)
        assert _bits(o) == _bits(ro) and _bits(d) == _bits(rd), (row, col, ux, uy)


@pytest.mark.parametrize("width,height", [(40, 24), (24, 40)])
@pytest.mark.parametrize("name", ["look_at", "up", "mirrored"])
def test_posed_rays_equal_the_restated_rule(name, width, height, oracle):
    pose = poses()[name]
    assert {p.film_distance for p in poses().values()} == {1.0, 0.5, 2.5}
    for row, col, ux, uy in _pixels(width, height, 100, 7):
        o, d = pose.ray(width, height, row, col, ux, uy)
        ro, rd = rule_ray(oracle, pose, width, height, row, col, ux, uy)
        assert _bits(o) == _bits(ro) and _bits(d) == _bits(rd), (row, col, ux, uy)
        assert abs(np.dot(d, d) - 1.0) < 1e-15


def test_camera_ray_argument_errors():
    L = N.lib()
    p = DEFAULT._c()
    o, d = np.zeros(3), np.zeros(3)
    po, pd = o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    assert L.vr_camera_ray(C.byref(p), 8, 8, 0, 0, 0.0, 0.0, po, pd) == 0
    assert L.vr_camera_ray(None, 8, 8, 0, 0, 0.0, 0.0, po, pd) == -1
    assert L.vr_camera_ray(C.byref(p), 8, 8, 0, 0, 0.0, 0.0, None, pd) == -1
    assert L.vr_camera_ray(C.byref(p), 8, 8, 0, 0, 0.0, 0.0, po, None) == -1
    for w, h, row, col in ((0, 8, 0, 0), (8, 0, 0, 0), (8, 8, 8, 0), (8, 8, 0, 8)):
        assert L.vr_camera_ray(C.byref(p), w, h, row, col, 0.0, 0.0, po, pd) == -1


# ------------------------------------------------------------------ look_at
def test_look_at_defaults_and_restatement(oracle):
    assert pose_bits(look_at((0.0, 0.0, 0.0), (0.0, 0.0, 1.0))) == pose_bits(DEFAULT)
    assert pose_bits(look_at((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.0)) == pose_bits(DEFAULT)
    g = np.random.default_rng(11)
    cases = [((0.4, 0.15, -2.3), (-3.2, -0.6, 1.2), (0.2, 1.0, 0.1), 1.0), ((1.0, 2.0, 3.0), (1.0, 2.0, -4.0), (0, 1, 0), 1e-3),
             ((0.0, 0.0, 0.0), (1e-100, 0.0, 0.0), (0.0, 0.0, 5.0), 1e3)]
    cases += [(tuple(g.uniform(-1e3, 1e3, 3)), tuple(g.uniform(-1e3, 1e3, 3)), tuple(g.normal(size=3)),
               float(g.uniform(0.5, 2.5))) for _ in range(200)]
    for eye, target, up, fd in cases:
        got = look_at(eye, target, up, fd)
        assert pose_bits(got) == pose_bits(look_at_restated(oracle, eye, target, up, fd)), (eye, target, up, fd)
        r, u, f = (np.array(v) for v in (got.right, got.up, got.forward))
        assert np.dot(np.cross(r, u), f) > 0.999999  # left-handed: right x up = forward
    down = look_at((0.0, 5.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0))
    assert down.forward == (0.0, -1.0, 0.0) and down.up == (0.0, 0.0, 1.0) and down.right == (1.0, 0.0, 0.0)


def test_look_at_output_passes_validation():
    ds = _host()
    g = np.random.default_rng(5)
    for _ in range(1000):
        eye, target = g.uniform(-1e3, 1e3, 3), g.uniform(-1e3, 1e3, 3)
        ds.set_camera_pose(look_at(eye, target, (0.0, 1.0, 0.0), float(g.uniform(1e-3, 1e3))))


def test_look_at_errors():
    L = N.lib()
    out = N.CameraPose()
    out.film_distance = 77.0
    v = lambda *c: N.Vec3(*c)  # noqa: E731
    assert L.vr_camera_look_at(v(0, 0, 0), v(0, 0, 1), v(0, 1, 0), 1.0, None) == -1
    bad = [((np.nan, 0, 0), (0, 0, 1), (0, 1, 0), 1.0), ((0, 0, 0), (0, np.inf, 1), (0, 1, 0), 1.0),
           ((0, 0, 0), (0, 0, 1), (0, 1, -np.inf), 1.0), ((0, 0, 0), (0, 0, 1), (0, 1, 0), np.nan),
           ((1.0, 2.0, 3.0), (1.0, 2.0, 3.0), (0, 1, 0), 1.0),                      # eye == target
           ((0, 0, 0), (0, 0, 1), (0, 0, 2.0), 1.0), ((0, 0, 0), (0, 3.0, 0), (0, -1.0, 0), 1.0),  # parallel up hints
           ((0, 0, 0), (0, 0, 1), (0, 0, 0), 1.0),                                     # no up hint at all
           ((0, 0, 0), (0, 0, 1), (1e-13, 0, 1.0), 1.0),                               # |cross|^2 = 1e-26 |up|^2
           ((0, 0, 0), (0, 0, 1), (0, 1, 0), 0.999e-3), ((0, 0, 0), (0, 0, 1), (0, 1, 0), 1.001e3),
           ((0, 0, 0), (0, 0, 1), (0, 1, 0), -1.0)]
    for eye, target, up, fd in bad:
        assert L.vr_camera_look_at(v(*eye), v(*target), v(*up), fd, C.byref(out)) == -1, (eye, target, up, fd)
        assert out.film_distance == 77.0  # written on VR_OK only
    assert L.vr_camera_look_at(v(0, 0, 0), v(0, 0, 1), v(1e-11, 0, 1.0), 1.0, C.byref(out)) == 0  # 1e-22 > 1e-24
