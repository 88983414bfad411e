"""The camera lens (VR_HAS_CAMERA_LENS) without a GPU: the lens of VR_SCENE_HOST_ONLY scenes, its
validation, and the fixed arithmetic of vr_camera_lens_point and vr_camera_lens_ray (the lens rule, from the
inline functions the kernels compile) against restatements (tests/camera_lens_checks.py), bit for bit.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from camera_lens_checks import disc, lens_bits, lens_draws_grid, lens_rule_ray, poly_cos, poly_sin
from camera_pose_checks import pose_bits, poses
from vanrijn_amd import _native as N
from vanrijn_amd import lens_point
from vanrijn_amd.scene import (BoundingVolumeHierarchy, CameraLens, CameraPose, DeviceScene, LambertianMaterial, Mesh,
                               Plane, Scene, Sphere, Spectrum)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAMERA = (-2.0, 1.0, -5.0)
PROTOTYPES = {
    "vr_scene_set_camera_lens": r"int vr_scene_set_camera_lens\(vr_scene\* \w+, const vr_camera_lens\* \w+\);",
    "vr_scene_get_camera_lens": r"int vr_scene_get_camera_lens\(const vr_scene\* \w+, vr_camera_lens\* \w+\);",
    "vr_camera_lens_point": r"int vr_camera_lens_point\(double lu, double lv, double out\[2\]\);",
    "vr_camera_lens_ray": r"int vr_camera_lens_ray\(const vr_camera_pose\* \w+, const vr_camera_lens\* \w+, uint64_t width, "
                          r"uint64_t height, uint64_t row, uint64_t column, double ux, double uy, double lu, double lv, "
                          r"double origin\[3\], double direction\[3\]\);",
}


def _scene():
    v = np.random.default_rng(3).normal(size=(17, 3, 3))
    n = np.zeros_like(v)
    n[..., 2] = 1.0
    grey = [LambertianMaterial(Spectrum.grey(g), 0.1) for g in (0.2, 0.4, 0.6)]
    return Scene(CAMERA, [[Plane((0.0, 1.0, 0.0), -2.0, grey[0]), Sphere((-6.25, -0.5, 1.0), 1.25, grey[1])],
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
    assert re.search(r"^#define VR_HAS_CAMERA_LENS 1\b", text, flags=re.M)
    assert re.search(r"^#define VR_ABI_VERSION 10\b", text, flags=re.M)
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert re.search(r"typedef struct vr_camera_lens \{ double lens_radius, focus_distance; \} vr_camera_lens;", flat)
    for name, prototype in PROTOTYPES.items():
        assert re.search(prototype, flat), name
        assert hasattr(N.lib(), name) and name in N.SIGNATURES, name
    assert C.sizeof(N.CameraLens) == 16


# ------------------------------------------------------------------ the disc map
def test_lens_point_equals_the_restatement():
    pts = lens_draws_grid()
    branches = {True: 0, False: 0}
    for lu, lv in pts:
        got = lens_point(lu, lv)
        want = disc(lu, lv)
        assert _bits(got) == _bits(want), (lu, lv)
        ox, oy = 2.0 * lu - 1.0, 2.0 * lv - 1.0
        branches[abs(ox) > abs(oy)] += 1
    assert min(branches.values()) > 100
    assert _bits(lens_point(0.5, 0.5)) == _bits([0.0, 0.0])
    diagonals = [(lu, lv) for lu, lv in pts if abs(2.0 * lu - 1.0) == abs(2.0 * lv - 1.0) and lu != 0.5]
    assert len(diagonals) >= 120
    corners = [(lu, lv) for lu, lv in pts if lu in (0.0, 1.0 - 2.0 ** -53) and lv in (0.0, 1.0 - 2.0 ** -53)]
    assert len(set(corners)) == 4


def test_lens_point_against_libm_and_the_unit_disc():
    """The mapped point is within 1e-15 of the same map through libm, and no point leaves the disc by more than
    8 ulp of 1.  The polynomials themselves: the truncation is below (pi/4)^17 / 17! = 4.7e-17, the last Horner
    step and the product with x round values below 1 (at most 1.1e-16 each, the earlier steps' errors shrink by
    x^2 <= 0.62 per step), libm is within an ulp: 3e-16 bounds the difference on [-pi/4, pi/4]."""
    x = np.linspace(-np.pi / 4, np.pi / 4, 20001)
    sin_err = max(abs(float(poly_sin(v)) - np.sin(v)) for v in x)
    cos_err = max(abs(float(poly_cos(v)) - np.cos(v)) for v in x)
    print(f"polynomials against libm: sin {sin_err:.3e} cos {cos_err:.3e}")
    assert sin_err < 3e-16 and cos_err < 3e-16
    g = np.random.default_rng(19)
    pts = lens_draws_grid() + [tuple(p) for p in g.random((2000, 2))]
    worst, radius = 0.0, 0.0
    for lu, lv in pts:
        got = lens_point(lu, lv)
        want = disc(lu, lv, sin=np.sin, cos=np.cos)
        worst = max(worst, abs(got[0] - want[0]), abs(got[1] - want[1]))
        radius = max(radius, float(np.hypot(got[0], got[1])))
    assert worst <= 1e-15
    assert radius <= 1.0 + 8 * 2.0 ** -52
    assert radius > 0.999  # the rim is reached


# ------------------------------------------------------------------ the lens rule on the host
def _samples(width, height, n, seed):
    g = np.random.default_rng(seed)
    top = 1.0 - 2.0 ** -53
    fixed = [(0, 0, 0.0, 0.0, 0.0, 0.0), (height - 1, width - 1, top, top, top, top),
             (height // 2 - 1, width // 2, 0.0, 0.0, 0.5, 0.5), (0, width - 1, 0.5, 0.5, 0.25, 0.75),
             (height - 1, 0, 0.5, 0.5, 0.75, 0.75)]
    rows, cols = g.integers(0, height, n), g.integers(0, width, n)
    u = g.random((n, 4))
    return fixed + [(int(r), int(c), *(float(t) for t in q)) for r, c, q in zip(rows, cols, u)]


LENSES = [CameraLens(0.4, 12.0), CameraLens(0.05, 3.5), CameraLens(50.0, 1e-3), CameraLens(1e3, 1e6)]


@pytest.mark.parametrize("width,height", [(40, 24), (24, 40)])
@pytest.mark.parametrize("name", ["default", "look_at", "up", "mirrored"])
def test_lens_rays_equal_the_restated_rule(name, width, height, oracle):
    pose = CameraPose(location=CAMERA) if name == "default" else poses()[name]
    for lens in LENSES:
        for row, col, ux, uy, lu, lv in _samples(width, height, 60, 7):
            o, d = pose.ray(width, height, row, col, ux, uy, lens=lens, lu=lu, lv=lv)
            ro, rd = lens_rule_ray(oracle, pose, lens, width, height, row, col, ux, uy, lu, lv)
            assert _bits(o) == _bits(ro) and _bits(d) == _bits(rd), (lens, row, col, ux, uy, lu, lv)
            assert abs(np.dot(d, d) - 1.0) < 1e-15


@pytest.mark.parametrize("width,height", [(40, 24), (24, 40)])
def test_lens_radius_zero_is_the_pinhole(width, height):
    for pose in [CameraPose(location=(-0.0, 1.0, -5.0)), *poses().values()]:
        for focus in (1.0, 7.0):
            for row, col, ux, uy, lu, lv in _samples(width, height, 40, 3):
                o, d = pose.ray(width, height, row, col, ux, uy, lens=CameraLens(0.0, focus), lu=lu, lv=lv)
                po, pd = pose.ray(width, height, row, col, ux, uy)
                assert _bits(o) == _bits(po) and _bits(d) == _bits(pd)
                assert _bits(o) == _bits(pose.location)  # a -0.0 coordinate stays -0.0


def test_lens_rays_pass_through_the_focus_plane_point():
    """The line origin + t direction passes the point where the pinhole ray of the same film point meets the
    focus plane, within 1e-12 (focus_distance + |location|)."""
    g = np.random.default_rng(23)
    width, height = 40, 24
    for pose in [CameraPose(location=CAMERA), *poses().values()]:
        loc, fwd = np.array(pose.location), np.array(pose.forward)
        for lens in (CameraLens(0.4, 12.0), CameraLens(0.05, 3.5), CameraLens(2.0, 40.0)):
            for _ in range(200):
                row, col = int(g.integers(0, height)), int(g.integers(0, width))
                ux, uy, lu, lv = (float(t) for t in g.random(4))
                _, pd = pose.ray(width, height, row, col, ux, uy)
                focus_point = loc + pd * (lens.focus_distance / np.dot(pd, fwd))
                o, d = pose.ray(width, height, row, col, ux, uy, lens=lens, lu=lu, lv=lv)
                rel = focus_point - o
                off = np.linalg.norm(rel - d * np.dot(rel, d))
                assert off <= 1e-12 * (lens.focus_distance + np.linalg.norm(loc)), (pose, lens, off)
                # the origin is on the lens: in the right / up plane, within lens_radius of the location
                assert abs(np.dot(o - loc, fwd)) <= 1e-9 * lens.lens_radius + 1e-14
                assert np.linalg.norm(o - loc) <= lens.lens_radius * (1.0 + 1e-8)


def test_lens_ray_argument_errors():
    L = N.lib()
    p, cl = CameraPose()._c(), CameraLens(0.4, 12.0)._c()
    o, d, out = np.zeros(3), np.zeros(3), np.zeros(2)
    po, pd = o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)
    assert L.vr_camera_lens_ray(C.byref(p), C.byref(cl), 8, 8, 0, 0, 0.0, 0.0, 0.5, 0.5, po, pd) == 0
    assert L.vr_camera_lens_ray(None, C.byref(cl), 8, 8, 0, 0, 0.0, 0.0, 0.5, 0.5, po, pd) == -1
    assert L.vr_camera_lens_ray(C.byref(p), None, 8, 8, 0, 0, 0.0, 0.0, 0.5, 0.5, po, pd) == -1
    assert L.vr_camera_lens_ray(C.byref(p), C.byref(cl), 8, 8, 0, 0, 0.0, 0.0, 0.5, 0.5, None, pd) == -1
    assert L.vr_camera_lens_ray(C.byref(p), C.byref(cl), 8, 8, 0, 0, 0.0, 0.0, 0.5, 0.5, po, None) == -1
    off = CameraLens(0.0, 1.0)._c()
    for lens in (cl, off):
        for w, h, row, col in ((0, 8, 0, 0), (8, 0, 0, 0), (8, 8, 8, 0), (8, 8, 0, 8)):
            assert L.vr_camera_lens_ray(C.byref(p), C.byref(lens), w, h, row, col, 0.0, 0.0, 0.5, 0.5, po, pd) == -1
    assert L.vr_camera_lens_point(0.5, 0.5, None) == -1
    assert L.vr_camera_lens_point(0.5, 0.5, out.ctypes.data_as(C.c_void_p)) == 0


# ------------------------------------------------------------------ set / get
def test_fresh_scene_and_round_trip():
    ds = _host()
    assert lens_bits(ds.camera_lens()) == lens_bits(CameraLens(0.0, 1.0))
    pose = ds.camera_pose()
    for lens in LENSES + [CameraLens(0.0, 1e-3), CameraLens(0.0, 1e6), CameraLens(1e-300, 2.0)]:
        ds.set_camera_lens(lens)
        assert lens_bits(ds.camera_lens()) == lens_bits(lens)
        assert pose_bits(ds.camera_pose()) == pose_bits(pose)  # the lens calls leave the pose alone


def test_set_camera_and_set_camera_pose_keep_the_lens():
    ds = _host()
    lens = CameraLens(0.4, 12.0)
    ds.set_camera_lens(lens)
    ds.set_camera((1.0, 2.0, 3.0))
    assert lens_bits(ds.camera_lens()) == lens_bits(lens)
    for p in poses().values():
        ds.set_camera_pose(p)
        assert lens_bits(ds.camera_lens()) == lens_bits(lens)
        assert pose_bits(ds.camera_pose()) == pose_bits(p)


def test_extent_follows_the_lens_radius():
    ds = _host()
    extent = ds.info()["extent"]
    assert extent == 6.25 + 1.25  # the sphere: |centre x| + radius; the camera's part is 5
    ds.set_camera_lens(CameraLens(2.0, 5.0))
    assert ds.info()["extent"] == extent  # 5 + 2 stays below it
    ds.set_camera_lens(CameraLens(3.0, 5.0))
    assert ds.info()["extent"] == 5.0 + 3.0
    ds.set_camera((1.0, -40.0, 3.0))
    assert ds.info()["extent"] == 40.0 + 3.0  # max |location_c| + lens_radius
    ds.set_camera_pose(poses()["up"])
    assert ds.info()["extent"] == max(extent, 2.0 + 3.0)
    ds.set_camera_lens(CameraLens(0.0, 5.0))
    ds.set_camera(CAMERA)
    assert ds.info()["extent"] == extent


def _bad_lenses():
    for bad in (np.nan, np.inf, -np.inf):
        yield f"lens_radius={bad}", CameraLens(bad, 2.0)
        yield f"focus_distance={bad}", CameraLens(0.5, bad)
    for bad in (-1e-300, -1.0, 1.001e3):
        yield f"lens_radius={bad}", CameraLens(bad, 2.0)
    for bad in (0.0, -1.0, 0.999e-3, 1.001e6):
        yield f"focus_distance={bad}", CameraLens(0.5, bad)


def test_every_error_case_leaves_lens_and_pose_untouched():
    ds = _host()
    L = N.lib()
    kept, pose = CameraLens(0.4, 12.0), poses()["mirrored"]
    ds.set_camera_pose(pose)
    ds.set_camera_lens(kept)
    info = ds.info()
    cases = list(_bad_lenses())
    assert len(cases) == 6 + 3 + 4
    for what, bad in cases:
        assert _code(lambda: ds.set_camera_lens(bad)) == -1, what
        assert lens_bits(ds.camera_lens()) == lens_bits(kept), what
        assert pose_bits(ds.camera_pose()) == pose_bits(pose), what
    assert ds.info() == info
    cl = kept._c()
    assert L.vr_scene_set_camera_lens(None, C.byref(cl)) == -1
    assert L.vr_scene_set_camera_lens(ds.handle, None) == -1
    assert L.vr_scene_get_camera_lens(None, C.byref(cl)) == -1
    assert L.vr_scene_get_camera_lens(ds.handle, None) == -1
    assert lens_bits(ds.camera_lens()) == lens_bits(kept)
    assert pose_bits(ds.camera_pose()) == pose_bits(pose)
