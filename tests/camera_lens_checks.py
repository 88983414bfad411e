"""Helpers of the camera-lens tests (tests/test_camera_lens_host.py, tests/test_gpu_camera_lens.py):
restatements of the library's fixed lens arithmetic (include/vanrijn_amd.h "Camera lens",
vanrijn_amd/csrc/vr_camera.h) in numpy float64 scalars -- every product, quotient and sum a separate IEEE
operation, in the header's order -- and the lenses under test.
"""
import numpy as np

from camera_pose_checks import film_xy
from vanrijn_amd.scene import CameraLens, CameraPose

F = np.float64
PI = F(3.14159265358979323846)

# Taylor coefficients, highest power first: sin through x^15 (times x), cos through x^16; Horner in x * x
SIN_TERMS = [F(-1.0) / F(1307674368000.0), F(1.0) / F(6227020800.0), F(-1.0) / F(39916800.0), F(1.0) / F(362880.0),
             F(-1.0) / F(5040.0), F(1.0) / F(120.0), F(-1.0) / F(6.0), F(1.0)]
COS_TERMS = [F(1.0) / F(20922789888000.0), F(-1.0) / F(87178291200.0), F(1.0) / F(479001600.0), F(-1.0) / F(3628800.0),
             F(1.0) / F(40320.0), F(-1.0) / F(720.0), F(1.0) / F(24.0), F(-1.0) / F(2.0), F(1.0)]


def _horner(terms, z):
    p = terms[0]
    for t in terms[1:]:
        p = p * z
        p = p + t
    return p


def poly_sin(x):
    x = F(x)
    return x * _horner(SIN_TERMS, x * x)


def poly_cos(x):
    x = F(x)
    return _horner(COS_TERMS, x * x)


def disc(lu, lv, sin=poly_sin, cos=poly_cos):
    """Shirley's concentric map as unit_disc.rs:28-40 states it, over ox = 2 lu - 1, oy = 2 lv - 1; the second
    branch's angle pi / 2 - phi has cosine sin phi and sine cos phi."""
    ox, oy = F(2.0) * F(lu) - F(1.0), F(2.0) * F(lv) - F(1.0)
    if ox == 0.0 and oy == 0.0:
        return ox, oy
    if abs(ox) > abs(oy):
        phi = ((PI / F(4.0)) * oy) / ox
        return ox * cos(phi), ox * sin(phi)
    phi = ((PI / F(4.0)) * ox) / oy
    return oy * sin(phi), oy * cos(phi)


def lens_rule_ray(oracle, pose: CameraPose, lens: CameraLens, width, height, row, column, ux, uy, lu, lv):
    """The lens rule: the lens point (a, b), the origin location + (a right + b up), and the direction of the
    ray rule at the film point shifted by -(a, b) k, k = film_distance / focus_distance."""
    x, y = film_xy(width, height, row, column, ux, uy)
    dx, dy = disc(lu, lv)
    fd = F(pose.film_distance)
    k = fd / F(lens.focus_distance)
    a, b = F(lens.lens_radius) * dx, F(lens.lens_radius) * dy
    right, up, forward = ([F(v) for v in axis] for axis in (pose.right, pose.up, pose.forward))
    origin = [F(pose.location[c]) + (a * right[c] + b * up[c]) for c in range(3)]
    xs, ys = x - a * k, y - b * k
    d = [(xs * right[c] + ys * up[c]) + fd * forward[c] for c in range(3)]
    return np.array(origin, dtype=F), oracle.normalize(d)


def lens_bits(lens: CameraLens):
    return np.array([lens.lens_radius, lens.focus_distance], dtype=F).tobytes()


def lens_draws_grid(n=33):
    """(lu, lv): a grid with both ends of [0, 1) and the centre, the diagonals |ox| == |oy| (exactly: lv = lu and
    lv = 1 - lu on dyadic lu), the four corners, and points well inside both branches."""
    top = 1.0 - 2.0 ** -53
    g = [min(i / (n - 1), top) for i in range(n)]
    pts = [(u, v) for u in g for v in g]
    dyadic = [i / 64.0 for i in range(1, 64)]
    pts += [(u, u) for u in dyadic] + [(u, 1.0 - u) for u in dyadic]
    pts += [(0.0, 0.0), (0.0, top), (top, 0.0), (top, top), (0.5, 0.5)]
    pts += [(0.9, 0.45), (0.1, 0.6), (0.45, 0.9), (0.6, 0.1)]  # |ox| > |oy| twice, then the other branch twice
    return pts
