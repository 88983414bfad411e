"""Helpers of the camera-pose tests (tests/test_camera_pose_host.py, tests/test_gpu_camera_pose.py): the
poses under test and restatements of the library's fixed arithmetic (include/vanrijn_amd.h "Camera pose")
in numpy float64 scalars -- every product and sum a separate IEEE operation, in the header's order -- with
the oracle's normalize (oracle/vr_oracle.c, Vec3::normalize: the sum folds from -0.0, multiply by 1 / norm).
"""
import numpy as np

from vanrijn_amd.scene import CameraPose, look_at

F = np.float64


def film_xy(width, height, row, column, ux, uy):
    """ImageSampler's film point (camera.rs:24-66): the shorter film side is 1."""
    fw, fh = F(width), F(height)
    film_w = fw / fh if fw > fh else F(1.0)
    film_h = F(1.0) if fw > fh else fw / fh
    x = (F(column) + F(ux)) * (film_w * (F(1.0) / fw)) - film_w * F(0.5)
    y = (F(height - (row + 1)) + F(uy)) * (film_h * (F(1.0) / fh)) - film_h * F(0.5)
    return x, y


def rule_ray(oracle, pose: CameraPose, width, height, row, column, ux, uy):
    """The ray rule: d_c = (x * right_c + y * up_c) + film_distance * forward_c, then normalize."""
    x, y = film_xy(width, height, row, column, ux, uy)
    d = [(x * F(pose.right[c]) + y * F(pose.up[c])) + F(pose.film_distance) * F(pose.forward[c]) for c in range(3)]
    return np.array(pose.location, dtype=F), oracle.normalize(d)


def cross(a, b):  # vec3.rs:84-89
    a, b = [F(v) for v in a], [F(v) for v in b]
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def look_at_restated(oracle, eye, target, up_hint, film_distance):
    forward = oracle.normalize([F(t) - F(e) for t, e in zip(target, eye)])
    right = oracle.normalize(cross(up_hint, forward))
    up = cross(forward, right)
    return CameraPose(tuple(float(v) for v in eye), tuple(float(v) for v in right), tuple(float(v) for v in up),
                      tuple(float(v) for v in forward), float(film_distance))


def pose_bits(p: CameraPose):
    return np.array([*p.location, *p.right, *p.up, *p.forward, p.film_distance], dtype=F).tobytes()


def mirrored(p: CameraPose):
    """The same view flipped left to right: a right-handed basis."""
    return CameraPose(p.location, tuple(-v for v in p.right), p.up, p.forward, p.film_distance)


# The three poses, chosen for tests/test_gpu_camera_pose.py's main-like scene (plane y = -2, spheres left of a
# mesh in x [-2.95, -0.45], y [-1.85, 0.25], z [-1.15, 1.15]); each has camera-ray hits and misses in frame:
#  * "look_at": yaw, pitch and roll (a tilted up hint) from the right of the scene's camera, far enough for the
#    mesh's root box to leave the frame's upper corners free, with sky above the mesh;
#  * "up": straight up from in front of the mesh and above its lowest point, film at 0.5 (90 degrees across
#    the short side): the mesh's root box straddles the plane through the camera, so the block cull falls
#    through to its bounding sphere, which the camera is outside of;
#  * "mirrored": a narrow view (film at 2.5) from the scene's own camera with a right-handed basis; the
#    plane's horizon crosses the frame (the plane is edge-on within it).
def poses():
    return {
        "look_at": look_at((1.5, 0.6, -4.5), (-2.2, -0.6, 0.4), (0.2, 1.0, 0.1), 1.0),
        "up": CameraPose((-1.7, -1.5, -2.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 0.5),
        "mirrored": mirrored(look_at((-2.0, 1.0, -5.0), (-1.6, 0.7, 0.0), (0.0, 1.0, 0.0), 2.5)),
    }
