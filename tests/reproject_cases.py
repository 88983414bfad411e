"""Inputs of the reprojection tests (tests/test_reproject_host.py, tests/test_gpu_reproject.py) and their
references, each computed once per session by tests/reproject_reference.py and never modified.

The scene is analytic: two spheres (objects 0 and 1) over a ground plane (object 2) under an empty sky, seen
through the pinhole rays of the pixel centres.  For any pose, and any rigid placement of the objects, it
yields hits, normal_sum, distance_sum and object per pixel; the hit counts are random (1..3), so the sums
are multiples of the means.  Colour states are random and positive, with random weights and garbage in the
bias half (which the rule must not read).

Special values (`specials`), placed in the previous or the current frame at pixels of the interior that the
moved-pose footprints touch:
    "nan_sum" / "inf_sum"      a NaN / +inf in a previous colour sum, and an infinite previous weight
    "nan_prev_normal"          NaN previous normal sums
    "nan_cur_normal"           NaN current normal sums
    "zero_depth" / "nan_depth" distance_sum 0 / NaN with hits > 0, in both frames
    "absent_prev" / "absent_cur"   weight 0 records
    "background"               hits == 0 blocks in both frames (besides the sky, which every case has)
    "other_object"             previous pixels of the same geometry under another object id
    "mixed"                    all of the above at once, at different pixels
"""
import functools
import math

import numpy as np

from reproject_reference import MATCH_OBJECT, Pose, footprint, pixel_rays, reproject_reference
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE

TOLERANCES = (0.05, 0.25)  # depth, normal: the library's defaults
SPHERES = (((-0.7, -0.1, 4.0), 0.9), ((1.0, 0.2, 5.5), 1.1))  # objects 0 and 1: centre, radius
PLANE_Y = -1.0                                                 # object 2: the plane y = PLANE_Y, normal +y
IDENTITY = np.eye(3, 4).reshape(12)
SPECIALS = ["nan_sum", "inf_sum", "nan_prev_normal", "nan_cur_normal", "zero_depth", "nan_depth", "absent_prev",
            "absent_cur", "background", "other_object", "mixed"]


def rotation(axis, degrees):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    t = math.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def turned(yaw_degrees=0.0, pitch_degrees=0.0, location=(0.0, 0.0, 0.0), film_distance=1.0):
    """The default pose turned about +y and then about its own right axis; an exactly orthonormal basis is
    not needed, only one within the library's 1e-9."""
    R = rotation((0, 1, 0), yaw_degrees) @ rotation((1, 0, 0), pitch_degrees)
    return Pose(location, R[:, 0], R[:, 1], R[:, 2], film_distance)


BASE = Pose()
# name -> (pose, previous_pose).  The steps are sized for 37 x 29, where a pixel spans 0.034 of film.
POSES = {
    "identical": (BASE, BASE),
    "translation": (Pose(location=(0.03, 0.01, -0.02)), BASE),
    "rotation": (turned(2.5, -1.0), BASE),
    "film_distance": (Pose(film_distance=1.08), BASE),
    "out_of_frame": (turned(21.0), BASE),          # a third of the 65-degree view leaves the frame
    "turned_away": (BASE, turned(180.0)),          # the previous camera looks the other way: c <= 0 everywhere
}
MOVED = ["translation", "rotation", "film_distance", "out_of_frame"]  # the cases that must find history

# name -> rows (current -> previous position); None: no motion array at all
MOTIONS = {
    "none": None,
    "identity": np.stack([IDENTITY] * 3),
    "translation": np.stack([np.hstack([np.eye(3), [[0.5], [0.2], [-0.3]]]).reshape(12), IDENTITY, IDENTITY]),
    "rotation": np.stack([IDENTITY, np.hstack([rotation((0.2, 1.0, 0.1), 3.0), [[0.05], [0.0], [0.02]]]).reshape(12),
                          IDENTITY]),
    "first_only": np.hstack([np.eye(3), [[-0.03], [0.03], [0.0]]]).reshape(1, 12),
}


def trace(width, height, pose, placement=None):
    """(hit [h, w] bool, normal [h, w, 3], distance [h, w], object [h, w]) of the scene; `placement`: rows
    [A | t] that move the spheres (objects 0, 1) rigidly from where SPHERES puts them."""
    d = pixel_rays(width, height, pose)
    o = np.asarray(pose.location)
    best = np.full((height, width), np.inf)
    normal = np.zeros((height, width, 3))
    obj = np.full((height, width), -1, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i, (centre, radius) in enumerate(SPHERES):
            c = np.asarray(centre, dtype=np.float64)
            if placement is not None and i < len(placement):
                m = np.asarray(placement[i]).reshape(3, 4)
                c = m[:, :3] @ c + m[:, 3]
            oc = o - c
            b = (d * oc).sum(-1)
            disc = b * b - ((oc * oc).sum() - radius * radius)
            t = -b - np.sqrt(disc)
            ok = (disc > 0) & (t > 1e-9) & (t < best)
            best = np.where(ok, t, best)
            normal = np.where(ok[..., None], ((o + d * t[..., None]) - c) / radius, normal)
            obj = np.where(ok, i, obj)
        t = (PLANE_Y - o[1]) / d[..., 1]
        ok = (t > 1e-9) & (t < best) & (t < 60.0)  # the far plane fades into the sky
        best = np.where(ok, t, best)
        normal = np.where(ok[..., None], np.array([0.0, 1.0, 0.0]), normal)
        obj = np.where(ok, 2, obj)
    hit = obj >= 0
    return hit, normal, np.where(hit, best, 0.0), obj


def feature_records(g, width, height, pose, placement=None):
    hit, normal, distance, obj = trace(width, height, pose, placement)
    feat = np.zeros((height, width), dtype=PIXEL_FEATURES_DTYPE)
    hits = np.where(hit, g.integers(1, 4, (height, width)), 0).astype(np.uint32)
    feat["hits"] = hits
    feat["samples"] = 3
    feat["normal_sum"] = normal * hits[..., None]
    feat["distance_sum"] = distance * hits
    feat["distance_min"] = distance
    feat["object"] = obj
    feat["primitive"] = np.where(hit, 0, -1)
    return feat


def colour_state(g, width, height):
    n = width * height
    state = g.normal(size=8 * n)  # the bias half stays garbage
    rec = state[:4 * n].reshape(height, width, 4)
    weight = g.integers(1, 9, (height, width)).astype(np.float64)
    rec[..., :3] = g.uniform(0.05, 2.0, (height, width, 3)) * weight[..., None]
    rec[..., 3] = weight
    return state


class Inputs:
    def __init__(self, width, height, pose, previous_pose, state, features, previous_state, previous_features, motion):
        self.width, self.height, self.pose, self.previous_pose = width, height, pose, previous_pose
        self.state, self.features = state, features
        self.previous_state, self.previous_features = previous_state, previous_features
        self.motion = motion
        self.motion_count = 0 if motion is None else len(motion)


def _special_pixels(width, height, count):
    """`count` distinct interior pixels (x, y), spread over the lower half where the plane and the spheres are."""
    g = np.random.default_rng([99, width, height])
    seen = []
    while len(seen) < count:
        x, y = int(g.integers(0, width)), int(g.integers(height // 3, height))
        if (x, y) not in seen:
            seen.append((x, y))
        if len(seen) == width * (height - height // 3):
            break
    return seen


@functools.lru_cache(maxsize=None)
def inputs(width, height, poses="translation", motion="none", specials=None, seed=1):
    g = np.random.default_rng([seed, width, height])
    pose, previous_pose = POSES[poses]
    rows = MOTIONS[motion]
    feat = feature_records(g, width, height, pose)
    pfeat = feature_records(g, width, height, previous_pose, rows)  # the objects were where the rows put them
    state, pstate = colour_state(g, width, height), colour_state(g, width, height)
    rec = state[:4 * width * height].reshape(height, width, 4)
    prec = pstate[:4 * width * height].reshape(height, width, 4)

    def apply(kind, x, y):
        if kind == "nan_sum":
            prec[y, x, 1] = np.nan
        elif kind == "inf_sum":
            prec[y, x, 0] = np.inf
            prec[y, (x + 2) % width, 3] = np.inf
        elif kind == "nan_prev_normal":
            pfeat["normal_sum"][y, x] = np.nan
        elif kind == "nan_cur_normal":
            feat["normal_sum"][y, x] = np.nan
        elif kind == "zero_depth":
            feat["distance_sum"][y, x] = 0.0
            pfeat["distance_sum"][y, (x + 2) % width] = 0.0
        elif kind == "nan_depth":
            feat["distance_sum"][y, x] = np.nan
            pfeat["distance_sum"][y, (x + 2) % width] = np.nan
        elif kind == "absent_prev":
            prec[y, x] = 0.0
        elif kind == "absent_cur":
            rec[y, x] = 0.0
        elif kind == "other_object":
            pfeat["object"][max(y - 1, 0):y + 1, max(x - 1, 0):x + 1] = 7
        elif kind == "background":
            for f in (feat, pfeat):
                blk = f[max(y - 1, 0):y + 1, max(x - 1, 0):x + 1]
                blk["hits"] = 0
                blk["normal_sum"] = 0.0
                blk["distance_sum"] = 0.0
                blk["object"] = -1
                x = (x + 3) % width

    if specials == "mixed":
        kinds = SPECIALS[:-1] * 2
        for kind, (x, y) in zip(kinds, _special_pixels(width, height, len(kinds))):
            apply(kind, x, y)
    elif specials is not None:
        for x, y in _special_pixels(width, height, 3):
            apply(specials, x, y)
    for a in (state, feat, pstate, pfeat):
        a.setflags(write=False)
    return Inputs(width, height, pose, previous_pose, state, feat, pstate, pfeat, rows)


@functools.lru_cache(maxsize=None)
def reference(width, height, poses="translation", motion="none", specials=None, flags=MATCH_OBJECT, cap=math.inf, seed=1):
    """(out_state, history) of the reference on inputs(...)."""
    inp = inputs(width, height, poses, motion, specials, seed)
    out, history = reproject_reference(width, height, inp.pose, inp.previous_pose, *TOLERANCES, cap, flags, inp.state,
                                       inp.features, inp.previous_state, inp.previous_features, inp.motion,
                                       inp.motion_count)
    out.setflags(write=False)
    history.setflags(write=False)
    return out, history


def history_share(inp, history):
    """The share of the current frame's hit pixels that received history."""
    hit = inp.features["hits"] > 0
    return float(history[hit].sum()) / max(int(hit.sum()), 1)


@functools.lru_cache(maxsize=None)
def zero_weight_tap(width=37, height=29):
    """Inputs in which one footprint has a tap of weight exactly 0 that holds a NaN.  The camera steps sideways
    by `step`; a pixel at depth z then lands fx = column + shift(z) in the previous frame.  The depth of one
    plane pixel is searched, one representable value at a time around the depth where shift(z) = 1, until
    the reference's own fx is a whole number: then tx == 0, tap (0,1) has b == 0 and is never read, and the
    NaN put there must reach nothing.  Returns (Inputs, (row, column), (tap row, tap column))."""
    base = inputs(width, height, "translation")
    pose, previous_pose = Pose(location=(0.125, 0.0, 0.0)), BASE
    feat = feature_records(np.random.default_rng(5), width, height, pose)
    pfeat = feature_records(np.random.default_rng(6), width, height, previous_pose)
    row, column = height - 4, width // 2
    assert feat["object"][row, column] == 2
    feat["hits"][row, column] = 1
    feat["normal_sum"][row, column] = (0.0, 1.0, 0.0)
    f0 = (width / height) / width
    z = 0.125 / f0 / pixel_rays(width, height, pose)[row, column, 2]  # shift(z) = step / (z * d_z * f0) is near 1 here
    found = None
    for direction in (1.0, -1.0):
        value = z
        for _ in range(4096):
            feat["distance_sum"][row, column] = value
            fp = footprint(width, height, pose, previous_pose, feat)
            fx = fp.fx[row, column]
            if fx == np.floor(fx):
                found = value
                break
            value = np.nextafter(value, direction * np.inf)
        if found is not None:
            break
    assert found is not None, "no depth gives a whole fx"
    fx, fr = fp.fx[row, column], fp.fr[row, column]
    tap = (int(np.floor(fr)), int(fx) + 1)
    assert 0 <= tap[1] < width and 0 <= tap[0] < height
    # the tap pixel's own depth passes against the searched one, so only its weight keeps the NaN out
    pfeat["distance_sum"][row, column + 1:column + 3] = found * pfeat["hits"][row, column + 1:column + 3]
    pfeat["distance_sum"][row, column] = found * pfeat["hits"][row, column]
    pstate = base.previous_state.copy()
    pstate[:4 * width * height].reshape(height, width, 4)[tap[0], tap[1], 1] = np.nan
    for a in (feat, pfeat, pstate):
        a.setflags(write=False)
    return Inputs(width, height, pose, previous_pose, base.state, feat, pstate, pfeat, None), (row, column), tap
