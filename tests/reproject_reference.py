"""An independent numpy reference of the temporal reprojection's rule (include/vanrijn_amd.h, "Temporal
reprojection"), written from the header's text.

It works on whole-image arrays: every step of the rule is an elementwise f64 expression in the order the
header states (numpy's elementwise add, subtract, multiply, divide, sqrt and floor are single IEEE
operations), the skips are masks applied with np.where, and the four taps are gathered with clipped indices.
It imports nothing of the library: the film constants and the camera ray of the "Camera pose" section are
restated here.  Nothing here shares a line with vanrijn_amd/csrc/vr_reproject.h.
"""
import numpy as np

MATCH_OBJECT = 1


class Pose:
    """location, right, up, forward (3 floats each) and film_distance, as vr_camera_pose."""

    def __init__(self, location=(0.0, 0.0, 0.0), right=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), forward=(0.0, 0.0, 1.0),
                 film_distance=1.0):
        self.location, self.right, self.up, self.forward = (tuple(float(c) for c in v)
                                                            for v in (location, right, up, forward))
        self.film_distance = float(film_distance)

    def fields(self):
        return self.location + self.right + self.up + self.forward + (self.film_distance,)


def film_constants(width, height):
    fw, fh = np.float64(width), np.float64(height)
    film_w = fw / fh if fw > fh else np.float64(1.0)
    film_h = np.float64(1.0) if fw > fh else fw / fh
    return film_w * (1.0 / fw), film_w * 0.5, film_h * (1.0 / fh), film_h * 0.5


def pixel_rays(width, height, pose):
    """Unit directions [height, width, 3] of the pinhole rays through the pixel centres."""
    f0, f1, f2, f3 = film_constants(width, height)
    x = ((np.arange(width, dtype=np.float64) + 0.5) * f0 - f1)[None, :]
    y = (((height - (np.arange(height) + 1)).astype(np.float64) + 0.5) * f2 - f3)[:, None]
    d = [(x * pose.right[c] + y * pose.up[c]) + pose.film_distance * pose.forward[c] for c in range(3)]
    norm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    inv = 1.0 / norm
    return np.stack([d[0] * inv, d[1] * inv, d[2] * inv], axis=-1)


class Footprint:
    """Steps 2-6 for every pixel: `alive` (the pixel reached the taps), g' [.., 3], z', 1 / z', the object, and
    per tap j = 0..3 the row, the column, the weight b and whether the tap is visited at all."""


def footprint(width, height, pose, previous_pose, features, motion=None, motion_count=0):
    feat = np.asarray(features).reshape(height, width)
    fp = Footprint()
    with np.errstate(all="ignore"):
        hits = feat["hits"]
        alive = hits != 0
        inv = 1.0 / hits.astype(np.float64)
        g = feat["normal_sum"] * inv[..., None]
        z = feat["distance_sum"] * inv
        alive = alive & (z > 0.0) & ~np.isinf(z)
        d = pixel_rays(width, height, pose)
        P = np.stack([pose.location[c] + d[..., c] * z for c in range(3)], axis=-1)
        obj = feat["object"]
        has_row = np.zeros((height, width), dtype=bool)
        identity_row = np.zeros((height, width), dtype=bool)
        if motion is not None:
            rows = np.asarray(motion, dtype=np.float64).reshape(-1, 12)
            has_row = (obj >= 0) & (obj < motion_count)
            if motion_count > 0:
                m = rows[np.clip(obj, 0, motion_count - 1)]
                Pm = np.stack([((m[..., 4 * c] * P[..., 0] + m[..., 4 * c + 1] * P[..., 1]) + m[..., 4 * c + 2] * P[..., 2])
                               + m[..., 4 * c + 3] for c in range(3)], axis=-1)
                gm = np.stack([(m[..., 4 * c] * g[..., 0] + m[..., 4 * c + 1] * g[..., 1]) + m[..., 4 * c + 2] * g[..., 2]
                               for c in range(3)], axis=-1)
                P = np.where(has_row[..., None], Pm, P)
                g = np.where(has_row[..., None], gm, g)
                identity_row = (m == np.eye(3, 4).reshape(12)).all(axis=-1)
        same_pose = all(a == b for a, b in zip(pose.fields(), previous_pose.fields()))
        shortcut = same_pose & (~has_row | identity_row)
        # the general path
        pp = previous_pose
        v = [P[..., c] - pp.location[c] for c in range(3)]
        a = (v[0] * pp.right[0] + v[1] * pp.right[1]) + v[2] * pp.right[2]
        bb = (v[0] * pp.up[0] + v[1] * pp.up[1]) + v[2] * pp.up[2]
        c = (v[0] * pp.forward[0] + v[1] * pp.forward[1]) + v[2] * pp.forward[2]
        s = pp.film_distance / c
        xp, yp = a * s, bb * s
        zp = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        f0, f1, f2, f3 = film_constants(width, height)
        fx = (xp + f1) / f0 - 0.5
        fy = (yp + f3) / f2 - 0.5
        fr = np.float64(height - 1) - fy
        inside = (c > 0.0) & (fx >= -1.0) & (fx < np.float64(width)) & (fr >= -1.0) & (fr < np.float64(height))
        fix = np.where(inside, np.floor(fx), 0.0)
        fiy = np.where(inside, np.floor(fr), 0.0)
        tx, ty = fx - fix, fr - fiy
        ix, iy = fix.astype(np.int64), fiy.astype(np.int64)
        row, col = np.indices((height, width))
        fp.tap = []
        for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
            b = (tx if dx else 1.0 - tx) * (ty if dy else 1.0 - ty)
            qy, qx = iy + dy, ix + dx
            visited = inside & (b != 0.0) & ~np.isnan(b) & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
            first = dy == 0 and dx == 0
            qy = np.where(shortcut, row, qy)
            qx = np.where(shortcut, col, qx)
            b = np.where(shortcut, 1.0 if first else 0.0, b)
            visited = np.where(shortcut, first, visited) & alive
            fp.tap.append((np.clip(qy, 0, height - 1), np.clip(qx, 0, width - 1), b, visited))
        fp.alive = alive
        fp.g = g
        fp.z = np.where(shortcut, z, zp)
        fp.iz = np.where(shortcut, 1.0 / z, 1.0 / zp)
        fp.object = obj
        fp.fx, fp.fr, fp.shortcut = fx, fr, shortcut
    return fp


def reproject_reference(width, height, pose, previous_pose, depth_tolerance, normal_tolerance, max_history_weight, flags,
                        state, features, previous_state, previous_features, motion=None, motion_count=0):
    """(out_state, history): the flat output state (8 f64 per pixel) of the rule, and [height][width] booleans
    that say which pixels received history (B != 0)."""
    n = width * height
    cur = np.asarray(state, dtype=np.float64).reshape(-1)[:4 * n].reshape(height, width, 4)
    prev = np.asarray(previous_state, dtype=np.float64).reshape(-1)[:4 * n].reshape(height, width, 4)
    pfeat = np.asarray(previous_features).reshape(height, width)
    fp = footprint(width, height, pose, previous_pose, features, motion, motion_count)
    dt2 = np.float64(depth_tolerance) * np.float64(depth_tolerance)
    nt2 = np.float64(normal_tolerance) * np.float64(normal_tolerance)
    cap = np.float64(max_history_weight)
    with np.errstate(all="ignore"):
        W = cur[..., 3]
        absent = W == 0.0
        B = np.zeros((height, width))
        H = np.zeros((height, width, 3))
        Wh = np.zeros((height, width))
        for qy, qx, b, visited in fp.tap:
            S = prev[qy, qx]
            keep = visited & ~((S - S) != 0.0).any(axis=-1)
            keep &= S[..., 3] != 0.0
            rec = pfeat[qy, qx]
            hq = rec["hits"]
            keep &= hq != 0
            if flags & MATCH_OBJECT:
                keep &= rec["object"] == fp.object
            invq = 1.0 / hq.astype(np.float64)
            zq = rec["distance_sum"] * invq
            t = (zq - fp.z) * fp.iz
            keep &= t * t <= dt2
            m = rec["normal_sum"] * invq[..., None] - fp.g
            keep &= ((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]) <= nt2
            B = np.where(keep, B + b, B)
            H = np.where(keep[..., None], H + b[..., None] * S[..., :3], H)
            Wh = np.where(keep, Wh + b * S[..., 3], Wh)
        history = ~absent & (B != 0.0)
        r = 1.0 / B
        H = H * r[..., None]
        Wh = Wh * r
        over = Wh > cap
        f = cap / Wh
        H = np.where(over[..., None], H * f[..., None], H)
        Wh = np.where(over, cap, Wh)
        with_history = np.concatenate([cur[..., :3] + H, (W + Wh)[..., None]], axis=-1)
    out = np.zeros(8 * n)
    rec = out[:4 * n].reshape(height, width, 4)
    rec[...] = np.where(absent[..., None], 0.0, np.where(history[..., None], with_history, cur))
    return out, history


def same_bits(a, b):
    """Bit for bit, except that a NaN need only be a NaN in the same place; zeros must match in sign."""
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
    if a.shape != b.shape:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a.view(np.uint64)[~nan_a], b.view(np.uint64)[~nan_b]))
