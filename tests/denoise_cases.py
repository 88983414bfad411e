"""Inputs of the denoiser tests (tests/test_denoise_host.py, tests/test_gpu_denoise.py) and their references,
each computed once per session by tests/denoise_reference.py and never modified.

An image has two or three flat regions (columns) of distinct object, normal and depth with a depth ramp down
the rows, positive random colours with some negative X values, random weights and hit counts, and garbage in
the bias half of the state (which the filter must not read).  Special values, each in a corner pixel and in
an interior pixel where the image has both:
    set "a": a NaN colour, a +inf colour, NaN normal sums, distance_sum == 0 with hits > 0
    set "b": a background block (hits == 0) and absent pixels (weight 0)
"""
import functools

import numpy as np

from denoise_reference import denoise_reference
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE

SIGMAS = (0.6, 0.5, 0.1)  # colour, normal, depth: wide enough in colour that neighbours of a region do mix


class Inputs:
    def __init__(self, width, height, state, features, albedo_state, nonfinite):
        self.width, self.height = width, height
        self.state, self.features, self.albedo_state = state, features, albedo_state
        self.nonfinite = nonfinite  # [height][width]: pixels whose own colour is NaN or infinite


def _corners_and_interior(width, height):
    corners = [(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1)]
    cx, cy = width // 2, height // 2
    interior = [(cx, cy), (max(cx - 1, 0), cy), (cx, max(cy - 1, 0)), (min(cx + 1, width - 1), min(cy + 1, height - 1))]
    return corners, interior


@functools.lru_cache(maxsize=None)
def inputs(width, height, seed=1, specials=None, regions=3):
    g = np.random.default_rng([seed, width, height])
    n = width * height
    weight = g.integers(1, 5, (height, width)).astype(np.float64)
    mean = g.uniform(0.05, 2.0, (height, width, 3))
    mean[..., 0] = np.where(g.random((height, width)) < 0.1, -mean[..., 0], mean[..., 0])
    state = g.normal(size=8 * n)  # the bias half stays garbage
    rec = state[:4 * n].reshape(height, width, 4)
    rec[..., :3] = mean * weight[..., None]
    rec[..., 3] = weight

    feat = np.zeros((height, width), dtype=PIXEL_FEATURES_DTYPE)
    region = (np.arange(width) * regions // max(width, 1))[None, :].repeat(height, 0)
    normals = np.array([[0.0, 0.0, -1.0], [0.6, 0.0, -0.8], [0.0, 1.0, 0.0]])
    hits = g.integers(1, 4, (height, width)).astype(np.uint32)
    depth = 2.0 + 3.0 * region + 0.05 * np.arange(height)[:, None]
    feat["hits"] = hits
    feat["samples"] = hits + g.integers(0, 2, (height, width)).astype(np.uint32)
    feat["normal_sum"] = normals[region] * hits[..., None] + g.normal(scale=1e-3, size=(height, width, 3))
    feat["distance_sum"] = depth * hits
    feat["distance_min"] = depth
    feat["object"] = region + 1
    feat["primitive"] = g.integers(0, 100, (height, width))

    # the albedo: channels on both sides of the floor, and pixels of weight 0
    aw = g.integers(0, 4, (height, width)).astype(np.float64)
    amean = g.uniform(0.2, 0.9, (height, width, 3))
    low = g.random((height, width, 3))
    amean = np.where(low < 0.15, 1e-4, np.where(low < 0.25, 0.0, amean))
    albedo = g.normal(size=8 * n)
    arec = albedo[:4 * n].reshape(height, width, 4)
    arec[..., :3] = amean * aw[..., None]
    arec[..., 3] = aw

    nonfinite = np.zeros((height, width), dtype=bool)
    corners, interior = _corners_and_interior(width, height)
    used = set()

    def place(k, fn):
        for x, y in (corners[k % 4], interior[k % 4]):
            if (x, y) not in used:
                used.add((x, y))
                fn(x, y)

    def nan_colour(x, y):
        rec[y, x, 1] = np.nan
        nonfinite[y, x] = True

    def inf_colour(x, y):
        rec[y, x, 0] = np.inf
        nonfinite[y, x] = True

    def nan_normal(x, y):
        feat["normal_sum"][y, x] = np.nan

    def zero_depth(x, y):
        feat["distance_sum"][y, x] = 0.0

    def background(x, y):
        blk = feat[max(y - 1, 0):y + 1, max(x - 1, 0):x + 1]
        blk["hits"] = 0
        blk["normal_sum"] = 0.0
        blk["distance_sum"] = 0.0
        blk["object"] = -1

    def absent(x, y):
        rec[y, x] = 0.0

    if specials == "a":
        for k, fn in enumerate((nan_colour, inf_colour, nan_normal, zero_depth)):
            place(k, fn)
    elif specials == "b":
        place(0, background)
        place(1, absent)
        place(2, background)
        place(3, absent)
    elif specials is not None:
        place(0, {"nan_colour": nan_colour, "inf_colour": inf_colour, "nan_normal": nan_normal,
                  "zero_depth": zero_depth, "background": background, "absent": absent}[specials])
    for a in (state, feat, albedo, nonfinite):
        a.setflags(write=False)
    return Inputs(width, height, state, feat, albedo, nonfinite)


@functools.lru_cache(maxsize=None)
def reference(width, height, iterations, flags=0, seed=1, specials=None, regions=3):
    inp = inputs(width, height, seed, specials, regions)
    out = denoise_reference(width, height, iterations, flags, *SIGMAS, inp.state, inp.features, inp.albedo_state)
    out.setflags(write=False)
    return out
