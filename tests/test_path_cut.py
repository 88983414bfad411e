"""The forward (iterative) form of SimpleRandomIntegrator's recursion, with cut levels, on the CPU.

The reference returns from the innermost level outward: I_k = bsdf_k(I_{k+1} pdf_k |cos_k|), an
affine map a_k I_{k+1} + b_k -- except that a mirror or Phong surface met from behind returns the
constant 0 without reading I_{k+1} (reflective_material.rs:20-24, phong_material.rs:19-21).  The
kernels (vr_render_kernel.h shade(), vr_integrate.hip) accumulate outward-in, Acc += T b_k, T *= a_k, and
a cut level used to be a_k = b_k = 0 like any other: a NaN below it (a bounce ray that re-hits its
own surface at distance 0 -- every trapped path of a scene scaled by 1e20, tests/test_gpu_magnitudes.py)
then made T = 0 * NaN where the reference has discarded it.  Found on the device at (1e20, 0),
(3e34, 0) and (1e36, 0): 6, 9 and 12 of 5,760 samples NaN where the oracle's are finite.  Since then
the kernels freeze Acc and T from the first cut level on (kPathCut) and drop the path's end term.

Here both forms are restated with factors that are powers of two (so the two associations agree bit
for bit), NaN and zero factors at random levels, and both ends of a path (the sky term; the
recursion limit's 0 in the lambda-0 channel).  Infinite factors are left out: with or without cut
levels the forward form gives inf * 0 = NaN where the recursion keeps an infinity, and no level's
pdf |cos| colour product is infinite for finite hit records.
"""
import math

import numpy as np

NAN = float("nan")


def recursive(levels, end):
    """levels: [(a, b, cut)] from the camera hit inward; end: what the innermost call returns"""
    def go(k):
        if k == len(levels):
            return end
        below = go(k + 1)  # traced and evaluated whether or not it is read
        a, b, cut = levels[k]
        return 0.0 if cut else below * a + b
    return go(0)


def forward(levels, end, freeze=True):
    acc, t, dead = 0.0, 1.0, False
    for a, b, cut in levels:
        if cut:
            a, b = 0.0, 0.0
        if not (freeze and dead):
            acc = acc + t * b
            t = t * a
        dead = dead or cut
    return acc if (freeze and dead) else acc + t * end


def _same(x, y):
    return (math.isnan(x) and math.isnan(y)) or x == y


def _paths(rng, count, special):
    for _ in range(count):
        n = int(rng.integers(1, 12))
        levels = []
        for _ in range(n):
            a = float(2.0 ** rng.integers(-3, 1))
            b = float(rng.choice([0.0, 0.5, 0.25]))
            u = rng.random()
            if special and u < 0.15:
                a = float(rng.choice([NAN, 0.0]))
            elif special and u < 0.2:
                b = NAN
            levels.append((a, b, bool(special and rng.random() < 0.2)))
        end = float(rng.choice([0.0, 1.0, 0.75] + ([NAN] if special else [])))
        yield levels, end


def test_forward_form_equals_the_recursion():
    rng = np.random.default_rng(0xC07)
    cut_then_nan = 0
    for levels, end in _paths(rng, 20000, special=True):
        want = recursive(levels, end)
        assert _same(forward(levels, end), want), (levels, end)
        first_cut = next((k for k, lv in enumerate(levels) if lv[2]), None)
        if first_cut is not None and not math.isnan(want):
            below = levels[first_cut + 1:]
            cut_then_nan += any(math.isnan(a) or math.isnan(b) for a, b, _ in below) or math.isnan(end)
    assert cut_then_nan > 500  # finite results whose discarded tail holds a NaN


def test_without_the_freeze_a_discarded_nan_comes_back():
    """The finding: a = b = 0 at the cut level alone is not the reference's discard"""
    levels = [(0.5, 0.5, False), (1.0, 0.0, True), (NAN, 0.0, False)]
    assert recursive(levels, 0.0) == 0.5
    assert forward(levels, 0.0) == 0.5
    assert math.isnan(forward(levels, 0.0, freeze=False))
    assert recursive(levels[:2], NAN) == 0.5 and forward(levels[:2], NAN) == 0.5  # a NaN sky term below a cut


def test_without_special_values_the_freeze_changes_nothing():
    rng = np.random.default_rng(0xC08)
    for levels, end in _paths(rng, 5000, special=False):
        assert forward(levels, end) == forward(levels, end, freeze=False) == recursive(levels, end)
