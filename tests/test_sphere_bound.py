"""The f32 sphere pre-test's margin (vr_device.h sphere_maybe32_lanes), checked on the CPU.

begin_ray skips the f64 Sphere::intersect (sphere.rs:39-93) when every lane's f32 estimate says
the LINE passes the sphere by more than 1e-4 |oc|^2 + 1e-12 (|o|^2 + |c|^2) + 2^-120.  That is only sound if
the reference's f64 discriminant b^2 - 4ac is then negative (the reference returns None).  Here the
f32 arithmetic is emulated exactly (numpy float32 operations round each operation to nearest, like
the kernel built with -ffp-contract=off) and the f64 discriminant follows sphere.rs's operation
order, on rays built to graze the sphere (relative offsets 1e-9 .. 1e-1, both sides, origins near
and far).  Every "missed" verdict must have a negative discriminant.

The scale sweep maps the same rays through x -> S x, S = 1e-23 .. 1e20 (centres, radii and offsets):
below S ~ 1e-19 the f32 squares are denormal (or flushed), their quantisation exceeds a purely
relative margin, and without the absolute term 2^-120 real hits are skipped from S = 1e-20 down
(test_the_sweep_needs_the_absolute_term keeps that finding); above S ~ 1e19 the sums overflow and the
test never says "missed".
"""
import numpy as np
import pytest

F32 = np.float32


FLT_MIN = F32(2.0 ** -126)
ABS_TERM = F32(2.0 ** -120)  # vr_device.h sphere_maybe32_lanes: "missed" needs f32 squares in the normal range


def missed32(o, d, c, r, ftz=False, abs_term=ABS_TERM):
    """sphere_maybe32_lanes' verdict, operation by operation.  ftz: every f32 input and result below
    FLT_MIN is flushed to zero (the code objects keep denormals; the margin must not depend on it).
    abs_term=0: the margin as it was before the absolute term."""
    def z(x):
        x = np.asarray(x, dtype=F32)
        return np.where(np.abs(x) < FLT_MIN, F32(0.0) * x, x).astype(F32) if ftz else x

    ox, oy, oz = (z(F32(o[:, k] - c[:, k])) for k in range(3))
    dx, dy, dz = (z(d[:, k].astype(F32)) for k in range(3))
    t = z(z(z(ox * dx) + z(oy * dy)) + z(oz * dz))
    oc2 = z(z(z(ox * ox) + z(oy * oy)) + z(oz * oz))
    rf = z(r.astype(F32))
    o32 = z(o.astype(F32))
    c32 = z(c.astype(F32))
    po = z(z(z(o32[:, 0] * o32[:, 0]) + z(o32[:, 1] * o32[:, 1])) + z(o32[:, 2] * o32[:, 2]))
    pc = z(z(z(c32[:, 0] * c32[:, 0]) + z(c32[:, 1] * c32[:, 1])) + z(c32[:, 2] * c32[:, 2]))
    lhs = z(z(oc2 - z(t * t)) - z(rf * rf))
    rhs = z(z(z(F32(1e-4) * oc2) + z(F32(1e-12) * z(po + pc))) + abs_term)
    return lhs > rhs


def discriminant(o, d, c, r):
    """sphere.rs:43-59: a, b, c from component products, folded from 0.0; b^2 - 4ac."""
    a = ((0.0 + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    bv = 2.0 * (o * d - c * d)
    b = ((0.0 + bv[:, 0]) + bv[:, 1]) + bv[:, 2]
    cv = (o * o + c * c) - 2.0 * (c * o)
    cc = ((0.0 + cv[:, 0]) + cv[:, 1]) + cv[:, 2]
    cc = cc - r * r
    return b * b - 4.0 * a * cc


def _grazing(rng, n, scale, far):
    c = rng.uniform(-scale, scale, (n, 3))
    r = rng.uniform(0.05, 3.0, n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = rng.normal(size=(n, 3))
    p -= (p * d).sum(1, keepdims=True) * d
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    rel = 10.0 ** rng.uniform(-9, -1, n) * rng.choice([-1.0, 1.0], n)
    s = rng.uniform(-far, far, n)
    o = c + p * (r * (1.0 + rel))[:, None] + d * s[:, None]
    return o, d, c, r


def test_missed_implies_negative_discriminant():
    rng = np.random.default_rng(0x5EED)
    total_skips = 0
    for scale, far in ((10.0, 20.0), (10.0, 1e3), (1e3, 50.0), (1.0, 5.0)):
        o, d, c, r = _grazing(rng, 200_000, scale, far)
        m = missed32(o, d, c, r)
        delta = discriminant(o, d, c, r)
        assert (delta[m] < 0.0).all(), np.flatnonzero(m & ~(delta < 0.0))[:5]
        total_skips += int(m.sum())
    assert total_skips > 30_000  # the margin still lets clear misses (rel >~ 1e-4) be skipped


def test_clear_misses_and_hits():
    rng = np.random.default_rng(7)
    o, d, c, r = _grazing(rng, 10_000, 10.0, 20.0)
    # lines at 1.5 r: skipped; lines through the centre: never skipped
    d2 = d.copy()
    p = rng.normal(size=d.shape)
    p -= (p * d2).sum(1, keepdims=True) * d2
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    far_o = c + p * (1.5 * r)[:, None] + d2 * rng.uniform(-5, 5, (len(r), 1))
    assert missed32(far_o, d2, c, r).all()
    centre_o = c + d2 * rng.uniform(-5, 5, (len(r), 1))
    assert not missed32(centre_o, d2, c, r).any()


# ------------------------------------------------------------------------------- the scale sweep
SWEEP_EXPONENTS = tuple(range(-23, 21))
_GRAZING_SHAPES = ((10.0, 20.0), (10.0, 1e3), (1e3, 50.0), (1.0, 5.0))  # (scale, far) as above


def _scaled_grazing(exponent):
    """400,000 grazing rays of the unit recipe, centres, radii and offsets multiplied by S = 10^exponent."""
    S = 10.0 ** exponent
    rng = np.random.default_rng(0x5CA1E + exponent)
    parts = [_grazing(rng, 100_000, scale, far) for scale, far in _GRAZING_SHAPES]
    o, d, c, r = (np.concatenate([p[k] for p in parts]) for k in range(4))
    return o * S, d, c * S, r * S


@pytest.mark.parametrize("ftz", [False, True], ids=["denormals", "flushed"])
@pytest.mark.parametrize("exponent", SWEEP_EXPONENTS)
def test_missed_implies_negative_discriminant_at_every_scale(exponent, ftz):
    o, d, c, r = _scaled_grazing(exponent)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        m = missed32(o, d, c, r, ftz=ftz)
        delta = discriminant(o, d, c, r)
    wrong = m & ~(delta < 0.0)
    assert not wrong.any(), (int(wrong.sum()), np.flatnonzero(wrong)[:5])
    # what the pre-test is for: between the underflow and the overflow of the squares it still skips
    # the clear misses (at S = 1 about a tenth of these grazing rays), outside it skips nothing
    if -16 <= exponent <= 16:
        assert m.sum() > 30_000
    if exponent <= -20 or exponent >= 20:
        assert not m.any()


def test_the_sweep_needs_the_absolute_term():
    """The finding the absolute term answers: with the relative margin alone, real hits are skipped
    at S = 1e-21 (3,270 of these 400,000, up to 4 % of the radius inside the limb; 21,496 at 1e-22, up to
    10 %; with denormals flushed, 339 at 1e-19 instead)."""
    o, d, c, r = _scaled_grazing(-21)
    with np.errstate(under="ignore"):
        m = missed32(o, d, c, r, abs_term=F32(0.0))
        delta = discriminant(o, d, c, r)
    assert (m & ~(delta < 0.0)).sum() > 1000


def test_absolute_term_changes_no_verdict_at_ordinary_scales():
    rng = np.random.default_rng(0x5EED)
    for scale, far in _GRAZING_SHAPES:
        o, d, c, r = _grazing(rng, 100_000, scale, far)
        assert np.array_equal(missed32(o, d, c, r), missed32(o, d, c, r, abs_term=F32(0.0)))
