"""The node step's ordered slab test (vr_device.h slab32_ordered) against the pairwise form
(slab32_flags), checked on the CPU with exact f32 emulation.

The 4-wide node stores its child boxes per axis and side (vr_layout.h Node4); the node step reads
each axis's two quads in the order the ray meets them -- the sign bit of the f32 reciprocal that
multiplies in the fma picks the near side -- and takes lo = max3(near), hi = min3(far) without the
per-axis fminf / fmaxf of the pairwise form.  The claim:

* where the ray's margin e2 is finite, near <= far on every axis of a live child, so lo and hi are
  numerically what the pairwise form gives (the sign of a zero may differ), and `sure`, `maybe`, the
  cull decisions against any thresholds and the 32-bit sort key are identical;
* where e2 is infinite (a huge or infinite reciprocal, or an exact_only() ray), NaNs may make lo / hi
  differ, but `sure` is False and `maybe` is True in both forms and the cull thresholds, which carry
  E = e2 / 2 = inf, cull nothing: every live child goes to the exact test either way.

The emulation: numpy float32 products are IEEE round-to-nearest; the fma is the exact f64 product
plus the addend, rounded to odd in f64 (TwoSum gives the sum's error) and then once to f32, which
is the correctly rounded fused result.  The kernel's reciprocal is v_rcp_f32 (within 1 ulp): per
axis the test takes, at random, the correctly rounded reciprocal or either f32 neighbour.
"""
import numpy as np

F32 = np.float32
N_RAYS = 40000  # x 4 child slots = 160,000 box cases
EXTENT = 8.0
MARGIN, BEHIND_MARGIN = 1e-9, 1e-6  # DeviceScene::margin / behind_margin stand-ins (any finite value)


def fma32(a, b, c):
    """RN_f32(a * b + c) for float32 arrays, one rounding."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 + 24 bits
        c = np.broadcast_to(c.astype(np.float64), p.shape)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: p + c = s + err exactly (finite s)
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0.0)
        even = (s.view(np.int64) & 1) == 0
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(inexact & even, np.nextafter(s, toward), s)  # round to odd
        return s.astype(F32)


def reciprocals(d32, rng):
    """1 / d32 correctly rounded, or either f32 neighbour of the exact value (a 1-ulp reciprocal)"""
    with np.errstate(divide="ignore", over="ignore"):
        rn = (F32(1.0) / d32).astype(F32)
        exact = 1.0 / d32.astype(np.float64)
    fin = np.isfinite(rn) & np.isfinite(exact)
    rnd = rn.astype(np.float64)
    down = np.where(rnd <= exact, rn, np.nextafter(rn, F32(-np.inf)))
    up = np.where(rnd >= exact, rn, np.nextafter(rn, F32(np.inf)))
    pick = rng.integers(0, 3, size=rn.shape)
    out = np.where(pick == 0, rn, np.where(pick == 1, down, up)).astype(F32)
    out = np.where(fin & np.isfinite(out), out, rn)
    assert np.array_equal(np.signbit(out), np.signbit(d32))  # a reciprocal keeps its operand's sign
    return out


def round_away_f32(t):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(t, dtype=np.float64).astype(F32) * F32(1.0 + 2.0 ** -22)).astype(F32)


def make_cases(seed):
    rng = np.random.default_rng(seed)
    n = N_RAYS
    # --- boxes: four child slots per node, f32 bounds lo <= hi, some flat, some slots empty
    c = rng.uniform(-EXTENT * 0.8, EXTENT * 0.8, (n, 4, 3))
    h = rng.exponential(0.4, (n, 4, 3))
    flat_axes = rng.integers(0, 4, (n, 4))  # 0..3 axes of zero thickness
    flat = (np.argsort(rng.random((n, 4, 3)), axis=2) < flat_axes[..., None]) & (rng.random((n, 4, 1)) < 0.3)
    h[flat] = 0.0
    lo = np.clip(c - h, -EXTENT, EXTENT).astype(F32)
    hi = np.clip(c + h, -EXTENT, EXTENT).astype(F32)
    hi = np.maximum(hi, lo)
    hi[flat] = lo[flat]
    empty = rng.random((n, 4)) < 0.25
    lo[empty] = np.nan
    hi[empty] = np.nan
    # --- directions: all eight octants; special components
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kind = rng.integers(0, 10, n)
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    sgn = rng.choice([-1.0, 1.0], (n, 3))
    special = np.array([0.0, 1e-40, 1e-39, 1e-30, 1e-160, 1e-12, 1e-6])  # +-0, f32 denormals, overflowing
    # reciprocals (1e-39: denormal, 1 / d > f32 max), e2-overflow (1e-30), exact_only (1e-160), large finite
    m1 = kind == 1  # one special component
    d[rows[m1], ax[m1]] = rng.choice(special, m1.sum()) * sgn[m1, 0]
    m2 = kind == 2  # two special components
    for a in range(2):
        aa = (ax[m2] + a) % 3
        d[rows[m2], aa] = rng.choice(special, m2.sum()) * sgn[m2, a]
    m3 = kind == 3  # axis-aligned: +-1 on one axis, +-0 on the others
    d[m3] = 0.0 * sgn[m3]
    d[rows[m3], ax[m3]] = sgn[m3, 0]
    m4 = (kind == 4) & (rng.random(n) < 0.05)  # the zero vector: invalid, skipped (counted below)
    d[m4] = 0.0 * sgn[m4]
    # --- origins: anywhere; on a bound exactly; inside a child's box
    o = rng.uniform(-EXTENT, EXTENT, (n, 3))
    okind = rng.integers(0, 4, n)
    slot = rng.integers(0, 4, n)
    blo = lo[rows, slot].astype(np.float64)
    bhi = hi[rows, slot].astype(np.float64)
    live_slot = ~empty[rows, slot]
    on = (okind == 1) & live_slot  # o == bound exactly on one axis (lower or upper)
    side = rng.random(n) < 0.5
    o[rows[on], ax[on]] = np.where(side[on], blo[rows[on], ax[on]], bhi[rows[on], ax[on]])
    ins = (okind == 2) & live_slot  # inside (or on, for flat boxes) the box on every axis
    u = rng.random((n, 3))
    o[ins] = (blo + u * (bhi - blo))[ins]
    both = (okind == 3) & live_slot  # on a corner: o == bound on all three axes
    o[both] = np.where(rng.random((n, 3)) < 0.5, blo, bhi)[both]
    valid = np.any(d != 0.0, axis=1)
    return rng, lo, hi, empty, o, d, valid


def kernel_forms(rng, lo, hi, o, d):
    """prepare32 and both slab forms for every (ray, child slot)"""
    d32 = d.astype(F32)
    i32 = reciprocals(d32, rng)
    o32 = o.astype(F32)
    with np.errstate(over="ignore", invalid="ignore"):
        n32 = (-(o32 * i32)).astype(F32)
        big = np.maximum(EXTENT, np.abs(o).max(axis=1)) + 1.0
        m = np.abs(i32).astype(np.float64).max(axis=1)
        ek = 6e-7 * big * m
        exact_only = ~np.all(np.abs(d) > 1e-150, axis=1)
        e2 = np.where(exact_only | ~(ek < 1e30), F32(np.inf), round_away_f32(2.0 * (3.001 * ek))).astype(F32)
    I, Nn = i32[:, None, :], n32[:, None, :]
    t_lo = fma32(lo, np.broadcast_to(I, lo.shape), np.broadcast_to(Nn, lo.shape))  # from the min bounds
    t_hi = fma32(hi, np.broadcast_to(I, hi.shape), np.broadcast_to(Nn, hi.shape))  # from the max bounds
    # pairwise (slab32_flags): NaN-ignoring fminf / fmaxf of each pair, then across the axes
    mn, mx = np.fmin(t_lo, t_hi), np.fmax(t_lo, t_hi)
    p_lo = np.fmax(np.fmax(mn[..., 0], mn[..., 1]), mn[..., 2])
    p_hi = np.fmin(np.fmin(mx[..., 0], mx[..., 1]), mx[..., 2])
    # ordered (slab32_ordered): the near side is the max bound where the reciprocal's sign bit is set
    neg = np.broadcast_to(np.signbit(i32)[:, None, :], lo.shape)
    near, far = np.where(neg, t_hi, t_lo), np.where(neg, t_lo, t_hi)
    q_lo = np.fmax(np.fmax(near[..., 0], near[..., 1]), near[..., 2])
    q_hi = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2])
    return e2, (p_lo, p_hi), (q_lo, q_hi), near, far


def flags(lo, hi, e2):
    with np.errstate(invalid="ignore"):
        dd = (lo - hi).astype(F32)
        return dd < -e2[:, None], ~(dd > e2[:, None])  # sure, maybe


def sort_key(lo):
    return np.maximum(np.ascontiguousarray(lo).view(np.int32), 0)  # the node step's clamp of the entry distance


def test_ordered_form_decides_what_the_pairwise_form_decides():
    rng, lo, hi, empty, o, d, valid = make_cases(7)
    assert (~valid).sum() <= 0.01 * len(valid)  # skipped as invalid (a zero direction): at most 1 %
    assert valid.sum() * 4 >= 100000
    lo, hi, empty, o, d = lo[valid], hi[valid], empty[valid], o[valid], d[valid]
    e2, (p_lo, p_hi), (q_lo, q_hi), near, far = kernel_forms(rng, lo, hi, o, d)
    live = ~empty
    fin = np.isfinite(e2)[:, None] & live
    inf = ~np.isfinite(e2)[:, None] & live
    # the generator reaches both regimes, every octant, flat boxes and empty slots beside live ones
    assert fin.sum() > 50000 and inf.sum() > 10000
    assert len(np.unique(np.signbit(d) @ np.array([1, 2, 4]))) == 8
    assert (empty.any(axis=1) & live.any(axis=1)).sum() > 1000
    assert ((lo == hi).all(axis=2) & live).sum() > 100 and ((lo == hi).any(axis=2) & live).sum() > 1000

    # --- finite e2: the same numbers, hence the same decisions
    assert np.all(np.isfinite(near[fin])) and np.all(np.isfinite(far[fin]))
    assert np.all(near[fin] <= far[fin])  # monotone fma: the sign of the multiplier orders the pair
    assert np.array_equal(p_lo[fin], q_lo[fin]) and np.array_equal(p_hi[fin], q_hi[fin])  # numerically (+0 == -0)
    ps, pm = flags(p_lo, p_hi, e2)
    qs, qm = flags(q_lo, q_hi, e2)
    assert np.array_equal(ps[fin], qs[fin]) and np.array_equal(pm[fin], qm[fin])
    assert ps[fin].any() and (~pm[fin]).any() and (pm & ~ps)[fin].any()  # hits, misses and ties all occur
    assert np.array_equal(sort_key(p_lo)[fin], sort_key(q_lo)[fin])
    # cull decisions against arbitrary thresholds: random ones, and ones at or next to lo / hi themselves
    up, dn = F32(np.inf), F32(-np.inf)
    for cf, cb in [
        (rng.normal(0, 4, p_lo.shape).astype(F32), rng.normal(0, 4, p_lo.shape).astype(F32)),
        (p_lo, p_hi), (q_lo, q_hi),
        (np.nextafter(p_lo, dn), np.nextafter(p_hi, up)), (np.nextafter(q_lo, up), np.nextafter(q_hi, dn)),
        (np.zeros_like(p_lo), np.zeros_like(p_lo)), (-np.zeros_like(p_lo), -np.zeros_like(p_lo)),
        (np.full_like(p_lo, np.inf), np.full_like(p_lo, -np.inf)),
    ]:
        with np.errstate(invalid="ignore"):
            pc = (p_lo > cf) | (p_hi < cb)
            qc = (q_lo > cf) | (q_hi < cb)
        assert np.array_equal(pc[fin], qc[fin])

    # --- infinite e2: nothing is decided in f32 and nothing is culled, in either form
    assert not ps[inf].any() and not qs[inf].any()
    assert pm[inf].all() and qm[inf].all()
    E = 0.5 * e2.astype(np.float64)  # margin_of
    for bound in (np.full(len(e2), np.inf), rng.exponential(3.0, len(e2)), np.zeros(len(e2))):
        with np.errstate(invalid="ignore"):
            cf = round_away_f32(bound + MARGIN * (1.0 + np.abs(bound)) + E)[:, None]  # set_cull_far
            for cb in (round_away_f32(-BEHIND_MARGIN - E)[:, None], F32(-np.inf)):   # behind_ok() or not
                assert not ((p_lo > cf) | (p_hi < cb))[inf].any()
                assert not ((q_lo > cf) | (q_hi < cb))[inf].any()
    # (that regime is where the forms may differ: NaN slab values exist there)
    assert np.isnan(near[inf]).any() or np.isnan(far[inf]).any()


def test_fma_emulation_is_correctly_rounded():
    """the emulated fma against exact rational arithmetic, on operands built to double-round"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.normal(0, 4, 3000).astype(F32)
    b = rng.normal(0, 4, 3000).astype(F32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.normal(0, 1e-7, 3000))).astype(F32)
    c[::3] = rng.normal(0, 4, 1000).astype(F32)
    got = fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        g = float(g)
        lo_n, hi_n = float(np.nextafter(F32(g), F32(-np.inf))), float(np.nextafter(F32(g), F32(np.inf)))
        err = abs(Fraction(g) - exact)
        assert err <= abs(Fraction(lo_n) - exact) and err <= abs(Fraction(hi_n) - exact)
