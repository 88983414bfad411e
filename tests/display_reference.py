"""Exact references for the display end of the path, and the input sets its tests share.

What follows the photon -- the ordered reduce (accumulate_kernel: CIE lobes, then update_pixel's
Kahan chain), film_merge_kernel and tonemap_kernel -- is compared here with references that do not
share the kernels' arithmetic:

* the lobes and the gamma curve in the standard library's `decimal` at 80 digits, with derived bounds
  (`colour_bound`, the `ambiguous` band of `tone_map_exact`) on how far IEEE doubles may lie from them;
* the Kahan chain and the film merge as numpy f64 replays: they use only +, -, * and / on doubles,
  every one correctly rounded, so the device must agree bit for bit.

tests/test_display_reference.py holds these references to the oracle; tests/test_gpu_display.py holds
the kernels to them.  Both read their inputs from the builders at the end of this file.
"""
import math
from decimal import Context, Decimal, localcontext

import numpy as np

from vanrijn_amd.render import Tile

PRECISION = 80  # decimal digits: a double has at most 53 bits, its square 106 (32 digits)
U = Decimal(2) ** -53  # the unit roundoff of f64
TINY = Decimal(2) ** -1074  # the smallest subnormal
MAX_ULP = 2  # vr_exp_tab against exp (tests/test_exp_table.py)

# colour_xyz.rs:86-103: (channel, alpha, mu, sigma below mu, sigma above mu)
LOBES = ((0, 1.056, 599.8, 37.9, 31.0), (0, 0.362, 442.0, 16.0, 26.7), (0, -0.065, 501.1, 20.4, 26.2),
         (1, 0.821, 568.8, 46.9, 40.5), (1, 0.286, 530.9, 16.3, 31.1),
         (2, 1.217, 437.0, 11.8, 36.0), (2, 0.681, 459.0, 26.0, 13.8))
LOBE_MUS = tuple(l[2] for l in LOBES)
PDF_SCALE = 360.0  # photon.rs:26-28: LONGEST_VISIBLE - SHORTEST_VISIBLE


def _ctx():
    return localcontext(Context(prec=PRECISION))


def same_bits(a, b):
    """Equal bit for bit, NaNs compared by position (the sign and payload of a NaN that an invalid
    operation makes are the machine's choice: x86 gives the negative quiet NaN, the GPU the positive)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


def step(x, n):
    """The double n ulps above x (below for n < 0); x finite and positive, and so is the result."""
    b = np.array([x], dtype=np.float64).view(np.int64)
    b[0] += n
    assert 0 < b[0] < 0x7FF0000000000000
    return float(b.view(np.float64)[0])


# ------------------------------------------------------------------------------------------------
# The CIE lobes
# ------------------------------------------------------------------------------------------------
_LOBE_CACHE = {}


def lobes_exact(wl):
    """ColourXyz::for_wavelength (colour_xyz.rs:86-103) of the double `wl`, exactly.

    Returns (sums, terms): sums[c] the channel's exact value as a Decimal, and terms[c] a list of
    (alpha_i * E_i, x_i) over the channel's lobes, with E_i = exp(x_i), x_i = -(wl - mu_i)^2 * k_i.
    alpha, mu and k = 1 / (2 s^2) are the exact binary values of the doubles the kernel holds (k as
    the compiler folds it: s * s, 2.0 * that, 1.0 / that, each rounded once), and the side of the lobe
    is chosen by `wl < mu` on doubles as the kernel and the reference choose it.  Everything after
    that is real arithmetic at 80 digits.  x_i below -1000 counts as E_i = 0: the true value is under
    1e-434, beyond every double (colour_bound's absolute term covers it).  An infinite wavelength gives
    x_i = -Infinity, E_i = 0.  NaN gives None."""
    wl = float(wl)
    if wl != wl:
        return None
    if wl in _LOBE_CACHE and (wl != 0.0 or math.copysign(1.0, wl) > 0):
        return _LOBE_CACHE[wl]
    sums, terms = [Decimal(0)] * 3, ([], [], [])
    with _ctx():
        for c, alpha, mu, s1, s2 in LOBES:
            s = s1 if wl < mu else s2
            k = 1.0 / (2.0 * (s * s))
            if math.isinf(wl):
                x, e = Decimal("-Infinity"), Decimal(0)
            else:
                t = Decimal(wl) - Decimal(mu)
                x = -(t * t) * Decimal(k)
                e = x.exp() if x >= -1000 else Decimal(0)
            term = Decimal(alpha) * e
            terms[c].append((term, x))
            sums[c] = sums[c] + term
    out = (tuple(sums), terms)
    _LOBE_CACHE[wl] = out
    return out


def colour_exact(wl, intensity):
    """ColourXyz::from_photon scaled as the reduce scales it: lobes_exact(wl) * 360 * I, exactly."""
    sums, _ = lobes_exact(wl)
    with _ctx():
        scale = Decimal(PDF_SCALE) * Decimal(float(intensity))
        return tuple(s * scale for s in sums)


def colour_bound(wl, intensity):
    """How far the device colour of the photon {wl, I} may lie from colour_exact, per channel.

    Derivation (u = 2^-53; every f64 operation is correctly rounded, relative error <= u each; the
    kernel computes alpha * exp_tab(-(t * t) * k), t = wl - mu, then sums the channel and multiplies
    by Is = I * 360):

      argument   t carries one rounding, so t*t carries 2u from it and u of its own, and the product
                 with k another u (k is taken as the kernel's binary constant, so its own rounding is
                 in x_i already): the computed argument is x_i (1 + d), |d| <= 4u.  exp(x (1 + d)) =
                 E (1 + x d + ..): relative error 4 |x_i| u, and 2u granted on top for the second-order
                 terms (|x d| < 4e-13 on the table's range, its square far below u).
                                                                              (4 |x_i| + 2) u
      exp        vr_exp_tab is within MAX_ULP = 2 ulp of exp; an ulp is at most 2u relative.   4 u
      alpha      one multiplication.                                                          1 u
      sum        two additions at most (X has three lobes); each rounds a partial sum that is
                 no larger than sum |alpha_i| E_i, so u of that total per addition.            2 u
      Is         I * 360 is one rounding and colour * Is another.                              2 u

    Total, to first order:  |360 I| * sum_i |alpha_i| E_i (4 |x_i| + 11) u.  It is a sum over lobes of
    absolute terms, not a relative bound on the channel: X's third lobe is negative and cancels.

    Below the normal range a rounding is absolute, half of 2^-1074 at most, and exp_tab's 2 ulp are
    2 * 2^-1074.  Per lobe that is (2 |alpha_i| + 1) * 2^-1074 before the scale by |360 I| (the lobes
    this file counts as 0 are far inside it), and 4 * 2^-1074 after it for the last product and for
    Is itself when I is subnormal."""
    _, terms = lobes_exact(wl)
    with _ctx():
        scale = abs(Decimal(PDF_SCALE) * Decimal(float(intensity)))
        out = []
        for c in range(3):
            b = Decimal(0)
            for (term, x), lobe in zip(terms[c], [l for l in LOBES if l[0] == c]):
                if term != 0:  # E_i = 0 (x_i below -1000 or infinite): the absolute term alone
                    b += abs(term) * (4 * abs(x) + 11) * U
                b += (2 * abs(Decimal(lobe[1])) + 1) * TINY
            out.append(b * scale + 4 * TINY)
        return tuple(out)


# ------------------------------------------------------------------------------------------------
# The Kahan chain and the film merge: exact IEEE replays
# ------------------------------------------------------------------------------------------------
def kahan_replay(colours, state=None):
    """update_pixel (accumulation_buffer.rs:44-60) with weight 1.0, sample by sample, in numpy f64.

    colours: [spp, n, 3].  state: None for fresh records, or (sums [n, 3], compensations [n, 3],
    weight [n], weight compensation [n]) to continue from.  Returns the same four arrays.  Only +, -
    and * on doubles, no contraction: exact IEEE, compared with the device bit for bit."""
    colours = np.asarray(colours, dtype=np.float64)
    n = colours.shape[1]
    if state is None:
        s, b, w, wb = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    else:
        s, b, w, wb = (np.array(a, dtype=np.float64) for a in state)
    with np.errstate(all="ignore"):
        for c in colours:
            wy = 1.0 - wb
            wt = w + wy
            wb = (wt - w) - wy
            w = wt
            y = c * 1.0 - b
            t = s + y
            b = (t - s) - y
            s = t
    return s, b, w, wb


def merge_replay(film_xyzw, tile_records, tile, film_width):
    """film_merge_kernel's documented operation order (AccumulationBuffer::merge_tile,
    accumulation_buffer.rs:62-91, as vr_merge_tile) in numpy f64.

    film_xyzw: [pixels, 4] {colour X, Y, Z, weight}, row-major over a film `film_width` wide;
    tile_records: the tile's flat records (8 f64 per pixel; the compensations half is not read);
    tile: start_column / end_column / start_row / end_row.  Returns the merged film as a new array.
    Source colour = sum * (1 / w2), 0 where w2 == 0; colour = (c1 * w1 + c2 * w2) * (1 / (w1 + w2));
    weight = w1 + w2.  Exact IEEE operations: compared bit for bit, NaN positions included."""
    film = np.array(film_xyzw, dtype=np.float64).reshape(-1, 4)
    tw, th = tile.end_column - tile.start_column, tile.end_row - tile.start_row
    rec = np.asarray(tile_records, dtype=np.float64).reshape(-1)[:4 * tw * th].reshape(th * tw, 4)
    rows, cols = np.divmod(np.arange(tw * th), tw)
    d = (tile.start_row + rows) * film_width + (tile.start_column + cols)
    with np.errstate(all="ignore"):
        w1, w2 = film[d, 3], rec[:, 3]
        inv2 = 1.0 / w2
        c2 = np.where((w2 != 0.0)[:, None], rec[:, 0:3] * inv2[:, None], 0.0)
        inv = 1.0 / (w1 + w2)
        film[d, 0:3] = (film[d, 0:3] * w1[:, None] + c2 * w2[:, None]) * inv[:, None]
        film[d, 3] = w1 + w2
    return film


def records_colour(records):
    """The colour the display reads from flat records: sum * (1 / w), 0 where w == 0 (exact IEEE)."""
    r = np.asarray(records, dtype=np.float64).reshape(-1)
    n = r.size // 8
    r = r[:4 * n].reshape(n, 4)
    with np.errstate(all="ignore"):
        return np.where((r[:, 3] != 0.0)[:, None], r[:, 0:3] * (1.0 / r[:, 3])[:, None], 0.0)


# ------------------------------------------------------------------------------------------------
# The tone map
# ------------------------------------------------------------------------------------------------
TO_RGB = ((3.24096994, -1.53738318, -0.49861076), (-0.96924364, 1.87596750, 0.04155506),
          (0.05563008, -0.20397696, 1.05697151))  # colour_xyz.rs:49-56
KNEE = 0.0031308
GAMMA_EXPONENT = 1.0 / 2.4  # the double the reference passes to powf
BAND = 8  # in units of 2^-53, relative to 255 v


def linear_rgb(xyz):
    """ColourXyz::to_linear_rgb as an f64 restatement: three dot products folded from -0.0 in the
    reference's order (mat3.rs:147-157, vec3.rs:76-82), no contraction."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for i, (a, b, c) in enumerate(TO_RGB):
            s = -0.0 + a * xyz[:, 0]
            s = s + b * xyz[:, 1]
            s = s + c * xyz[:, 2]
            out[:, i] = s
    return out


_GAMMA_CACHE = {}


def _gamma_byte(u):
    """(byte, ambiguous, exact 255 v or None) for one linear channel value."""
    u = float(u)
    if u != u:
        return 0, False, None  # NaN survives the clamp; the saturating cast gives 0
    if u in _GAMMA_CACHE:
        return _GAMMA_CACHE[u]
    if u <= KNEE:
        # the linear branch: 12.98 * u, the clamp and * 255 are three exact IEEE operations (two
        # multiplications and comparisons), replayed here as they stand -- nothing to be ambiguous about
        v = 12.98 * u
        c = 0.0 if v < 0.0 else (1.0 if v > 1.0 else v)
        out = (int(c * 255.0), False, None)
    elif math.isinf(u):
        out = (255, False, None)
    else:
        # far from every integer the floor needs no 80 digits: the same expression in doubles is
        # within 2e-15 relative of the exact 255 v (pow 1 ulp, three roundings, the subtraction's
        # factor of 2.4 at most), and a point 1e-13 away is 100 times outside the band as well
        t64 = 255.0 * (1.005 * u ** GAMMA_EXPONENT - 0.055)
        if abs(t64 - round(t64)) > 1e-13 * t64:
            out = (255 if t64 >= 255.0 else int(t64), False, None)
            _GAMMA_CACHE[u] = out
            return out
        with _ctx():
            v = Decimal(1.005) * (Decimal(u) ** Decimal(GAMMA_EXPONENT)) - Decimal(0.055)
            t = 255 * v
            k = t.to_integral_value()  # the nearest integer
            near = 1 <= k <= 255 and abs(t - k) <= BAND * U * t
            byte = 255 if t >= 255 else int(t)  # v > 0.036 on this branch: no clamp below
            out = (byte, bool(near), t)
    _GAMMA_CACHE[u] = out
    return out


def tone_map_exact(xyz):
    """ClampingToneMapper over ColourXyz::to_srgb (image.rs:166-187, colour_xyz.rs:49-84).

    Returns (bytes [n, 3] uint8, ambiguous [n, 3] bool).  The 3x3 transform is `linear_rgb`, exact
    IEEE.  Then per channel the gamma with the reference's constants as written there (12.98 / 1.005 /
    0.055, the knee at u <= 0.0031308, the exponent the double 1.0 / 2.4): above the knee v = 1.005 *
    u^e - 0.055 at 80 digits from the binary values of the constants, the exact 255 * clamp(v), and its
    floor.

    `ambiguous` marks the channels where the exact 255 v lies within 8 * 2^-53 * 255 v of an integer
    1..255, so that a correct f64 evaluation may land on either side.  The band is derived, not
    measured: after pow come three roundings (* 1.005, - 0.055, * 255), 2^-53 relative each, and pow
    itself may be off by 2 ulp (the device's documented accuracy; glibc's is under 1); that total is
    doubled.  (The subtraction magnifies what came before it by (v + 0.055) / v, which is 1.06 at
    v = 1 and 2.4 at the knee; the doubling is what covers it for a pow that is within 1 ulp.)
    Never ambiguous: the linear branch (exact operations, replayed), values clamped at 0 or beyond the
    band above 255, NaN (byte 0) and the infinities (0 and 255)."""
    lin = linear_rgb(xyz)
    out = np.zeros(lin.shape, dtype=np.uint8)
    amb = np.zeros(lin.shape, dtype=bool)
    for i in range(lin.shape[0]):
        for c in range(3):
            out[i, c], amb[i, c], _ = _gamma_byte(lin[i, c])
    return out, amb


# ------------------------------------------------------------------------------------------------
# The shared input sets
# ------------------------------------------------------------------------------------------------
def colour_wavelengths():
    """0; 380..740 in steps of 7.5 with 0.4 either side of every lobe's mu; each mu and the doubles
    next to it; wavelengths whose lobes underflow: 100, 1000, 2000, 1e4, -500, and 1812.6, where Z is
    one subnormal lobe (x = -730) and nothing else."""
    w = [0.0] + [380.0 + 7.5 * i for i in range(49)]
    for mu in LOBE_MUS:
        w += [mu - 0.4, float(np.nextafter(mu, -np.inf)), mu, float(np.nextafter(mu, np.inf)), mu + 0.4]
    return w + [100.0, 1000.0, 2000.0, 1e4, -500.0, 1812.6]


def colour_intensities():
    """1, 2^-30, 2^30, a negative one, -0.0 and a subnormal."""
    return [1.0, 2.0 ** -30, 2.0 ** 30, -1.5, -0.0, 3 * 2.0 ** -1074]


OUT_OF_DOMAIN_WAVELENGTHS = (1e36, -1e36, 1e40, -1e40, 1e150, 1e160, math.inf, -math.inf)

THRESHOLD_OFFSETS = tuple([0] + [s * 2 ** j for j in range(21) for s in (1, -1)])  # ulps of the channel value


def byte_thresholds():
    """[(k, u)]: the channel values u (doubles nearest the exact ones) at which 255 v(u) reaches the
    integer k.  k = 1..10 on the linear branch (12.98 u = k / 255) and k = 10..255 above the knee: the
    curve drops from 0.0406 to 0.0360 across the knee, so byte 10 is reached twice."""
    out = []
    with _ctx():
        for k in range(1, 11):
            out.append((k, float(Decimal(k) / 255 / Decimal(12.98))))
        for k in range(10, 256):
            w = (Decimal(k) / 255 + Decimal(0.055)) / Decimal(1.005)
            out.append((k, float((w.ln() / Decimal(GAMMA_EXPONENT)).exp())))
    assert all(u <= KNEE for _, u in out[:10]) and all(u > KNEE for _, u in out[10:])
    return out


def _axis_input(channel, target):
    """The XYZ axis value q for which `channel` of linear_rgb((.., q, ..)) is the double nearest
    `target`: with the other two components +0 the dot product is fl(m * q) exactly (adding the
    products -0.0 and +-0 changes nothing).  Not every double is a rounded product, so the value
    reached may be an ulp off; callers work with the value reached."""
    m = TO_RGB[channel][channel]
    q0 = target / m
    best = None
    for j in range(-3, 4):
        q = q0
        for _ in range(abs(j)):
            q = float(np.nextafter(q, np.inf if j > 0 else -np.inf))
        err = abs(m * q - target)
        if best is None or err < best[0]:
            best = (err, q)
    return best[1]


def axis_xyz(channel, target):
    xyz = [0.0, 0.0, 0.0]
    xyz[channel] = _axis_input(channel, target)
    return xyz


_THRESHOLD_SET = {}


def threshold_points():
    """The tone map's threshold inputs: for every byte threshold, every offset of THRESHOLD_OFFSETS and
    each of R, G, B in turn, an XYZ on that channel's own axis whose channel value is the threshold
    moved by that many ulps (or the rounded product nearest to it).  The other two channels are then
    fixed multiples of it, negative or far smaller, away from their own thresholds
    (test_display_reference.py asserts that none of them is ambiguous).

    Returns (xyz [n, 3], channel [n], k [n], threshold value [n])."""
    if not _THRESHOLD_SET:
        xyz, ch, ks, us = [], [], [], []
        for k, u in byte_thresholds():
            for off in THRESHOLD_OFFSETS:
                for c in range(3):
                    xyz.append(axis_xyz(c, step(u, off)))
                    ch.append(c)
                    ks.append(k)
                    us.append(u)
        _THRESHOLD_SET["v"] = (np.array(xyz), np.array(ch), np.array(ks), np.array(us))
    return _THRESHOLD_SET["v"]


def ulps_between(a, b):
    """Distance in ulps between positive finite doubles (arrays)."""
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return np.abs(a - b)


def edge_points():
    """Further tone-map inputs [n, 3]: on each channel's axis the knee and the doubles beside it, 0,
    -0.0, a subnormal, 1, the doubles beside 1, 2, negative values, and +-inf and NaN in each channel;
    then a few off-axis colours (mid-grey, a saturated one, mixed infinities)."""
    vals = [KNEE, step(KNEE, -1), step(KNEE, 1), 0.0, 3 * 2.0 ** -1074, 1.0, step(1.0, -1), step(1.0, 1), 2.0]
    pts = []
    for c in range(3):
        pts += [axis_xyz(c, v) for v in vals]
        for special in (-0.0, -0.25, -3.0, -1e300, math.inf, -math.inf, math.nan):
            p = [0.0, 0.0, 0.0]
            p[c] = special
            pts.append(p)
            p = [0.2, 0.21, 0.23]
            p[c] = special
            pts.append(p)
    pts += [[0.2, 0.21, 0.23], [0.9505, 1.0, 1.089], [0.01, 0.9, 0.02], [math.inf, math.inf, -math.inf],
            [1e308, 1e308, 1e308], [-0.0, -0.0, -0.0], [2.0 ** -1074, 0.0, 0.0]]
    return np.array(pts, dtype=np.float64)


def merge_cases(film_width=23, film_height=11):
    """The film merge's synthetic cases over one film: [(Tile, flat numpy records)] in merge order.
    Tiles: the whole film, one pixel, a 1-wide column at an odd column, a tile ending at the last row
    and column, then the whole film twice more, so that the film's own weight varies.  The records hold
    weights 0 (with zero and with non-zero sums), 1, 3, 2^53, 2^-1074 and a negative one, sums that are
    -0.0, NaN and infinite, and the last merge cancels the film's weight on a band of pixels, so that
    w1 + w2 == 0 there."""
    W, H = film_width, film_height
    rng = np.random.RandomState(0x5EED)
    special_w = [0.0, 0.0, 1.0, 3.0, 2.0 ** 53, 2.0 ** -1074, -2.0, 1.0, 1.0, 1.0]
    special_s = [(0.0, 0.0, 0.0), (0.3, 0.2, 0.1), (0.25, 0.5, 0.125), (1.5, 0.75, 2.25), (2.0 ** 52, 3.0, 1e10),
                 (2.0 ** -1074, 0.0, 2.0 ** -1060), (0.5, -0.25, 1.0), (-0.0, 0.5, -0.0), (math.nan, 0.5, 0.25),
                 (math.inf, 0.5, -math.inf)]

    def records(n, salt):
        sums = np.empty((n, 4))
        sums[:, 0:3] = rng.uniform(0.0, 4.0, (n, 3))
        sums[:, 3] = rng.randint(1, 6, n).astype(np.float64)
        for i in range(n):  # the special records, spread so that every tile shape meets some
            j = (i + salt) % 13
            if j < len(special_w):
                sums[i, 3] = special_w[j]
                sums[i, 0:3] = special_s[j]
        rec = np.empty(8 * n)
        rec[:4 * n] = sums.reshape(-1)
        rec[4 * n:] = rng.uniform(-1e-17, 1e-17, 4 * n)  # compensations: present, never read by a merge
        return rec

    tiles = [Tile(0, W, 0, H), Tile(5, 6, 3, 4), Tile(7, 8, 0, H), Tile(W - 9, W, H - 4, H), Tile(0, W, 0, H),
             Tile(0, W, 0, H)]
    out = [(t, records(t.width() * t.height(), salt)) for salt, t in enumerate(tiles)]
    # the closing merge: on the pixels 40..79 its weight is minus the weight the film has by then
    # (replayed here), so that w1 + w2 == 0 there and 1 / (w1 + w2) is infinite
    film = np.zeros((W * H, 4))
    for t, rec in out[:-1]:
        film = merge_replay(film, rec, t, W)
    last = out[-1][1]
    for p in range(40, 80):
        w1 = film[p, 3]
        if w1 == w1 and w1 != 0.0 and not math.isinf(w1):
            last[4 * p + 3] = -w1
    return out


def weight_records(n=357):
    """Records for the tone map's records mode: (flat records, sums [n, 3], weights [n]) over weights
    0, -0.0, 2^-1074 (1 / w is inf), 1, 3, negative, NaN, inf and 2^53, each with zero, ordinary,
    negative, infinite and NaN sums; the compensations are non-zero and must not be read."""
    nan, inf, tiny = math.nan, math.inf, 2.0 ** -1074
    sums = [(0.2, 0.21, 0.23), (0.0, 0.0, 0.0), (0.5, 0.4, 0.3), (-0.2, 0.9, 0.1), (inf, 1.0, 1.0), (nan, 0.3, 0.3)]
    weights = [0.0, -0.0, tiny, 1.0, 3.0, -2.0, nan, inf, 2.0 ** 53]
    rows = [(s, w) for w in weights for s in sums]
    rows = (rows * (n // len(rows) + 1))[:n]
    s = np.array([r[0] for r in rows])
    w = np.array([r[1] for r in rows])
    rec = np.empty(8 * n)
    rec[:4 * n].reshape(n, 4)[:, 0:3] = s
    rec[:4 * n].reshape(n, 4)[:, 3] = w
    rec[4 * n:].reshape(n, 4)[:, 0:3] = 0.125
    rec[4 * n:].reshape(n, 4)[:, 3] = -0.5
    return rec, s, w


def photon_pool(n, seed):
    """n lit photons [n, 2] for the chain tests: visible wavelengths, intensities over 12 binades with
    both signs (so the Kahan compensations are busy), never {+0, +0}."""
    rng = np.random.RandomState(seed)
    wl = 380.0 + 360.0 * rng.random_sample(n)
    inten = rng.random_sample(n) * 2.0 ** rng.randint(-6, 6, n) * np.where(rng.random_sample(n) < 0.25, -1.0, 1.0)
    inten[inten == 0.0] = 0.5
    return np.stack([wl, inten], axis=1)
