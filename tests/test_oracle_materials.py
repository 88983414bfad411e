"""The oracle's materials (orc_fresnel, orc_material_bsdf, orc_material_sample: thin exports of the
statics its integrators call) against tests/material_reference.py, an independent restatement of the
reference's Rust text that runs in f64 and in 50-digit arithmetic ("exact").

Grid: incidence 0 exactly, 1e-8 rad, 10, 41, 42, 45, 56.3, 60, 89 degrees and 90 degrees - 1e-6 rad,
at two azimuths, on both sides of the surface (38 directions); eta 1, 1 + 1e-12, 1.3, 1.5, 2.4, 0.75;
Phong smoothness 0, 1, 40, 1000; strengths 0 and 1.

Branches (TIR or not, the sampler's arm and its number of draws, the Phong / reflective cut, which of
R, T, 0 the dielectric's bsdf returns) must equal the exact run's.  Points where the reference's own
f64 run takes another branch than the exact run would be left out;
test_grid_is_a_function_of_the_mathematics checks that these are at most 2 % and none of the exact
edges.  Measured: 0 of the 228 fresnel points, 0 of their sampler and bsdf decisions, 0 of the 8512
Phong and 2128 reflective cuts.

Values: relative error against the exact run (directions: largest component error of the unit
vector; where the exact value is 0, as R at eta 1, the absolute error).  The reference's own f64
error over the grid, and the oracle's bound 4 x that, never below 16 ulp = 2^-49 = 1.78e-15:

    family           reference f64 max   oracle's bound
    fresnel R, T     1.21e-04            4.83e-04   (eta 1 + 1e-12: cos(theta2) - cos(theta1) ~ 1e-12 is
    fresnel tdir     1.11e-11            4.42e-11    computed from numbers near 1; 1e-15 at the other etas)
    dielectric bsdf  1.21e-04            4.83e-04
    phong            1.57e-13            6.27e-13   (x^1000 multiplies the dot product's rounding by 1000)
    reflective       9.02e-14            3.61e-13   (1 - factor with factor near 1)
    lambertian       1.89e-16            1.78e-15
    spectrum         1.21e-16            1.78e-15

Because a family's maximum comes from its few ill-conditioned points, every point is also held to
4 x the reference's f64 error AT THAT POINT (same floor), the tighter bound everywhere else; the
oracle's measured maxima equal the reference's in every family.  A result whose exact value lies
below the smallest normal f64 (x^1000 underflows) must be below 2^-1021.  Values that are exactly 0
or 1 in the reference must be exactly that: TIR gives R = 1, T = 0, tdir = 0; cut directions give 0.

The reference's fresnel, restated as written: when w_i.z < 0 it negates z of BOTH directions at the
end, so seen from below the "reflected" direction is -w_i (straight on, to the other side) and the
refracted one stays below.  The oracle and the kernels do the same.
"""
import numpy as np
import pytest

import material_reference as MR
from material_grid import (ANGLES, BASES, COLOUR, DEG, ETAS, FIRST_DRAW, INTENSITY, SMOOTHNESS, STRENGTHS, ULP16,
                           W_IN, WAVELENGTH, direction, rel, vec_err)
from material_reference import EXACT, F64

class Family:
    """Errors of the reference's f64 run and of the oracle against the exact run, point by point."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def add(self, label, ref_err, orc_err):
        self.rows.append((label, ref_err, orc_err))

    def check(self):
        assert self.rows
        ref_max = max(r for _, r, _ in self.rows)
        bound = max(4.0 * ref_max, ULP16)
        print(f"{self.name}: {len(self.rows)} values, reference f64 max {ref_max:.3g}, bound {bound:.3g}, "
              f"oracle max {max(o for _, _, o in self.rows):.3g}")
        bad = [(lb, r, o) for lb, r, o in self.rows if o > bound or o > max(4.0 * r, ULP16)]
        assert not bad, (self.name, bound, bad[:5])
        return ref_max


# ------------------------------------------------------------------------------------ the fresnel grid
def eta_pair(w_i, eta):
    return (1.0, eta) if w_i[2] >= 0.0 else (eta, 1.0)


def fresnel_points():
    for label, w_i in W_IN:
        for eta in ETAS:
            yield f"{label} eta {eta!r}", w_i, eta


@pytest.fixture(scope="module")
def fresnel_grid():
    """[(label, w_i, eta, f64 result, exact result)] and the labels whose f64 branch differs."""
    rows, unstable = [], set()
    for label, w_i, eta in fresnel_points():
        e1, e2 = eta_pair(w_i, eta)
        f, x = MR.fresnel(F64, w_i, e1, e2), MR.fresnel(EXACT, w_i, e1, e2)
        if f[4] != x[4]:
            unstable.add(label)
        rows.append((label, w_i, eta, f, x))
    return rows, unstable


def test_grid_is_a_function_of_the_mathematics(fresnel_grid):
    """The reference alone: its f64 and exact runs take the same branch on all but 2 % of the grid,
    and on every exact edge."""
    rows, unstable = fresnel_grid
    decisions, differ = 0, set(unstable)
    for label, w_i, eta, f, x in rows:
        m = MR.Dielectric(MR.Spectrum.grey(eta))
        for coin in (True, False):
            decisions += 1
            if m.sample(F64, w_i, WAVELENGTH, lambda: coin)[2] != m.sample(EXACT, w_i, WAVELENGTH, lambda: coin)[2]:
                differ.add(label)
        for w_o in dielectric_outgoing(f):
            decisions += 1
            if m.bsdf(F64, w_o, w_i, WAVELENGTH, INTENSITY)[1] != m.bsdf(EXACT, w_o, w_i, WAVELENGTH, INTENSITY)[1]:
                differ.add(label)
    print(f"fresnel points {len(rows)}, f64/exact branch differs at {len(unstable)}; "
          f"with the sampler and bsdf decisions: {len(differ)} points {sorted(differ)}")
    assert len(differ) <= 0.02 * len(rows)
    edges = [lb for lb in differ if lb.startswith("0/") or lb.endswith("eta 1.0") or
             (lb.startswith("60/") and lb.endswith("- eta 1.5"))]
    assert not edges, edges
    for kind, points in (("phong", phong_points()), ("reflective", reflective_points())):
        total = bad = 0
        for label, m, w_o, w_i in points:
            total += 1
            bad += m.bsdf(F64, w_o, w_i, WAVELENGTH, INTENSITY)[1] != m.bsdf(EXACT, w_o, w_i, WAVELENGTH, INTENSITY)[1]
        print(f"{kind}: {total} points, f64/exact cut differs at {bad}")
        assert bad == 0


def test_fresnel(oracle, fresnel_grid):
    rows, unstable = fresnel_grid
    strengths, tdirs = Family("fresnel R, T"), Family("fresnel tdir")
    seen = set()
    for label, w_i, eta, f, x in rows:
        if label in unstable:
            continue
        e1, e2 = eta_pair(w_i, eta)
        rdir, tdir, R, T = oracle.fresnel(w_i, e1, e2)
        tir = x[4] == "tir"
        seen.add(x[4])
        assert tuple(rdir) == f[0], label  # negations only: exact in every arithmetic
        if tir:
            assert R == 1.0 and T == 0.0 and not tdir.any(), (label, R, T, tdir)
            continue
        assert tdir.any(), label
        strengths.add(label + " R", rel(f[2], x[2]), rel(R, x[2]))
        strengths.add(label + " T", rel(f[3], x[3]), rel(T, x[3]))
        tdirs.add(label, vec_err(f[1], x[1]), vec_err(tdir, x[1]))
    assert seen == {"tir", "refract"}
    strengths.check()
    tdirs.check()


def test_fresnel_exact_edges(oracle):
    """TIR at 60 degrees from inside eta 1.5; eta 1 and normal incidence: T = 1 - R with R tiny or 0."""
    w = direction(60 * DEG, 0.0, -1)
    rdir, tdir, R, T = oracle.fresnel(w, 1.5, 1.0)
    assert (R, T) == (1.0, 0.0) and not tdir.any() and tuple(rdir) == (-w[0], -w[1], -w[2])
    assert MR.fresnel(EXACT, w, 1.5, 1.0)[4] == "tir"
    for label, w_i in W_IN:
        rdir, tdir, R, T = oracle.fresnel(w_i, 1.0, 1.0)
        assert R <= MR.THRESHOLD and T == 1.0 - R, (label, R, T)  # the sampler's transmit-certain arm
    for eta in ETAS:
        for z in (1.0, -1.0):
            e1, e2 = eta_pair((0.0, 0.0, z), eta)
            rdir, tdir, R, T = oracle.fresnel((0.0, 0.0, z), e1, e2)
            # from below, the reference's final z flip gives the same pair as from above
            assert tuple(tdir) == (0.0, 0.0, -1.0) and tuple(rdir) == (0.0, 0.0, 1.0), (eta, z, tdir, rdir)
            want = ((e1 - e2) / (e1 + e2)) ** 2
            assert abs(R - want) <= 1e-15 * want, (eta, z, R, want)


def test_physics_of_the_restatement(fresnel_grid):
    """A guard on material_reference itself: R + T = 1, Snell's law, the normal-incidence R."""
    rows, _ = fresnel_grid
    for label, w_i, eta, f, x in rows:
        e1, e2 = eta_pair(w_i, eta)
        for K, res, tol in ((F64, f, 1e-14), (EXACT, x, 1e-14)):  # w_i is unit to an ulp only
            rdir, tdir, R, T, branch = res
            assert abs(R + T - 1) <= (1e-15 if K is F64 else 1e-45), label
            assert 0 <= R <= 1
            if branch == "tir":
                continue
            sin1 = K.sqrt(K.num(w_i[0]) ** 2 + K.num(w_i[1]) ** 2) / K.sqrt(MR.dot(K, MR.vec(K, w_i), MR.vec(K, w_i)))
            sin2 = K.sqrt(tdir[0] * tdir[0] + tdir[1] * tdir[1])
            assert abs(K.num(e1) * sin1 - K.num(e2) * sin2) <= tol, (label, K.name)
            # from above the transmitted ray goes below.  From below the reference's last step
            # (`coords[2] *= -1.0` on both directions when w_i.z < 0) sends it below as well, and
            # the reflected one above: restated as written, not as optics has it
            assert tdir[2] < 0 and (rdir[2] > 0 or w_i[2] == 0), label
            if w_i[0] == 0.0 and w_i[1] == 0.0:
                want = ((K.num(e1) - K.num(e2)) / (K.num(e1) + K.num(e2))) ** 2
                assert abs(R - want) <= 1e-15 * want, (label, K.name)


# --------------------------------------------------------------------------- the dielectric's sampler
def _glass(eta):
    return (3, 380.0, 740.0, [eta, eta], 0.0, 0.0, 0.0)


def test_dielectric_sampler_arms_and_draws(oracle, fresnel_grid):
    """Which arm, how many draws and which direction: the exact run's, the coin being the top bit of
    the stream's draw `FIRST_DRAW`."""
    rows, unstable = fresnel_grid
    arms = {}
    for label, w_i, eta, f, x in rows:
        m = MR.Dielectric(MR.Spectrum.grey(eta))
        e1, e2 = eta_pair(w_i, eta)
        looked_up = oracle.spectrum_intensity(380.0, 740.0, [eta, eta], WAVELENGTH)  # eta to an ulp
        rdir, tdir, _, _ = oracle.fresnel(w_i, *eta_pair(w_i, looked_up))
        for base in BASES:
            coin = oracle.stream_bool(base, FIRST_DRAW)
            a64 = m.sample(F64, w_i, WAVELENGTH, lambda: coin)
            want = m.sample(EXACT, w_i, WAVELENGTH, lambda: coin)
            if label in unstable or a64[2] != want[2]:
                continue
            w_o, pdf, draws = oracle.material_sample(*_glass(eta), w_i, WAVELENGTH, base, FIRST_DRAW)
            arm = want[2]
            arms[arm] = arms.get(arm, 0) + 1
            assert draws == want[3] and pdf == 0.5, (label, arm, draws)
            took_t = arm in ("transmit-certain", "coin-transmit")
            assert np.array_equal(w_o, tdir if took_t else rdir), (label, arm, w_o, rdir, tdir)
            if not np.array_equal(rdir, tdir):
                assert not np.array_equal(w_o, rdir if took_t else tdir), (label, arm)
    print("sampler arms:", arms)
    assert all(arms.get(a, 0) >= 20 for a in ("reflect-certain", "transmit-certain", "coin-transmit", "coin-reflect"))
    # the other materials: reflective draws nothing, Phong and Lambertian draw (at least) two
    w_i = direction(45 * DEG, 0.7, 1)
    w_o, pdf, draws = oracle.material_sample(1, 400.0, 700.0, COLOUR.samples, 0.5, 0.5, 0.0, w_i, WAVELENGTH, BASES[0], 3)
    assert (tuple(w_o), pdf, draws) == ((-w_i[0], -w_i[1], w_i[2]), 1.0, 0)
    assert oracle.material_sample(2, 400.0, 700.0, COLOUR.samples, 0.5, 0.5, 40.0, w_i, WAVELENGTH, BASES[0], 3)[2] == 2
    assert oracle.material_sample(0, 400.0, 700.0, COLOUR.samples, 0.5, 0.0, 0.0, w_i, WAVELENGTH, BASES[0], 3)[2] >= 2


# ------------------------------------------------------------------------------ the dielectric's bsdf
def dielectric_outgoing(f):
    """Outgoing directions for a fresnel result: its two directions, each moved by less and by more
    than the bsdf's 1e-5 radius, and one unrelated direction."""
    rdir, tdir = f[0], f[1]
    out = [rdir, tdir, (0.36, -0.48, 0.8)]
    for base in (rdir, tdir):
        for step in (0.7e-5, 1.4e-5):
            out.append((base[0] + step * 0.6, base[1] - step * 0.8, base[2]))
    return out


def test_dielectric_bsdf(oracle, fresnel_grid):
    rows, unstable = fresnel_grid
    fam, branches = Family("dielectric bsdf"), {}
    for label, w_i, eta, f, x in rows:
        if label in unstable:
            continue
        m = MR.Dielectric(MR.Spectrum.grey(eta))
        for k, w_o in enumerate(dielectric_outgoing(f)):
            v64, b64 = m.bsdf(F64, w_o, w_i, WAVELENGTH, INTENSITY)
            want, branch = m.bsdf(EXACT, w_o, w_i, WAVELENGTH, INTENSITY)
            if b64 != branch:
                continue
            got = oracle.material_bsdf(*_glass(eta), w_o, w_i, WAVELENGTH, INTENSITY)
            branches[branch] = branches.get(branch, 0) + 1
            if branch == "0":
                assert got == 0.0, (label, k, got)
            elif x[4] == "tir" and branch == "R":
                assert got == INTENSITY, (label, k, got)
            else:
                fam.add(f"{label} w_o {k}", rel(v64, want), rel(got, want))
    print("bsdf branches:", branches)
    assert all(branches.get(b, 0) >= 100 for b in ("R", "T", "0"))
    fam.check()


# ------------------------------------------------------------------------------- Phong and reflective
def outgoing():
    """w_o for the lobe materials: the grid's directions above the surface at another azimuth, one
    exactly in the surface (z = +0 and -0), one below."""
    for name, theta in ANGLES:
        yield name, direction(theta, 2.1, 1)
    yield "in-plane", (0.6, 0.8, 0.0)
    yield "in-plane-0", (0.6, 0.8, -0.0)
    yield "below", direction(30 * DEG, 2.1, -1)


def phong_points():
    for li, w_i in W_IN:
        for lo, w_o in list(outgoing()) + [("mirror", (-w_i[0], -w_i[1], w_i[2]))]:
            for smooth in SMOOTHNESS:
                for spec in STRENGTHS:
                    for diff in STRENGTHS:
                        yield f"{li} {lo} n {smooth} s {spec} d {diff}", MR.Phong(COLOUR, diff, spec, smooth), w_o, w_i


def reflective_points():
    for li, w_i in W_IN:
        for lo, w_o in list(outgoing()) + [("mirror", (-w_i[0], -w_i[1], w_i[2]))]:
            for refl in STRENGTHS:
                for diff in STRENGTHS:
                    yield f"{li} {lo} r {refl} d {diff}", MR.Reflective(COLOUR, diff, refl), w_o, w_i


def _args(m):
    c = m.colour
    return (m.kind, c.shortest, c.longest, c.samples, m.diffuse, getattr(m, "reflection", getattr(m, "specular", 0.0)),
            getattr(m, "smoothness", 0.0))


@pytest.mark.parametrize("kind", ["phong", "reflective"])
def test_lobe_bsdf(oracle, kind):
    fam, cuts, values = Family(kind), 0, 0
    for label, m, w_o, w_i in (phong_points() if kind == "phong" else reflective_points()):
        v64, _ = m.bsdf(F64, w_o, w_i, WAVELENGTH, INTENSITY)
        want, branch = m.bsdf(EXACT, w_o, w_i, WAVELENGTH, INTENSITY)
        got = oracle.material_bsdf(*_args(m), w_o, w_i, WAVELENGTH, INTENSITY)
        if branch == "cut":
            cuts += 1
            assert got == 0.0, (label, got)
            continue
        values += 1
        if want == 0:
            assert got == 0.0, (label, got)
        else:
            fam.add(label, rel(v64, want), rel(got, want))
    print(f"{kind}: {cuts} cut, {values} values")
    assert cuts >= 100 and values >= 100
    fam.check()


def test_the_cut_is_strict_for_phong_only(oracle):
    """w_o exactly in the surface: Phong (`<`) returns a value, reflective (`<=`) returns 0."""
    w_i, w_o = direction(45 * DEG, 0.0, 1), (0.6, 0.8, 0.0)
    phong, mirror = MR.Phong(COLOUR, 1.0, 1.0, 1.0), MR.Reflective(COLOUR, 1.0, 1.0)
    assert phong.bsdf(EXACT, w_o, w_i, WAVELENGTH, INTENSITY)[1] == "value"
    assert mirror.bsdf(EXACT, w_o, w_i, WAVELENGTH, INTENSITY)[1] == "cut"
    assert oracle.material_bsdf(*_args(phong), w_o, w_i, WAVELENGTH, INTENSITY) > 0.1
    assert oracle.material_bsdf(*_args(mirror), w_o, w_i, WAVELENGTH, INTENSITY) == 0.0


def test_lambertian_bsdf_and_spectrum(oracle):
    eta = MR.Spectrum(380.0, 740.0, [1.7, 1.62, 1.55, 1.48, 1.41, 1.35, 1.3])
    lam, spec = Family("lambertian"), Family("spectrum")
    for sp in (COLOUR, eta):
        n = len(sp.samples)
        knots = [sp.shortest + (sp.longest - sp.shortest) * k / (n - 1) for k in range(n)]
        wls = [w for k in knots for w in (np.nextafter(k, 0.0), k, np.nextafter(k, 1e9))] + [WAVELENGTH, 431.7, 0.0]
        for wl in wls:
            wl = float(wl)
            want = sp.intensity_at_wavelength(EXACT, wl)
            got = oracle.spectrum_intensity(sp.shortest, sp.longest, sp.samples, wl)
            if want == 0:
                assert got == 0.0 and not (sp.shortest <= wl <= sp.longest), wl
                continue
            spec.add(f"{wl!r}", rel(sp.intensity_at_wavelength(F64, wl), want), rel(got, want))
            for diff in STRENGTHS + [0.05]:
                m = MR.Lambertian(sp, diff)
                w = m.bsdf(EXACT, None, None, wl, INTENSITY)[0]
                g = oracle.material_bsdf(0, sp.shortest, sp.longest, sp.samples, diff, 0.0, 0.0, (0, 0, 1), (0, 0, 1), wl,
                                         INTENSITY)
                if w == 0:
                    assert g == 0.0
                else:
                    lam.add(f"{wl!r} d {diff}", rel(m.bsdf(F64, None, None, wl, INTENSITY)[0], w), rel(g, w))
    # at the range ends the value is the sample itself
    for k, wl in ((0, 380.0), (6, 740.0)):
        assert oracle.spectrum_intensity(380.0, 740.0, eta.samples, wl) == eta.samples[k]
    spec.check()
    lam.check()

