"""Every material and Whitted branch on the device, on "goniometer" scenes: one surface of the material
under test in otherwise empty space, hit at chosen incidences by caller-supplied rays
(integrate_rays) or seen by a camera a few pixels wide.

  (a) WhittedIntegrator, closed form: the continuation ray leaves the only surface, so the photon
      is the sum of the light terms; compared with tests/material_reference.py in 50-digit
      arithmetic ("exact").  0, 1, 2 and VR_MAX_LIGHTS lights: a non-unit direction, one below the
      horizon, the dielectric's own reflection and refraction directions, one blocked by a small
      sphere (the ambient term).
  (b) SimpleRandomIntegrator, closed form under the sky, reflective and dielectric; the
      dielectric's arm statistics.
  (c) draw alignment: glass over a Lambertian floor against the oracle, every sampler arm present.
  (d) dispersion: eta from a 7-knot spectrum at every knot and one ulp beside it, closed form and
      camera path; and a wavelength at which only the reference's way of looking eta up is right.
  (e) material parameters on a sphere and on a bumpy mesh against the oracle, both integrators.
  (f) the 0 nm chain at the recursion limit with a colour that is not dark at 0 nm, and glass.
  (g) the general kernel against the kernels instantiated for one material kind.

Bounds of (a), (b) and (d): 4 x the reference's own f64 error against the exact run over the same
rays, never below 16 ulp (2^-49 = 1.78e-15); each test prints its figures (run with -s).  Measured,
the reference's f64 maximum / the bound / the device's maximum, on the plane with 16 lights:
Lambertian 1.95e-16 / 1.78e-15 / 1.19e-16; reflective (0.05, 0.9) 1.80e-14 / 7.18e-14 / 1.80e-14;
Phong 40 3.27e-15 / 1.31e-14 / 3.10e-15; Phong 1000 1.36e-14 / 5.43e-14 / 1.36e-14; glass 1.5
2.22e-16 / 1.78e-15 / 2.22e-16; glass 0.75 9.45e-16 / 3.78e-15 / 9.45e-16.
(c), (e), (f): flags, bounces and wavelengths equal the oracle's, intensities within
INTENSITY_REL_TOL = 1e-12 (tests/test_gpu_ties.py), and integrate_rays equals the megakernel bit for
bit.

Seeds of (e).  With smoothness 1000 a photon can consist of x^1000 lobes, which multiply the last-bit
differences of x = |w_o . r| by 1000, and w_o comes from the sampler's cos and sin, which the
device's libm and glibc may round differently.  Measured on the reference side alone
(tests/libm_sensitivity.py: a test-only copy of the oracle whose cos and sin are moved by one ulp):
at seed 7 two of the 1024 photons of [phong-1000-simple] move by 4.6e-12 and 1.1e-12, past the bar of
1e-12 (the two on which both kernels then differ from the oracle, by up to 2.55e-12), and one photon
of [phong-1-simple] by 2.0e-12.  Such a photon is not a function of the mathematics at the bar, so
each case of (e) takes the first seed from 7 on at which no photon moves past the bar and no decision
changes (settled_seed: 10 for phong-1000-simple, 8 for phong-1-simple, 7 for the others); the bar
stays 1e-12 on every sample.

What the reference does and this file therefore expects: a ray that runs inside an infinite plane
"hits" it (plane.rs divides by 0 and tests t < 0), so a light exactly in a plane is shadowed by the
plane itself; and under total internal reflection the path goes straight on (see
tests/test_oracle_materials.py), so a slab cannot hold a path: (f) stacks 130 panes instead.
"""

import numpy as np
import pytest

import material_reference as MR
from material_reference import EXACT, F64
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import Tile, integrate_rays, query_closest, render_samples
from vanrijn_amd.scene import (BoundingVolumeHierarchy, DirectionalLight, LambertianMaterial, Mesh, PhongMaterial,
                               Plane, ReflectiveMaterial, Scene, SmoothTransparentDialectric, Spectrum, Sphere,
                               WhittedIntegrator)

from libm_sensitivity import photon_moves
from test_gpu_integrate import Case, _oracle_rays
from test_gpu_ties import INTENSITY_REL_TOL
from material_grid import DEG, ETAS, ULP16, W_IN, direction, rel

pytestmark = pytest.mark.gpu

WAVELENGTHS = (431.7, 523.25, 655.0)
COLOUR = MR.Spectrum(400.0, 700.0, [0.5, 1.0, 0.75, 0.25])
COLOUR0 = MR.Spectrum(0.0, 800.0, [0.6, 0.9, 0.3, 0.8, 0.5])  # not dark at 0 nm
AMBIENT = MR.Spectrum(380.0, 740.0, [0.05, 0.08, 0.03])
LIGHT_SPECTRA = [MR.Spectrum(380.0, 740.0, s) for s in ([1.0, 0.8, 0.6, 0.9], [0.3, 0.5, 0.9], [0.7, 0.7],
                                                        [0.2, 1.1, 0.4, 0.6, 0.8])]


def twin(sp):
    """The project's Spectrum of a material_reference one."""
    return Spectrum(sp.shortest, sp.longest, np.array(sp.samples))


def project_material(m):
    if isinstance(m, MR.Lambertian):
        return LambertianMaterial(twin(m.colour), m.diffuse)
    if isinstance(m, MR.Reflective):
        return ReflectiveMaterial(twin(m.colour), m.diffuse, m.reflection)
    if isinstance(m, MR.Phong):
        return PhongMaterial(twin(m.colour), m.diffuse, m.specular, m.smoothness)
    return SmoothTransparentDialectric(twin(m.eta))


MATERIALS = {
    "lambertian": MR.Lambertian(COLOUR, 0.4),
    "reflective": MR.Reflective(COLOUR, 0.05, 0.9),
    "reflective-r0": MR.Reflective(COLOUR, 1.0, 0.0),
    "reflective-r1": MR.Reflective(COLOUR, 1.0, 1.0),
    "reflective-d0": MR.Reflective(COLOUR, 0.0, 1.0),
    "phong-40": MR.Phong(COLOUR, 0.1, 0.3, 40.0),
    "phong-0": MR.Phong(COLOUR, 1.0, 1.0, 0.0),
    "phong-1": MR.Phong(COLOUR, 1.0, 1.0, 1.0),
    "phong-1000": MR.Phong(COLOUR, 1.0, 1.0, 1000.0),
    "phong-s0": MR.Phong(COLOUR, 1.0, 0.0, 40.0),
}
MATERIALS.update({f"glass-{eta!r}": MR.Dielectric(MR.Spectrum.grey(eta)) for eta in ETAS})


# ----------------------------------------------------------------------------------- the goniometer
def flat_mesh(material):
    """Two triangles in a plane through the origin in general position (an axis-aligned one meets the
    triangle test's signed-zero cases, which are not this file's subject), with vertex normals equal
    to the face normal; the origin, where every ray lands, is inside the first triangle."""
    n = np.array([0.36, -0.48, 0.8])
    u = np.cross(n, [0.0, 0.0, 1.0])
    u /= np.sqrt(u @ u)
    v = np.cross(n, u)
    q = [a * u + c * v for a, c in ((-40.0, -50.0), (60.0, -50.0), (60.0, 50.0), (-40.0, 50.0))]
    tri = np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]])
    return BoundingVolumeHierarchy.build(Mesh(tri, np.tile(n, (2, 3, 1)), material))


def surface_objects(surface, material, blocker=None):
    if surface == "plane":
        objs = [[Plane((0.0, 0.0, 1.0), 0.0, material)]]
    elif surface == "mesh":
        objs = [flat_mesh(material)]
    else:  # "mesh-z0": the same two triangles in z = 0, where a direction can lie in the surface exactly
        q = np.array([[-40.0, -50.0, 0.0], [60.0, -50.0, 0.0], [60.0, 50.0, 0.0], [-40.0, 50.0, 0.0]])
        tri = np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]])
        objs = [BoundingVolumeHierarchy.build(Mesh(tri, np.tile([0.0, 0.0, 1.0], (2, 3, 1)), material))]
    if blocker is not None:
        objs.append([Sphere(tuple(3.0 * b for b in blocker), 0.02, LambertianMaterial(twin(COLOUR), 0.5))])
    return objs


class Bench:
    """The surface's shading basis (read from the device's own hit records and checked to be
    orthonormal) and the rays that meet the origin at every incidence of the grid.  On the plane
    the basis is the same bits for every ray and the incidences are the grid's exactly; on the mesh
    the interpolated normal moves in its last bits from ray to ray, so each ray's closed form takes
    its own record's basis."""

    def __init__(self, surface):
        self.surface = surface
        probe = Scene((0.0, 0.0, 5.0), surface_objects(surface, LambertianMaterial(twin(COLOUR), 0.5)))
        up = np.array([[0.3, -0.2, 2.0]]) if surface == "plane" else np.array([[0.8, -0.9, 1.7]])
        d = -up / np.linalg.norm(up)
        _, rec = query_closest(probe, up, d, records=True)
        assert rec["valid"].all()
        self.basis = np.array([rec[k][0] for k in ("tangent", "cotangent", "normal")])
        self.labels, o, d, wl = [], [], [], []
        for label, w in W_IN:
            if surface == "mesh-z0" and label.startswith("0/"):
                continue  # straight down an axis: the triangle test's signed zeros, not this file's subject
            retro = self.world(w)
            for lam in WAVELENGTHS:
                self.labels.append(f"{label} @{lam}")
                o.append(2.0 * retro)
                d.append(-retro)
                wl.append(lam)
        self.o, self.d, self.wl = np.array(o), np.array(d), np.array(wl)
        self.rows = self.check_hits(probe)
        if surface == "plane":
            assert abs(self.basis[2, 2]) == 1.0 and all(r == self.rows[0] for r in self.rows)

    def world(self, w):
        """A shading-space direction in world space (the basis is orthonormal: its transpose)."""
        return self.basis.T @ np.array(w, dtype=np.float64)

    def check_hits(self, scene):
        """Every ray hits the surface at the origin with an orthonormal basis; -> the bases."""
        _, rec = query_closest(scene, self.o, self.d, records=True)
        assert rec["valid"].all() and (rec["object"] == 0).all()
        assert np.array_equal(rec["retro"], -self.d) or self.surface != "plane"
        assert np.abs(rec["location"]).max() < 1e-6  # the blocker is 0.02 wide, 3 away
        bases = np.stack([rec["tangent"], rec["cotangent"], rec["normal"]], axis=1)
        gram = np.einsum("nij,nkj->nik", bases, bases)
        assert np.abs(gram - np.eye(3)).max() <= 1e-15, np.abs(gram - np.eye(3)).max()
        assert np.abs(bases - self.basis).max() <= 1e-15
        self.retro = [tuple(float(c) for c in r) for r in rec["retro"]]
        return [tuple(tuple(float(c) for c in row) for row in m) for m in bases]


@pytest.fixture(scope="module", params=["plane", "mesh"])
def bench(request):
    return Bench(request.param)


def held(name, got, f64, exact, labels):
    """got within 4 x the reference's own f64 error (at least 16 ulp) of the exact values."""
    ref = max(rel(f, x) for f, x in zip(f64, exact))
    bound = max(4.0 * ref, ULP16)
    errs = [rel(g, x) for g, x in zip(got, exact)]
    print(f"{name}: {len(errs)} photons, reference f64 max {ref:.3g}, bound {bound:.3g}, device max {max(errs):.3g}")
    bad = [(lb, float(g), float(x), e) for lb, g, x, e in zip(labels, got, exact, errs) if not e <= bound]
    assert not bad, (name, bound, len(bad), bad[:4])


# ------------------------------------------------------------------------ (a) Whitted, closed form
BLOCKED = 5


def light_list(b):
    """VR_MAX_LIGHTS lights in world space; [(direction, spectrum index)], light BLOCKED is the one
    behind the small sphere."""
    glass = MR.Dielectric(MR.Spectrum.grey(1.5))
    above, below = direction(45 * DEG, 0.0, 1), direction(10 * DEG, 0.0, -1)  # 45 from below is TIR: no tdir
    ra, ta = glass.fresnel(F64, above, WAVELENGTHS[1])[:2]
    rb, tb = glass.fresnel(F64, below, WAVELENGTHS[1])[:2]
    dirs = [0.7 * b.world((0.4, 0.3, 1.0)),               # not unit length
            b.world((0.3, -0.2, -0.9)),                 # below the horizon, not unit length
            b.world(ra), b.world(ta),                   # the glass's own directions, seen from above
            -b.world(above),                            # straight through
            b.world(direction(35 * DEG, 2.5, 1)),       # BLOCKED
            b.world(rb), b.world(tb), -b.world(below),  # the same three, seen from below
            b.world(direction(80 * DEG, 4.0, 1)), b.world(direction(5 * DEG, 1.0, 1)),
            0.25 * b.world(direction(60 * DEG, 5.5, 1)), b.world(direction(20 * DEG, 3.3, -1)),
            b.world(direction(89 * DEG, 0.3, 1)), b.world((0.0, 0.0, 1.0)), b.world(direction(50 * DEG, 2.0, 1))]
    assert len(dirs) == 16
    return [(tuple(float(c) for c in d), k % len(LIGHT_SPECTRA)) for k, d in enumerate(dirs)]


def whitted_scene(b, material, lights, blocker="auto"):
    """-> the scene and, per light, whether its shadow ray is stopped (by the small sphere)."""
    if blocker == "auto":
        blocker = lights[BLOCKED][0] if len(lights) == 16 else (lights[1][0] if len(lights) == 2 else None)
    s = Scene((0.0, 0.0, 5.0), surface_objects(b.surface, project_material(material), blocker))
    s.integrator = WhittedIntegrator(twin(AMBIENT), [DirectionalLight(d, twin(LIGHT_SPECTRA[k])) for d, k in lights])
    blocked = [blocker is not None and d == blocker for d, _ in lights]
    return s, blocked


def whitted_expected(K, b, material, lights, blocked):
    ls = [(d, LIGHT_SPECTRA[k]) for d, k in lights]
    return [MR.whitted_level(K, b.rows[i], b.retro[i], material, b.wl[i], AMBIENT, ls, blocked)
            for i in range(len(b.o))]


def run_whitted(b, name, lights, seed=11):
    material = MATERIALS[name]
    scene, blocked = whitted_scene(b, material, lights)
    assert b.check_hits(scene) == b.rows
    ph, info = integrate_rays(scene, b.o, b.d, seed, wavelengths=b.wl, info=True)
    assert (info["flags"] == 1).all() and np.array_equal(ph["wavelength"], b.wl)
    assert (info["bounces"] == 1).all()  # the continuation ray was traced and left the scene
    exact = whitted_expected(EXACT, b, material, lights, blocked)
    held(f"whitted {b.surface} {name} {len(lights)} lights", ph["intensity"], whitted_expected(F64, b, material, lights, blocked),
         exact, b.labels)
    return ph, exact, blocked


@pytest.mark.parametrize("name", list(MATERIALS))
def test_whitted_light_sum_all_lights(bench, name):
    lights = light_list(bench)
    ph, exact, blocked = run_whitted(bench, name, lights)
    assert sum(blocked) == 1
    if name == "glass-1.5":
        # the lights on the glass's own directions are the only ones a dielectric answers to
        m, ls = MATERIALS[name], [(d, LIGHT_SPECTRA[k]) for d, k in lights]
        lit = 0
        for i in range(len(bench.o)):
            for (d, sp) in ls:
                rows = tuple(MR.vec(EXACT, r) for r in bench.rows[i])
                w = MR.mat_vec(EXACT, rows, MR.vec(EXACT, d))
                retro = MR.mat_vec(EXACT, rows, MR.vec(EXACT, bench.retro[i]))
                lit += m.bsdf(EXACT, retro, w, bench.wl[i], 1.0)[1] != "0"
        assert lit >= 6, lit


@pytest.mark.parametrize("count", [0, 1, 2])
@pytest.mark.parametrize("name", ["phong-40", "glass-1.5", "reflective"])
def test_whitted_light_counts(bench, name, count):
    """No light: the photon is exactly 0.  One: the non-unit one.  Two: the glass's reflection
    direction and a blocked one (the ambient term alone answers for it)."""
    lights = light_list(bench)
    chosen = {0: [], 1: [lights[0]], 2: [lights[2], lights[BLOCKED]]}[count]
    ph, exact, blocked = run_whitted(bench, name, chosen)
    if count == 0:
        assert not ph["intensity"].any()
    if count == 2:
        assert blocked == [False, True]
        amb = [float(AMBIENT.intensity_at_wavelength(EXACT, w)) for w in bench.wl]
        assert all(float(x) >= a > 0 for x, a in zip(exact, amb))


def test_phong_cut_is_strict(bench):
    """A light exactly in the surface.  On the infinite plane its shadow ray runs inside the plane,
    which the reference's plane test counts as a hit (t = 0 / 0 or x / 0 is not < 0): the ambient
    term.  On the mesh it is free: Phong's cut is `w_i.z < 0`, so the lobe is evaluated and its
    `specular / w_i.z` is +inf in IEEE arithmetic, while the reflective cut (`<=`) gives 0 and
    leaves the other light's term."""
    b = bench if bench.surface == "plane" else Bench("mesh-z0")
    grazing = tuple(float(c) for c in b.world((0.6, 0.8, 0.0)))
    assert all(MR.dot(F64, rows[2], grazing) == 0.0 for rows in b.rows)
    other = light_list(b)[0]
    above = np.array([-b.d[i] @ b.basis[2] > 0 for i in range(len(b.o))])
    assert above.sum() > 20
    for name in ("phong-1", "reflective"):
        material = MATERIALS[name]
        scene, _ = whitted_scene(b, material, [(grazing, 0), other], blocker=None)
        ph = integrate_rays(scene, b.o, b.d, 11, wavelengths=b.wl)
        if b.surface == "plane":
            args = (b, material, [(grazing, 0), other], [True, False])
            held(f"{name} on the plane, in-plane light", ph["intensity"], whitted_expected(F64, *args),
                 whitted_expected(EXACT, *args), b.labels)
            continue
        args = (b, material, [other], [False])
        only = whitted_expected(EXACT, *args)
        if name == "phong-1":
            assert np.isposinf(ph["intensity"][above]).all(), ph["intensity"][above][:6]
            assert all(float(x) == 0.0 for x, a in zip(only, above) if not a)
            assert not ph["intensity"][~above].any()
        else:
            held("reflective on the mesh, in-plane light", ph["intensity"], whitted_expected(F64, *args), only, b.labels)


# ------------------------------------------------------------------- (b) SimpleRandom, closed form
def sky_scene(b, material):
    return Scene((0.0, 0.0, 5.0), surface_objects(b.surface, project_material(material)))


def sky_of(oracle, wl):
    return lambda world: oracle.sky_intensity([float(c) for c in world], wl)


@pytest.mark.parametrize("name", [n for n in MATERIALS if n.startswith("reflective")])
def test_reflective_under_the_sky(bench, oracle, name):
    b, m = bench, MATERIALS[name]
    ph, info = integrate_rays(sky_scene(b, m), b.o, b.d, 3, wavelengths=b.wl, info=True)
    assert (info["flags"] == 1).all() and (info["bounces"] == 1).all() and np.array_equal(ph["wavelength"], b.wl)
    res = {K: [MR.simple_random_level(K, b.rows[i], b.retro[i], m, b.wl[i], sky_of(oracle, b.wl[i]))[0]
               for i in range(len(b.o))] for K in (F64, EXACT)}
    held(f"sky {b.surface} {name}", ph["intensity"], res[F64], res[EXACT], b.labels)
    below = np.array([-b.d[i] @ b.basis[2] < 0 for i in range(len(b.o))])
    assert below.sum() > 20 and not ph["intensity"][below].any()  # the cut, exactly 0


def _arms(oracle, b, m, i, wl=None):
    """The exact run's photon of ray i (at its own wavelength, or at wl) for each side of the coin,
    with the arm's name; None where the f64 run takes another arm."""
    return _arms_of(oracle, b.rows[i], b.retro[i], m, b.wl[i] if wl is None else wl)


def _arms_of(oracle, rows, retro, m, wl):
    out = {}
    for coin in (True, False):
        f = MR.simple_random_level(F64, rows, retro, m, wl, sky_of(oracle, wl), lambda: coin)
        # the sky is looked up where the f64 direction points (the device's own input to it)
        sky = lambda world, v=sky_of(oracle, wl)(f[2]): v
        x = MR.simple_random_level(EXACT, rows, retro, m, wl, sky, lambda: coin)
        if f[1] != x[1]:
            return None
        out[x[1]] = (f[0], x[0])
    return out


@pytest.mark.parametrize("name", [n for n in MATERIALS if n.startswith("glass")])
def test_dielectric_under_the_sky(bench, oracle, name):
    """Each photon is the exact run's reflect-arm or transmit-arm value; the certain arms are taken by
    every ray that has them."""
    b, m = bench, MATERIALS[name]
    ph, info = integrate_rays(sky_scene(b, m), b.o, b.d, 3, wavelengths=b.wl, info=True)
    assert (info["flags"] == 1).all() and (info["bounces"] == 1).all()
    got, f64, exact, labels, seen, normal = [], [], [], [], {}, {}
    for i in range(len(b.o)):
        arms = _arms(oracle, b, m, i)
        if arms is None:
            continue
        g = ph["intensity"][i]
        arm = min(arms, key=lambda a: abs(float(arms[a][1]) - g))
        seen[arm] = seen.get(arm, 0) + 1
        if b.labels[i].startswith("0/"):
            normal[arm] = normal.get(arm, 0) + 1
        got.append(g), f64.append(arms[arm][0]), exact.append(arms[arm][1]), labels.append(b.labels[i] + " " + arm)
    print(name, seen)
    assert len(got) >= 0.98 * len(b.o)
    held(f"sky {b.surface} {name}", got, f64, exact, labels)
    if name == "glass-1.0":
        assert set(seen) == {"transmit-certain"}
    if name in ("glass-1.0", "glass-1.000000000001"):  # normal incidence with R <= 1e-10: through, no coin
        assert normal == {"transmit-certain": 2 * len(WAVELENGTHS)}, normal
    if name == "glass-1.5":
        assert seen.get("reflect-certain", 0) >= 3 * 4  # 42, 45 ... degrees from inside: TIR
        k = b.labels.index("60/0.0/- @523.25")
        arms = _arms(oracle, b, m, k)
        assert set(arms) == {"reflect-certain"}
        # strength 1: sky * pdf 0.5 * |cos 60|
        w = b.world(MR.fresnel(F64, tuple(b.basis @ -b.d[k]), 1.5, 1.0)[0])
        want = oracle.sky_intensity(list(w), b.wl[k]) * 0.5 * abs(w @ b.basis[2])
        assert abs(ph["intensity"][k] - want) <= 4 * ULP16 * want


def test_dielectric_coin_is_fair(bench, oracle):
    """4096 rays of one incidence on consecutive streams: the transmit count of a fair coin within
    five standard deviations (2048 +- 160); at eta 1 and under TIR no coin is thrown."""
    b = bench
    for name, label, lo, hi in (("glass-1.5", "45/0.0/+ @523.25", 2048 - 160, 2048 + 160),
                                ("glass-1.0", "45/0.0/+ @523.25", 4096, 4096),
                                ("glass-1.5", "60/0.0/- @523.25", 0, 0)):
        m, i = MATERIALS[name], b.labels.index(label)
        arms = _arms(oracle, b, m, i)
        n = 4096
        ph = integrate_rays(sky_scene(b, m), np.repeat(b.o[i:i + 1], n, 0), np.repeat(b.d[i:i + 1], n, 0), 17,
                            wavelengths=np.full(n, b.wl[i]), first_stream=100)
        values = {a: float(x) for a, (_, x) in arms.items()}
        assert len(set(values.values())) == len(values)
        near = {a: np.abs(ph["intensity"] - v) <= 4 * ULP16 * abs(v) for a, v in values.items()}
        assert np.logical_or.reduce(list(near.values())).all()
        transmitted = sum(int(near[a].sum()) for a in near if "transmit" in a)
        print(name, label, "transmitted", transmitted)
        assert lo <= transmitted <= hi, (name, label, transmitted)


# ------------------------------------------------------------------------------- (d) dispersion
ETA = MR.Spectrum(380.0, 740.0, [1.7, 1.62, 1.55, 1.48, 1.41, 1.35, 1.3])


def knot_wavelengths():
    """Every knot of ETA and one ulp on either side of it, inside the spectrum's range (outside it
    eta is 0 and the reference divides by it)."""
    out = []
    for k in range(7):
        knot = 380.0 + 360.0 * k / 6.0
        out += [float(w) for w in (np.nextafter(knot, 0.0), knot, np.nextafter(knot, 1e9)) if 380.0 <= w <= 740.0]
    assert len(out) == 19
    return out


def test_dispersion(oracle):
    """Glass whose eta falls from 1.7 to 1.3 over 7 knots, at every knot and its neighbours: the
    photon under the sky is the exact run's for one of the two arms (the looked-up eta sets R, T and
    the refracted direction), and the refracted rays, rebuilt from the f64 reference's direction, hit
    a plane 3 units behind the glass with the oracle's records bit for bit."""
    b = Bench("plane")
    m = MR.Dielectric(ETA)
    wls = knot_wavelengths()
    idx = [b.labels.index(f"{inc} @{WAVELENGTHS[0]}") for inc in ("10/0.7/+", "45/0.0/+", "60/0.7/+", "10/0.0/-", "89/0.0/+")]
    rays = [(i, w) for i in idx for w in wls]
    o = np.array([b.o[i] for i, _ in rays])
    d = np.array([b.d[i] for i, _ in rays])
    lam = np.array([w for _, w in rays])
    ph, info = integrate_rays(sky_scene(b, m), o, d, 5, wavelengths=lam, info=True)
    assert (info["flags"] == 1).all() and (info["bounces"] == 1).all() and np.array_equal(ph["wavelength"], lam)
    got, f64, exact, labels, refracted, seen = [], [], [], [], [], set()
    for k, (i, w) in enumerate(rays):
        arms = _arms(oracle, b, m, i, w)
        assert arms is not None
        arm = min(arms, key=lambda a: abs(float(arms[a][1]) - ph["intensity"][k]))
        seen.add(arm)
        got.append(ph["intensity"][k]), f64.append(arms[arm][0]), exact.append(arms[arm][1])
        labels.append(f"{b.labels[i]} -> {w!r} {arm}")
        t = b.world(m.fresnel(F64, MR.mat_vec(F64, b.rows[i], b.retro[i]), w)[1])
        refracted.append(t / np.sqrt(t @ t))
    assert {"coin-transmit", "coin-reflect"} <= seen
    held("dispersion under the sky", got, f64, exact, labels)
    # the refracted rays onto a second plane
    behind = Scene((0.0, 0.0, 5.0), [[Plane((0.0, 0.0, 1.0), 0.0, project_material(m)),
                                      Plane((0.0, 0.0, 1.0), -3.0, LambertianMaterial(twin(COLOUR), 0.5))]])
    t = np.array(refracted)
    origins = 1e-7 * t
    hits, rec = query_closest(behind, origins, t, records=True)
    ref, _ = oracle.OracleScene(behind.spec()).trace(origins, t)
    assert sum(h.valid and h.primitive == 1 for h in ref) >= 0.7 * len(t)
    for k, h in enumerate(ref):
        assert bool(rec["valid"][k]) == bool(h.valid) and hits["valid"][k] == h.valid
        if h.valid:
            assert (rec["object"][k], rec["primitive"][k]) == (h.object, h.primitive)
            assert rec["distance"][k] == h.distance == hits["distance"][k]
            for f in ("location", "normal", "tangent", "cotangent", "retro"):
                assert np.array_equal(rec[f][k], np.array(getattr(h, f)[:])), (k, f)


ETA_OFFSET = MR.Spectrum(390.0, 710.0, ETA.samples)  # knots at 390 + 160 k / 3: not exact in f64


def lookup_by_one_multiplication(sp, wl):
    """The other way to look a spectrum up, which the kernels use for plain intensities and must not
    use for eta: the segment from (wl - shortest) * ((n - 1) / range), the knots from a table."""
    n, rng = len(sp.samples), sp.longest - sp.shortest
    knots = [j / (n - 1) * rng + sp.shortest for j in range(n)]
    i = min(max(int((wl - sp.shortest) * ((n - 1) / rng)), 0), n - 1)
    if i == n - 1:
        return sp.samples[i]
    ratio = (wl - knots[i]) / (knots[i + 1] - knots[i])
    return sp.samples[i] * (1.0 - ratio) + sp.samples[i + 1] * ratio


def test_eta_is_looked_up_as_the_reference_does(oracle):
    """One ulp below the knot at 656.67 nm of ETA_OFFSET the reference's lookup gives 1.3500000000000005
    and the one-multiplication lookup 1.35.  Seen from inside at the two incidences found below, the
    first is totally reflected (in f64, and in exact arithmetic from that f64 eta: R = 1, no draw) and the second
    is refracted with R = 0.9999999 and a coin.  Every ray must be the exact run's reflect-certain
    photon; the other lookup is off by 1e-7 on half the rays and by everything on the others."""
    wl = float(np.nextafter(390.0 + 320.0 * 5.0 / 6.0, 0.0))
    eta = ETA_OFFSET.intensity_at_wavelength(F64, wl)
    other = lookup_by_one_multiplication(ETA_OFFSET, wl)
    assert eta != other and abs(eta - other) < 1e-15
    assert oracle.spectrum_intensity(390.0, 710.0, ETA_OFFSET.samples, wl) == eta
    found, c = [], float(np.sqrt(1.0 - 1.0 / (eta * eta)))
    for _ in range(64):
        c = float(np.nextafter(c, 0.0))
    for _ in range(128):
        c = float(np.nextafter(c, 1.0))
        w_i = (float(np.sqrt(1.0 - c * c)), 0.0, -c)
        if (MR.fresnel(F64, w_i, eta, 1.0)[4], MR.fresnel(EXACT, w_i, eta, 1.0)[4],
                MR.fresnel(F64, w_i, other, 1.0)[4]) == ("tir", "tir", "refract"):
            found.append(w_i)
    assert len(found) >= 2
    b, m, per = Bench("plane"), MR.Dielectric(ETA_OFFSET), 64
    retro = [b.world(w) for w in found for _ in range(per)]
    o, d = np.array([2.0 * r for r in retro]), np.array([-r for r in retro])
    ph, info = integrate_rays(sky_scene(b, m), o, d, 23, wavelengths=np.full(len(o), wl), first_stream=500, info=True)
    assert (info["flags"] == 1).all() and (info["bounces"] == 1).all()
    # the f64 run looks eta up as the reference does; the exact run takes that f64 value as given (a
    # lookup in exact arithmetic gives 1.35 and the other branch: the reference's own rounding of
    # eta is what steers this ray, and the kernels must reproduce it)
    given = MR.Dielectric(MR.Spectrum.grey(eta))
    got, f64, exact, labels = [], [], [], []
    for k, r in enumerate(retro):
        r = tuple(float(x) for x in r)
        f = MR.simple_random_level(F64, b.rows[0], r, m, wl, sky_of(oracle, wl))
        x = MR.simple_random_level(EXACT, b.rows[0], r, given, wl, lambda world, v=sky_of(oracle, wl)(f[2]): v)
        assert f[1] == x[1] == "reflect-certain"
        got.append(ph["intensity"][k]), f64.append(f[0]), exact.append(x[0])
        labels.append(f"incidence {k // per} stream {k % per}")
    held("eta one ulp below a knot, at the critical angle", got, f64, exact, labels)


# ------------------------------------------------------------- scenes seen by a camera, with the oracle
H = W = 16
TILE = Tile(0, W, 0, H)
SPP = 4


def first_hits(oracle, scene, seed):
    """The camera rays of the tile and the oracle's first hit of each: what the conditions on a scene
    are counted from."""
    o, d, ids, wl = _oracle_rays(oracle, scene.spec().camera_location, TILE, H, W, SPP, seed)
    hits, _ = oracle.OracleScene(scene.spec()).trace(o, d)
    return o, d, wl, hits


def settled_seed(scene, first=7, last=64):
    """The first seed on which every photon of the tile is a function of the mathematics at the bar:
    on the reference side alone (tests/libm_sensitivity.py), moving the Phong sampler's cos and sin by
    one ulp changes no decision and moves no intensity by more than INTENSITY_REL_TOL."""
    for seed in range(first, last):
        move, _ = photon_moves(scene.spec(), TILE, H, W, SPP, seed)
        if move.max() <= INTENSITY_REL_TOL:
            print(f"seed {seed}: largest move of a photon under one ulp of cos and sin {move.max():.3g}")
            return seed
    raise AssertionError("no seed on which the reference's photons hold still at the bar")


def camera_case(oracle, scene, seed=7):
    """The megakernel and integrate_rays (wavelengths drawn and given) against the oracle's records,
    every sample at INTENSITY_REL_TOL, and against each other bit for bit (Case.check)."""
    c = Case(oracle, scene, TILE, H, W, SPP, seed)
    g, r = c.mega["intensity"], c.ref["intensity"]
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where((g == r) | (np.isnan(g) & np.isnan(r)), 0.0, np.abs(g - r) / np.abs(r))
    print(f"megakernel against the oracle: largest relative intensity error {np.nanmax(err):.3g}")
    for given in (False, True):
        c.check(None, given)
    return c


# (c) ------------------------------------------------------------------------------ draw alignment
def alignment_scene(eta=None):
    """eta: the glass's spectrum (None: the constant 1.5)."""
    floor = LambertianMaterial(twin(COLOUR), 0.8)
    glass = SmoothTransparentDialectric(Spectrum.grey(1.5) if eta is None else twin(eta))
    return Scene((0.0, 0.0, 0.0), [[
        Plane((0.0, 1.0, 0.0), 1.0, glass),   # overhead, seen from inside
        Plane((0.0, 1.0, 0.0), -1.0, SmoothTransparentDialectric(Spectrum.grey(1.0))),  # eta 1: always through
        Plane((0.0, 1.0, 0.0), -2.0, floor),
        Plane((0.0, 1.0, 0.0), 2.5, floor),
        Sphere((0.0, -0.45, 2.2), 0.5, glass),  # from outside: the coin
    ]])


def sampler_arms(oracle, scene, seed):
    """The dielectric sampler's arm at each camera ray's first hit, from the oracle's exports."""
    o, d, wl, hits = first_hits(oracle, scene, seed)
    spec = scene.spec()
    arms = {}
    for i, h in enumerate(hits):
        if not h.valid or spec.materials[h.material].kind != N.MATERIAL_DIELECTRIC:
            continue
        m = spec.materials[h.material]
        w_i = oracle.mat3_mul_vec(np.array([h.tangent[:], h.cotangent[:], h.normal[:]]), h.retro[:])
        eta = oracle.spectrum_intensity(m.colour.shortest_wavelength, m.colour.longest_wavelength, m.colour.samples, wl[i])
        rdir, tdir, R, T = oracle.fresnel(w_i, *((1.0, eta) if w_i[2] >= 0 else (eta, 1.0)))
        _, _, draws = oracle.material_sample(3, m.colour.shortest_wavelength, m.colour.longest_wavelength,
                                             m.colour.samples, 0.0, 0.0, 0.0, w_i, wl[i], 1, 0)
        arm = "coin" if draws else ("reflect-certain" if T <= 1e-10 else "transmit-certain")
        arms[arm] = arms.get(arm, 0) + 1
    return arms


def test_draw_alignment(oracle):
    """A coin thrown where the reference throws none (or the reverse) shifts every later draw: the
    Lambertian bounces behind the glass then take other directions and the records differ."""
    scene = alignment_scene()
    arms = sampler_arms(oracle, scene, 7)
    print(arms)
    assert all(arms.get(a, 0) >= 50 for a in ("coin", "reflect-certain", "transmit-certain")), arms
    c = camera_case(oracle, scene)
    assert (c.ref["bounces"] >= 3).sum() >= 200  # paths go on behind the glass


def test_dispersion_on_the_camera_path(oracle):
    """(d) through the megakernel: the same scene with the dispersive glass (a pane seen from inside
    and a sphere, in front of Lambertian floors).  The looked-up eta steers every path behind the
    glass; records equal the oracle's and integrate_rays equals the megakernel bit for bit."""
    scene = alignment_scene(ETA)
    arms = sampler_arms(oracle, scene, 7)
    print(arms)
    assert arms.get("coin", 0) >= 50 and arms.get("reflect-certain", 0) >= 50, arms
    c = camera_case(oracle, scene)
    assert (c.ref["bounces"] >= 3).sum() >= 200


# (e) --------------------------------------------------------------- parameters, sphere and mesh
def bumpy_mesh(material, centre):
    """192 triangles whose vertex normals are the smooth ones tilted by up to ~60 degrees (hashed,
    the same at every corner that shares the vertex): the interpolated shading normal is far from
    the face's, and many rays see it from behind (w_i.z < 0 on a surface they face)."""
    v, n = scenes.displaced_mesh(4, [((0.3, 0.5, -0.8), 0.8, 0.35)], noise_seed=0xBEE5, noise_count=12, noise_amp=0.12,
                                 scale=(0.9, 0.9, 0.9), centre=centre)
    assert len(v) == 192
    key = np.round(v.reshape(-1, 3) * 4096.0).astype(np.int64) @ np.array([73856093, 19349663, 83492791])
    tilt = np.array([[2.0 * scenes._unit(int(k) & 0xFFFFFFFF, j) - 1.0 for j in range(3)] for k in key])
    n = scenes._normalize_rows(n.reshape(-1, 3) + 2.0 * tilt).reshape(v.shape)
    return BoundingVolumeHierarchy.build(Mesh(v, n, material))


PARAMETERS = {
    "phong-0": MR.Phong(COLOUR, 0.3, 0.4, 0.0), "phong-1": MR.Phong(COLOUR, 0.3, 0.4, 1.0),
    "phong-1000": MR.Phong(COLOUR, 0.3, 0.4, 1000.0), "phong-s0": MR.Phong(COLOUR, 0.3, 0.0, 40.0),
    "reflective-r0": MR.Reflective(COLOUR, 0.5, 0.0), "reflective-r1": MR.Reflective(COLOUR, 0.5, 1.0),
    "reflective-d0": MR.Reflective(COLOUR, 0.0, 0.9),
    "glass-0.75": MR.Dielectric(MR.Spectrum.grey(0.75)), "glass-1.0": MR.Dielectric(MR.Spectrum.grey(1.0)),
    "glass-2.4": MR.Dielectric(MR.Spectrum.grey(2.4)),
    "lambertian": MR.Lambertian(COLOUR, 0.4),
}


def parameter_scene(name, whitted, extra=()):
    m = project_material(PARAMETERS[name])
    s = Scene((0.0, 0.0, -3.0), [[Sphere((-0.95, 0.0, 0.0), 0.9, m)] + list(extra), bumpy_mesh(m, (0.95, 0.0, 0.0))])
    if whitted:
        s.integrator = WhittedIntegrator(twin(AMBIENT), [
            DirectionalLight((0.4, 1.0, -0.3), twin(LIGHT_SPECTRA[0])),
            DirectionalLight((-0.6, 0.8, -0.2), twin(LIGHT_SPECTRA[1]))])
    return s


def scene_conditions(oracle, scene, seed=7):
    """Counted from the oracle's hits alone: the material under test is hit by at least 200 samples,
    on the sphere and on the mesh; on the mesh at least 20 see the shading normal from behind."""
    o, d, wl, hits = first_hits(oracle, scene, seed)
    sphere = sum(1 for h in hits if h.valid and h.object == 0)
    mesh = [h for h in hits if h.valid and h.object == 1]
    behind = sum(1 for h in mesh if np.dot(h.normal[:], h.retro[:]) < 0)
    print(f"sphere {sphere}, mesh {len(mesh)}, behind the shading normal {behind}")
    assert sphere >= 200 and len(mesh) >= 200 and behind >= 20


@pytest.mark.parametrize("whitted", [False, True], ids=["simple", "whitted"])
@pytest.mark.parametrize("name", [n for n in PARAMETERS if n != "lambertian"])
def test_parameters_on_sphere_and_mesh(oracle, name, whitted):
    scene = parameter_scene(name, whitted)
    seed = settled_seed(scene)
    scene_conditions(oracle, scene, seed)
    camera_case(oracle, scene, seed)


# (f) ------------------------------------------------------------ the 0 nm chain at the recursion limit
def corridor(kind):
    """mirrors: two facing reflective planes whose colour is 0.6 at 0 nm (the lambda-0 chain is live).
    panes: 130 parallel glass panes (eta 1.5) above and 130 below, all turning their back to the
    camera, which sees them beyond the critical angle.  The reference's fresnel negates z of both
    directions when w_i.z < 0, so its total internal "reflection" is -w_i, straight on: a single
    slab cannot hold a path, but every pane is crossed by the TIR branch (R = 1, no draw) and the
    path runs into the recursion limit."""
    if kind in ("mirrors", "mirror-and-pane"):
        m = ReflectiveMaterial(twin(COLOUR0), 0.3, 0.9)
        planes = [Plane((0.0, 1.0, 0.0), -1.0, m), Plane((0.0, -1.0, 0.0), -1.0, m)]
        if kind == "mirror-and-pane":
            # a pane whose eta is 1 over the visible range and 1.5 at 0 nm: at lambda the path goes
            # through it, at 0 nm its strength for that direction is another number, and the photon at
            # the limit carries the lobes collected before the first crossing
            planes.append(Plane((0.0, 1.0, 0.0), 0.5, SmoothTransparentDialectric(
                Spectrum(0.0, 760.0, np.array([1.5, 1.0, 1.0])))))
        return Scene((0.0, 0.0, 0.0), [planes])
    m = SmoothTransparentDialectric(Spectrum.grey(1.5))
    return Scene((0.0, 0.0, 0.0), [[Plane((0.0, s, 0.0), 1.0 + 0.01 * k, m) for k in range(130) for s in (1.0, -1.0)]])


@pytest.mark.parametrize("kind", ["mirrors", "mirror-and-pane", "panes"])
def test_zero_wavelength_chain_at_the_limit(oracle, kind):
    scene = corridor(kind)
    c = Case(oracle, scene, Tile(0, 8, 0, 8), 8, 8, 2, 7)
    limit = ((c.ref["flags"] & 2) != 0) & (c.ref["bounces"] == 128) & (c.ref["wavelength"] == 0)
    print(kind, "samples at the limit:", int(limit.sum()), "NaN:", int(np.isnan(c.ref["intensity"]).sum()),
          "non-zero:", int((c.ref["intensity"] != 0).sum()))
    assert limit.sum() >= 100
    assert limit.all()
    finite = np.isfinite(c.ref["intensity"])
    if kind == "panes":  # glass alone has no lobe: the photon at the limit is 0 times the 0 nm throughput
        assert finite.all() and not c.ref["intensity"].any()
    else:
        # with the pane, the half of the tile that looks up meets the pane before any mirror: 0
        assert (finite & (c.ref["intensity"] > 0)).sum() >= (100 if kind == "mirrors" else 50)
    for given in (False, True):
        c.check(None, given)
    c.check(None, False, device=True)


# (g) ------------------------------------------------------------------------------ instantiations
@pytest.mark.parametrize("name", ["reflective-r1", "lambertian"])
def test_general_kernel_equals_the_specialised_one(oracle, name):
    """A scene of one material kind runs the kernel instantiated for that kind alone.  The same
    scene plus a Phong sphere far behind the camera, which no path touches (the oracle's records of
    the two scenes are the same bytes), runs the general kernel: its records are the same bits."""
    unseen = Sphere((0.0, 0.0, -30.0), 0.5, project_material(MATERIALS["phong-40"]))
    alone, general = parameter_scene(name, False), parameter_scene(name, False, extra=[unseen])
    kinds = [m.kind for m in general.spec().materials]
    assert N.MATERIAL_PHONG in kinds and N.MATERIAL_PHONG not in [m.kind for m in alone.spec().materials]
    want = [oracle.OracleScene(s.spec()).render_samples(TILE, H, W, SPP, 7) for s in (alone, general)]
    assert want[0].tobytes() == want[1].tobytes() and (want[0]["flags"] & 1).sum() >= 400
    got = [render_samples(s, TILE, H, W, SPP, 7) for s in (alone, general)]
    for f in ("wavelength", "intensity", "xyz"):
        assert got[0][f].tobytes() == got[1][f].tobytes(), f
    assert np.array_equal(got[0]["bounces"], got[1]["bounces"]) and np.array_equal(got[0]["flags"], got[1]["flags"])
    assert np.array_equal(got[0]["bounces"], want[0]["bounces"]) and got[0]["bounces"].max() >= 5
