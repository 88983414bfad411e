"""An independent restatement of the reference's materials and of one level of its integrators.

Written from the reference's Rust text (materials/*.rs, colour/spectrum.rs, integrators/*.rs,
math/vec3.rs, math/mat3.rs), not from oracle/vr_oracle.c and not from the device code, so that the
oracle and the kernels can be pinned against something that shares no line with them.

Every function takes a number kind `K` first and is run in two ways:

  * `F64`   -- Python floats in the reference's operation order ("the reference in f64");
  * `EXACT` -- mpmath at 50 significant digits on the same f64 inputs ("exact").

Vectors are 3-tuples of K numbers.  Functions that branch also report which branch they took, so a
test can compare decisions and leave out the inputs on which f64 and exact arithmetic disagree.
"""
import math

import mpmath

THRESHOLD = 0.0000000001  # the dielectric's literal in sample and bsdf
PI_F64 = 3.14159265358979323846  # std::f64::consts::PI, an f64 constant in both runs


class F64:
    name = "f64"
    zero = -0.0  # `impl Sum for f64` folds from -0.0

    @staticmethod
    def num(x):
        return float(x)

    sqrt = staticmethod(math.sqrt)
    acos = staticmethod(math.acos)
    exp = staticmethod(math.exp)

    @staticmethod
    def pow(x, y):
        try:
            return math.pow(x, y)
        except OverflowError:
            return math.inf

    @staticmethod
    def trunc(x):
        return int(x)


_MP = mpmath.mp.clone()
_MP.dps = 50


class EXACT:
    name = "exact"
    zero = _MP.mpf(0)

    @staticmethod
    def num(x):
        return _MP.mpf(x)  # an f64 converts exactly

    sqrt = staticmethod(_MP.sqrt)
    acos = staticmethod(_MP.acos)
    exp = staticmethod(_MP.exp)

    @staticmethod
    def pow(x, y):
        return _MP.power(x, y)

    @staticmethod
    def trunc(x):
        return int(_MP.floor(x)) if x >= 0 else -int(_MP.floor(-x))


def vec(K, v):
    return tuple(K.num(c) for c in v)


# ----------------------------------------------------------------------------- math/vec3.rs, mat3.rs
def dot(K, a, b):
    s = K.zero
    for x, y in zip(a, b):
        s = s + x * y
    return s


def sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def normalize(K, a):
    inverse_norm = K.num(1.0) / K.sqrt(dot(K, a, a))
    return tuple(x * inverse_norm for x in a)


def mat_vec(K, rows, v):
    return tuple(dot(K, r, v) for r in rows)


def _minor(m, row, col):
    e = [[m[i][j] for j in range(3) if j != col] for i in range(3) if i != row]
    return e[0][0] * e[1][1] - e[1][0] * e[0][1]


def determinant(m):
    return m[0][0] * _minor(m, 0, 0) - m[0][1] * _minor(m, 0, 1) + m[0][2] * _minor(m, 0, 2)


def try_inverse(K, m):
    """Mat3::try_inverse as the reference has it: transpose(cofactors) TIMES the determinant (not
    divided by it), the true inverse only where the determinant is +-1."""
    det = determinant(m)
    if det == 0:
        return None
    cof = [[K.num((-1) ** (i + j)) * _minor(m, i, j) for j in range(3)] for i in range(3)]
    return tuple(tuple(cof[j][i] * det for j in range(3)) for i in range(3))


# ------------------------------------------------------------------------------- colour/spectrum.rs
class Spectrum:
    def __init__(self, shortest, longest, samples):
        self.shortest, self.longest, self.samples = float(shortest), float(longest), [float(s) for s in samples]

    @staticmethod
    def grey(v):
        return Spectrum(380.0, 740.0, [v, v])

    def intensity_at_wavelength(self, K, wavelength):
        wl, lo, hi = K.num(wavelength), K.num(self.shortest), K.num(self.longest)
        if wl < lo or wl > hi:
            return K.num(0.0)
        last = len(self.samples) - 1
        rng = hi - lo
        index = K.trunc(K.num(last) * ((wl - lo) / rng))

        def at(i):
            return K.num(i) / K.num(last) * rng + lo

        before = at(index)
        if index == last:
            return K.num(self.samples[index])
        delta = at(index + 1) - before
        ratio = (wl - before) / delta
        return K.num(self.samples[index]) * (K.num(1.0) - ratio) + K.num(self.samples[index + 1]) * ratio


# ------------------------------------------------------------------------------------ the materials
class Lambertian:
    kind = 0

    def __init__(self, colour, diffuse):
        self.colour, self.diffuse = colour, float(diffuse)

    def bsdf(self, K, w_o, w_i, wavelength, intensity):
        out = K.num(intensity) * self.colour.intensity_at_wavelength(K, wavelength)
        return out * K.num(self.diffuse), "value"


class Reflective:
    kind = 1

    def __init__(self, colour, diffuse, reflection):
        self.colour, self.diffuse, self.reflection = colour, float(diffuse), float(reflection)

    def bsdf(self, K, w_o, w_i, wavelength, intensity):
        w_o, w_i = vec(K, w_o), vec(K, w_i)
        if w_i[2] <= 0 or w_o[2] <= 0:
            return K.num(0.0), "cut"
        reflection_vector = (-w_o[0], -w_o[1], w_o[2])
        out = K.num(intensity) * self.colour.intensity_at_wavelength(K, wavelength)
        out = out * K.num(self.diffuse)
        sigma, two = K.num(0.05), K.num(2.0)
        c = dot(K, w_i, reflection_vector)
        c = K.num(0.0) if c < 0 else (K.num(1.0) if c > 1 else c)  # f64::clamp(0, 1)
        theta = K.acos(abs(c))
        factor = K.num(self.reflection) * K.exp(-(K.pow(theta, two)) / (two * sigma * sigma))
        return out * (K.num(1.0) - factor) + factor, "value"

    def sample(self, K, w_i, wavelength, coin=None):
        w = vec(K, w_i)
        return (-w[0], -w[1], w[2]), K.num(1.0), "mirror", 0


class Phong:
    kind = 2

    def __init__(self, colour, diffuse, specular, smoothness):
        self.colour, self.diffuse, self.specular, self.smoothness = colour, float(diffuse), float(specular), float(
            smoothness)

    def bsdf(self, K, w_o, w_i, wavelength, intensity):
        w_o, w_i = vec(K, w_o), vec(K, w_i)
        if w_i[2] < 0 or w_o[2] < 0:
            return K.num(0.0), "cut"
        reflection_vector = (-w_i[0], -w_i[1], w_i[2])
        unit_z = vec(K, (0.0, 0.0, 1.0))
        diffuse = K.num(intensity) * self.colour.intensity_at_wavelength(K, wavelength) * K.num(self.diffuse)
        lobe = K.pow(abs(dot(K, w_o, reflection_vector)), K.num(self.smoothness))
        return diffuse + lobe * (K.num(self.specular) / dot(K, w_i, unit_z)), "value"


def fresnel(K, w_i, eta1, eta2):
    """-> (reflection_direction, transmission_direction, R, T, "tir" | "refract")."""
    w_i, eta1, eta2 = vec(K, w_i), K.num(eta1), K.num(eta2)
    one = K.num(1.0)
    normal = vec(K, (0.0, 0.0, 1.0)) if w_i[2] > 0 else vec(K, (-0.0, -0.0, -1.0))
    rdir = (-w_i[0], -w_i[1], w_i[2])
    r = eta1 / eta2
    cos1 = dot(K, normal, w_i)
    cos2_squared = one - r * r * (one - cos1 * cos1)
    if cos2_squared >= 0:
        cos2 = K.sqrt(cos2_squared)
        par = (eta1 * cos2 - eta2 * cos1) / (eta1 * cos2 + eta2 * cos1)
        per = (eta1 * cos1 - eta2 * cos2) / (eta1 * cos1 + eta2 * cos2)
        R = K.num(0.5) * (par * par + per * per)
        k = r * cos1 - cos2
        tdir = normalize(K, tuple((-r) * w + k * n for w, n in zip(w_i, normal)))
        T = one - R
        branch = "refract"
    else:
        R, T, tdir, branch = one, K.num(0.0), vec(K, (0.0, 0.0, 0.0)), "tir"
    if w_i[2] < 0:
        rdir = (rdir[0], rdir[1], rdir[2] * K.num(-1.0))
        tdir = (tdir[0], tdir[1], tdir[2] * K.num(-1.0))
    return rdir, tdir, R, T, branch


class Dielectric:
    kind = 3

    def __init__(self, eta):
        self.eta = eta

    def fresnel(self, K, w_i, wavelength):
        eta = self.eta.intensity_at_wavelength(K, wavelength)
        if K.num(w_i[2]) >= 0:
            return fresnel(K, w_i, K.num(1.0), eta)
        return fresnel(K, w_i, eta, K.num(1.0))

    def bsdf(self, K, w_o, w_i, wavelength, intensity):
        rdir, tdir, R, T, _ = self.fresnel(K, w_i, wavelength)
        w_o = vec(K, w_o)
        dr, dt = sub(w_o, rdir), sub(w_o, tdir)
        if dot(K, dr, dr) < K.num(THRESHOLD):
            return K.num(intensity) * R, "R"
        if dot(K, dt, dt) < K.num(THRESHOLD):
            return K.num(intensity) * T, "T"
        return K.num(0.0), "0"

    def sample(self, K, w_i, wavelength, coin=None):
        """-> (direction, pdf, arm, draws); `coin()` is rand's random::<bool>(), called only by the
        third arm."""
        rdir, tdir, R, T, _ = self.fresnel(K, w_i, wavelength)
        half = K.num(0.5)
        if T <= K.num(THRESHOLD):
            return rdir, half, "reflect-certain", 0
        if R <= K.num(THRESHOLD):
            return tdir, half, "transmit-certain", 0
        return (tdir, half, "coin-transmit", 1) if coin() else (rdir, half, "coin-reflect", 1)


# ---------------------------------------------------------------------------------- the integrators
def whitted_level(K, basis, retro, material, wavelength, ambient, lights, blocked, below=None, photon_intensity=0.0,
                  coin=None):
    """One level of WhittedIntegrator::integrate.  basis = (tangent, cotangent, normal); lights =
    [(direction, Spectrum)]; blocked[j]: light j's shadow ray hit something; below: None when the
    continuation ray leaves the scene or the recursion limit is 0, else the intensity returned by
    the level below.  -> the photon's intensity."""
    rows = tuple(vec(K, r) for r in basis)
    to_world = try_inverse(K, rows)
    normal = rows[2]
    w_retro = mat_vec(K, rows, vec(K, retro))
    acc = K.num(photon_intensity)
    for (direction, spectrum), shadowed in zip(lights, blocked):
        d = vec(K, direction)
        if shadowed:
            term = ambient.intensity_at_wavelength(K, wavelength)
        else:
            incoming = spectrum.intensity_at_wavelength(K, wavelength) * abs(dot(K, d, normal))
            term, _ = material.bsdf(K, w_retro, mat_vec(K, rows, d), wavelength, incoming)
        acc = acc + term
    if below is None:
        return acc + K.num(photon_intensity) * K.num(0.0)
    direction, _, _, _ = material.sample(K, w_retro, wavelength, coin)
    world = mat_vec(K, to_world, direction)
    out, _ = material.bsdf(K, w_retro, direction, wavelength, below)
    return acc + out * abs(dot(K, world, normal))


def simple_random_level(K, basis, retro, material, wavelength, incoming, coin=None):
    """One level of SimpleRandomIntegrator::integrate for a material with its own `sample`.
    incoming(world_w_o) is the intensity that arrives along the sampled direction (the sky's, or the
    level below's).  -> (intensity, arm, world_w_o)."""
    rows = tuple(vec(K, r) for r in basis)
    to_world = try_inverse(K, rows)
    w_i = mat_vec(K, rows, vec(K, retro))
    w_o, pdf, arm, _ = material.sample(K, w_i, wavelength, coin)
    world = mat_vec(K, to_world, w_o)
    arriving = K.num(incoming(world)) * pdf * abs(dot(K, world, rows[2]))
    out, _ = material.bsdf(K, w_o, w_i, wavelength, arriving)
    return out, arm, world


def relative_error(got, exact):
    """|got - exact| / |exact| as a float; 0 where both are 0, inf where only exact is."""
    got, exact = _MP.mpf(got), _MP.mpf(exact)
    if got == exact:
        return 0.0
    if exact == 0:
        return math.inf
    return float(abs(got - exact) / abs(exact))
