"""The grid of tests/test_oracle_materials.py and tests/test_gpu_material_branches.py: incidences,
etas, Phong smoothness, strengths, and the error measures both files use."""
import math

import material_reference as MR

ULP16 = 2.0 ** -49
DEG = math.pi / 180.0
ANGLES = [("0", 0.0), ("1e-8", 1e-8), ("10", 10 * DEG), ("41", 41 * DEG), ("42", 42 * DEG), ("45", 45 * DEG),
          ("56.3", 56.3 * DEG), ("60", 60 * DEG), ("89", 89 * DEG), ("90-1e-6", math.pi / 2 - 1e-6)]
AZIMUTHS = [0.0, 0.7]
ETAS = [1.0, 1.0 + 1e-12, 1.3, 1.5, 2.4, 0.75]
SMOOTHNESS = [0.0, 1.0, 40.0, 1000.0]
STRENGTHS = [0.0, 1.0]
WAVELENGTH, INTENSITY = 523.25, 0.7
COLOUR = MR.Spectrum(400.0, 700.0, [0.5, 1.0, 0.75, 0.25])
BASES = (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0x2545F4914F6CDD1D, 0x123456789ABCDEF)
FIRST_DRAW = 5


def direction(theta, phi, side):
    if theta == 0.0:
        return (0.0, 0.0, float(side))
    return (math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), side * math.cos(theta))


def incidences():
    for name, theta in ANGLES:
        for phi in (AZIMUTHS if theta else AZIMUTHS[:1]):
            for side in (1, -1):
                yield f"{name}/{phi}/{'+' if side > 0 else '-'}", direction(theta, phi, side)


W_IN = list(incidences())


def rel(got, exact):
    exact = MR._MP.mpf(exact)
    if exact == 0:  # eta 1: R is exactly 0; nothing to be relative to but the photon's scale, 1
        return abs(float(got))
    if exact != 0 and abs(exact) < 2.0 ** -1022:  # underflows in f64: only "tiny" can be asked
        return 0.0 if abs(got) < 2.0 ** -1021 else math.inf
    return MR.relative_error(got, exact)


def vec_err(got, exact):
    return max(float(abs(MR._MP.mpf(g) - e)) for g, e in zip(got, exact))
