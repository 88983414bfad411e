"""The display references (tests/display_reference.py) held to the oracle, on the CPU.

tests/test_gpu_display.py compares the reduce, the film merge and the tone map with exact references;
a wrong reference must not pass for a wrong kernel, so each one is checked here against the C oracle
(glibc's exp and pow) or the library's host code, on the very inputs the GPU tests use.

Figures of the threshold set (256 byte thresholds x 43 ulp offsets x 3 channels = 33 024 points):
20.3 % of the points are ambiguous (6 703), every one of them within 17 ulp of its threshold; on 711 of
them glibc's pow lands on the other side of the integer than the exact value.  The oracle's lobes
reach 0.338 of colour_bound at the worst wavelength.
"""
from decimal import Decimal

import numpy as np
import pytest

import display_reference as D
from oracle import oracle_ffi as O
from vanrijn_amd.render import AccumulationBuffer


def test_oracle_lobes_within_colour_bound():
    worst = Decimal(0)
    for wl in D.colour_wavelengths():
        got = O.xyz_for_wavelength(wl)
        exact = D.colour_exact(wl, 1.0 / 360.0)  # 360 * (1 / 360) == 1.0 exactly in f64 and here
        bound = D.colour_bound(wl, 1.0 / 360.0)
        for c in range(3):
            err = abs(Decimal(float(got[c])) - exact[c])
            worst = max(worst, err / bound[c])
            assert err <= bound[c], (wl, c, got[c], exact[c], err / bound[c])
    print(f"oracle lobes: worst error / bound {float(worst):.3f}")


def test_oracle_lobes_are_zero_out_of_domain():
    for wl in D.OUT_OF_DOMAIN_WAVELENGTHS:
        assert not O.xyz_for_wavelength(wl).any(), wl
        assert not any(D.lobes_exact(wl)[0]), wl


def test_scale_of_the_lobe_test_is_one():
    assert 360.0 * (1.0 / 360.0) == 1.0 and Decimal(360.0) * Decimal(1.0 / 360.0) != 1  # the exact product is not 1


@pytest.fixture(scope="module")
def thresholds():
    xyz, channel, k, u = D.threshold_points()
    exact, amb = D.tone_map_exact(xyz)
    return xyz, channel, k, u, exact, amb


def test_tone_map_bytes_threshold_set(thresholds):
    xyz, _, _, _, exact, amb = thresholds
    got = O.tone_map(xyz)
    assert np.array_equal(got[~amb], exact[~amb])
    differ = int((got[amb] != exact[amb]).sum())
    print(f"threshold set: {int(amb.sum())} ambiguous channel values, the oracle differs from the exact floor on {differ}")


def test_tone_map_bytes_edge_set():
    xyz = D.edge_points()
    exact, amb = D.tone_map_exact(xyz)
    assert not amb.any()
    assert np.array_equal(O.tone_map(xyz), exact)
    lin = D.linear_rgb(xyz)
    # the set reaches what it is meant to: the knee and both neighbours, 1 and both neighbours
    for v in (D.KNEE, D.step(D.KNEE, -1), D.step(D.KNEE, 1), 1.0, D.step(1.0, -1), D.step(1.0, 1), 2.0):
        assert (lin == v).any(), v
    assert np.isnan(lin).any() and np.isposinf(lin).any() and np.isneginf(lin).any()


def test_tone_map_bytes_of_weighted_records():
    rec, s, w = D.weight_records()
    colour = D.records_colour(rec)
    assert colour.shape == (357, 3) and not colour[w == 0.0].any()
    exact, amb = D.tone_map_exact(colour)
    assert not amb.any()
    assert np.array_equal(O.tone_map(colour), exact)
    assert exact[w == 3.0].any() and not exact[np.isnan(w)].any()


def test_tone_map_coverage_conditions(thresholds):
    xyz, channel, k, u, exact, amb = thresholds
    n = len(xyz)
    lin = D.linear_rgb(xyz)
    idx = np.arange(n)
    value = lin[idx, channel]  # the channel that carries the threshold
    own_amb = amb[idx, channel]
    own_byte = exact[idx, channel]
    # the other two channels stay away from any threshold
    others = amb.copy()
    others[idx, channel] = False
    assert not others.any()
    # at most 30 % of the threshold points are ambiguous
    share = own_amb.mean()
    print(f"threshold points: {n}, ambiguous {int(own_amb.sum())} ({100 * share:.1f} %)")
    assert share <= 0.30
    # at every byte threshold both bytes occur among the non-ambiguous points
    for kk in range(1, 256):
        sel = (k == kk) & ~own_amb
        seen = set(own_byte[sel].tolist())
        assert {kk - 1, kk} <= seen, (kk, seen)
    # every point 64 ulp or more from its threshold is non-ambiguous
    dist = D.ulps_between(value, u)
    assert not own_amb[dist >= 64].any()
    assert (dist >= 64).sum() > n // 2 and (dist <= 1).sum() >= 3 * 3 * 256 // 2
    print(f"largest distance of an ambiguous point from its threshold: {int(dist[own_amb].max())} ulp")


def _film_buffer(film, width, height):
    b = AccumulationBuffer(width, height)
    b.colour_buffer[...] = film[:, 0:3].reshape(height, width, 3)
    b.weight_buffer[...] = film[:, 3].reshape(height, width)
    return b


def test_merge_replay_equals_host_merge_tile():
    W, H = 23, 11
    film = np.zeros((W * H, 4))
    host = AccumulationBuffer(W, H)
    zero_weight_sums = 0
    for tile, rec in D.merge_cases(W, H):
        before = film
        film = D.merge_replay(film, rec, tile, W)
        with np.errstate(over="ignore"):  # 1 / 2^-1074
            host.merge_tile(tile, AccumulationBuffer.from_state(rec, tile.width(), tile.height()))
        assert D.same_bits(host.colour_buffer.reshape(-1, 3), film[:, 0:3]), tile
        assert D.same_bits(host.weight_buffer.reshape(-1), film[:, 3]), tile
        zero_weight_sums += int(((film[:, 3] == 0.0) & (before[:, 3] != 0.0)).sum())
    # the cases reach what they are meant to: NaN and infinite colours, and w1 + w2 == 0
    assert np.isnan(film).any() and np.isinf(film).any()
    assert zero_weight_sums >= 20


def test_kahan_replay_equals_oracle_update_pixel():
    # orc_update_pixel folds one photon into one pixel; its colour is glibc's, so the replay is fed the
    # colours the oracle itself forms (xyz_for_wavelength * (I * 360)) and must then agree bit for bit
    photons = D.photon_pool(40, 7).reshape(8, 5, 2)
    colours = np.empty((8, 5, 3))
    for s in range(8):
        for p in range(5):
            colours[s, p] = O.xyz_for_wavelength(photons[s, p, 0]) * (photons[s, p, 1] * 360.0)
    s_, b_, w_, wb_ = D.kahan_replay(colours)
    lib = O.lib()
    for p in range(5):
        colour, csum, bias = np.zeros(3), np.zeros(3), np.zeros(3)
        w, wb = np.zeros(1), np.zeros(1)
        for s in range(8):
            lib.orc_update_pixel(O._ptr(colour), O._ptr(csum), O._ptr(bias), O._ptr(w), O._ptr(wb),
                                 photons[s, p, 0], photons[s, p, 1] * 360.0, 1.0)
        assert D.same_bits(csum, s_[p]) and D.same_bits(bias, b_[p])
        assert w[0] == w_[p] == 8.0 and wb[0] == wb_[p]
