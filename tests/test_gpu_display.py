"""The ordered reduce, the film merge and the tone map against exact references, on synthetic data.

Every other check of accumulate_kernel, film_merge_kernel and tonemap_kernel runs on photons the
renderer happens to produce and compares GPU with GPU, or allows 1e-5 L2 on an image.  Here the
kernels are driven through their public entry points (accumulate_photons_device, Film.merge_state,
tone_map_device, AccumulationBuffer.to_image_rgb_u8, Film.to_image_rgb_u8 / _device) with inputs chosen
for where they can go wrong, and held to tests/display_reference.py: the lobes in `decimal` with a
derived bound, the Kahan chain and the merge as bit-exact IEEE replays, the tone map's bytes as exact
floors outside a derived ambiguity band.  tests/test_display_reference.py holds those references to
the oracle.  357 pixels (one full block, one full wave, one 37-lane wave), at most 9 samples.

Measured on an MI355X (printed by the tests):
  colours: largest error / colour_bound = 0.3253 (wavelength -500, intensity 2^30, X) over 2142
  photon-channels;
  tone map: 20.3 % of the 33 024 threshold points are ambiguous (6 703); on those the device and the
  oracle give different bytes at 262, in each of the three modes alike.  No byte outside the band differs.
"""
import math
from decimal import Decimal

import numpy as np
import pytest

import display_reference as D
from oracle import oracle_ffi as O
from vanrijn_amd import records as R
from vanrijn_amd.render import (AccumulationBuffer, Film, Tile, accumulate_photons_device, tone_map_device)

pytestmark = pytest.mark.gpu

NPIX = 357
SPPS = (1, 2, 3, 4, 5, 7, 8, 9)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def reduce(torch, photons, state=None):
    """accumulate_photons_device of photons [spp, n, 2] -> flat records (numpy).  The records sit 16
    bytes into their allocation: the documented 16-byte alignment alone must do.  `state`: flat records
    to continue from (accumulate=True), else fresh ones over a buffer full of NaN."""
    photons = np.ascontiguousarray(photons, dtype=np.float64)
    spp, n = photons.shape[0], photons.shape[1]
    buf = torch.full((8 * n + 2,), math.nan, dtype=torch.float64, device="cuda")
    st = buf[2:]
    assert st.data_ptr() % 32 == 16
    if state is not None:
        st.copy_(torch.from_numpy(np.ascontiguousarray(state)))
    ph = torch.from_numpy(photons).cuda()
    accumulate_photons_device(st.data_ptr(), ph.data_ptr(), n, spp, accumulate=state is not None)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    assert np.isnan(out[:2]).all()  # nothing written in front of the records
    return out[2:].copy()


def colours_of(torch, photons):
    """The per-sample colours [spp, n, 3] of photons [spp, n, 2]: one fresh spp-1 run per sample, where
    sum == colour and the compensation is 0, both exact (asserted)."""
    out = np.empty(photons.shape[:2] + (3,))
    for s in range(photons.shape[0]):
        f = R.fields(reduce(torch, photons[s:s + 1]))
        ok = ~np.isnan(f["colour_sum"])
        assert not f["colour_bias"][ok & ~np.isinf(f["colour_sum"])].any()
        assert np.array_equal(f["weight"], np.ones(photons.shape[1])) and not f["weight_bias"].any()
        out[s] = f["colour_sum"]
    return out


def assert_records_equal(got, want_state, what=""):
    f = R.fields(got)
    s, b, w, wb = want_state
    assert D.same_bits(f["colour_sum"], s), what
    assert D.same_bits(f["colour_bias"], b), what
    assert D.same_bits(f["weight"], w), what
    assert D.same_bits(f["weight_bias"], wb), what


def state_of(records):
    f = R.fields(records)
    return f["colour_sum"], f["colour_bias"], f["weight"], f["weight_bias"]


# ------------------------------------------------------------------------------------------------
# a. the reduce
# ------------------------------------------------------------------------------------------------
def test_colours_within_the_derived_bound(torch):
    pairs = [(wl, i) for i in D.colour_intensities() for wl in D.colour_wavelengths()]
    worst, worst_at, checked = Decimal(0), None, 0
    for first in range(0, len(pairs), NPIX):
        chunk = pairs[first:first + NPIX]
        chunk = chunk + [chunk[-1]] * (NPIX - len(chunk))  # the last run padded to the same 357 pixels
        f = R.fields(reduce(torch, np.array(chunk).reshape(1, NPIX, 2)))
        assert not f["colour_bias"].any() and not f["weight_bias"].any()  # spp 1, fresh: sum == colour
        assert np.array_equal(f["weight"], np.ones(NPIX))
        for p, (wl, inten) in enumerate(chunk):
            exact, bound = D.colour_exact(wl, inten), D.colour_bound(wl, inten)
            for c in range(3):
                got = float(f["colour_sum"][p, c])
                assert got == got and not math.isinf(got), (wl, inten, c)
                err = abs(Decimal(got) - exact[c])
                checked += 1
                if err / bound[c] > worst:
                    worst, worst_at = err / bound[c], (wl, inten, c)
                assert err <= bound[c], (wl, inten, c, got, float(exact[c]), float(err / bound[c]))
    print(f"colours: largest error / bound {float(worst):.4f} at {worst_at}, {checked} photon-channels")


def test_out_of_domain_wavelengths_give_zero(torch):
    photons = [(wl, i) for wl in D.OUT_OF_DOMAIN_WAVELENGTHS for i in (1.0, -2.5, 2.0 ** 30, 2.0 ** -30)]
    lit = D.photon_pool(NPIX, 3)
    for k, ph in enumerate(photons):  # spread over every wave, lit photons between them
        lit[(k * 11) % NPIX] = ph
    where = [(k * 11) % NPIX for k in range(len(photons))]
    assert len(set(where)) == len(photons)
    f = R.fields(reduce(torch, lit.reshape(1, NPIX, 2)))
    got = f["colour_sum"][where]
    assert np.array_equal(got, np.zeros_like(got)), got  # exactly 0, as the reference's exp gives
    assert not f["colour_bias"][where].any()
    for p in where:
        assert not O.xyz_for_wavelength(lit[p, 0]).any()
    # and through the batched path: four and five samples of them
    for spp in (4, 5):
        many = np.stack([np.roll(lit, s, axis=0) for s in range(spp)])
        colours = colours_of(torch, many)
        assert not np.isnan(colours).any() and not np.isinf(colours).any()
        assert_records_equal(reduce(torch, many), D.kahan_replay(colours), spp)


def test_nan_and_infinite_photons(torch):
    nan, inf = math.nan, math.inf
    special = [(550.0, nan), (0.0, nan), (550.0, inf), (550.0, -inf), (1e4, inf), (nan, 1.0), (nan, 0.0), (nan, -0.0),
               (inf, inf), (440.0, inf), (nan, nan)]
    lit = D.photon_pool(NPIX, 4)
    where = [(k * 29 + 5) % NPIX for k in range(len(special))]
    for p, ph in zip(where, special):
        lit[p] = ph
    with np.errstate(all="ignore"):
        ref = np.array([O.xyz_for_wavelength(wl) * (i * 360.0) for wl, i in lit])  # the reference's colour
    want = D.kahan_replay(ref[None])
    got = state_of(reduce(torch, lit.reshape(1, NPIX, 2)))
    assert np.isnan(want[0][where]).any(axis=1).sum() >= 8
    for g, w in zip(got, want):  # sums, compensations, weight, weight compensation
        assert np.array_equal(np.isnan(g), np.isnan(w))
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(g[np.isinf(w)], w[np.isinf(w)])
    # in a longer chain a NaN sample poisons its own pixel and channel only
    many = np.stack([np.roll(lit, 3 * s, axis=0) for s in range(9)])
    assert_records_equal(reduce(torch, many), D.kahan_replay(colours_of(torch, many)), "nan chain")


@pytest.fixture(scope="module")
def chain(torch):
    photons = D.photon_pool(9 * NPIX, 11).reshape(9, NPIX, 2)
    return photons, colours_of(torch, photons)


@pytest.mark.parametrize("spp", SPPS)
def test_chain_from_fresh_records(torch, chain, spp):
    photons, colours = chain
    assert_records_equal(reduce(torch, photons[:spp]), D.kahan_replay(colours[:spp]), spp)


@pytest.mark.parametrize("spp", SPPS)
def test_chain_continues_records(torch, chain, spp):
    photons, colours = chain
    first = reduce(torch, photons[:5])
    assert R.fields(first)["colour_bias"].any()  # non-zero compensations to continue from
    got = reduce(torch, photons[9 - spp:], state=first)
    assert_records_equal(got, D.kahan_replay(colours[9 - spp:], D.kahan_replay(colours[:5])), spp)


@pytest.mark.parametrize("spp", SPPS)
def test_chain_over_crafted_records(torch, chain, spp):
    photons, colours = chain
    rng = np.random.RandomState(17)
    s = rng.uniform(-3.0, 3.0, (NPIX, 3))
    b = rng.uniform(-1e-16, 1e-16, (NPIX, 3))
    w = rng.uniform(0.0, 40.0, NPIX)  # non-integer weights
    wb = rng.uniform(-1e-15, 1e-15, NPIX)
    s[0::7] = -0.0
    b[0::14] = -0.0
    s[3::31, 1] = math.nan  # a NaN in one channel stays in that channel
    s[5::41, 2] = math.inf
    w[2::23] = 2.0 ** 53  # + 1 is lost to the compensation
    got = reduce(torch, photons[:spp], state=R.from_fields(s, b, w, wb))
    want = D.kahan_replay(colours[:spp], (s, b, w, wb))
    assert_records_equal(got, want, spp)
    f = R.fields(got)
    assert np.isnan(f["colour_sum"][3::31, 1]).all() and not np.isnan(f["colour_sum"][3::31, 0]).any()


def _lane_sets():
    """Two assignments of dark lanes to the six waves of 357 pixels (wave w = pixels 64 w ..)."""
    a = np.zeros(NPIX, dtype=bool)
    a[0:64] = True                       # wave 0: all dark
    # wave 1: all lit
    a[128:192] = True; a[128 + 0] = False    # wave 2: one lit lane, lane 0
    a[192:256] = True; a[192 + 31] = False   # wave 3: lane 31
    a[256:320] = True; a[256 + 32] = False   # wave 4: lane 32 (the second block)
    a[320:357] = True; a[320 + 36] = False   # wave 5: the 37-lane wave, its last lane lit
    b = np.zeros(NPIX, dtype=bool)
    b[0:64] = True; b[63] = False            # wave 0: one lit lane, lane 63
    b[64 + 17] = True                        # wave 1: exactly one dark lane
    b[128 + 63] = True                       # wave 2: exactly one dark lane, the last
    b[192:256] = True; b[192 + 32] = False   # wave 3: lane 32 lit
    b[256] = True                            # wave 4: exactly one dark lane, lane 0
    b[320:357] = True                        # wave 5: the 37-lane wave all dark
    return {"a": a, "b": b}


_TIMES = {"all": range(9), "first batch": range(0, 4), "second batch": range(4, 8), "tail": range(8, 9),
          "both batches": range(0, 8)}


@pytest.mark.parametrize("when", sorted(_TIMES))
@pytest.mark.parametrize("lanes", ["a", "b"])
def test_dark_lanes(torch, chain, lanes, when):
    lit, colours = chain
    dark_lane = _lane_sets()[lanes]
    photons, want_colours = lit.copy(), colours.copy()
    for s in _TIMES[when]:
        photons[s, dark_lane] = 0.0  # {+0, +0}
        want_colours[s, dark_lane] = 0.0
    got = reduce(torch, photons)
    assert_records_equal(got, D.kahan_replay(want_colours), (lanes, when))
    f, all_lit = R.fields(got), R.fields(reduce(torch, lit))
    # lit pixels of the same waves: bit for bit what an all-lit run gives
    for k in ("colour_sum", "colour_bias", "weight", "weight_bias"):
        assert D.same_bits(f[k][~dark_lane], all_lit[k][~dark_lane]), k
    assert np.array_equal(f["weight"], np.full(NPIX, 9.0))
    if when == "all":  # a dark pixel: sums and compensations exactly +0
        for k in ("colour_sum", "colour_bias"):
            z = f[k][dark_lane]
            assert not z.any() and not np.signbit(z).any(), k


@pytest.mark.parametrize("spp", (1, 4, 5, 9))
def test_negative_zero_photons_are_not_dark(torch, chain, spp):
    lit, _ = chain
    photons = lit[:spp].copy()
    photons[:, 0:64] = (-0.0, 0.0)      # a whole wave of {-0.0, 0}
    photons[:, 64:128] = (0.0, -0.0)    # a whole wave of {0, -0.0}
    photons[:, 128:192:2] = (-0.0, 0.0)
    photons[:, 129:192:2] = (0.0, 0.0)  # mixed with dark ones
    photons[:, 320:357] = (0.0, -0.0)
    colours = colours_of(torch, photons)
    # both kinds are zero colours (a -0.0 colour reads back as +0: a fresh sum is +0 + -0.0)
    for zero in (colours[:, 0:128], colours[:, 128:192], colours[:, 320:357]):
        assert not zero.any() and not np.signbit(zero).any()
    assert_records_equal(reduce(torch, photons), D.kahan_replay(colours), spp)


# ------------------------------------------------------------------------------------------------
# b. the film merge
# ------------------------------------------------------------------------------------------------
def test_film_merge_equals_the_replay_and_the_host(torch):
    W, H = 23, 11
    want = np.zeros((W * H, 4))
    host = AccumulationBuffer(W, H)
    with Film(W, H) as film:
        for index, (tile, rec) in enumerate(D.merge_cases(W, H)):
            dev = torch.from_numpy(rec).cuda()
            assert film.merge_state(tile, dev.data_ptr()) == index
            want = D.merge_replay(want, rec, tile, W)
            with np.errstate(over="ignore"):  # 1 / 2^-1074
                host.merge_tile(tile, AccumulationBuffer.from_state(rec, tile.width(), tile.height()))
            got, seen = film.read()
            assert seen == index + 1
            assert D.same_bits(got.colour_buffer.reshape(-1, 3), want[:, 0:3]), tile
            assert D.same_bits(got.weight_buffer.reshape(-1), want[:, 3]), tile
            assert D.same_bits(got.colour_buffer, host.colour_buffer), tile
            assert D.same_bits(got.weight_buffer, host.weight_buffer), tile
            for a in (got.colour_sum_buffer, got.colour_bias_buffer, got.weight_bias_buffer):
                assert not a.any()
    assert np.isnan(want).any() and np.isinf(want).any()


# ------------------------------------------------------------------------------------------------
# c. the tone map
# ------------------------------------------------------------------------------------------------
def _records_with_weight_one(xyz):
    n = len(xyz)
    return R.from_fields(xyz, np.zeros((n, 3)), np.ones(n), np.zeros(n))


def tone_map_modes(torch, xyz):
    """The bytes of colours xyz [n, 3] through the three modes: {name: (bytes [n, 3], the colours that
    mode really mapped [n, 3])}.  Records carry weight 1 (sum * (1 / 1) is the sum); the film gets them
    by one merge into a cleared film, (0 * 0 + c * 1) * (1 / 1), and is read back to say what it holds."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    n = len(xyz)
    out = {}
    b = AccumulationBuffer(n, 1)
    b.colour_buffer[...] = xyz.reshape(1, n, 3)
    out["colour"] = (b.to_image_rgb_u8().data.reshape(n, 3), xyz)
    rec = torch.from_numpy(_records_with_weight_one(xyz)).cuda()
    rgb = torch.zeros(3 * n + 1, dtype=torch.uint8, device="cuda")
    tone_map_device(rec.data_ptr(), n, rgb.data_ptr())
    torch.cuda.synchronize()
    assert int(rgb[3 * n]) == 0  # nothing written past the last pixel
    out["records"] = (rgb[:3 * n].cpu().numpy().reshape(n, 3), xyz)
    with Film(n, 1) as film:
        film.merge_state(Tile(0, n, 0, 1), rec.data_ptr())
        held = film.read()[0].colour_buffer.reshape(n, 3).copy()
        host_bytes = film.to_image_rgb_u8().data.reshape(n, 3)
        rgb.zero_()
        film.to_image_rgb_u8_device(rgb.data_ptr())
        torch.cuda.synchronize()
        assert int(rgb[3 * n]) == 0
        assert np.array_equal(rgb[:3 * n].cpu().numpy().reshape(n, 3), host_bytes)
        out["film"] = (host_bytes, held)
    return out


def check_bytes(got, xyz, what):
    """Non-ambiguous channel values: the exact bytes.  Returns (ambiguous count, how many of them differ
    from the oracle's bytes)."""
    exact, amb = D.tone_map_exact(xyz)
    bad = (got != exact) & ~amb
    assert not bad.any(), (what, int(bad.sum()), xyz[bad.any(axis=1)][:4], got[bad][:4], exact[bad][:4])
    orc = O.tone_map(xyz)
    return int(amb.sum()), int((got[amb] != orc[amb]).sum())


def test_tone_map_threshold_set(torch):
    xyz = D.threshold_points()[0]
    for name, (got, mapped) in tone_map_modes(torch, xyz).items():
        ambiguous, differ = check_bytes(got, mapped, name)
        print(f"tone map, {name} mode: {len(xyz)} threshold points, {ambiguous} ambiguous channel values "
              f"({100.0 * ambiguous / len(xyz):.1f} %), device != oracle on {differ} of them")
        assert differ <= ambiguous


@pytest.mark.parametrize("npix", (1, 255, 256, 357))
def test_tone_map_edges_and_pixel_counts(torch, npix):
    # the first npix of: every edge point, then a sample of the threshold set
    xyz = np.concatenate([D.edge_points(), D.threshold_points()[0][::97]])[:npix]
    assert len(xyz) == npix
    for name, (got, mapped) in tone_map_modes(torch, xyz).items():
        check_bytes(got, mapped, (name, npix))


def test_tone_map_records_weights(torch):
    tiny = 2.0 ** -1074
    rec, s, w = D.weight_records(NPIX)
    colour = D.records_colour(rec)
    assert not colour[w == 0.0].any()  # weight 0: black, whatever the sums
    assert np.isnan(colour[(w == tiny) & (s[:, 0] == 0.0)]).all()  # 0 * (1 / 2^-1074) = 0 * inf
    assert np.isinf(colour[(w == tiny) & (s[:, 0] == 0.5)]).all()
    dev = torch.from_numpy(rec).cuda()
    rgb = torch.zeros(3 * NPIX, dtype=torch.uint8, device="cuda")
    tone_map_device(dev.data_ptr(), NPIX, rgb.data_ptr())
    torch.cuda.synchronize()
    got = rgb.cpu().numpy().reshape(NPIX, 3)
    check_bytes(got, colour, "records with special weights")
    assert not got[w == 0.0].any() and not got[np.isnan(w)].any()
    assert got[w == 3.0].any()
