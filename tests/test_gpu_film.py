"""The film (vr_film, vanrijn_amd.Film): the reference's full-image AccumulationBuffer on the device.

main.rs:197-243 renders 1-spp tiles on worker threads, folds each into the image with merge_tile
and displays the image through to_image_rgb_u8.  With a film the tile buffer never leaves the GPU
and merge_tile runs there.  The yardstick everywhere is the library's host path -- render_tile /
partial_render_scene into host buffers, then AccumulationBuffer.merge_tile, itself pinned to the
oracle in test_abi.py and test_gpu_parity.py -- replayed in the film's reported merge order: colour
and weight must be equal bit for bit, and the three arrays merge_tile never touches must be zero.
"""
import threading

import numpy as np
import pytest

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import AccumulationBuffer, Film, Tile, TileIterator, render_tile, render_tile_device
from vanrijn_amd.scene import DeviceScene

pytestmark = pytest.mark.gpu

PARTIAL_SEED = 0x5EED0001  # vr_partial_render_scene's stream seed (include/vanrijn_amd.h)


@pytest.fixture(scope="module")
def small_main():
    return scenes.main_scene(scenes.displaced_mesh(16, scenes._BUNNY_BUMPS, 0xB0BB1E, 24, 0.04,
                                                   (1.25, 1.05, 1.15), (-1.7, -0.8, 0.0)))


def _run_threads(fns):
    errs = []

    def work(fn):
        try:
            fn()
        except Exception as e:  # noqa: BLE001 -- reported below
            errs.append(e)

    ts = [threading.Thread(target=work, args=(fn,)) for fn in fns]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs


def _assert_film_equals(got: AccumulationBuffer, want: AccumulationBuffer, what=""):
    assert np.array_equal(got.colour_buffer, want.colour_buffer), what
    assert np.array_equal(got.weight_buffer, want.weight_buffer), what
    for a in (got.colour_sum_buffer, got.colour_bias_buffer, got.weight_bias_buffer):
        assert not a.any(), what


def _host_merge(image, ds, tile, spp, seed, first_sample):
    """The host path: render the tile into a host buffer, merge_tile it into `image`."""
    image.merge_tile(tile, render_tile(ds, tile, image.height(), image.width(), spp, seed, first_sample))


def _copy(image):
    c = AccumulationBuffer(image.width(), image.height())
    c.colour_buffer[...] = image.colour_buffer
    c.weight_buffer[...] = image.weight_buffer
    return c


def test_ragged_tiles_several_passes(small_main):
    W, H = 52, 37
    ds = small_main.device_scene(0)
    tiles = list(TileIterator(W, H, 16))
    assert {t.width() for t in tiles} == {16, 4} and {t.height() for t in tiles} == {16, 5}
    want = AccumulationBuffer(W, H)
    with Film(W, H) as film:
        merges = 0
        for spp, first in ((1, 0), (1, 1), (1, 2), (3, 3)):
            for t in tiles:
                assert film.render_tile(ds, t, spp, 11, first) == (merges, first)
                _host_merge(want, ds, t, spp, 11, first)
                merges += 1
            got, seen = film.read()
            assert seen == merges
            _assert_film_equals(got, want, (spp, first))
        # the last pixel alone, and a 1-wide column at an odd column
        for t in (Tile(W - 1, W, H - 1, H), Tile(7, 8, 0, H)):
            film.render_tile(ds, t, 1, 11, 6)
            _host_merge(want, ds, t, 1, 11, 6)
        got, seen = film.read()
        assert seen == merges + 2
        _assert_film_equals(got, want, "1x1 and column tiles")


def test_merge_indices_and_clear(small_main):
    W, H = 24, 10
    ds = small_main.device_scene(0)
    full = Tile(0, W, 0, H)
    with Film(W, H) as film:
        assert [film.render_tile(ds, full, 1, 11, k)[0] for k in range(5)] == [0, 1, 2, 3, 4]
        assert film.read()[1] == 5
        film.clear()
        got, seen = film.read()
        assert seen == 0
        _assert_film_equals(got, AccumulationBuffer.new(W, H), "cleared")
        assert film.render_tile(ds, full, 1, 11, 9) == (0, 9)
        want = AccumulationBuffer(W, H)
        _host_merge(want, ds, full, 1, 11, 9)
        _assert_film_equals(film.read()[0], want, "after clear")


def test_concurrent_callers_overlapping_tiles(small_main):
    W, H = 56, 40
    ds = DeviceScene(small_main.spec(), 0)  # a fresh scene: its pass counter starts at 0
    tiles = (Tile(0, W, 0, H), Tile(8, 40, 5, 33))
    calls = []  # (merge_index, first_sample, tile); list.append is atomic
    with Film(W, H) as film:
        def worker(k):
            def run():
                for _ in range(4):
                    calls.append(film.partial_render_scene(ds, tiles[k % 2]) + (tiles[k % 2],))
            return run

        _run_threads([worker(k) for k in range(8)])
        got, seen = film.read()
    assert seen == 32
    assert sorted(c[0] for c in calls) == list(range(32))
    assert sorted(c[1] for c in calls) == list(range(32))
    want = AccumulationBuffer(W, H)
    for _, first, t in sorted(calls):
        _host_merge(want, ds, t, 1, PARTIAL_SEED, first)
    _assert_film_equals(got, want, "replay in merge_index order")


def test_snapshot_under_load(small_main):
    W, H = 56, 40
    ds = small_main.device_scene(0)
    tiles = (Tile(0, W, 0, H), Tile(8, 40, 5, 33))
    per_thread = 6
    calls, snaps = [], []
    with Film(W, H) as film:
        def merger(k):
            def run():
                for i in range(per_thread):
                    t = tiles[(k + i) % 2]
                    calls.append(film.render_tile(ds, t, 1, 11, k * per_thread + i) + (t,))
            return run

        def reader():
            for _ in range(4):
                snaps.append(film.read())

        _run_threads([merger(k) for k in range(4)] + [reader])
        snaps.append(film.read())
    assert sorted(c[0] for c in calls) == list(range(4 * per_thread))
    seen = [s[1] for s in snaps]
    assert seen == sorted(seen) and seen[-1] == 4 * per_thread
    prefix = {0: AccumulationBuffer(W, H)}
    want = AccumulationBuffer(W, H)
    for index, first, t in sorted(calls):
        _host_merge(want, ds, t, 1, 11, first)
        if index + 1 in seen:
            prefix[index + 1] = _copy(want)
    for got, n in snaps:
        _assert_film_equals(got, prefix[n], f"snapshot of the first {n} merges")


def test_tone_map_bytes(small_main):
    import torch
    W, H = 52, 37
    ds = small_main.device_scene(0)
    with Film(W, H) as film:
        for k in range(3):
            film.render_tile(ds, Tile(0, W, 0, H), 2, 11, 2 * k)
        film.render_tile(ds, Tile(3, 30, 2, 21), 1, 11, 6)  # unequal weights
        image = film.to_image_rgb_u8()
        assert film.merges_seen == 4
        want = film.read()[0].to_image_rgb_u8()
        assert image.data.shape == (H, W, 3) and image.data.any()
        assert np.array_equal(image.data, want.data)
        stream = torch.cuda.Stream()
        rgb = torch.zeros(H * W * 3, dtype=torch.uint8, device="cuda")
        assert film.to_image_rgb_u8_device(rgb.data_ptr(), stream.cuda_stream) == 4
        stream.synchronize()
        assert np.array_equal(rgb.cpu().numpy().reshape(H, W, 3), want.data)


def test_merge_state(small_main):
    import torch
    W, H = 52, 37
    ds = small_main.device_scene(0)
    sub = Tile(5, 34, 3, 30)
    stream = torch.cuda.Stream()
    state = torch.zeros(sub.width() * sub.height() * 8, dtype=torch.float64, device="cuda")
    want = AccumulationBuffer(W, H)
    with Film(W, H) as film:
        film.render_tile(ds, Tile(0, W, 0, H), 1, 11, 0)
        _host_merge(want, ds, Tile(0, W, 0, H), 1, 11, 0)
        render_tile_device(ds, sub, H, W, 4, 11, 1, state.data_ptr(), stream.cuda_stream)
        assert film.merge_state(sub, state.data_ptr(), stream.cuda_stream) == 1
        got, seen = film.read()  # waits for the merge
    assert seen == 2
    want.merge_tile(sub, AccumulationBuffer.from_state(state, sub.width(), sub.height()))
    _assert_film_equals(got, want, "merge_state")


def test_failed_call_leaves_the_film_intact(small_main):
    W = H = 64
    full = Tile(0, W, 0, H)
    ds = DeviceScene(small_main.spec(), 0)
    want = AccumulationBuffer(W, H)
    with Film(W, H) as film:
        film.render_tile(ds, full, 1, 11, 0)
        _host_merge(want, ds, full, 1, 11, 0)
        before = film.read()[0]
        _assert_film_equals(before, want, "first pass")
        ds.set_fault_object(1)  # the mesh: every hit on it takes the singular-basis path
        try:
            with pytest.raises(N.VrError) as e:
                film.render_tile(ds, full, 1, 11, 1)
            assert e.value.code == -5  # VR_ERROR_SINGULAR_BASIS
            with pytest.raises(N.VrError) as e:
                film.partial_render_scene(ds, full)
            assert e.value.code == -5
        finally:
            ds.set_fault_object(-1)
        after = film.read()[0]
        assert np.array_equal(after.colour_buffer, before.colour_buffer)
        assert np.array_equal(after.weight_buffer, before.weight_buffer)
        # the next calls on this thread are clean and merge
        for first in (2, 3):
            last, _ = film.render_tile(ds, full, 1, 11, first)
            _host_merge(want, ds, full, 1, 11, first)
        got, seen = film.read()
        assert seen == last + 1 and 3 <= seen <= 5  # a failed call may take an index
        _assert_film_equals(got, want, "after the failed calls")


def test_launch_variant_flags_give_the_same_film(small_main):
    W, H = 52, 37
    full = Tile(0, W, 0, H)
    ds = DeviceScene(small_main.spec(), 0)
    with Film(W, H) as plain, Film(W, H) as flagged:
        plain.render_tile(ds, full, 2, 11, 0)
        ds.set_launch_flags(no_cull=True, no_coop=True)
        try:
            flagged.render_tile(ds, full, 2, 11, 0)
        finally:
            ds.set_launch_flags()
        _assert_film_equals(flagged.read()[0], plain.read()[0], "NO_CULL | NO_COOP")
