"""Drop-in call pattern (src/main.rs:197-216) breakdown on one GPU: per-call latency of
partial_render_scene (1 spp, full frame, host buffers), merge_tile time, and the aggregate
Msamples/s with T worker threads + one merging thread -- then the same pattern on a device-resident
film (vanrijn_amd.Film): T workers call Film.partial_render_scene (render + merge_tile on the GPU),
the main thread takes to_image_rgb_u8 once per 16 merged frames (main.rs's display role), with the
HIP-event times of the film's merge and tone-map kernels.  Each Msamples/s figure is one run of
`frames` frames.
    python tools/dropin.py [size] [frames]"""
import json
import os
import sys
import threading
import time

import torch  # noqa: F401  (binds the library to torch's HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from vanrijn_amd import scenes  # noqa: E402
from vanrijn_amd.render import (AccumulationBuffer, Film, Tile, partial_render_scene,  # noqa: E402
                                render_tile_device)

DISPLAY_EVERY = 16  # merged frames per to_image_rgb_u8 of the film leg


def film_leg(dscene, size, frames, threads):
    """main.rs:197-243 on a film: `threads` workers each call Film.partial_render_scene (1 spp, whole
    frame; the tile buffer stays on the device and merge_tile runs there) until `frames` passes are
    done; the main thread calls to_image_rgb_u8 once per DISPLAY_EVERY merged frames and once at the
    end (3 B per pixel cross PCIe)."""
    tile = Tile(0, size, 0, size)
    with Film(size, size) as film:
        # warm-up as bench.drop_in_leg's: one call per worker at once, so every call context exists
        warm = [threading.Thread(target=film.partial_render_scene, args=(dscene, tile)) for _ in range(threads)]
        for w in warm:
            w.start()
        for w in warm:
            w.join()
        film.to_image_rgb_u8()
        film.clear()
        todo = iter(range(frames))
        lock = threading.Lock()
        cond = threading.Condition()
        merged = [0]

        def worker():
            while True:
                with lock:
                    if next(todo, None) is None:
                        break
                film.partial_render_scene(dscene, tile)
                with cond:
                    merged[0] += 1
                    cond.notify()

        t0 = time.perf_counter()
        ws = [threading.Thread(target=worker) for _ in range(threads)]
        for w in ws:
            w.start()
        shown = images = 0
        while shown < frames:
            due = min(frames, shown + DISPLAY_EVERY)
            with cond:
                cond.wait_for(lambda: merged[0] >= due)
            film.to_image_rgb_u8()
            images += 1
            shown = due
        dt = time.perf_counter() - t0
        for w in ws:
            w.join()
        buf, seen = film.read()
        assert seen == frames and float(buf.weight_buffer.min()) == frames
    return {"msamples_s": round(frames * size * size / dt / 1e6, 3), "ms_per_frame": round(dt / frames * 1e3, 3),
            "images": images}


def film_kernel_times(dscene, size, reps=6):
    """HIP-event times of the film's merge and tone-map kernels: vr_film_merge_state and
    vr_film_to_image_rgb_u8_device only enqueue on the caller's stream, so events recorded around
    them on that stream bracket the kernels.  Medians of `reps` after one warm-up."""
    tile = Tile(0, size, 0, size)
    stream = torch.cuda.Stream()
    state = torch.zeros(size * size * 8, dtype=torch.float64, device="cuda")
    rgb = torch.empty(size * size * 3, dtype=torch.uint8, device="cuda")
    render_tile_device(dscene, tile, size, size, 1, 0x5EED0001, 0, state.data_ptr(), stream.cuda_stream)
    marks = []
    with Film(size, size) as film:
        for _ in range(reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record(stream)
            film.merge_state(tile, state.data_ptr(), stream.cuda_stream)
            ev[1].record(stream)
            film.to_image_rgb_u8_device(rgb.data_ptr(), stream.cuda_stream)
            ev[2].record(stream)
            marks.append(ev)
        stream.synchronize()
    merge = sorted(a.elapsed_time(b) for a, b, _ in marks[1:])
    tone = sorted(b.elapsed_time(c) for _, b, c in marks[1:])
    return {"merge_kernel_ms": round(merge[len(merge) // 2], 4), "tonemap_kernel_ms": round(tone[len(tone) // 2], 4),
            "reps": reps}


size = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 32
ds = scenes.main_scene().device_scene(0)
tile = Tile(0, size, 0, size)
out = {"size": size}
lat = []
os.environ["VR_HOST_TIMING"] = "1"
for i in range(6):
    t0 = time.perf_counter()
    b = partial_render_scene(ds, tile, size, size)
    lat.append((time.perf_counter() - t0) * 1e3)
out["call_ms"] = [round(x, 2) for x in lat]
t0 = time.perf_counter()
for i in range(6):
    b2 = AccumulationBuffer._for_output(size, size)
    for a in (b2.colour_buffer, b2.colour_sum_buffer, b2.colour_bias_buffer, b2.weight_buffer, b2.weight_bias_buffer):
        a.fill(0.0)
out["alloc_touch_ms"] = round((time.perf_counter() - t0) / 6 * 1e3, 2)
grab = {}
for g in ("64", "128", "256", "512", ""):
    if g:
        os.environ["VR_GRAB"] = g
    else:
        os.environ.pop("VR_GRAB", None)
    ts = []
    for i in range(5):
        t0 = time.perf_counter()
        partial_render_scene(ds, tile, size, size)
        ts.append((time.perf_counter() - t0) * 1e3)
    grab[g or "auto"] = round(sorted(ts)[2], 2)
out["call_ms_by_grab"] = grab
img = AccumulationBuffer(size, size)
mt = []
for i in range(6):
    t0 = time.perf_counter()
    img.merge_tile(tile, b)
    mt.append((time.perf_counter() - t0) * 1e3)
out["merge_ms"] = [round(x, 2) for x in mt]
out["threads"] = {}
for t in (1, 2, 4, 8, 16):
    r = bench.drop_in_leg(ds, size, size, frames, t, 0)
    out["threads"][t] = {"msamples_s": r["value"], "ms_per_frame": r["ms_per_frame"]}
    print(t, r["value"], flush=True)
film = {"display_every": DISPLAY_EVERY}
lat = []
with Film(size, size) as f:
    for i in range(6):
        t0 = time.perf_counter()
        f.partial_render_scene(ds, tile)
        lat.append((time.perf_counter() - t0) * 1e3)
film["call_ms"] = [round(x, 2) for x in lat]
film.update(film_kernel_times(ds, size))
film["threads"] = {}
for t in (1, 2, 4, 8, 16):
    film["threads"][t] = film_leg(ds, size, frames, t)
    print("film", t, film["threads"][t]["msamples_s"], flush=True)
out["film"] = film
print(json.dumps(out))
