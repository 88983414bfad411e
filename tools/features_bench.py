"""The feature pass against the routes a caller had before it: C3's scene, 1024 x 1024 at 64 spp.

    python tools/features_bench.py [--size 1024] [--spp 64] [--rounds 5] [--warmup 1] [--out FILE]

Legs, alternating inside each round (one process, one device, one stream, HIP events), after warm-up rounds:
  features         vr_render_features_device, records and albedo state;
  features_only    the same without the albedo (no wavelength drawn, no material read);
  albedo_only      the same without the records;
  staged           vr_camera_rays_device + vr_query_closest_device with 144-B records: the staged route to
                   the same first hits, WITHOUT the per-pixel reduction its caller must still add;
  render           vr_render_tile_device of the same frame (wall time of the call's launches, and the
                   library's own kernel and reduce times).
Median and best per leg, and a check that the pass counts the hits the staged route finds.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vanrijn_amd import scenes  # noqa: E402
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE  # noqa: E402
from vanrijn_amd.render import (Tile, camera_rays_device, query_closest_device, render_features_device,  # noqa: E402
                                render_tile_device, stream_check_error)

SEED = 0x5EED0001


def run(size, spp, rounds, warmup):
    ds = scenes.main_scene().device_scene(0)
    tile = Tile(0, size, 0, size)
    npix, n = size * size, size * size * spp
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    with torch.cuda.stream(stream):
        o = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        d = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        ids = torch.zeros(n, dtype=torch.int64, device="cuda")
        hits = torch.zeros(n * 4, dtype=torch.int64, device="cuda")      # vr_ray_hit, 32 B
        records = torch.zeros(n * 18, dtype=torch.float64, device="cuda")  # vr_hit_record, 144 B
        feat = torch.zeros(npix * 8, dtype=torch.int64, device="cuda")   # vr_pixel_features, 64 B
        albedo = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        state = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    stream.synchronize()

    def features(with_records, with_albedo):
        render_features_device(ds, tile, size, size, spp, SEED, 0, feat.data_ptr() if with_records else None,
                               albedo.data_ptr() if with_albedo else None, stream_ptr=sp)

    def staged():
        camera_rays_device(ds, tile, size, size, spp, SEED, 0, o.data_ptr(), d.data_ptr(), ids.data_ptr(), sp)
        query_closest_device(ds, n, o.data_ptr(), d.data_ptr(), hits.data_ptr(), records.data_ptr(), sp)

    legs = {"features_only": lambda: features(True, False), "albedo_only": lambda: features(False, True),
            "features": lambda: features(True, True), "staged": staged}
    times = {k: [] for k in list(legs) + ["render", "render_kernel", "render_reduce"]}
    for r in range(warmup + rounds):
        events = []
        for leg, call in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            events.append((leg, e0, e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = render_tile_device(ds, tile, size, size, spp, SEED, 0, state.data_ptr(), sp, timed=True)
        e1.record(stream)
        events.append(("render", e0, e1))
        stream.synchronize()
        if r >= warmup:
            for leg, a, b in events:
                times[leg].append(a.elapsed_time(b))
            times["render_kernel"].append(st["kernel_ms"])
            times["render_reduce"].append(st["reduce_ms"])
    stream_check_error(ds, sp)
    rec = feat.cpu().numpy().view(PIXEL_FEATURES_DTYPE)
    valid = int((hits.view(n, 4)[:, 2] >> 32).sum())  # vr_ray_hit::valid, the high word of the third quad word
    out = {"scene": "main_scene (C3)", "size": size, "spp": spp, "samples": n,
           "hit_fraction": round(int(rec["hits"].sum()) / n, 4),
           "hits_equal_staged": int(rec["hits"].sum()) == valid and bool((rec["samples"] == spp).all()),
           "staged_bytes": n * (72 + 176), "feature_bytes": npix * 128, "legs": {}}
    for leg, t in times.items():
        out["legs"][leg] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4)}
    med = {k: statistics.median(t) for k, t in times.items()}
    out["features_over_staged"] = round(med["features"] / med["staged"], 4)
    out["features_over_render_kernel"] = round(med["features"] / med["render_kernel"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("features_bench needs a GPU: no timing is taken without one")
    result = {"tool": "features_bench", "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    result.update(run(a.size, a.spp, a.rounds, a.warmup))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not result["hits_equal_staged"]:
        sys.exit("the feature pass and the staged route count different hits")


if __name__ == "__main__":
    main()
