"""Per-lane integrator throughput: vr_integrate_rays_device against the render megakernel on the same samples.

    python tools/integrate_bench.py [--rounds 10] [--warmup 2] [--out FILE]

Configurations: C3, the main.rs scene's 1024 x 1024 frame at 1 spp, and C1, the bench
scene's 256 x 256 frame at 16 spp.  The rays are the scene's own camera rays, made once on the device by
vr_camera_rays_device, so both sides trace the same samples with the same random streams.
Legs, alternating inside each round (one process, one device, one stream), after warm-up rounds:
  integrate_info  one launch of vr_integrate_rays_device writing photons and path info, HIP events;
  integrate       the same without the info array;
  render          vr_render_tile_device, timed: its render-kernel time (and the ordered reduce's apart).
Median and best per leg, the ratio integrate / render, and a check that the staged pipeline
(integrate, then vr_accumulate_photons_device) reproduces the render's records bit for bit.
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
from vanrijn_amd.render import (Tile, accumulate_photons_device, camera_rays_device, integrate_rays_device,  # noqa: E402
                                render_tile_device, stream_check_error)

SEED = 0x5EED0001
CONFIGS = {"c3": (scenes.main_scene, 1024, 1), "c1": (scenes.bench_scene, 256, 16)}


def run(name, rounds, warmup):
    make, size, spp = CONFIGS[name]
    ds = make().device_scene(0)
    tile = Tile(0, size, 0, size)
    npix, n = size * size, size * size * spp
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    with torch.cuda.stream(stream):
        o = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        d = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        ids = torch.zeros(n, dtype=torch.int64, device="cuda")
        ph = torch.zeros(n * 2, dtype=torch.float64, device="cuda")
        info = torch.zeros(n * 2, dtype=torch.int32, device="cuda")
        staged = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        direct = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    camera_rays_device(ds, tile, size, size, spp, SEED, 0, o.data_ptr(), d.data_ptr(), ids.data_ptr(), sp)
    stream.synchronize()

    def integrate(with_info):
        integrate_rays_device(ds, n, o.data_ptr(), d.data_ptr(), ph.data_ptr(), SEED, stream_ids_ptr=ids.data_ptr(),
                              info_ptr=info.data_ptr() if with_info else None, first_draw=2, stream_ptr=sp)

    times = {"integrate_info": [], "integrate": [], "render": [], "render_reduce": []}
    for r in range(warmup + rounds):
        events = []
        for leg in ("integrate_info", "integrate"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            integrate(leg == "integrate_info")
            e1.record(stream)
            events.append((leg, e0, e1))
        st = render_tile_device(ds, tile, size, size, spp, SEED, 0, direct.data_ptr(), sp, timed=True)
        stream.synchronize()
        if r >= warmup:
            for leg, e0, e1 in events:
                times[leg].append(e0.elapsed_time(e1))
            times["render"].append(st["kernel_ms"])
            times["render_reduce"].append(st["reduce_ms"])
    accumulate_photons_device(staged.data_ptr(), ph.data_ptr(), npix, spp, stream_ptr=sp)
    stream.synchronize()
    stream_check_error(ds, sp)
    hit = float((info.view(n, 2)[:, 1] & 1).double().mean())
    bounces = float(info.view(n, 2)[:, 0].double().mean())
    out = {"size": size, "spp": spp, "samples": n, "hit_fraction": round(hit, 4), "mean_bounces": round(bounces, 3),
           "max_bounces": int(info.view(n, 2)[:, 0].max()),
           "pipeline_equals_render": bool(torch.equal(staged.view(torch.int64), direct.view(torch.int64))), "legs": {}}
    for leg, t in times.items():
        med, best = statistics.median(t), min(t)
        out["legs"][leg] = {"ms_median": round(med, 4), "ms_min": round(best, 4),
                            "msamples_per_s_median": round(n / med * 1e-3, 1)}
    out["integrate_over_render"] = round(statistics.median(times["integrate"]) / statistics.median(times["render"]), 3)
    out["integrate_info_over_render"] = round(
        statistics.median(times["integrate_info"]) / statistics.median(times["render"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="c3,c1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("integrate_bench needs a GPU: no timing is taken without one")
    result = {"tool": "integrate_bench", "rounds": a.rounds, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "configs": {}}
    for name in a.configs.split(","):
        result["configs"][name] = run(name, a.rounds, a.warmup)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not all(c["pipeline_equals_render"] for c in result["configs"].values()):
        sys.exit("the staged pipeline's records differ from the render's")


if __name__ == "__main__":
    main()
