"""Ray-query throughput: the 4-wide walk against the binary f64 walk (VR_QUERY_REFERENCE_WALK).

    python tools/query_bench.py [--size 1024] [--rounds 10] [--warmup 2] [--out FILE]

Ray sets, both resident on the device as torch tensors:
  camera: the C3 scene's (main.rs scene, the stand-in bunny) camera rays through the pixel centres of
          a size x size image;
  bounce: from their hit points, hit point + 1e-7 d with a random unit d (the recipe of
          tests/test_gpu_parity.py test_trace_rays_from_surface_points).
Legs: closest and any, each on the 4-wide tree and on the binary tree.  Every leg is one launch of
vr_query_*_device timed with HIP events on one stream; the legs alternate inside each round (one
process, one device), after warm-up rounds; median and best Mrays/s per leg are reported, and the two
walks' outputs are compared byte for byte.  Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vanrijn_amd import scenes  # noqa: E402
from vanrijn_amd.render import query_any_device, query_closest_device  # noqa: E402


def camera_rays(camera, size):
    """camera.rs:24-66 at the pixel centres (u = v = 0.5) of a square image, Ray::new's normalisation."""
    i = torch.arange(size, dtype=torch.float64, device="cuda")
    x = (i + 0.5) * (1.0 / size) - 0.5                 # by column
    y = ((size - (i + 1.0)) + 0.5) * (1.0 / size) - 0.5  # by row
    d = torch.stack([x[None, :].expand(size, size), y[:, None].expand(size, size),
                     torch.ones(size, size, dtype=torch.float64, device="cuda")], dim=2).reshape(-1, 3)
    d = d * (1.0 / torch.sqrt((d * d).sum(dim=1, keepdim=True)))
    o = torch.tensor(camera, dtype=torch.float64, device="cuda").expand(len(d), 3).contiguous()
    return o, d.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("query_bench needs a GPU: no timing is taken without one")
    scene = scenes.main_scene()
    ds = scene.device_scene(0)
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    with torch.cuda.stream(stream):
        co, cd = camera_rays(scene.spec().camera_location, a.size)
        n = len(co)
        rec = torch.zeros(n * 18, dtype=torch.float64, device="cuda")  # vr_hit_record: 144 B
        hits = torch.zeros(n * 4, dtype=torch.int64, device="cuda")    # vr_ray_hit: 32 B
        query_closest_device(ds, n, co.data_ptr(), cd.data_ptr(), hits.data_ptr(), rec.data_ptr(), stream_ptr=sp)
        valid = hits.view(n, 4)[:, 2] >> 32 != 0                       # {object, valid} share a word
        loc = rec.view(n, 18)[:, 3:6][valid]
        g = torch.Generator(device="cuda")
        g.manual_seed(3)
        bd = torch.randn(loc.shape, dtype=torch.float64, device="cuda", generator=g)
        bd = (bd * (1.0 / torch.sqrt((bd * bd).sum(dim=1, keepdim=True)))).contiguous()
        bo = (loc + bd * 1e-7).contiguous()
    stream.synchronize()
    sets = {"camera": (co, cd), "bounce": (bo, bd)}
    legs = [(kind, walk) for kind in ("closest", "any") for walk in ("wide", "binary")]
    out = {}
    for name, (o, d) in sets.items():
        m = len(o)
        out[(name, "closest")] = {w: torch.empty(m * 4, dtype=torch.int64, device="cuda") for w in ("wide", "binary")}
        out[(name, "any")] = {w: torch.empty(m, dtype=torch.uint8, device="cuda") for w in ("wide", "binary")}

    def launch(name, kind, walk):
        o, d = sets[name]
        dst = out[(name, kind)][walk]
        if kind == "closest":
            query_closest_device(ds, len(o), o.data_ptr(), d.data_ptr(), dst.data_ptr(), None, stream_ptr=sp,
                                 reference_walk=walk == "binary")
        else:
            query_any_device(ds, len(o), o.data_ptr(), d.data_ptr(), dst.data_ptr(), stream_ptr=sp,
                             reference_walk=walk == "binary")

    times = {(name, kind, walk): [] for name in sets for kind, walk in legs}
    for r in range(a.warmup + a.rounds):
        events = []
        for name in sets:
            for kind, walk in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch(name, kind, walk)
                e1.record(stream)
                events.append(((name, kind, walk), e0, e1))
        stream.synchronize()
        if r >= a.warmup:
            for key, e0, e1 in events:
                times[key].append(e0.elapsed_time(e1))
    result = {"tool": "query_bench", "size": a.size, "rounds": a.rounds, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "rays": {k: len(v[0]) for k, v in sets.items()},
              "hit_fraction": {}, "walks_equal": True, "legs": {}}
    for name in sets:
        m = len(sets[name][0])
        for kind in ("closest", "any"):
            same = bool(torch.equal(out[(name, kind)]["wide"], out[(name, kind)]["binary"]))
            result["walks_equal"] = result["walks_equal"] and same
            for walk in ("wide", "binary"):
                t = times[(name, kind, walk)]
                med, best = statistics.median(t), min(t)
                result["legs"][f"{name}_{kind}_{walk}"] = {
                    "ms_median": round(med, 4), "ms_min": round(best, 4),
                    "mrays_per_s_median": round(m / med * 1e-3, 1), "mrays_per_s_best": round(m / best * 1e-3, 1)}
            w, b = (statistics.median(times[(name, kind, x)]) for x in ("wide", "binary"))
            result["legs"][f"{name}_{kind}_speedup_wide_over_binary"] = round(b / w, 3)
        result["hit_fraction"][name] = round(float(out[(name, "any")]["wide"].float().mean()), 4)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not result["walks_equal"]:
        sys.exit("the two walks' outputs differ")


if __name__ == "__main__":
    main()
