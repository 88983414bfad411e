"""A posed camera in the render kernel against the staged pipeline it replaces.

    python tools/camera_bench.py [--rounds 5] [--warmup 2] [--size 1024] [--spp 16] [--out FILE]

C3's scene (main.rs), 1024 x 1024 at 16 spp by default.  Legs, alternating inside each round (one process,
one device, one stream), after warm-up rounds:
  default  vr_render_tile_device under the default pose, timed: render kernel and ordered reduce apart;
  posed    the same under a look_at pose: the scene's camera carried 40 degrees round the vertical axis
           through the mesh, turned to keep the mesh in view;
  staged   the posed view as a caller had to build it before poses: vr_camera_rays_device +
           vr_integrate_rays_device + vr_accumulate_photons_device, HIP events around the three.
Median and best per leg, staged / posed, the counters of one untimed counting launch per view (hit rate and
culled share move with the view), and a check that the staged records equal the posed render's bit for bit.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vanrijn_amd import scenes  # noqa: E402
from vanrijn_amd.render import (Tile, accumulate_photons_device, camera_rays_device, integrate_rays_device,  # noqa: E402
                                render_tile_device, stream_check_error)
from vanrijn_amd.scene import CameraPose, DeviceScene, look_at  # noqa: E402

SEED = 0x5EED0001
MESH_CENTRE = (-1.7, -0.8, 0.0)  # scenes.procedural_bunny
ORBIT_DEGREES = 40.0


def orbit_pose(camera, degrees):
    """The camera carried `degrees` round the vertical axis through the mesh, looking at the mesh."""
    a = math.radians(degrees)
    dx, dz = camera[0] - MESH_CENTRE[0], camera[2] - MESH_CENTRE[2]
    eye = (MESH_CENTRE[0] + math.cos(a) * dx + math.sin(a) * dz, camera[1], MESH_CENTRE[2] - math.sin(a) * dx + math.cos(a) * dz)
    return look_at(eye, MESH_CENTRE, (0.0, 1.0, 0.0), 1.0)


def counters_of(ds, tile, size, spp, state, sp):
    c = render_tile_device(ds, tile, size, size, spp, SEED, 0, state.data_ptr(), sp, counters=True)
    total = size * size * spp
    return {"samples_traced": c["samples"], "culled_share": round(1.0 - c["samples"] / total, 4),
            "rays": c["rays"], "rays_per_sample": round(c["rays"] / total, 3), "node_visits": c["node_visits"],
            "triangle_tests": c["triangle_tests"], "shaded_triangle_hits": c["shaded_triangle_hits"]}


def run(size, spp, rounds, warmup):
    spec = scenes.main_scene().spec()
    default, posed = DeviceScene(spec, 0), DeviceScene(spec, 0)
    pose = orbit_pose(spec.camera_location, ORBIT_DEGREES)
    posed.set_camera_pose(pose)
    tile = Tile(0, size, 0, size)
    npix, n = size * size, size * size * spp
    stream = torch.cuda.Stream()
    sp = stream.cuda_stream
    with torch.cuda.stream(stream):
        o = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        d = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        ids = torch.zeros(n, dtype=torch.int64, device="cuda")
        ph = torch.zeros(n * 2, dtype=torch.float64, device="cuda")
        staged = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        direct = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        other = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    stream.synchronize()
    times = {"default": [], "default_reduce": [], "posed": [], "posed_reduce": [], "staged": []}
    for r in range(warmup + rounds):
        sd = render_tile_device(default, tile, size, size, spp, SEED, 0, other.data_ptr(), sp, timed=True)
        spo = render_tile_device(posed, tile, size, size, spp, SEED, 0, direct.data_ptr(), sp, timed=True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        camera_rays_device(posed, tile, size, size, spp, SEED, 0, o.data_ptr(), d.data_ptr(), ids.data_ptr(), sp)
        integrate_rays_device(posed, n, o.data_ptr(), d.data_ptr(), ph.data_ptr(), SEED, stream_ids_ptr=ids.data_ptr(),
                              first_draw=2, stream_ptr=sp)
        accumulate_photons_device(staged.data_ptr(), ph.data_ptr(), npix, spp, stream_ptr=sp)
        e1.record(stream)
        stream.synchronize()
        if r >= warmup:
            times["default"].append(sd["kernel_ms"])
            times["default_reduce"].append(sd["reduce_ms"])
            times["posed"].append(spo["kernel_ms"])
            times["posed_reduce"].append(spo["reduce_ms"])
            times["staged"].append(e0.elapsed_time(e1))
    stream_check_error(posed, sp)
    equal = bool(torch.equal(staged.view(torch.int64), direct.view(torch.int64)))
    out = {"size": size, "spp": spp, "samples": n, "orbit_degrees": ORBIT_DEGREES,
           "pose": {k: getattr(pose, k) for k in CameraPose.__dataclass_fields__},
           "staged_equals_posed_render": equal, "legs": {},
           "counters": {"default": counters_of(default, tile, size, spp, other, sp),
                        "posed": counters_of(posed, tile, size, spp, other, sp)}}
    stream.synchronize()
    for leg, t in times.items():
        out["legs"][leg] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4)}
    med = {leg: statistics.median(t) for leg, t in times.items()}
    out["staged_over_posed"] = round(med["staged"] / (med["posed"] + med["posed_reduce"]), 3)
    out["posed_over_default"] = round(med["posed"] / med["default"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("camera_bench needs a GPU: no timing is taken without one")
    result = {"tool": "camera_bench", "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "scene": "main_scene (C3)", **run(a.size, a.spp, a.rounds, a.warmup)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not result["staged_equals_posed_render"]:
        sys.exit("the staged pipeline's records differ from the posed render's")


if __name__ == "__main__":
    main()
