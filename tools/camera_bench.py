"""A posed camera in the render kernel against the staged pipeline it replaces.

    python tools/camera_bench.py [--rounds 5] [--warmup 2] [--size 1024] [--spp 16] [--out FILE]

C3's scene (main.rs), 1024 x 1024 at 16 spp by default.  Legs, alternating inside each round (one process,
one device, one stream), after warm-up rounds:
  default  vr_render_tile_device under the default pose, timed: render kernel and ordered reduce apart;
  posed    the same under a look_at pose: the scene's camera carried 40 degrees round the vertical axis
           through the mesh, turned to keep the mesh in view;
  staged   the posed view as a caller had to build it before poses: vr_camera_rays_device +
           vr_integrate_rays_device + vr_accumulate_photons_device, HIP events around the three.
  lens     the default pose with a thin lens (radius 0.05, focused on the mesh's centre): the render kernel's
           lens instantiations; the default leg is the pinhole of the same view;
  lens_staged  that view through the staged pipeline (first_draw = 4: the lens spends draws 2 and 3).
Median and best per leg, staged / posed, lens_staged / lens, lens / default, the counters of one untimed counting launch per view (hit rate and
culled share move with the view), and checks that the staged records equal the posed render's and the lens
render's bit for bit.
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
from vanrijn_amd.scene import CameraLens, CameraPose, DeviceScene, look_at  # noqa: E402

SEED = 0x5EED0001
MESH_CENTRE = (-1.7, -0.8, 0.0)  # scenes.procedural_bunny
ORBIT_DEGREES = 40.0
LENS_RADIUS = 0.05


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
    default, posed, lensed = DeviceScene(spec, 0), DeviceScene(spec, 0), DeviceScene(spec, 0)
    pose = orbit_pose(spec.camera_location, ORBIT_DEGREES)
    posed.set_camera_pose(pose)
    lens = CameraLens(LENS_RADIUS, math.dist(spec.camera_location, MESH_CENTRE))
    lensed.set_camera_lens(lens)
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
        lens_staged = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        lens_direct = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
        other = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    stream.synchronize()
    times = {"default": [], "default_reduce": [], "posed": [], "posed_reduce": [], "staged": [], "lens": [],
             "lens_reduce": [], "lens_staged": []}

    def staged_pipeline(ds, first_draw, into):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        camera_rays_device(ds, tile, size, size, spp, SEED, 0, o.data_ptr(), d.data_ptr(), ids.data_ptr(), sp)
        integrate_rays_device(ds, n, o.data_ptr(), d.data_ptr(), ph.data_ptr(), SEED, stream_ids_ptr=ids.data_ptr(),
                              first_draw=first_draw, stream_ptr=sp)
        accumulate_photons_device(into.data_ptr(), ph.data_ptr(), npix, spp, stream_ptr=sp)
        e1.record(stream)
        return e0, e1

    for r in range(warmup + rounds):
        sd = render_tile_device(default, tile, size, size, spp, SEED, 0, other.data_ptr(), sp, timed=True)
        spo = render_tile_device(posed, tile, size, size, spp, SEED, 0, direct.data_ptr(), sp, timed=True)
        e0, e1 = staged_pipeline(posed, 2, staged)
        sl = render_tile_device(lensed, tile, size, size, spp, SEED, 0, lens_direct.data_ptr(), sp, timed=True)
        l0, l1 = staged_pipeline(lensed, 4, lens_staged)
        stream.synchronize()
        if r >= warmup:
            times["default"].append(sd["kernel_ms"])
            times["default_reduce"].append(sd["reduce_ms"])
            times["posed"].append(spo["kernel_ms"])
            times["posed_reduce"].append(spo["reduce_ms"])
            times["staged"].append(e0.elapsed_time(e1))
            times["lens"].append(sl["kernel_ms"])
            times["lens_reduce"].append(sl["reduce_ms"])
            times["lens_staged"].append(l0.elapsed_time(l1))
    stream_check_error(posed, sp)
    stream_check_error(lensed, sp)
    equal = bool(torch.equal(staged.view(torch.int64), direct.view(torch.int64)))
    lens_equal = bool(torch.equal(lens_staged.view(torch.int64), lens_direct.view(torch.int64)))
    out = {"size": size, "spp": spp, "samples": n, "orbit_degrees": ORBIT_DEGREES,
           "pose": {k: getattr(pose, k) for k in CameraPose.__dataclass_fields__},
           "staged_equals_posed_render": equal,
           "lens": {"lens_radius": lens.lens_radius, "focus_distance": lens.focus_distance},
           "staged_equals_lens_render": lens_equal, "legs": {},
           "counters": {"default": counters_of(default, tile, size, spp, other, sp),
                        "posed": counters_of(posed, tile, size, spp, other, sp),
                        "lens": counters_of(lensed, tile, size, spp, other, sp)}}
    stream.synchronize()
    for leg, t in times.items():
        out["legs"][leg] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4)}
    med = {leg: statistics.median(t) for leg, t in times.items()}
    out["staged_over_posed"] = round(med["staged"] / (med["posed"] + med["posed_reduce"]), 3)
    out["posed_over_default"] = round(med["posed"] / med["default"], 3)
    out["lens_staged_over_lens"] = round(med["lens_staged"] / (med["lens"] + med["lens_reduce"]), 3)
    out["lens_over_default"] = round(med["lens"] / med["default"], 3)
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
    if not result["staged_equals_lens_render"]:
        sys.exit("the staged pipeline's records differ from the lens render's")


if __name__ == "__main__":
    main()
