"""What per-triangle materials save against cutting a model into one mesh per material, and what the
set call costs.

    python tools/materials_bench.py [--mesh FILE.obj] [--size 1024] [--spp 64] [--reps 3]
                                    [--ks 1,2,4,8,16,32] [--out profiles/r12/materials/materials_bench.json]

C3's scene (main.rs's plane and spheres around the stand-in bunny, or --mesh) with K materials of
identical parameters on the mesh, assigned to its triangles in two ways: by spatial slab along x (what a
model's parts look like) and at random (the worst case for a split: every piece spans the whole model).
Each assignment is rendered the split way -- K meshes, K BVH objects, the multi-BVH walk -- and the merged
way -- one mesh, one tree, vr_scene_set_mesh_materials -- with VR_LAUNCH_TIMED, the two legs alternating;
one JSON line per (assignment, K) with both legs' kernel times and whether the two state buffers agree bit
for bit (identical materials, so they render the same image unless two triangles tie exactly).
Then the set call on C5's 1,051,392-triangle mesh: the first call (plan included) and the steady-state
host and device forms, wall time around the blocking call.
Nothing here is asserted by the test suite.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from vanrijn_amd import scenes  # noqa: E402
from vanrijn_amd.render import Tile, render_tile_device  # noqa: E402
from vanrijn_amd.scene import (BoundingVolumeHierarchy, ColourRgbF, DeviceScene, LambertianMaterial, Mesh,  # noqa: E402
                               NamedColour, Scene, Spectrum, load_obj)

SEED = 0x5EED0001


def material():
    return LambertianMaterial(Spectrum.reflection_from_linear_rgb(ColourRgbF.from_named(NamedColour.Yellow)), 0.05)


def assignments(v, k):
    """ids [n] in [0, k): equal-count slabs along x by triangle centroid, and uniformly at random."""
    x = v[:, :, 0].mean(axis=1)
    slab = np.empty(len(v), dtype=np.uint32)
    slab[np.argsort(x, kind="stable")] = (np.arange(len(v)) * k // len(v)).astype(np.uint32)
    rand = np.random.default_rng(k).integers(0, k, size=len(v)).astype(np.uint32)
    return {"slab_x": slab, "random": rand}


def scene_pair(v, n, ids, k):
    """(split, merged) DeviceScenes of main.rs's primitives around the mesh."""
    prims = scenes.main_scene((v[:1], n[:1])).objects[0]
    mats = [material() for _ in range(k)]
    split = Scene(scenes.CAMERA_LOCATION, [prims] + [BoundingVolumeHierarchy.build(
        Mesh(np.ascontiguousarray(v[ids == m]), np.ascontiguousarray(n[ids == m]), mats[m])) for m in range(k)
        if (ids == m).any()])
    merged = Scene(scenes.CAMERA_LOCATION, [prims, BoundingVolumeHierarchy.build(
        Mesh(v, n, mats[0], triangle_materials=(mats, ids)))])
    return DeviceScene(split.spec(), 0, device_sah=True), DeviceScene(merged.spec(), 0, device_sah=True)


def render_legs(legs, size, spp, reps):
    """Kernel times of the legs' scenes, alternating, after one warm-up each; their variants and states."""
    t = Tile(0, size, 0, size)
    out = {name: {"ms": []} for name in legs}
    state = {name: torch.zeros(size * size * 8, dtype=torch.float64, device="cuda") for name in legs}
    for rep in range(reps + 1):
        for name, ds in legs.items():
            r = render_tile_device(ds, t, size, size, spp, SEED, 0, state[name].data_ptr(), timed=True)
            torch.cuda.synchronize()
            if rep:
                out[name]["ms"].append(round(r["kernel_ms"], 3))
            out[name]["variant"] = r["variant"]
    for name in legs:
        out[name]["ms_median"] = round(statistics.median(out[name]["ms"]), 3)
    return out, state


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def set_call_c5(calls):
    v, n = scenes.synthetic_sphere_mesh()
    v, n = np.ascontiguousarray(v), np.ascontiguousarray(n)
    sc = scenes.main_scene((v, n))
    spec = sc.spec()
    ds = DeviceScene(spec, 0, device_sah=True)
    ids = np.random.default_rng(1).integers(0, len(spec.materials), size=len(v)).astype(np.uint32)
    before = ds.info()["device_bytes"]
    out = {"figure": "set_mesh_materials", "mesh": "c5", "triangles": len(v),
           "first_call_ms": round(timed(lambda: ds.set_mesh_materials(0, ids)), 3),
           "plan_and_stage_bytes": ds.info()["device_bytes"] - before}
    dev = torch.from_numpy(ids.astype(np.int32)).cuda()
    stream = torch.cuda.Stream()
    forms = {"host": lambda: ds.set_mesh_materials(0, ids),
             "device": lambda: ds.set_mesh_materials_device(0, dev.data_ptr(), stream.cuda_stream),
             "reset": lambda: ds.set_mesh_materials(0, None)}
    for name, fn in forms.items():
        fn()
        t = [timed(fn) for _ in range(calls)]
        out[name] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "calls": calls}
    ds.set_mesh_materials(0, ids)
    assert np.array_equal(ds.mesh_materials(0), ids)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", default=None, help="an OBJ file instead of C3's stand-in mesh")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--set-calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "materials", "materials_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("materials_bench needs a GPU: no timing is taken without one")
    if a.mesh:
        m = load_obj(a.mesh, None)
        v, n = m.vertices, m.normals
    else:
        v, n = scenes.procedural_bunny()
    v, n = np.ascontiguousarray(v), np.ascontiguousarray(n)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    gpu = torch.cuda.get_device_name(0)
    with open(a.out, "w") as f:
        def emit(row):
            line = json.dumps({"tool": "materials_bench", "gpu": gpu, **row})
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for k in (int(x) for x in a.ks.split(",")):
            for how, ids in assignments(v, k).items():
                split, merged = scene_pair(v, n, ids, k)
                res, state = render_legs({"split": split, "merged": merged}, a.size, a.spp, a.reps)
                emit({"figure": "split_vs_merged", "assignment": how, "k": k, "triangles": len(v), "size": a.size,
                      "spp": a.spp, "split": res["split"], "merged": res["merged"],
                      "split_over_merged": round(res["split"]["ms_median"] / res["merged"]["ms_median"], 4),
                      "split_wide_nodes": split.info()["wide_node_count"],
                      "merged_wide_nodes": merged.info()["wide_node_count"],
                      "states_equal": bool(torch.equal(state["split"].view(torch.int64),
                                                       state["merged"].view(torch.int64)))})
                split.release()
                merged.release()
        emit(set_call_c5(a.set_calls))


if __name__ == "__main__":
    main()
