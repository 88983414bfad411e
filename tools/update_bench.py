"""What vr_scene_update_mesh and the scene edits cost against vr_scene_create, and how far a refitted
tree degrades.

    python tools/update_bench.py [--meshes bunny,c5] [--updates 20] [--out-dir profiles/r10/edit]

Per mesh (the stand-in bunny, 69,312 triangles, and C5's 1,051,392-triangle mesh, each in main.rs's
scene of a plane and spheres), one JSON under --out-dir:
  create_*       wall time of vr_scene_create with the default flags and with VR_SCENE_DEVICE_SAH;
  first_update   the first update of the mesh: plan (links read back where the scene keeps no host copy,
                 level lists, upload) + refit; plan_bytes: what it adds to device_bytes;
  host / device  median and best wall time of --updates steady-state updates from host arrays and from
                 device arrays, the bytes each moves on the device (and over the bus for the host form),
                 the resulting GB/s beside the chip's measured copy rate, and the kernel launches;
  degradation    the render kernel's time for one 1024 x 1024 frame at 16 spp on the refitted tree and on
                 a freshly built tree of the same geometry, for no deformation, per-vertex noise of 1 % of
                 the mesh radius, and a twist of pi about the vertical axis -- with a check that both
                 render the same records;
  edits          the scene edits, in the same run: the mesh's first vr_scene_transform_mesh (base snapshot
                 included) and base_bytes, what it adds to device_bytes; median and best wall time of
                 --updates steady-state transforms (a rotation about the vertical axis through the mesh's
                 centre, a new absolute angle each time), to be read beside `device` above -- the
                 transform runs the update's launches plus two passes over resident records; and the
                 wall time of set_camera, update_primitives (3 spheres) and update_material.
Nothing here is asserted by the test suite; the comparison that matters is update against creation in
the same run.  Wall times are host clocks around blocking calls.
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
from vanrijn_amd.scene import DeviceScene  # noqa: E402

SEED = 0x5EED0001
COPY_RATE_GBS = 6290.0  # float4 copy on one MI355X, measured (79 % of the 8 TB/s HBM3E peak)
MESHES = {"bunny": scenes.procedural_bunny, "c5": scenes.synthetic_sphere_mesh}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def levels(child, roots):
    """Depth of the tree(s) below `roots` by child links: the launches of one tree's refit."""
    depth, frontier = 0, np.array([r for r in roots if r >= 0], dtype=np.int64)
    while len(frontier):
        depth += 1
        kids = child[frontier].reshape(-1)
        frontier = kids[kids >= 0]
    return depth


def deformations(v, n):
    centre = 0.5 * (v.reshape(-1, 3).min(axis=0) + v.reshape(-1, 3).max(axis=0))
    radius = float(np.linalg.norm(v.reshape(-1, 3) - centre, axis=1).max())
    g = np.random.default_rng(9)
    # per-vertex noise: the same offset for every copy of a shared vertex (keyed by its coordinates)
    flat = v.reshape(-1, 3)
    _, inverse = np.unique(flat, axis=0, return_inverse=True)
    offsets = g.normal(size=(inverse.max() + 1, 3)) * (0.01 * radius / np.sqrt(3.0))
    noisy = (flat + offsets[inverse.reshape(-1)]).reshape(v.shape)
    # twist of pi about the vertical (y) axis through the centre: the angle grows linearly with height
    rel = flat - centre
    y0, y1 = rel[:, 1].min(), rel[:, 1].max()
    a = np.pi * (rel[:, 1] - y0) / (y1 - y0)
    c, s = np.cos(a), np.sin(a)

    def rot(p):
        return np.stack([c * p[:, 0] + s * p[:, 2], p[:, 1], -s * p[:, 0] + c * p[:, 2]], axis=1)

    twisted = (rot(rel) + centre).reshape(v.shape)
    twisted_n = rot(n.reshape(-1, 3)).reshape(n.shape)
    return {"none": (v, n), "noise_1pct": (np.ascontiguousarray(noisy), n),
            "twist_pi": (np.ascontiguousarray(twisted), np.ascontiguousarray(twisted_n))}, radius


def frame_ms(ds, size=1024, spp=16, reps=2):
    st = torch.zeros(size * size * 8, dtype=torch.float64, device="cuda")
    t = []
    for _ in range(1 + reps):  # the first is the warm-up
        stats = render_tile_device(ds, Tile(0, size, 0, size), size, size, spp, SEED, 0, st.data_ptr(), timed=True)
        t.append(stats["kernel_ms"])
    return statistics.median(t[1:]), st


def run(name, updates):
    v, n = MESHES[name]()
    v, n = np.ascontiguousarray(v), np.ascontiguousarray(n)
    tris = len(v)
    spec = scenes.main_scene((v, n)).spec()
    out = {"mesh": name, "triangles": tris}
    ds, out["create_default_ms"] = timed(lambda: DeviceScene(spec, 0))
    sah, out["create_device_sah_ms"] = timed(lambda: DeviceScene(spec, 0, device_sah=True))
    info = ds.info()
    out["node_count"], out["wide_node_count"] = info["node_count"], info["wide_node_count"]
    roots = ds.bvh_roots()
    l2 = levels(ds.bvh_nodes()["child"], [int(roots["root"][0])])
    l4 = levels(ds.wide_nodes()["child"], [int(roots["root4"][0])])
    out["levels_binary"], out["levels_wide"] = l2, l4
    out["launches_per_update"] = 3 + l2 + l4  # validate, gather, one per level of each tree, root
    shapes, radius = deformations(v, n)
    out["mesh_radius"] = radius
    # bytes a refit moves on the device: the new arrays read twice (validate, gather: 144 B per
    # triangle each), the plan's index and the kept rank / padding quads read and both records written
    # by the gather (4 + 32 + 160 B), each triangle record read once per tree as a leaf child (80 B),
    # every node of both trees read once as a child and written once (128 B each) with its plan index
    nodes = info["node_count"] + info["wide_node_count"]
    dev_bytes = (2 * 144 + 4 + 32 + 160 + 2 * 80) * tris + (2 * 128 + 4) * nodes
    out["device_bytes_moved"] = dev_bytes
    out["host_form_bus_bytes"] = 144 * tris
    for label, scene in (("default", ds), ("device_sah", sah)):
        before = scene.info()["device_bytes"]
        _, ms = timed(lambda: scene.update_mesh(0, v, n))
        out[f"first_update_{label}_ms"] = ms
        out[f"plan_bytes_{label}"] = scene.info()["device_bytes"] - before
    tv, tn = torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda()
    stream = torch.cuda.Stream()
    legs = {"host": lambda: ds.update_mesh(0, v, n),
            "device": lambda: ds.update_mesh_device(0, tv.data_ptr(), tn.data_ptr(), stream.cuda_stream)}
    for leg, fn in legs.items():
        fn()
        t = [timed(fn)[1] for _ in range(updates)]
        med = statistics.median(t)
        out[leg] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "updates": updates,
                    "device_gb_per_s": round(dev_bytes / med * 1e-6, 1), "copy_rate_gb_per_s": COPY_RATE_GBS}
    # the one-time part of the first update: the plan (and, for the first scene, the kernels' first launch)
    for label in ("default", "device_sah"):
        out[f"plan_ms_{label}"] = round(out[f"first_update_{label}_ms"] - out["host"]["ms_median"], 3)
    out["update_over_create_default"] = round(out["device"]["ms_median"] / out["create_default_ms"], 5)
    out["update_over_create_device_sah"] = round(out["device"]["ms_median"] / out["create_device_sah_ms"], 5)
    out["degradation"] = {}
    for label, (dv, dn) in shapes.items():
        ds.update_mesh(0, dv, dn)
        refit_ms, refit_state = frame_ms(ds)
        fresh = DeviceScene(scenes.main_scene((dv, dn)).spec(), 0)
        fresh_ms, fresh_state = frame_ms(fresh)
        out["degradation"][label] = {
            "refitted_kernel_ms": round(refit_ms, 3), "fresh_kernel_ms": round(fresh_ms, 3),
            "ratio": round(refit_ms / fresh_ms, 4),
            "records_equal": bool(torch.equal(refit_state.view(torch.int64), fresh_state.view(torch.int64)))}
        fresh.release()
    out["edits"] = edits(ds, v, n, updates)
    return out


def edits(ds, v, n, updates):
    """The scene edits on the resident scene `ds` (main.rs's scene: a plane, three spheres, the mesh)."""
    ds.update_mesh(0, v, n)  # the base: the undeformed mesh
    flat = v.reshape(-1, 3)
    cx, _, cz = 0.5 * (flat.min(axis=0) + flat.max(axis=0))

    def turn(k):  # rotate by angle k / 10 about the vertical axis through the mesh's centre
        c, s = np.cos(0.1 * k), np.sin(0.1 * k)
        return [c, 0.0, s, cx - (c * cx + s * cz), 0.0, 1.0, 0.0, 0.0, -s, 0.0, c, cz - (-s * cx + c * cz)]

    def median_of(fn):
        fn(0)
        t = [timed(lambda: fn(k))[1] for k in range(1, updates + 1)]
        return {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "calls": updates}

    out = {}
    before = ds.info()["device_bytes"]
    _, out["first_transform_ms"] = timed(lambda: ds.transform_mesh(0, turn(1)))
    out["base_bytes"] = ds.info()["device_bytes"] - before
    out["transform"] = median_of(lambda k: ds.transform_mesh(0, turn(k)))
    cam = np.array(ds.camera())
    out["set_camera"] = median_of(lambda k: ds.set_camera(cam + [0.01 * k, 0.0, 0.0]))
    spheres = [p for p in ds.spec.objects[0].primitives if p.kind == 1][:3]
    first = ds.spec.objects[0].primitives.index(spheres[0])
    out["update_primitives_3_spheres"] = median_of(lambda k: ds.update_primitives(first, [
        type(p)(p.kind, p.material, (p.vector[0], p.vector[1] + 0.01 * k, p.vector[2]), p.scalar) for p in spheres]))
    mat = ds.spec.materials[ds.spec.meshes[0].material]
    out["update_material"] = median_of(lambda k: ds.update_material(
        ds.spec.meshes[0].material, type(mat)(mat.kind, mat.colour, 0.05 + 0.001 * k, mat.reflection_strength,
                                              mat.smoothness)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--meshes", default="bunny,c5")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--out-dir", default=os.path.join("profiles", "r10", "edit"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("update_bench needs a GPU: no timing is taken without one")
    os.makedirs(a.out_dir, exist_ok=True)
    for name in a.meshes.split(","):
        result = {"tool": "update_bench", "gpu": torch.cuda.get_device_name(0), **run(name, max(20, a.updates))}
        line = json.dumps(result)
        print(line, flush=True)
        with open(os.path.join(a.out_dir, f"{name}.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
