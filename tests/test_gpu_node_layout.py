"""The 4-wide node's per-axis layout (vr_layout.h Node4: six quads of bounds, read in the ray's
order by the node step, coop_step and lone_walk) at the smallest shapes where the layout or its
addressing can go wrong, on the GPU against the oracle and across the kernel instantiations.

* Tiny trees: meshes of 1 to 17 triangles (a leaf root; a root node with 2, 3 and 4 live slots and
  NaN slots beside them; a second level) and a flat mesh (every triangle in y = 0: zero-thickness
  boxes), each in a corner of Lambertian and mirror planes (floor, mirror side, back
  wall), so bounce rays come back at the mesh in all eight direction octants.  Per-sample decisions equal the oracle's reference
  mode, with the distance culling off and on, for the host-built (WideBuilder), reference-order and
  device-built (fill_wide_kernel) trees.
* Instantiations: one ~3,000-triangle mirror mesh; the device records of the cooperative-tail
  kernel with whole walks (lone_walk) and without (coop_step only), the plain kernel with 16-bit
  and 32-bit stacks and the 64-bit-offset kernel are equal bit for bit, and every launch reports
  the instantiation that ran.
"""
import numpy as np
import pytest
import torch

from vanrijn_amd import _native as N
from vanrijn_amd.render import Tile, render_samples, render_tile_device
from vanrijn_amd.scene import (BoundingVolumeHierarchy, DeviceScene, LambertianMaterial, Mesh, Plane, ReflectiveMaterial,
                               Scene, Spectrum)

from test_gpu_ties import INTENSITY_REL_TOL

pytestmark = pytest.mark.gpu

CAMERA = (0.3, 1.7, -5.0)  # looks along +z, from above the y = 0 plane (the flat mesh is not edge-on)
H, W, SPP, SEED = 40, 48, 3, 0x5EED0007


def tiny_mesh(kind):
    """n large triangles around (0, 1, 0) in front of the camera, or 12 triangles in the plane y = 0"""
    if kind == "flat":
        rng = np.random.default_rng(40)
        v = np.empty((12, 3, 3))
        v[..., 0] = rng.normal(0.0, 2.0, (12, 3))
        v[..., 1] = 0.0
        v[:4, :, 1] = -0.0
        v[..., 2] = rng.uniform(-2.0, 5.0, (12, 3))
        return v
    if kind == 1:  # (a leaf root: no wide node at all)
        return np.array([[[-3.0, -1.0, 0.5], [3.0, -0.5, 1.0], [0.2, 4.0, 0.0]]])
    rng = np.random.default_rng(100 + kind)
    v = rng.normal(0.0, 1.6, (kind, 3, 3)) + np.array([0.0, 1.0, 0.5])
    v[..., 2] *= 0.5  # facing the camera rather than edge-on
    return v


def _mesh(v, material):
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3, 3)
    n = np.zeros_like(v)
    n[..., 2] = -1.0
    return BoundingVolumeHierarchy.build(Mesh(v, n, material))


def enclosed_scene(v):
    grey = LambertianMaterial(Spectrum.grey(0.6), 0.4)
    mirror = ReflectiveMaterial(Spectrum.grey(0.8), 0.05, 0.9)
    # a floor, a mirror side and a back wall (infinite planes: a closed box would trap every path for
    # the full 128 bounces): camera rays cover +z with either sign of x and y, floor bounces +y with
    # either sign of x and z, back-wall bounces -z with either sign of x and y -- all eight octants --
    # and the mirror flips x; paths that leave upward, sideways or backward end at any bounce count
    walls = [
        Plane((0.0, 1.0, 0.0), -2.0, grey),    # floor
        Plane((1.0, 0.0, 0.0), 5.0, mirror),   # side
        Plane((0.0, 0.0, 1.0), 6.0, grey),     # behind the mesh
    ]
    return Scene(CAMERA, [walls, _mesh(v, LambertianMaterial(Spectrum.grey(0.3), 0.9))])


def _decisions_equal(gpu, ref):
    assert np.array_equal(gpu["flags"], ref["flags"])
    assert np.array_equal(gpu["bounces"], ref["bounces"])
    assert np.array_equal(gpu["wavelength"], ref["wavelength"])
    den = np.maximum(np.abs(ref["intensity"]), 1e-300)
    rel = np.abs(gpu["intensity"] - ref["intensity"]) / den
    ok = (ref["intensity"] == 0) | (rel < INTENSITY_REL_TOL) | (np.isnan(ref["intensity"]) & np.isnan(gpu["intensity"]))
    assert ok.all()


@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5, 17, "flat"])
def test_tiny_trees_match_the_oracle(kind, oracle):
    v = tiny_mesh(kind)
    scene = enclosed_scene(v)
    t = Tile(0, W, 0, H)
    # the oracle alone: camera rays that hit the mesh (rendered without the enclosure, the same rays)
    alone = oracle.OracleScene(Scene(CAMERA, [_mesh(v, LambertianMaterial(Spectrum.grey(0.5), 0.5))]).spec())
    hits = alone.render_samples(t, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)["flags"] & 1
    assert hits.sum() > 500
    ref = oracle.OracleScene(scene.spec()).render_samples(t, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE,
                                                          nthreads=8)
    assert (ref["bounces"] >= 2).sum() > 500  # paths come back from the planes
    for kw in ({}, {"reference_bvh": True}, {"device_sah": True}):
        for no_dist_cull in (True, False):
            ds = DeviceScene(scene.spec(), 0, **kw)
            ds.set_launch_flags(no_dist_cull=no_dist_cull)
            _decisions_equal(render_samples(ds, t, H, W, SPP, seed=SEED), ref)


def test_instantiations_are_bit_identical():
    rng = np.random.default_rng(23)
    v = rng.normal(size=(3001, 3, 3))
    mirror = ReflectiveMaterial(Spectrum.grey(0.8), 0.05, 0.9)
    scene = Scene((0.0, 0.0, -5.0), [_mesh(v, mirror)])
    S = 64
    t = Tile(0, S, 0, S)
    stream = torch.cuda.current_stream().cuda_stream
    COOP, WIDE, S16 = N.VARIANT_COOP, N.VARIANT_WIDE_OFFSETS, N.VARIANT_STACK16
    runs = [  # scene options, launch options, the variant bits the launch must report
        ({}, {}, COOP),                                        # the default: the cooperative tail, whole walks
        ({}, {"lone_walk": False}, COOP),                      # coop_step only
        ({}, {"coop": False}, S16),                            # the plain kernel, 16-bit stack entries
        ({}, {"coop": False, "stack16": False}, 0),            # 32-bit stack entries
        ({"wide_offsets": True}, {}, WIDE),                    # 64-bit node addresses plus the per-lane offset
    ]
    out = []
    for skw, lkw, bits in runs:
        ds = DeviceScene(scene.spec(), 0, **skw)
        st = torch.zeros(S * S * 8, dtype=torch.float64, device="cuda")
        s = render_tile_device(ds, t, S, S, 6, SEED, 0, st.data_ptr(), stream, **lkw)
        torch.cuda.synchronize()
        assert s["variant"] & (COOP | WIDE | S16) == bits, (skw, lkw, s["variant"])
        out.append(st.cpu())
    assert (out[0][: S * S * 4].view(-1, 4)[:, 3] > 0).all()  # every pixel's weight sum: the records were written
    for o in out[1:]:
        assert torch.equal(out[0].view(torch.int64), o.view(torch.int64))  # bitwise, NaN included
