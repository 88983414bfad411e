"""Which launches run the single-BVH instantiation of the render kernel (VR_VARIANT_ONE_BVH), on the host.

The choice is one function of the library (vr_host.cpp takes_one_bvh, exported as vr_launch_takes_one_bvh):
exactly one BVH whose 4-wide root is a node, none of the kernels that have no such instantiation selected
(counting, record, Whitted, 64-bit offsets, a launch small enough for the cooperative tail, or the generic
kernel asked for with VR_LAUNCH_MULTI_BVH), and a stack class the instantiation exists in.
vr_scene_launch_variant gives what a launch of a scene would report, with nothing launched, so host-only
scenes answer it: the scene descriptions below go through the same code as a launch.
"""
import numpy as np
import pytest

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.scene import (BoundingVolumeHierarchy, DeviceScene, LambertianMaterial, Mesh, Plane, Scene, Spectrum)

INT32_MIN = -(2 ** 31)
ONE, S16, COOP, WIDE = N.VARIANT_ONE_BVH, N.VARIANT_STACK16, N.VARIANT_COOP, N.VARIANT_WIDE_OFFSETS
SMALL = 64 * 64 * 4           # a launch small enough for the cooperative tail (at most 4 M pixel-samples)
FRAME = 1024 * 1024 * 256     # C3's


def _takes(bvh_count, root4, other=0, stack=27, s16=True):
    return bool(N.lib().vr_launch_takes_one_bvh(bvh_count, root4, other, stack, int(s16)))


def test_the_choice_function():
    # main.rs and benches/simple_scene.rs: one 69,312-triangle mesh, 27 stack entries, 16-bit entries;
    # C5: one 1.05 M-triangle mesh, 31 entries, 413 K wide nodes (32-bit entries)
    assert _takes(1, 0, stack=27, s16=True)
    assert _takes(1, 0, stack=31, s16=False)
    assert _takes(1, 5)  # (a root is any node index)
    # the BVH list
    assert not _takes(2, 0)
    assert not _takes(0, INT32_MIN)
    assert not _takes(1, -1)  # a one-triangle mesh: its root is the leaf link ~0
    assert not _takes(1, -7)
    assert not _takes(1, INT32_MIN)  # an empty mesh
    # what else the launch selected
    for other in (N.CHOICE_COUNTING, N.CHOICE_RECORD, N.CHOICE_WHITTED, N.CHOICE_COOP_GATED, N.CHOICE_WIDE_OFFSETS,
                  N.CHOICE_MULTI_BVH, N.CHOICE_COUNTING | N.CHOICE_WIDE_OFFSETS):
        assert not _takes(1, 0, other)
    # the stack classes the instantiation exists in: 16-bit entries 24 and 32, 32-bit entries 32
    assert _takes(1, 0, stack=8, s16=True) and _takes(1, 0, stack=24, s16=True) and _takes(1, 0, stack=32, s16=True)
    assert _takes(1, 0, stack=25, s16=False) and _takes(1, 0, stack=32, s16=False)
    assert not _takes(1, 0, stack=24, s16=False)
    assert not _takes(1, 0, stack=33, s16=False) and not _takes(1, 0, stack=48, s16=False)


@pytest.fixture(scope="module")
def main_ds():
    return DeviceScene(scenes.main_scene().spec(), 0, host_only=True)


@pytest.fixture(scope="module")
def bench_ds():
    return DeviceScene(scenes.bench_scene().spec(), 0, host_only=True)


def test_main_scene(main_ds):
    """Lambertian: never gated for the cooperative tail, so every timed launch takes it."""
    for n in (SMALL, FRAME):
        assert main_ds.launch_variant(n) == ONE | S16
        assert main_ds.launch_variant(n, N.LAUNCH_STACK32) == ONE
        assert main_ds.launch_variant(n, N.LAUNCH_MULTI_BVH) == S16
        assert main_ds.launch_variant(n, N.LAUNCH_NO_COOP) == ONE | S16
        assert main_ds.launch_variant(n, N.LAUNCH_COUNTERS) == 0
        assert main_ds.launch_variant(n, recording=True) == 0


def test_debug_launch_flags_reach_the_choice(main_ds):
    main_ds.set_launch_flags(multi_bvh=True)
    try:
        assert main_ds.launch_variant(FRAME) == S16
    finally:
        main_ds.set_launch_flags()
    assert main_ds.launch_variant(FRAME) == ONE | S16


def test_bench_scene_is_gated_by_size(bench_ds):
    """The reflective bench scene: launches of at most 4 M pixel-samples keep the kernels they had, with
    the cooperative tail or (VR_LAUNCH_NO_COOP) without it; larger ones take the single-BVH kernel."""
    assert bench_ds.launch_variant(SMALL) == COOP
    assert bench_ds.launch_variant(SMALL, N.LAUNCH_NO_COOP) == S16
    assert bench_ds.launch_variant(256 * 256 * 16) == COOP  # C1
    assert bench_ds.launch_variant(4 << 20) == COOP
    assert bench_ds.launch_variant((4 << 20) + 1) == ONE | S16
    assert bench_ds.launch_variant(1024 * 1024 * 32) == ONE | S16
    assert bench_ds.launch_variant(1024 * 1024 * 32, N.LAUNCH_MULTI_BVH) == S16


def test_whitted_and_wide_offsets():
    mesh = scenes.procedural_bunny(20)
    assert not DeviceScene(scenes.whitted_scene(mesh).spec(), 0, host_only=True).launch_variant(FRAME) & ONE
    wide = DeviceScene(scenes.main_scene(mesh).spec(), 0, host_only=True, wide_offsets=True)
    assert wide.launch_variant(FRAME) == WIDE
    assert DeviceScene(scenes.main_scene(mesh).spec(), 0, host_only=True).launch_variant(FRAME) == ONE | S16


def test_mesh_lists():
    g = np.random.default_rng(5)
    mat = LambertianMaterial(Spectrum.grey(0.6), 0.5)
    floor = [Plane((0.0, 1.0, 0.0), -1.5, mat)]

    def bvh(n):
        v = g.uniform(-1.0, 1.0, (n, 1, 3)) + g.normal(scale=0.2, size=(n, 3, 3))
        return BoundingVolumeHierarchy.build(Mesh(v, np.tile([0.0, 0.0, -1.0], (n, 3, 1)), mat))

    def variant(objects):
        return DeviceScene(Scene((0.0, 0.0, -4.0), objects).spec(), 0, host_only=True).launch_variant(FRAME)

    assert variant([floor, bvh(200)]) == ONE | S16
    assert variant([bvh(200), floor]) == ONE | S16
    assert not variant([floor, bvh(200), bvh(100)]) & ONE  # two meshes
    assert not variant([floor]) & ONE                      # no mesh
    assert not variant([floor, bvh(1)]) & ONE              # a one-triangle mesh: its root is a leaf
    assert variant([floor, bvh(2)]) & ONE                  # two triangles: one wide node
