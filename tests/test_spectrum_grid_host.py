"""The host's proof that a scene's intensity rows lie on one wavelength grid (vr_host_scene.cpp grids_shared,
update_grid_shared; exported as vr_material_grids_shared and vr_scene_grid_shared).

A row's grid is what the device's intensity lookup reads beside the samples: shortest, longest, n, inv_step
and knots[0..n).  The single-BVH render kernels of one material kind find a path's segment and ratio on it
once per path, so they run only while every material row (and, in a Whitted scene, every light row) has the
same grid bit for bit (bit 0 of vr_scene_grid_shared); the sky row's lookup uses the path's pair when the sky
row lies on that grid too (bit 1) and keeps its own otherwise.  No GPU: host-only scenes.
"""
import numpy as np
import pytest

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.scene import ColourRgbF, DeviceScene, DirectionalLight, MaterialSpec, Spectrum, WhittedIntegrator

ONE, S16 = N.VARIANT_ONE_BVH, N.VARIANT_STACK16
FRAME = 1024 * 1024 * 256
MESH = scenes.procedural_bunny(12)


def _rgb(r, g, b):
    return Spectrum.reflection_from_linear_rgb(ColourRgbF.new(r, g, b))


def _coarse(sp, n=16):
    """`sp` resampled on a grid of `n` knots over the same range"""
    x = np.linspace(sp.shortest_wavelength, sp.longest_wavelength, n)
    xp = np.linspace(sp.shortest_wavelength, sp.longest_wavelength, sp.samples.size)
    return Spectrum(sp.shortest_wavelength, sp.longest_wavelength, np.interp(x, xp, sp.samples))


def _flip(rows, row, field, index=None, bit=0):
    """a copy of `rows` with one bit of one field of one row inverted"""
    out = rows.copy()
    word = out[field][row:row + 1] if index is None else out[field][row][index:index + 1]
    raw = word.view(np.uint32 if word.dtype.itemsize == 4 else np.uint64)
    raw ^= raw.dtype.type(1) << raw.dtype.type(bit)
    return out


@pytest.fixture(scope="module")
def main_ds():
    return DeviceScene(scenes.main_scene(MESH).spec(), 0, host_only=True)


def test_equal_grids_pass(main_ds):
    rows = main_ds.materials()
    assert len(rows) == 6 and (rows["n"] == 32).all()  # five materials and the sky row, the last
    assert DeviceScene.grids_shared(rows)
    assert DeviceScene.grids_shared(rows[:1]) and DeviceScene.grids_shared(rows[-1:])
    assert main_ds.grid_shared() == 3


@pytest.mark.parametrize("row", [0, 3, 5], ids=["first-material", "a-material", "sky"])
def test_one_differing_bit_fails(main_ds, row):
    rows = main_ds.materials()
    n = int(rows["n"][row])
    for bit in (0, 51, 63):
        for k in (0, 1, n - 1):
            assert not DeviceScene.grids_shared(_flip(rows, row, "knots", k, bit)), (k, bit)
        assert not DeviceScene.grids_shared(_flip(rows, row, "inv_step", bit=bit))
        assert not DeviceScene.grids_shared(_flip(rows, row, "shortest", bit=bit))
        assert not DeviceScene.grids_shared(_flip(rows, row, "longest", bit=bit))
    for bit in (0, 1, 5):
        assert not DeviceScene.grids_shared(_flip(rows, row, "n", bit=bit))
    # what is not the grid: the samples, the strengths, and the knots past n
    assert DeviceScene.grids_shared(_flip(rows, row, "samples", 3, 40))
    assert DeviceScene.grids_shared(_flip(rows, row, "diffuse", bit=40))
    assert DeviceScene.grids_shared(_flip(rows, row, "knots", n, 40))
    assert DeviceScene.grids_shared(_flip(rows, row, "knots", 63, 40))


def test_a_material_on_another_grid_and_its_edits():
    """One material of main.rs's scene on 16 knots: no single-BVH kernel; edited back it returns, edited away
    it leaves again."""
    spec = scenes.main_scene(MESH).spec()
    fine = spec.materials[1]
    coarse = MaterialSpec(fine.kind, _coarse(fine.colour), fine.diffuse_strength)
    spec.materials[1] = coarse
    ds = DeviceScene(spec, 0, host_only=True)
    rows = ds.materials()
    assert rows["n"].tolist() == [32, 16, 32, 32, 32, 32] and not DeviceScene.grids_shared(rows)
    assert ds.grid_shared() == 0 and ds.launch_variant(FRAME) == S16
    ds.update_material(1, fine)
    assert ds.grid_shared() == 3 and ds.launch_variant(FRAME) == ONE | S16
    ds.update_material(1, coarse)
    assert ds.grid_shared() == 0 and ds.launch_variant(FRAME) == S16
    # the same n on another range is another grid too
    ds.update_material(1, MaterialSpec(fine.kind, Spectrum(380.0, 740.0, fine.colour.samples), fine.diffuse_strength))
    assert ds.materials()["n"].tolist() == [32] * 6
    assert ds.grid_shared() == 0 and ds.launch_variant(FRAME) == S16
    ds.update_material(1, fine)
    assert ds.launch_variant(FRAME) == ONE | S16


def test_a_sky_row_on_another_grid_keeps_the_kernel():
    """Two-sample grey materials share a grid that is not the sky's 32 knots: the single-BVH kernel still
    runs (the sky lookup keeps its own segment and ratio there)."""
    spec = scenes.main_scene(MESH).spec()
    spec.materials = [MaterialSpec(m.kind, Spectrum.grey(0.5), m.diffuse_strength) for m in spec.materials]
    ds = DeviceScene(spec, 0, host_only=True)
    assert ds.materials()["n"].tolist() == [2, 2, 2, 2, 2, 32]
    assert ds.grid_shared() == 1 and ds.launch_variant(FRAME) == ONE | S16
    ds.update_material(2, MaterialSpec(N.MATERIAL_LAMBERTIAN, _rgb(0.2, 0.4, 0.6), 0.1))
    assert ds.grid_shared() == 0 and ds.launch_variant(FRAME) == S16


def test_kernels_that_keep_the_full_lookup_are_not_gated():
    """A scene with several material kinds runs the general kernel, which looks every spectrum up in full: its
    single-BVH form does not need the shared grid (materials_scene's glass has a two-sample eta)."""
    ds = DeviceScene(scenes.materials_scene(MESH).spec(), 0, host_only=True)
    assert ds.grid_shared() == 0 and ds.launch_variant(FRAME) & ONE


def test_light_rows_are_included():
    scene = scenes.main_scene(MESH)
    lights = [DirectionalLight((0.4, 1.0, -0.3), _rgb(1.0, 0.9, 0.7)), DirectionalLight((-0.6, 0.8, 0.2), _rgb(0.3, 0.4, 0.8))]
    scene.integrator = WhittedIntegrator(_rgb(0.05, 0.05, 0.05), lights)
    ds = DeviceScene(scene.spec(), 0, host_only=True)
    rows = ds.materials()
    assert len(rows) == 9 and DeviceScene.grids_shared(rows)  # 5 materials, ambient, 2 lights, sky
    assert ds.grid_shared() == 3
    for row in (5, 7):  # the ambient row, the last light's
        assert not DeviceScene.grids_shared(_flip(rows, row, "knots", 7, 0))
    grey = WhittedIntegrator(Spectrum.grey(0.05), lights)
    ds.set_lights(grey)
    assert ds.materials()["n"].tolist() == [32] * 5 + [2, 32, 32, 32] and ds.grid_shared() == 0
    ds.set_lights(scene.integrator)
    assert ds.grid_shared() == 3
    coarse = WhittedIntegrator(scene.integrator.ambient_light, [lights[0], DirectionalLight(lights[1].direction,
                                                                                    _coarse(lights[1].spectrum))])
    ds.set_lights(coarse)
    assert ds.grid_shared() == 0
    assert DeviceScene(scenes.whitted_scene(MESH).spec(), 0, host_only=True).grid_shared() == 0  # its grey ambient
