"""The single-BVH render kernels of one material kind look a path's wavelength up once (vr_render_kernel.h PATHWL).

Where lambda is drawn, at the camera hit, they find its segment and ratio on the wavelength grid the scene's
material rows share (vr_device.h path_segment); the surface colour of every later hit and the sky at the
path's end blend their two samples with that pair instead of finding it again.  The expressions are the full
lookup's on the same operands, so device records must be bit-identical to the generic kernel's
(VR_LAUNCH_MULTI_BVH, which keeps the full lookup), not merely close.  The host launches these kernels only
while the material rows share a grid bit for bit (tests/test_spectrum_grid_host.py); a sky row on another
grid keeps its own lookup inside them.
"""
import numpy as np
import pytest
import torch

from test_gpu_node_layout import _decisions_equal
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import Tile, render_samples, render_tile_device
from vanrijn_amd.scene import DeviceScene, MaterialSpec, Spectrum

pytestmark = pytest.mark.gpu

SEED = 0x5EED0B0B
ONE, S16 = N.VARIANT_ONE_BVH, N.VARIANT_STACK16
H = W = 128
TILE = Tile(16, 80, 48, 112)  # main.rs's scene at 128^2: floor, spheres, mesh and sky pixels (asserted below)
SPP = 6


def _records(ds, tile, h, w, spp, more=0, seed=SEED, **kw):
    """The device records of one launch (then `more` samples added onto them) as int64, and the last launch's stats"""
    st = torch.zeros(tile.width() * tile.height() * 8, dtype=torch.float64, device="cuda")
    s = render_tile_device(ds, tile, h, w, spp, seed, 0, st.data_ptr(), **kw)
    if more:
        s = render_tile_device(ds, tile, h, w, more, seed, spp, st.data_ptr(), accumulate=True, **kw)
    torch.cuda.synchronize()
    return st.cpu().view(torch.int64), s


def _same_as_the_generic_kernel(ds, tile, h, w, spp, seed=SEED, more=3):
    """default launch == VR_LAUNCH_MULTI_BVH bit for bit: fresh and accumulating (`more` samples onto the first
    `spp`), 16- and 32-bit stack entries"""
    for more in (0, more):
        for stack16 in (True, False):
            got, s = _records(ds, tile, h, w, spp, more=more, seed=seed, stack16=stack16)
            assert s["variant"] == ONE | (S16 if stack16 else 0)
            want, s = _records(ds, tile, h, w, spp, more=more, seed=seed, stack16=stack16, one_bvh=False)
            assert s["variant"] == (S16 if stack16 else 0)
            assert torch.equal(got, want), (more, stack16)
            assert np.count_nonzero(got.numpy()) > tile.width() * tile.height()
    return got


def _what_the_pixels_see(oracle, spec, tile, h, w):
    """the object and primitive of each tile pixel's centre ray: (object or -1, primitive)"""
    rays = [oracle.ray_for_pixel(spec.camera_location, w, h, r, c, 0.5, 0.5)
            for r in range(tile.start_row, tile.end_row) for c in range(tile.start_column, tile.end_column)]
    hits, _ = oracle.OracleScene(spec).trace(np.array([o for o, _ in rays]), np.array([d for _, d in rays]))
    return [(hh.object if hh.valid else -1, int(hh.primitive) if hh.valid else -1) for hh in hits]


def test_main_scene(oracle):
    scene = scenes.main_scene()
    seen = _what_the_pixels_see(oracle, scene.spec(), TILE, H, W)
    sky = sum(1 for o, _ in seen if o == -1)
    mesh = sum(1 for o, _ in seen if o == 1)
    floor, spheres = seen.count((0, 0)), sum(seen.count((0, k)) for k in (1, 2, 3))
    print(f"pixels: sky {sky}, mesh {mesh}, floor {floor}, spheres {spheres}")
    assert sky >= 200 and mesh >= 200 and floor >= 200 and spheres >= 100
    # Lambertian surfaces only: a path whose wavelength lies past the spectra's 720 nm carries nothing
    ref = oracle.OracleScene(scene.spec()).render_samples(TILE, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    red = (ref["wavelength"] > 720.0) & (ref["wavelength"] < 740.0)
    assert red.sum() >= 500 and (ref["intensity"][red] == 0.0).all()
    ds = scene.device_scene(0)
    assert ds.grid_shared() == 3
    _same_as_the_generic_kernel(ds, TILE, H, W, SPP)
    _decisions_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED), ref)


def test_bench_scene():
    """benches/simple_scene.rs's mirror mesh (the reflective-only kernels): a launch of more than 4 M
    pixel-samples, which the cooperative tail does not take."""
    ds = scenes.bench_scene().device_scene(0)
    assert ds.grid_shared() == 3
    t = Tile(0, 512, 0, 512)
    assert 512 * 512 * 17 > 4 << 20  # (the accumulating launch too)
    _same_as_the_generic_kernel(ds, t, 512, 512, 17, more=17)


def _coarse(sp, n=16):
    x = np.linspace(sp.shortest_wavelength, sp.longest_wavelength, n)
    xp = np.linspace(sp.shortest_wavelength, sp.longest_wavelength, sp.samples.size)
    return Spectrum(sp.shortest_wavelength, sp.longest_wavelength, np.interp(x, xp, sp.samples))


def test_a_material_on_another_grid(oracle):
    """main.rs's scene with the floor's spectrum on 16 knots: the generic kernel, held to the oracle; edited
    back to the shared grid the single-BVH kernel returns, edited away it leaves again."""
    spec = scenes.main_scene().spec()
    floor = spec.materials[0]
    coarse = MaterialSpec(floor.kind, _coarse(floor.colour), floor.diffuse_strength)
    spec.materials[0] = coarse
    ds = DeviceScene(spec, 0)
    assert ds.materials()["n"].tolist() == [16, 32, 32, 32, 32, 32] and ds.grid_shared() == 0
    got, s = _records(ds, TILE, H, W, SPP)
    assert not s["variant"] & ONE and s["variant"] == S16
    assert torch.equal(got, _records(ds, TILE, H, W, SPP, one_bvh=False)[0])
    ref = oracle.OracleScene(spec).render_samples(TILE, H, W, SPP, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    assert (ref["flags"] & 1).sum() >= 10000
    _decisions_equal(render_samples(ds, TILE, H, W, SPP, seed=SEED), ref)
    ds.update_material(0, floor)
    assert ds.grid_shared() == 3
    back = _same_as_the_generic_kernel(ds, TILE, H, W, SPP)
    assert torch.equal(back, _records(scenes.main_scene().device_scene(0), TILE, H, W, SPP, more=3, stack16=False)[0])
    ds.update_material(0, coarse)
    again, s = _records(ds, TILE, H, W, SPP)
    assert s["variant"] == S16 and torch.equal(again, got)


def test_a_sky_row_on_another_grid(oracle):
    """Two-sample grey materials share a grid that is not the sky's: the single-BVH kernel runs, its surface
    lookups with the path's pair and its sky lookup in full."""
    scene = scenes.main_scene()
    spec = scene.spec()
    spec.materials = [MaterialSpec(m.kind, Spectrum(380.0, 740.0, np.array([0.2 + 0.1 * i, 0.9 - 0.15 * i])),
                                   m.diffuse_strength) for i, m in enumerate(spec.materials)]
    ds = DeviceScene(spec, 0)
    assert ds.grid_shared() == 1
    _same_as_the_generic_kernel(ds, TILE, H, W, SPP)
    ref = oracle.OracleScene(spec).render_samples(TILE, H, W, 2, seed=SEED, mode=oracle.MODE_REFERENCE, nthreads=8)
    _decisions_equal(render_samples(ds, TILE, H, W, 2, seed=SEED), ref)


# ------------------------------------------------------------------------------------ wavelength edges
EDGE_SEED = 0x5EED0E06
EDGE_CROP = Tile(240, 304, 340, 404)  # of the 512^2 bench frame: on the mesh, with trapped paths (asserted below)


def test_out_of_range_wavelengths_and_the_recursion_limit(oracle):
    """The spectra end at 720 nm and wavelengths are drawn up to 740: for a path with lambda in (720, 740)
    every surface colour and the sky are 0 (the segment value -1; a mirror's specular term remains).  A path
    trapped between mirror facets ends at the recursion limit and reports wavelength 0.  Both occur in the
    crop (the oracle, on the CPU, before the device is asked)."""
    scene = scenes.bench_scene()
    ref = oracle.OracleScene(scene.spec()).render_samples(EDGE_CROP, 512, 512, 17, seed=EDGE_SEED,
                                                          mode=oracle.MODE_REFERENCE, nthreads=8)
    red = int(((ref["wavelength"] > 720.0) & (ref["wavelength"] < 740.0)).sum())
    limit = int(((ref["flags"] & 2) != 0).sum())
    print(f"lambda in (720, 740): {red} paths, recursion limit: {limit} paths of {ref.size}")
    assert red >= 500 and limit >= 10 and (ref["flags"] & 1).sum() >= 60000
    ds = scene.device_scene(0)
    t = Tile(0, 512, 0, 512)
    got, s = _records(ds, t, 512, 512, 17, seed=EDGE_SEED)
    assert s["variant"] == ONE | S16
    want, s = _records(ds, t, 512, 512, 17, seed=EDGE_SEED, one_bvh=False)
    assert s["variant"] == S16 and torch.equal(got, want)
    _decisions_equal(render_samples(ds, EDGE_CROP, 512, 512, 17, seed=EDGE_SEED), ref)
