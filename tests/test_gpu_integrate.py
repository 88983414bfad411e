"""The integrators for caller-supplied rays (vr_integrate_rays*, vanrijn_amd/csrc/vr_integrate.hip).

The rays, their stream ids and their wavelengths are rebuilt here from the oracle's own functions
(orc_stream_base / orc_stream_draw / orc_u64_to_standard, ray_for_pixel), so the kernel under test
gets nothing from the library's camera.  The photons are compared

  * with the oracle's per-sample records: flags, bounces and wavelength equal, the intensity within
    INTENSITY_REL_TOL (the project's bound for the forward against the recursive throughput product
    with ocml against glibc: tests/test_gpu_parity.py), NaN matching NaN;
  * with the megakernel's per-sample records (render_samples): bit for bit.

Rays are kept in the staging order [sample][pixel], so sample s of a full frame is the run of
consecutive streams first_stream = 0, sample = s.
"""
import numpy as np
import pytest
import torch

from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.render import (PATH_INFO_DTYPE, PHOTON_DTYPE, Tile, accumulate_photons_device, camera_rays_device,
                                integrate_rays, integrate_rays_device, render_samples, render_tile_device,
                                stream_check_error)
from vanrijn_amd.scene import DeviceScene, Scene

from test_gpu_fullframe import nan_scene
from test_gpu_ties import INTENSITY_REL_TOL

pytestmark = pytest.mark.gpu

PREFIXES = (1, 63, 257)  # one lane, a partial wave, a partial workgroup (and every ray: the whole batch)


# ------------------------------------------------------------------------------------- helpers
def _oracle_rays(oracle, camera, tile, H, W, spp, seed, first_sample=0):
    """ImageSampler's rays for every (sample, pixel) of the tile in [s][p] order, from the oracle:
    origins, directions, stream ids ((pixel << 32) + sample) and the wavelengths (draw 2)."""
    L = oracle.lib()
    tw, th = tile.end_column - tile.start_column, tile.end_row - tile.start_row
    n = tw * th
    o, d = np.empty((spp, n, 3)), np.empty((spp, n, 3))
    ids, wl = np.empty((spp, n), dtype=np.uint64), np.empty((spp, n))
    for s in range(spp):
        for p in range(n):
            row, col = tile.start_row + p // tw, tile.start_column + p % tw
            base = L.orc_stream_base(seed, row * W + col, first_sample + s)
            ux = L.orc_u64_to_standard(L.orc_stream_draw(base, 0))
            uy = L.orc_u64_to_standard(L.orc_stream_draw(base, 1))
            o[s, p], d[s, p] = oracle.ray_for_pixel(camera, W, H, row, col, ux, uy)
            ids[s, p] = ((row * W + col) << 32) + first_sample + s
            wl[s, p] = 380.0 + 360.0 * L.orc_u64_to_standard(L.orc_stream_draw(base, 2))
    out = (o.reshape(-1, 3), d.reshape(-1, 3), ids.reshape(-1), wl.reshape(-1))
    for a in out:
        a.setflags(write=False)
    return out


def _staging_order(rec):
    """[tile_h][tile_w][spp] records -> [s][p] order, flat."""
    spp = rec.shape[2]
    return np.ascontiguousarray(rec.reshape(-1, spp).T).reshape(-1)


def _matches_oracle(ph, info, ref):
    assert np.array_equal(info["flags"], ref["flags"])
    assert np.array_equal(info["bounces"], ref["bounces"])
    assert np.array_equal(ph["wavelength"], ref["wavelength"])
    g, r = ph["intensity"], ref["intensity"]
    both_nan = np.isnan(g) & np.isnan(r)
    with np.errstate(invalid="ignore"):
        ok = both_nan | (np.abs(g - r) <= INTENSITY_REL_TOL * np.abs(r))
    assert ok.all(), (int((~ok).sum()), g[~ok][:4], r[~ok][:4])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _equals_megakernel(ph, info, rec):
    assert np.array_equal(_bits(ph["wavelength"]), _bits(rec["wavelength"]))
    assert np.array_equal(_bits(ph["intensity"]), _bits(rec["intensity"]))
    assert np.array_equal(info["bounces"], rec["bounces"])
    assert np.array_equal(info["flags"], rec["flags"])


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # a writable copy


def _device_form(ds, o, d, seed, ids=None, wl=None, info=True, stream=None, extra=0, **kw):
    """vr_integrate_rays_device on torch buffers; `extra` guard records follow the n outputs."""
    n = len(o)
    to, td = _dev(o), _dev(d)
    tid = _dev(ids.view(np.int64)) if ids is not None else None
    twl = _dev(wl) if wl is not None else None
    ph = torch.full((n + extra, 2), -7.0, dtype=torch.float64, device="cuda")
    inf = torch.full((n + extra, 2), -7, dtype=torch.int32, device="cuda") if info else None
    torch.cuda.synchronize()
    integrate_rays_device(ds, n, to.data_ptr(), td.data_ptr(), ph.data_ptr(), seed,
                          wavelengths_ptr=twl.data_ptr() if wl is not None else None,
                          stream_ids_ptr=tid.data_ptr() if ids is not None else None,
                          info_ptr=inf.data_ptr() if info else None,
                          stream_ptr=stream.cuda_stream if stream is not None else None, **kw)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    p = ph.cpu().numpy().reshape(-1).view(PHOTON_DTYPE)
    i = inf.cpu().numpy().reshape(-1).view(PATH_INFO_DTYPE) if info else None
    return p, i


class Case:
    """A scene, the oracle's rays through one of its tiles and the two references, computed once."""

    def __init__(self, oracle, scene, tile, H, W, spp, seed, ray_camera=None, mode=None):
        self.scene, self.seed, self.spp = scene, seed, spp
        self.ds = scene.device_scene(0)
        self.npix = (tile.end_column - tile.start_column) * (tile.end_row - tile.start_row)
        spec = scene.spec()
        ray_scene = scene if ray_camera is None else Scene(ray_camera, scene.objects)
        self.o, self.d, self.ids, self.wl = _oracle_rays(
            oracle, ray_camera or spec.camera_location, tile, H, W, spp, seed)
        orc = oracle.OracleScene(ray_scene.spec())
        self.ref = _staging_order(orc.render_samples(tile, H, W, spp, seed=seed,
                                                     mode=oracle.MODE_REFERENCE if mode is None else mode, nthreads=8))
        self.ref.setflags(write=False)
        # the megakernel renders the scene's own camera only
        self.mega = _staging_order(render_samples(self.ds, tile, H, W, spp, seed=seed)) if ray_camera is None else None

    def check(self, n=None, given=False, device=False):
        n = len(self.o) if n is None else n
        kw = dict(wavelengths=self.wl[:n], first_draw=3) if given else dict(first_draw=2)
        if device:
            ph, info = _device_form(self.ds, self.o[:n], self.d[:n], self.seed, ids=self.ids[:n],
                                    wl=kw.get("wavelengths"), first_draw=kw["first_draw"])
        else:
            ph, info = integrate_rays(self.ds, self.o[:n], self.d[:n], self.seed, stream_ids=self.ids[:n], info=True,
                                      **kw)
        _matches_oracle(ph, info, self.ref[:n])
        if self.mega is not None:
            _equals_megakernel(ph, info, self.mega[:n])
        return ph, info


@pytest.fixture(scope="module")
def main_case(oracle):
    c = Case(oracle, scenes.main_scene(), Tile(0, 64, 0, 48), 48, 64, 2, 7)
    assert (c.ref["flags"] & 1).sum() > 1000 and (c.ref["bounces"] >= 2).sum() > 300
    return c


@pytest.fixture(scope="module", params=["materials", "whitted"])
def kinds_case(request, oracle):
    scene = {"materials": scenes.materials_scene, "whitted": scenes.whitted_scene}[request.param]()
    c = Case(oracle, scene, Tile(0, 48, 0, 32), 32, 48, 2, 7)
    assert (c.ref["flags"] & 1).sum() > 1000
    return c


# ------------------------------------------------------- 1 + 2. the oracle and the megakernel, per sample
@pytest.mark.parametrize("given", [False, True], ids=["drawn", "given"])
def test_main_scene(main_case, given):
    for n in PREFIXES:
        main_case.check(n, given)
    ph, info = main_case.check(None, given)
    dph, dinfo = main_case.check(None, given, device=True)
    assert np.array_equal(_bits(ph["intensity"]), _bits(dph["intensity"])) and np.array_equal(info, dinfo)
    assert info["bounces"].max() >= 8


@pytest.mark.parametrize("given", [False, True], ids=["drawn", "given"])
def test_every_material_and_whitted(kinds_case, given):
    for n in PREFIXES:
        kinds_case.check(n, given)
    kinds_case.check(None, given)
    kinds_case.check(None, given, device=True)


def test_consecutive_streams_without_ids(main_case):
    """stream_ids == NULL: ray i of a full frame's sample s draws from (first_stream + i, s)."""
    c = main_case
    for s, first in ((1, 1400), (0, 2000)):  # rows below the horizon
        sl = slice(s * c.npix + first, s * c.npix + first + 700)
        ph, info = integrate_rays(c.ds, c.o[sl], c.d[sl], c.seed, first_stream=first, sample=s, first_draw=2,
                                  info=True)
        _equals_megakernel(ph, info, c.mega[sl])
        assert (info["flags"] & 1).sum() > 100
        only = integrate_rays(c.ds, c.o[sl], c.d[sl], c.seed, first_stream=first, sample=s, first_draw=2)
        assert np.array_equal(_bits(only["intensity"]), _bits(ph["intensity"]))  # without `info`


def test_nan_photons_where_the_megakernel_has_them(oracle, tmp_path):
    """test_gpu_fullframe.py's scene with a normal-less wall behind the camera: NaN photons exactly
    where the megakernel's (and the reference's) are."""
    c = Case(oracle, nan_scene(tmp_path), Tile(0, 48, 0, 48), 48, 48, 4, 0x5EED0001)
    assert np.isnan(c.mega["intensity"]).sum() > 100
    for given in (False, True):
        ph, _ = c.check(None, given)
        assert np.array_equal(np.isnan(ph["intensity"]), np.isnan(c.mega["intensity"]))


# ----------------------------------------------------------------------------- 3. the recursion limit
def _two_mirror_scene():
    """tests/test_gpu_launch_variants.py's scene: two reflective bunny-like meshes side by side, close
    enough that paths bounce between them up to the recursion limit."""
    from vanrijn_amd.scene import (BoundingVolumeHierarchy, ColourRgbF, Mesh, NamedColour, ReflectiveMaterial,
                                   Spectrum)
    objs = []
    for centre, seed, colour in (((-2.55, -0.5, 0.0), 0xB0BB1E, NamedColour.Yellow),
                                 ((-0.95, -0.35, 0.25), 0xC0FFEE, NamedColour.Red)):
        v, n = scenes.displaced_mesh(20, scenes._BUNNY_BUMPS, noise_seed=seed, noise_count=24, noise_amp=0.05,
                                     scale=(0.8, 0.75, 0.8), centre=centre)
        mat = ReflectiveMaterial(Spectrum.reflection_from_linear_rgb(ColourRgbF.from_named(colour)), 0.05, 0.9)
        objs.append(BoundingVolumeHierarchy.build(Mesh(v, n, mat)))
    return Scene(scenes.CAMERA_LOCATION, objs)


def test_recursion_limit(oracle):
    c = Case(oracle, _two_mirror_scene(), Tile(56, 104, 72, 120), 160, 160, 4, 0x5EED0001, mode=oracle.MODE_PRUNED)
    limit = ((c.ref["flags"] & 2) != 0) & (c.ref["bounces"] == 128)
    assert limit.sum() >= 10 and (c.ref["flags"] & 1).sum() > 1000
    assert (c.ref["wavelength"][limit] == 0).all()
    for given in (False, True):
        c.check(None, given)
    c.check(None, False, device=True)


# -------------------------------------------------------------- 4. a camera the library does not have
def test_rays_of_another_camera(oracle):
    """The device scene keeps its camera (-2, 1, -5); the rays and the reference are those of the same
    objects seen from (0.5, 2, -4): nothing depends on the scene's camera or its frustum cull."""
    scene = scenes.main_scene()
    assert tuple(scene.spec().camera_location) == (-2.0, 1.0, -5.0)
    c = Case(oracle, scene, Tile(0, 64, 0, 48), 48, 64, 2, 7, ray_camera=(0.5, 2.0, -4.0))
    assert (c.ref["flags"] & 1).sum() > 1000
    for given in (False, True):
        for n in PREFIXES + (None,):
            c.check(n, given)
    c.check(None, False, device=True)


# ------------------------------------------------------------------------ 5. the staged pipeline
def test_staged_pipeline_equals_the_render(oracle):
    scene = scenes.main_scene()
    ds = scene.device_scene(0)
    H, W, seed = 48, 64, 7
    tile = Tile(8, 56, 8, 40)
    npix = tile.width() * tile.height()
    stream = torch.cuda.current_stream().cuda_stream
    staged = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    direct = torch.zeros(npix * 8, dtype=torch.float64, device="cuda")
    for first, spp, acc in ((0, 3, False), (3, 2, True)):
        n = npix * spp
        o = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        d = torch.zeros(n * 3, dtype=torch.float64, device="cuda")
        ids = torch.zeros(n, dtype=torch.int64, device="cuda")
        ph = torch.zeros(n * 2, dtype=torch.float64, device="cuda")
        camera_rays_device(ds, tile, H, W, spp, seed, first, o.data_ptr(), d.data_ptr(), ids.data_ptr(), stream)
        integrate_rays_device(ds, n, o.data_ptr(), d.data_ptr(), ph.data_ptr(), seed, stream_ids_ptr=ids.data_ptr(),
                              first_draw=2, stream_ptr=stream)
        accumulate_photons_device(staged.data_ptr(), ph.data_ptr(), npix, spp, accumulate=acc, stream_ptr=stream)
        render_tile_device(ds, tile, H, W, spp, seed, first, direct.data_ptr(), stream, accumulate=acc)
        torch.cuda.synchronize()
        stream_check_error(ds, stream)
        assert torch.equal(staged.view(torch.int64), direct.view(torch.int64)), (first, spp)
        ro, rd, rids, _ = _oracle_rays(oracle, scene.spec().camera_location, tile, H, W, spp, seed, first)
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(ro.reshape(-1)))
        assert np.array_equal(_bits(d.cpu().numpy()), _bits(rd.reshape(-1)))
        assert np.array_equal(ids.cpu().numpy().view(np.uint64), rids)
    assert float(staged.cpu().numpy()[:4 * npix].reshape(-1, 4)[:, 3].sum()) == 5 * npix  # the weights


# -------------------------------------------------------------------------- 6. VR_QUERY_NORMALIZE
def test_normalize_flag(oracle, main_case):
    """Directions that are not unit length, with the flag: the photons of Ray::new's unit ones (scaling by
    a power of two leaves every operation of the normalisation exact)."""
    ds = main_case.ds
    g = np.random.default_rng(5)
    cam = np.array(main_case.scene.spec().camera_location)
    n = 600
    v = g.uniform([-3.5, -2.5, -1.5], [0.5, 1.5, 1.5], (n, 3)) - cam
    o = np.repeat(cam[None], n, 0)
    unit = np.array([oracle.ray_new(o[k], v[k])[1] for k in range(n)])
    want, winfo = integrate_rays(ds, o, unit, 11, info=True)
    assert (winfo["flags"] & 1).sum() > 200
    for scaled in (v, 4.0 * v, 0.125 * v):
        ph, info = integrate_rays(ds, o, scaled, 11, normalize=True, info=True)
        assert np.array_equal(_bits(ph["wavelength"]), _bits(want["wavelength"]))
        assert np.array_equal(_bits(ph["intensity"]), _bits(want["intensity"]))
        assert np.array_equal(info, winfo)


# ----------------------------------------------------------------------------------- 7. the error path
def test_fault_object_error_path(main_case):
    c = main_case
    n = len(c.o)
    faulty = DeviceScene(c.scene.spec(), 0)
    faulty.set_fault_object(1)  # the mesh BVH
    with pytest.raises(N.VrError) as e:
        integrate_rays(faulty, c.o, c.d, c.seed, stream_ids=c.ids, first_draw=2)
    assert e.value.code == -5
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    # a second stream used at the same time, with rays that miss everything (straight up)
    up = np.tile([0.0, 1.0, 0.0], (n, 1))
    to, tup = _dev(c.o), _dev(up)
    ph2 = torch.full((n, 2), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    integrate_rays_device(faulty, n, to.data_ptr(), tup.data_ptr(), ph2.data_ptr(), c.seed, stream_ptr=s2.cuda_stream)
    ph, info = _device_form(faulty, c.o, c.d, c.seed, ids=c.ids, first_draw=2, stream=s1)
    with pytest.raises(N.VrError) as e:
        stream_check_error(faulty, s1.cuda_stream)
    assert e.value.code == -5
    stream_check_error(faulty, s1.cuda_stream)  # cleared by the check
    stream_check_error(faulty, s2.cuda_stream)  # the other stream never saw it
    assert not ph2.cpu().numpy().any()
    # a path that touches object 1 ends there with flag bit 2 and photon {0, 0}; every other ray's
    # photon is the clean scene's
    hit1 = (info["flags"] & 4) != 0
    assert hit1.sum() > 100 and ((info["flags"] & 1) != 0)[~hit1].sum() > 500
    assert not ph["wavelength"][hit1].any() and not ph["intensity"][hit1].any()
    _equals_megakernel(ph[~hit1], info[~hit1], c.mega[~hit1])


# ------------------------------------------------------------------- 8. nothing past n is written
def test_outputs_past_n_are_not_written(main_case):
    c = main_case
    for n in (1, 63, 257, 1500):
        ph, info = _device_form(c.ds, c.o[:n], c.d[:n], c.seed, ids=c.ids[:n], first_draw=2, extra=300)
        _equals_megakernel(ph[:n], info[:n], c.mega[:n])
        assert (ph["wavelength"][n:] == -7.0).all() and (ph["intensity"][n:] == -7.0).all()
        assert (info["bounces"][n:] == -7).all() and (info["flags"][n:] == -7).all()
