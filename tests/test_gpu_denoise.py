"""The denoiser's device forms (vr_denoise_device, vr_denoise, vanrijn_amd/csrc/vr_denoise.hip) against the
independent numpy reference of tests/denoise_reference.py, bit for bit, on the cases of
tests/test_denoise_host.py and on shapes that cross workgroup and halo boundaries in both directions -- the
direct-load form's 64 x 4 blocks, the LDS form's 128-column runs and its 2 * step columns of halo.  Both load
forms and the library's own choice are run everywhere; past step 16 the LDS form is the direct one.

Every case is at most 129 pixels on a side; the references are computed once per session
(tests/denoise_cases.py).  The last test renders 64x48 at 512 spp."""
import ctypes as C

import numpy as np
import pytest
import torch

import denoise_cases as cases
from denoise_reference import DEMODULATE, MATCH_OBJECT, denoise_reference, same_bits
from vanrijn_amd import _native as N
from vanrijn_amd import scenes
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE
from vanrijn_amd.render import (DenoiseParams, Tile, denoise, denoise_device, denoise_workspace_bytes,
                                render_features_device, render_tile_device, resolve_state, tone_map_device)

pytestmark = pytest.mark.gpu

GUARD = 16  # doubles past the output's last record, and past the reported workspace
GUARD_VALUE = -7.0
LOADS = [None, "direct", "lds"]


def params(width, height, iterations, flags=0, loads=None):
    p = DenoiseParams(width, height, iterations, *cases.SIGMAS, loads=loads)
    p.flags |= flags
    return p


def run_device(inp, iterations, flags=0, loads=None, in_place=False, stream=None, albedo=True):
    """vr_denoise_device on device copies of the inputs; the guards after the output and after the reported
    workspace size are checked, and so is that the inputs stayed as they were."""
    n = inp.width * inp.height
    p = params(inp.width, inp.height, iterations, flags, loads)
    ws_bytes = denoise_workspace_bytes(p)
    assert ws_bytes % 8 == 0 and ws_bytes <= 128 * n
    state = torch.from_numpy(np.concatenate([inp.state, np.full(GUARD, GUARD_VALUE)])).cuda()
    out = state if in_place else torch.full((8 * n + GUARD,), GUARD_VALUE, dtype=torch.float64, device="cuda")
    feat = torch.from_numpy(inp.features.reshape(-1).view(np.uint8).copy()).cuda()
    alb = torch.from_numpy(inp.albedo_state.copy()).cuda()
    ws = torch.full((ws_bytes // 8 + GUARD,), GUARD_VALUE, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    denoise_device(p, state.data_ptr(), feat.data_ptr(), alb.data_ptr() if albedo else None, out.data_ptr(), ws.data_ptr(),
                   stream_ptr=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[8 * n:] == GUARD_VALUE).all(), "guard values past the last record changed"
    assert (ws.cpu().numpy()[ws_bytes // 8:] == GUARD_VALUE).all(), "written past the reported workspace size"
    assert feat.cpu().numpy().tobytes() == inp.features.tobytes() and same_bits(alb.cpu().numpy(), inp.albedo_state)
    if not in_place:
        assert same_bits(state.cpu().numpy()[:8 * n], inp.state)
    return got[:8 * n]


@pytest.mark.parametrize("loads", LOADS)
@pytest.mark.parametrize("iterations", [1, 3, 8])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 5), (37, 29)], ids=lambda s: "%dx%d" % s)
def test_plain_images(shape, iterations, loads):
    assert same_bits(run_device(cases.inputs(*shape), iterations, loads=loads), cases.reference(*shape, iterations))


@pytest.mark.parametrize("loads", LOADS)
@pytest.mark.parametrize("iterations", [1, 3, 8])
@pytest.mark.parametrize("specials", ["a", "b"])
@pytest.mark.parametrize("shape", [(5, 5), (37, 29)], ids=lambda s: "%dx%d" % s)
def test_special_values(shape, specials, iterations, loads):
    inp = cases.inputs(*shape, specials=specials)
    out = run_device(inp, iterations, loads=loads)
    assert same_bits(out, cases.reference(*shape, iterations, specials=specials))
    n = shape[0] * shape[1]
    assert np.isfinite(out[:4 * n].reshape(shape[1], shape[0], 4)[~inp.nonfinite]).all()


@pytest.mark.parametrize("loads", LOADS)
@pytest.mark.parametrize("kind", ["nan_colour", "inf_colour", "nan_normal", "zero_depth", "background", "absent"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)], ids=lambda s: "%dx%d" % s)
def test_special_values_on_thin_images(shape, kind, loads):
    out = run_device(cases.inputs(*shape, specials=kind), 3, loads=loads)
    assert same_bits(out, cases.reference(*shape, 3, specials=kind))


@pytest.mark.parametrize("loads", LOADS)
@pytest.mark.parametrize("specials", [None, "a", "b"])
@pytest.mark.parametrize("flags", [MATCH_OBJECT, DEMODULATE, MATCH_OBJECT | DEMODULATE])
def test_flags(flags, specials, loads):
    out = run_device(cases.inputs(37, 29, specials=specials), 3, flags, loads=loads)
    assert same_bits(out, cases.reference(37, 29, 3, flags, specials=specials))


@pytest.mark.parametrize("loads", LOADS)
@pytest.mark.parametrize("specials", [None, "a", "b"])
@pytest.mark.parametrize("shape", [(70, 45), (129, 3), (3, 129), (37, 29)], ids=lambda s: "%dx%d" % s)
def test_shapes_across_workgroups_and_halos(shape, specials, loads):
    """Five iterations: steps 1 .. 16, the LDS form's widest halo (32 columns on each side)."""
    flags = MATCH_OBJECT | DEMODULATE if specials == "b" else 0
    out = run_device(cases.inputs(*shape, specials=specials), 5, flags, loads=loads)
    assert same_bits(out, cases.reference(*shape, 5, flags, specials=specials))


@pytest.mark.parametrize("loads", LOADS)
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("on_stream", [False, True], ids=["null_stream", "torch_stream"])
def test_streams_and_in_place(on_stream, in_place, loads):
    inp = cases.inputs(70, 45, specials="a")
    flags = MATCH_OBJECT | DEMODULATE
    out = run_device(inp, 5, flags, loads=loads, in_place=in_place, stream=torch.cuda.Stream() if on_stream else None)
    assert same_bits(out, cases.reference(70, 45, 5, flags, specials="a"))


def test_a_null_albedo_without_demodulate():
    out = run_device(cases.inputs(37, 29), 3, albedo=False)
    assert same_bits(out, cases.reference(37, 29, 3))


@pytest.mark.parametrize("flags", [0, MATCH_OBJECT | DEMODULATE])
@pytest.mark.parametrize("specials", [None, "a", "b"])
def test_the_three_forms_agree(specials, flags):
    inp = cases.inputs(70, 45, specials=specials)
    p = params(70, 45, 5, flags)
    dev = run_device(inp, 5, flags)
    staged = denoise(inp.state, inp.features, inp.albedo_state, params=p)
    host = denoise(inp.state, inp.features, inp.albedo_state, params=p, host=True)
    assert same_bits(staged, dev) and same_bits(host, dev)


def test_stages_in_order_are_the_call():
    inp = cases.inputs(70, 45, specials="b")
    n = 70 * 45
    p = params(70, 45, 3, DEMODULATE)
    state = torch.from_numpy(inp.state.copy()).cuda()
    feat = torch.from_numpy(inp.features.reshape(-1).view(np.uint8).copy()).cuda()
    alb = torch.from_numpy(inp.albedo_state.copy()).cuda()
    out = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    ws = torch.zeros(denoise_workspace_bytes(p) // 8, dtype=torch.float64, device="cuda")
    for stage in range(5):
        denoise_device(p, state.data_ptr(), feat.data_ptr(), alb.data_ptr(), out.data_ptr(), ws.data_ptr(), stage=stage)
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), cases.reference(70, 45, 3, DEMODULATE, specials="b"))


W, H, SEED = 64, 48, 0x5EED0D15


@pytest.fixture(scope="module")
def main_ds():
    return scenes.main_scene().device_scene(0)


def test_end_to_end_on_one_stream(main_ds):
    """render_tile_device, render_features_device with the albedo, denoise_device and tone_map_device
    enqueued on one stream with no synchronisation in between."""
    n, tile = W * H, Tile(0, W, 0, H)
    p = DenoiseParams(W, H, demodulate=True)
    state = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    feat = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    alb = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    out = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    ws = torch.zeros(denoise_workspace_bytes(p) // 8, dtype=torch.float64, device="cuda")
    rgb = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
    rgb_ref = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    render_tile_device(main_ds, tile, H, W, 3, SEED, 0, state.data_ptr(), stream_ptr=s)
    render_features_device(main_ds, tile, H, W, 3, SEED, 0, feat.data_ptr(), alb.data_ptr(), stream_ptr=s)
    denoise_device(p, state.data_ptr(), feat.data_ptr(), alb.data_ptr(), out.data_ptr(), ws.data_ptr(), stream_ptr=s)
    tone_map_device(out.data_ptr(), n, rgb.data_ptr(), stream_ptr=s)
    stream.synchronize()
    torch.cuda.synchronize()
    records = feat.cpu().numpy().view(PIXEL_FEATURES_DTYPE).reshape(H, W)
    assert (records["hits"] > 0).sum() > 1000 and (records["hits"] == 0).sum() > 400
    want = denoise_reference(W, H, p.iterations, p.flags, p.sigma_colour, p.sigma_normal, p.sigma_depth,
                             state.cpu().numpy(), records, alb.cpu().numpy())
    got = out.cpu().numpy()
    assert same_bits(got, want)
    assert not same_bits(got[:4 * n], state.cpu().numpy()[:4 * n])
    up = torch.from_numpy(want).cuda()
    tone_map_device(up.data_ptr(), n, rgb_ref.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(rgb, rgb_ref) and int(rgb.max()) > 0


def test_it_denoises(main_ds):
    """XYZ RMSE against a 512-spp render with another seed: the denoised 2-spp image must be closer than the
    2-spp image itself, with the default parameters.  A condition, not a tuned number; the figures are printed."""
    n, tile = W * H, Tile(0, W, 0, H)
    p = DenoiseParams(W, H)
    noisy = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    truth = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    feat = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    out = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    ws = torch.zeros(denoise_workspace_bytes(p) // 8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    render_tile_device(main_ds, tile, H, W, 2, SEED, 0, noisy.data_ptr())
    render_features_device(main_ds, tile, H, W, 2, SEED, 0, feat.data_ptr(), None)
    render_tile_device(main_ds, tile, H, W, 512, SEED + 1, 0, truth.data_ptr())
    denoise_device(p, noisy.data_ptr(), feat.data_ptr(), None, out.data_ptr(), ws.data_ptr())
    torch.cuda.synchronize()
    ref = resolve_state(truth.cpu().numpy())

    def rmse(state):
        return float(np.sqrt(np.mean((resolve_state(state.cpu().numpy()) - ref) ** 2)))

    e_noisy, e_denoised = rmse(noisy), rmse(out)
    print(f"XYZ RMSE vs 512 spp: noisy {e_noisy:.6f} denoised {e_denoised:.6f} ratio {e_denoised / e_noisy:.4f}")
    assert np.isfinite(e_noisy) and np.isfinite(e_denoised)
    assert e_denoised < e_noisy
