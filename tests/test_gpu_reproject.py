"""The temporal reprojection's device forms (vr_reproject_device, vr_reproject, vanrijn_amd/csrc/vr_reproject.hip)
against the independent numpy reference of tests/reproject_reference.py, bit for bit, on the cases of
tests/test_reproject_host.py and on shapes that cross the kernel's 64 x 4 blocks in both directions.

Every case is at most 129 pixels on a side; the references are computed once per session
(tests/reproject_cases.py).  The last tests render 64x48 frames of scenes.main_scene(); one of them renders
512 spp once."""
import math

import numpy as np
import pytest
import torch

import reproject_cases as cases
from reproject_reference import MATCH_OBJECT, Pose, reproject_reference, same_bits
from vanrijn_amd import scenes
from vanrijn_amd.records import PIXEL_FEATURES_DTYPE
from vanrijn_amd.render import (DenoiseParams, ReprojectParams, Tile, denoise_device, denoise_workspace_bytes, motion_rows,
                                render_features_device, render_tile_device, reproject, reproject_device, resolve_state,
                                tone_map_device)
from vanrijn_amd.scene import CameraPose, look_at

pytestmark = pytest.mark.gpu

GUARD = 16  # doubles past the output's last record
GUARD_VALUE = -7.0
ids = lambda s: "%dx%d" % s  # noqa: E731


def c_pose(pose):
    return CameraPose(pose.location, pose.right, pose.up, pose.forward, pose.film_distance)


def params(inp, flags=MATCH_OBJECT, cap=math.inf):
    p = ReprojectParams(inp.width, inp.height, c_pose(inp.pose), c_pose(inp.previous_pose), *cases.TOLERANCES, cap,
                        motion_count=inp.motion_count)
    p.flags = flags
    return p


def features_tensor(records):
    return torch.from_numpy(np.ascontiguousarray(records).reshape(-1).view(np.uint8).copy()).cuda()


def run_device(inp, flags=MATCH_OBJECT, cap=math.inf, in_place=False, stream=None):
    """vr_reproject_device on device copies of the inputs; the guards after the output are checked, and so is
    that the inputs stayed as they were."""
    n = inp.width * inp.height
    state = torch.from_numpy(np.concatenate([inp.state, np.full(GUARD, GUARD_VALUE)])).cuda()
    out = state if in_place else torch.full((8 * n + GUARD,), GUARD_VALUE, dtype=torch.float64, device="cuda")
    feat, pfeat = features_tensor(inp.features), features_tensor(inp.previous_features)
    pstate = torch.from_numpy(inp.previous_state.copy()).cuda()
    motion = None if inp.motion is None else torch.from_numpy(np.ascontiguousarray(inp.motion).copy()).cuda()
    torch.cuda.synchronize()
    reproject_device(params(inp, flags, cap), state.data_ptr(), feat.data_ptr(), pstate.data_ptr(), pfeat.data_ptr(),
                     out.data_ptr(), motion_ptr=motion.data_ptr() if motion is not None else None,
                     stream_ptr=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[8 * n:] == GUARD_VALUE).all(), "guard values past the last record changed"
    assert feat.cpu().numpy().tobytes() == inp.features.tobytes()
    assert pfeat.cpu().numpy().tobytes() == inp.previous_features.tobytes()
    assert same_bits(pstate.cpu().numpy(), inp.previous_state)
    assert motion is None or same_bits(motion.cpu().numpy(), inp.motion)
    if not in_place:
        assert same_bits(state.cpu().numpy()[:8 * n], inp.state)
    return got[:8 * n]


@pytest.mark.parametrize("poses", list(cases.POSES))
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 5), (37, 29)], ids=ids)
def test_pose_pairs(shape, poses):
    assert same_bits(run_device(cases.inputs(*shape, poses)), cases.reference(*shape, poses)[0])


@pytest.mark.parametrize("specials", cases.SPECIALS)
@pytest.mark.parametrize("poses", ["identical", "translation", "rotation"])
@pytest.mark.parametrize("shape", [(5, 5), (37, 29)], ids=ids)
def test_special_values(shape, poses, specials):
    inp = cases.inputs(*shape, poses, specials=specials)
    assert same_bits(run_device(inp), cases.reference(*shape, poses, specials=specials)[0])


@pytest.mark.parametrize("specials", ["nan_sum", "absent_cur", "background", "mixed"])
@pytest.mark.parametrize("poses", ["identical", "translation"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)], ids=ids)
def test_special_values_on_thin_images(shape, poses, specials):
    inp = cases.inputs(*shape, poses, specials=specials)
    assert same_bits(run_device(inp), cases.reference(*shape, poses, specials=specials)[0])


def test_a_tap_of_weight_zero_is_never_read():
    inp, (row, column), _ = cases.zero_weight_tap()
    want, history = reproject_reference(37, 29, inp.pose, inp.previous_pose, *cases.TOLERANCES, math.inf, MATCH_OBJECT,
                                        inp.state, inp.features, inp.previous_state, inp.previous_features)
    assert history[row, column]
    out = run_device(inp)
    assert same_bits(out, want) and np.isfinite(out[:4 * 37 * 29].reshape(29, 37, 4)[row, column]).all()


@pytest.mark.parametrize("specials", [None, "mixed"])
@pytest.mark.parametrize("poses", ["identical", "translation", "rotation", "out_of_frame"])
def test_without_match_object(poses, specials):
    inp = cases.inputs(37, 29, poses, specials=specials)
    assert same_bits(run_device(inp, flags=0), cases.reference(37, 29, poses, specials=specials, flags=0)[0])


@pytest.mark.parametrize("cap", [math.inf, 8.0, 0.5])
@pytest.mark.parametrize("poses", ["identical", "translation", "film_distance"])
def test_caps(poses, cap):
    inp = cases.inputs(37, 29, poses, specials="mixed")
    assert same_bits(run_device(inp, cap=cap), cases.reference(37, 29, poses, specials="mixed", cap=cap)[0])


@pytest.mark.parametrize("motion", [m for m in cases.MOTIONS if m != "none"])
@pytest.mark.parametrize("poses", ["identical", "translation"])
@pytest.mark.parametrize("shape", [(5, 5), (37, 29)], ids=ids)
def test_motion_rows(shape, poses, motion):
    specials = "mixed" if shape == (37, 29) else None
    inp = cases.inputs(*shape, poses, motion, specials)
    assert same_bits(run_device(inp), cases.reference(*shape, poses, motion, specials)[0])


@pytest.mark.parametrize("poses,motion,specials", [("identical", "none", None), ("translation", "none", "mixed"),
                                                   ("rotation", "rotation", "mixed"), ("out_of_frame", "none", None),
                                                   ("film_distance", "first_only", "mixed")])
@pytest.mark.parametrize("shape", [(70, 45), (129, 3), (3, 129)], ids=ids)
def test_shapes_across_blocks(shape, poses, motion, specials):
    inp = cases.inputs(*shape, poses, motion, specials)
    assert same_bits(run_device(inp), cases.reference(*shape, poses, motion, specials)[0])


@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("on_stream", [False, True], ids=["null_stream", "torch_stream"])
@pytest.mark.parametrize("poses", ["identical", "rotation"])
def test_streams_and_in_place(poses, on_stream, in_place):
    inp = cases.inputs(70, 45, poses, "rotation", "mixed")
    out = run_device(inp, in_place=in_place, stream=torch.cuda.Stream() if on_stream else None)
    assert same_bits(out, cases.reference(70, 45, poses, "rotation", "mixed")[0])


@pytest.mark.parametrize("poses,motion", [("identical", "none"), ("translation", "translation"), ("out_of_frame", "none")])
def test_the_three_forms_agree(poses, motion):
    inp = cases.inputs(70, 45, poses, motion, "mixed")
    p = params(inp)
    p.motion_count = 0
    dev = run_device(inp)
    args = (inp.state, inp.features, inp.previous_state, inp.previous_features, p)
    staged = reproject(*args, motion=inp.motion)
    host = reproject(*args, motion=inp.motion, host=True)
    assert same_bits(staged, dev) and same_bits(host, dev)
    assert same_bits(dev, cases.reference(70, 45, poses, motion, "mixed")[0])


# ---- rendered frames ----
W, H, SEED, SPP = 64, 48, 0x5EED0D15, 4
POSE_A = CameraPose(location=scenes.CAMERA_LOCATION)
EYE_B = (scenes.CAMERA_LOCATION[0] + 0.08, scenes.CAMERA_LOCATION[1] + 0.03, scenes.CAMERA_LOCATION[2])
TARGET = (scenes.CAMERA_LOCATION[0], scenes.CAMERA_LOCATION[1], 0.0)  # 5 ahead of pose A: B turns by 0.016 rad, a pixel is 0.021


def ref_pose(pose):
    return Pose(pose.location, pose.right, pose.up, pose.forward, pose.film_distance)


@pytest.fixture(scope="module")
def main_ds():
    return scenes.main_scene().device_scene(0)


class Frame:
    """State and feature records of one rendered frame, on the device."""

    def __init__(self):
        self.state = torch.zeros(8 * W * H, dtype=torch.float64, device="cuda")
        self.features = torch.zeros(64 * W * H, dtype=torch.uint8, device="cuda")

    def render(self, ds, first_sample, stream_ptr=None, spp=SPP, seed=SEED):
        tile = Tile(0, W, 0, H)
        render_tile_device(ds, tile, H, W, spp, seed, first_sample, self.state.data_ptr(), stream_ptr=stream_ptr)
        render_features_device(ds, tile, H, W, spp, seed, first_sample, self.features.data_ptr(), None, stream_ptr=stream_ptr)

    def records(self):
        return self.features.cpu().numpy().view(PIXEL_FEATURES_DTYPE).reshape(H, W)


def reference_of(p, a, b, motion=None):
    return reproject_reference(W, H, ref_pose(CameraPose._from_c(p.pose)), ref_pose(CameraPose._from_c(p.previous_pose)),
                               p.depth_tolerance, p.normal_tolerance, p.max_history_weight, p.flags, b.state.cpu().numpy(),
                               b.records(), a.state.cpu().numpy(), a.records(), motion, 0 if motion is None else len(motion))


def test_end_to_end_on_one_stream(main_ds):
    """Frame A, a camera step of about a pixel, frame B, reproject_device, denoise_device on its output and
    tone_map_device, enqueued on one stream with no synchronisation in between."""
    n = W * H
    pose_b = look_at(EYE_B, TARGET)
    rp = ReprojectParams(W, H, pose_b, POSE_A)
    dp = DenoiseParams(W, H)
    a, b = Frame(), Frame()
    merged = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    clean = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    ws = torch.zeros(denoise_workspace_bytes(dp) // 8, dtype=torch.float64, device="cuda")
    rgb = torch.zeros(3 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    try:
        main_ds.set_camera_pose(POSE_A)
        a.render(main_ds, 0, s)
        main_ds.set_camera_pose(pose_b)  # a launch argument: frame A's launches carry their own copy
        b.render(main_ds, SPP, s)
        reproject_device(rp, b.state.data_ptr(), b.features.data_ptr(), a.state.data_ptr(), a.features.data_ptr(),
                         merged.data_ptr(), stream_ptr=s)
        denoise_device(dp, merged.data_ptr(), b.features.data_ptr(), None, clean.data_ptr(), ws.data_ptr(), stream_ptr=s)
        tone_map_device(clean.data_ptr(), n, rgb.data_ptr(), stream_ptr=s)
        stream.synchronize()
        torch.cuda.synchronize()
    finally:
        main_ds.set_camera_pose(POSE_A)
    want, history = reference_of(rp, a, b)
    hit = b.records()["hits"] > 0
    share = float(history[hit].sum()) / int(hit.sum())
    print(f"history at {share:.3f} of {int(hit.sum())} hit pixels")
    assert hit.sum() > 1000 and share >= 0.5
    got = merged.cpu().numpy()
    assert same_bits(got, want)
    assert not same_bits(got[:4 * n], b.state.cpu().numpy()[:4 * n])
    assert int(rgb.max()) > 0 and np.isfinite(clean.cpu().numpy()).all()


def test_it_accumulates(main_ds):
    """XYZ RMSE over the hit pixels against a 512-spp render of pose B with another seed: frame B with frame A's
    history reprojected into it must be closer than frame B alone, with the default parameters.  A condition,
    not a tuned number; the figures are printed."""
    n = W * H
    pose_b = look_at(EYE_B, TARGET)
    rp = ReprojectParams(W, H, pose_b, POSE_A)
    a, b, truth = Frame(), Frame(), Frame()
    merged = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    try:
        main_ds.set_camera_pose(POSE_A)
        a.render(main_ds, 0)
        main_ds.set_camera_pose(pose_b)
        b.render(main_ds, SPP)
        render_tile_device(main_ds, Tile(0, W, 0, H), H, W, 512, SEED + 1, 0, truth.state.data_ptr())
        reproject_device(rp, b.state.data_ptr(), b.features.data_ptr(), a.state.data_ptr(), a.features.data_ptr(),
                         merged.data_ptr())
        torch.cuda.synchronize()
    finally:
        main_ds.set_camera_pose(POSE_A)
    hit = (b.records()["hits"] > 0).reshape(-1)
    ref = resolve_state(truth.state.cpu().numpy())[hit]

    def rmse(state):
        return float(np.sqrt(np.mean((resolve_state(state.cpu().numpy())[hit] - ref) ** 2)))

    e_frame, e_merged = rmse(b.state), rmse(merged)
    print(f"XYZ RMSE vs 512 spp over {int(hit.sum())} hit pixels: frame B {e_frame:.6f} reprojected {e_merged:.6f} "
          f"ratio {e_merged / e_frame:.4f}")
    assert np.isfinite(e_frame) and np.isfinite(e_merged)
    assert e_merged < e_frame


def test_a_moved_mesh_needs_its_motion_row(main_ds):
    """A fixed camera, the mesh moved by transform_mesh between two frames.  On the reference: with the rows of
    motion_rows the mesh's pixels find history that they do not find without a motion array; and the device
    gives the reference's bits both ways."""
    n = W * H
    identity = np.eye(3, 4)
    moved = np.hstack([np.eye(3), [[0.3], [0.0], [1.0]]])  # a fifth of the mesh's depth: far past depth_tolerance
    rows = motion_rows([identity, identity], [identity, moved])  # object 0: the primitives; object 1: the mesh
    rp = ReprojectParams(W, H, POSE_A, POSE_A, motion_count=2)
    plain = ReprojectParams(W, H, POSE_A, POSE_A)
    a, b = Frame(), Frame()
    with_rows = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    without = torch.zeros(8 * n, dtype=torch.float64, device="cuda")
    d_rows = torch.from_numpy(rows.copy()).cuda()
    torch.cuda.synchronize()
    try:
        main_ds.set_camera_pose(POSE_A)
        main_ds.transform_mesh(0, identity)
        a.render(main_ds, 0)
        main_ds.transform_mesh(0, moved)
        b.render(main_ds, SPP)
        args = (b.state.data_ptr(), b.features.data_ptr(), a.state.data_ptr(), a.features.data_ptr())
        reproject_device(rp, *args, with_rows.data_ptr(), motion_ptr=d_rows.data_ptr())
        reproject_device(plain, *args, without.data_ptr())
        torch.cuda.synchronize()
    finally:
        main_ds.transform_mesh(0, identity)
    mesh = b.records()["object"] == 1
    want_with, history_with = reference_of(rp, a, b, rows)
    want_without, history_without = reference_of(plain, a, b)
    print(f"mesh pixels {int(mesh.sum())}: history with rows {int(history_with[mesh].sum())}, "
          f"without {int(history_without[mesh].sum())}")
    assert mesh.sum() > 30
    assert (history_with & ~history_without)[mesh].sum() > 0
    assert history_with[mesh].sum() > history_without[mesh].sum()
    assert same_bits(with_rows.cpu().numpy(), want_with)
    assert same_bits(without.cpu().numpy(), want_without)
