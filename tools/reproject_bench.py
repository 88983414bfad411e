"""The temporal reprojection on C3's scene, 1024 x 1024 at 4 spp: its time beside the frame's other stages, and
the sweep of its three defaults.

    python tools/reproject_bench.py [--size 1024] [--spp 4] [--rounds 7] [--warmup 2] [--reps 20] [--out FILE]
    python tools/reproject_bench.py --sweep [--poses 6] [--reference-spp 1024] [--out FILE]

Timing (one process, one device, one stream, HIP events around `reps` back-to-back calls of a leg, legs
alternating inside each round, the median of the rounds after the warm-up, per call).  Frame A is rendered from
the scene's pose, frame B after a camera step of about --step-pixels pixels; the reprojection of B over A is
timed with the default parameters, without VR_REPROJECT_MATCH_OBJECT, and from an unchanged pose (the same-view
shortcut: one tap).  In the same rounds: one denoiser iteration (stage 1) and the feature pass of frame B, the
render of frame B (its kernel time from the library's own events), and a torch device-to-device copy that
moves as many bytes as the reprojection must -- the yardstick for a streaming kernel, not the code under test.
`floor_bytes` is what the rule makes the kernel move once per pixel: its own sums record (32 B) and feature
record (64 B; 48 B without the object id), every previous sums record and feature record once (32 + 64 B:
the four footprints that share a record are left to the caches), and the output record (64 B).

--sweep: a path of --poses poses, each a step of about --step-pixels pixels from the last.  Frame 0 starts the
history; every later frame is reprojected over the history and becomes it.  For each value of one parameter,
the others at their defaults: the XYZ RMSE over the hit pixels against a --reference-spp render of each pose
with another seed (the mean over the path's poses), and the share of hit pixels that received history.
`frame_alone` is the same RMSE of the 4-spp frames themselves.
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
from vanrijn_amd.render import (DenoiseParams, ReprojectParams, Tile, denoise_device, denoise_workspace_bytes,  # noqa: E402
                                render_features_device, render_tile_device, reproject_device, stream_check_error)
from vanrijn_amd.scene import CameraPose, look_at  # noqa: E402

SEED = 0x5EED0001
FLOOR_BYTES = {"reproject": 32 + 64 + 32 + 64 + 64, "reproject_no_match": 32 + 48 + 32 + 48 + 64,
               "reproject_same_view": 32 + 64 + 32 + 64 + 64, "denoise_iteration": 32 + 32 + 8 + 32}


def path_pose(i, size, step_pixels):
    """Pose i of the path: the eye slides right and up by `step_pixels` pixels' worth of parallax at the depth
    of the scene (5) per pose and keeps looking at the point 5 ahead of pose 0; pose 0 is the scene's own."""
    x, y, z = scenes.CAMERA_LOCATION
    if i == 0:
        return CameraPose(location=(x, y, z))
    step = step_pixels * (1.0 / size) * 5.0  # the image's shorter side spans a film length of 1 at film distance 1
    return look_at((x + 0.8 * step * i, y + 0.6 * step * i, z), (x, y, z + 5.0))


class Frames:
    """The scene, a stream, and per pose the device arrays of one frame: state and feature records."""

    def __init__(self, size, spp, stream):
        self.ds = scenes.main_scene().device_scene(0)
        self.size, self.spp, self.n, self.stream, self.sp = size, spp, size * size, stream, stream.cuda_stream
        self.tile = Tile(0, size, 0, size)

    def zeros(self, doubles=8):
        with torch.cuda.stream(self.stream):
            return torch.zeros(self.n * doubles, dtype=torch.float64, device="cuda")

    def render(self, pose, index, state, timed=False, spp=None, seed=SEED, first_sample=None, accumulate=False):
        self.ds.set_camera_pose(pose)
        return render_tile_device(self.ds, self.tile, self.size, self.size, spp or self.spp, seed,
                                  self.spp * index if first_sample is None else first_sample, state.data_ptr(), self.sp,
                                  timed=timed, accumulate=accumulate)

    def features(self, pose, index, feat):
        self.ds.set_camera_pose(pose)
        render_features_device(self.ds, self.tile, self.size, self.size, self.spp, SEED, self.spp * index, feat.data_ptr(),
                               None, stream_ptr=self.sp)


def timing(size, spp, rounds, warmup, reps, step_pixels):
    stream = torch.cuda.Stream()
    f = Frames(size, spp, stream)
    n = f.n
    pose_a, pose_b = path_pose(0, size, step_pixels), path_pose(1, size, step_pixels)
    state_a, state_b, out, clean = f.zeros(), f.zeros(), f.zeros(), f.zeros()
    feat_a, feat_b = f.zeros(), f.zeros()  # vr_pixel_features, 64 B
    dp = DenoiseParams(size, size)
    ws = f.zeros(denoise_workspace_bytes(dp) // (8 * n))
    f.render(pose_a, 0, state_a)
    f.features(pose_a, 0, feat_a)
    f.render(pose_b, 1, state_b)
    f.features(pose_b, 1, feat_b)
    denoise_device(dp, state_b.data_ptr(), feat_b.data_ptr(), None, clean.data_ptr(), ws.data_ptr(), stream_ptr=f.sp)
    stream.synchronize()
    moved = ReprojectParams(size, size, pose_b, pose_a)
    no_match = ReprojectParams(size, size, pose_b, pose_a, match_object=False)
    still = ReprojectParams(size, size, pose_b, pose_b)
    copy_bytes = FLOOR_BYTES["reproject"] * n
    with torch.cuda.stream(stream):
        src = torch.zeros(copy_bytes // 16, dtype=torch.float64, device="cuda")  # read once and written once
        dst = torch.empty_like(src)

    def reproject(p):
        reproject_device(p, state_b.data_ptr(), feat_b.data_ptr(), state_a.data_ptr(), feat_a.data_ptr(), out.data_ptr(),
                         stream_ptr=f.sp)

    def copy():
        with torch.cuda.stream(stream):
            dst.copy_(src, non_blocking=True)

    legs = [("reproject", lambda: reproject(moved)), ("device_copy", copy),
            ("reproject_no_match", lambda: reproject(no_match)), ("reproject_same_view", lambda: reproject(still)),
            ("denoise_iteration", lambda: denoise_device(dp, state_b.data_ptr(), feat_b.data_ptr(), None, clean.data_ptr(),
                                                         ws.data_ptr(), stream_ptr=f.sp, stage=1)),
            ("features", lambda: f.features(pose_b, 1, feat_b))]
    times = {k: [] for k, _ in legs}
    times.update(render=[], render_kernel=[])
    for r in range(warmup + rounds):
        events = []
        for leg, call in legs:
            count = 1 if leg == "features" else reps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(count):
                call()
            e1.record(stream)
            events.append((leg, e0, e1, count))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = f.render(pose_b, 1, state_b, timed=True)
        e1.record(stream)
        events.append(("render", e0, e1, 1))
        stream.synchronize()
        if r >= warmup:
            for leg, a, b, count in events:
                times[leg].append(a.elapsed_time(b) / count)
            times["render_kernel"].append(st["kernel_ms"])
    stream_check_error(f.ds, f.sp)
    reproject(moved)
    with torch.cuda.stream(stream):
        hit = (feat_b.view(torch.int64).view(n, 8)[:, 5] & 0xFFFFFFFF) > 0  # hits: the low half of the sixth word
        got = out[:4 * n].view(n, 4)[:, 3] > state_b[:4 * n].view(n, 4)[:, 3]
        share = float((got & hit).sum()) / max(int(hit.sum()), 1)
    result = {"scene": "main_scene (C3)", "size": size, "spp": spp, "step_pixels": step_pixels, "reps": reps,
              "history_share": round(share, 4), "legs": {}}
    med = {k: statistics.median(t) for k, t in times.items()}
    for leg, t in times.items():
        row = {"ms_median": round(med[leg], 5), "ms_min": round(min(t), 5), "ms_max": round(max(t), 5)}
        bytes_moved = copy_bytes if leg == "device_copy" else FLOOR_BYTES.get(leg, 0) * n
        if bytes_moved:
            row["floor_bytes_per_pixel"] = bytes_moved // n
            row["tb_per_s"] = round(bytes_moved / (med[leg] * 1e-3) / 1e12, 3)
        result["legs"][leg] = row
    result["reproject_over_copy"] = round(med["reproject"] / med["device_copy"], 4)
    result["reproject_over_render_kernel"] = round(med["reproject"] / med["render_kernel"], 4)
    return result


def colour_of(state, n):
    s = state[:4 * n].view(n, 4)
    return torch.where(s[:, 3:] != 0, s[:, :3] * (1.0 / s[:, 3:]), torch.zeros_like(s[:, :3]))


def sweep(size, spp, poses, reference_spp, step_pixels):
    stream = torch.cuda.Stream()
    f = Frames(size, spp, stream)
    n = f.n
    path = [path_pose(i, size, step_pixels) for i in range(poses)]
    states, feats, truths, hits = [], [], [], []
    for i, pose in enumerate(path):
        state, feat, truth = f.zeros(), f.zeros(), f.zeros()
        f.render(pose, i, state)
        f.features(pose, i, feat)
        done = 0
        while done < reference_spp:  # in pieces, continued in place
            piece = min(256, reference_spp - done)
            f.render(pose, i, truth, spp=piece, seed=SEED + 1, first_sample=done, accumulate=done > 0)
            done += piece
        stream.synchronize()
        stream_check_error(f.ds, f.sp)
        with torch.cuda.stream(stream):
            truths.append(colour_of(truth, n))
            hits.append((feat.view(torch.int64).view(n, 8)[:, 5] & 0xFFFFFFFF) > 0)
        states.append(state)
        feats.append(feat)
        del truth
    history = [f.zeros(), f.zeros()]

    def rmse(state, i):
        d = (colour_of(state, n) - truths[i])[hits[i]]
        return float(torch.sqrt(torch.mean(d * d)))

    def run(**changed):
        errors, shares = [], []
        with torch.cuda.stream(stream):
            history[0].copy_(states[0])
        for i in range(1, poses):
            p = ReprojectParams(size, size, path[i], path[i - 1], **changed)
            src, dst = history[(i - 1) & 1], history[i & 1]
            reproject_device(p, states[i].data_ptr(), feats[i].data_ptr(), src.data_ptr(), feats[i - 1].data_ptr(),
                             dst.data_ptr(), stream_ptr=f.sp)
            stream.synchronize()
            with torch.cuda.stream(stream):
                errors.append(rmse(dst, i))
                got = dst[:4 * n].view(n, 4)[:, 3] > states[i][:4 * n].view(n, 4)[:, 3]
                shares.append(float((got & hits[i]).sum()) / max(int(hits[i].sum()), 1))
        return {"rmse": statistics.mean(errors), "rmse_last": errors[-1], "history_share": statistics.mean(shares)}

    with torch.cuda.stream(stream):
        alone = statistics.mean(rmse(states[i], i) for i in range(1, poses))
    defaults = ReprojectParams(size, size, path[0], path[0])
    out = {"scene": "main_scene (C3)", "size": size, "spp": spp, "poses": poses, "step_pixels": step_pixels,
           "reference_spp": reference_spp, "frame_alone": alone,
           "defaults": {"depth_tolerance": defaults.depth_tolerance, "normal_tolerance": defaults.normal_tolerance,
                        "max_history_weight": defaults.max_history_weight, "match_object": bool(defaults.flags & 1),
                        **run()},
           "no_match_object": run(match_object=False), "sweep": {}}
    grids = {"depth_tolerance": [0.0125, 0.025, 0.05, 0.1, 0.2, 0.4],
             "normal_tolerance": [0.0625, 0.125, 0.25, 0.5, 1.0, 2.0],
             "max_history_weight": [4.0, 8.0, 16.0, 32.0, 64.0, 128.0, math.inf]}
    for name, values in grids.items():
        rows = [dict({name: v}, **run(**{name: v})) for v in values]
        out["sweep"][name] = rows
        out.setdefault("best", {})[name] = min(rows, key=lambda r: r["rmse"])[name]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-pixels", type=float, default=1.0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--poses", type=int, default=6)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reproject_bench needs a GPU: no timing is taken without one")
    result = {"tool": "reproject_bench", "device": torch.cuda.get_device_name(0)}
    if a.sweep:
        result.update(sweep(a.size, a.spp, a.poses, a.reference_spp, a.step_pixels))
    else:
        result.update(rounds=a.rounds, warmup=a.warmup)
        result.update(timing(a.size, a.spp, a.rounds, a.warmup, a.reps, a.step_pixels))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
