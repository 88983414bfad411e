"""The denoiser on C3's scene, 1024 x 1024 at 4 spp: stage times for both load forms, and the sigma_colour sweep.

    python tools/denoise_bench.py [--size 1024] [--spp 4] [--rounds 5] [--warmup 1] [--out FILE]
    python tools/denoise_bench.py --sweep [--reference-spp 1024] [--out FILE]

Timing (one process, one device, one stream, HIP events, legs alternating inside each round, the median of the
rounds after the warm-up).  The stages run in the call's order on the frame's real data, each through
vr_denoise_stage_device: prepare; every iteration in the direct-load form and in the LDS form (both read the
same buffer and write the same result); finish.  Then the whole call in the library's choice and in either
form, and in the same rounds the tone map, the feature pass and the render of the frame.  Beside each stage:
the bytes it must move once (`floor_bytes`) and their time at the HBM rate a streaming kernel reaches
(6.3 TB/s); the 128 B per pixel of workspace at 1024 x 1024 fit the 256 MiB Infinity Cache, so a stage can
run under that figure.

--sweep: XYZ RMSE against a --reference-spp render of another seed after 5 iterations, over sigma_colour,
with VR_DENOISE_DEMODULATE on and off; `best` is the least.
Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from vanrijn_amd import scenes  # noqa: E402
from vanrijn_amd.render import (DenoiseParams, Tile, denoise_device, denoise_workspace_bytes,  # noqa: E402
                                render_features_device, render_tile_device, stream_check_error, tone_map_device)

SEED = 0x5EED0001
HBM_BYTES_PER_MS = 6.3e9  # 6.3 TB/s


class Frame:
    """The device arrays of one noisy frame with its features and albedo, rendered on `stream`."""

    def __init__(self, size, spp, stream):
        self.ds = scenes.main_scene().device_scene(0)
        self.size, self.spp, self.n, self.stream, self.sp = size, spp, size * size, stream, stream.cuda_stream
        self.tile = Tile(0, size, 0, size)
        with torch.cuda.stream(stream):
            self.state, self.albedo, self.out = (torch.zeros(self.n * 8, dtype=torch.float64, device="cuda") for _ in range(3))
            self.feat = torch.zeros(self.n * 8, dtype=torch.int64, device="cuda")  # vr_pixel_features, 64 B
            self.ws = torch.zeros(self.n * 16, dtype=torch.float64, device="cuda")
            self.rgb = torch.zeros(self.n * 3, dtype=torch.uint8, device="cuda")
        stream.synchronize()
        self.render()
        self.features()
        stream.synchronize()

    def render(self, state=None, spp=None, seed=SEED, timed=False):
        return render_tile_device(self.ds, self.tile, self.size, self.size, spp or self.spp, seed, 0,
                                  (self.state if state is None else state).data_ptr(), self.sp, timed=timed)

    def features(self):
        render_features_device(self.ds, self.tile, self.size, self.size, self.spp, SEED, 0, self.feat.data_ptr(),
                               self.albedo.data_ptr(), stream_ptr=self.sp)

    def denoise(self, p, stage=None):
        assert denoise_workspace_bytes(p) <= self.ws.numel() * 8
        denoise_device(p, self.state.data_ptr(), self.feat.data_ptr(), self.albedo.data_ptr(), self.out.data_ptr(),
                       self.ws.data_ptr(), stream_ptr=self.sp, stage=stage)


def colour_of(state, n):
    s = state[:4 * n].view(n, 4)
    return torch.where(s[:, 3:] != 0, s[:, :3] * (1.0 / s[:, 3:]), torch.zeros_like(s[:, :3]))


def timing(size, spp, rounds, warmup, demodulate):
    stream = torch.cuda.Stream()
    f = Frame(size, spp, stream)
    n = f.n
    forms = {loads: DenoiseParams(size, size, demodulate=demodulate, loads=loads) for loads in (None, "direct", "lds")}
    it = forms[None].iterations
    legs = [("prepare", lambda: f.denoise(forms["direct"], 0))]
    for i in range(it):
        legs.append((f"iteration{i}_direct", lambda i=i: f.denoise(forms["direct"], 1 + i)))
        legs.append((f"iteration{i}_lds", lambda i=i: f.denoise(forms["lds"], 1 + i)))
    legs.append(("finish", lambda: f.denoise(forms["direct"], it + 1)))
    legs += [("call", lambda: f.denoise(forms[None])), ("call_direct", lambda: f.denoise(forms["direct"])),
             ("call_lds", lambda: f.denoise(forms["lds"])),
             ("tone_map", lambda: tone_map_device(f.out.data_ptr(), n, f.rgb.data_ptr(), stream_ptr=f.sp)),
             ("features", f.features)]
    times = {k: [] for k, _ in legs}
    times.update(render=[], render_kernel=[], render_reduce=[])
    for r in range(warmup + rounds):
        events = []
        for leg, call in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            call()
            e1.record(stream)
            events.append((leg, e0, e1))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        st = f.render(timed=True)
        e1.record(stream)
        events.append(("render", e0, e1))
        stream.synchronize()
        if r >= warmup:
            for leg, a, b in events:
                times[leg].append(a.elapsed_time(b))
            times["render_kernel"].append(st["kernel_ms"])
            times["render_reduce"].append(st["reduce_ms"])
    stream_check_error(f.ds, f.sp)
    # bytes each stage must move once per pixel: reads + writes
    extra = 32 if demodulate else 0
    floor = {"prepare": 32 + 64 + extra + 96, "finish": 32 + extra + 64}
    for i in range(it):
        floor[f"iteration{i}_direct"] = floor[f"iteration{i}_lds"] = 32 + 32 + 8 + 32
    floor["call"] = floor["call_direct"] = floor["call_lds"] = floor["prepare"] + floor["finish"] + it * 104
    floor["tone_map"] = 32 + 3
    out = {"scene": "main_scene (C3)", "size": size, "spp": spp, "iterations": it, "demodulate": demodulate,
           "hbm_tb_per_s": 6.3, "legs": {}}
    for leg, t in times.items():
        out["legs"][leg] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4)}
        if leg in floor:
            out["legs"][leg]["floor_bytes"] = floor[leg] * n
            out["legs"][leg]["floor_ms"] = round(floor[leg] * n / HBM_BYTES_PER_MS, 4)
    med = {k: statistics.median(t) for k, t in times.items()}
    out["lds_over_direct"] = [round(med[f"iteration{i}_lds"] / med[f"iteration{i}_direct"], 4) for i in range(it)]
    out["call_over_render_kernel"] = round(med["call"] / med["render_kernel"], 4)
    return out


def sweep(size, spp, reference_spp):
    stream = torch.cuda.Stream()
    f = Frame(size, spp, stream)
    n = f.n
    with torch.cuda.stream(stream):
        truth = torch.zeros(n * 8, dtype=torch.float64, device="cuda")
    done = 0
    while done < reference_spp:  # in pieces, continued in place
        piece = min(256, reference_spp - done)
        render_tile_device(f.ds, f.tile, size, size, piece, SEED + 1, done, truth.data_ptr(), f.sp, accumulate=done > 0)
        done += piece
    stream.synchronize()
    stream_check_error(f.ds, f.sp)
    with torch.cuda.stream(stream):
        ref = colour_of(truth, n)

        def rmse(state):
            return float(torch.sqrt(torch.mean((colour_of(state, n) - ref) ** 2)))

        out = {"scene": "main_scene (C3)", "size": size, "spp": spp, "reference_spp": reference_spp, "iterations": 5,
               "rmse_noisy": rmse(f.state), "sweep": []}
        best = None
        for e in range(-6, 11):
            sigma = 2.0 ** (e / 2.0)
            row = {"sigma_colour": sigma}
            for demodulate in (False, True):
                f.denoise(DenoiseParams(size, size, iterations=5, sigma_colour=sigma, demodulate=demodulate))
                stream.synchronize()
                row["rmse_demodulated" if demodulate else "rmse"] = rmse(f.out)
            out["sweep"].append(row)
            if best is None or row["rmse"] < best["rmse"]:
                best = row
    out["best"] = best
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--demodulate", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("denoise_bench needs a GPU: no timing is taken without one")
    result = {"tool": "denoise_bench", "device": torch.cuda.get_device_name(0)}
    if a.sweep:
        result.update(sweep(a.size, a.spp, a.reference_spp))
    else:
        result.update(rounds=a.rounds, warmup=a.warmup)
        result.update(timing(a.size, a.spp, a.rounds, a.warmup, a.demodulate))
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
