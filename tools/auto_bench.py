"""Time the image statistics and the auto-rendered burst.

(a) Kernel, 7680x4320 output by default: mfsr_finishStats (matrix on, chromaTol 64) on the accumulators of the textured
``synth.make_burst`` merge, on a flat image (one level plus noise of a few codes: a handful of histogram bins take every add)
and on a constant image (every lane of every wave on one counter), and in the same process mfsr_finishRendered to RGB8 with a
colour matrix and a 4096-interval tone table on the textured accumulators: it reads the same 24 bytes per pixel and is the
yardstick.  The calls take turns; after --warmup calls, --iters calls of each as one batch of back-to-back calls between two HIP
events, --rounds times each.  Reported: the median microseconds, the spread and GB/s of the 24 bytes per pixel read (the
yardstick: 27 with its output).  The fallback image of the kernel legs is the merge's own float image at the raw size.

(b) Burst, 16 frames of 3840x2160 by default: ``BurstPipeline.process_auto`` (two white-balance passes, one tone pass: three
statistics launches, three waits, one table upload) against ``process`` with a fixed render description of the same kind
(RGB8, matrix, table), wall clock from the first call to the synchronised stream, the two taking turns, --rounds times each.

Each of the two steps runs in a child process of its own under its own time limit (--limit seconds); a step that fails or runs
out of time ends the run.  One JSON line per step.

    python tools/auto_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5]

Record: profiles/auto_bench_4k16.txt.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools._stage_bench import timed

CCM = [1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56]


def _stat(v, moved=None):
    med = statistics.median(v)
    out = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    if moved is not None:
        out["gb_per_s"] = round(moved / med / 1e3, 1)
    return out


def _burst(a):
    import torch
    from multi_frame_super_resolution_amd import synth
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config

    W, H, N = a.width, a.height, a.frames
    frames, _, _ = synth.make_burst(W, H, N, seed=29, device="cpu")
    dev = torch.device("cuda:0")
    cfg = default_config(W, H, N, 2, False)
    cfg.applyGamma = 0
    return BurstPipeline(cfg, dev), [f.to(dev) for f in frames], dev


def kernel_leg(a):
    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import render_row_bytes, tone_lut_srgb

    W, H = a.width, a.height
    hrW, hrH = 2 * W, 2 * H
    pipe, frames, dev = _burst(a)
    img, _ = pipe.process(frames)
    L = capi.lib()
    thr = float(pipe.cfg.weightThreshold)
    fb = torch.nn.functional.avg_pool2d(img.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0).contiguous()
    acc = {"textured": (pipe.img_out.clone(), pipe.total_weights.clone())}
    pipe.close()
    del pipe, frames, img
    g = torch.Generator(device="cuda:0").manual_seed(1)
    ones = torch.ones(hrH, hrW, 3, device=dev)
    acc["flat"] = (0.5 + 0.002 * torch.randn(hrH, hrW, 3, generator=g, device=dev), ones)
    acc["constant"] = (torch.full((hrH, hrW, 3), 0.5, device=dev), ones)
    table = torch.zeros(capi.IMAGE_STATS_WORDS, dtype=torch.int64, device=dev)
    par = capi.ImageStatsParams()
    par.useMatrix, par.lo, par.hi, par.chromaTol = 1, 64, 3967, 64
    par.matrix = (ctypes.c_float * 9)(*CCM)
    lut = tone_lut_srgb(4096).to(dev)
    r = capi.Render()
    r.format, r.useMatrix, r.toneLut, r.toneSize = capi.OUT_RGB8, 1, lut.data_ptr(), lut.numel() - 1
    r.matrix = (ctypes.c_float * 9)(*CCM)
    rb = render_row_bytes(capi.OUT_RGB8, hrW)
    outbuf = torch.empty(hrH * rb, dtype=torch.uint8, device=dev)
    calls, moved = {}, {}

    def stats(fin, wt):
        L.finishStats(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, hrW, hrH, thr, 0, 0,
                      hrW, hrH, ctypes.byref(par), table.data_ptr(), torch.cuda.current_stream().cuda_stream)

    for name, (fin, wt) in acc.items():
        calls[f"finishStats_{name}"] = lambda fin=fin, wt=wt: stats(fin, wt)
        moved[f"finishStats_{name}"] = 24 * hrW * hrH

    def rendered():
        fin, wt = acc["textured"]
        L.finishRendered(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                         outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 0, 0, 0, hrW, hrH,
                         torch.cuda.current_stream().cuda_stream)

    calls["finishRendered_rgb8_ccm_lut"] = rendered
    moved["finishRendered_rgb8_ccm_lut"] = 27 * hrW * hrH
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    out = {"leg": "kernel", "out_width": hrW, "out_height": hrH, "iters": iters, "rounds": rounds,
           **{name: _stat(v, moved[name]) for name, v in us.items()}}
    y = out["finishRendered_rgb8_ccm_lut"]["us_median"]
    out["stats_over_yardstick"] = {k: round(out[f"finishStats_{k}"]["us_median"] / y, 3) for k in acc}
    out["flat_over_textured"] = round(out["finishStats_flat"]["us_median"] / out["finishStats_textured"]["us_median"], 3)
    print(json.dumps(out), flush=True)


def burst_leg(a):
    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import tone_lut_srgb

    pipe, frames, _ = _burst(a)
    fixed = dict(format=capi.OUT_RGB8, matrix=CCM, tone_lut=tone_lut_srgb(4096))

    def run_fixed():
        pipe.set_render(**fixed)
        pipe.process(frames)

    def run_auto():
        pipe.process_auto(frames, format=capi.OUT_RGB8, matrix=CCM)

    us = {"process_fixed_render": [], "process_auto": []}
    for fn in (run_fixed, run_auto):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    for _ in range(max(a.rounds, 1)):
        for name, fn in (("process_fixed_render", run_fixed), ("process_auto", run_auto)):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6)
    res = pipe.auto_result
    out = {"leg": "burst", "width": a.width, "height": a.height, "frames": a.frames, **{k: _stat(v) for k, v in us.items()},
           "gains": [round(float(v), 6) for v in res.gains], "black": res.black, "white": res.white, "gamma": res.gamma}
    out["auto_minus_fixed_us"] = round(out["process_auto"]["us_median"] - out["process_fixed_render"]["us_median"], 1)
    pipe.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--leg", choices=["kernel", "burst"], help="run this step in this process (what the parent starts)")
    a = ap.parse_args()
    if a.leg:
        return (kernel_leg if a.leg == "kernel" else burst_leg)(a)
    for leg in ("kernel", "burst"):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--leg", leg]
        for k in ("width", "height", "frames", "iters", "warmup", "rounds"):
            cmd += [f"--{k}", str(getattr(a, k))]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:     # nothing more is started on the device after a step that failed or ran out of time
            raise SystemExit(f"auto_bench: step {leg} ended with status {rc}")


if __name__ == "__main__":
    main()
