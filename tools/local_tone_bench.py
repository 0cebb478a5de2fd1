"""Time local tone mapping in the finish.

(a) Slice, 7680x4320 output by default, colour matrix + 4096-interval tone table on the accumulators of the textured
``synth.make_burst`` merge: mfsr_finishLocalTone for RGB8 and RGBA8, each with the grid's corner columns staged in LDS
(MFSR_LOCAL_TONE_GRID=lds) and read through the cache (=cache), beside mfsr_finishRendered of the same format, which reads and
writes the same bytes.  The grid is the library's fit of the merge's own statistics (defaults).

(b) Statistics: mfsr_finishToneGridStats (matrix on, the default cell and 16 bins) on the textured accumulators and on a flat
image (one level plus noise of a few codes, weight 1), beside mfsr_finishStats, which makes the same 24 B/px read.

The calls of a leg take turns in one process; after --warmup calls, --iters calls of each as one batch of back-to-back calls
between two HIP events, --rounds times each.  Reported: the median microseconds, the spread, and GB/s of the bytes moved.

(c) Burst, 16 frames of 3840x2160 by default: ``BurstPipeline.process`` with ``set_local_tone`` (one statistics launch, one wait,
the host fit, the grid upload) against ``process`` without, both with the same fixed render description (RGB8, matrix, table);
wall clock from the first call to the synchronised stream, the two taking turns, --rounds times each.

Each step runs in a child process of its own under its own time limit (--limit seconds); a step that fails or runs out of time
ends the run.  One JSON line per step.

    python tools/local_tone_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5]

Record: profiles/local_tone_bench_4k16.txt.
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


def _turns(a, calls, moved):
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    return {"iters": iters, "rounds": rounds, **{name: _stat(v, moved[name]) for name, v in us.items()}}


def kernel_leg(a):
    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import (local_tone_defaults, local_tone_fit, local_tone_grid, render_row_bytes,
                                                           tone_lut_srgb)

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
    acc["flat"] = (0.5 + 0.002 * torch.randn(hrH, hrW, 3, generator=g, device=dev), torch.ones(hrH, hrW, 3, device=dev))
    lt = local_tone_defaults(hrW, hrH)
    gx, gy, gz = local_tone_grid(hrW, hrH, lt)
    m = (ctypes.c_float * 9)(*CCM)
    table = torch.zeros(gy, gx, gz, 2, dtype=torch.int64, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def grid_stats(fin, wt):
        L.finishToneGridStats(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, hrW, hrH, thr,
                              0, 0, hrW, hrH, m, ctypes.byref(lt), table.data_ptr(), stream())

    grid_stats(*acc["textured"])
    fit = local_tone_fit(table, hrW, hrH, lt)
    grid = fit.grid.to(dev)
    lut = tone_lut_srgb(4096).to(dev)
    out = {"leg": "kernel", "out_width": hrW, "out_height": hrH, "cell": lt.cell, "bins": lt.bins,
           "grid_bytes": 4 * gx * gy * gz, "pivot": fit.pivot, "gain_min": float(grid.min()), "gain_max": float(grid.max())}

    # (a) the slice beside the rendered finish
    calls, moved = {}, {}
    fin, wt = acc["textured"]
    for name, fmt in (("rgb8", capi.OUT_RGB8), ("rgba8", capi.OUT_RGBA8)):
        r = capi.Render()
        r.format, r.useMatrix, r.toneLut, r.toneSize = fmt, 1, lut.data_ptr(), lut.numel() - 1
        r.matrix = m
        rb = render_row_bytes(fmt, hrW)
        outbuf = torch.empty(hrH * rb, dtype=torch.uint8, device=dev)

        def rendered(r=r, rb=rb, outbuf=outbuf):
            L.finishRendered(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                             outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 0, 0, 0, hrW, hrH, stream())

        def local(form, r=r, rb=rb, outbuf=outbuf):
            os.environ["MFSR_LOCAL_TONE_GRID"] = form       # (read by the library at every call)
            L.finishLocalTone(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                              outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 0, 0, 0, hrW, hrH, grid.data_ptr(),
                              ctypes.byref(lt), stream())

        calls[f"finishRendered_{name}"] = rendered
        calls[f"finishLocalTone_{name}_grid_lds"] = lambda local=local: local("lds")
        calls[f"finishLocalTone_{name}_grid_cache"] = lambda local=local: local("cache")
        for k in (f"finishRendered_{name}", f"finishLocalTone_{name}_grid_lds", f"finishLocalTone_{name}_grid_cache"):
            moved[k] = (24 + rb // hrW) * hrW * hrH
    out["slice"] = _turns(a, calls, moved)
    for name in ("rgb8", "rgba8"):
        y = out["slice"][f"finishRendered_{name}"]["us_median"]
        out["slice"][f"{name}_over_rendered"] = {form: round(out["slice"][f"finishLocalTone_{name}_grid_{form}"]["us_median"] / y, 3)
                                                 for form in ("lds", "cache")}

    # (b) the statistics beside mfsr_finishStats
    par = capi.ImageStatsParams()
    par.useMatrix, par.lo, par.hi, par.chromaTol = 1, 64, 3967, 64
    par.matrix = m
    table2 = torch.zeros(capi.IMAGE_STATS_WORDS, dtype=torch.int64, device=dev)

    def image_stats(fin, wt):
        L.finishStats(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, hrW, hrH, thr, 0, 0,
                      hrW, hrH, ctypes.byref(par), table2.data_ptr(), stream())

    calls, moved = {}, {}
    for name, (fin2, wt2) in acc.items():
        calls[f"finishStats_{name}"] = lambda fin2=fin2, wt2=wt2: image_stats(fin2, wt2)
        calls[f"finishToneGridStats_{name}"] = lambda fin2=fin2, wt2=wt2: grid_stats(fin2, wt2)
        moved[f"finishStats_{name}"] = moved[f"finishToneGridStats_{name}"] = 24 * hrW * hrH
    out["stats"] = _turns(a, calls, moved)
    out["stats"]["grid_over_image_stats"] = {
        k: round(out["stats"][f"finishToneGridStats_{k}"]["us_median"] / out["stats"][f"finishStats_{k}"]["us_median"], 3) for k in acc}
    out["stats"]["flat_over_textured"] = round(out["stats"]["finishToneGridStats_flat"]["us_median"]
                                               / out["stats"]["finishToneGridStats_textured"]["us_median"], 3)
    print(json.dumps(out), flush=True)


def burst_leg(a):
    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import tone_lut_srgb

    pipe, frames, _ = _burst(a)
    pipe.set_render(format=capi.OUT_RGB8, matrix=CCM, tone_lut=tone_lut_srgb(4096))

    def plain():
        pipe.set_local_tone(None)

    def local():
        pipe.set_local_tone(0.5, 0.25)

    us = {"process_rendered": [], "process_local_tone": []}
    for setup in (plain, local):
        setup()
        for _ in range(2):
            pipe.process(frames)
    torch.cuda.synchronize()
    for _ in range(max(a.rounds, 1)):
        for name, setup in (("process_rendered", plain), ("process_local_tone", local)):
            setup()                             # (the description and its buffers: outside the timed region)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.process(frames)
            torch.cuda.synchronize()
            us[name].append((time.perf_counter() - t0) * 1e6)
    res = pipe.local_tone_result
    out = {"leg": "burst", "width": a.width, "height": a.height, "frames": a.frames, **{k: _stat(v) for k, v in us.items()},
           "pivot": res.pivot, "gain_min": res.minGain, "gain_max": res.maxGain, "status": res.status}
    out["local_minus_rendered_us"] = round(out["process_local_tone"]["us_median"] - out["process_rendered"]["us_median"], 1)
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
            raise SystemExit(f"local_tone_bench: step {leg} ended with status {rc}")


if __name__ == "__main__":
    main()
