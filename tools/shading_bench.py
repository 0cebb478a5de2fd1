"""Time the application and the measurement of lens-shading correction (mfsr_applyShading / mfsr_shadingStats, csrc/shading.hip)
beside their yardsticks in the same run: mfsr_applyGains on the same frames (the same bytes in and out) and mfsr_frameLevels
(the same bytes in).  16 frames of 3840x2160 RGGB by default, 12-bit noise, default levels, cell 64; the gain map alternates
about 1.0 from call to call, so that repeated calls neither saturate nor empty the frames.  After --warmup calls, --iters calls
of each are timed with HIP events on the current stream as one batch of back-to-back calls (the queue stays full: the device
time of a call; for the two measurements that includes the memsets of their sums), --rounds times each, the four taking turns;
prints one JSON line with the median microseconds, the spread (min .. max over the rounds) and the effective rates (apply: a
read and a write of the frames; statistics: a read).  The kernels alone:
``rocprofv3 --kernel-trace --stats -- python tools/shading_bench.py``.

    python tools/shading_bench.py [--width 3840 --height 2160 --frames 16 --cell 64 --iters 50 --warmup 5 --rounds 5] [--parent DIR]

Record: profiles/shading_bench_4k16.txt.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools._stage_bench import bench_turns, timed


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--cell", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py of both trees taking turns first")
    ap.add_argument("--ab-rounds", type=int, default=2)
    a = ap.parse_args()
    if a.parent:
        bench_turns(os.path.abspath(a.parent), a.ab_rounds)

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import default_config, shading_defaults, shading_grid, sharpness_rect

    W, H, N = a.width, a.height, a.frames
    cfg = default_config(W, H, N, 2, False)
    d = shading_defaults(cfg)
    gw, gh = shading_grid(cfg, a.cell)
    rect = sharpness_rect(cfg)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    frames = [torch.randint(0, 4096, (H, W), generator=g, device="cuda:0", dtype=torch.int32).to(torch.int16) for _ in range(N)]
    ptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in frames])
    I4 = ctypes.c_int32 * 4
    cfa, black, r4 = I4(*cfg.cfa), I4(*d.black), I4(*rect)
    # two maps about 1.0, a smooth falloff on top: up and down in turn
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, gh), torch.linspace(-1, 1, gw), indexing="ij")
    fall = (300.0 * (xx * xx + yy * yy)).to(torch.int32)[None].expand(4, -1, -1)
    maps = [(65536 + 300 + fall).contiguous().to("cuda:0"), (65536 - 300 - fall).contiguous().to("cuda:0")]
    gains = (ctypes.c_int32 * (3 * N))(*[v for k in range(N) for v in [65536 + (300 if k % 2 else -300)] * 3])
    status = (ctypes.c_int32 * N)(*([0] * N))
    sums = torch.zeros(4, gh, gw, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(gh, gw, dtype=torch.int64, device="cuda:0")
    levels = torch.zeros(N, 5, dtype=torch.int64, device="cuda:0")
    L = capi.lib()
    turn = [0]

    def shade():
        turn[0] ^= 1
        L.applyShading(N, ptrs, 2 * W, W, H, maps[turn[0]].data_ptr(), a.cell, black, d.max_value, torch.cuda.current_stream().cuda_stream)

    def gain():
        L.applyGains(N, ptrs, 2 * W, W, H, cfa, 0, black, d.sat, d.max_value, gains, status, torch.cuda.current_stream().cuda_stream)

    def stats():
        L.shadingStats(N, ptrs, 2 * W, W, H, a.cell, black, d.sat, sums.data_ptr(), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def lev():
        L.frameLevels(N, ptrs, 2 * W, W, H, black, d.sat, r4, levels.data_ptr(), torch.cuda.current_stream().cuda_stream)

    calls = {"apply_shading": shade, "apply_gains": gain, "shading_stats": stats, "frame_levels": lev}
    us = {name: [] for name in calls}
    for _ in range(max(a.rounds, 1)):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), max(a.iters, 20), singles=False)[2])
    nbytes = 2 * W * H * N
    out = {"width": W, "height": H, "frames": N, "cell": a.cell, "grid": [gw, gh], "iters": max(a.iters, 20), "rounds": max(a.rounds, 1),
           "frame_bytes": nbytes}
    for name, v in us.items():
        moved = 2 * nbytes if name.startswith("apply") else nbytes
        med = statistics.median(v)
        out[name] = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                     "tb_per_s": round(moved / med / 1e6, 3)}
    out["apply_shading_over_apply_gains"] = round(out["apply_shading"]["us_median"] / out["apply_gains"]["us_median"], 3)
    out["shading_stats_over_frame_levels"] = round(out["shading_stats"]["us_median"] / out["frame_levels"]["us_median"], 3)
    out["counts_total"] = int(counts.sum().item())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
