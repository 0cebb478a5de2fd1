"""Time the block statistics of noise calibration (mfsr_noiseStats, csrc/noise.hip) beside the sharpness score
(mfsr_frameSharpness, the yardstick: it reads the same frames): 16 frames of 3840x2160 RGGB by default, three bursts -- a
textured one (the synth.make_burst scene: histogram updates spread over many counters), a flat one (the synth.make_chart_burst
chart: a wave's updates concentrate on a few counters) and a constant one (every update of a position on ONE counter).  After
--warmup calls, --iters calls of each are timed with HIP events on the current stream, one by one (each includes the host's
enqueue latency) and as one batch of back-to-back calls (the queue stays full: the device time of a call, the three memsets of
the tables included); prints one JSON line per burst with the microseconds and the effective rate (the raw bytes of the frames
over the time).  The kernels alone: ``rocprofv3 --kernel-trace --stats -- python tools/noise_bench.py``.

With --parent DIR (a built checkout of the parent commit) it first runs ``bench.py --gpus 1 --steps 10 --warmup 3`` of this
tree and of that one taking turns, --ab-rounds times each, every run in a child process of its own, and prints their JSON
lines: the default path must not have moved.

    python tools/noise_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5] [--parent DIR]

Record: profiles/noise_bench_4k16.txt.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py of both trees taking turns first")
    ap.add_argument("--ab-rounds", type=int, default=2)
    a = ap.parse_args()
    if a.parent:
        bench_turns(os.path.abspath(a.parent), a.ab_rounds)

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import default_config, noise_defaults, noise_fit, sharpness_rect
    from multi_frame_super_resolution_amd.synth import make_burst, make_chart_burst

    W, H, N = a.width, a.height, a.frames
    cfg = default_config(W, H, N, 2, False)
    d = noise_defaults(cfg)
    srect = sharpness_rect(cfg)
    dev = "cuda:0"
    bursts = {
        "textured": make_burst(W, H, N, device=dev)[0],
        "flat": make_chart_burst(W, H, N, 1e-4, 1e-6, device=dev),
        "constant": [torch.full((H, W), 1000, dtype=torch.int16, device=dev) for _ in range(N)],
    }
    hist = torch.zeros(4, 64, 272, dtype=torch.int32, device=dev)
    level_sum = torch.zeros(4, 64, dtype=torch.int64, device=dev)
    count = torch.zeros(4, 64, dtype=torch.int64, device=dev)
    sums = torch.zeros(N, dtype=torch.int64, device=dev)
    I4 = ctypes.c_int32 * 4
    cfa, black, r4, s4 = I4(*cfg.cfa), I4(*d.black), I4(*d.rect), I4(*srect)
    L = capi.lib()

    nbytes = 2 * W * H * N
    for name, frames in bursts.items():
        ptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in frames])

        def stats():
            L.noiseStats(N, ptrs, 2 * W, W, H, black, d.sat, r4, hist.data_ptr(), level_sum.data_ptr(), count.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)

        def sharp():
            L.frameSharpness(N, ptrs, 2 * W, W, H, cfa, 0, s4, sums.data_ptr(), torch.cuda.current_stream().cuda_stream)

        s_med, s_min, s_batch, iters = timed(sharp, max(a.warmup, 1), max(a.iters, 20))
        n_med, n_min, n_batch, _ = timed(stats, max(a.warmup, 1), max(a.iters, 20))
        alpha, beta, status, points = noise_fit((hist, level_sum, count), cfg)
        print(json.dumps({
            "burst": name, "width": W, "height": H, "frames": N, "rect": list(d.rect), "black": list(d.black), "sat": d.sat,
            "iters": iters, "bytes": nbytes,
            "stats_us_batched": round(n_batch, 2), "stats_tb_per_s_batched": round(nbytes / n_batch / 1e6, 3),
            "stats_us_single_median": round(n_med, 2), "stats_us_single_min": round(n_min, 2),
            "sharpness_us_batched": round(s_batch, 2), "sharpness_tb_per_s_batched": round(nbytes / s_batch / 1e6, 3),
            "sharpness_us_single_median": round(s_med, 2), "stats_over_sharpness_rate": round(s_batch / n_batch, 3),
            "blocks": int(count.sum().item()) // 4, "nonzero_counters": int((hist != 0).sum().item()),
            "fit": {"alpha": alpha, "beta": beta, "status": status, "points": points},
        }), flush=True)


if __name__ == "__main__":
    main()
