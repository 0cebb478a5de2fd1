"""Time the measurement and the application of exposure matching (mfsr_frameLevels / mfsr_applyGains, csrc/exposure.hip) beside
the sharpness score (mfsr_frameSharpness, the yardstick: it reads the same frames): 16 frames of 3840x2160 RGGB by default,
12-bit noise, default levels (black 256, sat = maxValue = 4095), every frame but the first gets a gain.  After --warmup calls,
--iters calls of each are timed with HIP events on the current stream, one by one (each includes the host's enqueue latency)
and as one batch of back-to-back calls (the queue stays full: the device time of a call; for the two measurements that
includes the memset of their sums); prints one JSON line with the microseconds and the effective rates (levels and sharpness:
the raw bytes of the frames over the time; apply: a read and a write of the frames that get a gain).  The kernels alone:
``rocprofv3 --kernel-trace --stats -- python tools/exposure_bench.py``.

With --parent DIR (a built checkout of the parent commit) it first runs ``bench.py --gpus 1 --steps 10 --warmup 3`` of this
tree and of that one taking turns, --ab-rounds times each, every run in a child process of its own, and prints their JSON
lines: the default path must not have moved.

    python tools/exposure_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5] [--parent DIR]

Record: profiles/exposure_bench_4k16.txt.
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
    from multi_frame_super_resolution_amd.pipeline import default_config, exposure_defaults, sharpness_rect

    W, H, N = a.width, a.height, a.frames
    cfg = default_config(W, H, N, 2, False)
    d = exposure_defaults(cfg)
    rect = sharpness_rect(cfg)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    frames = [torch.randint(0, 4096, (H, W), generator=g, device="cuda:0", dtype=torch.int32).to(torch.int16) for _ in range(N)]
    levels = torch.zeros(N, 5, dtype=torch.int64, device="cuda:0")
    sums = torch.zeros(N, dtype=torch.int64, device="cuda:0")
    ptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in frames])
    I4 = ctypes.c_int32 * 4
    cfa, black, r4 = I4(*cfg.cfa), I4(*d.black), I4(*rect)
    # gains that alternate about 1.0, so that repeated calls neither saturate nor empty the frames; the first frame is the reference
    gains = (ctypes.c_int32 * (3 * N))(*[v for k in range(N) for v in [65536 + (300 if k % 2 else -300)] * 3])
    status = (ctypes.c_int32 * N)(*([1] + [0] * (N - 1)))
    L = capi.lib()

    def measure():
        L.frameLevels(N, ptrs, 2 * W, W, H, black, d.sat, r4, levels.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def apply():
        L.applyGains(N, ptrs, 2 * W, W, H, cfa, 0, black, d.sat, d.max_value, gains, status, torch.cuda.current_stream().cuda_stream)

    def sharp():
        L.frameSharpness(N, ptrs, 2 * W, W, H, cfa, 0, r4, sums.data_ptr(), torch.cuda.current_stream().cuda_stream)

    s_med, s_min, s_batch, iters = timed(sharp, max(a.warmup, 1), max(a.iters, 20))
    m_med, m_min, m_batch, _ = timed(measure, max(a.warmup, 1), max(a.iters, 20))
    head = levels[:2].cpu().tolist()
    a_med, a_min, a_batch, _ = timed(apply, max(a.warmup, 1), max(a.iters, 20))
    nbytes = 2 * W * H * N
    abytes = 2 * 2 * W * H * (N - 1)
    print(json.dumps({
        "width": W, "height": H, "frames": N, "rect": list(rect), "black": list(d.black), "sat": d.sat, "iters": iters, "bytes": nbytes,
        "levels_us_batched": round(m_batch, 2), "levels_tb_per_s_batched": round(nbytes / m_batch / 1e6, 3),
        "levels_us_single_median": round(m_med, 2), "levels_us_single_min": round(m_min, 2),
        "sharpness_us_batched": round(s_batch, 2), "sharpness_tb_per_s_batched": round(nbytes / s_batch / 1e6, 3),
        "sharpness_us_single_median": round(s_med, 2), "levels_over_sharpness_rate": round(s_batch / m_batch, 3),
        "apply_frames": N - 1, "apply_bytes": abytes, "apply_us_batched": round(a_batch, 2),
        "apply_tb_per_s_batched": round(abytes / a_batch / 1e6, 3), "apply_us_single_median": round(a_med, 2),
        "apply_us_single_min": round(a_min, 2), "levels_head": head,
    }), flush=True)


if __name__ == "__main__":
    main()
