"""Time the defect vote and the repair of a burst (mfsr_detectDefects / mfsr_repairDefects, csrc/defect.hip): 16 frames of
3840x2160 RGGB by default, 12-bit noise with 300 stuck pixels, default parameters.  After --warmup calls, --iters calls of
each are timed with HIP events on the current stream, one by one (each includes the host's enqueue latency) and as one batch
of back-to-back calls (the queue stays full: the device time of a call; for the vote that includes the 8-byte memset of the
counters); prints one JSON line with the median microseconds and the effective rate (the raw bytes of the frames plus the map
over the time).  The kernels alone: ``rocprofv3 --kernel-trace --stats -- python tools/defect_bench.py``.

    python tools/defect_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5]

Record: profiles/defect_bench_4k16.txt (beside tools/select_bench.py from the same run: it reads the same bytes).
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

from tools._stage_bench import timed


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import default_config, defect_defaults

    W, H, N = a.width, a.height, a.frames
    cfg = default_config(W, H, N, 2, False)
    threshold, spread, votes = defect_defaults(cfg, N)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    frames = [torch.randint(1000, 1040, (H, W), generator=g, device="cuda:0", dtype=torch.int32).to(torch.int16) for _ in range(N)]
    # 300 distinct cells of an 8 x 8 grid plus a jitter in [0, 3): no two stuck pixels are same-colour neighbours
    cells = torch.randperm((W // 8) * (H // 8), generator=g, device="cuda:0")[:300]
    jit = torch.randint(0, 3, (300, 2), generator=g, device="cuda:0")
    xs = (cells % (W // 8)) * 8 + jit[:, 0]
    ys = (cells // (W // 8)) * 8 + jit[:, 1]
    for f in frames:
        f[ys[:150], xs[:150]] = 4095
        f[ys[150:], xs[150:]] = 0
    dmap = torch.empty(H, W, dtype=torch.uint8, device="cuda:0")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in frames])
    L = capi.lib()

    def vote():
        L.detectDefects(N, ptrs, 2 * W, W, H, 0, threshold, spread, votes, dmap.data_ptr(), W, counts.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)

    def fix():  # (after the first call the flagged pixels hold their neighbours' median: the work per call stays the same)
        L.repairDefects(N, ptrs, 2 * W, W, H, 0, dmap.data_ptr(), W, torch.cuda.current_stream().cuda_stream)

    v_med, v_min, v_batch, iters = timed(vote, max(a.warmup, 1), max(a.iters, 20))
    found = counts.cpu().tolist()
    r_med, r_min, r_batch, _ = timed(fix, max(a.warmup, 1), max(a.iters, 20))
    nbytes = 2 * W * H * N + W * H
    print(json.dumps({
        "width": W, "height": H, "frames": N, "threshold": threshold, "spread": spread, "min_votes": votes, "iters": iters,
        "defects_found": found, "bytes": nbytes,
        "vote_us_batched": round(v_batch, 2), "vote_tb_per_s_batched": round(nbytes / v_batch / 1e6, 3),
        "vote_us_single_median": round(v_med, 2), "vote_us_single_min": round(v_min, 2),
        "repair_us_batched": round(r_batch, 2), "repair_us_single_median": round(r_med, 2), "repair_us_single_min": round(r_min, 2),
        "repair_map_bytes": W * H,
    }), flush=True)


if __name__ == "__main__":
    main()
