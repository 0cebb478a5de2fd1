"""Time the sharpness score of a burst (mfsr_frameSharpness, csrc/select.hip): 16 frames of 3840x2160 RGGB by default, all
in one call, the whole-frame rectangle of mfsr_burst_select_frames.  After --warmup calls, --iters calls are timed with HIP
events on the current stream, one by one (each includes the host's enqueue latency, the GPU waits for it) and as one batch
of back-to-back calls (the queue stays full: the device time of a call, its memset of the sums included); prints one JSON
line with microseconds per call and the effective bandwidth (the raw bytes of the frames / time).  The kernel alone:
``rocprofv3 --kernel-trace --stats -- python tools/select_bench.py``.

    python tools/select_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5]

Record: profiles/select_bench_4k16.txt.
"""
from __future__ import annotations

import argparse
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
    from multi_frame_super_resolution_amd.pipeline import default_config, frame_sharpness, sharpness_rect

    W, H, N = a.width, a.height, a.frames
    cfg = default_config(W, H, N, 2, False)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    frames = [torch.randint(0, 4096, (H, W), generator=g, device="cuda:0", dtype=torch.int32).to(torch.int16) for _ in range(N)]
    med, fastest, batch, iters = timed(lambda: frame_sharpness(frames, cfg), max(a.warmup, 1), max(a.iters, 1))
    sums = frame_sharpness(frames, cfg)
    nbytes = 2 * W * H * N
    print(json.dumps({
        "width": W, "height": H, "frames": N, "rect": list(sharpness_rect(cfg)), "iters": iters,
        "us_per_call_batched": round(batch, 2), "tb_per_s_batched": round(nbytes / batch / 1e6, 3),
        "us_single_median": round(med, 2), "us_single_min": round(fastest, 2), "bytes": nbytes,
        "tb_per_s_single_median": round(nbytes / med / 1e6, 3),
        "sums_head": [int(v) for v in sums.cpu()[:2]],
    }), flush=True)


if __name__ == "__main__":
    main()
