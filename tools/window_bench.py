"""Zoom-window bursts against the whole frame (include/mfsr.h, mfsr_burst_set_window).

For each workload (frames resident on the device) the legs are the whole frame and centred windows of 1/4 and 1/16 of the
HR area.  Every leg is warmed up, then the legs take turns burst by burst (--bursts each), timed with HIP events on the
compute stream.  One JSON line per leg: ms per burst (median, mean), output Mpix, accumulator bytes (the two plane-sets),
and the sha256 of the u16 result against that of the same rectangle cut from the whole-frame result.

    python tools/window_bench.py [--workloads 4k16_rggb_x4,4k16_rggb_x2] [--bursts 20] [--warmup 2]

Per-kernel fuse times: run the same command under ``rocprofv3 --kernel-trace --stats -- python tools/window_bench.py ...``.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WORKLOADS = {  # as bench.py: (width, height, frames, scale, mono)
    "4k16_rggb_x4": (3840, 2160, 16, 4, False),
    "4k16_rggb_x2": (3840, 2160, 16, 2, False),
}


def centred(hr_w: int, hr_h: int, frac: int):
    """The centred window of 1/frac**2 of the area, on the 16-pixel grid."""
    w, h = hr_w // frac // 16 * 16, hr_h // frac // 16 * 16
    return ((hr_w - w) // 2 // 16 * 16, (hr_h - h) // 2 // 16 * 16, w, h)


def sha(t) -> str:
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def run(name: str, bursts: int, warmup: int):
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    from multi_frame_super_resolution_amd.synth import make_burst

    W, H, N, s, mono = WORKLOADS[name]
    cfg = default_config(W, H, N, s, mono)
    frames, _, _ = make_burst(W, H, N, scale=s, mono=mono, seed=1234, device="cuda:0")
    frames = [f.to("cuda:0").contiguous() for f in frames]
    hr_w, hr_h = W * s, H * s
    legs = {"whole": None, "quarter": centred(hr_w, hr_h, 2), "sixteenth": centred(hr_w, hr_h, 4)}
    pipes = {k: BurstPipeline(cfg, window=v) for k, v in legs.items()}
    times = {k: [] for k in legs}
    for k, p in pipes.items():
        for _ in range(warmup):
            p.process(frames)
    torch.cuda.synchronize()
    for _ in range(bursts):
        for k, p in pipes.items():  # the legs alternate burst by burst
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            p.process(frames)
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    whole16 = pipes["whole"].process(frames)[1].clone()
    torch.cuda.synchronize()
    for k, p in pipes.items():
        x, y, w, h = legs[k] or (0, 0, hr_w, hr_h)
        got = p.process(frames)[1]
        torch.cuda.synchronize()
        want = whole16[y:y + h, x:x + w]
        print(json.dumps({
            "workload": name, "leg": k, "window": [x, y, w, h], "bursts": len(times[k]),
            "ms_per_burst_median": round(statistics.median(times[k]), 3), "ms_per_burst_mean": round(statistics.mean(times[k]), 3),
            "output_mpix": round(w * h / 1e6, 3), "accumulator_bytes": 2 * 12 * w * h,
            "out16_sha256_16": sha(got), "whole_crop_sha256_16": sha(want), "bit_identical": bool(torch.equal(got, want)),
        }), flush=True)
    for p in pipes.values():
        p.close()
    del pipes, frames
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--workloads", default="4k16_rggb_x4,4k16_rggb_x2")
    ap.add_argument("--bursts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    for name in a.workloads.split(","):
        run(name, max(a.bursts, 1), max(a.warmup, 1))


if __name__ == "__main__":
    main()
