"""Time the erosion of the certainty mask (mfsr_erodeMaskBatch, csrc/erode.hip) on 4 masks of 1920x1080 cells (one fuse group of a
4K Bayer burst) beside the robustness kernel on the same geometry (mfsr_robustnessMaskFusedBatch: the stage that writes those
masks), and one whole 3840x2160 x 16 burst with cfg.maskErode 0 and 2 taking turns.  HIP events on the current stream around
--reps back-to-back launches after a warm-up (the queue stays full: device time per launch); the bursts are timed one by one
with a host clock around process() + synchronise, --bursts times each, alternating, and reported as median and min..max (the
run-to-run spread).  The erosion must move 2 x 16 bytes per cell (33.2 MB in, 33.2 MB out per 4K mask): achieved GB/s against
that.  Prints one JSON line.  The kernels alone: ``rocprofv3 --kernel-trace --stats -- python tools/erode_bench.py``.

    python tools/erode_bench.py [--reps 200 --bursts 7 --radius 2]

Record: profiles/erode_bench_4k16.txt.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools._stage_bench import timed


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("erode_bench needs a HIP device: a time from anything else says nothing")
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config, erode_mask
    from multi_frame_super_resolution_amd.synth import make_burst

    dev = torch.device("cuda:0")
    L = capi.lib()
    W, H, N, n = a.width, a.height, a.frames, 4
    w, h = W // 2, H // 2
    st = torch.cuda.current_stream().cuda_stream

    # the robustness kernel on the same geometry: reference / moved half-resolution images, a smooth flow
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    ref = torch.rand(h, w, 3, generator=g, device=dev)
    moved = [(ref + 0.02 * torch.randn(h, w, 3, generator=g, device=dev)).contiguous() for _ in range(n)]
    flows = [(0.7 * torch.randn(1, 1, 2, generator=g, device=dev)).expand(h, w, 2).contiguous() for _ in range(n)]
    masks = torch.empty(n, h, w, 4, device=dev)
    rf = (capi.RobustnessFrame * n)(*[capi.RobustnessFrame(moved[k].data_ptr(), masks[k].data_ptr(), flows[k].data_ptr())
                                     for k in range(n)])
    cfg0 = default_config(W, H, N, 2, False)

    def robustness():
        L.robustnessMaskFusedBatch(n, rf, ref.data_ptr(), w * 8, w, h, w, h, w * 12, w * 16, cfg0.alpha, cfg0.beta, cfg0.thresholdM, st)

    rob_us = timed(robustness, 5, a.reps, singles=False)[2]
    out = torch.empty_like(masks)

    def erode():
        erode_mask(masks, a.radius, out=out)

    er_us = timed(erode, 5, a.reps, singles=False)[2]
    bytes_moved = 2 * 16 * w * h * n

    # whole bursts, maskErode 0 and 2 taking turns
    frames = make_burst(W, H, N, device=dev)[0]
    pipes = {}
    for r in (0, a.radius):
        cfg = default_config(W, H, N, 2, False)
        cfg.maskErode = r
        pipes[r] = BurstPipeline(cfg, dev)
        for _ in range(2):
            pipes[r].process(frames)
    torch.cuda.synchronize()
    ms = {r: [] for r in pipes}
    for _ in range(a.bursts):
        for r, p in pipes.items():
            t0 = time.perf_counter()
            p.process(frames)
            torch.cuda.synchronize()
            ms[r].append((time.perf_counter() - t0) * 1000.0)
    for p in pipes.values():
        p.close()

    def stats(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    print(json.dumps({
        "tool": "erode_bench", "masks": n, "mask_w": w, "mask_h": h, "radius": a.radius, "reps": a.reps,
        "erode_us": round(er_us, 2), "robustness_us": round(rob_us, 2),
        "erode_bytes": bytes_moved, "erode_gbps": round(bytes_moved / er_us / 1e3, 1),
        "burst": f"{W}x{H}x{N}", "bursts_timed": a.bursts,
        "burst_ms_erode0": stats(ms[0])["median"], "burst_ms_erode0_spread": stats(ms[0]),
        f"burst_ms_erode{a.radius}": stats(ms[a.radius])["median"], f"burst_ms_erode{a.radius}_spread": stats(ms[a.radius]),
    }), flush=True)


if __name__ == "__main__":
    main()
