"""Time burst noise calibration: the statistics launch mfsr_noiseStatsTemporal (csrc/noise_temporal.hip)
beside mfsr_noiseStats (the yardstick: the single-frame statistics of the same frames, in the same session), and the burst driver
mfsr_burst_calibrate_noise_temporal end to end.  16 frames of 3840x2160 RGGB by default, the synth.make_burst scene.  Three flow
sets for the statistics launch: the burst's own (mfsr_burst_align_frames: the accepted pairs are rare), whole-quad translations
(every pair accepted at every block: all the sample loads and histogram updates there can be) and no flows at all (the same
with every site on the block grid).  After --warmup calls, --iters calls are timed with HIP events, one by one and as one batch
of back-to-back calls (tools/_stage_bench.py); the driver waits for the stream itself, so it is timed with the host's clock.
Prints one JSON line per measurement.  No threshold: the alignment dominates the driver.

    python tools/noise_temporal_bench.py [--width 3840 --height 2160 --frames 16 --iters 30 --warmup 3]

Record: profiles/noise_temporal_bench_4k16.txt.
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
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import (NOISE_TEMPORAL_TOL, BurstPipeline, default_config, noise_defaults, noise_fit,
                                                           noise_stats_temporal)
    from multi_frame_super_resolution_amd.synth import make_burst

    W, H, N = a.width, a.height, a.frames
    cfg = default_config(W, H, N, 2, False)
    d = noise_defaults(cfg)
    dev = "cuda:0"
    frames = make_burst(W, H, N, device=dev)[0]
    L = capi.lib()
    stream = torch.cuda.current_stream().cuda_stream
    I4 = ctypes.c_int32 * 4
    black, r4 = I4(*d.black), I4(*d.rect)
    hist = torch.zeros(4, 64, 272, dtype=torch.int32, device=dev)
    level_sum = torch.zeros(4, 64, dtype=torch.int64, device=dev)
    count = torch.zeros(4, 64, dtype=torch.int64, device=dev)
    ptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in frames])
    blocks = (d.rect[2] - d.rect[0]) * (d.rect[3] - d.rect[1])
    base = dict(width=W, height=H, frames=N, rect=list(d.rect), blocks=blocks, pairs=N * (N - 1) // 2, tol=NOISE_TEMPORAL_TOL)

    def single():
        L.noiseStats(N, ptrs, 2 * W, W, H, black, d.sat, r4, hist.data_ptr(), level_sum.data_ptr(), count.data_ptr(), stream)

    med, low, batch, iters = timed(single, max(a.warmup, 1), max(a.iters, 10))
    print(json.dumps(dict(base, what="mfsr_noiseStats", us_batched=round(batch, 2), us_single_median=round(med, 2),
                          us_single_min=round(low, 2), iters=iters)), flush=True)

    # the burst's own flows
    pipe = BurstPipeline(cfg, device=dev)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    prods = [pipe.new_frame_products() for _ in range(N - 1)]
    P = ctypes.c_void_p * (N - 1)
    L.burst_align_frames(pipe._h, N - 1, P(*[f.data_ptr() for f in frames[1:]]), None, P(*[p[0].data_ptr() for p in prods]),
                         prods[0][0].stride(0) * 4, P(*[p[1].data_ptr() for p in prods]), prods[0][1].stride(0) * 4, stream)
    torch.cuda.synchronize()
    own = [None] + [p[0] for p in prods]
    (fh, fw), _ = pipe.field_dims()
    moved = []
    for k in range(N):                      # whole-quad translations: 2 * (k % 5 - 2, k % 3 - 1) raw pixels
        f = torch.empty(fh, fw, 2, dtype=torch.float32, device=dev)
        f[..., 0], f[..., 1] = 2.0 * (k % 5 - 2), 2.0 * (k % 3 - 1)
        moved.append(f)
    for name, flows in (("own flows", own), ("whole-quad translations", moved), ("no flows", [None] * N)):
        fptrs = (ctypes.c_void_p * N)(*[None if f is None else f.data_ptr() for f in flows])

        def temporal():
            L.noiseStatsTemporal(N, ptrs, 2 * W, W, H, fptrs, 8 * fw, fw, fh, black, d.sat, r4, NOISE_TEMPORAL_TOL, hist.data_ptr(),
                                 level_sum.data_ptr(), count.data_ptr(), stream)

        med, low, batch, iters = timed(temporal, max(a.warmup, 1), max(a.iters, 10))
        torch.cuda.synchronize()
        st = noise_stats_temporal(frames, flows, cfg)
        fa, fb, fs, fn = noise_fit(st, cfg, temporal=True)
        print(json.dumps(dict(base, what="mfsr_noiseStatsTemporal", flows=name, us_batched=round(batch, 2),
                              us_single_median=round(med, 2), us_single_min=round(low, 2), iters=iters,
                              terms=int(st.count[0].sum().item()), nonzero_counters=int((st.hist != 0).sum().item()),
                              fit=dict(alpha=fa, beta=fb, status=fs, points=fn))), flush=True)

    # the driver, end to end (alignment of N - 1 frames, the statistics launch, the download, the fit)
    for _ in range(max(a.warmup, 1)):
        res = pipe.calibrate_noise(frames)
    times = []
    for _ in range(max(a.iters // 3, 5)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = pipe.calibrate_noise(frames)
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(base, what="BurstPipeline.calibrate_noise", ms_median=round(statistics.median(times), 3),
                          ms_min=round(min(times), 3), calls=len(times),
                          result=dict(alpha=res[0], beta=res[1], status=res[2], points=res[3], blocks=res[4]))), flush=True)


if __name__ == "__main__":
    main()
