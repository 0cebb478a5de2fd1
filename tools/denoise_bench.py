"""Time the denoised finish: k_finishDenoised beside k_finishRendered and k_finishSharpened at the same
R, beside itself with a fade under which every pixel skips, and beside the two-launch alternative on the same accumulators;
and host bursts with and without denoising, all in one process.

Kernel, 7680x4320 output by default, one row in twenty on the fallback, colour matrix + 4096-interval tone table, RGBA8 and RGB8,
the calls taking turns:
(a) mfsr_finishRendered;
(b) mfsr_finishSharpened at R = 1, 2, 3 (Gaussian taps, amount 1);
(c) mfsr_finishDenoised at R = 1, 2, 3 without fade (strength 3, gain 2, alpha 1.6e-3, beta 1.6e-5);
(d) mfsr_finishDenoised at R = 2 with a fade (wLo 0.25, wHi 0.5) under which every pixel has lambda = 0: staging only;
(e) the two launches: mfsr_finishFusedWindow to a float image (no gamma, no integers), then mfsr_denoiseImage at R = 2 with the
    weights as its count image.
After --warmup calls, --iters calls of each as one batch of back-to-back calls between two HIP events (the queue stays full:
the device time of a call), --rounds times each.  Reported: the median microseconds, the spread over the rounds and GB/s of
the bytes the algorithm needs (24 bytes of accumulators in + the format's bytes out per pixel; (e) also writes and reads 12
bytes per pixel of float image and reads the weights again, which are not counted), and microseconds per tap of the stencil,
(us(c, R) - us(d)) / (2R + 1)^2.

Host bursts, 16 frames of 3840x2160 by default: BurstPipeline.process_host to RGB8 with matrix + table, without denoising and
with it (R = 2): --burst-batch bursts back to back (one host_sync at the end, per burst) and one at a time, --rounds times
each, the kinds taking turns, every turn on a fresh pipeline after three warm-up bursts (as tools/sharpen_bench.py).  One JSON
line.

    python tools/denoise_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5]

Record: profiles/denoise_bench_4k16.txt.
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


def _stat(v, moved=None):
    med = statistics.median(v)
    out = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    if moved is not None:
        out["gb_per_s"] = round(moved / med / 1e3, 1)
    return out


CCM = [1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56]
SIGMA = {1: 0.6, 2: 0.9, 3: 1.0}
NOISE = dict(alpha=1.6e-3, beta=1.6e-5)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--burst-batch", type=int, default=8, help="bursts back to back between two host_sync")
    ap.add_argument("--no-bursts", action="store_true", help="the kernels only")
    ap.add_argument("--formats", default="rgba8,rgb8", help="the formats to time (kernel part)")
    a = ap.parse_args()

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import (BurstPipeline, _denoise_struct, default_config, render_row_bytes,
                                                           sharpen_gaussian, tone_lut_srgb)

    W, H, N = a.width, a.height, a.frames
    hrW, hrH = 2 * W, 2 * H
    dev = torch.device("cuda:0")
    L = capi.lib()
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    L.denoise_tile(ctypes.byref(tw), ctypes.byref(th))
    tw, th = tw.value, th.value
    out = {"width": W, "height": H, "frames": N, "iters": iters, "rounds": rounds, "tile": [tw, th],
           "halo_factor": {f"R{R}": round((tw + 2 * R) * (th + 2 * R) / (tw * th), 4) for R in SIGMA}}
    names = {capi.OUT_RGBA8: "rgba8", capi.OUT_RGB8: "rgb8", capi.OUT_RGB16: "rgb16", capi.OUT_RGB10A2: "rgb10a2"}
    names = {k: v for k, v in names.items() if v in a.formats.split(",")}

    # ---- the kernels --------------------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda:0").manual_seed(1)
    fin = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 2.0
    wt = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 3.5 + 0.5
    wt[::20] = 0.0                                     # one row in twenty takes the fallback resample (its count is 1)
    fb = torch.rand(H, W, 3, generator=g, device=dev)
    lut = tone_lut_srgb(4096).to(dev)
    outbuf = torch.empty(hrH * hrW * 6, dtype=torch.uint8, device=dev)
    lin = torch.empty(hrH, hrW, 3, dtype=torch.float32, device=dev)
    thr = 1e-3
    sharpen = {R: sharpen_gaussian(SIGMA[R], R, 1.0, 0.0) for R in SIGMA}
    denoise = {R: _denoise_struct(3.0, R, 2.0, **NOISE) for R in SIGMA}
    skip = _denoise_struct(3.0, 2, 2.0, fade=(0.25, 0.5), **NOISE)   # every count is >= 0.5: lambda = 0 everywhere
    calls, moved, keep = {}, {}, []

    def stream():
        return torch.cuda.current_stream().cuda_stream

    for fmt, name in names.items():
        r = capi.Render()
        r.format = fmt
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*CCM)
        r.toneLut = lut.data_ptr()
        r.toneSize = lut.numel() - 1
        keep.append(r)
        rb = render_row_bytes(fmt, hrW)
        need = (24 + rb // hrW) * hrW * hrH

        def rendered(r=r, rb=rb):
            L.finishRendered(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                             outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW, hrH, stream())

        calls[f"a_finishRendered_{name}"] = rendered
        for R, s in sharpen.items():
            def sharpened(r=r, rb=rb, s=s):
                L.finishSharpened(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None,
                                  12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW, hrH, ctypes.byref(s),
                                  0, 0, stream())

            calls[f"b_finishSharpened_{name}_R{R}"] = sharpened

        def denoised_call(d, r=r, rb=rb):
            def call():
                L.finishDenoised(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None,
                                 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW, hrH, ctypes.byref(d),
                                 0, 0, stream())
            return call

        for R, d in denoise.items():
            calls[f"c_finishDenoised_{name}_R{R}"] = denoised_call(d)
        calls[f"d_finishDenoised_all_skip_{name}_R2"] = denoised_call(skip)

        def two_launches(r=r, rb=rb, d=denoise[2]):
            L.finishFusedWindow(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0,
                                lin.data_ptr(), 12 * hrW, None, hrW, hrH, thr, 0, 65535.0, 0, 0, hrW, hrH, stream())
            L.denoiseImage(lin.data_ptr(), 12 * hrW, wt.data_ptr(), 12 * hrW, None, 0, outbuf.data_ptr(), rb, hrW, hrH,
                           ctypes.byref(d), ctypes.byref(r), 1, stream())

        calls[f"e_finish_then_denoiseImage_{name}_R2"] = two_launches
        for key in calls:
            moved.setdefault(key, need)
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    out["kernel"] = {"out_width": hrW, "out_height": hrH, **{name: _stat(v, moved[name]) for name, v in us.items()}}
    out["us_per_tap"] = {}
    for name in names.values():
        base = statistics.median(us[f"d_finishDenoised_all_skip_{name}_R2"])
        for R in SIGMA:
            out["us_per_tap"][f"{name}_R{R}"] = round((statistics.median(us[f"c_finishDenoised_{name}_R{R}"]) - base) / (2 * R + 1) ** 2, 2)
    del fin, wt, fb, outbuf, lin
    torch.cuda.empty_cache()

    # ---- host bursts --------------------------------------------------------------------------------------------------------
    if not a.no_bursts:
        gc = torch.Generator().manual_seed(2)
        base = torch.randint(200, 1200, (H, W), generator=gc, dtype=torch.int32)
        host = [(base + torch.randint(0, 64, (H, W), generator=gc, dtype=torch.int32)).to(torch.int16).pin_memory() for _ in range(N)]
        kinds = {"rgb8_ccm_lut": None, "rgb8_ccm_lut_denoised": dict(strength=3.0, radius=2, gain=2.0)}

        def pipeline(den):
            c = default_config(W, H, N, 2, False)
            c.uploadRing = min(N, 32)
            pipe = BurstPipeline(c, dev)
            pipe.set_render(format=capi.OUT_RGB8, matrix=CCM, tone_lut=lut)
            if den:
                pipe.set_denoise(**den)
            return pipe

        single = {k: [] for k in kinds}
        batched = {k: [] for k in kinds}
        for _ in range(rounds):
            for name, den in kinds.items():
                pipe = pipeline(den)
                for _ in range(3):
                    pipe.process_host(host)
                    pipe.host_sync()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.process_host(host)
                pipe.host_sync()
                single[name].append((time.perf_counter() - t0) * 1e6)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.burst_batch):
                    pipe.process_host(host)
                pipe.host_sync()
                batched[name].append((time.perf_counter() - t0) * 1e6 / a.burst_batch)
                torch.cuda.synchronize()
                pipe.close()
                del pipe
                torch.cuda.empty_cache()
        out["host_burst"] = {name: {"one_at_a_time": _stat(single[name]), "back_to_back": _stat(batched[name])} for name in kinds}
        out["burst_batch"] = a.burst_batch
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
