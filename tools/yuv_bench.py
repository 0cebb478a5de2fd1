"""Time the two-plane YUV 4:2:0 finish: k_finishRenderedYuv beside k_finishRendered<RGB8> and <RGBA8>
on the same accumulators, and host bursts that download NV12 beside the ones that download RGB8, all in one process.

(a) Kernel, 7680x4320 output by default, colour matrix + 4096-interval tone table: mfsr_finishRenderedYuv for NV12 and P010,
each with the table staged in LDS (MFSR_RENDER_LUT=lds) and read through the cache (=cache), and mfsr_finishRendered for RGB8
and RGBA8 with their default table form, the calls taking turns; after --warmup calls, --iters calls of each as one batch of
back-to-back calls between two HIP events (the queue stays full: the device time of a call), --rounds times each.  With
--parent-lib PATH (a libmfsr_hip.so built from the parent commit) the RGB8 and RGBA8 finish of that library is timed in the
same turns, twice (two entries, "_a" and "_b": their difference is the session's run-to-run spread).  Reported: the median
microseconds, the spread over the rounds and GB/s of the bytes moved (24 bytes of accumulators in + the format's bytes out
per pixel; the fallback image is read only where a weight is under the threshold: one row in twenty here).

(b) Host bursts, 16 frames of 3840x2160 by default: BurstPipeline.process_host with RGB8, NV12 and P010 (matrix + table): one
burst at a time (process_host + host_sync, wall clock from the first call to the image in host memory) and --burst-batch
bursts back to back (one host_sync at the end, per burst), --rounds times each, the kinds taking turns, every turn on a fresh
pipeline after three warm-up bursts (one pipeline alive at a time, as tools/render_bench.py explains).  One JSON line.

    python tools/yuv_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5] [--parent-lib PATH]

Record: profiles/yuv_bench_4k16.txt.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--burst-batch", type=int, default=8, help="bursts back to back between two host_sync")
    ap.add_argument("--no-bursts", action="store_true", help="the kernel only")
    ap.add_argument("--parent-lib", default=None, help="a libmfsr_hip.so of the parent commit: its RGB8 / RGBA8 finish is timed too")
    a = ap.parse_args()

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config, render_row_bytes, tone_lut_srgb

    W, H, N = a.width, a.height, a.frames
    hrW, hrH = 2 * W, 2 * H
    dev = torch.device("cuda:0")
    L = capi.lib()
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    out = {"width": W, "height": H, "frames": N, "iters": iters, "rounds": rounds}

    # ---- (a) the kernel -----------------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda:0").manual_seed(1)
    fin = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 2.0
    wt = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 3.5 + 0.5
    wt[::20] = 0.0                                     # one row in twenty takes the fallback resample
    fb = torch.rand(H, W, 3, generator=g, device=dev)
    lut = tone_lut_srgb(4096).to(dev)
    outbuf = torch.empty(hrH * hrW * 4, dtype=torch.uint8, device=dev)
    thr = 1e-3
    calls, moved, keep = {}, {}, []

    def description(fmt):
        r = capi.Render()
        r.format = fmt
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*CCM)
        r.toneLut = lut.data_ptr()
        r.toneSize = lut.numel() - 1
        keep.append(r)
        return r

    def single_plane(fn, fmt):
        r, rb = description(fmt), render_row_bytes(fmt, hrW)

        def call():
            rc = fn(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                    outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW, hrH, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc

        return call, (24 + rb // hrW) * hrW * hrH

    def two_planes(fmt, how):
        r, rb = description(fmt), render_row_bytes(fmt, hrW)

        def call():
            os.environ["MFSR_RENDER_LUT"] = how
            L.finishRenderedYuv(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                                outbuf.data_ptr(), rb, outbuf.data_ptr() + rb * hrH, rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW,
                                hrH, torch.cuda.current_stream().cuda_stream)
            del os.environ["MFSR_RENDER_LUT"]

        return call, 24 * hrW * hrH + rb * hrH * 3 // 2

    libs = {"": L.raw["mfsr_finishRendered"]}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        fn = parent.mfsr_finishRendered
        fn.restype, fn.argtypes = ctypes.c_int, L.raw["mfsr_finishRendered"].argtypes
        libs["_parent_a"] = libs["_parent_b"] = fn
        out["parent_lib"] = os.path.basename(a.parent_lib)
    for suffix, fn in libs.items():
        for fmt, name in ((capi.OUT_RGB8, "rgb8"), (capi.OUT_RGBA8, "rgba8")):
            key = f"finishRendered_{name}{suffix}"
            calls[key], moved[key] = single_plane(fn, fmt)
    for fmt, name in ((capi.OUT_NV12, "nv12"), (capi.OUT_P010, "p010")):
        for how in ("lds", "cache"):
            key = f"finishRenderedYuv_{name}_lut_{how}"
            calls[key], moved[key] = two_planes(fmt, how)
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    out["kernel"] = {"out_width": hrW, "out_height": hrH, **{name: _stat(v, moved[name]) for name, v in us.items()}}
    del fin, wt, fb, outbuf
    torch.cuda.empty_cache()

    # ---- (b) host bursts ----------------------------------------------------------------------------------------------------
    if not a.no_bursts:
        gc = torch.Generator().manual_seed(2)
        base = torch.randint(200, 1200, (H, W), generator=gc, dtype=torch.int32)
        host = [(base + torch.randint(0, 64, (H, W), generator=gc, dtype=torch.int32)).to(torch.int16).pin_memory() for _ in range(N)]
        kinds = {"rgb8_ccm_lut": capi.OUT_RGB8, "nv12_ccm_lut": capi.OUT_NV12, "p010_ccm_lut": capi.OUT_P010}

        def pipeline(fmt):
            c = default_config(W, H, N, 2, False)
            c.uploadRing = min(N, 32)
            pipe = BurstPipeline(c, dev)
            pipe.set_render(fmt, matrix=CCM, tone_lut=lut)
            return pipe

        single = {k: [] for k in kinds}
        batched = {k: [] for k in kinds}
        down = {}
        for _ in range(rounds):
            for name, fmt in kinds.items():
                pipe = pipeline(fmt)
                down[name] = pipe.out16.numel() * pipe.out16.element_size()
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
        out["host_burst"] = {name: {"download_bytes": down[name], "one_at_a_time": _stat(single[name]),
                                    "back_to_back": _stat(batched[name])} for name in kinds}
        out["burst_batch"] = a.burst_batch
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
