"""Time the rendered finish: k_finishRendered beside k_finishFused on the same accumulators, and host
bursts that download RGB8 beside the ones that download 16-bit RGB, all in one process.

(a) Kernel, 7680x4320 output by default: mfsr_finishFused writing the uint16_t image (what a host burst's finish does) and
mfsr_finishRendered per format without matrix and table, then with a colour matrix and a 4096-interval tone table read
through the cache (MFSR_RENDER_LUT=cache), then with the table staged in LDS (MFSR_RENDER_LUT=lds), the calls taking turns;
after --warmup calls, --iters calls of each as one batch of back-to-back calls between two HIP events (the queue stays full:
the device time of a call), --rounds times each.  Reported: the median microseconds, the spread over the rounds and GB/s of the bytes moved (24
bytes of accumulators in + the format's bytes out per pixel; the fallback image is read only where a weight is under the
threshold: one row in twenty here).

(b) Host bursts, 16 frames of 3840x2160 by default: BurstPipeline.process_host without a render (16-bit RGB down, 6 bytes per
pixel), with RGB8 and with RGB8 + matrix + table: one burst at a time (process_host + host_sync, wall clock from the first
call to the image in host memory) and --burst-batch bursts back to back (one host_sync at the end, per burst), --rounds times
each.  One pipeline is alive at a time (each owns a copy and a download stream, and the streams of several pipelines share
the process's hardware queues: six pipelines side by side made three of them 2-3.5 ms slower back to back, whichever they
were); the kinds take turns, every turn on a fresh pipeline after three warm-up bursts.  (c) The same with cfg.rawPacking =
MIPI10.  One JSON line.

    python tools/render_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5]

Record: profiles/render_bench_4k16.txt.
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
    a = ap.parse_args()

    import torch
    from multi_frame_super_resolution_amd import capi, synth
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config, render_row_bytes, tone_lut_srgb

    W, H, N = a.width, a.height, a.frames
    hrW, hrH = 2 * W, 2 * H
    dev = torch.device("cuda:0")
    L = capi.lib()
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    out = {"width": W, "height": H, "frames": N, "iters": iters, "rounds": rounds}
    names = {capi.OUT_RGB16: "rgb16", capi.OUT_RGB8: "rgb8", capi.OUT_RGBA8: "rgba8", capi.OUT_RGB10A2: "rgb10a2"}

    # ---- (a) the kernel -----------------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda:0").manual_seed(1)
    fin = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 2.0
    wt = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 3.5 + 0.5
    wt[::20] = 0.0                                     # one row in twenty takes the fallback resample
    fb = torch.rand(H, W, 3, generator=g, device=dev)
    lut = tone_lut_srgb(4096).to(dev)
    outbuf = torch.empty(hrH * hrW * 6, dtype=torch.uint8, device=dev)
    thr = 1e-3
    calls, moved = {}, {}

    def plain():
        L.finishFused(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None, 12 * hrW,
                      outbuf.data_ptr(), hrW, hrH, thr, 1, 65535.0, torch.cuda.current_stream().cuda_stream)

    calls["finishFused_u16"] = plain
    moved["finishFused_u16"] = 30 * hrW * hrH
    keep = []
    for fmt, name in names.items():
        for variant in ("", "_ccm_lut_cache", "_ccm_lut_lds"):
            r = capi.Render()
            r.format = fmt
            if variant:
                r.useMatrix = 1
                r.matrix = (ctypes.c_float * 9)(*CCM)
                r.toneLut = lut.data_ptr()
                r.toneSize = lut.numel() - 1
            keep.append(r)
            rb = render_row_bytes(fmt, hrW)

            def rendered(r=r, rb=rb, how=variant.rsplit("_", 1)[-1]):
                if how:
                    os.environ["MFSR_RENDER_LUT"] = how
                L.finishRendered(fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0, None,
                                 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW, hrH,
                                 torch.cuda.current_stream().cuda_stream)
                if how:
                    del os.environ["MFSR_RENDER_LUT"]

            calls[f"finishRendered_{name}{variant}"] = rendered
            moved[f"finishRendered_{name}{variant}"] = (24 + rb // hrW) * hrW * hrH
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    out["kernel"] = {"out_width": hrW, "out_height": hrH, **{name: _stat(v, moved[name]) for name, v in us.items()}}
    del fin, wt, fb, outbuf
    torch.cuda.empty_cache()

    # ---- (b), (c) host bursts -----------------------------------------------------------------------------------------------
    if not a.no_bursts:
        gc = torch.Generator().manual_seed(2)
        base = torch.randint(200, 1200, (H, W), generator=gc, dtype=torch.int32)
        burst12 = [(base + torch.randint(0, 64, (H, W), generator=gc, dtype=torch.int32)).to(torch.int16) for _ in range(N)]
        kinds = {}
        for pname, packing in (("unpacked", 0), ("mipi10", capi.PACK_MIPI10)):
            src = burst12
            if packing:
                src = [(f.to(torch.int32) >> 2).to(torch.int16) for f in burst12]
            host = [t.pin_memory() for t in (synth.pack_raw(src, packing) if packing else src)]
            for rname, render in (("rgb16", None), ("rgb8", dict(format=capi.OUT_RGB8)),
                                  ("rgb8_ccm_lut", dict(format=capi.OUT_RGB8, matrix=CCM, tone_lut=lut))):
                kinds[f"{pname}_{rname}"] = (packing, host, render)

        def pipeline(packing, render):
            c = default_config(W, H, N, 2, False)
            c.uploadRing = min(N, 32)
            c.rawPacking = packing
            if packing:
                for i in range(3):
                    c.black[i], c.white[i] = c.black[i] / 4, 1023.0 - c.black[i] / 4
                c.maxVal = 1023.0
            pipe = BurstPipeline(c, dev)
            if render:
                pipe.set_render(**render)
            return pipe

        single = {k: [] for k in kinds}
        batched = {k: [] for k in kinds}
        down = {}
        for _ in range(rounds):
            for name, (packing, host, render) in kinds.items():
                pipe = pipeline(packing, render)
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
