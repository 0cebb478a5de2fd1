"""Time the finish chain: k_finishChain beside the shortest sequence of existing launches that gives the
same image, beside the single-stage finishes, and resident bursts with and without a chain, all in one process.

Kernel, 7680x4320 output by default, one row in twenty on the fallback, colour matrix + 4096-interval tone table, the calls
taking turns:
(a) mfsr_finishChain, D+S at (R_d, R_s) = (2, 2) and (3, 4), to RGB8, RGBA8 and NV12; D+S+L at (2, 2) to RGB8;
(b) the sequence for the same image: mfsr_finishDenoised to a float image, then mfsr_sharpenImage to the format; for NV12
    mfsr_sharpenImage to a float image and a third launch, mfsr_renderImageYuv; for D+S+L mfsr_sharpenImage to a float image,
    then mfsr_localToneImage;
(c) the single-stage finishes: mfsr_finishRendered, mfsr_finishDenoised (R = 2, 3), mfsr_finishSharpened (R = 2, 4),
    mfsr_finishLocalTone, mfsr_finishRenderedYuv, and the chain with that one stage on.
After --warmup calls, --iters calls of each as one batch of back-to-back calls between two HIP events (the queue stays full:
the device time of a call), --rounds times each.  Reported: the median microseconds and the spread over the rounds, GB/s of
the bytes the algorithm needs (24 bytes of accumulators in + the format's bytes out per pixel; the sequences also write and
read 12 bytes per pixel per intermediate float image, which are not counted), and chain / sequence.

Resident bursts, 16 frames of 3840x2160 by default: BurstPipeline.process to RGB8 with matrix + table, without a chain, with
set_denoise (R = 2) alone and with the chain D+S (2, 2), the kinds taking turns, every turn on a fresh pipeline after three
warm-up bursts.  One JSON line.

    python tools/chain_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5]
    python tools/chain_bench.py --no-bursts --rounds 1 --only DS_rgb8_R22      # one row, e.g. under a counter collection

Record: profiles/chain_bench_4k16.txt.
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
SIGMA = {2: 0.9, 3: 1.0, 4: 1.3}
NOISE = dict(alpha=1.6e-3, beta=1.6e-5)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-bursts", action="store_true", help="the kernels only")
    ap.add_argument("--only", default=None, metavar="REGEX", help="time only the calls whose name matches (a counter run of one row)")
    a = ap.parse_args()

    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import (BurstPipeline, _chain_struct, _denoise_struct, default_config,
                                                           local_tone_defaults, local_tone_grid, render_row_bytes, sharpen_gaussian,
                                                           tone_lut_srgb)

    W, H, N = a.width, a.height, a.frames
    hrW, hrH = 2 * W, 2 * H
    dev = torch.device("cuda:0")
    L = capi.lib()
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    out = {"width": W, "height": H, "frames": N, "iters": iters, "rounds": rounds}

    # ---- the kernels --------------------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda:0").manual_seed(1)
    fin = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 2.0
    wt = torch.rand(hrH, hrW, 3, generator=g, device=dev) * 3.5 + 0.5
    wt[::20] = 0.0                                     # one row in twenty takes the fallback resample (its count is 1)
    fb = torch.rand(H, W, 3, generator=g, device=dev)
    lut = tone_lut_srgb(4096).to(dev)
    outbuf = torch.empty(hrH * hrW * 6, dtype=torch.uint8, device=dev)
    lin = torch.empty(hrH, hrW, 3, dtype=torch.float32, device=dev)
    lin2 = torch.empty(hrH, hrW, 3, dtype=torch.float32, device=dev)
    thr = 1e-3
    lt = local_tone_defaults(hrW, hrH)
    gx, gy, gz = local_tone_grid(hrW, hrH, lt)
    grid = torch.rand(gy, gx, gz, generator=g, device=dev) * 1.5 + 0.5
    sharpen = {R: sharpen_gaussian(SIGMA[R], R, 1.0, 0.0) for R in (2, 4)}
    denoise = {R: _denoise_struct(3.0, R, 2.0, **NOISE) for R in (2, 3)}

    def chain_of(rd, rs, tone=False):
        c, gr, _ = _chain_struct(hrW, hrH, dict(strength=3.0, radius=rd, gain=2.0, **NOISE) if rd else None,
                                 dict(amount=1.0, sigma=SIGMA[rs], radius=rs) if rs else None, (lt, grid) if tone else None, dev)
        return c

    names = {capi.OUT_RGB8: "rgb8", capi.OUT_RGBA8: "rgba8", capi.OUT_NV12: "nv12"}
    calls, moved, keep = {}, {}, []

    def stream():
        return torch.cuda.current_stream().cuda_stream

    src = (fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0)
    place = (0, 0, hrW, hrH)
    for fmt, name in names.items():
        r = capi.Render()
        r.format = fmt
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*CCM)
        r.toneLut = lut.data_ptr()
        r.toneSize = lut.numel() - 1
        keep.append(r)
        two = fmt == capi.OUT_NV12
        rb = render_row_bytes(fmt, hrW)
        uv = outbuf.data_ptr() + rb * hrH if two else None
        need = (24 + (rb * 3 // 2 if two else rb) // hrW) * hrW * hrH

        def chained(c, tone, r=r, rb=rb, uv=uv, two=two):
            keep.append(c)

            def call():
                L.finishChain(*src, None, 12 * hrW, outbuf.data_ptr(), rb, uv, rb if two else 0, ctypes.byref(r), hrW, hrH, thr, 1, *place,
                              ctypes.byref(c), grid.data_ptr() if tone else None, 0, 0, stream())
            return call

        def sequence(rd, rs, tone, r=r, rb=rb, uv=uv, two=two):
            d, s = denoise[rd], sharpen[rs]

            def call():
                L.finishDenoised(*src, lin.data_ptr(), 12 * hrW, None, 0, None, hrW, hrH, thr, 0, *place, ctypes.byref(d), 0, 0, stream())
                if two or tone:
                    L.sharpenImage(lin.data_ptr(), 12 * hrW, lin2.data_ptr(), 12 * hrW, None, 0, hrW, hrH, ctypes.byref(s), None, 0, stream())
                    if tone:
                        L.localToneImage(lin2.data_ptr(), 12 * hrW, None, 0, outbuf.data_ptr(), rb, hrW, hrH, ctypes.byref(r), 1,
                                         grid.data_ptr(), ctypes.byref(lt), *place, stream())
                    else:
                        L.renderImageYuv(lin2.data_ptr(), 12 * hrW, None, 0, outbuf.data_ptr(), rb, uv, rb, hrW, hrH, ctypes.byref(r), 1,
                                         stream())
                else:
                    L.sharpenImage(lin.data_ptr(), 12 * hrW, None, 0, outbuf.data_ptr(), rb, hrW, hrH, ctypes.byref(s), ctypes.byref(r), 1,
                                   stream())
            return call

        for rd, rs in ((2, 2), (3, 4)):
            calls[f"a_finishChain_DS_{name}_R{rd}{rs}"] = chained(chain_of(rd, rs), False)
            calls[f"b_sequence_DS_{name}_R{rd}{rs}"] = sequence(rd, rs, False)
        if fmt == capi.OUT_RGB8:
            calls[f"a_finishChain_DSL_{name}_R22"] = chained(chain_of(2, 2, True), True)
            calls[f"b_sequence_DSL_{name}_R22"] = sequence(2, 2, True)
        # the single-stage finishes and the chain with that stage alone
        if two:
            def yuv(r=r, rb=rb, uv=uv):
                L.finishRenderedYuv(*src, None, 12 * hrW, outbuf.data_ptr(), rb, uv, rb, ctypes.byref(r), hrW, hrH, thr, 1, *place, stream())
            calls[f"c_finishRenderedYuv_{name}"] = yuv
        else:
            def rendered(r=r, rb=rb):
                L.finishRendered(*src, None, 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, *place, stream())
            calls[f"c_finishRendered_{name}"] = rendered
            for R, d in denoise.items():
                def denoised(r=r, rb=rb, d=d):
                    L.finishDenoised(*src, None, 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, *place, ctypes.byref(d),
                                     0, 0, stream())
                calls[f"c_finishDenoised_{name}_R{R}"] = denoised
            for R, s in sharpen.items():
                def sharpened(r=r, rb=rb, s=s):
                    L.finishSharpened(*src, None, 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, *place,
                                      ctypes.byref(s), 0, 0, stream())
                calls[f"c_finishSharpened_{name}_R{R}"] = sharpened

            def toned(r=r, rb=rb):
                L.finishLocalTone(*src, None, 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, *place, grid.data_ptr(),
                                  ctypes.byref(lt), stream())
            calls[f"c_finishLocalTone_{name}"] = toned
            calls[f"c_finishChain_L_{name}"] = chained(chain_of(0, 0, True), True)
        calls[f"c_finishChain_D_{name}_R2"] = chained(chain_of(2, 0), False)
        calls[f"c_finishChain_S_{name}_R2"] = chained(chain_of(0, 2), False)
        for key in calls:
            moved.setdefault(key, need)
    if a.only:
        import re
        calls = {k: v for k, v in calls.items() if re.search(a.only, k)}
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    out["kernel"] = {"out_width": hrW, "out_height": hrH, **{name: _stat(v, moved[name]) for name, v in us.items()}}
    out["chain_over_sequence"] = {k[len("a_finishChain_"):]: round(statistics.median(us[k]) / statistics.median(us["b_sequence_" + k[len("a_finishChain_"):]]), 3)
                                  for k in calls if k.startswith("a_finishChain_") and "b_sequence_" + k[len("a_finishChain_"):] in calls}
    del fin, wt, fb, outbuf, lin, lin2
    torch.cuda.empty_cache()

    # ---- resident bursts ----------------------------------------------------------------------------------------------------
    if not a.no_bursts:
        gc = torch.Generator().manual_seed(2)
        base = torch.randint(200, 1200, (H, W), generator=gc, dtype=torch.int32)
        frames = [(base + torch.randint(0, 64, (H, W), generator=gc, dtype=torch.int32)).to(torch.int16).to(dev) for _ in range(N)]
        kinds = ("rgb8_ccm_lut", "rgb8_ccm_lut_denoised", "rgb8_ccm_lut_chain_DS")

        def pipeline(kind):
            pipe = BurstPipeline(default_config(W, H, N, 2, False), dev)
            pipe.set_render(format=capi.OUT_RGB8, matrix=CCM, tone_lut=lut)
            if kind.endswith("denoised"):
                pipe.set_denoise(strength=3.0, radius=2, gain=2.0)
            if kind.endswith("chain_DS"):
                pipe.set_finish_chain(denoise=dict(strength=3.0, radius=2, gain=2.0), sharpen=dict(amount=1.0, sigma=SIGMA[2], radius=2))
            return pipe

        single = {k: [] for k in kinds}
        for _ in range(rounds):
            for kind in kinds:
                pipe = pipeline(kind)
                for _ in range(3):
                    pipe.process(frames)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.process(frames)
                torch.cuda.synchronize()
                single[kind].append((time.perf_counter() - t0) * 1e6)
                pipe.close()
                del pipe
                torch.cuda.empty_cache()
        out["burst"] = {kind: _stat(single[kind]) for kind in kinds}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
