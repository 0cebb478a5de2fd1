"""Time the geometric finish: k_finishGeometry staged and with every tap read from memory
(MFSR_GEOMETRY_STAGE=0), beside mfsr_finishRendered on the same source as the yardstick, and resident bursts finished plainly
and through finish_geometry, all in one process.

Kernel, a 7680x4320 source by default, one row in twenty on the fallback, colour matrix + 4096-interval tone table, to RGB8 and
RGBA8, the calls taking turns:
(a) an output of the source's size, bilinear and cubic (the identity mapping: what the resample costs where it moves nothing);
(b) a 3/4-size output (5760x3240, step 4/3), cubic;
(c) (a) with k1 = 0.1 and lateral (1.002, 0.998);
(y) mfsr_finishRendered of the source: the yardstick (another file's kernel, untouched).
After --warmup calls, --iters calls of each as one batch of back-to-back calls between two HIP events (the queue stays full:
the device time of a call), --rounds times each.  Reported: the median microseconds and the spread over the rounds, and each
row's ratio to the yardstick of its format.  The stage knob is read at every call, so both forms run in the same turns.

Resident bursts, 16 frames of 3840x2160 by default: BurstPipeline.process (which ends in finish) to RGB8 with matrix + table,
against the same followed by finish_geometry (identity size, k1 = 0.1, lateral, cubic): what the extra launch adds.  One JSON
line.

    python tools/geometry_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5]
    python tools/geometry_bench.py --no-bursts --rounds 1 --only c_lens_cubic_rgb8_staged     # one row, e.g. under counters

Record: profiles/geometry_bench_4k16.txt.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools._stage_bench import timed

CCM = [1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56]
LENS = dict(distortion=(0.1, 0.0, 0.0), lateral=(1.002, 0.998))


def _stat(v):
    return {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}


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
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config, lens_geometry, render_row_bytes, tone_lut_srgb

    W, H, N = a.width, a.height, a.frames
    hrW, hrH = 2 * W, 2 * H
    dev = torch.device("cuda:0")
    L = capi.lib()
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    out = {"width": W, "height": H, "frames": N, "iters": iters, "rounds": rounds}

    # ---- the kernels --------------------------------------------------------------------------------------------------------
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    fin = torch.rand(hrH, hrW, 3, generator=gen, device=dev) * 2.0
    wt = torch.rand(hrH, hrW, 3, generator=gen, device=dev) * 3.5 + 0.5
    wt[::20] = 0.0                                     # one row in twenty takes the fallback resample
    fb = torch.rand(H, W, 3, generator=gen, device=dev)
    lut = tone_lut_srgb(4096).to(dev)
    outbuf = torch.empty(hrH * hrW * 4, dtype=torch.uint8, device=dev)
    thr = 1e-3
    src = (fin.data_ptr(), wt.data_ptr(), 12 * hrW, fb.data_ptr(), 12 * W, W, H, 0.0, 1.0, 0.0, 1.0)
    small = (hrW * 3 // 4, hrH * 3 // 4)
    geometries = {"a_identity_bilinear": lens_geometry(hrW, hrH, hrW, hrH, filter="bilinear"),
                  "a_identity_cubic": lens_geometry(hrW, hrH, hrW, hrH),
                  "b_threequarter_cubic": lens_geometry(hrW, hrH, *small),
                  "c_lens_bilinear": lens_geometry(hrW, hrH, hrW, hrH, filter="bilinear", **LENS),
                  "c_lens_cubic": lens_geometry(hrW, hrH, hrW, hrH, **LENS)}
    calls, keep = {}, []

    def stream():
        return torch.cuda.current_stream().cuda_stream

    for fmt, name in ((capi.OUT_RGB8, "rgb8"), (capi.OUT_RGBA8, "rgba8")):
        r = capi.Render()
        r.format = fmt
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*CCM)
        r.toneLut = lut.data_ptr()
        r.toneSize = lut.numel() - 1
        keep.append(r)

        def rendered(r=r, rb=render_row_bytes(fmt, hrW)):
            L.finishRendered(*src, None, 12 * hrW, outbuf.data_ptr(), rb, ctypes.byref(r), hrW, hrH, thr, 1, 0, 0, hrW, hrH, stream())
        calls[f"y_finishRendered_{name}"] = rendered
        for gname, g in geometries.items():
            for stage in ("staged", "direct"):
                def geo(r=r, g=g, rb=render_row_bytes(fmt, g.outW), stage=stage):
                    os.environ["MFSR_GEOMETRY_STAGE"] = "1" if stage == "staged" else "0"
                    L.finishGeometry(*src, hrW, hrH, None, 0, outbuf.data_ptr(), rb, ctypes.byref(r), ctypes.byref(g), thr, 1, 0, 0,
                                     g.outW, g.outH, stream())
                calls[f"{gname}_{name}_{stage}"] = geo
    if a.only:
        calls = {k: v for k, v in calls.items() if re.search(a.only, k)}
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    os.environ.pop("MFSR_GEOMETRY_STAGE", None)
    out["kernel"] = {"src_width": hrW, "src_height": hrH, "threequarter": list(small), **{name: _stat(v) for name, v in us.items()}}
    out["over_finishRendered"] = {k: round(statistics.median(v) / statistics.median(us["y_finishRendered_" + k.split("_")[-2]]), 3)
                                  for k, v in us.items() if not k.startswith("y_") and "y_finishRendered_" + k.split("_")[-2] in us}
    out["staged_over_direct"] = {k[:-len("_staged")]: round(statistics.median(v) / statistics.median(us[k[:-len("staged")] + "direct"]), 3)
                                 for k, v in us.items() if k.endswith("_staged") and k[:-len("staged")] + "direct" in us}
    del fin, wt, fb, outbuf
    torch.cuda.empty_cache()

    # ---- resident bursts ----------------------------------------------------------------------------------------------------
    if not a.no_bursts:
        gc = torch.Generator().manual_seed(2)
        base = torch.randint(200, 1200, (H, W), generator=gc, dtype=torch.int32)
        frames = [(base + torch.randint(0, 64, (H, W), generator=gc, dtype=torch.int32)).to(torch.int16).to(dev) for _ in range(N)]
        g = lens_geometry(hrW, hrH, hrW, hrH, **LENS)
        kinds = ("process_finish", "process_finish_then_finish_geometry")
        single = {k: [] for k in kinds}
        for _ in range(rounds):
            for kind in kinds:
                pipe = BurstPipeline(default_config(W, H, N, 2, False), dev)
                pipe.set_render(format=capi.OUT_RGB8, matrix=CCM, tone_lut=lut)

                def burst():
                    pipe.process(frames)
                    if kind.endswith("geometry"):
                        pipe.finish_geometry(g, want_float=False)

                for _ in range(3):
                    burst()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                burst()
                torch.cuda.synchronize()
                single[kind].append((time.perf_counter() - t0) * 1e6)
                pipe.close()
                del pipe
                torch.cuda.empty_cache()
        out["burst"] = {kind: _stat(single[kind]) for kind in kinds}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
