"""Time packed raw input: k_unpackRaw alone, and host bursts that take packed frames beside the unpacked
host burst of the same samples, all in one process.  16 frames of 3840x2160 RGGB by default.

Kernel: mfsr_unpackRaw for the four packings on both paths (sources at a 4-byte aligned base: dword loads and 16-byte stores;
the same sources one byte further: byte loads and 16-bit stores) and mfsr_applyGains on frames of the same size beside them,
the calls taking turns; after --warmup calls, --iters calls of each as one batch of back-to-back calls between two HIP events
(the queue stays full: the device time of a call), --rounds times each.  Reported: the median microseconds, the spread over
the rounds and GB/s of the bytes moved (unpack: packed bytes in + 2 bytes per sample out; gains: 2 in + 2 out).

Host bursts: BurstPipeline.process_host on one pipeline each for unpacked, MIPI10 and MIPI12 frames of the same burst (the
12-bit samples of synth-like noise; shifted right by two for MIPI10, whose levels are scaled to match), taking turns: one
burst at a time (process_host + host_sync, wall clock from the first call to the image in host memory) and --burst-batch
bursts back to back (one host_sync at the end, per burst), --rounds times each.  One JSON line.

    python tools/packed_bench.py [--width 3840 --height 2160 --frames 16 --iters 50 --warmup 5 --rounds 5] [--parent DIR]

Record: profiles/packed_bench_4k16.txt.
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

from tools._stage_bench import bench_turns, timed


def _stat(v, moved=None):
    med = statistics.median(v)
    out = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2)}
    if moved is not None:
        out["gb_per_s"] = round(moved / med / 1e3, 1)
    return out


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
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: bench.py of both trees taking turns first")
    ap.add_argument("--ab-rounds", type=int, default=2)
    a = ap.parse_args()
    if a.parent:
        bench_turns(os.path.abspath(a.parent), a.ab_rounds)

    import torch
    from multi_frame_super_resolution_amd import capi, synth
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config, exposure_defaults, packed_row_bytes

    W, H, N = a.width, a.height, a.frames
    dev = torch.device("cuda:0")
    L = capi.lib()
    names = {capi.PACK_MIPI10: "mipi10", capi.PACK_MIPI12: "mipi12", capi.PACK_BE10: "be10", capi.PACK_BE12: "be12"}
    rounds, iters = max(a.rounds, 1), max(a.iters, 20)
    out = {"width": W, "height": H, "frames": N, "iters": iters, "rounds": rounds}

    # ---- the kernel ---------------------------------------------------------------------------------------------------------
    g = torch.Generator(device="cuda:0").manual_seed(1)
    frames = [torch.randint(0, 4096, (H, W), generator=g, device=dev, dtype=torch.int32).to(torch.int16) for _ in range(N)]
    fptrs = (ctypes.c_void_p * N)(*[f.data_ptr() for f in frames])
    cfg = default_config(W, H, N, 2, False)
    d = exposure_defaults(cfg)
    I4 = ctypes.c_int32 * 4
    gains = (ctypes.c_int32 * (3 * N))(*[v for k in range(N) for v in [65536 + (300 if k % 2 else -300)] * 3])
    status = (ctypes.c_int32 * N)(*([0] * N))
    calls, moved = {}, {}

    def gain():
        L.applyGains(N, fptrs, 2 * W, W, H, I4(*cfg.cfa), 0, I4(*d.black), d.sat, d.max_value, gains, status,
                     torch.cuda.current_stream().cuda_stream)

    keep = []
    for packing, name in names.items():
        dense = packed_row_bytes(packing, W)
        for path, off in (("dword", 0), ("byte", 1)):
            # random bytes are valid packed frames of any of the four layouts
            bufs = [torch.randint(0, 256, (dense * H + 16,), generator=g, device=dev, dtype=torch.int32).to(torch.uint8) for _ in range(N)]
            keep.append(bufs)
            sptrs = (ctypes.c_void_p * N)(*[b.data_ptr() + off for b in bufs])

            def unpack(sptrs=sptrs, dense=dense, packing=packing):
                L.unpackRaw(N, sptrs, dense, packing, fptrs, 2 * W, W, H, torch.cuda.current_stream().cuda_stream)

            calls[f"unpack_{name}_{path}"] = unpack
            moved[f"unpack_{name}_{path}"] = (dense + 2 * W) * H * N
    calls["apply_gains"] = gain
    moved["apply_gains"] = 4 * W * H * N
    us = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            us[name].append(timed(fn, max(a.warmup, 1), iters, singles=False)[2])
    out["kernel"] = {name: _stat(v, moved[name]) for name, v in us.items()}
    del keep, frames
    torch.cuda.empty_cache()

    # ---- host bursts --------------------------------------------------------------------------------------------------------
    if not a.no_bursts:
        gc = torch.Generator().manual_seed(2)
        base = torch.randint(200, 1200, (H, W), generator=gc, dtype=torch.int32)
        burst12 = [(base + torch.randint(0, 64, (H, W), generator=gc, dtype=torch.int32)).to(torch.int16) for _ in range(N)]
        kinds = {}
        for name, packing in (("unpacked", 0), ("mipi10", capi.PACK_MIPI10), ("mipi12", capi.PACK_MIPI12)):
            c = default_config(W, H, N, 2, False)
            c.uploadRing = min(N, 32)
            c.rawPacking = packing
            src = burst12
            if packing == capi.PACK_MIPI10:
                src = [(f.to(torch.int32) >> 2).to(torch.int16) for f in burst12]
                for i in range(3):
                    c.black[i], c.white[i] = c.black[i] / 4, 1023.0 - c.black[i] / 4
                c.maxVal = 1023.0
            host = [t.pin_memory() for t in (synth.pack_raw(src, packing) if packing else src)]
            pipe = BurstPipeline(c, dev)
            kinds[name] = (pipe, host, sum(t.numel() * t.element_size() for t in host))
            for _ in range(3):
                pipe.process_host(host)
                pipe.host_sync()
        single = {k: [] for k in kinds}
        batched = {k: [] for k in kinds}
        for _ in range(rounds):
            for name, (pipe, host, _) in kinds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.process_host(host)
                pipe.host_sync()
                single[name].append((time.perf_counter() - t0) * 1e6)
            for name, (pipe, host, _) in kinds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.burst_batch):
                    pipe.process_host(host)
                pipe.host_sync()
                batched[name].append((time.perf_counter() - t0) * 1e6 / a.burst_batch)
        out["host_burst"] = {name: {"upload_bytes": kinds[name][2], "one_at_a_time": _stat(single[name]),
                                    "back_to_back": _stat(batched[name])} for name in kinds}
        out["burst_batch"] = a.burst_batch
        for pipe, _, _ in kinds.values():
            pipe.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
