"""What the stage benches share (select_bench, defect_bench, exposure_bench, noise_bench, erode_bench): the timing of one call
with HIP events, and the turns of ``bench.py`` between this tree and a built checkout of the parent commit."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, warmup: int, iters: int, singles: bool = True):
    """(median, min, batched, iters) microseconds per call of ``fn`` on the current stream after ``warmup`` calls: ``iters``
    calls timed one by one (each includes the host's enqueue latency; None, None with ``singles=False``), then ``iters``
    calls back to back between one pair of events (the queue stays full: the device time of a call)."""
    import torch

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters if singles else 0):
        e0, e1 = events()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    e0, e1 = events()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    batch = e0.elapsed_time(e1) * 1e3 / iters
    return (statistics.median(times), min(times), batch, iters) if singles else (None, None, batch, iters)


def bench_turns(parent: str, rounds: int):
    """``bench.py --gpus 1 --steps 10 --warmup 3`` of this tree and of ``parent`` taking turns, ``rounds`` times each, every
    run in a child process of its own; prints one JSON line per run."""
    for r in range(rounds):
        for name, d in (("this tree", ROOT), ("parent", parent)):
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"], cwd=d,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"bench.py of {name} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
            j = json.loads(line)
            print(json.dumps({"bench": name, "round": r, "ms_per_step": j.get("ms_per_step"),
                              "out16_sha256_16": j.get("out16_sha256_16")}), flush=True)
