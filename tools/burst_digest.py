#!/usr/bin/env python3
"""Digest of a list of small ragged bursts, for byte-for-byte A/B of two builds of libmfsr_hip.so (the same C-ABI).

    python tools/burst_digest.py <library directory> [name ...]

One line per configuration: the sha256 (16 hex digits) of the float image, of the integer or rendered image and of both
accumulator planes, then the non-zero mfsr_burst_debug_paths counters, mfsr_burst_fuse_stats, the in-launch / sharpened /
denoised finish counters, the robust-group launches and mfsr_burst_timing_read's launch and frame counts.  A configuration
the library refuses prints the refusal instead.  Run it once per library and per environment knob, each in a fresh process,
and diff the outputs: a change that moves no arithmetic leaves every line as it was.  232 x 156 frames: the HR grid is no
multiple of the fuse tiles, the tracking image no multiple of the tracker's."""
import ctypes
import hashlib
import os
import sys

if len(sys.argv) < 2:
    sys.exit(__doc__)
os.environ["MFSR_LIB"] = os.path.join(os.path.abspath(sys.argv[1]), "libmfsr_hip.so")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from multi_frame_super_resolution_amd import capi  # noqa: E402
from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream, default_config, tone_lut_srgb  # noqa: E402
from multi_frame_super_resolution_amd.synth import make_burst  # noqa: E402

W, H = 232, 156
DEV = torch.device("cuda", 0)
GBRG, BGGR = (1, 2, 0, 1), (2, 1, 1, 0)
MATRIX = (1.6, -0.4, -0.2, -0.3, 1.5, -0.2, 0.0, -0.5, 1.5)
_frames = {}


def frames(n, scale=2, mono=False, host=False):
    key = (n, scale, mono)
    if key not in _frames:
        fr, _, _ = make_burst(W, H, n, scale=scale, mono=mono, seed=4242, max_shift=3.0)
        _frames[key] = [f.to(DEV) for f in fr], [f.cpu().pin_memory() for f in fr]
    return _frames[key][1 if host else 0]


def sha(t):
    if t is None:
        return "-" * 16
    a = t.detach().cpu().contiguous()
    return hashlib.sha256(a.view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def config(n, scale=2, mono=False, **fields):
    cfg = default_config(W, H, n, scale, mono)
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(cfg, k)[i] = x
        else:
            setattr(cfg, k, v)
    return cfg


def timing_on(pipe):
    pipe.L.burst_timing(pipe._h, 1)


def counters(pipe):
    ms, nl, nf = ctypes.c_double(0), ctypes.c_int(-1), ctypes.c_int(-1)
    pipe.L.burst_timing_read(pipe._h, ctypes.byref(ms), ctypes.byref(nl), ctypes.byref(nf))
    paths = ",".join(f"{k}={v}" for k, v in pipe.debug_paths().items() if v)
    return (f"paths[{paths}] fuse_stats={pipe.fuse_stats()} in_launch={pipe.fused_finishes()} sharpened={pipe.sharpened_finishes()} "
            f"denoised={pipe.denoised_finishes()} robust_group={pipe.robust_group_launches()} timed={nl.value}/{nf.value}")


def digest(pipe, img, out):
    torch.cuda.synchronize()
    return f"float={sha(img)} int={sha(out)} acc={sha(pipe._img_out)} w={sha(pipe._total_weights)} {counters(pipe)}"


def resident(n, scale=2, mono=False, hold=True, window=None, setup=None, flush_after=(), n_frames=None, **fields):
    """begin, reference, n_frames frames (default: n = cfg.frames), the integer image alone (the finish the burst launch may
    take), then the float image from the finished accumulators"""
    def run():
        pipe = BurstPipeline(config(n, scale, mono, **fields), DEV, window=window)
        try:
            timing_on(pipe)
            pipe.hold_fuse(hold)
            if setup:
                setup(pipe)
            fr = frames(n_frames or n, scale, mono)
            pipe.begin_burst()
            pipe.set_reference(fr[0])
            for k, f in enumerate(fr):
                pipe.add_frame(f, k == 0)
                if k + 1 in flush_after:
                    pipe.flush()
            if pipe._local_tone is not None:
                pipe.local_tone()
            if fields.get("fused", 1):
                _, out = pipe.finish(want_float=False)
                out = out.clone()
                img, _ = pipe.finish(want_u16=False)
            else:
                img, out = pipe.finish()  # (the unfused chain quantises its float image)
            return digest(pipe, img, out)
        finally:
            pipe.close()
    return run


def host(n, scale=2, setup=None, **fields):
    def run():
        pipe = BurstPipeline(config(n, scale, uploadRing=4, **fields), DEV)
        try:
            timing_on(pipe)
            if setup:
                setup(pipe)
            out = pipe.process_host(frames(n, scale, host=True))
            pipe.host_sync()
            return digest(pipe, None, out)
        finally:
            pipe.close()
    return run


def joint(n):
    def run():
        pipe = BurstPipeline(config(n), DEV)
        try:
            timing_on(pipe)
            img, out = pipe.process_joint(frames(n))
            return digest(pipe, img, out)
        finally:
            pipe.close()
    return run


def stripes(n, cuts):
    """mfsr_burst_align_frames, then mfsr_burst_fuse_rows group by group over the row stripes between `cuts`"""
    def run():
        pipe = BurstPipeline(config(n), DEV)
        try:
            timing_on(pipe)
            fr = frames(n)
            prod = [pipe.new_frame_products() for _ in fr]
            flows, masks = [p[0] for p in prod], [p[1] for p in prod]
            P = ctypes.c_void_p * n
            pipe.set_reference(fr[0])  # (no mfsr_burst_begin: the first group of every stripe overwrites the accumulators)
            pipe.L.burst_align_frames(pipe._h, n, P(*[f.data_ptr() for f in fr]), (ctypes.c_int * n)(1, *([0] * (n - 1))),
                                      P(*[f.data_ptr() for f in flows]), flows[0].stride(0) * 4, P(*[m.data_ptr() for m in masks]),
                                      masks[0].stride(0) * 4, pipe._stream())
            g = pipe.group_size()
            for r0, r1 in zip(cuts[:-1], cuts[1:]):
                for k in range(0, n, g):
                    pipe.fuse_rows(fr[k:k + g], flows[k:k + g], masks[k:k + g], r0, r1, k == 0)
            img, out = pipe.finish()
            return digest(pipe, img, out)
        finally:
            pipe.close()
    return run


def stream(n, radius, cfa):
    def run():
        fs = FrameStream(config(2 * radius + 1, cfa=cfa), radius, DEV)
        try:
            h = hashlib.sha256()
            for f in frames(n):
                got = fs.push(f)
                if got:
                    h.update(sha(got[1]).encode())
            for got in fs.drain():
                h.update(sha(got[1]).encode())
            torch.cuda.synchronize()
            return f"outputs={h.hexdigest()[:16]}"
        finally:
            fs.close()
    return run


CASES = {
    "defaults_x2_n9": resident(9),
    "defaults_x2_n16": resident(16),
    "x2_n5_nohold": resident(5, hold=False),
    "x4_n5": resident(5, scale=4),
    "host_x2_n8": host(8),
    "mono_x2_n5": resident(5, mono=True),
    "gbrg_x2_n9": resident(9, cfa=GBRG),
    "bggr_x4_n3": resident(3, scale=4, cfa=BGGR),
    "window_x2": resident(5, window=(40, 24, 200, 120)),
    "window_x4": resident(5, scale=4, window=(40, 24, 200, 120)),
    "unfused_x2_n3": resident(3, fused=0),
    "nopair_x2_n5": resident(5, pairFrames=0),
    "prealign_x2_n5": resident(5, preAlign=1),
    "asyncfuse_x2_n9": resident(9, asyncFuse=1),
    "lk_h5_x2_n5": resident(5, lkHalfWindow=5),
    "host_x4_n5": host(5, scale=4),
    "rendered_rgb8_lut": resident(5, setup=lambda p: p.set_render(capi.OUT_RGB8, matrix=MATRIX, tone_lut=tone_lut_srgb())),
    "rendered_nv12": resident(5, setup=lambda p: p.set_render(capi.OUT_NV12, matrix=MATRIX)),
    "sharpened": resident(5, setup=lambda p: p.set_sharpen(1.0)),
    "denoised": resident(5, setup=lambda p: p.set_denoise(3.0)),
    "local_tone": resident(5, setup=lambda p: p.set_local_tone()),
    "host_rendered": host(8, setup=lambda p: p.set_render(capi.OUT_RGB8, matrix=MATRIX, tone_lut=tone_lut_srgb())),
    "stream_gbrg_r1": stream(6, 1, GBRG),
    # the fuse queue of the driver: groups that wait in the burst hold, the held group of a host burst, caller-driven stripes
    "hold_n17_ring8": resident(8, n_frames=17),
    "hold_n16_flush6": resident(16, flush_after=(6,)),
    "align_frames_fuse_rows": stripes(9, (0, 160, 2 * H)),
    "joint_x2_n5": joint(5),
    "host_sharpened": host(8, setup=lambda p: p.set_sharpen(1.0)),
}


def main():
    names = sys.argv[2:] or list(CASES)
    for name in names:
        try:
            line = CASES[name]()
        except (capi.MfsrError, ValueError) as e:
            line = "refused: " + repr(e)[:100]
        print(f"{name:24s} {line}", flush=True)


if __name__ == "__main__":
    main()
