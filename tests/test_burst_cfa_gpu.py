"""A burst and a frame stream take their CFA pattern from cfg.cfa alone: the process-wide pattern of mfsr_set_cfa_pattern (the
port of the reference's c_cfaPattern, which the reference-shaped kernel entry points read) is neither read nor written by the
driver, so bursts with different patterns can be interleaved on one thread or run on two.

Everything here is byte identity (np.array_equal on the accumulators and the u16 image) between two runs of the same driver
calls.  Sizes are the ragged ones of test_burst_matches_oracle_ragged_sizes (partial 256-pixel tiles, partial tracker tiles);
the frame counts make the three fuse forms run: a four-frame group's tile launch, a remainder fused alone, and -- with the
burst hold -- two groups in one burst launch."""
import ctypes
import threading

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi

pytestmark = pytest.mark.gpu

PATTERNS = {"RGGB": [0, 1, 1, 2], "BGGR": [2, 1, 1, 0], "GRBG": [1, 0, 2, 1], "GBRG": [1, 2, 0, 1]}
DEV = "cuda:0"


def _lib():
    import torch  # noqa: F401  (before the library is loaded: the process then has torch's HIP runtime alone)
    return capi.lib()


def _set_global(name):
    _lib().set_cfa_pattern((ctypes.c_int32 * 4)(*PATTERNS[name]))


def _get_global():
    got = (ctypes.c_int32 * 4)()
    _lib().get_cfa_pattern(got)
    return list(got)


@pytest.fixture(autouse=True)
def _rggb_around():
    _set_global("RGGB")
    yield
    _set_global("RGGB")


def _cfg(W, H, N, scale, cfa, fused=1):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, N, scale, False)
    cfg.fused = fused
    for i in range(4):
        cfg.cfa[i] = PATTERNS[cfa][i]
    return cfg


def _frames(W, H, N, scale, seed):
    import torch
    from multi_frame_super_resolution_amd.synth import make_burst
    frames, _, _ = make_burst(W, H, N, scale=scale, mono=False, seed=seed, max_shift=3.0)
    return [f.to(torch.device(DEV)) for f in frames]


class _Burst:
    """One burst as a list of driver calls (steps), so that two bursts can take turns; `before` runs ahead of each."""

    def __init__(self, cfg, frames, hold, before=None):
        import torch
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        self.pipe = BurstPipeline(cfg, torch.device(DEV))
        self.pipe.hold_fuse(hold)
        self.frames, self.before, self.res = frames, before or (lambda: None), None
        ref = cfg.reference
        self.steps = [self.pipe.begin_burst, lambda: self.pipe.set_reference(frames[ref])]
        self.steps += [lambda k=k: self.pipe.add_frame(frames[k], k == ref) for k in range(len(frames))]
        self.steps += [self.pipe.flush, self._finish]

    def _finish(self):
        _, out16 = self.pipe.finish()   # (the unfused chain's finish needs the float image as well)
        self.res = dict(out16=out16.cpu().numpy().copy(), img_out=self.pipe.img_out.cpu().numpy().copy(),
                        tw=self.pipe.total_weights.cpu().numpy().copy(), fuse=self.pipe.fuse_stats(), paths=self.pipe.debug_paths())

    def step(self, i):
        self.before()
        self.steps[i]()

    def run(self):
        for i in range(len(self.steps)):
            self.step(i)
        return self.close()

    def close(self):
        self.pipe.close()
        return self.res


def _assert_same_bytes(a, b, what):
    for k in ("img_out", "tw", "out16"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs"
    assert a["fuse"] == b["fuse"] and a["paths"] == b["paths"], what
    assert a["tw"].max() > 0.5 and a["out16"].max() > 0, what   # the burst fused and finished something


@pytest.mark.parametrize("W,H,N,scale,fused,hold", [(268, 196, 5, 2, 1, False), (392, 264, 9, 2, 1, True), (328, 200, 3, 4, 1, False),
                                                    (268, 196, 3, 2, 0, False)])
def test_burst_ignores_the_process_wide_pattern(W, H, N, scale, fused, hold):
    cfg = _cfg(W, H, N, scale, "BGGR", fused)
    frames = _frames(W, H, N, scale, 4321 + W)
    quiet = _Burst(cfg, frames, hold).run()
    assert _get_global() == PATTERNS["RGGB"]
    noisy = _Burst(cfg, frames, hold, before=lambda: _set_global("GRBG")).run()
    _assert_same_bytes(quiet, noisy, f"{W}x{H} N={N} x{scale} fused={fused}")
    assert _get_global() == PATTERNS["GRBG"]
    # the forms the frame counts are chosen for
    p = quiet["paths"]
    assert p["frames_deferred"] + p["frames_immediate"] == N
    if hold:
        assert quiet["fuse"] == (1, 2)           # two four-frame groups in one burst launch; the ninth frame alone
    else:
        assert quiet["fuse"] == (0, 0)
    if fused:
        assert p["align_batches"] >= 1 and p["prepare_fused"] >= 1 and p["prepare_chain"] == 0
    else:
        assert p["prepare_chain"] >= 1 and p["prepare_fused"] == 0 and p["robust_chain"] >= 1 and p["lk_chain"] >= 1   # the kernel chain


def _pair():
    W, H, N = 268, 196, 5
    return [(_cfg(W, H, N, 2, cfa), _frames(W, H, N, 2, seed)) for cfa, seed in (("RGGB", 1201), ("GBRG", 1202))]


@pytest.fixture(scope="module")
def alone():
    """pipelines A (RGGB) and B (GBRG), each run on its own"""
    return [_Burst(cfg, frames, False).run() for cfg, frames in _pair()]


def test_two_bursts_interleaved_on_one_thread(alone):
    a, b = [_Burst(cfg, frames, False) for cfg, frames in _pair()]
    for i in range(len(a.steps)):
        a.step(i)
        b.step(i)
    _assert_same_bytes(a.close(), alone[0], "A, interleaved with B")
    _assert_same_bytes(b.close(), alone[1], "B, interleaved with A")
    assert _get_global() == PATTERNS["RGGB"]


def test_two_bursts_on_two_threads(alone):
    import torch
    bursts = [_Burst(cfg, frames, False) for cfg, frames in _pair()]
    torch.cuda.synchronize()
    gate, errors = threading.Barrier(2), []

    def work(burst):
        try:
            stream = torch.cuda.Stream(device=DEV)
            gate.wait(timeout=60)
            with torch.cuda.stream(stream):
                for i in range(len(burst.steps)):
                    burst.step(i)
            stream.synchronize()
        except Exception as e:   # noqa: BLE001 (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(x,)) for x in bursts]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    _assert_same_bytes(bursts[0].close(), alone[0], "A, beside B on another thread")
    _assert_same_bytes(bursts[1].close(), alone[1], "B, beside A on another thread")


def _stream_outputs(cfg, frames):
    import torch
    from multi_frame_super_resolution_amd.pipeline import FrameStream
    fs = FrameStream(cfg, radius=1, device=torch.device(DEV))
    outs = []
    for f in frames:
        r = fs.push(f)
        if r is not None:
            outs.append((r[0], r[1].cpu().numpy().copy()))
    outs += [(t, img.cpu().numpy().copy()) for t, img in fs.drain()]
    fs.close()
    return outs


def test_frame_stream_ignores_the_process_wide_pattern():
    W, H = 268, 196
    cfg = _cfg(W, H, 3, 2, "GRBG")
    frames = _frames(W, H, 3, 2, 1301)
    under_rggb = _stream_outputs(cfg, frames)
    assert _get_global() == PATTERNS["RGGB"]
    _set_global("GRBG")
    under_grbg = _stream_outputs(cfg, frames)
    assert [t for t, _ in under_rggb] == [t for t, _ in under_grbg] == [0, 1, 2]
    for (t, a), (_, b) in zip(under_rggb, under_grbg):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"output {t}"
        assert a.max() > 0
