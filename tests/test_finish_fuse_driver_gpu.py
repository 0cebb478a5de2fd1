"""The finish inside the burst launch, as the driver takes it (mfsr_burst_finish -> mfsr_accumulateSuperResBurstFinish):
whole bursts at 256 x 192 through BurstPipeline with the process-wide switch on and off (mfsr_set_finish_fuse) give the same
uint16 image and the same accumulators bit for bit, and mfsr_burst_debug_finish_fused says which finishes were taken inside
the launch: only the plain whole-frame uint16 finish behind a burst launch that is the burst's last fuse."""
import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi
from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
from multi_frame_super_resolution_amd.synth import make_burst

pytestmark = pytest.mark.gpu

W, H = 256, 192
NMAX = 16


@pytest.fixture(scope="module")
def frames(hip):
    fr, _, _ = make_burst(W, H, NMAX, scale=2, mono=False, seed=778, max_shift=3.0)
    return [f.to(hip.dev) for f in fr]


def _one(pipe, frames, n, want_float=False):
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for k in range(n):
        pipe.add_frame(frames[k], k == 0)
    fl, out16 = pipe.finish(want_float=want_float)
    torch.cuda.synchronize()
    taken = pipe.fused_finishes()
    return (out16.cpu().numpy().copy(), pipe._img_out.cpu().numpy().copy(), pipe._total_weights.cpu().numpy().copy(),
            fl.cpu().numpy().copy() if fl is not None else None, taken)


def _burst(hip, frames, n, fuse, hold=True, cfg_setup=None, pipe_setup=None, window=None, want_float=False):
    """One burst of the first n frames with the switch at `fuse` -> (out16, imgOut, totalWeights, float image, finishes taken
    inside the launch)"""
    cfg = default_config(W, H, n, 2, False)
    if cfg_setup:
        cfg_setup(cfg)
    hip.L.set_finish_fuse(1 if fuse else 0)
    pipe = BurstPipeline(cfg, hip.dev, window=window)
    try:
        pipe.hold_fuse(hold)
        if pipe_setup:
            pipe_setup(pipe)
        return _one(pipe, frames, n, want_float)
    finally:
        pipe.close()
        hip.L.set_finish_fuse(1)


def _same(a, b):
    assert np.array_equal(a[0], b[0]), "out16"
    assert np.array_equal(a[1], b[1], equal_nan=True), "imgOut"
    assert np.array_equal(a[2], b[2], equal_nan=True), "totalWeights"
    if a[3] is not None or b[3] is not None:
        assert np.array_equal(a[3], b[3], equal_nan=True), "float image"


@pytest.mark.parametrize("n,taken", [(7, 0), (8, 1), (9, 0), (12, 1), (16, 1)])
def test_switch_on_equals_switch_off(hip, frames, n, taken):
    """7 frames: one held group, no burst launch.  9 frames: the burst launch is not the last fuse (the ninth frame follows),
    so it must not finish."""
    on, off = _burst(hip, frames, n, True), _burst(hip, frames, n, False)
    _same(on, off)
    assert on[4] == taken and off[4] == 0


def _gamma(cfg):
    cfg.applyGamma = 1


CASES = {
    "want_float": dict(want_float=True),
    "gamma": dict(cfg_setup=_gamma),
    "render": dict(pipe_setup=lambda p: p.set_render(capi.OUT_RGB16)),
    "sharpen": dict(pipe_setup=lambda p: p.set_sharpen(0.5)),
    "denoise": dict(pipe_setup=lambda p: p.set_denoise(1.0)),
    "window": dict(window=(64, 48, 200, 120)),
    "hold off": dict(hold=False),
}


@pytest.mark.parametrize("what", list(CASES) + ["MFSR_BURST_FUSE=0"])
def test_other_finishes_keep_their_launches(hip, frames, what):
    """Everything but the plain whole-frame uint16 finish behind a burst launch: no finish inside the launch with the switch on,
    and the output of the same burst with it off."""
    kw = CASES.get(what, {})
    if what == "MFSR_BURST_FUSE=0":
        hip.L.set_burst_fuse(0)
    try:
        on, off = _burst(hip, frames, 12, True, **kw), _burst(hip, frames, 12, False, **kw)
    finally:
        hip.L.set_burst_fuse(1)
    _same(on, off)
    assert on[4] == 0 and off[4] == 0


def test_second_burst_on_the_same_context(hip, frames):
    """A burst after a finish taken inside the launch gives the image a new context gives (and takes its finish there as well)."""
    cfg = default_config(W, H, 16, 2, False)
    pipe = BurstPipeline(cfg, hip.dev)
    try:
        pipe.hold_fuse(True)
        first = _one(pipe, frames, 16)
        second = _one(pipe, frames[::-1], 16)
    finally:
        pipe.close()
    assert first[4] == 1 and second[4] == 1
    alone = _burst(hip, frames[::-1], 16, True)
    _same(second, alone)
    _same(first, _burst(hip, frames, 16, False))
