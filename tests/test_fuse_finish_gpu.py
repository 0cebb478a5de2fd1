"""The finishing form of the burst warp+fuse launch (accumulate_fast.hip: k_accumulate2xTileBurst<CFA, true> and k_finishRing)
through mfsr_accumulateSuperResBurstFinish on guarded buffers.

The contract is bit identity with the two calls it replaces: mfsr_accumulateSuperResBurst followed by mfsr_finishFused on the
same inputs give the same uint16 image and the same two accumulator planes (np.array_equal, no tolerance).  out16 starts as a
canary in both runs, so a pixel the finishing launch leaves out -- tile epilogue and ring together must write every HR pixel --
differs as well.

Inputs: the hostile frames of tests/test_fuse_burst_gpu.py (_burst_frames), with a block of certainty cells zeroed in every
frame -- those pixels accumulate a weight of exactly 0 -- and alternating zero cells next to it.  With fresh = 0 the weight
plane is preloaded by rows of eight, so that the waves of the tile kernel (one HR row of a 256-pixel tile each) see: every
channel of every pixel below the threshold (rows 0, 1 of eight), all above it (2, 3), four-pixel strips -- lanes --
alternating (4, 5), pixels alternating (6) and a single channel below (7); and the value plane holds NaN, large negative and
large positive sums, which the quantiser clamps.  The share of pixels that take the fallback is asserted to lie in 5 .. 95 %
on the accumulators of the separate path.

Shapes: raw 328 x 104 (HR 656 x 208: two whole tiles and a partial one with live strips) and raw 136 x 36 (HR 272 x 72, the
smallest frame with live rows: its partial tile's columns are all ring).
"""
import ctypes

import numpy as np
import pytest

from tests.kernels import guarded_upload, pitch_of
from tests.test_fuse_burst_gpu import BIG, BLACK, E_INVALID, E_UNSUPPORTED, OK, SMALL, WHITE, _burst_frames
from tests.test_fuse_tile_layout_gpu import _smooth_kernel_field
from tests.test_parity_kernels import PATTERNS, _accum_inputs, _kernel_field, rng

pytestmark = pytest.mark.gpu

THR = 1e-3
CANARY = 0xC3C3


def _frames(n, W, H, seed):
    """_burst_frames with certainty cells that are zero in every frame: a block (weights exactly 0 over whole waves) and, right
    of it, every other cell of every other cell row (lanes and pixels with and without weight side by side)"""
    mh, mw = (H + 1) // 2, (W + 1) // 2
    out = []
    for raw, mask, flow in _burst_frames(n, W, H, seed):
        m = mask.copy()
        m[mh // 4:mh // 4 + mh // 3, 2:mw // 2] = 0.0
        m[mh // 4:mh // 4 + mh // 3:2, mw // 2:mw - 3:2] = 0.0
        out.append((raw, np.ascontiguousarray(m), flow))
    return out


def _preloaded(seed, W, H):
    """accumulators a launch with fresh = 0 starts from (see the module's text)"""
    _, a_i, a_w, _ = _accum_inputs(seed, W, H, 2 * W, 2 * H)
    a_w += np.float32(0.5)                      # (plainly above the threshold where nothing below lowers it)
    y = np.arange(2 * H)[:, None] % 8
    x = np.arange(2 * W)[None, :]
    low = (y < 2) | ((y >= 4) & (y < 6) & ((x // 4) % 2 == 0)) | ((y == 6) & (x % 2 == 0))
    a_w[low] = np.float32(-1e6)
    a_w[..., 1][np.broadcast_to(y == 7, low.shape)] = np.float32(-1e6)
    # weights that stay exactly 0: inside the block of zero certainty cells (_frames; a cell is four HR pixels, the taps reach two)
    mh, mw = (H + 1) // 2, (W + 1) // 2
    a_w[4 * (mh // 4) + 4:4 * (mh // 4 + mh // 3) - 4, 12:4 * (mw // 2) - 4] = 0.0
    a_i[::5, ::7] = np.nan
    a_i[1::5, ::3] = np.float32(-1e7)
    a_i[2::5, 1::3] = np.float32(1e7)
    return a_i, a_w


def _fallback(seed, W, H):
    return rng(seed).random((H, W, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)   # (some of it outside 0 .. 1)


def _run(hip, frames, kp, acc_i, acc_w, fresh, fb, fused, scale=2, thr=THR, gamma=0, window=None, expect=None):
    """fused: mfsr_accumulateSuperResBurstFinish; else mfsr_accumulateSuperResBurst then mfsr_finishFused, on guarded buffers
    -> (imgOut, totalWeights, out16).  With `expect` (a refusal) every buffer must come back unchanged."""
    import torch
    n = len(frames)
    fh, fw = frames[0][2].shape[:2]
    hrh, hrw = acc_i.shape[:2]
    checks = []

    def gup(a):
        t, c = guarded_upload(a, hip.dev)
        checks.append(c)
        return t

    d_raw = [gup(f[0]) for f in frames]
    d_mask = [gup(f[1]) for f in frames]
    d_sh = [gup(f[2]) for f in frames]
    d_kp = gup(kp)
    d_fb = gup(fb) if fb is not None else None
    n_in = len(checks)
    d_i, d_w = gup(acc_i), gup(acc_w)
    d_q = gup(np.full((hrh, hrw, 3), CANARY, np.uint16))
    T2 = hip.capi.Tex2D
    mh, mw = frames[0][1].shape[:2]
    raws = (ctypes.c_void_p * n)(*[t.data_ptr() for t in d_raw])
    masks = (T2 * n)(*[T2(t.data_ptr(), mw * 16, mw, mh) for t in d_mask])
    shs = (T2 * n)(*[T2(t.data_ptr(), fw * 8, fw, fh) for t in d_sh])
    ti, tw = T2(d_i.data_ptr(), pitch_of(acc_i), hrw, hrh), T2(d_w.data_ptr(), pitch_of(acc_w), hrw, hrh)
    tk = T2(d_kp.data_ptr(), fw * 16, fw, fh)
    fbh, fbw = fb.shape[:2] if fb is not None else (0, 0)
    fb_ptr = d_fb.data_ptr() if fb is not None else None
    if fused:
        x0, y0, w, h = window if window else (0, 0, hrw, hrh)
        rc = hip.L.raw["mfsr_accumulateSuperResBurstFinish"](n, raws, ti, tw, masks, tk, shs, hip.capi.f3(WHITE), hip.capi.f3(BLACK), scale,
                                                             fresh, T2(fb_ptr, fbw * 12, fbw, fbh), 0.0, 1.0, 0.0, 1.0, thr,
                                                             d_q.data_ptr(), w, h, gamma, 65535.0, x0, y0, hrw, hrh, None)
    else:
        rc = hip.L.raw["mfsr_accumulateSuperResBurst"](n, raws, ti, tw, masks, tk, shs, hip.capi.f3(WHITE), hip.capi.f3(BLACK), scale,
                                                       fresh, None)
        assert rc == OK, rc
        rc = hip.L.raw["mfsr_finishFused"](d_i.data_ptr(), d_w.data_ptr(), pitch_of(acc_i), fb_ptr, fbw * 12, fbw, fbh, 0.0, 1.0, 0.0, 1.0,
                                           None, 0, d_q.data_ptr(), hrw, hrh, thr, 0, 65535.0, None)
    torch.cuda.synchronize()
    what = "mfsr_accumulateSuperResBurstFinish" if fused else "mfsr_accumulateSuperResBurst + mfsr_finishFused"
    for i, c in enumerate(checks):
        c(f"{what}, buffer {i}", unchanged=(expect is not None) or i < n_in)
    assert rc == (OK if expect is None else expect), rc
    return d_i.cpu().numpy(), d_w.cpu().numpy(), d_q.cpu().numpy().view(np.uint16)


def _assert_same(hip, frames, kp, W, H, fresh, seed, with_fallback=True, thr=THR):
    a_i, a_w = _preloaded(seed, W, H)
    fb = _fallback(seed + 1, W, H) if with_fallback else None
    ref = _run(hip, frames, kp, a_i.copy(), a_w.copy(), fresh, fb, False, thr=thr)
    got = _run(hip, frames, kp, a_i.copy(), a_w.copy(), fresh, fb, True, thr=thr)
    # neither branch of the finish goes untested: on the separate path's accumulators
    below = (ref[1] < np.float32(thr)).any(axis=-1)
    share = float(below.mean())
    print(f"pixels taking the fallback: {share:.3f}; weights exactly 0: {int((ref[1] == 0).sum())}")
    assert 0.05 <= share <= 0.95, share
    assert (ref[1] == 0).any(), "no weight is exactly 0"
    if not fresh:
        assert np.isnan(ref[0]).any() and (ref[0] < 0).any() and (ref[0] > 1e6).any()
        # whole rows (so whole waves) under the threshold, whole rows above it, strips alternating within a row
        strips = below[16:-16, 16:-16].reshape(below.shape[0] - 32, -1, 4)
        assert strips.all(axis=(1, 2)).any() and (~strips).all(axis=(1, 2)).any()
        assert (strips.all(axis=2)[:, :-1] != strips.all(axis=2)[:, 1:]).all(axis=1).any()
    assert not (ref[2] == CANARY).all(axis=-1).any(), "the separate finish left a pixel unwritten"
    assert np.array_equal(got[0], ref[0], equal_nan=True), "imgOut"
    assert np.array_equal(got[1], ref[1], equal_nan=True), "totalWeights"
    bad = np.argwhere((got[2] != ref[2]).any(axis=-1))
    assert bad.size == 0, f"out16 differs at {len(bad)} pixels, first (y, x) = {bad[0].tolist()}: {got[2][tuple(bad[0])]} / {ref[2][tuple(bad[0])]}"
    return ref


@pytest.mark.parametrize("fresh", [1, 0])
@pytest.mark.parametrize("n", [8, 16])
def test_finish_equals_burst_then_finish(hip, n, fresh):
    W, H = BIG
    hip.set_cfa(PATTERNS["RGGB"])
    kp = _kernel_field(610, H // 2, W // 2, 4)
    _assert_same(hip, _frames(n, W, H, 620), kp, W, H, fresh, 619)


@pytest.mark.parametrize("pat", ["GBRG", "BGGR"])
def test_other_patterns_and_twelve_frames(hip, pat):
    W, H = BIG
    hip.set_cfa(PATTERNS[pat])
    kp = _kernel_field(630, H // 2, W // 2, 4)
    try:
        _assert_same(hip, _frames(12, W, H, 640), kp, W, H, 0 if pat == "GBRG" else 1, 639)
    finally:
        hip.set_cfa(PATTERNS["RGGB"])


@pytest.mark.parametrize("fresh", [1, 0])
@pytest.mark.parametrize("n", [8, 16])
def test_smallest_frame(hip, n, fresh):
    W, H = SMALL
    hip.set_cfa(PATTERNS["RGGB"])
    kp = _kernel_field(650, H // 2, W // 2, 4)
    _assert_same(hip, _frames(n, W, H, 660), kp, W, H, fresh, 659)


@pytest.mark.parametrize("thr", [THR, 0.0])
def test_null_fallback_and_zero_weights(hip, thr):
    """No fallback image: pixels under the threshold are val / (w + 1).  Threshold 0: a weight of exactly 0 is not under it, is
    not divided by, and gives 0."""
    W, H = BIG
    hip.set_cfa(PATTERNS["RGGB"])
    kp = _smooth_kernel_field(670, H // 2, W // 2)
    ref = _assert_same(hip, _frames(8, W, H, 680), kp, W, H, 0, 679, with_fallback=False, thr=thr)
    if thr == 0.0:
        zero = (ref[1] == 0)
        assert (ref[2][zero] == 0).all()


@pytest.mark.parametrize("case", ["7 frames", "10 frames", "20 frames", "mono", "x4", "gamma", "window"])
def test_refusals_touch_nothing(hip, case):
    """The refusals of mfsr_accumulateSuperResBurst, and everything but the plain finish of the whole frame: each returns its
    status and leaves every buffer -- accumulators, out16, guards -- as it was."""
    W, H = SMALL
    n = {"7 frames": 7, "10 frames": 10, "20 frames": 20}.get(case, 8)
    s = 4 if case == "x4" else 2
    hip.set_cfa([1, 1, 1, 1] if case == "mono" else PATTERNS["RGGB"])
    try:
        fh, fw = H // 2, W // 2
        kp = _smooth_kernel_field(690, fh, fw)
        frames = []
        for k in range(n):
            raw, _, _, mask = _accum_inputs(691 + k, W, H, s * W, s * H)
            frames.append((raw, mask, np.zeros((fh, fw, 2), np.float32)))
        _, a_i, a_w, _ = _accum_inputs(699, W, H, s * W, s * H)
        _run(hip, frames, kp, a_i, a_w, 0, _fallback(698, W, H), True, scale=s, gamma=1 if case == "gamma" else 0,
             window=(16, 16, 64, 32) if case == "window" else None, expect=E_INVALID if "frames" in case else E_UNSUPPORTED)
    finally:
        hip.set_cfa(PATTERNS["RGGB"])
