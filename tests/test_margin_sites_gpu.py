"""The site-wise body of the x2 margin kernels (accumulate_common.hpp: accumulate_pixel_sites; k_accumulateMargin,
k_accumulateMarginN, k_accumulateMarginBurst with SITES) against the per-tap body it replaces, selected with
mfsr_set_margin_sites(0).

The contract is bit identity: both accumulator planes, the whole image, np.array_equal with the switch on against the switch
off -- no tolerance, no pixel left out -- through every entry point that launches a margin kernel: mfsr_accumulateSuperResFullN
with 1 .. 4 frames, ...FullRows with row windows that cut the margin bands, ...FullWindow, and ...Burst with 8, 12 and 16
frames; each fresh (accumulatorsUndefined) and on random accumulators, every buffer between guards.

Shapes: raw 136 x 36 and 36 x 136 (the smallest frames with live rows between the bands; the tall one is nearly all side
columns) and the ragged 328 x 104.  Inputs are the ones that can break a tap -> site or tap -> cell mapping: constant flows of
each parity, parity alternating per texel, +-45 HR pixels towards each corner (sites clamped at all four borders, far past the
certainty clamp), NaN / Inf / 1e9 flows (the per-tap path of flows beyond 2^30), certainty that differs on every texel and
channel with NaN / Inf / negative texels, kernel texels that are NaN, overflowing, not positive semi-definite or >= 1e30 inside
the ring (the per-tap path), raw 0 and 65535, white and black levels that differ per channel, all four Bayer patterns."""
import ctypes

import numpy as np
import pytest

from tests.kernels import guarded_upload, pitch_of
from tests.test_fuse_tile_layout_gpu import _parity_flow
from tests.test_parity_kernels import PATTERNS, _accum_inputs, _kernel_field

pytestmark = pytest.mark.gpu

WIDE, TALL, BIG = (136, 36), (36, 136), (328, 104)
SHAPES = [WIDE, TALL, BIG]
WHITE, BLACK = [3839, 3700, 3900], [256, 260, 250]
KINDS = ["parity", "alternating", "border", "wild"]
PATS = list(PATTERNS)


def _kernel_param(seed, fh, fw):
    """_kernel_field (a NaN texel at (0, 0) and an overflowing one at (1, 1): both in the ring) plus, in the ring's other three
    sides, texels that are not positive semi-definite, negative, and >= 1e30: those pixels take the per-tap path."""
    kp = _kernel_field(seed, fh, fw, 4)
    kp[fh - 1, 4:7, 2] = 4.0          # kz^2 > kx ky
    kp[fh // 2, 0, 0] = -0.5
    kp[fh // 2 + 1, fw - 1, 0] = 2e30
    kp[2, fw - 2, 1] = np.inf
    return kp


def _mask(seed, W, H):
    """certainty that identifies its texel: a different value on every texel and channel (a wrong cell or a wrong component
    changes the sums), with NaN, Inf and negative texels, some of them in the ring's corners"""
    mh, mw = (H + 1) // 2, (W + 1) // 2
    yy, xx = np.mgrid[0:mh, 0:mw]
    r = np.random.default_rng(seed)
    m = np.zeros((mh, mw, 4), np.float32)
    for c in range(4):
        m[..., c] = 0.2 + 0.5 * ((xx + c) & 1) + 0.25 * ((yy + (c >> 1)) & 1) + 0.001 * ((3 * xx + 5 * yy + c) % 17)
    bad = r.random((mh, mw, 4)) < 0.03
    m[bad] = r.choice(np.float32([np.nan, np.inf, -np.inf, -0.75]), int(bad.sum()))
    m[0, 0, 0], m[0, mw - 1, 1], m[mh - 1, 0, 2], m[mh - 1, mw - 1, :3] = np.nan, np.inf, -1.5, [np.nan, -2.0, np.inf]
    return m


def _flow(kind, k, fh, fw, seed):
    if kind == "parity":
        return _parity_flow(k, 0, fh, fw)
    if kind == "alternating":
        return _parity_flow(k, 1, fh, fw)
    if kind == "border":    # 45 HR pixels towards one corner, half a pixel of parity on top
        sx, sy = [(1, 1), (-1, -1), (1, -1), (-1, 1)][k % 4]
        return np.ascontiguousarray(np.zeros((fh, fw, 2), np.float32) + np.float32([22.5 * sx + 0.5 * (k & 1), 22.5 * sy - 0.5 * ((k >> 1) & 1)]))
    r = np.random.default_rng(seed + k)
    f = r.uniform(-3.0, 3.0, (fh, fw, 2)).astype(np.float32)
    hostile = np.float32([np.nan, np.inf, -np.inf, 1e9, -1e9, 3e9])
    for i in range(12):   # around the ring: rows 0 and fh - 1, columns 0 and fw - 1
        y, x = [(0, i * 3 % fw), (fh - 1, i * 5 % fw), (i * 2 % fh, 0), (i * 3 % fh, fw - 1)][i % 4]
        f[y, x, i % 2] = hostile[i % len(hostile)]
    f[fh // 2, fw // 2] = np.nan
    return np.ascontiguousarray(f)


def _frames(n, kinds, W, H, seed):
    fh, fw = H // 2, W // 2
    frames = []
    for k in range(n):
        raw = _accum_inputs(seed + k, W, H, 2, 2)[0].copy()
        r = np.random.default_rng(seed + 100 + k)
        ext = r.random(raw.shape)
        raw[ext < 0.02] = 0
        raw[ext > 0.98] = 65535
        raw[0, 0], raw[0, -1], raw[-1, 0], raw[-1, -1] = 0, 65535, 65535, 0
        frames.append((raw, _mask(seed + 200 + k, W, H), _flow(kinds[k % len(kinds)], k + n, fh, fw, seed + 300)))
    return frames


def _launch(hip, entry, frames, kp, W, H, acc_i, acc_w, fresh, extra=()):
    """One entry point on guarded buffers -> (imgOut, totalWeights).  acc_i / acc_w: the accumulator planes as the entry point
    takes them (the whole HR frame; the window alone for FullWindow)."""
    import torch
    n = len(frames)
    fh, fw = frames[0][2].shape[:2]
    mh, mw = frames[0][1].shape[:2]
    checks = []

    def gup(a):
        t, c = guarded_upload(a, hip.dev)
        checks.append(c)
        return t

    d_raw = [gup(f[0]) for f in frames]
    d_mask = [gup(f[1]) for f in frames]
    d_sh = [gup(f[2]) for f in frames]
    d_kp = gup(kp)
    d_i, d_w = gup(acc_i), gup(acc_w)
    T2 = hip.capi.Tex2D
    P = ctypes.c_void_p * n
    raws = P(*[t.data_ptr() for t in d_raw])
    shs = (T2 * n)(*[T2(t.data_ptr(), fw * 8, fw, fh) for t in d_sh])
    tkp = T2(d_kp.data_ptr(), fw * 16, fw, fh)
    white, black = hip.capi.f3(WHITE), hip.capi.f3(BLACK)
    if entry == "Burst":
        hrh, hrw = acc_i.shape[:2]
        masks = (T2 * n)(*[T2(t.data_ptr(), mw * 16, mw, mh) for t in d_mask])
        hip.L.accumulateSuperResBurst(n, raws, T2(d_i.data_ptr(), pitch_of(acc_i), hrw, hrh), T2(d_w.data_ptr(), pitch_of(acc_w), hrw, hrh),
                                      masks, tkp, shs, white, black, 2, fresh, None)
    else:
        masks = P(*[t.data_ptr() for t in d_mask])
        fn = getattr(hip.L, "accumulateSuperResFull" + entry)
        fn(n, raws, d_i.data_ptr(), d_w.data_ptr(), masks, tkp, shs, white, black, W, H, 2, pitch_of(acc_i), mw * 16, fresh, *extra, None)
    torch.cuda.synchronize()
    for i, c in enumerate(checks):
        c(f"mfsr_accumulateSuperRes{'' if entry == 'Burst' else 'Full'}{entry}, buffer {i}", unchanged=i < len(checks) - 2)
    return d_i.cpu().numpy(), d_w.cpu().numpy()


def _assert_on_equals_off(hip, entry, frames, kp, W, H, seed, extra=(), acc_shape=None):
    shape = acc_shape or (2 * H, 2 * W, 3)
    r = np.random.default_rng(seed)
    a_i, a_w = r.random(shape, dtype=np.float32), r.random(shape, dtype=np.float32)
    try:
        for fresh in (1, 0):
            got = {}
            for sites in (0, 1):
                hip.L.set_margin_sites(sites)
                got[sites] = _launch(hip, entry, frames, kp, W, H, a_i.copy(), a_w.copy(), fresh, extra)
            for name, on, off in zip(("imgOut", "totalWeights"), got[1], got[0]):
                same = (on.view(np.uint32) == off.view(np.uint32)) | (np.isnan(on) & np.isnan(off))
                bad = np.argwhere(~same)
                assert bad.size == 0, f"{entry} fresh={fresh} {name}: {len(bad)} values differ, first (y, x, c) = {bad[0].tolist()}"
                assert np.array_equal(on, off, equal_nan=True)
            if not fresh:
                assert not np.array_equal(got[1][1], a_w, equal_nan=True)   # the launch accumulated something
    finally:
        hip.L.set_margin_sites(1)


def _case(hip, shape_i, k):
    """shape, frame dims and a Bayer pattern that rotates with the case"""
    W, H = SHAPES[shape_i]
    hip.set_cfa(PATTERNS[PATS[(shape_i + k) % 4]])
    return W, H, _kernel_param(700 + shape_i, H // 2, W // 2)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("shape_i", [0, 1, 2])
def test_full_n(hip, shape_i, n):
    W, H, kp = _case(hip, shape_i, n)
    try:
        for i, kind in enumerate(KINDS):
            _assert_on_equals_off(hip, "N", _frames(n, [kind], W, H, 710 + 10 * i), kp, W, H, 719 + i)
    finally:
        hip.set_cfa(PATTERNS["RGGB"])


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("shape_i", [0, 1, 2])
def test_full_rows_cutting_the_bands(hip, shape_i, n):
    """row windows [0, 16), [16, last), [last, hrH) and one that ends inside the lower band's 16-row block"""
    W, H, kp = _case(hip, shape_i, n + 1)
    hrH = 2 * H
    last = hrH // 16 * 16 if hrH % 16 else hrH - 16
    try:
        frames = _frames(n, KINDS, W, H, 760)
        for r0, r1 in [(0, 16), (16, last), (last, hrH), (0, hrH)]:
            _assert_on_equals_off(hip, "Rows", frames, kp, W, H, 769, extra=(r0, r1))
    finally:
        hip.set_cfa(PATTERNS["RGGB"])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape_i", [0, 1, 2])
def test_full_window(hip, shape_i, n):
    """windows over each corner of the ring, one inside the side columns only, and the whole frame; the accumulators hold the
    window alone"""
    W, H, kp = _case(hip, shape_i, n + 2)
    hrW, hrH = 2 * W, 2 * H
    try:
        frames = _frames(n, KINDS[::-1], W, H, 780)
        xr, yb = (hrW - 17) // 16 * 16, (hrH - 17) // 16 * 16     # the last 16-aligned origins that take in the whole ring
        for x, y, w, h in [(0, 0, 48, 32), (xr, 0, hrW - xr, 32), (0, yb, 32, hrH - yb), (xr, yb, hrW - xr, hrH - yb),
                           (0, 16, 32, yb - 16), (0, 0, hrW, hrH)]:
            _assert_on_equals_off(hip, "Window", frames, kp, W, H, 789, extra=(x, y, w, h), acc_shape=(h, w, 3))
    finally:
        hip.set_cfa(PATTERNS["RGGB"])


@pytest.mark.parametrize("n", [8, 12, 16])
@pytest.mark.parametrize("shape_i", [0, 1, 2])
def test_burst(hip, shape_i, n):
    W, H, kp = _case(hip, shape_i, n // 4)
    try:
        _assert_on_equals_off(hip, "Burst", _frames(n, KINDS, W, H, 800 + n), kp, W, H, 809)
    finally:
        hip.set_cfa(PATTERNS["RGGB"])
