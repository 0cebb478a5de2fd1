"""The burst form of the x2 Bayer warp+fuse tile kernel (accumulate_fast.hip: k_accumulate2xTileBurst, the 8 / 12 / 16-frame
margin launch) through mfsr_accumulateSuperResBurst on guarded buffers.

The contract is bit identity: 8, 12 or 16 frames in one launch give, on both accumulator planes, exactly what that many
four-frame mfsr_accumulateSuperResFullN calls give on the same inputs (np.array_equal, no tolerance) -- fresh
(accumulatorsUndefined on the first call) and on top of random accumulators.  The inputs are chosen so that a group boundary
can go wrong: a frame slot saturated in one group and not in the next, parity-alternating flows that differ per group, strips
refused in the second group only (each way of being refused), kernel texels that are not positive semi-definite (every group
takes the in-kernel straight path on planes that hold the groups before it), NaN certainties.

Shapes: raw 328 x 104, the ragged shape of the group tests (two whole 256-pixel tiles and a partial one with live strips, rows no
multiple of 16), and raw 136 x 36, the smallest frame the tile kernel admits that has a partial tile and live rows between
the margin bands (HR 272 x 72: live rows 16 .. 55; the partial tile's 16 columns are all side margin, so it stages and writes
chunks that only the margin kernel changes).
"""
import ctypes

import numpy as np
import pytest

from tests.kernels import F3, Tex, guarded_upload, pitch_of
from tests.test_fuse_tile_layout_gpu import _parity_flow, _plane_masks, _smooth_kernel_field
from tests.test_parity_kernels import PATTERNS, _accum_inputs, _accumulate_group_hip, _kernel_field

pytestmark = pytest.mark.gpu

BIG, SMALL = (328, 104), (136, 36)
WHITE, BLACK = [3839, 3700, 3900], [256, 260, 250]
M = 16          # STRIP_MARGIN: the ring the margin kernel owns
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -2   # include/mfsr.h: MFSR_OK, MFSR_E_INVALID, MFSR_E_UNSUPPORTED


def _burst_hip(hip, frames, kp, W, H, acc_i, acc_w, fresh, scale=2, expect=None):
    """mfsr_accumulateSuperResBurst on guarded buffers -> (imgOut, totalWeights, status).  With `expect` (a refusal) every
    buffer, the accumulators included, must come back unchanged."""
    import torch
    n = len(frames)
    fh, fw = frames[0][2].shape[:2]
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
    mh, mw = frames[0][1].shape[:2]
    raws = (ctypes.c_void_p * n)(*[t.data_ptr() for t in d_raw])
    masks = (T2 * n)(*[T2(t.data_ptr(), mw * 16, mw, mh) for t in d_mask])
    shs = (T2 * n)(*[T2(t.data_ptr(), fw * 8, fw, fh) for t in d_sh])
    hrh, hrw = acc_i.shape[:2]
    rc = hip.L.raw["mfsr_accumulateSuperResBurst"](n, raws, T2(d_i.data_ptr(), pitch_of(acc_i), hrw, hrh),
                                                   T2(d_w.data_ptr(), pitch_of(acc_w), hrw, hrh), masks,
                                                   T2(d_kp.data_ptr(), fw * 16, fw, fh), shs, hip.capi.f3(WHITE), hip.capi.f3(BLACK),
                                                   scale, fresh, None)
    torch.cuda.synchronize()
    for i, c in enumerate(checks):
        c(f"mfsr_accumulateSuperResBurst, buffer {i}", unchanged=(expect is not None) or i < len(checks) - 2)
    if expect is not None:
        assert rc == expect, rc
    else:
        assert rc == OK, rc
    return d_i.cpu().numpy(), d_w.cpu().numpy(), rc


def _groups_hip(hip, frames, kp, W, H, acc_i, acc_w, fresh):
    """the launches the burst form replaces: four frames per mfsr_accumulateSuperResFullN call, fresh on the first"""
    fh, fw = frames[0][2].shape[:2]
    i, w = acc_i, acc_w
    for g in range(0, len(frames), 4):
        i, w = _accumulate_group_hip(hip, frames[g:g + 4], kp, fw, fh, W, H, 2, F3(WHITE), F3(BLACK), i, w, fresh if g == 0 else 0)
    return i, w


def _ring(a):
    """the margin ring's pixels: top band, bottom band, left and right side chunks"""
    return a[:M], a[-M:], a[M:-M, :M], a[M:-M, -M:]


def _assert_same(hip, frames, kp, W, H, fresh, seed):
    _, a_i, a_w, _ = _accum_inputs(seed, W, H, 2 * W, 2 * H)
    ref_i, ref_w = _groups_hip(hip, frames, kp, W, H, a_i.copy(), a_w.copy(), fresh)
    got_i, got_w, _ = _burst_hip(hip, frames, kp, W, H, a_i.copy(), a_w.copy(), fresh)
    # the margin ring first (its own launch: one thread per pixel and frame, the frames added in call order): the top and
    # bottom bands, which a fresh call zeroes and only the margin kernel writes, and the side chunks, which a non-fresh tile
    # launch stages and must not write back
    for name, g, r in (("imgOut", got_i, ref_i), ("totalWeights", got_w, ref_w)):
        for part, gp, rp in zip(("top band", "bottom band", "left chunks", "right chunks"), _ring(g), _ring(r)):
            assert np.array_equal(gp, rp, equal_nan=True), f"{name}: {part} of the margin ring differ"
        assert np.array_equal(g, r, equal_nan=True), f"{name}: the tile kernel's pixels differ"
    assert np.abs(got_w - a_w).max() > 0.5   # the launch accumulated something
    return got_i, got_w


def _burst_frames(n, W, H, seed, nan_frac=0.01):
    """n frames whose groups differ where the kernel keeps per-group state: the certainty of frame slot j is saturated in one
    group and random in the next (strip_pixel_sat / strip_pixel_w), the flow of slot j alternates parity in one group and is
    constant in the next, and every group has its own base flow."""
    fh, fw = H // 2, W // 2
    mh, mw = (H + 1) // 2, (W + 1) // 2
    ones = np.ones((mh, mw, 4), np.float32)
    big_masks = _plane_masks() if (W, H) == BIG else None
    frames = []
    for k in range(n):
        g, j = divmod(k, 4)
        raw, _, _, mask = _accum_inputs(seed + k, W, H, 2 * W, 2 * H, nan_frac=nan_frac)
        if (g + j) % 2 == 0:
            mask = ones                                   # saturated here, not in the neighbouring groups
        elif big_masks is not None and j == 1:
            mask = big_masks[g % 3]                       # three-valued texels on the tiles' footprint edges, NaN included
        flow = _parity_flow((k + g) % 4, (g + j) & 1, fh, fw)
        frames.append((raw, np.ascontiguousarray(mask), flow))
    return frames


@pytest.mark.parametrize("fresh", [1, 0])
@pytest.mark.parametrize("pat", ["RGGB", "GBRG", "BGGR"])
@pytest.mark.parametrize("n", [8, 12, 16])
def test_burst_equals_group_launches(hip, n, pat, fresh):
    W, H = BIG
    hip.set_cfa(PATTERNS[pat])
    kp = _kernel_field(510, H // 2, W // 2, 4)   # a NaN and an overflowing texel: those strips take the straight path in every group
    _assert_same(hip, _burst_frames(n, W, H, 520), kp, W, H, fresh, 519)


@pytest.mark.parametrize("fresh", [1, 0])
@pytest.mark.parametrize("n", [8, 16])
def test_burst_equals_group_launches_smallest_frame(hip, n, fresh):
    W, H = SMALL
    hip.set_cfa(PATTERNS["RGGB"])
    kp = _kernel_field(530, H // 2, W // 2, 4)
    _assert_same(hip, _burst_frames(n, W, H, 540), kp, W, H, fresh, 539)


@pytest.mark.parametrize("kind", ["window", "wild", "nan", "margin"])
def test_strips_refused_in_the_second_group_only(hip, kind):
    """Group 1 is admitted everywhere (smooth PSD kernel field, small constant flows); in group 2 some strips are refused, so
    the in-kernel straight path runs on planes that already hold group 1: beyond the 8-bit window around the tile's own flow
    (d = 128 / -129), wild (1e9) flow, NaN flow, and a flow that carries the taps of the outermost live strips past the frame."""
    W, H = BIG
    fh, fw = H // 2, W // 2
    hip.set_cfa(PATTERNS["RGGB"])
    kp = _smooth_kernel_field(550, fh, fw)
    frames = []
    for k in range(8):
        raw, _, _, mask = _accum_inputs(551 + k, W, H, 2 * W, 2 * H)
        flow = np.zeros((fh, fw, 2), np.float32) + np.float32([0.5 * (k % 3), -0.5 * (k % 2)])
        if k >= 4:
            if kind == "window":
                flow[12:16, 8:11, 0] += 64.0      # d = +128
                flow[40:43, 70:73, 1] -= 64.5     # d = -129
            elif kind == "wild":
                flow[10:14, 10:14] = 1e9
                flow[30:33, 100:104] = -1e9
            elif kind == "nan":
                flow[20:23, 60:63] = np.nan
                flow[5, 130] = np.inf
            else:
                flow[...] = np.float32([7.5, -7.5]) if k & 1 else np.float32([-7.5, 7.5])
        frames.append((raw, mask, np.ascontiguousarray(flow)))
    _assert_same(hip, frames, kp, W, H, 0, 559)


def test_non_psd_kernel_texels_take_the_straight_path_in_every_group(hip):
    W, H = BIG
    fh, fw = H // 2, W // 2
    hip.set_cfa(PATTERNS["GBRG"])
    kp = _smooth_kernel_field(560, fh, fw)
    kp[..., 2] = 4.0                       # kz^2 > kx * ky on every texel: no strip is admitted
    kp[::7, ::5, 0] = -0.5
    frames = _burst_frames(8, W, H, 561)
    _assert_same(hip, frames, kp, W, H, 1, 569)
    _assert_same(hip, frames, kp, W, H, 0, 569)


def test_sixteen_frames_against_the_oracle(orc, hip):
    """One 16-frame burst launch against the oracle's frame-by-frame accumulateSuperResFull, at the tolerance of the group
    tests (the fast path re-associates the sums)."""
    W, H = BIG
    fh, fw = H // 2, W // 2
    orc.set_cfa(PATTERNS["RGGB"])
    hip.set_cfa(PATTERNS["RGGB"])
    kp = _kernel_field(570, fh, fw, 4)
    frames = _burst_frames(16, W, H, 571)
    _, oi, ow, _ = _accum_inputs(589, W, H, 2 * W, 2 * H)
    hi, hw = oi.copy(), ow.copy()
    for raw, m, sh in frames:
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), F3(WHITE), F3(BLACK), W, H, 2, pitch_of(oi), pitch_of(m))
    gi, gw, _ = _burst_hip(hip, frames, kp, W, H, hi, hw, 0)
    np.testing.assert_allclose(gw, ow, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(gi, oi, rtol=3e-5, atol=3e-5)


@pytest.mark.parametrize("case", ["7 frames", "10 frames", "4 frames", "20 frames", "mono", "x4", "fields at the raw size"])
def test_refusals_touch_nothing(hip, case):
    """Frame counts that are not two to four whole groups are invalid; a monochrome pattern, scale 4 and fields that are not at
    HR/4 are not the burst kernel's geometry.  Each returns its status and leaves every buffer, guards included, as it was."""
    W, H = SMALL
    n = {"7 frames": 7, "10 frames": 10, "4 frames": 4, "20 frames": 20}.get(case, 8)
    s = 4 if case == "x4" else 2
    hip.set_cfa([1, 1, 1, 1] if case == "mono" else PATTERNS["RGGB"])
    fh, fw = (H, W) if case == "fields at the raw size" else (H // 2, W // 2)
    kp = _smooth_kernel_field(590, fh, fw)
    frames = []
    for k in range(n):
        raw, _, _, mask = _accum_inputs(591 + k, W, H, s * W, s * H)
        frames.append((raw, mask, np.zeros((fh, fw, 2), np.float32)))
    _, a_i, a_w, _ = _accum_inputs(599, W, H, s * W, s * H)
    _burst_hip(hip, frames, kp, W, H, a_i, a_w, 0, scale=s, expect=E_INVALID if "frames" in case else E_UNSUPPORTED)
    hip.set_cfa(PATTERNS["RGGB"])
