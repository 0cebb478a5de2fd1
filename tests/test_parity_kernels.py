"""GPU parity: every HIP entry point of include/mfsr.h against the CPU oracle on
the same seeded inputs.

Tolerances (north_star: +-1 LSB on outputs, DeBayer bit-exact):
  * kernels made of + - * / fabs only (A1-A3, B1-B8 except the wave-sum in
    squaredSum, C*, E2, H1, box filters, fused tracker) : BIT-EXACT;
  * kernels with transcendentals (exp, pow, sin/cos/atan2) or re-ordered sums:
    the tolerance is written next to each assertion.
"""
import ctypes

import numpy as np
import pytest

from tests.kernels import F2, F3, Host, Tex, guarded_upload, pitch_of
from tests.tracker_ref import oracle_track

pytestmark = pytest.mark.gpu

RGGB = [0, 1, 1, 2]
PATTERNS = {"RGGB": [0, 1, 1, 2], "BGGR": [2, 1, 1, 0], "GRBG": [1, 0, 2, 1], "GBRG": [1, 2, 0, 1]}


def rng(seed):
    return np.random.default_rng(seed)


def run_both(orc, hip, fname, make):
    """make() -> (args, outputs): fresh arrays each time; returns (oracle_outputs, hip_outputs)."""
    res = []
    for k in (orc, hip):
        args, outs = make()
        k.call(fname, *args)
        res.append([o.copy() for o in outs])
    return res


def assert_bitexact(a, b, what=""):
    a = np.asarray(a)
    b = np.asarray(b)
    same = (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a == b)
    if a.dtype == np.float32:
        same = same | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {a.size} elements differ, max |d| = {np.nanmax(np.abs(a - b))}"


# ---------------------------------------------------------------- A: DeBayer
@pytest.mark.parametrize("pat", list(PATTERNS))
@pytest.mark.parametrize("shape", [(32, 32), (48, 64)])
def test_deBayersSubSample3(orc, hip, pat, shape):
    hh, hw = shape
    orc.set_cfa(PATTERNS[pat])
    hip.set_cfa(PATTERNS[pat])

    def make():
        raw = rng(1).integers(0, 4096, (2 * hh, 2 * hw), dtype=np.uint16)
        out = np.zeros((hh, hw + 3, 3), np.float32)  # odd pitch
        return (raw, out, 4095.0, hw, hh, pitch_of(out)), [out]

    (o,), (h,) = run_both(orc, hip, "deBayersSubSample3", make)
    assert_bitexact(o, h, "deBayersSubSample3")
    assert o[:, :hw].max() > 0


@pytest.mark.parametrize("pat", list(PATTERNS))
def test_deBayer_green_redblue_and_fused(orc, hip, pat):
    H, W = 40, 72
    orc.set_cfa(PATTERNS[pat])
    hip.set_cfa(PATTERNS[pat])
    bp = F3([256, 250, 260])
    sc = F3([1 / 3839.0, 1 / 3800.0, 1 / 3850.0])
    raw16 = rng(2).integers(200, 4096, (H, W), dtype=np.uint16)

    def make():
        rawf = raw16.astype(np.float32)
        out = np.zeros((H, W, 3), np.float32)
        return rawf, out

    outs = []
    for k in (orc, hip):
        rawf, out = make()
        k.call("deBayerGreenKernel", W, H, rawf, pitch_of(rawf), out, pitch_of(out), bp, sc)
        g = out.copy()
        k.call("deBayerRedBlueKernel", W, H, rawf, pitch_of(rawf), out, pitch_of(out), bp, sc)
        outs.append((g, out.copy()))
    assert_bitexact(outs[0][0], outs[1][0], "deBayerGreenKernel")
    assert_bitexact(outs[0][1], outs[1][1], "deBayerRedBlueKernel")
    # border ring untouched
    assert (outs[1][1][:2] == 0).all() and (outs[1][1][:, :2] == 0).all()
    # fused A2+A3 == two-launch chain, bit for bit
    fused = np.zeros((H, W, 3), np.float32)
    hip.call("deBayerFused", raw16.copy(), fused, pitch_of(fused), W, H, bp, sc)
    assert_bitexact(outs[0][1], fused, "deBayerFused vs oracle chain")


# ---------------------------------------------------------------- G: accumulate
def _accum_inputs(seed, W, H, hrW, hrH, nan_frac=0.0):
    r = rng(seed)
    raw = r.integers(256, 4096, (H, W), dtype=np.uint16)
    imgOut = r.random((hrH, hrW, 3), dtype=np.float32)
    tw = r.random((hrH, hrW, 3), dtype=np.float32)
    mask = r.random(((H + 1) // 2, (W + 1) // 2, 4), dtype=np.float32)
    if nan_frac:
        m = r.random(mask.shape) < nan_frac
        mask[m] = np.nan
    return raw, imgOut, tw, mask


def _kernel_field(seed, h, w, chan):
    # positive-definite-ish inverse covariances with a few hostile values
    r = rng(seed)
    k = np.zeros((h, w, chan), np.float32)
    k[..., 0] = r.uniform(0.05, 3.0, (h, w))
    k[..., 1] = r.uniform(0.05, 3.0, (h, w))
    k[..., 2] = r.uniform(-0.2, 0.2, (h, w))
    k[0, 0, :3] = np.nan            # -> w non finite -> axis rule (DeBayerKernels.cu:429-430)
    k[1, 1, :3] = [-50, -50, 0]     # exp overflow -> inf -> axis rule
    return k


@pytest.mark.parametrize("fast", [0, 1])
def test_accumulateImagesSuperRes_crop(orc, hip, fast):
    W, H = 96, 64
    orc.set_cfa(RGGB)
    hip.set_cfa(RGGB)
    hip.L.set_accumulate_fast_exp(fast)
    white, black = F3([3839, 3839, 3839]), F3([256, 256, 256])

    def make():
        raw, imgOut, tw, mask = _accum_inputs(3, W, H, W, H, nan_frac=0.01)
        kp = _kernel_field(4, H // 2, W // 2, 4)
        sh = rng(5).uniform(-3, 3, (H // 2, W // 2, 2)).astype(np.float32)
        args = (raw, imgOut, tw, mask, Tex(kp), Tex(sh), white, black, W, H, pitch_of(imgOut), pitch_of(mask))
        return args, [imgOut, tw]

    (oi, ow), (hi, hw_) = run_both(orc, hip, "accumulateImagesSuperRes", make)
    hip.L.set_accumulate_fast_exp(1)
    # exp differs by <= 2 ulp (ocml) / ~1e-6 rel (v_exp path); 25 taps of O(1) values
    tol = 2e-6 if fast == 0 else 2e-5
    np.testing.assert_allclose(hi, oi, rtol=tol, atol=tol)
    np.testing.assert_allclose(hw_, ow, rtol=tol, atol=tol)
    # border ring untouched
    raw, imgOut, tw, mask = _accum_inputs(3, W, H, W, H, nan_frac=0.01)
    assert_bitexact(hi[0], imgOut[0])
    assert_bitexact(hi[:, 0], imgOut[:, 0])


@pytest.mark.parametrize("scale", [1, 2, 3, 4])
def test_accumulateSuperResFull(orc, hip, scale):
    W, H = 64, 48
    hrW, hrH = W * scale, H * scale
    orc.set_cfa(PATTERNS["GRBG"])
    hip.set_cfa(PATTERNS["GRBG"])
    hip.L.set_accumulate_fast_exp(0)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])

    def make():
        raw, imgOut, tw, mask = _accum_inputs(6 + scale, W, H, hrW, hrH)
        kp = _kernel_field(7, H // 2, W // 2, 4)
        sh = rng(8).uniform(-4, 4, (H // 2, W // 2, 2)).astype(np.float32)
        args = (raw, imgOut, tw, mask, Tex(kp), Tex(sh), white, black, W, H, scale, pitch_of(imgOut), pitch_of(mask))
        return args, [imgOut, tw]

    (oi, ow), (hi, hw_) = run_both(orc, hip, "accumulateSuperResFull", make)
    hip.L.set_accumulate_fast_exp(1)
    np.testing.assert_allclose(hi, oi, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(hw_, ow, rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("field", ["quarter", "half", "odd"])
@pytest.mark.parametrize("pat", ["RGGB", "BGGR", "GRBG", "GBRG", "MONO"])
def test_accumulate_x2_strip_kernel(orc, hip, pat, field):
    """The restructured x2 strip kernel (accumulate_fast.hip) against the oracle AND against the
    straight kernel: big flows so that border strips take the per-pixel fallback, NaN certainties,
    hostile kernel parameters, every supported CFA."""
    W, H, s = 160, 96, 2
    cfa = [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]
    orc.set_cfa(cfa)
    hip.set_cfa(cfa)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])

    # field resolution: HR/4 (Bayer pipeline, shared-texel path FR=4), HR/2 (mono pipeline, FR=2),
    # anything else (per-pixel fetch, FR=0)
    fh, fw = {"quarter": (H // 2, W // 2), "half": (H, W), "odd": (H // 2 + 3, W // 2 + 5)}[field]

    def make():
        raw, imgOut, tw, mask = _accum_inputs(90, W, H, W * s, H * s, nan_frac=0.01)
        kp = _kernel_field(91, fh, fw, 4)
        sh = rng(92).uniform(-6, 6, (fh, fw, 2)).astype(np.float32)
        sh[10:14, 10:14] = 1e9       # wild flow -> fallback path
        sh[20, 20] = np.nan
        args = (raw, imgOut, tw, mask, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(imgOut), pitch_of(mask))
        return args, [imgOut, tw]

    args, (oi, ow) = make()
    orc.call("accumulateSuperResFull", *args)
    res = {}
    for mode in (1, 2):
        hip.L.set_accumulate_fast_exp(mode)
        args, (hi, hw_) = make()
        hip.call("accumulateSuperResFull", *args)
        res[mode] = (hi.copy(), hw_.copy())
    hip.L.set_accumulate_fast_exp(2)
    for mode in (1, 2):
        np.testing.assert_allclose(res[mode][0], oi, rtol=3e-5, atol=3e-5)
        np.testing.assert_allclose(res[mode][1], ow, rtol=3e-5, atol=3e-5)
    # strip vs straight kernel (same exp): only the re-association of the channel sums differs
    np.testing.assert_allclose(res[2][0], res[1][0], rtol=1e-5, atol=1e-5)
    assert not np.array_equal(res[2][0], res[1][0]) or pat == "MONO"   # the strip path really ran


@pytest.mark.parametrize("field", ["quarter", "half"])
@pytest.mark.parametrize("pat", ["RGGB", "GBRG", "MONO"])
def test_accumulate_x2_two_frames_per_call(orc, hip, pat, field):
    """accumulateSuperResFull2 (two frames, one pass over the accumulators) == two oracle calls.
    quarter-resolution fields take the fused LDS tile kernel, half-resolution ones the per-frame path."""
    W, H, s = 192, 96, 2
    cfa = [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]
    orc.set_cfa(cfa)
    hip.set_cfa(cfa)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = {"quarter": (H // 2, W // 2), "half": (H, W)}[field]

    def make():
        raw0, imgOut, tw, mask0 = _accum_inputs(120, W, H, W * s, H * s, nan_frac=0.01)
        raw1, _, _, mask1 = _accum_inputs(121, W, H, W * s, H * s, nan_frac=0.01)
        kp = _kernel_field(122, fh, fw, 4)
        # smooth-ish flows (many strips on the fast path) with a wild patch and a NaN texel
        yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
        sh0 = np.stack([1.3 + 0.01 * xx, -2.2 + 0.02 * yy], -1).astype(np.float32)
        sh1 = np.stack([-3.6 - 0.015 * yy, 0.4 + 0.01 * xx], -1).astype(np.float32)
        sh0[10:14, 10:14] = 1e9
        sh1[20, 20] = np.nan
        return raw0, raw1, imgOut, tw, mask0, mask1, kp, sh0, sh1

    raw0, raw1, oi, ow, m0, m1, kp, sh0, sh1 = make()
    for raw, m, sh in ((raw0, m0, sh0), (raw1, m1, sh1)):
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    raw0, raw1, hi, hw_, m0, m1, kp, sh0, sh1 = make()
    hip.call("accumulateSuperResFull2", raw0, raw1, hi, hw_, m0, m1, Tex(kp), Tex(sh0), Tex(sh1), white, black, W, H, s,
             pitch_of(hi), pitch_of(m0))
    np.testing.assert_allclose(hi, oi, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(hw_, ow, rtol=3e-5, atol=3e-5)
    assert np.abs(hw_).max() > 0.5


@pytest.mark.parametrize("fresh", [0, 1])
@pytest.mark.parametrize("n,field,s,pat", [(3, "quarter", 2, "RGGB"), (4, "quarter", 2, "RGGB"), (4, "quarter", 2, "GBRG"),
                                           (4, "quarter", 2, "MONO"), (3, "half", 2, "RGGB"), (3, "half", 2, "MONO"), (4, "quarter", 4, "RGGB")])
def test_accumulate_groups_of_three_and_four(orc, hip, n, field, s, pat, fresh):
    """mfsr_accumulateSuperResFullN with 3 / 4 frames == that many oracle calls in the same order.  x2 with quarter-resolution
    fields: ONE launch of the LDS tile kernel (pixel-major, tap weights once per pixel, one plane-set staged at a time)
    plus one margin launch; the other geometries split the group.  fresh: the accumulators hold garbage and are overwritten."""
    import torch
    W, H = 328, 104   # ragged: the last 256-pixel tile is partial; rows not a multiple of 16
    cfa = [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]
    orc.set_cfa(cfa)
    hip.set_cfa(cfa)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = {"quarter": (H // 2, W // 2), "half": (H, W)}[field]
    if s == 4:
        fh, fw = H // 2, W // 2
    kp = _kernel_field(170, fh, fw, 4)
    yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
    frames = []
    for k in range(n):
        raw, _, _, mask = _accum_inputs(171 + k, W, H, W * s, H * s, nan_frac=0.01)
        sh = np.stack([1.3 - 0.9 * k + 0.01 * xx, -2.2 + 1.1 * k + 0.02 * yy], -1).astype(np.float32)
        if k == 0:
            sh[10:14, 10:14] = 1e9      # wild patch: these strips take the straight arithmetic inside the tile kernel
        if k == n - 1:
            sh[20, 20] = np.nan
        frames.append((raw, mask, np.ascontiguousarray(sh)))
    _, oi, ow, _ = _accum_inputs(199, W, H, W * s, H * s, nan_frac=0.0)
    hi0, hw0 = oi.copy(), ow.copy()
    if fresh:
        oi[:] = 0
        ow[:] = 0
    for raw, m, sh in frames:
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    checks = []

    def gup(a):
        t, c = guarded_upload(a, hip.dev)
        checks.append(c)
        return t

    d_raw = [gup(f[0]) for f in frames]
    d_mask = [gup(f[1]) for f in frames]
    d_sh = [gup(f[2]) for f in frames]
    d_kp = gup(kp)
    d_i, d_w = gup(hi0), gup(hw0)
    P = ctypes.c_void_p * n
    T = hip.capi.Tex2D * n
    shs = T(*[hip.capi.Tex2D(t.data_ptr(), fw * 8, fw, fh) for t in d_sh])
    hip.L.accumulateSuperResFullN(n, P(*[t.data_ptr() for t in d_raw]), d_i.data_ptr(), d_w.data_ptr(),
                                  P(*[t.data_ptr() for t in d_mask]), hip.capi.Tex2D(d_kp.data_ptr(), fw * 16, fw, fh), shs,
                                  hip.capi.f3(white.v), hip.capi.f3(black.v), W, H, s, pitch_of(oi), pitch_of(frames[0][1]), fresh, None)
    torch.cuda.synchronize()
    for i, c in enumerate(checks):
        c(f"mfsr_accumulateSuperResFullN, buffer {i}", unchanged=i < len(checks) - 2)
    hi, hw_ = d_i.cpu().numpy(), d_w.cpu().numpy()
    np.testing.assert_allclose(hw_, ow, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(hi, oi, rtol=3e-5, atol=3e-5)
    assert np.abs(hw_).max() > 0.5


def _accumulate_group_hip(hip, frames, kp, fw, fh, W, H, s, white, black, acc_i, acc_w, fresh):
    import torch
    n = len(frames)
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
    P = ctypes.c_void_p * n
    T = hip.capi.Tex2D * n
    shs = T(*[hip.capi.Tex2D(t.data_ptr(), fw * 8, fw, fh) for t in d_sh])
    hip.L.accumulateSuperResFullN(n, P(*[t.data_ptr() for t in d_raw]), d_i.data_ptr(), d_w.data_ptr(),
                                  P(*[t.data_ptr() for t in d_mask]), hip.capi.Tex2D(d_kp.data_ptr(), fw * 16, fw, fh), shs,
                                  hip.capi.f3(white.v), hip.capi.f3(black.v), W, H, s, pitch_of(acc_i), pitch_of(frames[0][1]), fresh, None)
    torch.cuda.synchronize()
    for i, c in enumerate(checks):
        c(f"mfsr_accumulateSuperResFullN, buffer {i}", unchanged=i < len(checks) - 2)
    return d_i.cpu().numpy(), d_w.cpu().numpy()


@pytest.mark.parametrize("n,field,s,pat", [(4, "quarter", 2, "RGGB"), (4, "quarter", 2, "GBRG"), (3, "quarter", 2, "BGGR"), (2, "quarter", 2, "GRBG"),
                                           (4, "half", 2, "MONO"), (4, "quarter", 4, "RGGB"), (2, "quarter", 4, "GBRG")])
def test_accumulate_saturated_certainty_path(orc, hip, n, field, s, pat):
    """The tile kernels take a cheaper pixel body for the frames whose certainty is exactly (1, 1, 1) on every texel a wave
    reads (strip_pixel_sat: the robustness mask saturates over well-aligned content).  Masks here are saturated over
    whole frames, over parts of a frame, everywhere but isolated texels, and not at all -- so neighbouring waves take
    different bodies -- against the oracle; and the two bodies are BIT-identical where they compute the same pixel: a
    frame of ones (saturated body) against ones with one texel column in 64 lowered (general body in every wave), compared
    on the pixels whose taps do not read a lowered texel."""
    W, H = 840, 88
    cfa = [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]
    orc.set_cfa(cfa)
    hip.set_cfa(cfa)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = {"quarter": (H // 2, W // 2), "half": (H, W)}[field]
    kp = _kernel_field(270, fh, fw, 4)
    yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
    mh, mw = (H + 1) // 2, (W + 1) // 2
    r = rng(271)

    def frame(k, mask):
        raw, _, _, _ = _accum_inputs(272 + k, W, H, W * s, H * s)
        sh = np.stack([1.3 - 0.9 * k + 0.01 * xx, -2.2 + 1.1 * k + 0.02 * yy], -1).astype(np.float32)
        return raw, np.ascontiguousarray(mask.astype(np.float32)), np.ascontiguousarray(sh)

    ones = np.ones((mh, mw, 4), np.float32)
    part = ones.copy()
    part[:, : mw // 3] = r.random((mh, mw // 3, 4), dtype=np.float32)          # left third unsaturated
    part[mh // 2:, mw // 2: mw // 2 + 40, 1] = 0.999999                         # one channel just below 1
    dots = ones.copy()
    dots[r.integers(0, mh, 12), r.integers(0, mw, 12), r.integers(0, 3, 12)] = 0.25
    dots[3, 5] = np.nan                                                         # sanitised to 0: not saturated
    rand = r.random((mh, mw, 4), dtype=np.float32)
    masks = [ones, part, dots, rand][:n] if n > 2 else [part, ones]
    frames = [frame(k, m) for k, m in enumerate(masks)]
    _, oi, ow, _ = _accum_inputs(299, W, H, W * s, H * s)
    hi0, hw0 = oi.copy(), ow.copy()
    for raw, m, sh in frames:
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    hi, hw_ = _accumulate_group_hip(hip, frames, kp, fw, fh, W, H, s, white, black, hi0, hw0, 0)
    np.testing.assert_allclose(hw_, ow, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(hi, oi, rtol=3e-5, atol=3e-5)

    # the two bodies on the same pixels
    lowered = ones.copy()
    cols = np.arange(20, mw, 64)
    lowered[:, cols] = 0.5
    fa = [frame(k, ones) for k in range(n)]
    fb = [frame(k, lowered) for k in range(n)]
    z = np.zeros_like(hi0)
    ai, aw = _accumulate_group_hip(hip, fa, kp, fw, fh, W, H, s, white, black, z.copy(), z.copy(), 1)
    bi, bw = _accumulate_group_hip(hip, fb, kp, fw, fh, W, H, s, white, black, z.copy(), z.copy(), 1)
    # HR column X reads mask cells (X + t) // (2 s), t = -2..2: keep the columns at least two cells from a lowered one
    cell = np.arange(W * s) // (2 * s)
    far = np.min(np.abs(cell[:, None] - cols[None, :]), axis=1) >= 2
    assert far.mean() > 0.8
    assert np.array_equal(ai[:, far], bi[:, far]) and np.array_equal(aw[:, far], bw[:, far])
    assert not np.array_equal(aw[:, ~far], bw[:, ~far])


@pytest.mark.parametrize("s,base", [(2, (70.3, -40.2)), (4, (70.3, -40.2)), (2, (-150.6, 33.0)), (4, (12.2, 90.7))])
def test_accumulate_large_global_shift(orc, hip, s, base):
    """Frames displaced by tens to hundreds of pixels as a whole (a hand-held burst before any stabilisation): the group
    kernels keep the rounded flow of a strip in 8 bits per pixel RELATIVE to the rounded flow of the tile's centre texel,
    so such frames stay on the fast path wherever their taps are inside the frame -- against the oracle, with one frame
    whose flow also varies by more than 127 HR pixels inside a tile (those strips take the straight arithmetic)."""
    W, H, n = 840, 328, 4
    orc.set_cfa(PATTERNS["RGGB"])
    hip.set_cfa(PATTERNS["RGGB"])
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = H // 2, W // 2
    kp = _kernel_field(370, fh, fw, 4)
    yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
    frames = []
    for k in range(n):
        raw, _, _, mask = _accum_inputs(371 + k, W, H, W * s, H * s)
        sh = np.stack([base[0] * (1 - 0.5 * k) + 0.01 * xx, base[1] * (1 - 0.5 * k) + 0.02 * yy], -1).astype(np.float32)
        if k == 1:
            sh[:, 200:230, 0] += 90.0      # a step of 90 LR pixels inside some tiles
        frames.append((raw, np.ascontiguousarray(mask), np.ascontiguousarray(sh)))
    _, oi, ow, _ = _accum_inputs(399, W, H, W * s, H * s)
    hi0, hw0 = oi.copy(), ow.copy()
    for raw, m, sh in frames:
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    hi, hw_ = _accumulate_group_hip(hip, frames, kp, fw, fh, W, H, s, white, black, hi0, hw0, 0)
    np.testing.assert_allclose(hw_, ow, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(hi, oi, rtol=3e-5, atol=3e-5)
    assert np.abs(hw_ - hw0).max() > 0.5


@pytest.mark.parametrize("s", [2, 4])
def test_accumulate_anisotropic_kernels(orc, hip, s):
    """Kernel parameters as ComputeKernelParam makes them at strong edges: inverse covariances with
    eigenvalues 0.7 .. 44 at every orientation (|kz| up to ~22), plus a patch of extreme ones
    (|kz| up to 150): tap weights spanning many orders of magnitude."""
    W, H = 192, 96
    orc.set_cfa(RGGB)
    hip.set_cfa(RGGB)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = H // 2, W // 2
    r = rng(140)
    th = r.uniform(0, np.pi, (fh, fw))
    l1 = r.uniform(0.7, 2.7, (fh, fw))
    l2 = 0.7 + 43.0 * r.uniform(0, 1, (fh, fw)) ** 2
    l2[5:9, 5:9] = 300.0             # |kz| up to 150
    c, sn = np.cos(th), np.sin(th)
    kp = np.zeros((fh, fw, 4), np.float32)
    kp[..., 0] = l1 * c * c + l2 * sn * sn
    kp[..., 1] = l1 * sn * sn + l2 * c * c
    kp[..., 2] = (l1 - l2) * c * sn
    yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
    sh = np.stack([0.8 + 0.01 * xx, -1.7 + 0.015 * yy], -1).astype(np.float32)

    def make():
        raw, imgOut, tw, mask = _accum_inputs(141, W, H, W * s, H * s, nan_frac=0.0)
        return raw, imgOut, tw, mask

    raw, oi, ow, m = make()
    orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    raw, hi, hw_, m = make()
    hip.call("accumulateSuperResFull", raw, hi, hw_, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(hi), pitch_of(m))
    np.testing.assert_allclose(hw_, ow, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(hi, oi, rtol=3e-5, atol=3e-5)


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("pat", ["RGGB", "GRBG", "MONO"])
def test_accumulate_x4_tile_kernel(orc, hip, pat, pair):
    """x4 tile kernel (fields at HR/8) against the oracle, one and two frames per call: smooth flows so
    that most strips take the fast path, a wild patch, a NaN flow texel, NaN certainties, hostile
    kernel parameters; odd tile counts (width not a multiple of 512 HR pixels)."""
    W, H, s = 168, 72, 4
    cfa = [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]
    orc.set_cfa(cfa)
    hip.set_cfa(cfa)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = H // 2, W // 2

    def make():
        raw0, imgOut, tw, mask0 = _accum_inputs(130, W, H, W * s, H * s, nan_frac=0.01)
        raw1, _, _, mask1 = _accum_inputs(131, W, H, W * s, H * s, nan_frac=0.01)
        kp = _kernel_field(132, fh, fw, 4)
        yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
        sh0 = np.stack([1.3 + 0.01 * xx, -2.2 + 0.02 * yy], -1).astype(np.float32)
        sh1 = np.stack([-2.6 - 0.015 * yy, 0.4 + 0.01 * xx], -1).astype(np.float32)
        sh0[10:14, 10:14] = 1e9
        sh1[20, 20] = np.nan
        return raw0, raw1, imgOut, tw, mask0, mask1, kp, sh0, sh1

    raw0, raw1, oi, ow, m0, m1, kp, sh0, sh1 = make()
    todo = ((raw0, m0, sh0), (raw1, m1, sh1)) if pair else ((raw0, m0, sh0),)
    for raw, m, sh in todo:
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    raw0, raw1, hi, hw_, m0, m1, kp, sh0, sh1 = make()
    if pair:
        hip.call("accumulateSuperResFull2", raw0, raw1, hi, hw_, m0, m1, Tex(kp), Tex(sh0), Tex(sh1), white, black, W, H, s,
                 pitch_of(hi), pitch_of(m0))
    else:
        hip.call("accumulateSuperResFull", raw0, hi, hw_, m0, Tex(kp), Tex(sh0), white, black, W, H, s, pitch_of(hi),
                 pitch_of(m0))
    np.testing.assert_allclose(hi, oi, rtol=3e-5, atol=3e-5)
    np.testing.assert_allclose(hw_, ow, rtol=3e-5, atol=3e-5)
    # the straight kernel on the same inputs: the tile kernel really ran (sums are re-associated)
    if not pair:
        hip.L.set_accumulate_fast_exp(1)
        raw0, raw1, si, sw, m0, m1, kp, sh0, sh1 = make()
        hip.call("accumulateSuperResFull", raw0, si, sw, m0, Tex(kp), Tex(sh0), white, black, W, H, s, pitch_of(si), pitch_of(m0))
        hip.L.set_accumulate_fast_exp(2)
        np.testing.assert_allclose(hi, si, rtol=1e-5, atol=1e-5)
        assert not np.array_equal(hi, si) or pat == "MONO"


@pytest.mark.parametrize("W,H,sigma", [(192, 96, 0.5), (152, 70, 1.2)])
def test_prepareFrameFused_equals_chain(orc, hip, W, H, sigma):
    """A1 + luma + separable prefilter + 2x2 mean in one launch == the four-kernel chain, bit for bit
    (ragged tiles, clamped borders, odd half-resolution sizes)."""
    orc.set_cfa(RGGB)
    hip.set_cfa(RGGB)
    raw = rng(150).integers(0, 4096, (H, W), dtype=np.uint16)
    hw, hh = W // 2, H // 2
    taps = np.zeros(99, np.float32)
    n = hip.L.raw["mfsr_gaussin_filter_1D"](sigma, taps.ctypes.data_as(ctypes.c_void_p))
    assert 3 <= n <= 17
    half = np.zeros((hh, hw, 3), np.float32)
    gray = np.zeros((hh, hw), np.float32)
    tmp = np.zeros_like(gray)
    p0 = np.zeros_like(gray)
    p1 = np.zeros((hh // 2, hw // 2), np.float32)
    hip.call("deBayersSubSample3", raw, half, 4095.0, hw, hh, pitch_of(half))
    hip.call("rgbToGray", half, pitch_of(half), gray, pitch_of(gray), hw, hh)
    hip.call("separableFilter", gray, pitch_of(gray), tmp, p0, pitch_of(p0), hw, hh, 1, Host(taps), n)
    hip.call("downsample2x", p0, pitch_of(p0), p1, pitch_of(p1), hw // 2, hh // 2)
    fh = np.zeros_like(half)
    f0 = np.zeros_like(p0)
    f1 = np.zeros_like(p1)
    hip.call("prepareFrameFused", raw, fh, pitch_of(fh), 4095.0, hw, hh, f0, pitch_of(f0), f1, pitch_of(f1), Host(taps), n)
    assert_bitexact(half, fh, "half-res RGB")
    assert_bitexact(p0, f0, "prefiltered luma")
    assert_bitexact(p1, f1, "pyramid level 1")


def test_accumulateImages_x1(orc, hip):
    W, H = 64, 40
    orc.set_cfa(RGGB)
    hip.set_cfa(RGGB)
    white, black = F3([3839, 3839, 3839]), F3([256, 256, 256])

    def make():
        raw, imgOut, tw, mask = _accum_inputs(9, W, H, W, H)
        kp = _kernel_field(10, H, W, 3)
        sh = rng(11).uniform(-3, 3, (H, W, 2)).astype(np.float32)
        args = (raw, imgOut, tw, mask, kp, sh, white, black, W, H, pitch_of(imgOut), pitch_of(mask), pitch_of(sh))
        return args, [imgOut, tw]

    (oi, ow), (hi, hw_) = run_both(orc, hip, "accumulateImages", make)
    np.testing.assert_allclose(hi, oi, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(hw_, ow, rtol=2e-6, atol=2e-6)


# ---------------------------------------------------------------- B: tile tracker
def _tiles(seed, tiles, T, S):
    L = T + 2 * S
    return rng(seed).random((tiles, L, L), dtype=np.float32)


def test_squaredSum(orc, hip):
    T, S, n = 16, 3, 13

    def make():
        t = _tiles(20, n, T, S)
        out = np.zeros(n, np.float32)
        return (t, out, S, T, n), [out]

    (o,), (h,) = run_both(orc, hip, "squaredSum", make)
    # wavefront reduction re-orders the 256-term sum: fp32 rounding only
    np.testing.assert_allclose(h, o, rtol=2e-6)


@pytest.mark.parametrize("which", ["boxFilterWithBorderX", "boxFilterWithBorderY"])
def test_boxFilterWithBorder(orc, hip, which):
    T, S, n = 16, 4, 7

    def make():
        t = _tiles(21, n, T, S)
        out = np.full_like(t, -1)
        return (t, out, S, T, n), [out]

    (o,), (h,) = run_both(orc, hip, which, make)
    assert_bitexact(o, h, which)


def test_normalizedCC_and_crossCorrelate(orc, hip):
    T, S, n = 16, 3, 5
    L, R = T + 2 * S, 2 * S + 1

    def make_cc():
        a, b = _tiles(22, n, T, S), _tiles(23, n, T, S)
        cc = np.full((n, L, L), -1, np.float32)
        return (a, b, cc, S, T, n), [cc]

    (occ,), (hcc,) = run_both(orc, hip, "crossCorrelateTiles", make_cc)
    assert_bitexact(occ, hcc, "crossCorrelateTiles")

    def make():
        cc = occ.copy()
        sq = rng(24).random(n, dtype=np.float32) * 50
        box = _tiles(25, n, T, S) * 50
        out = np.zeros((n, R, R), np.float32)
        return (cc, sq, box, out, S, T, n), [out]

    (o,), (h,) = run_both(orc, hip, "normalizedCC", make)
    assert_bitexact(o, h, "normalizedCC")


@pytest.mark.parametrize("rot", [0.0, 0.05])
def test_convertToTiles(orc, hip, rot):
    W, H, T, S = 100, 70, 16, 3
    tcx, tcy = W // T, H // T
    L = T + 2 * S
    img = rng(26).random((H, W + 5), dtype=np.float32)
    base = F2([1.3, -0.7] if rot else [0, 0])

    def make_b():
        out = np.full((tcx * tcy, L, L), -1, np.float32)
        return (img, out, W, H, pitch_of(img), S, T, tcx, tcy, base, rot), [out]

    (o,), (h,) = run_both(orc, hip, "convertToTilesOverlapBorder", make_b)
    if rot == 0.0:
        assert_bitexact(o, h, "convertToTilesOverlapBorder")
    else:  # sinf/cosf feed a roundf: identical unless a rounding tie is hit
        assert np.mean(o != h) < 0.01

    pre = rng(27).uniform(-4, 4, (tcy, tcx, 2)).astype(np.float32)

    def make_p():
        out = np.full((tcx * tcy, L, L), -1, np.float32)
        return (img, out, pre, pitch_of(pre), W, H, pitch_of(img), S, T, tcx, tcy, base, rot), [out]

    (o,), (h,) = run_both(orc, hip, "convertToTilesOverlapPreShift", make_p)
    if rot == 0.0:
        assert_bitexact(o, h, "convertToTilesOverlapPreShift")
    else:
        assert np.mean(o != h) < 0.01


def _paraboloid(S, cx, cy, n=1, seed=0):
    R = 2 * S + 1
    y, x = np.mgrid[0:R, 0:R].astype(np.float32)
    img = np.stack([(1.5 * (x - S - cx) ** 2 + 0.8 * (y - S - cy) ** 2 + 0.3 * (x - S - cx) * (y - S - cy) + 2.0)
                    for _ in range(n)]).astype(np.float32)
    return img


def test_findMinimum(orc, hip):
    S = 4
    R = 2 * S + 1
    tcx, tcy = 5, 3
    n = tcx * tcy
    r = rng(28)
    imgs = r.random((n, R, R), dtype=np.float32) * 10
    imgs[0] = _paraboloid(S, 1.3, -0.6)[0]          # analytic interior minimum
    imgs[1] = 1.0                                    # flat tile -> (0,0)
    imgs[2] = _paraboloid(S, 4.0, 0.0)[0]            # minimum on the border ring -> (0,0)
    imgs[3, 2, 2] = imgs[3, 5, 5] = -5.0             # tie: first strict minimum wins
    imgs[4] = np.nan                                 # all NaN

    def make():
        out = np.full((tcy, tcx + 1, 2), 7, np.float32)
        return (imgs.copy(), out, pitch_of(out), S, n, tcx, 0.5), [out]

    (o,), (h,) = run_both(orc, hip, "findMinimum", make)
    assert_bitexact(o, h, "findMinimum")
    np.testing.assert_allclose(o[0, 0], [1.3, -0.6], atol=0.05)  # the quadratic fit recovers the analytic minimum
    assert (o[0, 1] == 0).all() and (o[0, 2] == 0).all()


def test_UpSampleShifts(orc, hip):
    ocx, ocy, ncx, ncy = 7, 5, 15, 11
    inS = rng(29).uniform(-5, 5, (ocy, ocx, 2)).astype(np.float32)

    def make():
        out = np.zeros((ncy, ncx, 2), np.float32)
        return (inS, out, pitch_of(inS), pitch_of(out), 4, 2, ocx, ocy, ncx, ncy, 16, 16), [out]

    (o,), (h,) = run_both(orc, hip, "UpSampleShifts", make)
    assert_bitexact(o, h, "UpSampleShifts")


@pytest.mark.parametrize("oldL,newL,oldT,T,S", [(4, 2, 16, 16, 3), (2, 1, 16, 32, 4), (4, 1, 32, 32, 8)])
def test_trackTilesFusedUp_equals_UpSampleShifts_then_tracker(orc, hip, oldL, newL, oldT, T, S):
    """B8 folded into the tracker: same bits as oracle UpSampleShifts (kernel.cu:642) followed by the fused tracker."""
    W, H = 224, 160  # 7 x 5 tiles of 32: the last workgroup of the compile-time kernel (2 tiles each) is half empty
    tcx, tcy = W // T, H // T
    ocx, ocy = (W * newL // oldL) // oldT, (H * newL // oldL) // oldT
    r = rng(77)
    base = r.random((H + 16, W + 16), dtype=np.float32)
    ref = np.ascontiguousarray(base[8:8 + H, 8:8 + W])
    mov = np.ascontiguousarray(base[7:7 + H, 10:10 + W])
    coarse = r.uniform(-2.5, 2.5, (ocy, ocx, 2)).astype(np.float32)
    pre = np.zeros((tcy, tcx, 2), np.float32)
    orc.call("UpSampleShifts", coarse, pre, pitch_of(coarse), pitch_of(pre), oldL, newL, ocx, ocy, tcx, tcy, oldT, T)
    want = np.zeros((tcy, tcx, 2), np.float32)
    hip.call("trackTilesFused", ref, mov, pre, pitch_of(pre), want, pitch_of(want), W, H, pitch_of(ref), S, T, tcx, tcy, 0.0, None)
    got = np.zeros((tcy, tcx, 2), np.float32)
    hip.call("trackTilesFusedUp", ref, mov, coarse, pitch_of(coarse), oldL, newL, ocx, ocy, oldT, got, pitch_of(got), W, H,
             pitch_of(ref), S, T, tcx, tcy, 0.0, None, None, 1.0)
    assert_bitexact(want, got, "trackTilesFusedUp")
    assert np.abs(want).max() > 0
    # with sum(ref^2) handed in (what the pipeline does) these tile sizes run the compile-time kernel: same bits,
    # also with a base shift (global pre-alignment without rotation: cos = 1, sin = 0 exactly)
    sq = np.zeros(tcx * tcy, np.float32)
    hip.call("tileSquaredSums", ref, sq, W, H, pitch_of(ref), S, T, tcx, tcy)
    got2 = np.zeros((tcy, tcx, 2), np.float32)
    hip.call("trackTilesFusedUp", ref, mov, coarse, pitch_of(coarse), oldL, newL, ocx, ocy, oldT, got2, pitch_of(got2), W, H,
             pitch_of(ref), S, T, tcx, tcy, 0.0, sq, None, 1.0)
    assert_bitexact(want, got2, "trackTilesFusedUp(refSquaredSums)")


@pytest.mark.parametrize("T,S", [(16, 3), (32, 4), (32, 8)])
def test_trackTilesFused_equals_chain(orc, hip, T, S):
    """Fused tracker == oracle chain B1,B2,cc,B3,B4x,B4y,B6,B7 + rounded pre-shift add, bit for bit."""
    W, H = 160, 96
    tcx, tcy = W // T, H // T
    n, L, R = tcx * tcy, T + 2 * S, 2 * S + 1
    r = rng(30)
    base = r.random((H + 16, W + 16), dtype=np.float32)
    ref = np.ascontiguousarray(base[8:8 + H, 8:8 + W])
    mov = np.ascontiguousarray(base[6:6 + H, 9:9 + W])  # moved(p + (-1,+2)) == ref(p)
    pre = r.uniform(-1.4, 1.4, (tcy, tcx, 2)).astype(np.float32)
    coord, _, sq, _ = oracle_track(orc, ref, mov, W, H, T, S, pre=pre, coord_pad=0)
    got = np.zeros((tcy, tcx, 2), np.float32)
    hip.call("trackTilesFused", ref, mov, pre, pitch_of(pre), got, pitch_of(got), W, H, pitch_of(ref), S, T, tcx, tcy, 0.0, None)
    assert_bitexact(coord, got, "trackTilesFused")
    # sum(ref^2) taken once per reference (tileSquaredSums) and handed in: same bits as squaredSum (B3)
    sq2 = np.zeros(n, np.float32)
    hip.call("tileSquaredSums", ref, sq2, W, H, pitch_of(ref), S, T, tcx, tcy)
    assert_bitexact(sq, sq2, "tileSquaredSums")
    got2 = np.zeros((tcy, tcx, 2), np.float32)
    hip.call("trackTilesFused", ref, mov, pre, pitch_of(pre), got2, pitch_of(got2), W, H, pitch_of(ref), S, T, tcx, tcy, 0.0, sq2)
    assert_bitexact(coord, got2, "trackTilesFused(refSquaredSums)")
    # global pre-alignment without rotation (B2's baseShift, kernel.cu:358-368; cos = 1 and sin = 0 exactly), read by the
    # kernel from a device mfsr_prealign: same bits as the oracle chain with that base shift -- both kernels
    coordB = oracle_track(orc, ref, mov, W, H, T, S, pre=pre, base=(3.0, -2.0, 0.0, 1.0), coord_pad=0)[0]
    assert not np.array_equal(coordB, coord)
    pa = np.zeros(12, np.float32)  # mfsr_prealign: shiftX, shiftY, rotation, cos, sin, 7 x int32
    pa[:5] = [3.0, -2.0, 0.0, 1.0, 0.0]
    for sqv, what in ((None, "generic"), (sq2, "compile-time")):
        gotB = np.zeros((tcy, tcx, 2), np.float32)
        hip.call("trackTilesFusedBase", ref, mov, pre, pitch_of(pre), gotB, pitch_of(gotB), W, H, pitch_of(ref), S, T, tcx, tcy,
                 0.0, sqv, pa, 1.0)
        assert_bitexact(coordB, gotB, f"trackTilesFusedBase({what})")
    # interior tiles whose residual (truth - round(pre)) lies strictly inside the search range
    # recover the true shift (-1, +2); on the border ring findMinimum returns 0 (kernel.cu:548-553)
    res = np.array([-1.0, 2.0]) - np.round(pre)
    ok = (np.abs(res) <= S - 1).all(-1)
    ok[0] = ok[-1] = False
    ok[:, 0] = ok[:, -1] = False
    assert ok.sum() >= 2
    np.testing.assert_allclose(got[ok], np.tile([-1.0, 2.0], (int(ok.sum()), 1)), atol=0.06)


# ---------------------------------------------------------------- C: shift minimiser
def _design(n_img, pairs):
    n1, m = n_img - 1, len(pairs)
    A = np.zeros((n1, m), np.float32)  # column-major m x n1  ==  C array [n1][m]
    for r, (a, b) in enumerate(pairs):
        A[a:b, r] = 1.0
    return A


def test_solve_and_checkForOutliers(orc, hip):
    n_img, tiles = 6, 37
    pairs = [(a, b) for a in range(n_img) for b in range(a + 1, n_img)]
    n1, m = n_img - 1, len(pairs)
    r = rng(40)
    d_true = r.uniform(-3, 3, (tiles, n1, 2)).astype(np.float32)
    A1 = _design(n_img, pairs)
    meas = np.zeros((tiles, m, 2), np.float32)
    for k, (a, b) in enumerate(pairs):
        meas[:, k] = d_true[:, a:b].sum(1)
    meas += r.normal(0, 0.02, meas.shape).astype(np.float32)
    meas[3, 4] += 5.0   # outlier
    meas[7, 0] -= 9.0
    res = []
    for k in (orc, hip):
        A = np.tile(A1[None], (tiles, 1, 1)).copy()
        ms = meas.copy()
        one = np.zeros((tiles, n1, 2), np.float32)
        opt = np.zeros((tiles, 2, m), np.float32)
        info = np.zeros(tiles, np.int32)
        status = np.zeros(tiles, np.int32)
        rounds = 0
        while True:
            k.call("solveShiftsBatched", A, ms, one, opt, info, tiles, n_img, m)
            k.call("checkForOutliers", ms, opt, A, status, info, tiles, n_img, m)
            rounds += 1
            if (status < 0).all() or rounds > m:
                break
        res.append((A, ms, one, opt, info, status, rounds))
    for i, nm in enumerate(["shiftMatrix", "measured", "oneToOne", "optimT", "info", "status"]):
        assert_bitexact(res[0][i], res[1][i], nm)
    assert res[0][6] == res[1][6] >= 2
    A, ms, one = res[1][0], res[1][1], res[1][2]
    assert (ms[3, 4] == 0).all() and (A[3, :, 4] == 0).all()      # the outlier row was dropped
    np.testing.assert_allclose(one, d_true, atol=0.1)


def test_solve_singular_reports_info(orc, hip):
    n_img, tiles = 4, 3
    pairs = [(0, 1), (0, 1), (2, 3)]   # image 1->2 never measured: singular normal matrix
    m = len(pairs)
    A1 = _design(n_img, pairs)

    def make():
        A = np.tile(A1[None], (tiles, 1, 1)).copy()
        ms = rng(41).random((tiles, m, 2), dtype=np.float32)
        one = np.ones((tiles, n_img - 1, 2), np.float32)
        opt = np.ones((tiles, 2, m), np.float32)
        info = np.zeros(tiles, np.int32)
        return (A, ms, one, opt, info, tiles, n_img, m), [one, opt, info]

    (o1, o2, o3), (h1, h2, h3) = run_both(orc, hip, "solveShiftsBatched", make)
    assert (o3 != 0).all()
    assert_bitexact(o3, h3)
    assert_bitexact(o1, h1)
    assert_bitexact(o2, h2)


def test_minimizeShifts_driver(orc, hip):
    """The C-ABI loop == the same loop written around the oracle."""
    import torch
    n_img, tiles = 5, 11
    pairs = [(a, b) for a in range(n_img) for b in range(a + 1, n_img)]
    n1, m = n_img - 1, len(pairs)
    r = rng(42)
    meas = r.uniform(-2, 2, (tiles, m, 2)).astype(np.float32)
    meas[2, 1] += 7
    A0 = np.tile(_design(n_img, pairs)[None], (tiles, 1, 1)).copy()
    A, ms = A0.copy(), meas.copy()
    one = np.zeros((tiles, n1, 2), np.float32)
    opt = np.zeros((tiles, 2, m), np.float32)
    info = np.zeros(tiles, np.int32)
    status = np.zeros(tiles, np.int32)
    rounds = 0
    while True:
        orc.call("solveShiftsBatched", A, ms, one, opt, info, tiles, n_img, m)
        orc.call("checkForOutliers", ms, opt, A, status, info, tiles, n_img, m)
        rounds += 1
        if (status < 0).all():
            break
    dev = "cuda:0"
    checks = []

    def gup(a):
        t, c = guarded_upload(a, dev)
        checks.append(c)
        return t

    tA, tms = gup(A0), gup(meas)
    tone, topt = gup(np.zeros_like(one)), gup(np.zeros((tiles, 2, m), np.float32))
    tinfo = gup(np.zeros(tiles, np.int32))
    tstat = gup(np.zeros(tiles, np.int32))
    import ctypes
    nr = ctypes.c_int(0)
    hip.L.minimizeShifts(tA.data_ptr(), tms.data_ptr(), tone.data_ptr(), topt.data_ptr(), tstat.data_ptr(),
                         tinfo.data_ptr(), tiles, n_img, m, ctypes.addressof(nr), None)
    assert nr.value == rounds
    assert_bitexact(one, tone.cpu().numpy(), "minimizeShifts oneToOne")
    assert (tstat.cpu().numpy() == -1).all()
    # the same loop inside one launch, no host round trips (what the burst pipeline's joint mode uses)
    fA, fms = gup(A0), gup(meas)
    fone, fopt = gup(np.zeros_like(one)), gup(np.zeros((tiles, 2, m), np.float32))
    finfo, fstat = gup(np.full(tiles, 5, np.int32)), gup(np.full(tiles, 5, np.int32))
    hip.L.minimizeShiftsFused(fA.data_ptr(), fms.data_ptr(), fone.data_ptr(), fopt.data_ptr(), fstat.data_ptr(), finfo.data_ptr(),
                              tiles, n_img, m, None)
    torch.cuda.synchronize()
    assert_bitexact(one, fone.cpu().numpy(), "minimizeShiftsFused oneToOne")
    assert_bitexact(opt, fopt.cpu().numpy(), "minimizeShiftsFused optimShiftsT")
    assert_bitexact(A, fA.cpu().numpy(), "minimizeShiftsFused shiftMatrix")
    assert_bitexact(ms, fms.cpu().numpy(), "minimizeShiftsFused measuredShifts")
    assert (fstat.cpu().numpy() == -1).all() and (finfo.cpu().numpy() == info).all()
    for i, c in enumerate(checks):
        c(f"mfsr_minimizeShifts / mfsr_minimizeShiftsFused, buffer {i}")


def test_shift_glue_kernels(orc, hip):
    n_img, tcx, tcy = 5, 6, 4
    n1 = n_img - 1
    tiles = tcx * tcy
    best = rng(43).uniform(-3, 3, (tiles, n1, 2)).astype(np.float32)
    for ref, trk in [(0, 3), (4, 1), (2, 2)]:
        def make():
            out = np.zeros((tcy, tcx + 2, 2), np.float32)
            return (out, best, n_img, tcx, tcy, pitch_of(out), ref, trk), [out]
        (o,), (h,) = run_both(orc, hip, "getOptimalShifts", make)
        assert_bitexact(o, h, "getOptimalShifts")
    m = 7
    mT = rng(44).random((tiles, 2, m), dtype=np.float32)
    oT = rng(45).random((tiles, 2, n1), dtype=np.float32)

    def make_t():
        ms = np.zeros((tiles, m, 2), np.float32)
        one = np.zeros((tiles, n1, 2), np.float32)
        return (ms, mT, oT, one, tiles, n_img, m), [ms, one]
    (o1, o2), (h1, h2) = run_both(orc, hip, "transposeShifts", make_t)
    assert_bitexact(o1, h1)
    assert_bitexact(o2, h2)
    np.testing.assert_array_equal(o1[..., 0], mT[:, 0])

    def make_c():
        mats = rng(46).random((tiles, n1, m), dtype=np.float32)
        return (mats, tiles, n_img, m), [mats]
    (o,), (h,) = run_both(orc, hip, "copyShiftMatrix", make_c)
    assert_bitexact(o, h)
    assert (h == h[0]).all()


def test_concatenate_separate_setPointers(hip):
    """Pointer-array ABI (ShiftMinimizerKernels.cu:51-55,224,244) on device pointers."""
    import torch
    dev = "cuda:0"
    m, tcx, tcy = 3, 5, 4
    checks = []

    def gup(a, readonly=False):
        t, c = guarded_upload(a, dev)
        checks.append((c, readonly))
        return t

    imgs = [gup(rng(47 + i).random((tcy, tcx + i, 2), dtype=np.float32), True) for i in range(m)]
    ptrs = gup(np.array([t.data_ptr() for t in imgs], np.int64), True)
    pitches = gup(np.array([t.stride(0) * 4 for t in imgs], np.int32), True)
    out = gup(np.zeros((tcy * tcx, m, 2), np.float32))
    hip.L.concatenateShifts(ptrs.data_ptr(), pitches.data_ptr(), out.data_ptr(), m, tcx, tcy, None)
    torch.cuda.synchronize()
    for k in range(m):
        assert torch.equal(out[:, k].reshape(tcy, tcx, 2), imgs[k][:, :tcx])
    back = [gup(np.zeros(tuple(t.shape), np.float32)) for t in imgs]
    bptrs = gup(np.array([t.data_ptr() for t in back], np.int64), True)
    hip.L.separateShifts(out.data_ptr(), bptrs.data_ptr(), pitches.data_ptr(), m, tcx, tcy, None)
    torch.cuda.synchronize()
    for k in range(m):
        assert torch.equal(back[k][:, :tcx], imgs[k][:, :tcx])
        assert (back[k][:, tcx:] == 0).all()          # the columns past tileCountX of a wider image are not written
    for i, (c, ro) in enumerate(checks):
        c(f"mfsr_concatenateShifts / mfsr_separateShifts, buffer {i}", unchanged=ro)
    # setPointers: per-tile base addresses
    tiles, n_img, mm = 9, 4, 5
    n1 = n_img - 1
    arrs = [torch.zeros(tiles, dtype=torch.int64, device=dev) for _ in range(8)]
    bases = [torch.zeros(tiles * n1 * mm, device=dev), torch.zeros(tiles * n1 * mm, device=dev),
             torch.zeros(tiles * n1 * n1, device=dev), torch.zeros(tiles * n1 * n1, device=dev),
             torch.zeros(tiles * n1 * mm, device=dev), torch.zeros(tiles * n1 * 2, device=dev),
             torch.zeros(tiles * mm * 2, device=dev), torch.zeros(tiles * mm * 2, device=dev)]
    hip.L.setPointers(*[a.data_ptr() for a in arrs], *[b.data_ptr() for b in bases], tiles, n_img, mm, None)
    torch.cuda.synchronize()
    strides = [n1 * mm * 4, n1 * mm * 4, n1 * n1 * 4, n1 * n1 * 4, n1 * mm * 4, n1 * 8, mm * 8, mm * 8]
    # array order: matrix, safe, square, inverted, solved, oneToOne, MEASURED, OPTIM (:51-53);
    # base order: ..., shiftsOneToOne, shiftsMeasured, shiftsOptim (:54-55)
    for a, b, s in zip(arrs, bases, strides):
        want = b.data_ptr() + torch.arange(tiles, dtype=torch.int64) * s
        assert torch.equal(a.cpu(), want)


# ---------------------------------------------------------------- D/E: optical flow
def _smooth_image(seed, H, W):
    r = rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = 0.5 + 0.2 * np.sin(x * 0.21 + 0.3 * y * 0.1) + 0.2 * np.cos(y * 0.17) + 0.05 * r.random((H, W), dtype=np.float32)
    return img.astype(np.float32)


def test_WarpingKernel(orc, hip):
    H, W = 50, 70
    img = _smooth_image(50, H, W)
    uv = rng(51).uniform(-6, 6, (H, W, 2)).astype(np.float32)
    uv[0, 0] = [-30, 200]  # far outside: mirror addressing

    def make():
        out = np.zeros((H, W + 1), np.float32)
        return (W, H, pitch_of(out), Tex(uv), out, Tex(img)), [out]

    (o,), (h,) = run_both(orc, hip, "WarpingKernel", make)
    assert_bitexact(o, h, "WarpingKernel")


@pytest.mark.parametrize("rot", [0.0, 0.02])
def test_CreateFlowFieldFromTiles(orc, hip, rot):
    H, W, tcx, tcy = 48, 80, 5, 3
    ts = rng(52).uniform(-3, 3, (tcy, tcx, 2)).astype(np.float32)

    def make():
        out = np.zeros((H, W, 2), np.float32)
        return (out, Tex(ts), 16, tcx, tcy, W, H, pitch_of(out), F2([0.5, -1.5] if rot else [0, 0]), rot), [out]

    (o,), (h,) = run_both(orc, hip, "CreateFlowFieldFromTiles", make)
    if rot == 0.0:
        assert_bitexact(o, h, "CreateFlowFieldFromTiles")
    else:  # sinf/cosf: ocml vs glibc, <= 2 ulp on O(50 px) lever arms
        np.testing.assert_allclose(h, o, atol=2e-5)


def test_ComputeDerivatives(orc, hip):
    H, W = 40, 56
    a, b = _smooth_image(53, H, W), _smooth_image(54, H, W)

    def make():
        Ix, Iy, Iz = (np.zeros((H, W), np.float32) for _ in range(3))
        return (W, H, pitch_of(Ix), Ix, Iy, Iz, Tex(a), Tex(b)), [Ix, Iy, Iz]

    o, h = run_both(orc, hip, "ComputeDerivativesKernel", make)
    for x, y in zip(o, h):
        assert_bitexact(x, y, "ComputeDerivativesKernel")

    def make2():
        Ix, Iy = (np.zeros((H, W), np.float32) for _ in range(2))
        return (W, H, pitch_of(Ix), Ix, Iy, Tex(a)), [Ix, Iy]

    o, h = run_both(orc, hip, "ComputeDerivatives2Kernel", make2)
    for x, y in zip(o, h):
        assert_bitexact(x, y, "ComputeDerivatives2Kernel")


@pytest.mark.parametrize("hw", [1, 3])
def test_lucasKanadeOptim(orc, hip, hw):
    H, W = 36, 52
    r = rng(55)
    fx = (r.random((H, W), dtype=np.float32) - 0.5) * 0.4
    fy = (r.random((H, W), dtype=np.float32) - 0.5) * 0.4
    ft = (r.random((H, W), dtype=np.float32) - 0.5) * 0.1
    fx[10:14, 10:14] = 0
    fy[10:14, 10:14] = 0       # singular windows -> rejected / zero pseudo-inverse
    sh0 = r.uniform(-1, 1, (H, W, 2)).astype(np.float32)

    def make():
        sh = sh0.copy()
        return (sh, fx, fy, ft, pitch_of(sh), pitch_of(fx), W, H, hw, 1e-3), [sh]

    (o,), (h,) = run_both(orc, hip, "lucasKanadeOptim", make)
    # atan2f/cosf/sinf differ by <= 2 ulp between ocml and glibc; the update is O(1) px
    np.testing.assert_allclose(h, o, atol=5e-5, rtol=1e-4)
    assert_bitexact(o[:hw], sh0[:hw])   # border ring untouched


@pytest.mark.parametrize("hw", [3, 0, 1, 2, 6, 7, 8])
def test_lucasKanadeIterationFused_equals_chain(orc, hip, hw):
    """Fused D2+D3+D4 == oracle chain Warping -> ComputeDerivatives(source=warped, target=ref) -> lucasKanadeOptim,
    for every dispatch arm of the host (half windows 1..7 have <h,48> and <h,32> kernels, all others the generic
    <0,32> one; W=100 is wide enough for the 48-wide tiles)."""
    H, W = 70, 100
    base = _smooth_image(56, H + 8, W + 8)
    ref = np.ascontiguousarray(base[4:4 + H, 4:4 + W])
    mov = np.ascontiguousarray(base[3:3 + H, 6:6 + W])
    flow0 = np.zeros((H, W, 2), np.float32)
    flow0[..., 0] = -1.6
    flow0[..., 1] = 0.7
    flow = flow0.copy()
    warped = np.zeros((H, W), np.float32)
    Ix, Iy, Iz = (np.zeros((H, W), np.float32) for _ in range(3))
    orc.call("WarpingKernel", W, H, pitch_of(warped), Tex(flow), warped, Tex(mov))
    orc.call("ComputeDerivativesKernel", W, H, pitch_of(Ix), Ix, Iy, Iz, Tex(warped), Tex(ref))  # source = warped
    orc.call("lucasKanadeOptim", flow, Ix, Iy, Iz, pitch_of(flow), pitch_of(Ix), W, H, hw, 1e-4)
    out = np.full((H, W, 2), 99, np.float32)
    hip.call("lucasKanadeIterationFused", flow0, out, pitch_of(out), ref, mov, pitch_of(ref), W, H, hw, 1e-4, 1.0)
    # outScale folds the pipeline's mfsr_scaleFlow pass into the last iteration: same bits
    out2 = np.full((H, W, 2), 99, np.float32)
    hip.call("lucasKanadeIterationFused", flow0, out2, pitch_of(out2), ref, mov, pitch_of(ref), W, H, hw, 1e-4, 2.0)
    scaled = out.copy()
    hip.call("scaleFlow", scaled, pitch_of(scaled), W, H, 2.0)
    assert_bitexact(scaled, out2, "lucasKanadeIterationFused(outScale)")
    # separable window sums + M^-1 * sum(grad*It) instead of sum(M^-1 grad * It): rounding only
    if hw >= 2:
        np.testing.assert_allclose(out, flow, atol=1e-4)
    elif hw == 1:
        # 3x3 windows are often nearly singular: the pseudo-inverse amplifies the rounding of the sums
        assert np.mean(np.abs(out - flow) > 1e-3) < 2e-2
    else:
        # 1x1 window: the normal matrix has rank 1, sigma2 = sqrt((S1 - S2)/2) is 0, NaN or 1e-4 by rounding alone
        # (opticalFlow.cu:251-259), in the reference as much as here: only the launch geometry is checked
        assert out.shape == flow.shape and not np.any(out == 99)
    assert_bitexact(out[:hw], flow0[:hw], "ring rows")   # the h-px ring keeps the input flow
    assert np.abs(flow - flow0).max() > 0.05   # the iteration did move the flow
    if hw >= 2:
        # true shift is (-2, +1): one iteration gets closer
        err0 = np.abs(flow0[10:-10, 10:-10] - [-2, 1]).mean()
        err1 = np.abs(out[10:-10, 10:-10] - [-2, 1]).mean()
        assert err1 < err0


@pytest.mark.parametrize("hw,W,H", [(3, 100, 70), (3, 333, 141), (2, 64, 40), (5, 130, 90)])
def test_lucasKanadeIterationWarped_is_bit_identical(hip, hw, W, H):
    """mfsr_CreateFlowFieldWarped + three mfsr_lucasKanadeIterationWarped (the warped image handed from launch to launch,
    every pixel warped once per iteration) == mfsr_CreateFlowFieldFromTiles + three mfsr_lucasKanadeIterationFused (tile +
    halo re-warped by every workgroup): same flow, bit for bit, ragged tiles and mirrored halos included; also with the
    base shift / rotation read from a device mfsr_prealign."""
    r = rng(333)
    base = _smooth_image(58, H + 8, W + 8)
    ref = np.ascontiguousarray(base[4:4 + H, 4:4 + W])
    mov = np.ascontiguousarray(base[3:3 + H, 6:6 + W])
    tcx, tcy = 5, 4
    tiles = r.uniform(-2.5, 2.5, (tcy, tcx, 2)).astype(np.float32)
    z = F2([0, 0])
    for use_base in (False, True):
        pa = np.zeros(12, np.float32)   # mfsr_prealign: shiftX, shiftY, rotation, cos, sin, 7 x int32
        ang = np.float32(0.02)
        pa[:5] = [1.5, -0.75, ang, np.cos(ang, dtype=np.float32), np.sin(ang, dtype=np.float32)]
        flows = [np.zeros((H, W, 2), np.float32) for _ in range(2)]
        if use_base:
            hip.call("CreateFlowFieldFromTilesBase", flows[0], Tex(tiles), W, H, pitch_of(flows[0]), pa)
        else:
            hip.call("CreateFlowFieldFromTiles", flows[0], Tex(tiles), 16, tcx, tcy, W, H, pitch_of(flows[0]), z, 0.0)
        for it in range(3):
            hip.call("lucasKanadeIterationFused", flows[it & 1], flows[(it & 1) ^ 1], pitch_of(flows[0]), ref, mov, pitch_of(ref),
                     W, H, hw, 1e-4, 2.0 if it == 2 else 1.0)
        want = flows[1]
        f = [np.zeros((H, W, 2), np.float32) for _ in range(2)]
        S = [np.full((H, W), np.nan, np.float32) for _ in range(2)]
        D = [np.full((H, W), np.nan, np.float32) for _ in range(2)]
        hip.call("CreateFlowFieldWarped", f[0], Tex(tiles), W, H, pitch_of(f[0]), z, 0.0, pa if use_base else None, ref, mov,
                 pitch_of(ref), S[0], D[0], pitch_of(S[0]))
        for it in range(3):
            i, o = it & 1, (it & 1) ^ 1
            last = it == 2
            hip.call("lucasKanadeIterationWarped", f[i], f[o], pitch_of(f[0]), ref, mov, pitch_of(ref), S[i], D[i],
                     None if last else S[o], None if last else D[o], pitch_of(S[0]), W, H, hw, 1e-4, 2.0 if last else 1.0)
        assert_bitexact(want, f[1], f"warped LK chain (base={use_base})")
        assert np.abs(want).max() > 0.5


@pytest.mark.parametrize("hw,W,H,nf", [(3, 100, 70, 1), (3, 333, 141, 4), (2, 130, 90, 1), (2, 200, 77, 4), (5, 130, 90, 4), (5, 257, 131, 1),
                                       (3, 640, 360, 4)])
def test_lucasKanadeSweepBatch_vs_oracle_chain(orc, hw, W, H, nf):
    """The kernel that carries Lucas-Kanade in every pipeline (k_lkSweep behind mfsr_lucasKanadeSweepBatch, fed by
    mfsr_CreateFlowFieldWarped) DIRECTLY against the oracle's restatement of opticalFlow.cu:28-325: three chained iterations
    of WarpingKernel -> ComputeDerivativesKernel(source = warped, target = reference) -> lucasKanadeOptim on the flow field
    CreateFlowFieldFromTiles makes, final flow x outScale.  The two differ by libm (atan2f / cosf / sinf / sqrtf: ocml vs
    glibc) and by the order of the window sums, amplified by 1 / sigma2 of the window's normal matrix: asserted <= 5e-4 px over
    the well-conditioned, converged interior windows (tests/burst_compare.flow_difference_report; the measured maximum there
    is ~1e-5), i.e. every larger difference sits in a low-sigma2 window, a border row or an unconverged flow.  Ragged strips
    (W not a multiple of 54 lanes) and bands, h = 2, 3, 5, one and four frames per launch."""
    import torch
    from multi_frame_super_resolution_amd import capi
    from tests.burst_compare import flow_difference_report
    dev = torch.device("cuda:0")
    r = rng(777 + W + hw)
    base = _smooth_image(63, H + 16, W + 16)
    ref_np = np.ascontiguousarray(base[8:8 + H, 8:8 + W])
    ref = torch.from_numpy(ref_np).to(dev)
    tcx, tcy = 5, 4
    L = capi.lib()
    shifts = [(10, 7), (6, 9), (11, 8), (7, 6)]
    movs_np, tiles_np = [], []
    for k in range(nf):
        dx, dy = shifts[k]
        movs_np.append(np.ascontiguousarray(base[dy:dy + H, dx:dx + W]))
        true = np.array([8 - dx, 8 - dy], np.float32)        # ref(p) = moved(p + u): u = -(offset of the moved crop)
        tiles_np.append((true + r.uniform(-0.4, 0.4, (tcy, tcx, 2))).astype(np.float32))
    # oracle: the reference's kernels one at a time
    want = []
    for k in range(nf):
        flow = np.zeros((H, W, 2), np.float32)
        orc.call("CreateFlowFieldFromTiles", flow, Tex(tiles_np[k]), 16, tcx, tcy, W, H, pitch_of(flow), F2([0, 0]), 0.0)
        for it in range(3):
            warped = np.zeros((H, W), np.float32)
            Ix, Iy, Iz = (np.zeros((H, W), np.float32) for _ in range(3))
            orc.call("WarpingKernel", W, H, pitch_of(warped), Tex(flow), warped, Tex(movs_np[k]))
            orc.call("ComputeDerivativesKernel", W, H, pitch_of(Ix), Ix, Iy, Iz, Tex(warped), Tex(ref_np))
            orc.call("lucasKanadeOptim", flow, Ix, Iy, Iz, pitch_of(flow), pitch_of(Ix), W, H, hw, 1e-4)
        want.append(flow * np.float32(2.0))        # outScale of the last iteration (exact)
    # HIP: flow field + first warp, then the sweep kernel, all frames per launch
    movs = [torch.from_numpy(m).to(dev) for m in movs_np]
    tiles = [torch.from_numpy(t).to(dev) for t in tiles_np]
    f = [[torch.zeros(H, W, 2, device=dev) for _ in range(2)] for _ in range(nf)]
    S = [[torch.full((H, W), float("nan"), device=dev) for _ in range(2)] for _ in range(nf)]
    D = [[torch.full((H, W), float("nan"), device=dev) for _ in range(2)] for _ in range(nf)]
    for k in range(nf):
        L.CreateFlowFieldWarped(f[k][0].data_ptr(), capi.tex(tiles[k]), W, H, W * 8, capi.f2([0, 0]), 0.0, None, ref.data_ptr(),
                                movs[k].data_ptr(), W * 4, S[k][0].data_ptr(), D[k][0].data_ptr(), W * 4, None)
    for it in range(3):
        i, o = it & 1, (it & 1) ^ 1
        last = it == 2
        arr = (capi.LkFrame * nf)()
        for k in range(nf):
            arr[k] = capi.LkFrame(f[k][i].data_ptr(), f[k][o].data_ptr(), movs[k].data_ptr(), S[k][i].data_ptr(), D[k][i].data_ptr(),
                                  None if last else S[k][o].data_ptr(), None if last else D[k][o].data_ptr())
        L.lucasKanadeSweepBatch(nf, arr, ref.data_ptr(), W * 8, W * 4, W * 4, W, H, hw, 1e-4, 2.0 if last else 1.0, None)
    torch.cuda.synchronize()
    for k in range(nf):
        got = f[k][1].cpu().numpy()
        assert np.isfinite(got).all()
        rep = flow_difference_report(got / 2.0, want[k] / 2.0, ref_np, hw, thr=5e-4)
        d = np.abs(got - want[k]) / 2.0
        true = np.array([8 - shifts[k][0], 8 - shifts[k][1]], np.float32)
        err = np.abs(got[12:-12, 12:-12] / 2.0 - true).mean()
        print(f"h={hw} {W}x{H} frame {k}/{nf}: |flow(k_lkSweep) - flow(oracle chain)| well-conditioned windows ({rep['well_fraction']:.0%}) max "
              f"{rep['max_well']:.2e} px, rest max {rep['max_rest']:.2e} px, median {np.median(d):.1e}, > 5e-4: {rep['n_big']} "
              f"({rep['big_in_rest_fraction']:.0%} of them in the rest); mean distance to the true shift {err:.3f} px")
        assert rep["well_fraction"] >= 0.3                     # the classification is not vacuous
        assert rep["max_well"] <= 5e-4                         # ... and every larger difference is in the rest
        assert np.median(d) <= 2e-5
        assert err < 0.25                                      # both converged on the translation
        # the h-px ring keeps the input flow (x outScale on the last iteration is applied to it as well in both)
        np.testing.assert_allclose(got[:hw], want[k][:hw], rtol=0, atol=1e-6)


@pytest.mark.parametrize("hw,W,H,nf", [(3, 100, 70, 1), (3, 333, 141, 3), (2, 64, 40, 2), (5, 130, 90, 4), (3, 1920, 1080, 4), (3, 1920, 1080, 1)])
def test_lucasKanadeSweepBatch_matches_the_tile_kernel(hip, hw, W, H, nf):
    """mfsr_lucasKanadeSweepBatch (k_lkSweep: register / DPP column sweep, several frames per launch) against
    mfsr_lucasKanadeIterationWarped frame by frame, three chained iterations: same products, same column order, same solve
    and warp code; only the row sums add in another order, so the flows agree to fp32 rounding -- asserted <= 2e-5 px at the
    window sizes the pipeline uses (the 3x3-window amplification of `lucasKanadeIterationFused` vs the chain applies to
    hw < 3 here as well).  Ragged strips and bands, mirrored halos, the h-px ring, outScale on the last iteration."""
    import torch
    from multi_frame_super_resolution_amd import capi
    dev = torch.device("cuda:0")
    r = rng(4242 + W)
    base = _smooth_image(61, H + 16, W + 16)
    ref = torch.from_numpy(np.ascontiguousarray(base[8:8 + H, 8:8 + W])).to(dev)
    tcx, tcy = 5, 4
    L = capi.lib()
    st = None
    movs, want, got = [], [], []
    for k in range(nf):
        dy, dx = [(7, 10), (9, 6), (8, 11), (6, 7)][k]
        mov = torch.from_numpy(np.ascontiguousarray(base[dy:dy + H, dx:dx + W])).to(dev)
        tiles = torch.from_numpy(r.uniform(-2.5, 2.5, (tcy, tcx, 2)).astype(np.float32)).to(dev)
        movs.append((mov, tiles))

    def chain(batch):
        out = []
        f = [[torch.zeros(H, W, 2, device=dev) for _ in range(2)] for _ in range(nf)]
        S = [[torch.full((H, W), float("nan"), device=dev) for _ in range(2)] for _ in range(nf)]
        D = [[torch.full((H, W), float("nan"), device=dev) for _ in range(2)] for _ in range(nf)]
        for k, (mov, tiles) in enumerate(movs):
            L.CreateFlowFieldWarped(f[k][0].data_ptr(), capi.tex(tiles), W, H, W * 8, capi.f2([0, 0]), 0.0, None, ref.data_ptr(),
                                    mov.data_ptr(), W * 4, S[k][0].data_ptr(), D[k][0].data_ptr(), W * 4, st)
        for it in range(3):
            i, o = it & 1, (it & 1) ^ 1
            last = it == 2
            if batch:
                arr = (capi.LkFrame * nf)()
                for k, (mov, _) in enumerate(movs):
                    arr[k] = capi.LkFrame(f[k][i].data_ptr(), f[k][o].data_ptr(), mov.data_ptr(), S[k][i].data_ptr(), D[k][i].data_ptr(),
                                          None if last else S[k][o].data_ptr(), None if last else D[k][o].data_ptr())
                L.lucasKanadeSweepBatch(nf, arr, ref.data_ptr(), W * 8, W * 4, W * 4, W, H, hw, 1e-4, 2.0 if last else 1.0, st)
            else:
                for k, (mov, _) in enumerate(movs):
                    L.lucasKanadeIterationWarped(f[k][i].data_ptr(), f[k][o].data_ptr(), W * 8, ref.data_ptr(), mov.data_ptr(), W * 4,
                                                 S[k][i].data_ptr(), D[k][i].data_ptr(), None if last else S[k][o].data_ptr(),
                                                 None if last else D[k][o].data_ptr(), W * 4, W, H, hw, 1e-4, 2.0 if last else 1.0, st)
        torch.cuda.synchronize()
        return [f[k][1].cpu().numpy() for k in range(nf)]

    want = chain(False)
    got = chain(True)
    for k in range(nf):
        d = np.abs(want[k] - got[k])
        print(f"frame {k}: |flow(sweep) - flow(tile kernel)|: max {d.max():.2e} px, p99.9 {np.percentile(d, 99.9):.2e}, p99 {np.percentile(d, 99):.2e}, "
              f"median {np.median(d):.2e}, fraction > 1e-4: {np.mean(d > 1e-4):.2e}; moved by {np.abs(want[k]).max():.2f}")
        assert np.abs(want[k]).max() > 0.5
        if hw >= 3:
            # windows whose smaller singular value is tiny amplify the last-bit differences of the sums (the same windows in
            # which either kernel differs from the three-kernel chain and from the oracle): classified, not excused by a
            # loose maximum -- over the well-conditioned interior windows the two kernels agree to 5e-4 px (they do to ~1e-5),
            # so every larger difference sits in a low-sigma2 window, a border row or an unconverged flow
            from tests.burst_compare import flow_difference_report
            rep = flow_difference_report(got[k] / 2.0, want[k] / 2.0, ref.cpu().numpy(), hw, thr=5e-4)
            print(f"   well-conditioned windows ({rep['well_fraction']:.0%}): max {rep['max_well']:.2e} px; rest: max {rep['max_rest']:.2e} px")
            assert np.median(d) <= 1e-5 and np.percentile(d, 99) <= 1.5e-4 and np.mean(d > 1e-3) <= 1e-4
            assert rep["max_well"] <= 5e-4 and rep["well_fraction"] >= 0.3
        else:
            assert np.mean(d > 1e-4) < 2e-2
    if W >= 1920:
        # informational: time per iteration-equivalent at the pipeline's size
        f = [[torch.zeros(H, W, 2, device=dev) for _ in range(2)] for _ in range(nf)]
        S = [[torch.zeros(H, W, device=dev) for _ in range(2)] for _ in range(nf)]
        D = [[torch.zeros(H, W, device=dev) for _ in range(2)] for _ in range(nf)]
        arr = (capi.LkFrame * nf)()
        for k, (mov, _) in enumerate(movs):
            arr[k] = capi.LkFrame(f[k][0].data_ptr(), f[k][1].data_ptr(), mov.data_ptr(), S[k][0].data_ptr(), D[k][0].data_ptr(),
                                  S[k][1].data_ptr(), D[k][1].data_ptr())
        for name, fn in (("sweep x%d" % nf, lambda: L.lucasKanadeSweepBatch(nf, arr, ref.data_ptr(), W * 8, W * 4, W * 4, W, H, hw, 1e-4, 1.0, st)),
                         ("tile kernel x%d" % nf, lambda: [L.lucasKanadeIterationWarped(f[k][0].data_ptr(), f[k][1].data_ptr(), W * 8, ref.data_ptr(),
                                                           movs[k][0].data_ptr(), W * 4, S[k][0].data_ptr(), D[k][0].data_ptr(), S[k][1].data_ptr(),
                                                           D[k][1].data_ptr(), W * 4, W, H, hw, 1e-4, 1.0, st) for k in range(nf)])):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                fn()
            e1.record()
            torch.cuda.synchronize()
            print(f"{name}: {e0.elapsed_time(e1) / 20 / nf * 1e3:.1f} us per frame-iteration at {W}x{H}")


def test_structure_tensor_and_kernel_param(orc, hip):
    H, W = 44, 60
    img = _smooth_image(57, H, W)
    Ix, Iy = (np.zeros((H, W), np.float32) for _ in range(2))
    orc.call("ComputeDerivatives2Kernel", W, H, pitch_of(Ix), Ix, Iy, Tex(img))

    def make():
        out = np.zeros((H, W, 3), np.float32)
        return (Ix, Iy, out, W, H, pitch_of(Ix), pitch_of(out)), [out]

    (o,), (h,) = run_both(orc, hip, "ComputeStructureTensor", make)
    assert_bitexact(o, h, "ComputeStructureTensor")
    fused = np.zeros((H, W, 3), np.float32)
    hip.call("structureTensorFused", img, pitch_of(img), fused, pitch_of(fused), W, H)
    # direct texel loads instead of bilinear fetches at pixel centres: <= 1e-6 relative blend error
    np.testing.assert_allclose(fused, o, rtol=1e-4, atol=1e-7)

    def make_k():
        t = o.copy()
        t[0, 0] = 0          # lam1+lam2 = 0 -> NaN anisotropy
        t[0, 1] = [1e-3, 1e-3, 0]  # isotropic: help = 0 -> (c,s) fallback
        return (t, W, H, pitch_of(t), 0.005, 0.05, 0.3, 2.0, 2.0, 2.0), [t]

    (ok,), (hk,) = run_both(orc, hip, "ComputeKernelParam", make_k)
    assert_bitexact(ok, hk, "ComputeKernelParam")


# ---------------------------------------------------------------- F: robustness
def test_ComputeRobustnessMask(orc, hip):
    H, W = 36, 52
    r = rng(60)
    ref = r.random((H, W, 3), dtype=np.float32)
    mov = np.clip(ref + r.normal(0, 0.02, ref.shape).astype(np.float32), 0, 1).astype(np.float32)
    mov[5:9, 5:9] += 0.5
    uv = r.uniform(-5, 5, (H, W, 2)).astype(np.float32)

    def make():
        mask = np.zeros((H, W, 4), np.float32)
        return (ref, mov, mask, Tex(uv), W, H, pitch_of(ref), pitch_of(mask), 1e-4, 1e-6, 0.8), [mask]

    (o,), (h,) = run_both(orc, hip, "ComputeRobustnessMask", make)
    # expf: ocml vs glibc (<= 2 ulp of an O(1) value)
    np.testing.assert_allclose(h, o, atol=1e-6, rtol=1e-6)
    assert (h[0] == 0).all() and (h[:, -1] == 0).all()  # ring untouched
    assert h[..., :3].max() > 0.5 and h[..., :3].min() == 0.0


@pytest.mark.parametrize("uv_scale", [1, 2])
def test_robustnessMaskFused(orc, hip, uv_scale):
    """The MI355X robustness kernel (LDS reference tile, hardware sqrt / rcp / exp, zero ring folded in) against the
    oracle's ComputeRobustnessMask: mask within 2e-6, the rounded moved-patch shifts identical (they are taken with the
    straight kernel's arithmetic), also with the flow field at twice the image resolution (monochrome pipeline)."""
    H, W = 75, 141          # partial tiles on both axes
    r = rng(61)
    ref = r.random((H, W, 3), dtype=np.float32)
    mov = np.clip(ref + r.normal(0, 0.02, ref.shape).astype(np.float32), 0, 1).astype(np.float32)
    mov[5:9, 5:9] += 0.5
    uv = r.uniform(-5, 5, (H * uv_scale, W * uv_scale, 2)).astype(np.float32)
    mo = np.zeros((H, W, 4), np.float32)
    orc.call("ComputeRobustnessMask", ref, mov, mo, Tex(uv), W, H, pitch_of(ref), pitch_of(mo), 1e-4, 1e-6, 0.8)
    mh = np.full((H, W, 4), 99.0, np.float32)
    hip.call("robustnessMaskFused", ref, mov, mh, Tex(uv), W, H, pitch_of(ref), pitch_of(mh), 1e-4, 1e-6, 0.8)
    assert (mh[0] == 0).all() and (mh[-1] == 0).all() and (mh[:, 0] == 0).all() and (mh[:, -1] == 0).all()
    # M decides s = 1.5 / 0 at the threshold: compare where both sides are on the same side of it (1-ulp sqrt)
    same = (mo[..., 3] > 0.8) == (mh[..., 3] > 0.8)
    assert same.mean() > 0.999
    d = np.abs(mh - mo) * same[..., None]
    worst = np.unravel_index(np.argsort(d.reshape(-1))[-3:], d.shape)
    for y, x, c in zip(*worst):
        print(f"worst |d| {d[y, x, c]:.2e} at ({y},{x}) ch {c}: hip {mh[y, x]} oracle {mo[y, x]} ref patch std "
              f"{ref[y - 1:y + 2, x - 1:x + 2].std(axis=(0, 1))}")
    print("fraction of mask samples off by more than 2e-6:", float((d[..., :3] > 2e-6).mean()))
    # hardware sqrt / rcp / exp (1 ulp each) through exp(-d^2 / sigma^2): a few 1e-6 where the exponent is large
    np.testing.assert_allclose(mh[same], mo[same], atol=1e-5, rtol=2e-6)
    assert float((d[..., :3] > 2e-6).mean()) < 5e-3
    assert mh[..., :3].max() > 0.5 and (mh[..., :3] == 0).any()


# ---------------------------------------------------------------- H / I / glue
def test_ApplyWeighting_Gamma(orc, hip):
    H, W = 30, 44
    r = rng(61)
    fin = r.random((H, W, 3), dtype=np.float32) * 4
    wt = r.random((H, W, 3), dtype=np.float32) * 4
    wt[0, :5] = 0
    wt[1, :5] = -1          # w + 1 == 0 -> output 0
    wt[2, :5] = 1e-4        # below threshold -> fallback blended in

    def make():
        io = r0.copy()
        return (io, fin, wt, W, H, pitch_of(io), 1e-3), [io]

    r0 = rng(62).random((H, W, 3), dtype=np.float32)
    (o,), (h,) = run_both(orc, hip, "ApplyWeighting", make)
    assert_bitexact(o, h, "ApplyWeighting")

    def make_g():
        io = (o * 1.2 - 0.1).astype(np.float32)
        io[0, 0] = np.nan
        return (io, W, H, pitch_of(io)), [io]

    (og,), (hg,) = run_both(orc, hip, "GammasRGB", make_g)
    np.testing.assert_allclose(hg, og, atol=3e-7, rtol=3e-7)  # powf: ocml vs glibc
    assert hg[0, 0, 0] == 0.0


def test_finishFused_equals_chain(orc, hip):
    H, W, s = 24, 36, 2
    hrH, hrW = H * s, W * s
    r = rng(63)
    fb = r.random((H, W, 3), dtype=np.float32)
    fin = r.random((hrH, hrW, 3), dtype=np.float32) * 3
    wt = r.random((hrH, hrW, 3), dtype=np.float32) * 3
    wt[:3] = 0
    io = np.zeros((hrH, hrW, 3), np.float32)
    orc.call("resampleFloat3", fb, pitch_of(fb), W, H, io, pitch_of(io), hrW, hrH, 0.0, 1.0, 0.0, 1.0)
    orc.call("ApplyWeighting", io, fin, wt, hrW, hrH, pitch_of(io), 1e-3)
    lin = io.copy()
    orc.call("GammasRGB", io, hrW, hrH, pitch_of(io))
    q = np.zeros((hrH, hrW, 3), np.uint16)
    orc.call("quantize", io, pitch_of(io), q, None, hrW, hrH, 65535.0)
    out = np.zeros_like(io)
    q2 = np.zeros_like(q)
    hip.call("finishFused", fin, wt, pitch_of(fin), fb, pitch_of(fb), W, H, 0.0, 1.0, 0.0, 1.0, out, pitch_of(out), q2,
             hrW, hrH, 1e-3, 1, 65535.0)
    np.testing.assert_allclose(out, io, atol=3e-7, rtol=3e-7)
    assert np.abs(q2.astype(np.int32) - q.astype(np.int32)).max() <= 1   # +-1 LSB (16 bit)
    out_lin = np.zeros_like(io)
    hip.call("finishFused", fin, wt, pitch_of(fin), fb, pitch_of(fb), W, H, 0.0, 1.0, 0.0, 1.0, out_lin, pitch_of(out),
             None, hrW, hrH, 1e-3, 0, 65535.0)
    assert_bitexact(lin, out_lin, "finishFused (no gamma)")


def test_fourier_helpers(orc, hip):
    H, W = 32, 48
    spec = rng(64).random((H, W // 2 + 1, 2), dtype=np.float32)
    for lp, hp, lps, hps, ca in [(0.3, 0.0, 0.0, 0.0, 0), (0.3, 0.05, 0.05, 0.02, 2), (0.0, 0.0, 0.1, 0.0, 0)]:
        def make():
            s = spec.copy()
            return (s, pitch_of(s), W, H, lp, hp, lps, hps, ca), [s]
        (o,), (h,) = run_both(orc, hip, "fourierFilter", make)
        np.testing.assert_allclose(h, o, atol=1e-6, rtol=1e-5)  # expf

    def make_s():
        s = rng(65).random((H, W, 2), dtype=np.float32)
        return (s, W, H), [s]
    (o,), (h,) = run_both(orc, hip, "fftshift", make_s)
    assert_bitexact(o, h, "fftshift")

    def make_c():
        a = rng(66).random((100, 2), dtype=np.float32)
        b = rng(67).random((100, 2), dtype=np.float32)
        return (a, b, 100), [b]
    (o,), (h,) = run_both(orc, hip, "conjugateComplexMulKernel", make_c)
    assert_bitexact(o, h, "conjugateComplexMulKernel")


def test_glue_stages(orc, hip):
    H, W = 34, 50
    r = rng(70)
    rgb = r.random((H, W, 3), dtype=np.float32)

    def mk_gray():
        out = np.zeros((H, W), np.float32)
        return (rgb, pitch_of(rgb), out, pitch_of(out), W, H), [out]
    (o,), (h,) = run_both(orc, hip, "rgbToGray", mk_gray)
    assert_bitexact(o, h, "rgbToGray")
    gray = o
    raw = r.integers(0, 4096, (H, W), dtype=np.uint16)

    def mk_u16():
        out = np.zeros((H, W), np.float32)
        return (raw, out, pitch_of(out), W, H, 1.0 / 4095.0), [out]
    (o,), (h,) = run_both(orc, hip, "u16ToFloat", mk_u16)
    assert_bitexact(o, h, "u16ToFloat")
    taps = np.zeros(99, np.float32)
    n = orc.o.gaussin_filter_1D(1.0, taps)
    for chan, src in [(1, gray), (3, rgb)]:
        def mk_f():
            tmp, out = np.zeros_like(src), np.zeros_like(src)
            return (src, pitch_of(src), tmp, out, pitch_of(out), W, H, chan, Host(taps), n), [out]
        (o,), (h,) = run_both(orc, hip, "separableFilter", mk_f)
        assert_bitexact(o, h, f"separableFilter chan={chan}")

    def mk_d():
        out = np.zeros((H // 2, W // 2), np.float32)
        return (gray, pitch_of(gray), out, pitch_of(out), W // 2, H // 2), [out]
    (o,), (h,) = run_both(orc, hip, "downsample2x", mk_d)
    assert_bitexact(o, h, "downsample2x")
    fl = r.uniform(-3, 3, (H, W, 2)).astype(np.float32)

    def mk_s():
        f = fl.copy()
        return (f, pitch_of(f), W, H, 2.0), [f]
    (o,), (h,) = run_both(orc, hip, "scaleFlow", mk_s)
    assert_bitexact(o, h, "scaleFlow")

    def mk_4():
        out = np.ones((H, W, 4), np.float32)
        return (rgb, pitch_of(rgb), out, pitch_of(out), W, H), [out]
    (o,), (h,) = run_both(orc, hip, "float3ToFloat4", mk_4)
    assert_bitexact(o, h, "float3ToFloat4")

    def mk_r():
        out = np.zeros((H * 3, W * 3, 3), np.float32)
        return (rgb, pitch_of(rgb), W, H, out, pitch_of(out), W * 3, H * 3, 0.25, 0.75, 0.1, 0.9), [out]
    (o,), (h,) = run_both(orc, hip, "resampleFloat3", mk_r)
    assert_bitexact(o, h, "resampleFloat3")
    img8 = r.integers(0, 256, (H, W, 3), dtype=np.uint8)

    def mk_sh():
        out = np.full((H, W, 3), 9, np.uint8)
        return (img8, out, H, W, 3, W * 3, W * 3), [out]
    (o,), (h,) = run_both(orc, hip, "sharpenImg2", mk_sh)
    np.testing.assert_array_equal(o, h)


def test_sharpenImg_unsharp_mask(orc, hip):
    """sharpenImg (test_opencv/main.cpp:525-534) on device u8 vs the oracle: identical bytes (integer decisions on float
    tap sums that are taken in the same order; the blur's rounding is RNE on both sides)."""
    r = rng(77)
    rows, cols, ch = 37, 53, 3
    img = r.integers(0, 256, (rows, cols, ch), dtype=np.uint8)
    img[10:20, 10:30] = 200          # flat block: low contrast -> copied through
    img[:, 40:] = np.clip(img[:, 40:].astype(int) // 8 + 100, 0, 255).astype(np.uint8)
    o = np.zeros_like(img)
    h = np.zeros_like(img)
    tmp_o, tmp_h = np.zeros_like(img), np.zeros_like(img)
    orc.call("sharpenImg", img, o, tmp_o, rows, cols, ch, cols * ch, cols * ch)
    hip.call("sharpenImg", img, h, tmp_h, rows, cols, ch, cols * ch, cols * ch)
    np.testing.assert_array_equal(tmp_o, tmp_h)
    np.testing.assert_array_equal(o, h)
    assert (o != img).mean() > 0.3 and (o[12:18, 14:26] == 200).all()
    # known answer: a constant image is its own blur -> returned unchanged
    flat = np.full((9, 11, 1), 77, np.uint8)
    out = np.zeros_like(flat)
    orc.call("sharpenImg", flat, out, np.zeros_like(flat), 9, 11, 1, 11, 11)
    assert (out == 77).all()


def test_gaussin_filter_1D_host(orc, hip):
    import ctypes
    for sigma in [0.0, 0.5, 1.0, 2.7, 100.0]:
        t1 = np.zeros(99, np.float32)
        n1 = orc.o.gaussin_filter_1D(sigma, t1)
        t2 = (ctypes.c_float * 99)()
        n2 = hip.L.gaussin_filter_1D(sigma, t2)
        assert n1 == n2
        np.testing.assert_array_equal(t1[:n1], np.array(t2[:n2], np.float32))


# ---- global pre-alignment (csrc/prealign.hip vs oracle/prealign.c): integer scores -> identical results ----------
def _rotated_pair(W, H, angle_deg, tx, ty, seed):
    """A smooth random image and the same scene sampled at c + R(angle)(p - c - t) (what the model says the moved
    frame shows at reference pixel p)."""
    from scipy import ndimage
    r = rng(seed)
    big = ndimage.gaussian_filter(r.random((H + 200, W + 200)), 2.0)
    big = ((big - big.min()) / (big.max() - big.min())).astype(np.float32)
    big += 0.25 * (ndimage.gaussian_filter(r.random(big.shape), 8.0) > 0.5)
    big = (big / big.max()).astype(np.float32)
    ref = np.ascontiguousarray(big[100:100 + H, 100:100 + W])
    a = np.radians(angle_deg)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = W // 2, H // 2
    # moved(q) = scene(p) with q = c + R(p - c - t)  <=>  p = c + t + R^-1 (q - c)
    dx, dy = xx - cx, yy - cy
    px = cx + tx + np.cos(a) * dx + np.sin(a) * dy
    py = cy + ty - np.sin(a) * dx + np.cos(a) * dy
    mov = ndimage.map_coordinates(big, [py + 100, px + 100], order=1, mode="nearest").astype(np.float32)
    return ref, np.ascontiguousarray(mov)


@pytest.mark.parametrize("W,H,angle,tx,ty", [(256, 128, 7.0, 3.0, -2.0), (200, 150, -12.5, -5.0, 4.0), (96, 64, 0.0, 1.0, 1.0),
                                             (1300, 700, 3.3, 20.0, -11.0)])
def test_preAlign_matches_oracle_exactly(orc, hip, W, H, angle, tx, ty):
    import torch
    ref, mov = _rotated_pair(W, H, angle, tx, ty, 91)
    res = np.zeros(5, np.float32)
    st = np.zeros(4, np.int32)
    n = orc.o.preAlign(ref, mov, W, H, pitch_of(ref), 20.0, res, st)
    assert n >= 1
    assert abs(np.degrees(res[2]) - angle) <= 0.6   # the grid step of the finest searched level is <= 0.5 degree
    L = hip.L
    dev = hip.dev
    pb = L.preAlign_pyramid_bytes(W, H)
    wb = L.preAlign_workspace_bytes(20.0)
    assert pb > 0 and wb > 0
    bufs = [torch.zeros(x + 256, dtype=torch.uint8, device=dev) for x in (pb, pb, wb, 256)]
    ptr = [(b.data_ptr() + 255) // 256 * 256 for b in bufs]
    dref, dmov = torch.from_numpy(ref).to(dev), torch.from_numpy(mov).to(dev)
    L.preAlign_init(ptr[2], 20.0, None)
    L.preAlignPyramid(dref.data_ptr(), W, H, pitch_of(ref), ptr[0], None)
    L.preAlignPyramid(dmov.data_ptr(), W, H, pitch_of(mov), ptr[1], None)
    for _ in range(2):   # a second search on the same workspace starts from clean scores
        L.preAlign(ptr[0], ptr[1], W, H, 20.0, ptr[2], ptr[3], None)
    torch.cuda.synchronize()
    off = ptr[3] - bufs[3].data_ptr()
    raw = bufs[3][off:off + 48].cpu().numpy()
    f = raw[:20].view(np.float32)
    i = raw[20:36].view(np.int32)
    assert tuple(i) == tuple(st), (i, st)
    assert_bitexact(f, res, "preAlign result")
