"""Launch-edge shapes with padded pitches, and the row-stripe entry points, against the oracle.

Every entry point of include/mfsr.h that takes a pitch or a width appears in ``SWEEP`` (this module) or in ``EXCLUDED``
(tests/test_kernel_edges_cpu.py checks that against the header).  Per entry point:

  * shapes: the smallest the entry accepts, block - 1 / block / block + 1 in x crossed with the same in y (the ``dim3 block``
    or tile constants of its launch site), and one odd x odd size of a few blocks;
  * the oracle runs on DENSE arrays, HIP on arrays whose pitch is the row bytes plus the smallest padding its alignment rule
    allows that makes the pitch no multiple of 64.  Input padding is 0xFF bytes (NaN / 0xFFFF / -1: a read of it cannot
    cancel out, because the oracle never sees it), output padding is a sentinel that must survive;
  * the tolerance is the one next to that kernel's assertion in tests/test_parity_kernels.py (None: bit for bit);
  * the hostile values of that test are kept (NaN certainties, NaN / 1e9 flows, non-PSD kernel parameters, w + 1 == 0).

All out-of-bounds detection goes through memory the test owns: the guards of ``tests/kernels.py::guarded_upload``, the pitch
padding, and canary rows.
"""
import ctypes

import numpy as np
import pytest

from tests.kernels import F2, F3, Host, Tex, guarded_upload
from tests.test_parity_kernels import PATTERNS, RGGB, _accum_inputs, _kernel_field, _smooth_image, assert_bitexact, rng

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3          # output padding and canary rows (not the guards' 0xFF, so a report tells the two apart)
POISON = 0xFF            # input padding


# ---------------------------------------------------------------- placement: dense (oracle) and padded (HIP)
def texel_align(a):
    """The pitch alignment the entry points ask of an image of this texel: 8 for float2, 16 for float4, else the scalar's size
    (float3 rows are only 4-byte aligned)."""
    texel = a.itemsize * int(np.prod(a.shape[2:], dtype=np.int64))
    return texel if texel in (8, 16) else a.itemsize


def padded_pitch(row_bytes, align):
    pitch = -(-row_bytes // align) * align
    if pitch == row_bytes:
        pitch += align
    while pitch % 64 == 0:
        pitch += align
    return pitch


class Dense:
    def inp(self, a, align=None):
        a = np.ascontiguousarray(a).copy()
        return a, a.strides[0]

    out = inp

    def tex(self, a, align=None):
        b, p = self.inp(a)
        return Tex(b, a.shape[1], a.shape[0], p)

    def get(self, b):
        return b


class Padded:
    def __init__(self):
        self.meta = {}

    def _place(self, a, fill, align, writeable):
        a = np.ascontiguousarray(a)
        rowb = a.strides[0]
        pitch = padded_pitch(rowb, align or texel_align(a))
        buf = np.full((a.shape[0], pitch), fill, np.uint8)
        buf[:, :rowb] = a.view(np.uint8).reshape(a.shape[0], rowb)
        buf.flags.writeable = writeable          # read-only: HipKernels.call also checks that the kernel left it alone
        self.meta[id(buf)] = (buf, a.shape, a.dtype, rowb)
        return buf, pitch

    def inp(self, a, align=None):
        return self._place(a, POISON, align, False)

    def out(self, a, align=None):
        return self._place(a, SENTINEL, align, True)

    def tex(self, a, align=None):
        b, p = self.inp(a, align)
        return Tex(b, a.shape[1], a.shape[0], p)

    def get(self, b):
        if id(b) not in self.meta:           # an argument that is dense by contract
            return b
        buf, shape, dtype, rowb = self.meta[id(b)]
        bad = np.argwhere(buf[:, rowb:] != SENTINEL)
        assert bad.size == 0, f"pitch padding of an output changed, first at row {bad[0][0]}, byte {rowb + bad[0][1]} of the row"
        return buf[:, :rowb].copy().view(dtype).reshape(shape)


def run(k, P, fname, build):
    args, outs = build(P)
    k.call(fname, *args)
    return [P.get(o).copy() for o in outs]


def both(orc, hip, fname, build):
    return run(orc, Dense(), fname, build), run(hip, Padded(), fname, build)


def same(o, h, tol, what):
    if tol is None:
        assert_bitexact(o, h, what)
    else:
        np.testing.assert_allclose(h, o, err_msg=what, **tol)


def shapes(bx, by, minw=1, minh=1, odd=(131, 11)):
    s = [(minw, minh)] + [(bx + dx, by + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)] + [odd]
    out = []
    for w, h in s:
        if w >= minw and h >= minh and (w, h) not in out:
            out.append((w, h))
    return out


B64x4 = shapes(64, 4)
SWEEP = {}        # entry point -> name of the case that covers it
CASES = {}        # case name -> (function, shapes)


def case(*entries, shp=B64x4):
    def deco(fn):
        CASES[fn.__name__] = (fn, shp)
        for e in entries:
            SWEEP["mfsr_" + e] = fn.__name__
        return fn
    return deco


def set_cfa(orc, hip, pat):
    orc.set_cfa(pat)
    hip.set_cfa(pat)


# ---------------------------------------------------------------- A: DeBayer
@case("deBayersSubSample3")
def c_subsample(orc, hip, w, h, first):
    for pat in (list(PATTERNS) if first else ["GRBG"]):
        set_cfa(orc, hip, PATTERNS[pat])
        raw = rng(1).integers(0, 4096, (2 * h, 2 * w), dtype=np.uint16)

        def build(P):
            out, p = P.out(np.zeros((h, w, 3), np.float32))
            return (raw, out, 4095.0, w, h, p), [out]

        (o,), (g,) = both(orc, hip, "deBayersSubSample3", build)
        same(o, g, None, f"deBayersSubSample3 {pat} {w}x{h}")


def _debayer_chain(k, P, raw16, w, h, bp, sc):
    rawf, pi = P.inp(raw16.astype(np.float32))
    out, po = P.out(np.zeros((h, w, 3), np.float32))
    k.call("deBayerGreenKernel", w, h, rawf, pi, out, po, bp, sc)
    green = P.get(out).copy()
    k.call("deBayerRedBlueKernel", w, h, rawf, pi, out, po, bp, sc)
    return green, P.get(out).copy()


@case("deBayerGreenKernel", "deBayerRedBlueKernel")
def c_debayer_chain(orc, hip, w, h, first):
    bp, sc = F3([256, 250, 260]), F3([1 / 3839.0, 1 / 3800.0, 1 / 3850.0])
    for pat in (list(PATTERNS) if first else ["GBRG"]):
        set_cfa(orc, hip, PATTERNS[pat])
        raw16 = rng(2).integers(200, 4096, (h, w), dtype=np.uint16)
        og, ob = _debayer_chain(orc, Dense(), raw16, w, h, bp, sc)
        hg, hb = _debayer_chain(hip, Padded(), raw16, w, h, bp, sc)
        same(og, hg, None, f"deBayerGreenKernel {pat} {w}x{h}")
        same(ob, hb, None, f"deBayerRedBlueKernel {pat} {w}x{h}")


@case("deBayerFused", shp=shapes(64, 8, 5, 5, (131, 19)))          # DBF_TX x DBF_TY tiles, width and height > 4
def c_debayer_fused(orc, hip, w, h, first):
    bp, sc = F3([256, 250, 260]), F3([1 / 3839.0, 1 / 3800.0, 1 / 3850.0])
    for pat in (list(PATTERNS) if first else ["BGGR"]):
        set_cfa(orc, hip, PATTERNS[pat])
        raw16 = rng(2).integers(200, 4096, (h, w), dtype=np.uint16)
        _, want = _debayer_chain(orc, Dense(), raw16, w, h, bp, sc)
        P = Padded()
        out, po = P.out(np.zeros((h, w, 3), np.float32))
        raw_in = raw16.copy()
        raw_in.flags.writeable = False         # so that the call checks that the input is left alone
        hip.call("deBayerFused", raw_in, out, po, w, h, bp, sc)
        same(want, P.get(out), None, f"deBayerFused {pat} {w}x{h}")


@case("prepareFrameFused", shp=shapes(64, 16, 2, 2, (131, 35)))    # PREP_TX x PREP_TY tiles of the half-resolution frame
def c_prepare(orc, hip, w, h, first):
    set_cfa(orc, hip, RGGB)
    raw = rng(150).integers(0, 4096, (2 * h, 2 * w), dtype=np.uint16)
    taps = np.zeros(99, np.float32)
    n = orc.o.gaussin_filter_1D(1.2, taps)
    half, gray = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    tmp, p0, p1 = np.zeros_like(gray), np.zeros_like(gray), np.zeros((h // 2, w // 2), np.float32)
    orc.call("deBayersSubSample3", raw, half, 4095.0, w, h, w * 12)
    orc.call("rgbToGray", half, w * 12, gray, w * 4, w, h)
    orc.call("separableFilter", gray, w * 4, tmp, p0, w * 4, w, h, 1, Host(taps), n)
    orc.call("downsample2x", p0, w * 4, p1, (w // 2) * 4, w // 2, h // 2)
    P = Padded()
    fh, ph = P.out(np.zeros_like(half))
    f0, q0 = P.out(np.zeros_like(p0))
    f1, q1 = P.out(np.zeros_like(p1))
    hip.call("prepareFrameFused", raw, fh, ph, 4095.0, w, h, f0, q0, f1, q1, Host(taps), n)
    same(half, P.get(fh), None, f"prepareFrameFused half-res RGB {w}x{h}")
    same(p0, P.get(f0), None, f"prepareFrameFused luma {w}x{h}")
    same(p1, P.get(f1), None, f"prepareFrameFused pyramid level 1 {w}x{h}")


# ---------------------------------------------------------------- glue stages
@case("rgbToGray")
def c_rgbToGray(orc, hip, w, h, first):
    rgb = rng(70).random((h, w, 3), dtype=np.float32)

    def build(P):
        i, pi = P.inp(rgb)
        o, po = P.out(np.zeros((h, w), np.float32))
        return (i, pi, o, po, w, h), [o]
    (o,), (g,) = both(orc, hip, "rgbToGray", build)
    same(o, g, None, f"rgbToGray {w}x{h}")


@case("u16ToFloat")
def c_u16ToFloat(orc, hip, w, h, first):
    raw = rng(71).integers(0, 4096, (h, w), dtype=np.uint16)

    def build(P):
        o, po = P.out(np.zeros((h, w), np.float32))
        return (raw, o, po, w, h, 1.0 / 4095.0), [o]
    (o,), (g,) = both(orc, hip, "u16ToFloat", build)
    same(o, g, None, f"u16ToFloat {w}x{h}")


@case("separableFilter")
def c_separableFilter(orc, hip, w, h, first):
    taps = np.zeros(99, np.float32)
    n = orc.o.gaussin_filter_1D(1.0, taps)
    for chan in (1, 3):
        src = rng(72).random((h, w) if chan == 1 else (h, w, 3), dtype=np.float32)

        def build(P):
            i, pi = P.inp(src)
            t, _ = P.out(np.zeros_like(src))           # the intermediate image has the output's pitch
            o, po = P.out(np.zeros_like(src))
            return (i, pi, t, o, po, w, h, chan, Host(taps), n), [o, t]
        # the intermediate image is fetched only so that its pitch padding is checked; its values are not part of the contract
        (o, ot), (g, gt) = both(orc, hip, "separableFilter", build)
        same(o, g, None, f"separableFilter chan={chan} {w}x{h}")


@case("downsample2x")
def c_downsample2x(orc, hip, w, h, first):
    # w x h is the OUTPUT; odd input sizes as well (the last input column / row is then not read)
    for ex in (0, 1):
        src = rng(73).random((2 * h + ex, 2 * w + ex), dtype=np.float32)

        def build(P):
            i, pi = P.inp(src, align=8)                # rows are read as float2
            o, po = P.out(np.zeros((h, w), np.float32))
            return (i, pi, o, po, w, h), [o]
        (o,), (g,) = both(orc, hip, "downsample2x", build)
        same(o, g, None, f"downsample2x {w}x{h} from {src.shape}")


@case("scaleFlow")
def c_scaleFlow(orc, hip, w, h, first):
    fl = rng(74).uniform(-3, 3, (h, w, 2)).astype(np.float32)
    fl[0, 0] = [np.nan, 1e9]

    def build(P):
        f, p = P.out(fl)
        return (f, p, w, h, 2.0), [f]
    (o,), (g,) = both(orc, hip, "scaleFlow", build)
    same(o, g, None, f"scaleFlow {w}x{h}")


@case("float3ToFloat4")
def c_float3ToFloat4(orc, hip, w, h, first):
    rgb = rng(75).random((h, w, 3), dtype=np.float32)

    def build(P):
        i, pi = P.inp(rgb)
        o, po = P.out(np.ones((h, w, 4), np.float32))
        return (i, pi, o, po, w, h), [o]
    (o,), (g,) = both(orc, hip, "float3ToFloat4", build)
    same(o, g, None, f"float3ToFloat4 {w}x{h}")


@case("resampleFloat3")
def c_resampleFloat3(orc, hip, w, h, first):
    iw, ih = w // 3 + 1, h // 3 + 1
    rgb = rng(76).random((ih, iw, 3), dtype=np.float32)

    def build(P):
        i, pi = P.inp(rgb)
        o, po = P.out(np.zeros((h, w, 3), np.float32))
        return (i, pi, iw, ih, o, po, w, h, 0.25, 0.75, 0.1, 0.9), [o]
    (o,), (g,) = both(orc, hip, "resampleFloat3", build)
    same(o, g, None, f"resampleFloat3 {iw}x{ih} -> {w}x{h}")


@case("quantize")
def c_quantize(orc, hip, w, h, first):
    img = (rng(77).random((h, w, 3), dtype=np.float32) * 1.2 - 0.1).astype(np.float32)
    for bits in (16, 8):
        def build(P):
            i, pi = P.inp(img)
            q = np.zeros((h, w, 3), np.uint16 if bits == 16 else np.uint8)       # dense by contract (no pitch argument)
            return (i, pi, q if bits == 16 else None, q if bits == 8 else None, w, h, 65535.0 if bits == 16 else 255.0), [q]
        (o,), (g,) = both(orc, hip, "quantize", build)
        np.testing.assert_array_equal(o, g, err_msg=f"quantize {bits} bit {w}x{h}")


SHARPEN = [(1, 1, 1), (255, 1, 1), (256, 2, 1), (257, 3, 1), (85, 4, 3), (86, 5, 3), (131, 11, 3)]   # 256 bytes of a row per block


@case("sharpenImg", "sharpenImg2", shp=SHARPEN)
def c_sharpen(orc, hip, cols, rows, ch, first):
    img = rng(78).integers(0, 256, (rows, cols * ch), dtype=np.uint8)
    img[:, cols * ch // 2:] = (img[:, cols * ch // 2:] // 8 + 100).astype(np.uint8)

    def build2(P):
        i, pi = P.inp(img)
        o, po = P.out(np.full((rows, cols * ch), 9, np.uint8))
        return (i, o, rows, cols, ch, pi, po), [o]
    (o,), (g,) = both(orc, hip, "sharpenImg2", build2)
    np.testing.assert_array_equal(o, g, err_msg=f"sharpenImg2 {cols}x{rows}x{ch}")

    def build(P):
        i, pi = P.inp(img)
        o, po = P.out(np.zeros((rows, cols * ch), np.uint8))
        t = np.zeros((rows, cols * ch), np.uint8)      # dense by contract
        return (i, o, t, rows, cols, ch, pi, po), [o]
    (o,), (g,) = both(orc, hip, "sharpenImg", build)
    np.testing.assert_array_equal(o, g, err_msg=f"sharpenImg {cols}x{rows}x{ch}")


# ---------------------------------------------------------------- optical flow
@case("WarpingKernel")
def c_warp(orc, hip, w, h, first):
    img = _smooth_image(50, h, w)
    uv = rng(51).uniform(-6, 6, (h, w, 2)).astype(np.float32)
    uv[0, 0] = [-30, 200]

    def build(P):
        o, po = P.out(np.zeros((h, w), np.float32))
        return (w, h, po, P.tex(uv), o, P.tex(img)), [o]
    (o,), (g,) = both(orc, hip, "WarpingKernel", build)
    same(o, g, None, f"WarpingKernel {w}x{h}")


@case("CreateFlowFieldFromTiles")
def c_flowfield(orc, hip, w, h, first):
    tcx, tcy = max(1, w // 16), max(1, h // 16)
    ts = rng(52).uniform(-3, 3, (tcy, tcx, 2)).astype(np.float32)
    for rot in (0.0, 0.02):
        def build(P):
            o, po = P.out(np.zeros((h, w, 2), np.float32))
            return (o, P.tex(ts), 16, tcx, tcy, w, h, po, F2([0.5, -1.5] if rot else [0, 0]), rot), [o]
        (o,), (g,) = both(orc, hip, "CreateFlowFieldFromTiles", build)
        same(o, g, None if rot == 0.0 else dict(atol=2e-5), f"CreateFlowFieldFromTiles rot={rot} {w}x{h}")


@case("ComputeDerivativesKernel", "ComputeDerivatives2Kernel")
def c_derivatives(orc, hip, w, h, first):
    a, b = _smooth_image(53, h, w), _smooth_image(54, h, w)

    def build(P):
        outs = [P.out(np.zeros((h, w), np.float32)) for _ in range(3)]
        return (w, h, outs[0][1], outs[0][0], outs[1][0], outs[2][0], P.tex(a), P.tex(b)), [o for o, _ in outs]
    o, g = both(orc, hip, "ComputeDerivativesKernel", build)
    for x, y in zip(o, g):
        same(x, y, None, f"ComputeDerivativesKernel {w}x{h}")

    def build2(P):
        outs = [P.out(np.zeros((h, w), np.float32)) for _ in range(2)]
        return (w, h, outs[0][1], outs[0][0], outs[1][0], P.tex(a)), [o for o, _ in outs]
    o, g = both(orc, hip, "ComputeDerivatives2Kernel", build2)
    for x, y in zip(o, g):
        same(x, y, None, f"ComputeDerivatives2Kernel {w}x{h}")


@case("lucasKanadeOptim")
def c_lkOptim(orc, hip, w, h, first):
    r = rng(55)
    fx = (r.random((h, w), dtype=np.float32) - 0.5) * 0.4
    fy = (r.random((h, w), dtype=np.float32) - 0.5) * 0.4
    ft = (r.random((h, w), dtype=np.float32) - 0.5) * 0.1
    fx[h // 2:h // 2 + 4, w // 2:w // 2 + 4] = 0
    fy[h // 2:h // 2 + 4, w // 2:w // 2 + 4] = 0       # singular windows
    sh0 = r.uniform(-1, 1, (h, w, 2)).astype(np.float32)
    for hw in (1, 3):
        def build(P):
            sh, ps = P.out(sh0)
            ins = [P.inp(f) for f in (fx, fy, ft)]
            return (sh, ins[0][0], ins[1][0], ins[2][0], ps, ins[0][1], w, h, hw, 1e-3), [sh]
        (o,), (g,) = both(orc, hip, "lucasKanadeOptim", build)
        same(o, g, dict(atol=5e-5, rtol=1e-4), f"lucasKanadeOptim h={hw} {w}x{h}")
        assert_bitexact(g[:hw], sh0[:hw], "ring rows")


# 48- and 32-wide tiles of LK_TY = 16 rows.  Below width 32 + 2 h + 4 or height 16 + 2 h + 4 the tile's halo reaches past one
# reflection of the image (clamped: only the +-2 stencil about an updated pixel matters): the first three shapes, among them
# the 32 x 32 tracking image of the smallest frame the pipeline accepts
LKF = [(32, 32), (33, 20), (40, 17), (42, 26), (47, 31), (48, 32), (49, 33), (65, 47), (97, 49), (131, 35)]


@case("lucasKanadeIterationFused", shp=LKF)
def c_lkFused(orc, hip, w, h, first):
    hw = 3
    base = _smooth_image(56, h + 8, w + 8)
    ref = np.ascontiguousarray(base[4:4 + h, 4:4 + w])
    mov = np.ascontiguousarray(base[3:3 + h, 6:6 + w])
    flow0 = np.zeros((h, w, 2), np.float32)
    flow0[..., 0], flow0[..., 1] = -1.6, 0.7
    flow = flow0.copy()
    warped = np.zeros((h, w), np.float32)
    Ix, Iy, Iz = (np.zeros((h, w), np.float32) for _ in range(3))
    orc.call("WarpingKernel", w, h, w * 4, Tex(flow), warped, Tex(mov))
    orc.call("ComputeDerivativesKernel", w, h, w * 4, Ix, Iy, Iz, Tex(warped), Tex(ref))
    orc.call("lucasKanadeOptim", flow, Ix, Iy, Iz, w * 8, w * 4, w, h, hw, 1e-4)
    P = Padded()
    fi, pf = P.inp(flow0)
    out, po = P.out(np.full((h, w, 2), 99, np.float32))
    assert pf == po
    r_, pr = P.inp(ref)
    m_, _ = P.inp(mov)
    hip.call("lucasKanadeIterationFused", fi, out, po, r_, m_, pr, w, h, hw, 1e-4, 1.0)
    got = P.get(out)
    same(flow, got, dict(atol=1e-4), f"lucasKanadeIterationFused h={hw} {w}x{h}")
    assert_bitexact(got[:hw], flow0[:hw], "ring rows")


# h = 3: strips of VW = 54 columns, bands of 8 rows.  The minimum (width 64, height 2 (h + 2)), then VW - 1 / VW / VW + 1 columns of a
# second strip crossed with band - 1 / band / band + 1 rows of a second band, and two odd sizes
LKS = [(64, 10), (64, 11), (107, 15), (108, 16), (109, 17), (131, 11), (163, 35)]


@case("lucasKanadeSweepBatch", shp=LKS)
def c_lkSweep(orc, hip, w, h, first):
    # the guarded harness of the sweep's own module (three different padded pitches, every buffer between guards), one frame and
    # three: one iteration against the oracle at c_lkFused's tolerance, ring rows and columns and both warped planes bit for bit
    from tests.test_lk_sweep_gpu import conditioned_case, one_iteration_against_the_oracle
    for nf in (1, 3) if first else (1 + (w + h) % 4,):
        one_iteration_against_the_oracle(orc, hip, conditioned_case(orc, 3, w, h, nf, 90 + w), f"lucasKanadeSweepBatch h=3 {w}x{h} x{nf}")


# ---------------------------------------------------------------- structure tensor / kernel parameters
@case("ComputeStructureTensor", "ComputeKernelParam")
def c_tensor(orc, hip, w, h, first):
    img = _smooth_image(57, h, w)
    Ix, Iy = (np.zeros((h, w), np.float32) for _ in range(2))
    orc.call("ComputeDerivatives2Kernel", w, h, w * 4, Ix, Iy, Tex(img))

    def build(P):
        a, pa = P.inp(Ix)
        b, _ = P.inp(Iy)
        o, po = P.out(np.zeros((h, w, 3), np.float32))
        return (a, b, o, w, h, pa, po), [o]
    (o,), (g,) = both(orc, hip, "ComputeStructureTensor", build)
    same(o, g, None, f"ComputeStructureTensor {w}x{h}")
    t0 = o.copy()
    t0[0, 0] = 0
    t0[-1, -1] = [1e-3, 1e-3, 0]

    def build_k(P):
        t, p = P.out(t0)
        return (t, w, h, p, 0.005, 0.05, 0.3, 2.0, 2.0, 2.0), [t]
    (o,), (g,) = both(orc, hip, "ComputeKernelParam", build_k)
    same(o, g, None, f"ComputeKernelParam {w}x{h}")


@case("structureTensorFused", shp=shapes(64, 8, 4, 4, (131, 19)))      # ST_TX x ST_TY tiles, width and height >= 4
def c_tensorFused(orc, hip, w, h, first):
    img = _smooth_image(57, h, w)
    Ix, Iy = (np.zeros((h, w), np.float32) for _ in range(2))
    want = np.zeros((h, w, 3), np.float32)
    orc.call("ComputeDerivatives2Kernel", w, h, w * 4, Ix, Iy, Tex(img))
    orc.call("ComputeStructureTensor", Ix, Iy, want, w, h, w * 4, w * 12)
    P = Padded()
    i, pi = P.inp(img)
    o, po = P.out(np.zeros((h, w, 3), np.float32))
    hip.call("structureTensorFused", i, pi, o, po, w, h)
    same(want, P.get(o), dict(rtol=1e-4, atol=1e-7), f"structureTensorFused {w}x{h}")


# ---------------------------------------------------------------- robustness
THRESHOLD_M = 0.8
ROBUST_SHAPES = shapes(64, 4, 3, 3)
ROBUST_FUSED_SHAPES = shapes(64, 8, 3, 3, (131, 19))                  # RB_TX x RB_TY tiles


def robustness_inputs(seed, w, h, uv_scale=1):
    r = rng(seed)
    ref = r.random((h, w, 3), dtype=np.float32)
    mov = np.clip(ref + r.normal(0, 0.02, ref.shape).astype(np.float32), 0, 1).astype(np.float32)
    mov[h // 2:h // 2 + 4, w // 2:w // 2 + 4] += 0.5
    uv = r.uniform(-5, 5, (h * uv_scale, w * uv_scale, 2)).astype(np.float32)
    return ref, mov, uv


def robustness_oracle(orc, seed, w, h, uv_scale=1):
    ref, mov, uv = robustness_inputs(seed, w, h, uv_scale)
    mo = np.zeros((h, w, 4), np.float32)
    orc.call("ComputeRobustnessMask", ref, mov, mo, Tex(uv), w, h, w * 12, w * 16, 1e-4, 1e-6, THRESHOLD_M)
    return mo


def robustness_seed(orc, w, h, uv_scale):
    """The first seed from 61 at which the ORACLE's M (mask channel 3) is nowhere within 1e-5 of thresholdM, so that the
    s = 1.5 / 0 decision cannot differ between two correct implementations and every cell can be compared."""
    for seed in range(61, 161):
        mo = robustness_oracle(orc, seed, w, h, uv_scale)
        if np.abs(mo[1:-1, 1:-1, 3] - THRESHOLD_M).min(initial=1.0) > 1e-5:
            return seed, mo
    raise AssertionError(f"no seed for {w}x{h} uv_scale {uv_scale}")


@case("ComputeRobustnessMask", shp=ROBUST_SHAPES)
def c_robustness(orc, hip, w, h, first):
    ref, mov, uv = robustness_inputs(60, w, h)

    def build(P):
        a, pa = P.inp(ref)
        b, _ = P.inp(mov)
        m, pm = P.out(np.zeros((h, w, 4), np.float32))
        return (a, b, m, P.tex(uv), w, h, pa, pm, 1e-4, 1e-6, THRESHOLD_M), [m]
    (o,), (g,) = both(orc, hip, "ComputeRobustnessMask", build)
    same(o, g, dict(atol=1e-6, rtol=1e-6), f"ComputeRobustnessMask {w}x{h}")
    assert (g[0] == 0).all() and (g[:, -1] == 0).all()


@case("robustnessMaskFused", shp=ROBUST_FUSED_SHAPES)
def c_robustnessFused(orc, hip, w, h, first):
    for uv_scale in (1, 2):
        seed, mo = robustness_seed(orc, w, h, uv_scale)
        assert np.abs(mo[1:-1, 1:-1, 3] - THRESHOLD_M).min(initial=1.0) > 1e-5
        ref, mov, uv = robustness_inputs(seed, w, h, uv_scale)
        P = Padded()
        a, pa = P.inp(ref)
        b, _ = P.inp(mov)
        m, pm = P.out(np.full((h, w, 4), 99.0, np.float32))
        hip.call("robustnessMaskFused", a, b, m, P.tex(uv), w, h, pa, pm, 1e-4, 1e-6, THRESHOLD_M)
        mh = P.get(m)
        assert (mh[0] == 0).all() and (mh[-1] == 0).all() and (mh[:, 0] == 0).all() and (mh[:, -1] == 0).all()
        assert ((mo[..., 3] > THRESHOLD_M) == (mh[..., 3] > THRESHOLD_M)).all(), f"threshold decisions {w}x{h} uv_scale {uv_scale}"
        same(mo, mh, dict(atol=1e-5, rtol=2e-6), f"robustnessMaskFused {w}x{h} uv_scale {uv_scale} seed {seed}")


# ---------------------------------------------------------------- finish
def _weights(seed, h, w):
    r = rng(seed)
    fin = r.random((h, w, 3), dtype=np.float32) * 4
    wt = r.random((h, w, 3), dtype=np.float32) * 4
    flat = wt.reshape(-1, 3)
    flat[0:3] = 0
    flat[3:6] = -1          # w + 1 == 0 -> output 0
    flat[6:9] = 1e-4        # below the threshold -> fallback blended in
    return fin, wt


@case("ApplyWeighting", "GammasRGB")
def c_weighting(orc, hip, w, h, first):
    fin, wt = _weights(61, h, w)
    r0 = rng(62).random((h, w, 3), dtype=np.float32)

    def build(P):
        io, p = P.out(r0)
        a, pa = P.inp(fin)
        b, pb = P.inp(wt)
        assert p == pa == pb
        return (io, a, b, w, h, p, 1e-3), [io]
    (o,), (g,) = both(orc, hip, "ApplyWeighting", build)
    same(o, g, None, f"ApplyWeighting {w}x{h}")
    g0 = (o * 1.2 - 0.1).astype(np.float32)
    g0[0, 0] = np.nan

    def build_g(P):
        io, p = P.out(g0)
        return (io, w, h, p), [io]
    (og,), (hg,) = both(orc, hip, "GammasRGB", build_g)
    same(og, hg, dict(atol=3e-7, rtol=3e-7), f"GammasRGB {w}x{h}")
    assert hg[0, 0, 0] == 0.0


def _finish_oracle(orc, fb, fin, wt, w, h, win, gamma):
    fh, fw = fb.shape[:2]
    io = np.zeros((h, w, 3), np.float32)
    orc.call("resampleFloat3", fb, fw * 12, fw, fh, io, w * 12, w, h, *win)
    orc.call("ApplyWeighting", io, fin, wt, w, h, w * 12, 1e-3)
    if gamma:
        orc.call("GammasRGB", io, w, h, w * 12)
    q = np.zeros((h, w, 3), np.uint16)
    orc.call("quantize", io, w * 12, q, None, w, h, 65535.0)
    return io, q


@case("finishFused")
def c_finishFused(orc, hip, w, h, first):
    fin, wt = _weights(63, h, w)
    fb = rng(64).random((h // 2 + 1, w // 2 + 1, 3), dtype=np.float32)
    win = (0.0, 1.0, 0.0, 1.0)
    for gamma in (1, 0):
        want, q = _finish_oracle(orc, fb, fin, wt, w, h, win, gamma)
        for with16 in (True, False):
            P = Padded()
            a, pa = P.inp(fin)
            b, _ = P.inp(wt)
            f, pf = P.inp(fb)
            o, po = P.out(np.zeros((h, w, 3), np.float32))
            q2 = np.zeros((h, w, 3), np.uint16) if with16 else None         # dense by contract
            hip.call("finishFused", a, b, pa, f, pf, fb.shape[1], fb.shape[0], *win, o, po, q2, w, h, 1e-3, gamma, 65535.0)
            same(want, P.get(o), dict(atol=3e-7, rtol=3e-7) if gamma else None, f"finishFused gamma={gamma} out16={with16} {w}x{h}")
            if with16:
                assert np.abs(q2.astype(np.int32) - q.astype(np.int32)).max() <= (1 if gamma else 0), f"finishFused out16 {w}x{h}"


# ---------------------------------------------------------------- accumulate
WHITE, BLACK = F3([3839, 3700, 3900]), F3([256, 260, 250])


def _fields(seed, fh, fw):
    kp = _kernel_field(seed, fh, fw, 4)
    sh = rng(seed + 1).uniform(-4, 4, (fh, fw, 2)).astype(np.float32)
    sh[1, 1] = 1e9
    sh[2, 2] = np.nan
    return kp, sh


@case("accumulateImages", shp=shapes(64, 4, 3, 3))
def c_accumulateImages(orc, hip, w, h, first):
    set_cfa(orc, hip, RGGB)
    raw, imgOut, tw, mask = _accum_inputs(9, w, h, w, h, nan_frac=0.05)
    kp = rng(10).uniform(0.05, 3.0, (h, w, 3)).astype(np.float32)
    kp[..., 2] = rng(12).uniform(-0.2, 0.2, (h, w))
    kp[1, 1] = [-50, -50, 0]
    sh = rng(11).uniform(-3, 3, (h, w, 2)).astype(np.float32)
    sh[1, 1] = [1e9, np.nan]

    def build(P):
        i, p = P.out(imgOut)
        t, _ = P.out(tw)
        m, pm = P.inp(mask)
        k, pk = P.inp(kp)                # read with imgOut's pitch (the reference's quirk)
        s, ps = P.inp(sh)
        assert pk == p
        return (raw, i, t, m, k, s, F3([3839] * 3), F3([256] * 3), w, h, p, pm, ps), [i, t]
    (oi, ow), (hi, hw_) = both(orc, hip, "accumulateImages", build)
    same(oi, hi, dict(rtol=2e-6, atol=2e-6), f"accumulateImages {w}x{h}")
    same(ow, hw_, dict(rtol=2e-6, atol=2e-6), f"accumulateImages weights {w}x{h}")


def _accumulate_case(orc, hip, fname, w, h, s, mode, tol, align):
    hip.L.set_accumulate_fast_exp(mode)
    try:
        raw, imgOut, tw, mask = _accum_inputs(6 + s, w, h, w * s, h * s, nan_frac=0.01)
        kp, sh = _fields(7, h // 2, w // 2)

        def build(P):
            i, p = P.out(imgOut, align)
            t, _ = P.out(tw, align)
            m, pm = P.inp(mask)
            args = (raw, i, t, m, P.tex(kp), P.tex(sh), WHITE, BLACK, w, h) + ((s,) if fname == "accumulateSuperResFull" else ()) + (p, pm)
            return args, [i, t]
        (oi, ow), (hi, hw_) = both(orc, hip, fname, build)
    finally:
        hip.L.set_accumulate_fast_exp(2)
    same(oi, hi, tol, f"{fname} x{s} mode {mode} {w}x{h}")
    same(ow, hw_, tol, f"{fname} weights x{s} mode {mode} {w}x{h}")


@case("accumulateImagesSuperRes", shp=shapes(64, 4, 8, 8))
def c_accumulateCrop(orc, hip, w, h, first):
    set_cfa(orc, hip, RGGB)
    _accumulate_case(orc, hip, "accumulateImagesSuperRes", w, h, 1, 0, dict(rtol=2e-6, atol=2e-6), None)


# (scale, LR width, LR height): 8x8 the minimum and an odd dimX (generic kernel); 32x32 the smallest the x2 strip / tile launcher
# and the x4 tile launcher take (a 16-pixel margin ring around a 32x32 live area at x2); an even size not divisible by 4; one
# full 256-pixel HR tile plus a partial one (150 x2, 70 x4)
ACCUMULATE = [(1, 8, 8), (1, 9, 11), (1, 66, 10), (3, 8, 8), (3, 9, 11), (3, 22, 10),
              (2, 8, 8), (2, 33, 32), (2, 32, 32), (2, 38, 34), (2, 150, 32),
              (4, 8, 8), (4, 32, 32), (4, 70, 34)]


@case("accumulateSuperResFull", shp=ACCUMULATE)
def c_accumulateFull(orc, hip, s, w, h, first):
    set_cfa(orc, hip, PATTERNS["GRBG"])
    # the straight kernel with the library's expf: test_accumulateSuperResFull's bound
    _accumulate_case(orc, hip, "accumulateSuperResFull", w, h, s, 0, dict(rtol=2e-6, atol=2e-6), None)
    if s in (2, 4):
        # the default mode; the strip / tile launchers need 16-byte accumulator pitches, so the padding is 16 here
        # (test_accumulate_x2_strip_kernel's / test_accumulate_x4_tile_kernel's bound)
        _accumulate_case(orc, hip, "accumulateSuperResFull", w, h, s, 2, dict(rtol=3e-5, atol=3e-5), 16)


# ---------------------------------------------------------------- direct device buffers (pointer-array entry points, stripes)
class DevBufs:
    def __init__(self, hip):
        self.hip, self.items = hip, []

    def up(self, buf, readonly=False):
        t, chk = guarded_upload(buf, self.hip.dev)
        self.items.append((buf, t, chk, readonly))
        return t.data_ptr()

    def finish(self, what):
        self.hip.torch.cuda.synchronize()
        for i, (buf, t, chk, ro) in enumerate(self.items):
            chk(f"{what}, buffer {i}", unchanged=ro)
            if not ro:
                buf.reshape(-1).view(np.uint8)[...] = t.cpu().numpy().reshape(-1).view(np.uint8)


def _pad2d(a, fill, align=None, rows_around=0, pitch=None):
    """-> (byte buffer [rows_around + H + rows_around, pitch], pitch, row bytes): ``a`` with padded rows, ``fill`` elsewhere.
    ``pitch``: a caller's own padded pitch (tests/test_lk_sweep_gpu.py: three different ones) instead of ``padded_pitch``'s."""
    a = np.ascontiguousarray(a)
    rowb = a.strides[0]
    if pitch is None:
        pitch = padded_pitch(rowb, align or texel_align(a))
    assert pitch > rowb
    buf = np.full((a.shape[0] + 2 * rows_around, pitch), fill, np.uint8)
    buf[rows_around:rows_around + a.shape[0], :rowb] = a.view(np.uint8).reshape(a.shape[0], rowb)
    return buf, pitch, rowb


@case("erodeMaskBatch", shp=shapes(64, 16, 3, 3, (131, 35)))           # ER_TX x ER_TY tiles, width and height >= 3
def c_erode(orc, hip, w, h, first):
    from tests.ghost_ref import erode_ref
    for r in (1, 2):
        n = 2
        masks = []
        for k in range(n):
            g = rng(80 + k)
            m = g.random((h, w, 4), dtype=np.float32)
            m[..., :3] = np.where(m[..., :3] < 0.2, 0.0, np.where(m[..., :3] > 0.7, 1.0, m[..., :3]))   # exact 0 / 1 plateaus
            m[0], m[-1], m[:, 0], m[:, -1] = 0, 0, 0, 0              # the ring as stage F leaves it
            m[..., 3] = g.standard_normal((h, w), dtype=np.float32) * 3
            masks.append(m)
        D = DevBufs(hip)
        ins = [_pad2d(m, POISON) for m in masks]
        outs = [_pad2d(np.full((h, w, 4), 7.0, np.float32), SENTINEL) for _ in masks]
        P = ctypes.c_void_p * n
        ip = P(*[D.up(b, True) for b, _, _ in ins])
        op = P(*[D.up(b) for b, _, _ in outs])
        hip.L.erodeMaskBatch(n, ip, op, w, h, ins[0][1], outs[0][1], r, None)
        D.finish("mfsr_erodeMaskBatch")
        for k in range(n):
            buf, pitch, rowb = outs[k]
            assert (buf[:, rowb:] == SENTINEL).all(), "pitch padding of an output changed"
            got = buf[:, :rowb].copy().view(np.float32).reshape(h, w, 4)
            same(erode_ref(masks[k], r), got, None, f"erodeMaskBatch r={r} frame {k} {w}x{h}")


# ---------------------------------------------------------------- raw-domain kernels, against their numpy restatements
I4 = ctypes.c_int32 * 4
# even sizes (whole Bayer quads): the smallest, the 64-lane / 256-thread boundaries of the launches in both directions, an odd
# number of quads
RAW_EVEN = [(2, 2), (62, 2), (64, 4), (66, 6), (126, 8), (128, 10), (130, 14), (258, 6), (262, 22)]
# measurements need a half-resolution rectangle inside the one-quad ring: 6 x 6 is the smallest frame; bands are 8 quad rows
RAW_RECT = [(6, 6), (62, 14), (64, 16), (66, 18), (126, 30), (128, 32), (130, 34), (262, 22)]


def _raw_frames(seed, n, w, h):
    g = rng(seed)
    return [g.integers(0, 65536, size=(h, w), dtype=np.uint16) for _ in range(n)]


def _raw_up(D, frames, fill, readonly):
    """-> (pointer array, pitch, [(buffer, row bytes)]) of u16 frames with padded rows on the device."""
    bufs = [_pad2d(f, fill, 2) for f in frames]
    P = ctypes.c_void_p * len(frames)
    return P(*[D.up(b, readonly) for b, _, _ in bufs]), bufs[0][1], [(b, rb) for b, _, rb in bufs]


def _raw_get(buf, rowb, shape):
    assert (buf[:, rowb:] == SENTINEL).all(), "pitch padding of a frame changed"
    return buf[:, :rowb].copy().view(np.uint16).reshape(shape)


def _rects(w, h):
    hw, hh = w // 2, h // 2
    return sorted({(1, 1, hw - 1, hh - 1), (1, 1, 2, 2), (hw - 2, hh - 2, hw - 1, hh - 1), (min(3, hw - 2), 1, hw - 1, hh - 1)})


UNPACK = [(4, 1), (12, 3), (16, 4), (20, 5), (252, 15), (256, 16), (260, 17), (132, 11)]   # 16 samples a lane, 256 lanes a block


@case("unpackRaw", shp=UNPACK)
def c_unpackRaw(orc, hip, w, h, first):
    from tests import packed_ref as R
    n = 2
    for packing in R.ALL:
        want = rng(7 + packing).integers(0, 1 << R.BITS[packing], (n, h, w)).astype(np.uint16)
        rb = padded_pitch(R.dense_row_bytes(packing, w), 1)
        D = DevBufs(hip)
        P = ctypes.c_void_p * n
        srcs = [np.ascontiguousarray(R.pack_ref(want[k], packing, rb, fill=POISON)).reshape(h, rb) for k in range(n)]
        ins = P(*[D.up(b, True) for b in srcs])
        outs, pitch, bufs = _raw_up(D, [np.zeros((h, w), np.uint16)] * n, SENTINEL, False)
        hip.L.unpackRaw(n, ins, rb, packing, outs, pitch, w, h, None)
        D.finish(f"mfsr_unpackRaw packing {packing} {w}x{h}")
        for k in range(n):
            np.testing.assert_array_equal(_raw_get(*bufs[k], (h, w)), want[k], err_msg=f"unpackRaw packing {packing} frame {k} {w}x{h}")


@case("frameLevels", shp=RAW_RECT)
def c_frameLevels(orc, hip, w, h, first):
    from tests.test_exposure_cpu import BLACK, SAT, measure
    n = 3
    host = _raw_frames(300 + w, n, w, h)
    host[1][: h // 2] = 65535                           # saturated quads
    for rect in _rects(w, h):
        D = DevBufs(hip)
        ptrs, pitch, _ = _raw_up(D, host, POISON, True)
        out = np.full((n, 5), -3, np.int64)
        po = D.up(out)
        hip.L.frameLevels(n, ptrs, pitch, w, h, I4(*BLACK), SAT, I4(*rect), po, None)
        D.finish(f"mfsr_frameLevels {w}x{h} rect {rect}")
        want = np.array([measure(f, rect, BLACK, SAT) for f in host], np.int64)
        np.testing.assert_array_equal(out, want, err_msg=f"frameLevels {w}x{h} rect {rect}")


@case("applyGains", shp=RAW_EVEN)
def c_applyGains(orc, hip, w, h, first):
    from tests.test_exposure_cpu import BLACK, MAXV, PHASES, RGGB as E_RGGB, SAT, apply_rule
    n = 3
    host = _raw_frames(310 + w, n, w, h)
    g = rng(w * 3 + h)
    for cfa, mono in ([(p, False) for p in PHASES] if first else [(PHASES[1], False)]) + [(E_RGGB, True)]:
        gains = [[int(v) for v in g.integers(4096, 1048577, size=3)] for _ in range(n)]
        status = [0, 2, 0]                              # a frame with status != 0 is left alone
        D = DevBufs(hip)
        ptrs, pitch, bufs = _raw_up(D, host, SENTINEL, False)
        hip.L.applyGains(n, ptrs, pitch, w, h, I4(*cfa), 1 if mono else 0, I4(*BLACK), SAT, MAXV,
                         (ctypes.c_int32 * (3 * n))(*[v for row in gains for v in row]), (ctypes.c_int32 * n)(*status), None)
        D.finish(f"mfsr_applyGains {w}x{h}")
        for k, f in enumerate(host):
            want = apply_rule(f, gains[k], cfa, mono, BLACK, SAT, MAXV) if status[k] == 0 else f
            np.testing.assert_array_equal(_raw_get(*bufs[k], (h, w)), want, err_msg=f"applyGains {w}x{h} frame {k} cfa {cfa} mono {mono}")


@case("applyShading", shp=RAW_EVEN)
def c_applyShading(orc, hip, w, h, first):
    from tests.test_shading_cpu import BLACK, MAXV, apply_rule, grid
    n, k = 2, 3
    host = _raw_frames(320 + w, n, w, h)
    gw, gh = grid(w, h, k)
    gmap = rng(w + 3 * h + k).integers(4096, 1048577, size=(4, gh, gw)).astype(np.int32)
    D = DevBufs(hip)
    ptrs, pitch, bufs = _raw_up(D, host, SENTINEL, False)
    pm = D.up(gmap, True)
    hip.L.applyShading(n, ptrs, pitch, w, h, pm, 1 << k, I4(*BLACK), MAXV, None)
    D.finish(f"mfsr_applyShading {w}x{h}")
    for i, f in enumerate(host):
        np.testing.assert_array_equal(_raw_get(*bufs[i], (h, w)), apply_rule(f, gmap, k, BLACK, MAXV), err_msg=f"applyShading {w}x{h} frame {i}")


# strips of 4 * 62 = 248 output columns, bands of 8 rows; 5 x 5 is the smallest Bayer frame
DEFECT = [(5, 5), (247, 7), (248, 8), (249, 9), (63, 15), (65, 17), (131, 11)]


@case("detectDefects", "repairDefects", shp=DEFECT)
def c_defects(orc, hip, w, h, first):
    from tests.test_defect_cpu import detect, repair
    n = 5
    g = rng(w * 7 + h)
    base = g.integers(0, 65536, size=(h, w), dtype=np.uint16)
    host = []
    for _ in range(n):
        a = g.integers(0, 65536, size=(h, w), dtype=np.uint16)
        keep = g.random((h, w)) < 0.5                   # half the pixels shared: many collect a majority of votes
        a[keep] = base[keep]
        host.append(a)
    for mono, thr, spread, votes in ((False, 59, 2, 3), (True, 0, 0, 3)):
        d = 1 if mono else 2
        want = detect(host, d, thr, spread, votes)
        D = DevBufs(hip)
        ptrs, pitch, _ = _raw_up(D, host, POISON, True)
        bm, pm, rowb = _pad2d(np.full((h, w), 0xAB, np.uint8), SENTINEL, 1)
        counts = np.full(2, 77, np.int32)
        hip.L.detectDefects(n, ptrs, pitch, w, h, 1 if mono else 0, thr, spread, votes, D.up(bm), pm, D.up(counts), None)
        D.finish(f"mfsr_detectDefects {w}x{h} mono {mono}")
        assert (bm[:, rowb:] == SENTINEL).all(), "pitch padding of the map changed"
        np.testing.assert_array_equal(bm[:, :rowb], want, err_msg=f"detectDefects {w}x{h} mono {mono}")
        assert tuple(counts) == (int((want == 1).sum()), int((want == 2).sum()))
        D = DevBufs(hip)
        ptrs, pitch, bufs = _raw_up(D, host, SENTINEL, False)
        bm, pm, _ = _pad2d(want.astype(np.uint8), POISON, 1)
        hip.L.repairDefects(n, ptrs, pitch, w, h, 1 if mono else 0, D.up(bm, True), pm, None)
        D.finish(f"mfsr_repairDefects {w}x{h} mono {mono}")
        for k, a in enumerate(host):
            np.testing.assert_array_equal(_raw_get(*bufs[k], (h, w)), repair(a, want, d), err_msg=f"repairDefects {w}x{h} frame {k} mono {mono}")


def sharpness_ref(raw, cfa, mono, rect):
    """The score of include/mfsr.h in numpy int64 (as tests/test_select_gpu.py::np_score): Sobel energy of the two greens' sum."""
    r = raw.astype(np.int64)
    greens = [(0, 1), (1, 0)] if mono else [(i >> 1, i & 1) for i in range(4) if cfa[i] == 1]
    (ay, ax), (by, bx) = greens
    G = r[ay::2, ax::2] + r[by::2, bx::2]
    x0, y0, x1, y1 = rect
    P = G[y0 - 1:y1 + 1, x0 - 1:x1 + 1]
    gx = (P[:-2, 2:] + 2 * P[1:-1, 2:] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[1:-1, :-2] + P[2:, :-2])
    gy = (P[2:, :-2] + 2 * P[2:, 1:-1] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[:-2, 1:-1] + P[:-2, 2:])
    return int((gx * gx + gy * gy).sum())


@case("frameSharpness", shp=RAW_RECT)
def c_frameSharpness(orc, hip, w, h, first):
    n = 3
    host = _raw_frames(330 + w, n, w, h)
    cfas = [(list(p), False) for p in PATTERNS.values()] if first else [(PATTERNS["GRBG"], False)]
    for cfa, mono in cfas + [(RGGB, True)]:
        for rect in _rects(w, h):
            D = DevBufs(hip)
            ptrs, pitch, _ = _raw_up(D, host, POISON, True)
            out = np.full(n, -3, np.int64)
            hip.L.frameSharpness(n, ptrs, pitch, w, h, I4(*cfa), 1 if mono else 0, I4(*rect), D.up(out), None)
            D.finish(f"mfsr_frameSharpness {w}x{h} rect {rect}")
            want = [sharpness_ref(f, cfa, mono, rect) for f in host]
            assert out.tolist() == want, f"frameSharpness {w}x{h} cfa {cfa} mono {mono} rect {rect}"


# ---------------------------------------------------------------- the sweep
@pytest.mark.parametrize("name", list(CASES))
def test_edge_shapes(orc, hip, name):
    fn, shp = CASES[name]
    for i, s in enumerate(shp):
        fn(orc, hip, *s, i == 0)


# ---------------------------------------------------------------- C: row stripes
def _stripes(hrH):
    last = hrH // 16 * 16 if hrH % 16 else hrH - 16
    return [(0, 16), (16, last), (last, hrH)]


CANARY = np.float32(-123.25)


@pytest.mark.parametrize("s,w,h", [(2, 64, 44), (4, 32, 34), (3, 24, 15)])      # x2 tile path, x4 tile path, generic
def test_accumulateSuperResFullRows(hip, s, w, h):
    """Rows of the stripe equal the whole-frame mfsr_accumulateSuperResFullN call bit for bit; every other byte -- the rows
    outside the stripe, two canary rows above and below the accumulators, the pitch padding -- is left alone.  HR heights
    that are no multiple of 16, accumulatorsUndefined 0 and 1, one and four frames."""
    hip.set_cfa(PATTERNS["RGGB"])
    hip.L.set_accumulate_fast_exp(2)              # the default mode: the strip / tile launchers where the geometry is theirs
    hrW, hrH = w * s, h * s
    assert hrH % 16
    fh, fw = h // 2, w // 2
    kp = _kernel_field(170, fh, fw, 4)
    yy, xx = np.mgrid[0:fh, 0:fw].astype(np.float32)
    allframes = []
    for k in range(4):
        raw, _, _, mask = _accum_inputs(171 + k, w, h, hrW, hrH, nan_frac=0.01)
        sh = np.stack([1.3 - 0.9 * k + 0.01 * xx, -2.2 + 1.1 * k + 0.02 * yy], -1).astype(np.float32)
        if k == 0:
            sh[1:3, 1:3] = 1e9
        if k == 3:
            sh[3, 3] = np.nan
        allframes.append((raw, mask, np.ascontiguousarray(sh)))
    acc0 = np.full((hrH, hrW, 3), CANARY, np.float32)
    align = 16 if s in (2, 4) else None           # the tile launchers need 16-byte accumulator pitches

    def call(n, fresh, r0, r1):
        D = DevBufs(hip)
        bi, pitch, rowb = _pad2d(acc0, SENTINEL, align, rows_around=2)
        bw, _, _ = _pad2d(acc0, SENTINEL, align, rows_around=2)
        start = bi.copy()
        pi, pw = D.up(bi) + 2 * pitch, D.up(bw) + 2 * pitch
        P, T = ctypes.c_void_p * n, hip.capi.Tex2D * n
        raws = P(*[D.up(f[0], True) for f in allframes[:n]])
        mk = [_pad2d(f[1], POISON) for f in allframes[:n]]
        masks = P(*[D.up(b, True) for b, _, _ in mk])
        fl = [_pad2d(f[2], POISON) for f in allframes[:n]]
        shs = T(*[hip.capi.Tex2D(D.up(b, True), p, fw, fh) for b, p, _ in fl])
        bk, pk, _ = _pad2d(kp, POISON)
        tk = hip.capi.Tex2D(D.up(bk, True), pk, fw, fh)
        hip.L.accumulateSuperResFullRows(n, raws, pi, pw, masks, tk, shs, hip.capi.f3(WHITE.v), hip.capi.f3(BLACK.v), w, h, s, pitch,
                                         mk[0][1], fresh, r0, r1, None)
        D.finish(f"mfsr_accumulateSuperResFullRows x{s} n={n} fresh={fresh} rows [{r0}, {r1})")
        return start, bi, bw, rowb

    for n in (1, 4):
        for fresh in (0, 1):
            start, wi, ww, rowb = call(n, fresh, 0, hrH)
            for b in (wi, ww):
                assert np.array_equal(b[:, rowb:], start[:, rowb:]) and np.array_equal(b[:2], start[:2]) and np.array_equal(b[-2:], start[-2:]), \
                    f"whole frame x{s} n={n} fresh={fresh}: bytes outside the image changed"
            assert not np.array_equal(wi[2:-2, :rowb], start[2:-2, :rowb])
            for r0, r1 in _stripes(hrH):
                _, gi, gw, _ = call(n, fresh, r0, r1)
                for got, whole, nm in ((gi, wi, "imgOut"), (gw, ww, "totalWeights")):
                    want = start.copy()
                    want[2 + r0:2 + r1, :rowb] = whole[2 + r0:2 + r1, :rowb]
                    bad = np.argwhere(got != want)
                    assert bad.size == 0, (f"x{s} n={n} fresh={fresh} rows [{r0}, {r1}) {nm}: first difference at buffer row "
                                           f"{bad[0][0] - 2}, byte {bad[0][1]} of the row ({rowb} row bytes)")


def test_finishFusedRows(hip):
    """outImg and out16 of each stripe equal those rows of mfsr_finishFused bit for bit, with a fallback image and a fallback
    window that is not the unit square; rows outside the stripe keep the canary."""
    w, h = 70, 45
    fin, wt = _weights(90, h, w)
    fb = rng(91).random((13, 17, 3), dtype=np.float32)
    win = (0.1, 0.9, 0.2, 0.7)
    canary = np.full((h, w, 3), CANARY, np.float32)

    def call(r0, r1):
        D = DevBufs(hip)
        bf, pf, _ = _pad2d(fin, POISON)
        bw, _, _ = _pad2d(wt, POISON)
        bb, pb, _ = _pad2d(fb, POISON)
        bo, po, rowb = _pad2d(canary, SENTINEL, rows_around=1)
        q = np.full((h + 2, w, 3), 0xC3C3, np.uint16)
        a, b, f, o, q16 = D.up(bf, True), D.up(bw, True), D.up(bb, True), D.up(bo), D.up(q)
        hip.L.finishFusedRows(a + r0 * pf, b + r0 * pf, pf, f, pb, 17, 13, *win, o + (1 + r0) * po, po, q16 + (1 + r0) * w * 6, w, r1 - r0,
                              1e-3, 1, 65535.0, r0, h, None)
        D.finish(f"mfsr_finishFusedRows rows [{r0}, {r1})")
        return bo, q, rowb

    D = DevBufs(hip)
    bf, pf, _ = _pad2d(fin, POISON)
    bw, _, _ = _pad2d(wt, POISON)
    bb, pb, _ = _pad2d(fb, POISON)
    wo, po, rowb = _pad2d(canary, SENTINEL, rows_around=1)
    wq = np.full((h + 2, w, 3), 0xC3C3, np.uint16)
    hip.L.finishFused(D.up(bf, True), D.up(bw, True), pf, D.up(bb, True), pb, 17, 13, *win, D.up(wo) + po, po, D.up(wq) + w * 6, w, h,
                      1e-3, 1, 65535.0, None)
    D.finish("mfsr_finishFused")
    blank_o, _, _ = _pad2d(canary, SENTINEL, rows_around=1)
    blank_q = np.full((h + 2, w, 3), 0xC3C3, np.uint16)
    assert not np.array_equal(wo[1:-1, :rowb], blank_o[1:-1, :rowb]) and np.array_equal(wo[:, rowb:], blank_o[:, rowb:])
    for r0, r1 in _stripes(h):
        go, gq, _ = call(r0, r1)
        want_o, want_q = blank_o.copy(), blank_q.copy()
        want_o[1 + r0:1 + r1, :rowb] = wo[1 + r0:1 + r1, :rowb]
        want_q[1 + r0:1 + r1] = wq[1 + r0:1 + r1]
        assert np.array_equal(go, want_o), f"outImg rows [{r0}, {r1})"
        assert np.array_equal(gq, want_q), f"out16 rows [{r0}, {r1})"


def test_finishFusedWindow(hip):
    """outImg and out16 of a 70 x 22 launch at (colOffset, rowOffset) = (6, 10) of a 96 x 48 frame equal that rectangle of
    mfsr_finishFused on the whole frame bit for bit, with and without the gamma: a 48 x 24 fallback, a third of the pixels with
    weights under the threshold (they take the resample at the full frame's coordinate), one weight of exactly zero inside the
    window.  The launch is neither a multiple of the 64 x 4 block nor aligned to it; bytes around its outputs keep the canary."""
    W, H, x0, y0, w, h = 96, 48, 6, 10, 70, 22
    g = rng(92)
    fin = g.random((H, W, 3), dtype=np.float32) * 4
    wt = 0.5 + g.random((H, W, 3), dtype=np.float32) * 4
    low = (np.add.outer(np.arange(H), np.arange(W)) % 3) == 0
    wt[low] = np.array([5e-4, 2e-4, 0.7], np.float32)
    wt[y0 + 5, x0 + 9] = 0
    inside = low[y0:y0 + h, x0:x0 + w]
    assert 0.3 < inside.mean() < 0.37 and (wt[y0:y0 + h, x0:x0 + w] == 0).any()
    fb = g.random((24, 48, 3), dtype=np.float32)
    bf, pf, _ = _pad2d(fin, POISON)
    bw, _, _ = _pad2d(wt, POISON)
    bb, pb, _ = _pad2d(fb, POISON)
    for gamma in (0, 1):
        D = DevBufs(hip)
        wo, po, _ = _pad2d(np.full((H, W, 3), CANARY, np.float32), SENTINEL)
        wq = np.full((H, W, 3), 0xC3C3, np.uint16)
        hip.L.finishFused(D.up(bf, True), D.up(bw, True), pf, D.up(bb, True), pb, 48, 24, 0.0, 1.0, 0.0, 1.0, D.up(wo), po, D.up(wq), W, H,
                          1e-3, gamma, 65535.0, None)
        D.finish("mfsr_finishFused")
        D = DevBufs(hip)
        go, gpo, rowb = _pad2d(np.full((h, w, 3), CANARY, np.float32), SENTINEL, rows_around=1)
        want_o = go.copy()
        gq = np.full((h + 2, w, 3), 0xC3C3, np.uint16)
        off = y0 * pf + 12 * x0
        hip.L.finishFusedWindow(D.up(bf, True) + off, D.up(bw, True) + off, pf, D.up(bb, True), pb, 48, 24, 0.0, 1.0, 0.0, 1.0,
                                D.up(go) + gpo, gpo, D.up(gq) + w * 6, w, h, 1e-3, gamma, 65535.0, x0, y0, W, H, None)
        D.finish("mfsr_finishFusedWindow")
        want_o[1:-1, :rowb] = wo[y0:y0 + h, 12 * x0:12 * (x0 + w)]
        want_q = np.full((h + 2, w, 3), 0xC3C3, np.uint16)
        want_q[1:-1] = wq[y0:y0 + h, x0:x0 + w]
        assert not np.array_equal(wq, np.full_like(wq, 0xC3C3))
        assert np.array_equal(go, want_o), f"outImg, gamma {gamma}"
        assert np.array_equal(gq, want_q), f"out16, gamma {gamma}"


def test_ComputeDerivatives2Rows(hip):
    """Rows [row0, row0 + rows) equal those rows of mfsr_ComputeDerivatives2Kernel bit for bit (MIRROR addressing at both
    ends: row0 = 0 and the last rows); all other rows keep the canary."""
    w, h = 67, 23
    img = _smooth_image(95, h, w)
    P = Padded()
    wx, p = P.out(np.zeros((h, w), np.float32))
    wy, _ = P.out(np.zeros((h, w), np.float32))
    hip.call("ComputeDerivatives2Kernel", w, h, p, wx, wy, P.tex(img))
    wx, wy = P.get(wx), P.get(wy)
    assert np.abs(wx).max() > 0
    for row0, rows in ((0, 1), (0, 4), (3, 5), (8, 9), (h - 3, 3), (h - 1, 1), (0, h)):
        P = Padded()
        gx, p = P.out(np.full((h, w), CANARY, np.float32))
        gy, _ = P.out(np.full((h, w), CANARY, np.float32))
        hip.call("ComputeDerivatives2Rows", w, h, p, gx, gy, P.tex(img), row0, rows)
        for got, whole, nm in ((P.get(gx), wx, "Ix"), (P.get(gy), wy, "Iy")):
            want = np.full((h, w), CANARY, np.float32)
            want[row0:row0 + rows] = whole[row0:row0 + rows]
            assert_bitexact(want, got, f"{nm} rows [{row0}, {row0 + rows})")


def _flow_case(hip, vy, bound, flag0, max0):
    """-> (flag, maxBits) of the two entry points on the field whose .y is ``vy``, padded rows holding huge values."""
    rows, width = vy.shape
    fl = np.zeros((rows, width, 2), np.float32)
    fl[..., 0] = 3e38                      # .x never counts
    fl[..., 1] = vy
    rowb = width * 8
    pitch = padded_pitch(rowb, 8)
    buf = np.empty((rows, pitch), np.uint8)
    buf[...] = np.frombuffer(np.float32(3e38).tobytes() * (pitch // 4), np.uint8)     # huge values in the padding: must NOT count
    buf[:, :rowb] = fl.view(np.uint8).reshape(rows, rowb)
    buf.flags.writeable = False
    flag, mx = np.array([flag0], np.int32), np.array([max0], np.int32)
    hip.call("checkFlowBound", buf, pitch, width, rows, float(bound), flag)
    hip.call("maxAbsFlowY", buf, pitch, width, rows, mx)
    return int(flag[0]), int(mx[0])


def _flow_expect(vy, bound, flag0, max0):
    a = np.abs(vy[~np.isnan(vy)])
    flag = flag0 | int(bool((a > np.float32(bound)).any()))
    m = int(a.max().view(np.int32)) if a.size and a.max() > 0 else 0
    return flag, max(max0, m)


@pytest.mark.parametrize("width", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 259])
def test_checkFlowBound_and_maxAbsFlowY(hip, width, rows):
    """flag |= any(|v| > bound) and maxBits = max(maxBits, bits of max |v|), NaN ignored, against numpy; 259 rows make the
    grid-stride loop of mfsr_maxAbsFlowY run more than once per thread."""
    bound = 2.5
    base = rng(97).uniform(-2.0, 2.0, (rows, width)).astype(np.float32)
    last_partial = width - 1               # the last column is the last active lane of the row's last, partial wavefront
    cases = [("quiet", base)]
    for nm, (y, x) in (("first", (0, 0)), ("last", (rows - 1, width - 1)), ("last lane of a partial wavefront", (rows // 2, last_partial))):
        v = base.copy()
        v[y, x] = -7.75
        cases.append((f"offender at the {nm}", v))
    v = base.copy()
    v[rows - 1, width - 1] = bound
    v[0, 0] = -bound
    cases.append(("exactly the bound", v))
    cases.append(("-0.0", np.full((rows, width), -0.0, np.float32)))
    v = base.copy()
    v[rows // 2, width // 2] = -np.inf
    cases.append(("-inf", v))
    cases.append(("all NaN", np.full((rows, width), np.nan, np.float32)))
    v = base.copy()
    v[0, 0] = np.nan
    cases.append(("one NaN", v))
    for nm, vy in cases:
        for flag0, max0 in ((0, 0), (1, int(np.float32(5.0).view(np.int32))), (0, int(np.float32(0.5).view(np.int32)))):
            got = _flow_case(hip, vy, bound, flag0, max0)
            want = _flow_expect(vy, bound, flag0, max0)
            assert got == want, f"{nm}, {width}x{rows}, preset ({flag0}, {max0:#x}): (flag, maxBits) = {got}, expected {want}"
    assert _flow_expect(cases[1][1], bound, 0, 0)[0] == 1 and _flow_expect(cases[4][1], bound, 0, 0)[0] == 0
    assert _flow_expect(cases[6][1], bound, 0, 0) == (1, int(np.float32(np.inf).view(np.int32)))
    assert _flow_expect(cases[7][1], bound, 0, 7) == (0, 7)


ROW_STRIPE_TESTS = {
    "mfsr_accumulateSuperResFullRows": "test_accumulateSuperResFullRows",
    "mfsr_finishFusedRows": "test_finishFusedRows",
    "mfsr_finishFusedWindow": "test_finishFusedWindow",
    "mfsr_ComputeDerivatives2Rows": "test_ComputeDerivatives2Rows",
    "mfsr_checkFlowBound": "test_checkFlowBound_and_maxAbsFlowY",
    "mfsr_maxAbsFlowY": "test_checkFlowBound_and_maxAbsFlowY",
}
