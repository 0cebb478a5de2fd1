"""Launch-edge shapes for the finish family: the entry points of include/mfsr.h that name their rows ``...RowBytes``.

The same rule as tests/test_kernel_edges_gpu.py, whose ``shapes`` and ``padded_pitch`` this module uses; tests/test_kernel_edges_cpu.py
checks ``SWEEP`` against the header.  Per entry point:

  * shapes: the smallest, tile - 1 / tile / tile + 1 in x crossed with the same in y, one odd size of a few tiles, and 255 / 256 /
    257 columns where an RGB8 lane owns four pixels.  The tile comes from the entry's ``mfsr_*_tile`` query where it has one, else
    from the ``dim3 block`` of its launch site (named next to the table);
  * the reference is the numpy restatement the entry's own test file uses (render_ref, yuv_ref, sharpen_ref, denoise_ref,
    local_tone_ref, chain_ref, geometry_ref, image_stats_ref), bit for bit: uint32 views of floats, bytes of the integer outputs,
    statistics words exactly.  A finish form is compared with the restatement of the float image mfsr_finishFusedWindow writes of
    the same accumulators (tests/test_kernel_edges_gpu.py compares that entry with the oracle);
  * inputs sit on rows padded by ``padded_pitch`` and filled with 0xFF, between the guards of ``guarded_upload``, and are checked
    unchanged; outputs sit on padded rows filled with a sentinel, the integer output at the odd byte offset its format allows;
  * at every shape every format the entry stores, with matrix + table and without; at the smallest shape, at (tile + 1, tile + 1)
    and at the odd shape also under MFSR_RENDER_LUT=lds and =cache, so that every compiled <FORMAT, LDS> instantiation runs on a
    tile that is partial in both axes; at the odd shape once with the float output alone and once with the integers alone;
  * the hostile values of the entry's own test file (NaN, +-1e30, negatives, values above 65536, weights of zero and on both sides
    of the threshold; inf where that file has it); the finishes with a place in a full frame run at (colOffset, rowOffset) = (5, 3).
"""
import ctypes

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi
from tests import chain_ref as C
from tests import denoise_ref as D
from tests import geometry_ref as G
from tests import image_stats_ref as IS
from tests import local_tone_ref as LT
from tests import render_ref as R
from tests import sharpen_ref as S
from tests import yuv_ref as Y
from tests.kernels import guarded_upload
from tests.test_kernel_edges_gpu import POISON, SENTINEL, padded_pitch, shapes

pytestmark = pytest.mark.gpu

f32 = np.float32
SINGLE = (R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2)
TWO_PLANE = (Y.NV12, Y.P010)
NAMES = {R.RGB16: "RGB16", R.RGB8: "RGB8", R.RGBA8: "RGBA8", R.RGB10A2: "RGB10A2", Y.NV12: "NV12", Y.P010: "P010"}
COLOUR = {Y.NV12: Y.BT709, Y.P010: Y.BT2020 | Y.FULL}
CCM = np.array([1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56], f32)
LUT = R.srgb_lut(4096)            # at most 8192 intervals: lut_in_lds takes it
OFFSET, PAD = (5, 3), (4, 4)      # a finish's place in its full frame, and what the frame has beyond it
THR = 1e-3


def _tile(name):
    """(tileW, tileH[, stageW, stageH]) of mfsr_<name>_tile"""
    n = 4 if name == "geometry" else 2
    v = [ctypes.c_int(0) for _ in range(n)]
    assert capi.lib().raw[f"mfsr_{name}_tile"](*(ctypes.byref(x) for x in v)) == 0
    return tuple(x.value for x in v)


# render.hip, local_tone.hip: dim3 block(64, lds ? 16 : 4), an RGB8 lane owns four pixels.  render_yuv.hip: dim3 block(64, lds ? 16 : 4)
# over quads of columns and pairs of rows: 256 x 8 (x 32) pixels.  image_stats.hip, local_tone.hip (statistics): 1024 lanes of
# four pixels a round and no 2-D block: 256 x 16 = one round, with rows of 255 / 257 pixels ending in a partial quad.
RGB8_COLUMNS = [(255, 3), (256, 4), (257, 5)]
RENDER = shapes(64, 4, odd=(131, 19)) + RGB8_COLUMNS
YUV = [(2, 2)] + [(w, h) for h in (6, 8, 10) for w in (254, 256, 258)] + [(130, 34)]
STATS = shapes(256, 16, odd=(131, 35))


def _stencil(name):
    tw, th = _tile(name)[:2]
    return shapes(tw, th, odd=(131, 35)) + [(4 * tw - 1, th - 1), (4 * tw, th), (4 * tw + 1, th + 1)]


def _even(name):
    """the two-plane formats: even sizes around the tile"""
    tw, th = _tile(name)[:2]
    return [(2, 2)] + [(tw + dx, th + dy) for dy in (-2, 0, 2) for dx in (-2, 0, 2)] + [(130, 34)]


SWEEP = {}        # entry point -> name of the case that covers it
CASES = {}        # case name -> (function, shapes)


def case(*entries, shp):
    def deco(fn):
        CASES[fn.__name__] = (fn, shp)
        for e in entries:
            SWEEP["mfsr_" + e] = fn.__name__
        return fn
    return deco


def extra_forms(shp, w, h):
    """the shapes that also run under MFSR_RENDER_LUT=lds and =cache: the smallest, the first with tile + 1 in both axes (the
    ninth of ``shapes``; the last of the 3 x 3 block of the even lists) and the odd one"""
    return (w, h) in (shp[0], shp[9], shp[10])


# ---------------------------------------------------------------- placement
class Inputs:
    """float3 images on padded rows of 0xFF bytes between guards; ``unchanged`` checks them all"""

    def __init__(self):
        self.checks = []

    def up(self, a, align=4):
        a = np.ascontiguousarray(a, f32)
        rowb = a.strides[0]
        pitch = padded_pitch(rowb, align)
        buf = np.full((a.shape[0], pitch), POISON, np.uint8)
        buf[:, :rowb] = a.view(np.uint8).reshape(a.shape[0], rowb)
        d, chk = guarded_upload(buf)
        self.checks.append(chk)
        return d.data_ptr(), pitch

    def dense(self, a):
        d, chk = guarded_upload(a)
        self.checks.append(chk)
        return d

    def unchanged(self, what):
        for chk in self.checks:
            chk(what, unchanged=True)


def _place(fmt, w):
    """(offset, row bytes) of an integer plane: the odd offset the format's stores allow, padded rows"""
    if fmt == R.RGB8:
        return 1, padded_pitch(3 * w, 1)
    if fmt == R.RGB16:
        return 2, padded_pitch(6 * w, 2)
    if fmt == Y.NV12:
        return 1, padded_pitch(w, 1)
    if fmt == Y.P010:
        return 2, padded_pitch(2 * w, 2)
    return 4, padded_pitch(4 * w, 4)


class Plane:
    """an output of `rows` rows between guards: `off` sentinel bytes, then rows `rb` bytes apart of which `dense` bytes may be written"""

    def __init__(self, rows, dense, off, rb):
        self.rows, self.dense, self.off, self.rb = rows, dense, off, rb
        self.dev, self.check = guarded_upload(np.full(off + rb * rows, SENTINEL, np.uint8))
        self.ptr = self.dev.data_ptr() + off

    def expect(self, want, what):
        """want: [rows, dense] bytes, or None = untouched"""
        self.check(what)
        full = np.full(self.off + self.rb * self.rows, SENTINEL, np.uint8)
        if want is not None:
            full[self.off:].reshape(self.rows, self.rb)[:, :self.dense] = want
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != full)
        first = int(bad[0]) - self.off if bad.size else 0
        assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first at byte {first} of the plane "
                               f"(row {first // self.rb}, byte {first % self.rb} of {self.dense} + padding)")


def _bytes(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def _render(fmt, rendered, lut_dev):
    r = capi.Render()
    r.format = fmt
    r.reserved[0] = COLOUR.get(fmt, 0)
    if rendered:
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*[float(v) for v in CCM])
        r.toneLut = lut_dev.data_ptr()
        r.toneSize = lut_dev.numel() - 1
    return r


_lut = {}


def _lut_dev():
    if not _lut:
        _lut["dev"] = torch.from_numpy(LUT).to("cuda:0")
    return _lut["dev"]


def run_forms(mp, what, w, h, formats, extra, launch, want_t, alone=False):
    """One launch per (format, matrix + table or neither, way of reading the table) of an entry that stores a float image and an
    integer output.  launch(render, float pointer, its row bytes, plane pointer, its row bytes, chroma pointer, its row bytes);
    want_t(m): the restatement's float image before the rendered output's steps (it may depend on the matrix: the local tone's
    luma key).  alone: also the float image alone and the integers alone."""
    lut_dev = _lut_dev()
    runs = 0
    for fmt in formats:
        two = fmt in TWO_PLANE
        for rendered in (False, True):
            m, lut = (CCM, LUT) if rendered else (None, None)
            t = want_t(m)
            if two:
                want_f, want_y, want_uv = Y.render(t, fmt, m, lut, False, COLOUR[fmt])
                want_q, want_c = _bytes(want_y), _bytes(want_uv)
            else:
                want_f, want_q = R.render(t, fmt, m, lut)
                want_q, want_c = R.as_bytes(want_q), None
            outs = [(True, True)] + ([(True, False), (False, True)] if alone and rendered else [])
            hows = [None] + (["lds", "cache"] if extra and rendered else [])
            for how in hows:
                if how:
                    mp.setenv("MFSR_RENDER_LUT", how)
                else:
                    mp.delenv("MFSR_RENDER_LUT", raising=False)
                for with_f, with_q in (outs if how is None else outs[:1]):
                    off, rb = _place(fmt, w)
                    pf = Plane(h, 12 * w, 0, padded_pitch(12 * w, 4))
                    pq = Plane(h, want_q.shape[1], off, rb)
                    pc = Plane(h // 2, want_c.shape[1], off, rb) if two else None
                    launch(_render(fmt, rendered, lut_dev), pf.ptr if with_f else None, pf.rb, pq.ptr if with_q else None, rb,
                           pc.ptr if two and with_q else None, rb if two else 0)
                    tag = f"{what} {NAMES[fmt]} {w}x{h} rendered={rendered} lut={how} float={with_f} integers={with_q}"
                    pf.expect(_bytes(want_f.reshape(h, 3 * w)) if with_f else None, tag + " (float image)")
                    pq.expect(want_q if with_q else None, tag)
                    if two:
                        pc.expect(want_c if with_q else None, tag + " (chroma plane)")
                    runs += 1
    mp.delenv("MFSR_RENDER_LUT", raising=False)
    return runs


def _cached(store, key, make):
    if key not in store:
        store[key] = make()
    return store[key]


_wants = {}


# ---------------------------------------------------------------- inputs
def _render_pixels(h, w, seed, inf=True):
    """tests/test_render_gpu.py::_pixels (inf=False: tests/test_sharpen_gpu.py's, which leaves +-inf out because inf - inf makes a
    NaN whose sign is the hardware's choice)"""
    from tests.test_render_gpu import _pixels as with_inf
    from tests.test_sharpen_gpu import _pixels as without
    return with_inf(h, w, seed) if inf else without(h, w, seed)


def _denoise_pixels(h, w):
    from tests.test_denoise_gpu import _counts, _pixels
    return _pixels(h, w, 100 * w + h), _counts(h, w, 7 * w + h)


def _accumulators(w, h):
    """tests/test_denoise_gpu.py::_accumulators of a w x h rectangle with a fallback of half the full frame: weights of 0, just
    below and just above the threshold, ordinary and large"""
    from tests.test_denoise_gpu import _accumulators as make
    fw, fh = w + OFFSET[0] + PAD[0], h + OFFSET[1] + PAD[1]
    fbw, fbh = fw // 2 + 1, fh // 2 + 1
    fin, wt, fb = make(w, h, fbw, fbh, THR)
    wt.reshape(-1, 3)[0] = [0.0, 5e-4, 0.7]          # (the smallest shapes too have a weight of zero and one under the threshold)
    return fin, wt, fb, (fw, fh), (fbw, fbh)


class Finish:
    """accumulators, weights (one pitch) and a fallback on padded rows, the arguments every finish entry begins with, and the
    float image mfsr_finishFusedWindow writes of them at the same place in the full frame"""

    def __init__(self, w, h, place=True, hostile=False):
        self.w, self.h = w, h
        fin, wt, fb, full, (fbw, fbh) = _accumulators(w, h)
        if hostile and fin.size > 40:
            fin.reshape(-1)[7::41] = np.nan
            wt.reshape(-1)[11::53] = np.nan
        self.wt = wt
        self.offset, self.full = (OFFSET, full) if place else ((0, 0), (w, h))
        self.I = Inputs()
        (pa, pitch), (pw, pitch_w), (pb, pitch_b) = self.I.up(fin), self.I.up(wt), self.I.up(fb)
        assert pitch == pitch_w
        self.head = (pa, pw, pitch, pb, pitch_b, fbw, fbh, 0.0, 1.0, 0.0, 1.0)
        self.where = (self.offset[0], self.offset[1], self.full[0], self.full[1])
        d_lin, chk = guarded_upload(np.zeros((h, w, 3), f32))
        capi.lib().finishFusedWindow(*self.head, d_lin.data_ptr(), 12 * w, None, w, h, THR, 0, 65535.0, *self.where, None)
        chk("plain finish")
        self.lin = d_lin.cpu().numpy()


# ---------------------------------------------------------------- the rendered finish
@case("renderImage", shp=RENDER)
def c_renderImage(mp, w, h):
    L = capi.lib()
    p = _render_pixels(h, w, 100 * w + h)
    I = Inputs()
    d_in, pi = I.up(p)
    n = run_forms(mp, "renderImage", w, h, SINGLE, extra_forms(RENDER, w, h),
                  lambda r, f, pf, q, rb, c, rc: L.renderImage(d_in, pi, f, pf, q, rb, w, h, ctypes.byref(r), 0, None),
                  lambda m: p, alone=(w, h) == RENDER[10])
    I.unchanged(f"renderImage {w}x{h}")
    assert n >= 8


@case("finishRendered", shp=RENDER)
def c_finishRendered(mp, w, h):
    L = capi.lib()
    F = Finish(w, h)
    run_forms(mp, "finishRendered", w, h, SINGLE, extra_forms(RENDER, w, h),
              lambda r, f, pf, q, rb, c, rc: L.finishRendered(*F.head, f, pf, q, rb, ctypes.byref(r), w, h, THR, 0, *F.where, None),
              lambda m: F.lin, alone=(w, h) == RENDER[10])
    F.I.unchanged(f"finishRendered {w}x{h}")


@case("renderImageYuv", shp=YUV)
def c_renderImageYuv(mp, w, h):
    L = capi.lib()
    p = _render_pixels(h, w, 100 * w + h)
    I = Inputs()
    d_in, pi = I.up(p)
    run_forms(mp, "renderImageYuv", w, h, TWO_PLANE, extra_forms(YUV, w, h),
              lambda r, f, pf, q, rb, c, rc: L.renderImageYuv(d_in, pi, f, pf, q, rb, c, rc, w, h, ctypes.byref(r), 0, None),
              lambda m: p, alone=(w, h) == YUV[10])
    I.unchanged(f"renderImageYuv {w}x{h}")


@case("finishRenderedYuv", shp=YUV)
def c_finishRenderedYuv(mp, w, h):
    L = capi.lib()
    F = Finish(w, h)
    run_forms(mp, "finishRenderedYuv", w, h, TWO_PLANE, extra_forms(YUV, w, h),
              lambda r, f, pf, q, rb, c, rc: L.finishRenderedYuv(*F.head, f, pf, q, rb, c, rc, ctypes.byref(r), w, h, THR, 0, *F.where, None),
              lambda m: F.lin, alone=(w, h) == YUV[10])
    F.I.unchanged(f"finishRenderedYuv {w}x{h}")


# ---------------------------------------------------------------- sharpen: radius 1 (0 is refused: "call the plain entry") and 4
SHARPEN = _stencil("sharpen")


def _sharpen(taps, amount, threshold):
    s = capi.Sharpen()
    s.radius = len(taps) - 1
    for d, k in enumerate(taps):
        s.taps[d] = float(k)
    s.amount, s.threshold = amount, threshold
    return s


def _sharpen_taps():
    from tests.test_sharpen_gpu import TAPS
    return [TAPS["odd", 1], TAPS["gauss", 4]]


@case("sharpenImage", shp=SHARPEN)
def c_sharpenImage(mp, w, h):
    L = capi.lib()
    p = _render_pixels(h, w, 100 * w + h, inf=False)
    I = Inputs()
    d_in, pi = I.up(p)
    off, nothing = _sharpen([1.0], 1.5, 0.01), Plane(h, 12 * w, 0, padded_pitch(12 * w, 4))
    assert L.raw["mfsr_sharpenImage"](d_in, pi, nothing.ptr, nothing.rb, None, 0, w, h, ctypes.byref(off), None, 0, None) != 0     # radius 0
    nothing.expect(None, "sharpenImage with radius 0")
    for taps in _sharpen_taps():
        s = _sharpen(taps, 1.5, 0.01)
        run_forms(mp, f"sharpenImage R={len(taps) - 1}", w, h, SINGLE, extra_forms(SHARPEN, w, h),
                  lambda r, f, pf, q, rb, c, rc: L.sharpenImage(d_in, pi, f, pf, q, rb, w, h, ctypes.byref(s), ctypes.byref(r), 0, None),
                  lambda m: _cached(_wants, ("sharpen", w, h, len(taps)), lambda: S.sharpen(p, taps, 1.5, 0.01)),
                  alone=(w, h) == SHARPEN[10])
    I.unchanged(f"sharpenImage {w}x{h}")


@case("finishSharpened", shp=SHARPEN)
def c_finishSharpened(mp, w, h):
    L = capi.lib()
    F = Finish(w, h)
    for taps in _sharpen_taps():
        s = _sharpen(taps, 1.25, 0.005)
        run_forms(mp, f"finishSharpened R={len(taps) - 1}", w, h, SINGLE, extra_forms(SHARPEN, w, h),
                  lambda r, f, pf, q, rb, c, rc: L.finishSharpened(*F.head, f, pf, q, rb, ctypes.byref(r), w, h, THR, 0, *F.where,
                                                                    ctypes.byref(s), 0, 0, None),
                  lambda m: _cached(_wants, ("finishSharpened", w, h, len(taps)), lambda: S.sharpen(F.lin, taps, 1.25, 0.005)),
                  alone=(w, h) == SHARPEN[10])
    F.I.unchanged(f"finishSharpened {w}x{h}")


# ---------------------------------------------------------------- denoise: radius 1 (0 is refused) and 3
DENOISE = _stencil("denoise")
DEN = dict(strength=3.0, gain=4.0, alpha=0.05, beta=0.01)
DEN_FINISH = dict(strength=3.0, gain=4.0, alpha=0.02, beta=0.002)


def _denoise(radius, strength, gain, alpha, beta):
    d = capi.Denoise()
    d.radius, d.strength, d.gain, d.alpha, d.beta = radius, strength, gain, alpha, beta
    return d


@case("denoiseImage", shp=DENOISE)
def c_denoiseImage(mp, w, h):
    L = capi.lib()
    p, n = _denoise_pixels(h, w)
    I = Inputs()
    (d_in, pi), (d_cnt, pc) = I.up(p), I.up(n)
    off, nothing = _denoise(0, **DEN), Plane(h, 12 * w, 0, padded_pitch(12 * w, 4))
    refused = L.raw["mfsr_denoiseImage"](d_in, pi, d_cnt, pc, nothing.ptr, nothing.rb, None, 0, w, h, ctypes.byref(off), None, 0, None)
    assert refused != 0                                                                                              # radius 0
    nothing.expect(None, "denoiseImage with radius 0")
    for radius in (1, 3):
        d = _denoise(radius, **DEN)
        run_forms(mp, f"denoiseImage R={radius}", w, h, SINGLE, extra_forms(DENOISE, w, h),
                  lambda r, f, pf, q, rb, c, rc: L.denoiseImage(d_in, pi, d_cnt, pc, f, pf, q, rb, w, h, ctypes.byref(d), ctypes.byref(r), 0,
                                                                 None),
                  lambda m: _cached(_wants, ("denoise", w, h, radius), lambda: D.denoise(p, n, radius=radius, **DEN)),
                  alone=(w, h) == DENOISE[10])
    I.unchanged(f"denoiseImage {w}x{h}")


@case("finishDenoised", shp=DENOISE)
def c_finishDenoised(mp, w, h):
    L = capi.lib()
    F = Finish(w, h)
    n = D.count_of_weight(F.wt, THR)
    for radius in (1, 3):
        d = _denoise(radius, **DEN_FINISH)
        run_forms(mp, f"finishDenoised R={radius}", w, h, SINGLE, extra_forms(DENOISE, w, h),
                  lambda r, f, pf, q, rb, c, rc: L.finishDenoised(*F.head, f, pf, q, rb, ctypes.byref(r), w, h, THR, 0, *F.where,
                                                                   ctypes.byref(d), 0, 0, None),
                  lambda m: _cached(_wants, ("finishDenoised", w, h, radius), lambda: D.denoise(F.lin, n, radius=radius, **DEN_FINISH)),
                  alone=(w, h) == DENOISE[10])
    F.I.unchanged(f"finishDenoised {w}x{h}")


# ---------------------------------------------------------------- statistics
def _stats_params(m, tol):
    p = capi.ImageStatsParams()
    p.lo, p.hi, p.chromaTol = 64, 3967, tol
    if m is not None:
        p.useMatrix = 1
        p.matrix = (ctypes.c_float * 9)(*[float(v) for v in m])
    return p


def _table(shape, launch, want, what):
    d_t, chk = guarded_upload(np.zeros(shape, np.int64))
    launch(d_t.data_ptr())
    chk(what)
    got = d_t.cpu().numpy().view(np.uint64)
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:6]}"


@case("imageStats", "finishStats", shp=STATS)
def c_imageStats(mp, w, h):
    L = capi.lib()
    p = _render_pixels(h, w, 1000 * w + h)
    I = Inputs()
    d_in, pi = I.up(p)
    F = Finish(w, h)
    for m, tol in ((None, 0), (CCM, 64)):
        par = _stats_params(m, tol)
        _table(IS.WORDS, lambda t: L.imageStats(d_in, pi, w, h, ctypes.byref(par), t, None), IS.stats(p, m, 64, 3967, tol),
               f"imageStats {w}x{h} matrix={m is not None}")
        _table(IS.WORDS, lambda t: L.finishStats(*F.head, w, h, THR, *F.where, ctypes.byref(par), t, None), IS.stats(F.lin, m, 64, 3967, tol),
               f"finishStats {w}x{h} matrix={m is not None}")
    I.unchanged(f"imageStats {w}x{h}")
    F.I.unchanged(f"finishStats {w}x{h}")


def _lt(cell, bins):
    lt = capi.LocalTone()
    lt.cell, lt.bins, lt.smooth, lt.shadows, lt.highlights, lt.pivot, lt.maxGain = cell, bins, 1, 0.5, 0.25, 0.0, 4.0
    return lt


def _m9(m):
    return None if m is None else (ctypes.c_float * 9)(*[float(v) for v in m])


@case("toneGridStats", "finishToneGridStats", shp=STATS)
def c_toneGridStats(mp, w, h):
    """C = 16: the rows 15 / 16 / 17 end below, on and over a row of cells, and (5, 3) puts every cell edge off the launch's"""
    L = capi.lib()
    p = _render_pixels(h, w, 1000 * w + h)
    I = Inputs()
    d_in, pi = I.up(p)
    F = Finish(w, h)
    for bins, m in ((4, None), (32, CCM)):
        lt = _lt(16, bins)
        want = LT.stats(p, 16, bins, m, F.offset, F.full)
        _table(want.shape, lambda t: L.toneGridStats(d_in, pi, w, h, *F.where, _m9(m), ctypes.byref(lt), t, None), want,
               f"toneGridStats {w}x{h} NZ={bins}")
        want = LT.stats(F.lin, 16, bins, m, F.offset, F.full)
        _table(want.shape, lambda t: L.finishToneGridStats(*F.head, w, h, THR, *F.where, _m9(m), ctypes.byref(lt), t, None), want,
               f"finishToneGridStats {w}x{h} NZ={bins}")
    I.unchanged(f"toneGridStats {w}x{h}")
    F.I.unchanged(f"finishToneGridStats {w}x{h}")


# ---------------------------------------------------------------- the local tone's slice
def _grid(full, bins=8, cell=16):
    gx, gy, gz = LT.grid_size(full[0], full[1], cell, bins)
    return np.random.default_rng(3).uniform(0.25, 4.0, (gy, gx, gz)).astype(f32)


def _slice_pixels(h, w):
    from tests.test_local_tone_gpu import _slice_pixels as make
    return make(h, w, 100 * w + h)


@case("localToneImage", shp=RENDER)
def c_localToneImage(mp, w, h):
    L = capi.lib()
    p = _slice_pixels(h, w)
    full = (w + OFFSET[0] + PAD[0], h + OFFSET[1] + PAD[1])
    grid, lt = _grid(full), _lt(16, 8)
    I = Inputs()
    d_in, pi = I.up(p)
    d_grid = I.dense(grid)
    run_forms(mp, "localToneImage", w, h, SINGLE, extra_forms(RENDER, w, h),
              lambda r, f, pf, q, rb, c, rc: L.localToneImage(d_in, pi, f, pf, q, rb, w, h, ctypes.byref(r), 0, d_grid.data_ptr(),
                                                               ctypes.byref(lt), *OFFSET, *full, None),
              lambda m: _cached(_wants, ("tone", w, h, m is not None), lambda: LT.apply(p, grid, 16, m, OFFSET)),
              alone=(w, h) == RENDER[10])
    I.unchanged(f"localToneImage {w}x{h}")


@case("finishLocalTone", shp=RENDER)
def c_finishLocalTone(mp, w, h):
    L = capi.lib()
    F = Finish(w, h)
    grid, lt = _grid(F.full), _lt(16, 8)
    d_grid = F.I.dense(grid)
    run_forms(mp, "finishLocalTone", w, h, SINGLE, extra_forms(RENDER, w, h),
              lambda r, f, pf, q, rb, c, rc: L.finishLocalTone(*F.head, f, pf, q, rb, ctypes.byref(r), w, h, THR, 0, *F.where,
                                                                d_grid.data_ptr(), ctypes.byref(lt), None),
              lambda m: _cached(_wants, ("finishTone", w, h, m is not None), lambda: LT.apply(F.lin, grid, 16, m, F.offset)),
              alone=(w, h) == RENDER[10])
    F.I.unchanged(f"finishLocalTone {w}x{h}")


# ---------------------------------------------------------------- the chain: reach 0 (both stencils off, the local tone alone) and 3 + 4
CHAIN = _stencil("chain")
CHAIN_EVEN = _even("chain")
CHAIN_SETS = ("L", "DS34L")


def _chain(name, full):
    """(chain_ref's denoise, sharpen and local_tone descriptions, the C struct, the grid on the device)"""
    from tests.test_finish_chain_gpu import _cstruct, _den, _sharp, _tone
    den, sharp = (_den(3), _sharp(4)) if name == "DS34L" else (None, None)
    tone = _tone(*full)
    c, grid = _cstruct(den, sharp, tone)
    return den, sharp, tone, c, grid


def _chain_image(mp, w, h, formats, shp):
    L = capi.lib()
    p, n = _denoise_pixels(h, w)
    full = (w + OFFSET[0] + PAD[0], h + OFFSET[1] + PAD[1])
    I = Inputs()
    (d_in, pi), (d_cnt, pc) = I.up(p), I.up(n)
    for name in CHAIN_SETS:
        den, sharp, tone, c, grid = _chain(name, full)
        run_forms(mp, f"chainImage {name}", w, h, formats, extra_forms(shp, w, h),
                  lambda r, f, pf, q, rb, cp, rc: L.chainImage(d_in, pi, d_cnt, pc, f, pf, q, rb, cp, rc, w, h, ctypes.byref(r), 0,
                                                                ctypes.byref(c), grid.data_ptr(), *OFFSET, *full, None),
                  lambda m: _cached(_wants, ("chain", name, w, h, m is not None), lambda: C.chain(p, n, den, sharp, tone, m, OFFSET)),
                  alone=(w, h) == shp[10])
    I.unchanged(f"chainImage {w}x{h}")


def _finish_chain(mp, w, h, formats, shp):
    L = capi.lib()
    F = Finish(w, h)
    n = D.count_of_weight(F.wt, THR)
    for name in CHAIN_SETS:
        den, sharp, tone, c, grid = _chain(name, F.full)
        if den:
            den = dict(den, alpha=0.02, beta=0.002)
            c.denoise.alpha, c.denoise.beta = 0.02, 0.002
        run_forms(mp, f"finishChain {name}", w, h, formats, extra_forms(shp, w, h),
                  lambda r, f, pf, q, rb, cp, rc: L.finishChain(*F.head, f, pf, q, rb, cp, rc, ctypes.byref(r), w, h, THR, 0, *F.where,
                                                                 ctypes.byref(c), grid.data_ptr(), 0, 0, None),
                  lambda m: _cached(_wants, ("finishChain", name, w, h, m is not None),
                                    lambda: C.chain(F.lin, n, den, sharp, tone, m, F.offset)),
                  alone=(w, h) == shp[10])
    F.I.unchanged(f"finishChain {w}x{h}")


@case("chainImage", shp=CHAIN)
def c_chainImage(mp, w, h):
    _chain_image(mp, w, h, SINGLE, CHAIN)


@case(shp=CHAIN_EVEN)
def c_chainImage_two_plane(mp, w, h):
    _chain_image(mp, w, h, TWO_PLANE, CHAIN_EVEN)


@case("finishChain", shp=CHAIN)
def c_finishChain(mp, w, h):
    _finish_chain(mp, w, h, SINGLE, CHAIN)


@case(shp=CHAIN_EVEN)
def c_finishChain_two_plane(mp, w, h):
    _finish_chain(mp, w, h, TWO_PLANE, CHAIN_EVEN)


# ---------------------------------------------------------------- the geometric finish
GEOMETRY = _stencil("geometry")
FILTERS = {"bilinear": G.BILINEAR, "cubic": G.CUBIC}
# with distortion and a lateral scale the three channels have their own coordinates; without, one coordinate serves the three
LENS = {"lens": dict(distortion=(0.03, -0.005, 0.0), lateral=(1.004, 0.997)), "same": {}}


def geometry_case(w, h, mapping, filt):
    """(source width, source height, description, rectangle): the w x h rectangle at OFFSET of an output PAD larger, from a source
    of 1.25 times the output (a step of about 1.25)"""
    ow, oh = w + OFFSET[0] + PAD[0], h + OFFSET[1] + PAD[1]
    sw, sh = max(1, round(1.25 * ow)), max(1, round(1.25 * oh))
    return sw, sh, G.lens(sw, sh, ow, oh, filter=filt, **LENS[mapping]), (OFFSET[0], OFFSET[1], w, h)


def _geometry_struct(gd):
    from tests.test_geometry_cpu import _struct
    g = _struct(gd)
    assert capi.lib().raw["mfsr_geometry_validate"](ctypes.byref(g)) == 0
    return g


def _geometry_source(h, w):
    from tests.test_geometry_gpu import _source
    return _source(h, w, 100 * w + h)


@case("geometryImage", shp=GEOMETRY)
def c_geometryImage(mp, w, h):
    L = capi.lib()
    sw, sh = geometry_case(w, h, "same", G.CUBIC)[:2]
    p = _geometry_source(sh, sw)
    I = Inputs()
    d_in, pi = I.up(p)
    for mapping in LENS:
        for fname, filt in FILTERS.items():
            _, _, gd, rect = geometry_case(w, h, mapping, filt)
            g = _geometry_struct(gd)
            run_forms(mp, f"geometryImage {mapping} {fname}", w, h, SINGLE, extra_forms(GEOMETRY, w, h),
                      lambda r, f, pf, q, rb, c, rc: L.geometryImage(d_in, pi, sw, sh, f, pf, q, rb, ctypes.byref(r), ctypes.byref(g), 0, *rect,
                                                                      None),
                      lambda m: _cached(_wants, ("geometry", w, h, mapping, fname), lambda: G.resample(p, gd, rect)),
                      alone=(w, h) == GEOMETRY[10] and mapping == "lens")
    I.unchanged(f"geometryImage {w}x{h}")


@case("finishGeometry", shp=GEOMETRY)
def c_finishGeometry(mp, w, h):
    L = capi.lib()
    sw, sh = geometry_case(w, h, "same", G.CUBIC)[:2]
    F = Finish(sw, sh, place=False, hostile=True)
    for mapping in LENS:
        for fname, filt in FILTERS.items():
            _, _, gd, rect = geometry_case(w, h, mapping, filt)
            g = _geometry_struct(gd)
            run_forms(mp, f"finishGeometry {mapping} {fname}", w, h, SINGLE, extra_forms(GEOMETRY, w, h),
                      lambda r, f, pf, q, rb, c, rc: L.finishGeometry(*F.head, sw, sh, f, pf, q, rb, ctypes.byref(r), ctypes.byref(g), THR, 0,
                                                                       *rect, None),
                      lambda m: _cached(_wants, ("finishGeometry", w, h, mapping, fname), lambda: G.resample(F.lin, gd, rect)),
                      alone=(w, h) == GEOMETRY[10] and mapping == "lens")
    F.I.unchanged(f"finishGeometry {w}x{h}")


# ---------------------------------------------------------------- three batch entries outside the finish family
# Their own test files take sizes below, on and over their tiles, but not tile - 1 in both axes: the comparisons of those files
# (which take any size, on rows padded with a sentinel) run here at the sweep's shapes.
# debayer.hip: PREP_TX x PREP_TY tiles of the half-resolution frame
@case("prepareFrameMeansBatch", shp=shapes(64, 16, 3, 3, odd=(131, 35)))
def c_prepareFrameMeansBatch(mp, w, h):
    from tests.test_robustness_group_gpu import test_prepare_with_means_equals_prepare_and_numpy as compare
    compare(w, h)


@case("robustnessMaskGroup", shp=shapes(64, 8, 3, 3, odd=(131, 19)))           # robustness.hip: dim3 block(RB_TX, RB_TY)
def c_robustnessMaskGroup(mp, w, h):
    from tests.test_robustness_group_gpu import test_group_masks_equal_the_fused_batch as compare
    compare(w, h)


# noise_temporal.hip: one lane per 8 x 8 block of the frame, 64 lanes a wave (1024 a workgroup: 65536 pixels, beyond this sweep's
# sizes; tests/test_noise_temporal_gpu.py runs 264 x 136).  One block; 9 x 7 = 63, 8 x 8 = 64 and 13 x 5 = 65 blocks, the first and
# the last with a partial block beyond the grid at the right and at the bottom; an odd number of blocks either way
NOISE_TEMPORAL = [(8, 8), (74, 62), (64, 64), (110, 42), (142, 38)]


@case("noiseStatsTemporal", shp=NOISE_TEMPORAL)
def c_noiseStatsTemporal(mp, w, h):
    """tests/test_noise_temporal_gpu.py::test_translated_frames at this size: three frames under whole-quad translations, on dense
    and padded pitches, base pointers on the 16-byte grid and 2 bytes off it; the tables equal the restatement's"""
    from tests.test_noise_cpu import full_rect
    from tests.test_noise_temporal_gpu import _block_flow, _check, _const, _noise
    shifts = ((0, 0), (1, -1), (-3, 2))
    host = _noise(3, w, h, 30 + w)
    for mono in (False, True):
        flows = [_block_flow(w, h, mono, _const(w, h, *s)) for s in shifts]
        for pad, offset, fpad in ((0, 0, 0), (8, 8, 3), (3, 1, 1)):
            _check(host, flows, rects=(full_rect(w, h),), pad=pad, offset=offset, fpad=fpad, min_terms=0 if (w, h) == (8, 8) else 3)


# ---------------------------------------------------------------- the sweep
@pytest.mark.parametrize("name", list(CASES))
def test_finish_edge_shapes(name, monkeypatch):
    fn, shp = CASES[name]
    for s in shp:
        fn(monkeypatch, *s)
