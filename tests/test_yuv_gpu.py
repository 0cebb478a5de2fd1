"""Two-plane YUV 4:2:0 output on the device: k_renderImageYuv against the numpy restatement of
tests/yuv_ref.py, k_finishRenderedYuv against the two-launch chain, and NV12 / P010 bursts (resident, unfused, windowed, striped,
host, streamed) against the restatement applied to the plain float image of the same pipeline.  Everything is bit for bit; with
the built-in gamma (powf) the planes are compared with the restatement of the float image the same launch wrote."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi, synth
from tests import render_ref as R
from tests import yuv_ref as Y
from tests.kernels import guarded_upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CANARY = 0xA5
FORMATS = (Y.NV12, Y.P010)
NAMES = {Y.NV12: "NV12", Y.P010: "P010"}
CCM = np.array([1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56], np.float32)
LUTS = {"none": None, "srgb4096": R.srgb_lut(4096), "five": np.array([0.1, 0.9, -0.2, 1.3, 0.5], np.float32)}
# A workgroup owns 256 columns x 8 rows (table through the cache, or none) or x 32 rows (table staged in LDS): the widths
# 254 / 256 / 258 / 514 and these heights lie on both sides of every tile edge, besides the heights every width is run at.
WIDTHS = (2, 4, 6, 8, 10, 254, 256, 258, 514)
HEIGHTS = (2, 6, 18)
TILE_EDGE_SHAPES = ((258, 8), (258, 10), (258, 30), (258, 32), (258, 34), (514, 34), (10, 34))


def _struct(fmt, m=None, lut_dev=None, colour=0):
    r = capi.Render()
    r.format = fmt
    r.reserved[0] = colour
    if m is not None:
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*[float(v) for v in m])
    if lut_dev is not None:
        r.toneLut = lut_dev.data_ptr()
        r.toneSize = lut_dev.numel() - 1
    return r


def _pixels(h, w, seed):
    """random values around [0, 1] with NaN, +-inf, negatives, values above 1 (and above 65536 for the matrix) and exact
    knots k/4096 and k/4 of the two tables at fixed strides"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.25, 1.25, h * w * 3).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -3.0, 2.5, 70000.0, 300.0, 0.0, 1.0, 0.25, 0.5, 0.75, 1000 / 4096, 4095 / 4096,
                        1 / 4096, 0.0031308, 1e-8], np.float32)
    idx = np.arange(0, p.size, 5)
    p[idx] = special[np.arange(idx.size) % special.size]
    return p.reshape(h, w, 3)


def _plane_bytes(plane):
    a = np.ascontiguousarray(plane)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def _expected(plane, off, pitch):
    """the whole allocation of one plane: `off` canary bytes, then rows of `pitch` bytes of which the dense part is written"""
    dense = _plane_bytes(plane)
    want = np.full(off + pitch * dense.shape[0], CANARY, np.uint8)
    want[off:].reshape(dense.shape[0], pitch)[:, :dense.shape[1]] = dense
    return want


def _layouts(fmt, w):
    """(Y offset, Y pitch, UV offset, UV pitch)"""
    rb = Y.row_bytes(fmt, w)
    if fmt == Y.NV12:
        return [(0, rb, 0, rb), (1, rb + 5, 3, rb + 5)]
    return [(0, rb, 0, rb), (2, rb + 2, 2, rb + 2)]


def _canary_planes(h, yo, yp, uo, up):
    d_y, check_y = guarded_upload(np.full(yo + yp * h, CANARY, np.uint8))
    d_uv, check_uv = guarded_upload(np.full(uo + up * (h // 2), CANARY, np.uint8))
    return d_y, check_y, d_uv, check_uv


# ---- 1. the pixel body on its own -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_renderImageYuv_equals_the_restatement(fmt):
    L = capi.lib()
    luts = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in LUTS.items()}
    shapes = list(itertools.product(WIDTHS, HEIGHTS)) + list(TILE_EDGE_SHAPES)
    n = 0
    for w, h in shapes:
        p = _pixels(h, w, 100 * w + h)
        d_in, check_in = guarded_upload(p)
        combos = list(itertools.product((False, True), LUTS)) if w in (2, 6, 258) else [(True, "srgb4096")]
        colours = Y.COLOURS if w == 6 else (Y.BT709,)
        for (use_m, lut_name), colour in itertools.product(combos, colours):
            m = CCM if use_m else None
            want_f, want_y, want_uv = Y.render(p, fmt, m, LUTS[lut_name], colour=colour)
            r = _struct(fmt, m, luts[lut_name], colour)
            for yo, yp, uo, up in _layouts(fmt, w):
                d_y, check_y, d_uv, check_uv = _canary_planes(h, yo, yp, uo, up)
                d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
                L.renderImageYuv(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_y.data_ptr() + yo, yp, d_uv.data_ptr() + uo, up,
                                 w, h, ctypes.byref(r), 0, None)
                what = f"{NAMES[fmt]} {w}x{h} matrix={use_m} lut={lut_name} colour={colour} Y+{yo}/{yp} UV+{uo}/{up}"
                check_y(what)
                check_uv(what)
                check_f(what)
                assert np.array_equal(d_y.cpu().numpy(), _expected(want_y, yo, yp)), what + " (Y)"
                assert np.array_equal(d_uv.cpu().numpy(), _expected(want_uv, uo, up)), what + " (UV)"
                assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), what + " (float image)"
                n += 1
        check_in(f"{NAMES[fmt]} {w}x{h}", unchanged=True)
    assert n > 2 * len(shapes)


def test_renderImageYuv_in_place_and_without_planes():
    L = capi.lib()
    w, h, pitch = 66, 6, 12 * 66 + 8
    p = _pixels(h, w, 5)
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    rows = np.full((h, pitch), CANARY, np.uint8)
    rows[:, :12 * w] = p.view(np.uint8).reshape(h, 12 * w)
    for fmt, with_planes in itertools.product(FORMATS, (True, False)):
        want_f, want_y, want_uv = Y.render(p, fmt, CCM, LUTS["srgb4096"], colour=Y.BT601)
        r = _struct(fmt, CCM, lut, Y.BT601)
        rb = Y.row_bytes(fmt, w)
        d_img, check_img = guarded_upload(rows)
        d_y, check_y, d_uv, check_uv = _canary_planes(h, 0, rb, 0, rb)
        L.renderImageYuv(d_img.data_ptr(), pitch, d_img.data_ptr(), pitch, d_y.data_ptr() if with_planes else None, rb,
                         d_uv.data_ptr() if with_planes else None, rb, w, h, ctypes.byref(r), 0, None)
        for c in (check_img, check_y, check_uv):
            c("in place")
        got = d_img.cpu().numpy()
        assert np.array_equal(got[:, :12 * w].copy().view(np.uint32).reshape(h, w, 3), want_f.view(np.uint32))
        assert (got[:, 12 * w:] == CANARY).all()
        if with_planes:
            assert np.array_equal(d_y.cpu().numpy(), _expected(want_y, 0, rb))
            assert np.array_equal(d_uv.cpu().numpy(), _expected(want_uv, 0, rb))
        else:
            assert (d_y.cpu().numpy() == CANARY).all() and (d_uv.cpu().numpy() == CANARY).all()


@pytest.mark.parametrize("how", ["lds", "cache"])
def test_renderImageYuv_lut_in_lds_and_through_the_cache_give_the_same_bytes(monkeypatch, how):
    """MFSR_RENDER_LUT=lds | cache (read at every call) forces one way of reading the tone table; unset, the two-plane formats
    stage tables of up to 8192 intervals in LDS (64 x 16 workgroups), which is what every other test here runs.  Both give the
    restatement's bytes; a table too long for LDS (65536 intervals) is read through the cache either way."""
    L = capi.lib()
    w, h = 130, 38
    p = _pixels(h, w, 9)
    d_in, _ = guarded_upload(p)
    monkeypatch.setenv("MFSR_RENDER_LUT", how)
    for n, fmt in ((4096, Y.NV12), (4096, Y.P010), (4, Y.P010), (8192, Y.NV12), (65536, Y.NV12), (1, Y.P010)):
        table = R.srgb_lut(n)
        lut = torch.from_numpy(table).to(DEV)
        want_f, want_y, want_uv = Y.render(p, fmt, CCM, table)
        rb = Y.row_bytes(fmt, w)
        d_y, check_y, d_uv, check_uv = _canary_planes(h, 0, rb, 0, rb)
        d_f, check_f = guarded_upload(np.zeros((h, w, 3), np.float32))
        r = _struct(fmt, CCM, lut)
        L.renderImageYuv(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_y.data_ptr(), rb, d_uv.data_ptr(), rb, w, h,
                         ctypes.byref(r), 0, None)
        for c in (check_y, check_uv, check_f):
            c(f"{how} {n}")
        assert np.array_equal(d_y.cpu().numpy(), _expected(want_y, 0, rb)), (how, n)
        assert np.array_equal(d_uv.cpu().numpy(), _expected(want_uv, 0, rb)), (how, n)
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (how, n)


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_renderImageYuv_builtin_gamma(fmt):
    """applyGamma = 1 without a table: powf is the only inexact operation.  The planes are bit for bit the restatement of the
    float image the same launch wrote; that float image is within one LSB (of 8 or 10 bits) of numpy's pow, and equal on the
    linear segment."""
    L = capi.lib()
    w, h = 130, 6
    p = _pixels(h, w, 77)
    lin = p.reshape(-1)[1::5]
    lin[:] = np.random.default_rng(3).uniform(0, 0.0031308, lin.size).astype(np.float32)
    d_in, _ = guarded_upload(p)
    rb = Y.row_bytes(fmt, w)
    d_y, check_y, d_uv, check_uv = _canary_planes(h, 0, rb, 0, rb)
    d_f, check_f = guarded_upload(np.zeros((h, w, 3), np.float32))
    r = _struct(fmt, None, None, Y.BT2020)
    L.renderImageYuv(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_y.data_ptr(), rb, d_uv.data_ptr(), rb, w, h, ctypes.byref(r), 1,
                     None)
    for c in (check_y, check_uv, check_f):
        c("gamma")
    got_f = d_f.cpu().numpy()
    want_y, want_uv = Y.planes(got_f, fmt, Y.BT2020)
    assert np.array_equal(d_y.cpu().numpy(), _expected(want_y, 0, rb))
    assert np.array_equal(d_uv.cpu().numpy(), _expected(want_uv, 0, rb))
    lsb = R.RGB8 if fmt == Y.NV12 else R.RGB10A2
    diff = np.abs(R.quantise(got_f, lsb) - R.quantise(R.gamma(p), lsb))
    with np.errstate(invalid="ignore"):
        linear = ~(p > np.float32(0.0031308))
    print(f"{NAMES[fmt]}: float image max difference {diff.max()} LSB, {int((diff > 0).sum())} of {diff.size} samples differ")
    assert diff.max() <= 1
    assert diff[linear].max() == 0
    assert np.array_equal(got_f[linear].view(np.uint32), R.gamma(p)[linear].view(np.uint32))


# ---- 2. the fused kernel against the chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_fallback", [True, False], ids=["fallback", "no-fallback"])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_finishRenderedYuv_equals_the_chain(fmt, with_fallback):
    """mfsr_finishFusedWindow (float image, no gamma) + mfsr_renderImageYuv against the one launch: whole (130 x 38), the stripe
    of rows [10, 32) and the window (16, 16, 64 x 16).  Weights: the left 64 columns of rows 0..19 are all above the threshold,
    a checkerboard of sub-threshold weights elsewhere."""
    L = capi.lib()
    W, H, fbW, fbH, thr = 130, 38, 65, 19, 1e-3
    rng = np.random.default_rng(11)
    fin = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    wt = rng.uniform(0.5, 2, (H, W, 3)).astype(np.float32)
    low = ((np.add.outer(np.arange(H), np.arange(W)) % 3) == 0)
    low[:20, :64] = False
    wt[low] = np.array([0.0, 5e-4, 0.7], np.float32)
    fb = rng.uniform(0, 1, (fbH, fbW, 3)).astype(np.float32)
    d_fin, c1 = guarded_upload(fin)
    d_wt, c2 = guarded_upload(wt)
    d_fb, c3 = guarded_upload(fb)
    fb_ptr = d_fb.data_ptr() if with_fallback else None
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    colour = Y.BT601 | Y.FULL
    r = _struct(fmt, CCM, lut, colour)
    rb = Y.row_bytes(fmt, W)
    # the chain
    d_lin, _ = guarded_upload(np.zeros((H, W, 3), np.float32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, fb_ptr, 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * W, None, W, H, thr, 0, 65535.0, 0, 0, W, H, None)
    d_cf, _ = guarded_upload(np.zeros((H, W, 3), np.float32))
    d_cy, _, d_cuv, _ = _canary_planes(H, 0, rb, 0, rb)
    L.renderImageYuv(d_lin.data_ptr(), 12 * W, d_cf.data_ptr(), 12 * W, d_cy.data_ptr(), rb, d_cuv.data_ptr(), rb, W, H,
                     ctypes.byref(r), 0, None)
    chain_f = d_cf.cpu().numpy()
    chain_y, chain_uv = d_cy.cpu().numpy().reshape(H, rb), d_cuv.cpu().numpy().reshape(H // 2, rb)
    # the restatement agrees with the chain (so the comparison below is not of two equal mistakes)
    ref_f, ref_y, ref_uv = Y.render(d_lin.cpu().numpy(), fmt, CCM, LUTS["srgb4096"], colour=colour)
    assert np.array_equal(chain_f.view(np.uint32), ref_f.view(np.uint32))
    assert np.array_equal(chain_y, _plane_bytes(ref_y)) and np.array_equal(chain_uv, _plane_bytes(ref_uv))
    bps = rb // W

    def launch(x0, y0, w, h, what):
        wrb = Y.row_bytes(fmt, w)
        d_f, cf = guarded_upload(np.zeros((h, w, 3), np.float32))
        d_y, cy, d_uv, cuv = _canary_planes(h, 0, wrb, 0, wrb)
        o = 12 * (y0 * W + x0)
        L.finishRenderedYuv(d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * W, fb_ptr, 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                            d_f.data_ptr(), 12 * w, d_y.data_ptr(), wrb, d_uv.data_ptr(), wrb, ctypes.byref(r), w, h, thr, 0, x0, y0,
                            W, H, None)
        for c in (cf, cy, cuv):
            c(what)
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), chain_f[y0:y0 + h, x0:x0 + w].view(np.uint32)), what
        assert np.array_equal(d_y.cpu().numpy().reshape(h, wrb), chain_y[y0:y0 + h, bps * x0:bps * (x0 + w)]), what
        assert np.array_equal(d_uv.cpu().numpy().reshape(h // 2, wrb), chain_uv[y0 // 2:(y0 + h) // 2, bps * x0:bps * (x0 + w)]), what

    launch(0, 0, W, H, "whole")
    launch(0, 10, W, 22, "stripe")
    launch(16, 16, 64, 16, "window")
    for c in (c1, c2, c3):
        c("inputs", unchanged=True)


# ---- bursts -----------------------------------------------------------------------------------------------------------------
W, H, N = 384, 256, 7
_cache = {}
RENDER = dict(matrix=CCM, tone_lut=LUTS["srgb4096"])


def _frames(bits=12, seed=29):
    if ("frames", bits, seed) not in _cache:
        frames, _, _ = synth.make_burst(W, H, N, seed=seed, device="cpu")
        if bits == 10:
            frames = [(f.view(torch.int16).to(torch.int32) >> 2).to(torch.int16).view(f.dtype) for f in frames]
        _cache["frames", bits, seed] = [f.contiguous() for f in frames]
    return _cache["frames", bits, seed]


def _config(gamma=0, fused=1, ring=0, packing=0, bits=12, frames=N, reference=0):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, frames, scale=2)
    if bits == 10:
        for i in range(3):
            cfg.black[i], cfg.white[i] = 64.0, 1023.0 - 64.0
        cfg.maxVal = 1023.0
    cfg.applyGamma, cfg.fused, cfg.uploadRing, cfg.rawPacking, cfg.reference = gamma, fused, ring, packing, reference
    return cfg


def _np(t):
    """a flat output tensor as the restatement's words"""
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _plain_float(bits=12, fused=1):
    """the plain float image (applyGamma = 0) of the burst: computed once per configuration, shared and left unchanged"""
    key = ("plain", bits, fused)
    if key not in _cache:
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        pipe = BurstPipeline(_config(fused=fused, bits=bits), DEV)
        img, _ = pipe.process([f.to(DEV) for f in _frames(bits)])
        _cache[key] = img.cpu().numpy().copy()
        pipe.close()
    return _cache[key]


def _want(fmt, bits=12, fused=1):
    """(float image, Y, UV) the burst must give"""
    key = ("want", fmt, bits, fused)
    if key not in _cache:
        _cache[key] = Y.render(_plain_float(bits, fused), fmt, CCM, LUTS["srgb4096"], colour=Y.BT709)
    return _cache[key]


def _flat(y, uv):
    return np.concatenate([y.reshape(-1), uv.reshape(-1)])


@pytest.mark.parametrize("fused", [1, 0])
def test_yuv_burst_equals_the_restatement_of_the_plain_float_image(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, yuv_planes
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(fused=fused), DEV)
    for fmt in FORMATS:
        pipe.set_render(fmt, **RENDER)
        img, q = pipe.process(frames)
        want_f, want_y, want_uv = _want(fmt, fused=fused)
        assert q.dtype == (torch.uint8 if fmt == Y.NV12 else torch.int16) and tuple(q.shape) == (2 * H * 2 * W * 3 // 2,)
        y, uv = yuv_planes(q, fmt, 2 * H, 2 * W)
        assert np.array_equal(_np(y), want_y) and np.array_equal(_np(uv), want_uv), (NAMES[fmt], fused)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (NAMES[fmt], fused)
    # another colour description reaches the kernel through the setter
    pipe.set_render(Y.NV12, yuv=capi.YUV_BT601 | capi.YUV_FULL, **RENDER)
    _, q = pipe.process(frames)
    _, y601, uv601 = Y.render(_plain_float(fused=fused), Y.NV12, CCM, LUTS["srgb4096"], colour=Y.BT601 | Y.FULL)
    assert np.array_equal(_np(q), _flat(y601, uv601))
    # and off again: the plain burst's bits
    pipe.set_render(None)
    img, q16 = pipe.process(frames)
    assert q16.dtype == torch.int16 and tuple(q16.shape) == (2 * H, 2 * W, 3)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), _plain_float(fused=fused).view(np.uint32))
    assert np.array_equal(_np(q16), R.render(_plain_float(fused=fused), R.RGB16)[1])
    pipe.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_yuv_zoom_window_is_the_crop_of_both_planes(fmt):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, yuv_planes
    x, y, w, h = 242, 98, 154, 110          # even, not on the 16-pixel grid: the library works on the aligned window around it
    pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
    pw.set_render(fmt, **RENDER)
    img, q = pw.process([f.to(DEV) for f in _frames()])
    want_f, want_y, want_uv = _want(fmt)
    gy, guv = yuv_planes(q, fmt, h, w)
    assert np.array_equal(_np(gy), want_y[y:y + h, x:x + w])
    assert np.array_equal(_np(guv), want_uv[y // 2:(y + h) // 2, x // 2:(x + w) // 2])
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f[y:y + h, x:x + w].view(np.uint32))
    pw.close()
    odd = BurstPipeline(_config(), DEV, window=(243, 98, 154, 110))
    with pytest.raises(ValueError):
        odd.set_render(fmt, **RENDER)
    odd.close()


def test_yuv_finish_rows_fills_both_planes():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, yuv_planes
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    pipe.set_render(capi.OUT_NV12, **RENDER)
    pipe.out16.fill_(CANARY)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for k, f in enumerate(frames):
        pipe.add_frame(f, k == 0)
    _, want_y, want_uv = _want(Y.NV12)
    with pytest.raises(capi.MfsrError):
        pipe.finish_rows(171, 340)               # odd row0
    with pytest.raises(capi.MfsrError):
        pipe.finish_rows(170, 341)               # odd rows
    assert bool((pipe.out16 == CANARY).all())
    done = np.zeros(2 * H, bool)
    for row0, rows in ((170, 342), (0, 86), (86, 84)):
        q = pipe.finish_rows(row0, rows)
        done[row0:row0 + rows] = True
        gy, guv = (t.cpu().numpy() for t in yuv_planes(q, Y.NV12, 2 * H, 2 * W))
        cdone = done[::2]
        assert np.array_equal(gy[done], want_y[done]) and (gy[~done] == CANARY).all(), (row0, rows)
        assert np.array_equal(guv[cdone], want_uv[cdone]) and (guv[~cdone] == CANARY).all(), (row0, rows)
    assert done.all()
    pipe.close()


# ---- host bursts -----------------------------------------------------------------------------------------------------------
def _guarded_host(like):
    """a pinned host buffer typed like `like` between two canary bands: (view, check)"""
    n, g = like.numel() * like.element_size(), 4096
    big = torch.full((g + n + g,), CANARY, dtype=torch.uint8).pin_memory()
    img = big[g:g + n].view(like.dtype).view(like.shape)

    def check(what):
        assert bool((big[:g] == CANARY).all()) and bool((big[g + n:] == CANARY).all()), f"{what}: the download wrote outside the host image"

    return img, check


def _three_host_bursts(cfg, fmt, host, want, what):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, render_image_bytes
    pipe = BurstPipeline(cfg, DEV)
    pipe.set_render(fmt, **RENDER)
    assert pipe.out16.numel() * pipe.out16.element_size() == render_image_bytes(fmt, 2 * W, 2 * H)
    out_host, check = _guarded_host(pipe.out16)
    for rep in range(3):
        out_host.view(torch.uint8).fill_(0)
        got = pipe.process_host(host, out16_host=out_host)
        pipe.host_sync()
        assert np.array_equal(_np(got), want), (what, rep)
        check(what)
    pipe.close()


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_yuv_host_burst_equals_the_resident_one(fmt):
    host = [f.pin_memory() for f in _frames()]
    _three_host_bursts(_config(ring=4), fmt, host, _flat(*_want(fmt)[1:]), NAMES[fmt])


def test_yuv_host_burst_from_packed_frames():
    host = [p.pin_memory() for p in synth.pack_raw(_frames(10), capi.PACK_MIPI10)]
    _three_host_bursts(_config(ring=4, packing=capi.PACK_MIPI10, bits=10), Y.NV12, host, _flat(*_want(Y.NV12, bits=10)[1:]),
                       "MIPI10 in, NV12 out")


_ONE_BAND_CHILD = """
import torch
from tests import test_yuv_gpu as T
host = [f.pin_memory() for f in T._frames()]
for fmt in T.FORMATS:
    T._three_host_bursts(T._config(ring=4), fmt, host, T._flat(*T._want(fmt)[1:]), "one band")
print("ONE-BAND-OK")
"""


def test_yuv_host_burst_in_one_band():
    """MFSR_HOST_BANDS is read once per process: a child process with MFSR_HOST_BANDS=1 (the whole-image finish and one download
    of 3h/2 rows; the default of 8 bands, two copies each, is what the tests above run)."""
    env = dict(os.environ, MFSR_HOST_BANDS="1")
    r = subprocess.run([sys.executable, "-c", _ONE_BAND_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ONE-BAND-OK" in r.stdout, r.stdout + r.stderr


# ---- streams ----------------------------------------------------------------------------------------------------------------
def test_frame_stream_gives_nv12_windows():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream
    frames = [f.to(DEV) for f in _frames()[:3]]
    st = FrameStream(_config(frames=3), 1, DEV, render=dict(format=capi.OUT_NV12, **RENDER))
    outs = {}
    for f in frames:
        r = st.push(f)
        if r is not None:
            outs[r[0]] = r[1].clone()
    torch.cuda.synchronize()
    st.close()
    assert sorted(outs) == [0, 1] and outs[1].dtype == torch.uint8 and tuple(outs[1].shape) == (2 * H * 2 * W * 3 // 2,)
    ref = BurstPipeline(_config(frames=3, reference=1), DEV)      # output 1 = frames [0, 2] around reference 1
    ref.set_render(capi.OUT_NV12, **RENDER)
    _, q = ref.process(frames)
    assert torch.equal(q, outs[1])
    ref.set_render(None)
    lin, _ = ref.process(frames)
    _, wy, wuv = Y.render(lin.cpu().numpy(), Y.NV12, CCM, LUTS["srgb4096"])
    assert np.array_equal(_np(outs[1]), _flat(wy, wuv))
    ref.close()
    ref0 = BurstPipeline(_config(frames=2, reference=0), DEV)     # output 0 = frames [0, 1] around reference 0
    ref0.set_render(capi.OUT_NV12, **RENDER)
    _, q0 = ref0.process(frames[:2])
    assert torch.equal(q0, outs[0])
    ref0.close()


# ---- sharpening and two planes do not go together ---------------------------------------------------------------------------
def test_sharpen_and_yuv_are_refused_by_the_second_setter():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    pipe.set_render(capi.OUT_NV12, **RENDER)
    with pytest.raises(capi.MfsrError):
        pipe.set_sharpen(1.0)
    pipe.set_sharpen(0.0)                        # an "off" description is no sharpening
    _, q = pipe.process(frames)
    assert np.array_equal(_np(q), _flat(*_want(Y.NV12)[1:]))     # the refused call changed nothing
    pipe.set_render(None)
    pipe.set_sharpen(1.0)
    for fmt in FORMATS:
        with pytest.raises(capi.MfsrError):
            pipe.set_render(fmt, **RENDER)
    pipe.set_render(capi.OUT_RGB8, **RENDER)     # (a single-plane format still goes with sharpening)
    pipe.set_sharpen(None)
    pipe.set_render(capi.OUT_P010, **RENDER)
    _, q = pipe.process(frames)
    assert np.array_equal(_np(q), _flat(*_want(Y.P010)[1:]))
    pipe.set_render(None)
    img, q16 = pipe.process(frames)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), _plain_float().view(np.uint32))
    assert np.array_equal(_np(q16), R.render(_plain_float(), R.RGB16)[1])
    pipe.close()
