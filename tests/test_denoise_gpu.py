"""Merge-aware denoise inside the finish on the device: k_denoiseImage against the numpy restatement of
tests/denoise_ref.py, k_finishDenoised against the chain (plain finish to a float image, then the restatement with the count of
the weights), the fade's skip path, and denoised bursts (resident, unfused, striped, windowed, host, streamed, CLI) against the
restatement applied to the plain float image and the weights of the same pipeline.  Every comparison is bit for bit: uint32 views
of floats, bytes of the integer output."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi, synth
from tests import denoise_ref as D
from tests import render_ref as R
from tests.kernels import guarded_upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CANARY = 0xA5
FORMATS = (R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2)
NAMES = {R.RGB16: "RGB16", R.RGB8: "RGB8", R.RGBA8: "RGBA8", R.RGB10A2: "RGB10A2"}
CCM = np.array([1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56], np.float32)
LUT = R.srgb_lut(4096)
f32 = np.float32
# what the kernel tests filter with: a tolerance wide enough that many neighbours of a random image take part
KW = dict(strength=3.0, gain=4.0, alpha=0.05, beta=0.01)


@pytest.fixture(scope="module", autouse=True)
def _default_accumulate_variant():
    """mfsr_set_accumulate_fast_exp is a process-wide selector that kernel-level tests running before this file leave at 1; the
    library's default, which a fresh process such as the CLI runs, is 2.  The selector is put back as found."""
    L = capi.lib()
    found = L.raw["mfsr_get_accumulate_fast_exp"]()
    L.set_accumulate_fast_exp(2)
    yield
    L.set_accumulate_fast_exp(found)


def _denoise(radius=2, strength=3.0, gain=2.0, alpha=0.0, beta=0.0, w_lo=0.0, w_hi=0.0):
    d = capi.Denoise()
    d.radius, d.strength, d.gain, d.alpha, d.beta, d.wLo, d.wHi = radius, strength, gain, alpha, beta, w_lo, w_hi
    return d


def _render(fmt, m=None, lut_dev=None):
    r = capi.Render()
    r.format = fmt
    if m is not None:
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*[float(v) for v in m])
    if lut_dev is not None:
        r.toneLut = lut_dev.data_ptr()
        r.toneSize = lut_dev.numel() - 1
    return r


def _pixels(h, w, seed):
    """a smooth ramp plus noise (so that neighbours fall inside and outside the tolerance), seeded with NaN, +-inf, 1e30,
    negative values and values above 1 and above 65536"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.15 + 0.7 * ((xx + 2 * yy) % 23) / 23.0
    p = (base[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.05, (h, w, 3))).astype(f32)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -3.0, 2.5, 70000.0, 0.0, -0.0, 1.0, 1e-8], f32)
    flat = p.reshape(-1)
    idx = np.arange(0, flat.size, 13)
    flat[idx] = special[np.arange(idx.size) % special.size]
    return p


def _counts(h, w, seed):
    """counts between 0.2 and 8, seeded with 0, NaN, 1e-9, 1e6, inf and a negative one"""
    rng = np.random.default_rng(seed)
    n = rng.uniform(0.2, 8.0, (h, w, 3)).astype(f32)
    special = np.array([0.0, np.nan, 1e-9, 1e6, np.inf, -2.0], f32)
    flat = n.reshape(-1)
    idx = np.arange(5, flat.size, 17)
    flat[idx] = special[np.arange(idx.size) % special.size]
    return n


def _expected_bytes(packed, off, row_bytes, h):
    dense = R.as_bytes(packed)
    want = np.full(off + row_bytes * h, CANARY, np.uint8)
    rows = want[off:].reshape(h, row_bytes)
    rows[:, :dense.shape[1]] = dense
    return want


def _layouts(fmt, w):
    if fmt == R.RGB8:
        return [(0, 3 * w), (1, 3 * w + 5), (3, 3 * w + 2)]      # odd byte offsets with padded rows
    if fmt == R.RGB16:
        return [(0, 6 * w), (2, 6 * w + 2)]
    return [(0, 4 * w), (4, 4 * w + 4)]


SIZES = [(1, 1), (3, 2), (67, 19), (130, 33)]


def _run_image(L, d_in, d_cnt, w, h, d, r, off, rb):
    d_out, check_out = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
    d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, f32))
    L.denoiseImage(d_in.data_ptr(), 12 * w, None if d_cnt is None else d_cnt.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w,
                   d_out.data_ptr() + off, rb, w, h, ctypes.byref(d), None if r is None else ctypes.byref(r), 0, None)
    return d_f, d_out, check_f, check_out


# ---- 1. the tile body on a float image --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_denoiseImage_equals_the_restatement(fmt):
    """Sizes: one pixel; 3 x 2 (smaller than R: every tap clamps); 67 x 19 and 130 x 33 (ragged in both tile directions, no
    multiple of 4 for the RGB8 span).  R = 1, 2, 3; with and without a count image; with and without matrix + table.  The output
    layout cycles through the format's offsets and row paddings."""
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    k = 0
    for w, h in SIZES:
        p, n = _pixels(h, w, 100 * w + h), _counts(h, w, 7 * w + h)
        d_in, check_in = guarded_upload(p)
        d_cnt, check_cnt = guarded_upload(n)
        layouts = _layouts(fmt, w)
        for radius, counted, rendered in itertools.product((1, 2, 3), (False, True), (False, True)):
            m, lut = (CCM, LUT) if rendered else (None, None)
            want_f, want_q = D.denoise_render(p, n if counted else None, fmt, m, lut, radius=radius, **KW)
            off, rb = layouts[k % len(layouts)]
            d_f, d_out, check_f, check_out = _run_image(L, d_in, d_cnt if counted else None, w, h, _denoise(radius, **KW),
                                                        _render(fmt, m, lut_dev if rendered else None), off, rb)
            what = f"{NAMES[fmt]} {w}x{h} R={radius} count={counted} rendered={rendered} offset={off} rowBytes={rb}"
            check_out(what)
            check_f(what)
            assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), what + " (float image)"
            assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, off, rb, h)), what
            k += 1
        check_in(f"{NAMES[fmt]} {w}x{h}", unchanged=True)
        check_cnt(f"{NAMES[fmt]} {w}x{h}", unchanged=True)
    assert k == 4 * 3 * 2 * 2


def test_denoiseImage_without_a_render_description_zero_noise_model_and_pitched_rows():
    """render = NULL is {RGB16, no matrix, no table}; the float image alone and the integers alone; pitched input and count rows;
    alpha = beta = 0 (the tolerance is the floor 1e-20: only equal neighbours take part)"""
    L = capi.lib()
    w, h, pitch = 70, 19, 12 * 70 + 16
    p, n = _pixels(h, w, 8), _counts(h, w, 9)
    p[4:9, 10:30] = p[4, 10]                      # a flat patch: equal neighbours even at the floor
    rows = np.full((2, h, pitch), CANARY, np.uint8)
    rows[0, :, :12 * w] = p.view(np.uint8).reshape(h, 12 * w)
    rows[1, :, :12 * w] = n.view(np.uint8).reshape(h, 12 * w)
    d_rows, check_rows = guarded_upload(rows)
    for kw in (KW, dict(strength=3.0, gain=2.0, alpha=0.0, beta=0.0)):
        d = _denoise(3, **kw)
        want_f, want_q = D.denoise_render(p, n, R.RGB16, radius=3, **kw)
        for with_f, with_q in ((True, False), (False, True), (True, True)):
            d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, f32))
            d_q, check_q = guarded_upload(np.full(6 * w * h, CANARY, np.uint8))
            L.denoiseImage(d_rows[0].data_ptr(), pitch, d_rows[1].data_ptr(), pitch, d_f.data_ptr() if with_f else None, 12 * w,
                           d_q.data_ptr() if with_q else None, 6 * w, w, h, ctypes.byref(d), None, 0, None)
            check_f("one output")
            check_q("one output")
            got_f, got_q = d_f.cpu().numpy(), d_q.cpu().numpy()
            assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)) if with_f else (got_f == -7.0).all()
            assert np.array_equal(got_q, _expected_bytes(want_q, 0, 6 * w, h)) if with_q else (got_q == CANARY).all()
    check_rows("pitched input", unchanged=True)


@pytest.mark.parametrize("how", ["lds", "cache"])
def test_denoiseImage_lut_in_lds_and_through_the_cache_give_the_same_bytes(monkeypatch, how):
    """MFSR_RENDER_LUT forces one way of reading the tone table; unset, the denoised kernels read it through the cache"""
    L = capi.lib()
    w, h = 130, 33
    p, n = _pixels(h, w, 9), _counts(h, w, 10)
    d_in, _ = guarded_upload(p)
    d_cnt, _ = guarded_upload(n)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    monkeypatch.setenv("MFSR_RENDER_LUT", how)
    for fmt in FORMATS:
        want_f, want_q = D.denoise_render(p, n, fmt, CCM, LUT, radius=2, **KW)
        rb = R.row_bytes(fmt, w)
        d_f, d_out, check_f, check_out = _run_image(L, d_in, d_cnt, w, h, _denoise(2, **KW), _render(fmt, CCM, lut_dev), 0, rb)
        check_out(how)
        check_f(how)
        assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, 0, rb, h)), (how, NAMES[fmt])
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (how, NAMES[fmt])


# ---- 2. the fade ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.RGB8, R.RGBA8], ids=NAMES.get)
def test_fade_skip_path_and_mixed_waves(fmt):
    """wLo = 1, wHi = 2.  Counts all >= 2: every wave skips the stencil and the output is mfsr_renderImage of s bit for bit.  A
    left / right split at column 64 (whole waves skip beside whole waves that filter) and a checkerboard of counts (every wave
    mixed) equal the restatement."""
    L = capi.lib()
    w, h = 130, 33
    p = _pixels(h, w, 21)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    d_in, _ = guarded_upload(p)
    kw = dict(KW, w_lo=1.0, w_hi=2.0)
    rb = R.row_bytes(fmt, w)
    rng = np.random.default_rng(4)
    high = rng.uniform(2.0, 9.0, (h, w, 3)).astype(f32)
    high[0, 0] = [2.0, np.inf, 1e6]
    split = high.copy()
    split[:, :64] = rng.uniform(0.3, 1.9, (h, 64, 3)).astype(f32)
    yy, xx = np.mgrid[0:h, 0:w]
    board = np.where(((yy + xx) % 2 == 0)[..., None], high, f32(1.5)).astype(f32)
    board[5, 7] = [np.nan, 0.0, 1.25]
    for name, n in (("all skip", high), ("split", split), ("checkerboard", board)):
        d_cnt, _ = guarded_upload(n)
        want_f, want_q = D.denoise_render(p, n, fmt, CCM, LUT, radius=3, **kw)
        d_f, d_out, check_f, check_out = _run_image(L, d_in, d_cnt, w, h, _denoise(3, **kw), _render(fmt, CCM, lut_dev), 0, rb)
        check_out(name)
        check_f(name)
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), name
        assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, 0, rb, h)), name
        if name == "all skip":
            s = D.clean(p)
            d_s, _ = guarded_upload(s)
            d_rf, check_rf = guarded_upload(np.zeros((h, w, 3), f32))
            d_rq, check_rq = guarded_upload(np.full(rb * h, CANARY, np.uint8))
            r = _render(fmt, CCM, lut_dev)
            L.renderImage(d_s.data_ptr(), 12 * w, d_rf.data_ptr(), 12 * w, d_rq.data_ptr(), rb, w, h, ctypes.byref(r), 0, None)
            check_rf(name)
            check_rq(name)
            assert torch.equal(d_rf.view(torch.int32), d_f.view(torch.int32)) and torch.equal(d_rq, d_out)
        else:
            assert not np.array_equal(want_f.view(np.uint32), R.render(D.clean(p), fmt, CCM, LUT)[0].view(np.uint32))


# ---- 3. the fused kernel against the chain ----------------------------------------------------------------------------------
def _accumulators(W, H, fbW, fbH, thr):
    """weights of 0, just below and just above the threshold, ordinary and large; the left 64 columns of rows 0..15 are all
    above the threshold (those waves skip the fallback resample)"""
    rng = np.random.default_rng(11)
    wt = rng.uniform(0.5, 6.0, (H, W, 3)).astype(f32)
    low = ((np.add.outer(np.arange(H), np.arange(W)) % 3) == 0)
    low[:16, :64] = False
    wt[low] = np.array([0.0, np.nextafter(f32(thr), f32(0)), np.nextafter(f32(thr), f32(1))], f32)
    wt[::5, 1::7] = np.array([1e-4, 250.0, 1e6], f32)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 0.2 + 0.6 * ((xx + yy) % 17) / 17.0
    val = (base[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.04, (H, W, 3))).astype(f32)
    fin = (val * np.maximum(wt, f32(0.3))).astype(f32)
    fb = rng.uniform(0.2, 0.8, (fbH, fbW, 3)).astype(f32)
    return fin, wt, fb


@pytest.mark.parametrize("lut_form", [None, "lds"])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_finishDenoised_equals_the_chain(fmt, lut_form, monkeypatch):
    """mfsr_finishFusedWindow (float image, no gamma) then the restatement with the count of the weights, against the one launch
    on a 130 x 33 rectangle at (colOffset, rowOffset) = (16, 8) of a 160 x 50 frame: the whole rectangle; stripes of 16 and 17
    rows with R rows of reach either way (= the rows of the whole); the first stripe with no reach below (= the restatement of
    the rows it may read: it clamps at its own edge)."""
    if lut_form:
        monkeypatch.setenv("MFSR_RENDER_LUT", lut_form)
    else:
        monkeypatch.delenv("MFSR_RENDER_LUT", raising=False)
    L = capi.lib()
    W, H, X0, Y0, FW, FH, fbW, fbH, thr = 130, 33, 16, 8, 160, 50, 80, 25, 1e-3
    Rr = 3
    fin, wt, fb = _accumulators(W, H, fbW, fbH, thr)
    d_fin, c1 = guarded_upload(fin)
    d_wt, c2 = guarded_upload(wt)
    d_fb, c3 = guarded_upload(fb)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    r = _render(fmt, CCM, lut_dev)
    kw = dict(strength=3.0, gain=4.0, alpha=0.02, beta=0.002)
    d = _denoise(Rr, **kw)
    d_lin, _ = guarded_upload(np.zeros((H, W, 3), f32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * W, None, W, H, thr, 0, 65535.0, X0, Y0, FW, FH, None)
    lin = d_lin.cpu().numpy()
    n = D.count_of_weight(wt, thr)

    def want(y0, y1):
        f, q = D.denoise_render(lin[y0:y1], n[y0:y1], fmt, CCM, LUT, radius=Rr, **kw)
        return f, R.as_bytes(q)

    def run(y0, h, above, below, what):
        rb = R.row_bytes(fmt, W)
        d_f, cf = guarded_upload(np.zeros((h, W, 3), f32))
        d_q, cq = guarded_upload(np.full(rb * h, CANARY, np.uint8))
        o = 12 * y0 * W
        L.finishDenoised(d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                         d_f.data_ptr(), 12 * W, d_q.data_ptr(), rb, ctypes.byref(r), W, h, thr, 0, X0, Y0 + y0, FW, FH, ctypes.byref(d),
                         above, below, None)
        cf(what)
        cq(what)
        return d_f.cpu().numpy(), d_q.cpu().numpy().reshape(h, rb)

    whole_f, whole_q = want(0, H)
    assert not np.array_equal(whole_f.view(np.uint32), R.render(D.clean(lin), fmt, CCM, LUT)[0].view(np.uint32))
    got_f, got_q = run(0, H, 0, 0, "whole")
    assert np.array_equal(got_f.view(np.uint32), whole_f.view(np.uint32)) and np.array_equal(got_q, whole_q)
    got_f, got_q = run(0, 16, 0, Rr, "stripe of 16 rows")
    assert np.array_equal(got_f.view(np.uint32), whole_f[:16].view(np.uint32)) and np.array_equal(got_q, whole_q[:16])
    got_f, got_q = run(16, 17, Rr, 0, "stripe of 17 rows")
    assert np.array_equal(got_f.view(np.uint32), whole_f[16:].view(np.uint32)) and np.array_equal(got_q, whole_q[16:])
    got_f, got_q = run(8, 16, Rr, Rr, "inner stripe")
    assert np.array_equal(got_f.view(np.uint32), whole_f[8:24].view(np.uint32)) and np.array_equal(got_q, whole_q[8:24])
    alone_f, alone_q = want(16, H)
    assert not np.array_equal(alone_q, whole_q[16:])
    got_f, got_q = run(16, 17, 0, 0, "stripe alone: rowsAbove = 0 clamps at its own edge")
    assert np.array_equal(got_f.view(np.uint32), alone_f.view(np.uint32)) and np.array_equal(got_q, alone_q)
    for c in (c1, c2, c3):
        c("inputs", unchanged=True)


# ---- bursts -----------------------------------------------------------------------------------------------------------------
W, H, N = 96, 64, 3
_cache = {}
RENDER = dict(matrix=CCM, tone_lut=LUT)
DENOISE = dict(strength=3.0, radius=2, gain=2.0, alpha=1.6e-3, beta=1.6e-5)
REF_KW = dict(radius=2, strength=3.0, gain=2.0, alpha=1.6e-3, beta=1.6e-5)


def _frames():
    if "frames" not in _cache:
        frames, _, _, _ = synth.make_moving_burst(W, H, N, alpha=1.6e-3, beta=1.6e-5)
        _cache["frames"] = [f.contiguous() for f in frames]
    return _cache["frames"]


def _config(fused=1, ring=0, frames=N, reference=0):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, frames, scale=2)
    cfg.applyGamma, cfg.fused, cfg.uploadRing, cfg.reference = 0, fused, ring, reference
    return cfg


def _np(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def _plain(fused=1):
    """(plain float image, total weights, weightThreshold) of the burst: computed once per configuration, shared, unchanged"""
    if ("plain", fused) not in _cache:
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        cfg = _config(fused=fused)
        pipe = BurstPipeline(cfg, DEV)
        img, _ = pipe.process([f.to(DEV) for f in _frames()])
        _cache["plain", fused] = (img.cpu().numpy().copy(), pipe.total_weights.cpu().numpy().copy(), float(cfg.weightThreshold))
        pipe.close()
    return _cache["plain", fused]


def _want(fmt, fused=1, rendered=True):
    key = ("want", fmt, fused, rendered)
    if key not in _cache:
        lin, tw, thr = _plain(fused)
        m, lut = (CCM, LUT) if rendered else (None, None)
        _cache[key] = R.render(D.finish_denoise(lin, tw, thr, **REF_KW), fmt, m, lut)
    return _cache[key]


@pytest.mark.parametrize("fused", [1, 0])
def test_denoised_burst_equals_the_restatement_of_the_plain_burst(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(fused=fused), DEV)
    pipe.set_denoise(**DENOISE)
    for fmt in FORMATS:
        pipe.set_render(fmt, **RENDER)
        img, q = pipe.process(frames)
        want_f, want_q = _want(fmt, fused)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (NAMES[fmt], fused)
        assert np.array_equal(_np(q), want_q), (NAMES[fmt], fused)
        assert pipe.denoised_finishes() == 1 and pipe.sharpened_finishes() == 0
    pipe.set_render(None)            # without a render description: uint16 RGB of the denoised linear image
    img, q = pipe.process(frames)
    want_f, want_q = _want(R.RGB16, fused, rendered=False)
    assert q.dtype == torch.int16
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)) and np.array_equal(_np(q), want_q)
    lin = _plain(fused)[0]
    assert not np.array_equal(want_f.view(np.uint32), lin.view(np.uint32))
    pipe.close()


def test_denoise_defaults_to_the_configurations_noise_model():
    """alpha / beta None = cfg.alpha / cfg.beta"""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    cfg = _config()
    pipe = BurstPipeline(cfg, DEV)
    pipe.set_denoise(strength=3.0)
    img, _ = pipe.process([f.to(DEV) for f in _frames()])
    lin, tw, thr = _plain()
    want = D.finish_denoise(lin, tw, thr, radius=2, strength=3.0, gain=2.0, alpha=cfg.alpha, beta=cfg.beta)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want.view(np.uint32))
    pipe.close()


def test_denoised_finish_rows_are_the_rows_of_the_whole():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    pipe.set_denoise(**DENOISE)
    pipe.out16.fill_(CANARY)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for k, f in enumerate(frames):
        pipe.add_frame(f, k == 0)
    want = _want(R.RGB8)[1]
    done = np.zeros(2 * H, bool)
    for row0, rows in ((64, 64), (0, 64)):
        q = pipe.finish_rows(row0, rows)
        done[row0:row0 + rows] = True
        got = q.cpu().numpy()
        assert np.array_equal(got[done], want[done]) and (got[~done] == CANARY).all(), (row0, rows)
    assert done.all() and pipe.denoised_finishes() == 2
    pipe.close()


def _host_bursts(fmt, what):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    host = [f.pin_memory() for f in _frames()]
    pipe = BurstPipeline(_config(ring=4), DEV)
    pipe.set_render(fmt, **RENDER)
    pipe.set_denoise(**DENOISE)
    want_q = _want(fmt)[1]
    for rep in range(2):
        got = pipe.process_host(host)
        pipe.host_sync()
        assert np.array_equal(_np(got), want_q), (what, rep)
    finishes = pipe.denoised_finishes()
    pipe.close()
    return finishes


@pytest.mark.parametrize("fmt", [R.RGB8, R.RGB10A2], ids=NAMES.get)
def test_denoised_host_burst_equals_the_resident_one(fmt):
    assert _host_bursts(fmt, NAMES[fmt]) > 1          # banded: one finish per band, each after the band below it was fused


_ONE_BAND_CHILD = """
from tests import test_denoise_gpu as T
from tests import render_ref as R
from multi_frame_super_resolution_amd import capi
capi.lib().set_accumulate_fast_exp(2)
for fmt in (R.RGB8, R.RGB10A2):
    finishes = T._host_bursts(fmt, "one band")
    assert finishes == 1, finishes
print("ONE-BAND-OK")
"""


def test_denoised_host_burst_in_one_band():
    """MFSR_HOST_BANDS is read once per process: a child process with MFSR_HOST_BANDS=0 (taken as one band)"""
    env = dict(os.environ, MFSR_HOST_BANDS="0")
    r = subprocess.run([sys.executable, "-c", _ONE_BAND_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ONE-BAND-OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("fmt", [R.RGB8, R.RGB10A2], ids=NAMES.get)
def test_denoised_zoom_window_is_the_crop(fmt):
    """the Python layer grows the aligned window by one 16-pixel ring (clipped to the frame) and crops"""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    want_f, want_q = _want(fmt)
    for x, y, w, h in ((40, 24, 100, 60), (0, 70, 90, 58)):
        pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
        pw.set_render(fmt, **RENDER)
        pw.set_denoise(**DENOISE)
        img, q = pw.process([f.to(DEV) for f in _frames()])
        assert tuple(q.shape[:2]) == (h, w)
        assert np.array_equal(_np(q), want_q[y:y + h, x:x + w]), (x, y, w, h)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f[y:y + h, x:x + w].view(np.uint32)), (x, y, w, h)
        pw.close()


def test_frame_stream_denoises_its_outputs():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream
    frames = [f.to(DEV) for f in _frames()]
    st = FrameStream(_config(frames=3), 1, DEV, render=dict(format=capi.OUT_RGB8, **RENDER), denoise=DENOISE)
    outs = {}
    for f in frames:
        r = st.push(f)
        if r is not None:
            outs[r[0]] = r[1].clone()
    torch.cuda.synchronize()
    st.close()
    assert sorted(outs) == [0, 1] and outs[1].dtype == torch.uint8 and tuple(outs[1].shape) == (2 * H, 2 * W, 3)
    ref = BurstPipeline(_config(frames=3, reference=1), DEV)      # output 1 = frames [0, 2] around reference 1
    lin, _ = ref.process(frames)
    want = R.render(D.finish_denoise(lin.cpu().numpy(), ref.total_weights.cpu().numpy(), float(ref.cfg.weightThreshold), **REF_KW),
                    R.RGB8, CCM, LUT)[1]
    assert np.array_equal(_np(outs[1]), want)
    ref.close()


def test_off_is_off():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    ref = BurstPipeline(_config(), DEV)
    ref.set_render(capi.OUT_RGB8, **RENDER)
    f0, q0 = (t.clone() for t in ref.process(frames))
    paths0 = ref.debug_paths()
    assert ref.denoised_finishes() == 0
    ref.close()
    for how in ("none", "strength 0", "radius 0", "on and off again"):
        pipe = BurstPipeline(_config(), DEV)
        pipe.set_render(capi.OUT_RGB8, **RENDER)
        if how == "none":
            pipe.set_denoise(None)
        elif how == "strength 0":
            pipe.set_denoise(0.0)
        elif how == "radius 0":
            pipe.set_denoise(3.0, radius=0)
        else:
            pipe.set_denoise(**DENOISE)
            _, q = pipe.process(frames)
            assert not torch.equal(q, q0) and pipe.denoised_finishes() == 1
            pipe.set_denoise(None)
        f1, q1 = pipe.process(frames)
        assert q1.dtype == q0.dtype and torch.equal(q1, q0), how
        assert torch.equal(f1.view(torch.int32), f0.view(torch.int32)), how
        assert pipe.debug_paths() == paths0 and pipe.denoised_finishes() == 0, how
        pipe.close()


def test_setter_is_refused_while_a_frame_is_pending_and_the_refused_pairs():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    assert pipe.group_size() > 1
    raw = capi.lib().raw
    set_denoise, set_sharpen, set_render = raw["mfsr_burst_set_denoise"], raw["mfsr_burst_set_sharpen"], raw["mfsr_burst_set_render"]
    d = _denoise(2, 3.0, 2.0, 1.6e-3, 1.6e-5)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    pipe.add_frame(frames[0], True)              # waits for the rest of its group
    assert set_denoise(pipe._h, ctypes.byref(d)) == -1 and set_denoise(pipe._h, None) == -1
    with pytest.raises(capi.MfsrError):
        pipe.set_denoise(**DENOISE)
    for f in frames[1:]:
        pipe.add_frame(f)
    img, _ = pipe.finish()
    assert np.array_equal(img.cpu().numpy().view(np.uint32), _plain()[0].view(np.uint32))   # the refused calls changed nothing
    assert pipe.denoised_finishes() == 0
    bad = _denoise(4, 3.0, 2.0)
    assert set_denoise(pipe._h, ctypes.byref(bad)) == -1
    # denoise + sharpen, in either order
    s = capi.Sharpen()
    s.radius, s.amount = 1, 1.0
    s.taps[0], s.taps[1] = 0.5, 0.25
    assert set_denoise(pipe._h, ctypes.byref(d)) == 0 and set_sharpen(pipe._h, ctypes.byref(s)) == -1
    assert set_denoise(pipe._h, None) == 0 and set_sharpen(pipe._h, ctypes.byref(s)) == 0
    assert set_denoise(pipe._h, ctypes.byref(d)) == -1
    off = _denoise(0, 3.0, 2.0)
    assert set_denoise(pipe._h, ctypes.byref(off)) == 0          # a description that is off pairs with anything
    assert set_sharpen(pipe._h, None) == 0
    # denoise + a two-plane format, in either order
    yuv = _render(capi.OUT_NV12)
    assert set_denoise(pipe._h, ctypes.byref(d)) == 0 and set_render(pipe._h, ctypes.byref(yuv)) == -1
    assert set_denoise(pipe._h, None) == 0 and set_render(pipe._h, ctypes.byref(yuv)) == 0
    assert set_denoise(pipe._h, ctypes.byref(d)) == -1
    assert set_render(pipe._h, None) == 0 and set_denoise(pipe._h, ctypes.byref(d)) == 0
    # the refusals left a working handle: the burst denoises
    img, _ = pipe.process(frames)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), _want(R.RGB16, rendered=False)[0].view(np.uint32))
    pipe.close()


# ---- the CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_denoises_inside_the_finish(tmp_path):
    """MFSR_DENOISE on the bundled burst: _sr_result is exactly the RGB8 image the Python pipeline renders with the same
    configuration and the same description (alpha, beta = cfg's), and it differs from the plain one.  Nothing else changes:
    _sr2_result is by construction the sharpenImg2 pass of _sr_result, so it follows the denoised image and is exactly
    mfsr_sharpenImg2 of it (as the plain run's is of the plain image); both runs write the same two files and no other, and
    print the same lines to stdout up to the numbers in them (times).  Bad values, MFSR_GPUS > 1 and MFSR_SHARPEN are refused
    with a message."""
    import re
    import shutil
    from PIL import Image
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    from tests.test_bundled_burst import CITY, _cfg, _raws
    cli = os.path.join(ROOT, "apps", "multi_frame_sr")
    assert os.path.exists(cli), "build apps/multi_frame_sr first (__graft_entry__.build())"
    outs, outs2, files, lines = {}, {}, {}, {}
    for name, env in (("plain", {}), ("denoised", {"MFSR_DENOISE": "4,3,8"})):
        d = tmp_path / name
        d.mkdir()
        for i in range(5):
            shutil.copy(os.path.join(CITY, f"img_{i:06d}.png"), d / f"img_{i:06d}.png")
        e = dict(os.environ, **env)
        for k in ("MFSR_CCM", "MFSR_SHARPEN", "MFSR_AUTO", "MFSR_NOISE", "MFSR_GPUS"):
            e.pop(k, None)
        if "MFSR_DENOISE" not in env:
            e.pop("MFSR_DENOISE", None)
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=d, capture_output=True, text=True, timeout=300, env=e)
        assert p.returncode == 0, p.stderr
        outs[name] = np.asarray(Image.open(d / "city_farneback_sr_result.png"))
        outs2[name] = np.asarray(Image.open(d / "city_farneback_sr2_result.png"))
        files[name] = sorted(f.name for f in d.iterdir() if not f.name.startswith("img_"))
        lines[name] = [re.sub(r"[-+]?\d+(\.\d+)?([eE][-+]?\d+)?", "#", ln) for ln in p.stdout.splitlines()]
    assert files["plain"] == files["denoised"] == ["city_farneback_sr2_result.png", "city_farneback_sr_result.png"]
    assert lines["plain"] == lines["denoised"]
    for name in outs:        # _sr2_result = sharpenImg2(_sr_result), with and without MFSR_DENOISE
        hh, ww = outs[name].shape[:2]
        d8 = torch.from_numpy(np.ascontiguousarray(outs[name])).to(DEV)
        d8s = torch.full_like(d8, CANARY)
        capi.lib().sharpenImg2(d8.data_ptr(), d8s.data_ptr(), hh, ww, 3, 3 * ww, 3 * ww, None)
        assert np.array_equal(d8s.cpu().numpy(), outs2[name]), name
    assert not np.array_equal(outs2["denoised"], outs2["plain"])
    assert not np.array_equal(outs["denoised"], outs["plain"])
    raws, w, h = _raws(5)
    cfg = _cfg(w, h, 5)
    cfg.preAlign = 1
    cfg.lkIterations = 3
    pipe = BurstPipeline(cfg, DEV)
    frames = [torch.from_numpy(r.view(np.int16)).to(DEV) for r in raws]
    pipe.set_render(capi.OUT_RGB8)
    pipe.set_denoise(4.0, radius=3, gain=8.0)
    _, q = pipe.process(frames)
    got = q.cpu().numpy()
    bad = np.argwhere(got != outs["denoised"])
    print(f"CLI denoised: {len(bad)} samples differ from the Python pipeline's")
    assert np.array_equal(got, outs["denoised"])
    pipe.close()
    for bad in ("", "x", "3,", "3,,2", "3,4", "3,0", "3,1.5", "3,2,0", "3,2,2000", "17", "0.01", "0", "3,2,2,1", "nan"):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, MFSR_DENOISE=bad))
        assert p.returncode != 0 and "MFSR_DENOISE" in p.stderr, bad
    p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, MFSR_DENOISE="3", MFSR_GPUS="2"))
    assert p.returncode != 0 and "MFSR_DENOISE is not supported with MFSR_GPUS > 1" in p.stderr
    p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, MFSR_DENOISE="3", MFSR_SHARPEN="1.0"))
    assert p.returncode != 0 and "MFSR_DENOISE is not supported with MFSR_SHARPEN" in p.stderr
