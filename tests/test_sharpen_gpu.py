"""Sharpening inside the finish on the device: k_sharpenImage against the numpy restatement of
tests/sharpen_ref.py, k_finishSharpened against the chain (plain finish to a float image, then the restatement), and sharpened
bursts (resident, unfused, striped, windowed, host, captured, streamed, CLI) against the restatement applied to the plain float
image of the same pipeline.  Every comparison is bit for bit: uint32 views of floats, bytes of the integer output."""
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
from tests import sharpen_ref as S
from tests.kernels import guarded_upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CANARY = 0xA5
FORMATS = (R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2)
NAMES = {R.RGB16: "RGB16", R.RGB8: "RGB8", R.RGBA8: "RGBA8", R.RGB10A2: "RGB10A2"}
CCM = np.array([1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56], np.float32)
LUT = R.srgb_lut(4096)
# k[0..R] per radius: the helper's Gaussian and a set that is none (it does not sum to 1 and has negative lobes)
TAPS = {
    ("gauss", 1): S.gaussian_taps(0.6, 1)[1], ("gauss", 4): S.gaussian_taps(1.7, 4)[1],
    ("odd", 1): np.array([0.5, 0.3], np.float32), ("odd", 4): np.array([0.5, 0.3, -0.05, 0.02, -0.01], np.float32),
}


@pytest.fixture(scope="module", autouse=True)
def _default_accumulate_variant():
    """mfsr_set_accumulate_fast_exp is a process-wide selector and kernel-level tests that run before this file leave it at 1
    (v_exp_f32 in the straight kernel); the library's default, which a fresh process such as the CLI runs, is 2.  The bursts
    here are the default ones (the CLI test compares an in-process burst with the CLI's, and sharpening amplifies the
    accumulators' last-bit differences between the two variants into 8-bit levels).  The selector is put back as found."""
    L = capi.lib()
    found = L.raw["mfsr_get_accumulate_fast_exp"]()
    L.set_accumulate_fast_exp(2)
    yield
    L.set_accumulate_fast_exp(found)


def _tile():
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    capi.lib().sharpen_tile(ctypes.byref(tw), ctypes.byref(th))
    return tw.value, th.value


def _sharpen(taps, amount=1.0, threshold=0.0):
    s = capi.Sharpen()
    s.radius = len(taps) - 1
    for d, k in enumerate(taps):
        s.taps[d] = float(k)
    s.amount, s.threshold = amount, threshold
    return s


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
    """as tests/test_render_gpu.py's, without +-inf: NaN, negatives, values above 1 and above 65536 stay"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.25, 1.25, h * w * 3).astype(np.float32)
    special = np.array([np.nan, -3.0, 2.5, 70000.0, 300.0, 0.0, 1.0, 0.25, 0.5, 0.75, 1000 / 4096, 4095 / 4096, 1 / 4096, 0.0031308,
                        1e-8], np.float32)
    idx = np.arange(0, p.size, 5)
    p[idx] = special[np.arange(idx.size) % special.size]
    return p.reshape(h, w, 3)


def _expected_bytes(packed, off, row_bytes, h):
    dense = R.as_bytes(packed)
    want = np.full(off + row_bytes * h, CANARY, np.uint8)
    rows = want[off:].reshape(h, row_bytes)
    rows[:, :dense.shape[1]] = dense
    return want


def _layouts(fmt, w):
    if fmt == R.RGB8:
        return list(itertools.product((0, 1, 2, 3), (3 * w, 3 * w + 5)))
    if fmt == R.RGB16:
        return [(0, 6 * w), (2, 6 * w + 2)]
    return [(0, 4 * w), (4, 4 * w + 4)]


def _sizes():
    tw, th = _tile()
    return [(1, 1), (3, 2), (tw + 1, th + 1), (2 * tw - 1, 3), (130, 37)]


# ---- 1. the tile body on a float image --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_sharpenImage_equals_the_restatement(fmt):
    """Sizes: one pixel; 3 x 2 (smaller than the halo: every tap clamps); one pixel more than a tile both ways; one less than two
    tiles; several tiles with a ragged edge.  The output layout cycles through the format's offsets and row paddings."""
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    n = 0
    for w, h in _sizes():
        p = _pixels(h, w, 100 * w + h)
        d_in, check_in = guarded_upload(p)
        layouts = _layouts(fmt, w)
        for (kind, rad), thr, rendered in itertools.product(TAPS, (0.0, 0.01), (False, True)):
            taps = TAPS[kind, rad]
            m, lut = (CCM, LUT) if rendered else (None, None)
            want_f, want_q = S.sharpen_render(p, taps, 1.5, thr, fmt, m, lut)
            s = _sharpen(taps, 1.5, thr)
            r = _render(fmt, m, lut_dev if rendered else None)
            off, rb = layouts[n % len(layouts)]
            d_out, check_out = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
            d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
            L.sharpenImage(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_out.data_ptr() + off, rb, w, h, ctypes.byref(s),
                           ctypes.byref(r), 0, None)
            what = f"{NAMES[fmt]} {w}x{h} taps={kind} R={rad} threshold={thr} rendered={rendered} offset={off} rowBytes={rb}"
            check_out(what)
            check_f(what)
            assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), what + " (float image)"
            assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, off, rb, h)), what
            n += 1
        check_in(f"{NAMES[fmt]} {w}x{h}", unchanged=True)
    assert n == 5 * 4 * 2 * 2


def test_sharpenImage_without_a_render_description_and_with_one_output():
    """render = NULL is {RGB16, no matrix, no table}; the float image alone, the integers alone, and pitched input rows"""
    L = capi.lib()
    w, h, pitch = 70, 19, 12 * 70 + 16
    p = _pixels(h, w, 8)
    rows = np.full((h, pitch), CANARY, np.uint8)
    rows[:, :12 * w] = p.view(np.uint8).reshape(h, 12 * w)
    d_in, check_in = guarded_upload(rows)
    taps = TAPS["gauss", 4]
    s = _sharpen(taps, 2.0, 0.0)
    want_f, want_q = S.sharpen_render(p, taps, 2.0, 0.0, R.RGB16)
    for with_f, with_q in ((True, False), (False, True), (True, True)):
        d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
        d_q, check_q = guarded_upload(np.full(6 * w * h, CANARY, np.uint8))
        L.sharpenImage(d_in.data_ptr(), pitch, d_f.data_ptr() if with_f else None, 12 * w, d_q.data_ptr() if with_q else None, 6 * w,
                       w, h, ctypes.byref(s), None, 0, None)
        check_f("one output")
        check_q("one output")
        got_f, got_q = d_f.cpu().numpy(), d_q.cpu().numpy()
        assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)) if with_f else (got_f == -7.0).all()
        assert np.array_equal(got_q, _expected_bytes(want_q, 0, 6 * w, h)) if with_q else (got_q == CANARY).all()
    check_in("pitched input", unchanged=True)


@pytest.mark.parametrize("how", ["lds", "cache"])
def test_sharpenImage_lut_in_lds_and_through_the_cache_give_the_same_bytes(monkeypatch, how):
    """MFSR_RENDER_LUT forces one way of reading the tone table (as for mfsr_renderImage); unset, the sharpened kernels read it
    through the cache for every format, which is what the tests above run"""
    L = capi.lib()
    w, h = 130, 37
    p = _pixels(h, w, 9)
    d_in, _ = guarded_upload(p)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    monkeypatch.setenv("MFSR_RENDER_LUT", how)
    for fmt in (R.RGB8, R.RGB10A2):
        taps = TAPS["odd", 4]
        want_f, want_q = S.sharpen_render(p, taps, 1.0, 0.01, fmt, CCM, LUT)
        rb = R.row_bytes(fmt, w)
        d_out, check_out = guarded_upload(np.full(rb * h, CANARY, np.uint8))
        d_f, check_f = guarded_upload(np.zeros((h, w, 3), np.float32))
        s, r = _sharpen(taps, 1.0, 0.01), _render(fmt, CCM, lut_dev)
        L.sharpenImage(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_out.data_ptr(), rb, w, h, ctypes.byref(s), ctypes.byref(r), 0,
                       None)
        check_out(how)
        check_f(how)
        assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, 0, rb, h)), (how, NAMES[fmt])
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (how, NAMES[fmt])


# ---- 2. the fused kernel against the chain ----------------------------------------------------------------------------------
def _accumulators(W, H, fbW, fbH):
    """what test_finishRendered_equals_the_chain uses: the left 64 columns of rows 0..19 are all above the threshold (those waves
    skip the fallback resample), a checkerboard of sub-threshold weights elsewhere (those take it)"""
    rng = np.random.default_rng(11)
    fin = rng.uniform(0, 2, (H, W, 3)).astype(np.float32)
    wt = rng.uniform(0.5, 2, (H, W, 3)).astype(np.float32)
    low = ((np.add.outer(np.arange(H), np.arange(W)) % 3) == 0)
    low[:20, :64] = False
    wt[low] = np.array([0.0, 5e-4, 0.7], np.float32)
    fb = rng.uniform(0, 1, (fbH, fbW, 3)).astype(np.float32)
    return fin, wt, fb


@pytest.mark.parametrize("lut_form", [None, "lds"])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_finishSharpened_equals_the_chain(fmt, lut_form, monkeypatch):
    """mfsr_finishFusedWindow (float image, no gamma) then the restatement, against the one launch: the whole 130 x 48 image, the
    stripe of rows [16, 32) with four rows of reach either way (= rows 16..31 of the whole), the same stripe with no reach (= the
    restatement of the stripe alone), and a window of columns [16, 80) of that stripe (which clamps at its own columns)."""
    if lut_form:        # (unset: every format reads the tone table through the cache; lds: staged by the workgroup)
        monkeypatch.setenv("MFSR_RENDER_LUT", lut_form)
    else:
        monkeypatch.delenv("MFSR_RENDER_LUT", raising=False)
    L = capi.lib()
    W, H, fbW, fbH, thr = 130, 48, 65, 24, 1e-3
    fin, wt, fb = _accumulators(W, H, fbW, fbH)
    d_fin, c1 = guarded_upload(fin)
    d_wt, c2 = guarded_upload(wt)
    d_fb, c3 = guarded_upload(fb)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    r = _render(fmt, CCM, lut_dev)
    taps = TAPS["gauss", 4]
    s = _sharpen(taps, 1.25, 0.005)
    bpp = R.BYTES_PER_PIXEL[fmt]
    d_lin, _ = guarded_upload(np.zeros((H, W, 3), np.float32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * W, None, W, H, thr, 0, 65535.0, 0, 0, W, H, None)
    lin = d_lin.cpu().numpy()

    def want(img):
        f, q = S.sharpen_render(img, taps, 1.25, 0.005, fmt, CCM, LUT)
        return f, R.as_bytes(q)

    def run(x0, y0, w, h, above, below, what):
        rb = R.row_bytes(fmt, w)
        d_f, cf = guarded_upload(np.zeros((h, w, 3), np.float32))
        d_q, cq = guarded_upload(np.full(rb * h, CANARY, np.uint8))
        o = 12 * (y0 * W + x0)
        L.finishSharpened(d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                          d_f.data_ptr(), 12 * w, d_q.data_ptr(), rb, ctypes.byref(r), w, h, thr, 0, x0, y0, W, H, ctypes.byref(s),
                          above, below, None)
        cf(what)
        cq(what)
        return d_f.cpu().numpy(), d_q.cpu().numpy().reshape(h, rb)

    whole_f, whole_q = want(lin)
    got_f, got_q = run(0, 0, W, H, 0, 0, "whole")
    assert np.array_equal(got_f.view(np.uint32), whole_f.view(np.uint32)) and np.array_equal(got_q, whole_q)
    got_f, got_q = run(0, 16, W, 16, 4, 4, "stripe with reach")
    assert np.array_equal(got_f.view(np.uint32), whole_f[16:32].view(np.uint32)) and np.array_equal(got_q, whole_q[16:32])
    alone_f, alone_q = want(lin[16:32])
    assert not np.array_equal(alone_q, whole_q[16:32])
    got_f, got_q = run(0, 16, W, 16, 0, 0, "stripe alone")
    assert np.array_equal(got_f.view(np.uint32), alone_f.view(np.uint32)) and np.array_equal(got_q, alone_q)
    # reach on one side only: the stripe with the rows above it, cut
    top_f, top_q = want(lin[12:32])
    got_f, got_q = run(0, 16, W, 16, 4, 0, "stripe with reach above")
    assert np.array_equal(got_f.view(np.uint32), top_f[4:].view(np.uint32)) and np.array_equal(got_q, top_q[4:])
    win_f, win_q = want(lin[12:36, 16:80])
    got_f, got_q = run(16, 16, 64, 16, 4, 4, "window")
    assert np.array_equal(got_f.view(np.uint32), win_f[4:20].view(np.uint32)) and np.array_equal(got_q, win_q[4:20])
    assert bpp * 64 == got_q.shape[1]
    for c in (c1, c2, c3):
        c("inputs", unchanged=True)


# ---- bursts -----------------------------------------------------------------------------------------------------------------
W, H, N = 384, 256, 7
_cache = {}
RENDER = dict(matrix=CCM, tone_lut=LUT)
SHARPEN = dict(amount=1.0, sigma=1.0)                     # radius 3
BURST_TAPS = S.gaussian_taps(1.0, 0)[1]


def _frames(bits=12, seed=29):
    if ("frames", bits, seed) not in _cache:
        frames, _, _ = synth.make_burst(W, H, N, seed=seed, device="cpu")
        if bits == 10:
            frames = [(f.view(torch.int16).to(torch.int32) >> 2).to(torch.int16).view(f.dtype) for f in frames]
        _cache["frames", bits, seed] = [f.contiguous() for f in frames]
    return _cache["frames", bits, seed]


def _config(gamma=0, fused=1, ring=0, packing=0, bits=12, async_fuse=0, frames=N, reference=0):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, frames, scale=2)
    if bits == 10:
        for i in range(3):
            cfg.black[i], cfg.white[i] = 64.0, 1023.0 - 64.0
        cfg.maxVal = 1023.0
    cfg.applyGamma, cfg.fused, cfg.uploadRing, cfg.rawPacking, cfg.asyncFuse, cfg.reference = gamma, fused, ring, packing, async_fuse, reference
    return cfg


def _np(t):
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


def _plain_float(bits=12, fused=1, seed=29):
    """the plain float image (applyGamma = 0) of the burst: computed once per configuration, shared and left unchanged"""
    key = ("plain", bits, fused, seed)
    if key not in _cache:
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        pipe = BurstPipeline(_config(fused=fused, bits=bits), DEV)
        img, _ = pipe.process([f.to(DEV) for f in _frames(bits, seed)])
        _cache[key] = img.cpu().numpy().copy()
        pipe.close()
    return _cache[key]


def _want(fmt, bits=12, fused=1, rendered=True, seed=29):
    """(float image, packed integers) of the sharpened, rendered burst: the restatement on the plain float image"""
    key = ("want", fmt, bits, fused, rendered, seed)
    if key not in _cache:
        m, lut = (CCM, LUT) if rendered else (None, None)
        _cache[key] = S.sharpen_render(_plain_float(bits, fused, seed), BURST_TAPS, 1.0, 0.0, fmt, m, lut)
    return _cache[key]


# ---- 3. off is off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rendered", [False, True])
def test_sharpen_off_is_off(rendered):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    ref = BurstPipeline(_config(gamma=1), DEV)
    if rendered:
        ref.set_render(capi.OUT_RGB8, **RENDER)
    f0, q0 = (t.clone() for t in ref.process(frames))
    paths0 = ref.debug_paths()
    assert ref.sharpened_finishes() == 0
    ref.close()
    for how in ("none", "amount 0", "radius 0", "on and off again"):
        pipe = BurstPipeline(_config(gamma=1), DEV)
        if rendered:
            pipe.set_render(capi.OUT_RGB8, **RENDER)
        if how == "none":
            pipe.set_sharpen(None)
        elif how == "amount 0":
            pipe.set_sharpen(0.0, sigma=1.0)
        elif how == "radius 0":
            s = _sharpen([1.0], 2.0)
            assert s.radius == 0
            pipe.L.burst_set_sharpen(pipe._h, ctypes.byref(s))
        else:
            pipe.set_sharpen(**SHARPEN)
            _, q = pipe.process(frames)
            assert not torch.equal(q, q0) and pipe.sharpened_finishes() == 1
            pipe.set_sharpen(None)
        f1, q1 = pipe.process(frames)
        assert q1.dtype == q0.dtype and torch.equal(q1, q0), how
        assert torch.equal(f1.view(torch.int32), f0.view(torch.int32)), how
        assert pipe.debug_paths() == paths0 and pipe.sharpened_finishes() == 0, how
        pipe.close()


# ---- 4. sharpened resident bursts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_sharpened_burst_equals_the_restatement_of_the_plain_float_image(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(fused=fused), DEV)
    pipe.set_sharpen(**SHARPEN)
    for fmt in FORMATS:
        pipe.set_render(fmt, **RENDER)
        img, q = pipe.process(frames)
        want_f, want_q = _want(fmt, fused=fused)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (NAMES[fmt], fused)
        assert np.array_equal(_np(q), want_q), (NAMES[fmt], fused)
        assert pipe.sharpened_finishes() == 1
    # and without a render description: uint16 RGB of the sharpened linear image
    pipe.set_render(None)
    img, q = pipe.process(frames)
    want_f, want_q = _want(R.RGB16, fused=fused, rendered=False)
    assert q.dtype == torch.int16
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)) and np.array_equal(_np(q), want_q)
    pipe.close()


def test_sharpened_finish_rows_are_the_rows_of_the_whole():
    """mfsr_burst_finish_rows reaches min(R, ...) rows beyond its stripe: stripes in any order fill one RGB8 buffer with the
    whole-frame image"""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    pipe.set_sharpen(**SHARPEN)
    pipe.out16.fill_(CANARY)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for k, f in enumerate(frames):
        pipe.add_frame(f, k == 0)
    want = _want(R.RGB8)[1]
    done = np.zeros(2 * H, bool)
    for row0, rows in ((171, 341), (0, 85), (85, 86)):
        q = pipe.finish_rows(row0, rows)
        done[row0:row0 + rows] = True
        got = q.cpu().numpy()
        assert np.array_equal(got[done], want[done]) and (got[~done] == CANARY).all(), (row0, rows)
    assert done.all() and pipe.sharpened_finishes() == 3
    pipe.close()


# ---- 5. sharpened host bursts: the lagged band ------------------------------------------------------------------------------
def _guarded_host(like):
    n, g = like.numel() * like.element_size(), 4096
    big = torch.full((g + n + g,), CANARY, dtype=torch.uint8).pin_memory()
    img = big[g:g + n].view(like.dtype).view(like.shape)

    def check(what):
        assert bool((big[:g] == CANARY).all()) and bool((big[g + n:] == CANARY).all()), f"{what}: the download wrote outside the host image"

    return img, check


def _three_host_bursts(cfg, fmt, host, want_q, what):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    pipe = BurstPipeline(cfg, DEV)
    pipe.set_render(fmt, **RENDER)
    pipe.set_sharpen(**SHARPEN)
    out_host, check = _guarded_host(pipe.out16)
    for rep in range(3):
        out_host.view(torch.uint8).fill_(0)
        got = pipe.process_host(host, out16_host=out_host)
        pipe.host_sync()
        assert np.array_equal(_np(got), want_q), (what, rep)
        check(what)
    finishes = pipe.sharpened_finishes()
    pipe.close()
    return finishes


@pytest.mark.parametrize("fmt", [R.RGB8, R.RGB10A2], ids=NAMES.get)
def test_sharpened_host_burst_equals_the_resident_one(fmt):
    host = [f.pin_memory() for f in _frames()]
    finishes = _three_host_bursts(_config(ring=4), fmt, host, _want(fmt)[1], NAMES[fmt])
    assert finishes > 1                           # banded: one finish per band, each after the band below it was fused


def test_sharpened_host_burst_from_packed_frames():
    host = [p.pin_memory() for p in synth.pack_raw(_frames(10), capi.PACK_MIPI10)]
    _three_host_bursts(_config(ring=4, packing=capi.PACK_MIPI10, bits=10), R.RGB8, host, _want(R.RGB8, bits=10)[1], "MIPI10 in, RGB8 out")


_ONE_BAND_CHILD = """
import torch
from tests import test_sharpen_gpu as T
from tests import render_ref as R
host = [f.pin_memory() for f in T._frames()]
for fmt in (R.RGB8, R.RGB10A2):
    finishes = T._three_host_bursts(T._config(ring=4), fmt, host, T._want(fmt)[1], "one band")
    assert finishes == 1, finishes
print("ONE-BAND-OK")
"""


def test_sharpened_host_burst_in_one_band():
    """MFSR_HOST_BANDS is read once per process: a child process with MFSR_HOST_BANDS=0 (taken as one band: the whole-image
    finish and one download; the default of 8 bands is what the tests above run)."""
    env = dict(os.environ, MFSR_HOST_BANDS="0")
    r = subprocess.run([sys.executable, "-c", _ONE_BAND_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ONE-BAND-OK" in r.stdout, r.stdout + r.stderr


def test_sharpened_host_burst_captured_as_a_graph():
    """as tests/test_render_gpu.py: one eager burst, host_sync and a device synchronisation; then the burst is captured on fixed
    pinned buffers and replayed on two bursts' data"""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    bursts = [_frames(), _frames(seed=31)]
    want = [_want(R.RGB8)[1], _want(R.RGB8, seed=31)[1]]
    assert not np.array_equal(want[0], want[1])
    static = [torch.empty_like(f).pin_memory() for f in bursts[0]]
    for dst, src in zip(static, bursts[0]):
        dst.copy_(src)
    gpipe = BurstPipeline(_config(ring=4, async_fuse=0), DEV)
    gpipe.set_render(capi.OUT_RGB8, **RENDER)
    gpipe.set_sharpen(**SHARPEN)
    out_host, check = _guarded_host(gpipe.out16)
    got = gpipe.process_host(static, out16_host=out_host)
    gpipe.host_sync()
    torch.cuda.synchronize()
    assert np.array_equal(_np(got), want[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g8 = gpipe.process_host(static, out16_host=out_host)
    for k in (1, 0):
        for dst, src in zip(static, bursts[k]):
            dst.copy_(src)
        g8.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_np(g8), want[k]), f"burst {k}: graph replay differs from the restatement of the plain burst"
        check("graph replay")
    del graph
    gpipe.close()


# ---- 6. zoom windows --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.RGB8, R.RGB10A2], ids=NAMES.get)
def test_sharpened_zoom_window_is_the_crop(fmt):
    """the Python layer grows the aligned window by one 16-pixel ring (clipped to the frame) and crops: the rectangle asked for
    is the crop of the whole-frame sharpened image.  (40, 24, 100, 60) lies inside the frame; (0, 400, 90, 112) touches the
    left and the bottom edge."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    want_f, want_q = _want(fmt)
    for x, y, w, h in ((40, 24, 100, 60), (0, 400, 90, 112)):
        pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
        pw.set_render(fmt, **RENDER)
        pw.set_sharpen(**SHARPEN)
        img, q = pw.process([f.to(DEV) for f in _frames()])
        assert tuple(q.shape[:2]) == (h, w)
        assert np.array_equal(_np(q), want_q[y:y + h, x:x + w]), (x, y, w, h)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f[y:y + h, x:x + w].view(np.uint32)), (x, y, w, h)
        pw.close()


def test_c_level_window_clamps_at_its_own_edges():
    """mfsr_burst_set_sharpen on a windowed burst (past the Python layer's growing): the window is the image.  Its interior, R
    and more from the window's edges, is the crop of the whole; an edge that is the frame's edge is exact up to the edge; and
    the whole window is the restatement of the plain window."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    want_f, _ = _want(R.RGB16, rendered=False)
    plain = _plain_float()
    Rr = len(BURST_TAPS) - 1
    s = _sharpen(BURST_TAPS, 1.0, 0.0)
    for x, y, w, h in ((32, 16, 112, 80), (0, 0, 112, 80), (656, 432, 112, 80)):
        pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
        assert pw.window.aligned == (x, y, w, h)
        pw.L.burst_set_sharpen(pw._h, ctypes.byref(s))
        img, _ = pw.process([f.to(DEV) for f in _frames()])
        got = img.cpu().numpy()
        pw.close()
        alone = S.sharpen(plain[y:y + h, x:x + w], BURST_TAPS, 1.0, 0.0)
        assert np.array_equal(got.view(np.uint32), alone.view(np.uint32)), (x, y)
        y0, x0 = (0 if y == 0 else Rr), (0 if x == 0 else Rr)
        y1, x1 = (h if y + h == 2 * H else h - Rr), (w if x + w == 2 * W else w - Rr)
        crop = want_f[y:y + h, x:x + w]
        assert np.array_equal(got[y0:y1, x0:x1].view(np.uint32), crop[y0:y1, x0:x1].view(np.uint32)), (x, y)
        assert not np.array_equal(got.view(np.uint32), crop.view(np.uint32)), (x, y)


# ---- 7. streams -------------------------------------------------------------------------------------------------------------
def test_frame_stream_sharpens_its_outputs():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream
    frames = [f.to(DEV) for f in _frames()[:3]]
    st = FrameStream(_config(frames=3), 1, DEV, render=dict(format=capi.OUT_RGB8, **RENDER), sharpen=SHARPEN)
    outs = {}
    for f in frames:
        r = st.push(f)
        if r is not None:
            outs[r[0]] = r[1].clone()
    torch.cuda.synchronize()
    st.close()
    assert sorted(outs) == [0, 1] and outs[1].dtype == torch.uint8 and tuple(outs[1].shape) == (2 * H, 2 * W, 3)
    ref = BurstPipeline(_config(frames=3, reference=1), DEV)      # output 1 = frames [0, 2] around reference 1
    ref.set_render(capi.OUT_RGB8, **RENDER)
    ref.set_sharpen(**SHARPEN)
    _, q = ref.process(frames)
    assert torch.equal(q, outs[1])
    ref.set_render(None)
    ref.set_sharpen(None)
    lin, _ = ref.process(frames)
    assert np.array_equal(_np(outs[1]), S.sharpen_render(lin.cpu().numpy(), BURST_TAPS, 1.0, 0.0, R.RGB8, CCM, LUT)[1])
    ref.close()
    # a windowed stream grows its window as BurstPipeline does: the rectangle is the crop of the whole-frame output
    x, y, w, h = 40, 24, 100, 60
    sw = FrameStream(_config(frames=3), 1, DEV, window=(x, y, w, h), render=dict(format=capi.OUT_RGB8, **RENDER), sharpen=SHARPEN)
    wouts = {}
    for f in frames:
        r = sw.push(f)
        if r is not None:
            wouts[r[0]] = r[1].clone()
    torch.cuda.synchronize()
    sw.close()
    assert tuple(wouts[1].shape) == (h, w, 3) and torch.equal(wouts[1], outs[1][y:y + h, x:x + w])


# ---- 8. between bursts only -------------------------------------------------------------------------------------------------
def test_set_sharpen_is_refused_while_a_frame_is_pending():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    assert pipe.group_size() > 1
    set_sharpen = capi.lib().raw["mfsr_burst_set_sharpen"]
    s = _sharpen(BURST_TAPS)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    pipe.add_frame(frames[0], True)              # waits for the rest of its group
    assert set_sharpen(pipe._h, ctypes.byref(s)) == -1 and set_sharpen(pipe._h, None) == -1
    with pytest.raises(capi.MfsrError):
        pipe.set_sharpen(**SHARPEN)
    for f in frames[1:]:
        pipe.add_frame(f)
    img, _ = pipe.finish()
    assert np.array_equal(img.cpu().numpy().view(np.uint32), _plain_float().view(np.uint32))   # the refused calls changed nothing
    assert set_sharpen(pipe._h, ctypes.byref(s)) == 0 and set_sharpen(pipe._h, None) == 0
    bad = _sharpen(BURST_TAPS, amount=17.0)
    assert set_sharpen(pipe._h, ctypes.byref(bad)) == -1
    pipe.close()


# ---- 9. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_sharpens_inside_the_finish(tmp_path):
    """MFSR_SHARPEN on the bundled burst: _sr_result is exactly the RGB8 image the Python pipeline renders with the same
    configuration and the same sharpen description (the CLI cannot dump its float image), with and without MFSR_CCM; it differs
    from the unsharpened one; _sr2_result is still produced; bad values and MFSR_GPUS > 1 are refused with a message."""
    import shutil
    from PIL import Image
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    from tests.test_bundled_burst import CITY, _cfg, _raws
    cli = os.path.join(ROOT, "apps", "multi_frame_sr")
    assert os.path.exists(cli), "build apps/multi_frame_sr first (__graft_entry__.build())"
    swap = [0, 0, 1, 0, 1, 0, 1, 0, 0]
    outs = {}
    for name, env in (("plain", {}), ("sharp", {"MFSR_SHARPEN": "1.0"}), ("full", {"MFSR_SHARPEN": "1.5,0.8,2,0.002"}),
                      ("ccm", {"MFSR_SHARPEN": "1.0", "MFSR_CCM": ",".join(str(v) for v in swap)})):
        d = tmp_path / name
        d.mkdir()
        for i in range(5):
            shutil.copy(os.path.join(CITY, f"img_{i:06d}.png"), d / f"img_{i:06d}.png")
        e = dict(os.environ, **env)
        if "MFSR_CCM" not in env:
            e.pop("MFSR_CCM", None)
        if "MFSR_SHARPEN" not in env:
            e.pop("MFSR_SHARPEN", None)
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=d, capture_output=True, text=True, timeout=300, env=e)
        assert p.returncode == 0, p.stderr
        outs[name] = np.asarray(Image.open(d / "city_farneback_sr_result.png"))
        assert np.asarray(Image.open(d / "city_farneback_sr2_result.png")).shape == outs[name].shape
    assert not np.array_equal(outs["sharp"], outs["plain"]) and not np.array_equal(outs["full"], outs["sharp"])
    raws, w, h = _raws(5)
    cfg = _cfg(w, h, 5)
    cfg.preAlign = 1
    cfg.lkIterations = 3
    pipe = BurstPipeline(cfg, DEV)
    frames = [torch.from_numpy(r.view(np.int16)).to(DEV) for r in raws]
    for name, sharpen, matrix in (("sharp", dict(amount=1.0), None), ("full", dict(amount=1.5, sigma=0.8, radius=2, threshold=0.002), None),
                                  ("ccm", dict(amount=1.0), swap)):
        pipe.set_render(capi.OUT_RGB8, matrix=matrix)
        pipe.set_sharpen(**sharpen)
        _, q = pipe.process(frames)
        got = q.cpu().numpy()
        bad = np.argwhere(got != outs[name])
        print(f"CLI {name}: {len(bad)} samples differ from the Python pipeline's" + (
            f", first at {bad[0].tolist()}, last at {bad[-1].tolist()}, max difference "
            f"{int(np.abs(got.astype(int) - outs[name].astype(int)).max())}" if len(bad) else ""))
        assert np.array_equal(got, outs[name]), name
    pipe.close()
    for bad in ("", "x", "1,", "1,,2", "1,1,5", "1,1,1.5", "1,1,1,0,3", "17", "1,0", "1,1,1,-1", "nan"):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, MFSR_SHARPEN=bad))
        assert p.returncode != 0 and "MFSR_SHARPEN" in p.stderr, bad
    p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, MFSR_SHARPEN="1.0", MFSR_GPUS="2"))
    assert p.returncode != 0 and "MFSR_SHARPEN is not supported with MFSR_GPUS > 1" in p.stderr
