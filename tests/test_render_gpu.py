"""The rendered finish on the device: k_renderImage against the numpy restatement of tests/render_ref.py
bit for bit, k_finishRendered against the two-launch chain, and rendered bursts (resident, unfused, windowed, striped, host,
captured, streamed, CLI) against the restatement applied to the plain float image of the same pipeline.  Only the built-in
gamma (powf) has a tolerance: one LSB of the format (section 3.1)."""
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
from tests.kernels import guarded_upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CANARY = 0xA5
FORMATS = (R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2)
NAMES = {R.RGB16: "RGB16", R.RGB8: "RGB8", R.RGBA8: "RGBA8", R.RGB10A2: "RGB10A2"}
# a camera -> display matrix with negative off-diagonals; every row has a positive coefficient
CCM = np.array([1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56], np.float32)
LUTS = {"none": None, "srgb4096": R.srgb_lut(4096), "five": np.array([0.1, 0.9, -0.2, 1.3, 0.5], np.float32)}


def _struct(fmt, m=None, lut_dev=None):
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
    """random values around [0, 1] with NaN, +-inf, negatives, values above 1 (and above 65536 for the matrix) and exact
    knots k/4096 and k/4 of the two tables at fixed strides"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.25, 1.25, h * w * 3).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, -3.0, 2.5, 70000.0, 300.0, 0.0, 1.0, 0.25, 0.5, 0.75, 1000 / 4096, 4095 / 4096,
                        1 / 4096, 0.0031308, 1e-8], np.float32)
    idx = np.arange(0, p.size, 5)
    p[idx] = special[np.arange(idx.size) % special.size]
    return p.reshape(h, w, 3)


def _expected_bytes(packed, off, row_bytes, h):
    """the whole output allocation: `off` canary bytes, then h rows of row_bytes of which the dense part is written"""
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


# ---- 1. the pixel body on its own -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_renderImage_equals_the_restatement(fmt):
    L = capi.lib()
    luts = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in LUTS.items()}
    n = 0
    for w, h in itertools.product((1, 2, 3, 4, 5, 7, 63, 64, 65, 130), (1, 3)):
        p = _pixels(h, w, 100 * w + h)
        d_in, check_in = guarded_upload(p)
        for use_m, lut_name in itertools.product((False, True), LUTS):
            m = CCM if use_m else None
            want_f, want_q = R.render(p, fmt, m, LUTS[lut_name])
            r = _struct(fmt, m, luts[lut_name])
            for off, rb in _layouts(fmt, w):
                d_out, check_out = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
                d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
                L.renderImage(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_out.data_ptr() + off, rb, w, h, ctypes.byref(r), 0, None)
                what = f"{NAMES[fmt]} {w}x{h} matrix={use_m} lut={lut_name} offset={off} rowBytes={rb}"
                check_out(what)
                check_f(what)
                assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, off, rb, h)), what
                assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), what + " (float image)"
                n += 1
        check_in(f"{NAMES[fmt]} {w}x{h}", unchanged=True)
    assert n == 20 * 6 * len(_layouts(fmt, 8))


def test_renderImage_in_place_and_without_an_integer_output():
    L = capi.lib()
    w, h, pitch = 65, 3, 12 * 65 + 8
    p = _pixels(h, w, 5)
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    want_f, want_q = R.render(p, R.RGB8, CCM, LUTS["srgb4096"])
    rows = np.full((h, pitch), CANARY, np.uint8)
    rows[:, :12 * w] = p.view(np.uint8).reshape(h, 12 * w)
    r = _struct(R.RGB8, CCM, lut)
    for with_out in (True, False):
        d_img, check_img = guarded_upload(rows)
        d_out, check_out = guarded_upload(np.full(3 * w * h, CANARY, np.uint8))
        L.renderImage(d_img.data_ptr(), pitch, d_img.data_ptr(), pitch, d_out.data_ptr() if with_out else None, 3 * w, w, h,
                      ctypes.byref(r), 0, None)
        check_img("in place")
        check_out("in place")
        got = d_img.cpu().numpy()
        assert np.array_equal(got[:, :12 * w].copy().view(np.uint32).reshape(h, w, 3), want_f.view(np.uint32))
        assert (got[:, 12 * w:] == CANARY).all()
        want_bytes = _expected_bytes(want_q, 0, 3 * w, h) if with_out else np.full(3 * w * h, CANARY, np.uint8)
        assert np.array_equal(d_out.cpu().numpy(), want_bytes)


@pytest.mark.parametrize("how", ["lds", "cache"])
def test_renderImage_lut_in_lds_and_through_the_cache_give_the_same_bytes(monkeypatch, how):
    """MFSR_RENDER_LUT=lds | cache (read at every call) forces one way of reading the tone table for every format; unset, RGB8
    stages tables of up to 8192 intervals in LDS (64 x 16 workgroups) and the other formats read through the cache, which is
    what every other test here runs.  Both give the restatement's bytes; a table too long for LDS (65536 intervals) is read
    through the cache either way."""
    L = capi.lib()
    w, h = 130, 37
    p = _pixels(h, w, 9)
    d_in, _ = guarded_upload(p)
    monkeypatch.setenv("MFSR_RENDER_LUT", how)
    for n, fmt in ((4096, R.RGB8), (4, R.RGB10A2), (8192, R.RGB16), (65536, R.RGBA8), (65536, R.RGB8), (1, R.RGB8)):
        table = R.srgb_lut(n)
        lut = torch.from_numpy(table).to(DEV)
        want_f, want_q = R.render(p, fmt, CCM, table)
        rb = R.row_bytes(fmt, w)
        d_out, check_out = guarded_upload(np.full(rb * h, CANARY, np.uint8))
        d_f, check_f = guarded_upload(np.zeros((h, w, 3), np.float32))
        r = _struct(fmt, CCM, lut)
        L.renderImage(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_out.data_ptr(), rb, w, h, ctypes.byref(r), 0, None)
        check_out(f"{how} {n}")
        check_f(f"{how} {n}")
        assert np.array_equal(d_out.cpu().numpy(), _expected_bytes(want_q, 0, rb, h)), (how, n)
        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (how, n)


# ---- 2. the built-in gamma --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_renderImage_builtin_gamma_within_one_lsb(fmt):
    """applyGamma = 1 without a table: powf is the only inexact operation, so at most 1 LSB of the format against numpy's pow
    (DESIGN.md section 3.1), and nothing differs on the linear segment (inputs <= 0.0031308)."""
    L = capi.lib()
    w, h = 130, 3
    p = _pixels(h, w, 77)
    lin = p.reshape(-1)[1::5]                  # (a view) every fifth value on the linear segment
    lin[:] = np.random.default_rng(3).uniform(0, 0.0031308, lin.size).astype(np.float32)
    d_in, _ = guarded_upload(p)
    rb = R.row_bytes(fmt, w)
    d_out, check_out = guarded_upload(np.full(rb * h, CANARY, np.uint8))
    r = _struct(fmt)
    L.renderImage(d_in.data_ptr(), 12 * w, None, 0, d_out.data_ptr(), rb, w, h, ctypes.byref(r), 1, None)
    check_out("gamma")
    got = d_out.cpu().numpy().reshape(h, rb)
    want = R.quantise(R.gamma(p), fmt)
    if fmt == R.RGB10A2:
        d = np.ascontiguousarray(got).view(np.uint32).reshape(h, w).astype(np.int64)
        got_q = np.stack([d & 1023, d >> 10 & 1023, d >> 20 & 1023], axis=-1)
        assert (d >> 30 == 3).all()
    elif fmt == R.RGB16:
        got_q = np.ascontiguousarray(got).view(np.uint16).reshape(h, w, 3).astype(np.int64)
    else:
        px = got.reshape(h, w, -1).astype(np.int64)
        got_q = px[..., :3]
        assert fmt == R.RGB8 or (px[..., 3] == 255).all()
    diff = np.abs(got_q - want)
    with np.errstate(invalid="ignore"):
        linear = ~(p > np.float32(0.0031308))      # NaN and negatives included: they clamp to 0
    print(f"{NAMES[fmt]}: max difference {diff.max()} LSB, {int((diff > 0).sum())} of {diff.size} samples differ")
    assert diff.max() <= 1
    assert diff[linear].max() == 0


# ---- 3. the fused kernel against the chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_finishRendered_equals_the_chain(fmt):
    """mfsr_finishFusedWindow (float image, no gamma) + mfsr_renderImage against the one launch, whole (130 x 37) and as the
    window (16, 16, 64 x 16) of it.  Weights: the left 64 columns of rows 0..19 are all above the threshold (those waves skip
    the fallback resample), a checkerboard of sub-threshold weights elsewhere (those take it)."""
    L = capi.lib()
    W, H, fbW, fbH, thr = 130, 37, 65, 19, 1e-3
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
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    r = _struct(fmt, CCM, lut)
    rb = R.row_bytes(fmt, W)
    # the chain
    d_lin, _ = guarded_upload(np.zeros((H, W, 3), np.float32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * W, None, W, H, thr, 0, 65535.0, 0, 0, W, H, None)
    d_cf, _ = guarded_upload(np.zeros((H, W, 3), np.float32))
    d_cq, _ = guarded_upload(np.full(rb * H, CANARY, np.uint8))
    L.renderImage(d_lin.data_ptr(), 12 * W, d_cf.data_ptr(), 12 * W, d_cq.data_ptr(), rb, W, H, ctypes.byref(r), 0, None)
    chain_f, chain_q = d_cf.cpu().numpy(), d_cq.cpu().numpy().reshape(H, rb)
    # the restatement agrees with the chain (so the comparison below is not of two equal mistakes)
    ref_f, ref_q = R.render(d_lin.cpu().numpy(), fmt, CCM, LUTS["srgb4096"])
    assert np.array_equal(chain_f.view(np.uint32), ref_f.view(np.uint32)) and np.array_equal(chain_q, R.as_bytes(ref_q))
    # one launch, whole image
    d_f, cf = guarded_upload(np.zeros((H, W, 3), np.float32))
    d_q, cq = guarded_upload(np.full(rb * H, CANARY, np.uint8))
    L.finishRendered(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                     d_f.data_ptr(), 12 * W, d_q.data_ptr(), rb, ctypes.byref(r), W, H, thr, 0, 0, 0, W, H, None)
    cf("whole")
    cq("whole")
    assert np.array_equal(d_f.cpu().numpy().view(np.uint32), chain_f.view(np.uint32))
    assert np.array_equal(d_q.cpu().numpy().reshape(H, rb), chain_q)
    # the window: pointers of its first pixel, the whole image's pitch; dense output rows of the window's width
    x0, y0, w, h = 16, 16, 64, 16
    wrb = R.row_bytes(fmt, w)
    d_wf, cwf = guarded_upload(np.zeros((h, w, 3), np.float32))
    d_wq, cwq = guarded_upload(np.full(wrb * h, CANARY, np.uint8))
    o = 12 * (y0 * W + x0)
    L.finishRendered(d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * W, d_fb.data_ptr(), 12 * fbW, fbW, fbH, 0.0, 1.0, 0.0, 1.0,
                     d_wf.data_ptr(), 12 * w, d_wq.data_ptr(), wrb, ctypes.byref(r), w, h, thr, 0, x0, y0, W, H, None)
    cwf("window")
    cwq("window")
    bpp = R.BYTES_PER_PIXEL[fmt]
    assert np.array_equal(d_wf.cpu().numpy().view(np.uint32), chain_f[y0:y0 + h, x0:x0 + w].view(np.uint32))
    assert np.array_equal(d_wq.cpu().numpy().reshape(h, wrb), chain_q[y0:y0 + h, bpp * x0:bpp * (x0 + w)])
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
    """a tensor typed for a format as the restatement's array"""
    a = t.cpu().numpy()
    return a.view({np.dtype(np.int16): np.uint16, np.dtype(np.int32): np.uint32}.get(a.dtype, a.dtype))


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
    key = ("want", fmt, bits, fused)
    if key not in _cache:
        _cache[key] = R.render(_plain_float(bits, fused), fmt, CCM, LUTS["srgb4096"])
    return _cache[key]


# ---- 4. off is off ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [0, 1])
def test_render_off_is_off(gamma):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    ref = BurstPipeline(_config(gamma), DEV)
    f0, q0 = (t.clone() for t in ref.process(frames))
    ref.close()
    for how in ("null", "rgb16"):
        pipe = BurstPipeline(_config(gamma), DEV)
        if how == "null":
            pipe.set_render(None)
        else:
            pipe.set_render(capi.OUT_RGB16)
        f1, q1 = pipe.process(frames)
        assert q1.dtype == torch.int16 and torch.equal(q1, q0), how
        assert torch.equal(f1.view(torch.int32), f0.view(torch.int32)), how
        if how == "rgb16":      # and off again on the same pipeline
            pipe.set_render(None)
            f2, q2 = pipe.process(frames)
            assert torch.equal(q2, q0) and torch.equal(f2.view(torch.int32), f0.view(torch.int32))
        pipe.close()


# ---- 5. rendered resident bursts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 0])
def test_rendered_burst_equals_the_restatement_of_the_plain_float_image(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(fused=fused), DEV)
    shapes = {R.RGB16: (2 * H, 2 * W, 3), R.RGB8: (2 * H, 2 * W, 3), R.RGBA8: (2 * H, 2 * W, 4), R.RGB10A2: (2 * H, 2 * W)}
    dtypes = {R.RGB16: torch.int16, R.RGB8: torch.uint8, R.RGBA8: torch.uint8, R.RGB10A2: torch.int32}
    for fmt in FORMATS:
        pipe.set_render(fmt, **RENDER)
        img, q = pipe.process(frames)
        want_f, want_q = _want(fmt, fused=fused)
        assert q.dtype == dtypes[fmt] and tuple(q.shape) == shapes[fmt]
        assert np.array_equal(_np(q), want_q), (NAMES[fmt], fused)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (NAMES[fmt], fused)
    pipe.close()


@pytest.mark.parametrize("fmt", [R.RGB8, R.RGB10A2], ids=NAMES.get)
def test_rendered_zoom_window_is_the_crop(fmt):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    x, y, w, h = 243, 97, 155, 110          # any rectangle: the library works on the 16-pixel window around it
    pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
    pw.set_render(fmt, **RENDER)
    img, q = pw.process([f.to(DEV) for f in _frames()])
    want_f, want_q = _want(fmt)
    assert np.array_equal(_np(q), want_q[y:y + h, x:x + w])
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f[y:y + h, x:x + w].view(np.uint32))
    pw.close()


def test_rendered_finish_rows_into_one_rgb8_buffer():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
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
    assert done.all()
    pipe.close()


# ---- 6. rendered host bursts ------------------------------------------------------------------------------------------------
def _guarded_host(like):
    """a pinned host image typed like `like` between two canary bands: (image view, check)"""
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
    out_host, check = _guarded_host(pipe.out16)
    for rep in range(3):
        out_host.view(torch.uint8).fill_(0)
        got = pipe.process_host(host, out16_host=out_host)
        pipe.host_sync()
        assert np.array_equal(_np(got), want_q), (what, rep)
        check(what)
    pipe.close()


@pytest.mark.parametrize("fmt", [R.RGB8, R.RGB10A2], ids=NAMES.get)
def test_rendered_host_burst_equals_the_resident_one(fmt):
    host = [f.pin_memory() for f in _frames()]
    _three_host_bursts(_config(ring=4), fmt, host, _want(fmt)[1], NAMES[fmt])


def test_rendered_host_burst_from_packed_frames():
    host = [p.pin_memory() for p in synth.pack_raw(_frames(10), capi.PACK_MIPI10)]
    _three_host_bursts(_config(ring=4, packing=capi.PACK_MIPI10, bits=10), R.RGB8, host, _want(R.RGB8, bits=10)[1], "MIPI10 in, RGB8 out")


_ONE_BAND_CHILD = """
import torch
from tests import test_render_gpu as T
from tests import render_ref as R
host = [f.pin_memory() for f in T._frames()]
for fmt in (R.RGB8, R.RGB10A2):
    T._three_host_bursts(T._config(ring=4), fmt, host, T._want(fmt)[1], "one band")
print("ONE-BAND-OK")
"""


def test_rendered_host_burst_in_one_band():
    """MFSR_HOST_BANDS is read once per process: a child process with MFSR_HOST_BANDS=1 (the whole-image finish and one download;
    the default of 8 bands is what the tests above run)."""
    env = dict(os.environ, MFSR_HOST_BANDS="1")
    r = subprocess.run([sys.executable, "-c", _ONE_BAND_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ONE-BAND-OK" in r.stdout, r.stdout + r.stderr


def test_rendered_host_burst_captured_as_a_graph():
    """What tests/test_packed_gpu.py does before a capture: one eager burst, host_sync and a device synchronisation; then the
    burst is captured on fixed pinned buffers and replayed on two bursts' data."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    bursts = [_frames(), _frames(seed=31)]
    pipe = BurstPipeline(_config(ring=4, async_fuse=0), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    eager = []
    for frames in bursts:
        got = pipe.process_host([f.pin_memory() for f in frames])
        pipe.host_sync()
        eager.append(got.clone())
    pipe.close()
    assert np.array_equal(_np(eager[0]), _want(R.RGB8)[1]) and not torch.equal(eager[0], eager[1])
    static = [torch.empty_like(f).pin_memory() for f in bursts[0]]
    for dst, src in zip(static, bursts[0]):
        dst.copy_(src)
    gpipe = BurstPipeline(_config(ring=4, async_fuse=0), DEV)
    gpipe.set_render(capi.OUT_RGB8, **RENDER)
    out_host, check = _guarded_host(gpipe.out16)
    gpipe.process_host(static, out16_host=out_host)
    gpipe.host_sync()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g8 = gpipe.process_host(static, out16_host=out_host)
    for k in (1, 0):
        for dst, src in zip(static, bursts[k]):
            dst.copy_(src)
        g8.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g8, eager[k]), f"burst {k}: graph replay differs from the eager rendered host burst"
        check("graph replay")
    del graph
    gpipe.close()


# ---- 7. streams -------------------------------------------------------------------------------------------------------------
def test_frame_stream_renders_its_windows():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream
    frames = [f.to(DEV) for f in _frames()[:3]]
    st = FrameStream(_config(frames=3), 1, DEV, render=dict(format=capi.OUT_RGB8, **RENDER))
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
    _, q = ref.process(frames)
    assert torch.equal(q, outs[1])
    ref.set_render(None)
    lin, _ = ref.process(frames)
    assert np.array_equal(_np(outs[1]), R.render(lin.cpu().numpy(), R.RGB8, CCM, LUTS["srgb4096"])[1])
    ref.close()


# ---- 8. between bursts only -------------------------------------------------------------------------------------------------
def test_set_render_is_refused_while_a_frame_is_pending():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    assert pipe.group_size() > 1
    set_render = capi.lib().raw["mfsr_burst_set_render"]
    r = _struct(capi.OUT_RGB8, CCM)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    pipe.add_frame(frames[0], True)              # waits for the rest of its group
    assert set_render(pipe._h, ctypes.byref(r)) == -1 and set_render(pipe._h, None) == -1
    with pytest.raises(capi.MfsrError):
        pipe.set_render(capi.OUT_RGB8)
    for f in frames[1:]:
        pipe.add_frame(f)
    _, q16 = pipe.finish()
    assert q16.dtype == torch.int16              # the refused calls changed nothing
    assert set_render(pipe._h, ctypes.byref(r)) == 0 and set_render(pipe._h, None) == 0
    bad = _struct(7)
    assert set_render(pipe._h, ctypes.byref(bad)) == -1
    pipe.close()


# ---- 9. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_colour_matrix(tmp_path):
    import shutil
    from PIL import Image
    from tests.test_bundled_burst import CITY
    cli = os.path.join(ROOT, "apps", "multi_frame_sr")
    assert os.path.exists(cli), "build apps/multi_frame_sr first (__graft_entry__.build())"
    outs = {}
    for name, ccm in (("plain", None), ("identity", "1,0,0,0,1,0,0,0,1"), ("swap", "0,0,1,0,1,0,1,0,0")):
        d = tmp_path / name
        d.mkdir()
        for i in range(5):
            shutil.copy(os.path.join(CITY, f"img_{i:06d}.png"), d / f"img_{i:06d}.png")
        env = dict(os.environ)
        env.pop("MFSR_CCM", None)
        if ccm:
            env["MFSR_CCM"] = ccm
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=d, capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stderr
        outs[name] = [open(d / f"city_farneback_{k}_result.png", "rb").read() for k in ("sr", "sr2")]
        outs[name].append(np.asarray(Image.open(d / "city_farneback_sr_result.png")))
    assert outs["identity"][0] == outs["plain"][0] and outs["identity"][1] == outs["plain"][1]
    assert np.array_equal(outs["swap"][2], outs["plain"][2][..., ::-1]) and not np.array_equal(outs["swap"][2], outs["plain"][2])
    for bad in ("1,0,0,0,1,0,0,0", "1,0,0,0,1,0,0,0,1,0", "1,0,0,0,x,0,0,0,1", "1,0,0,0,nan,0,0,0,1", "300,0,0,0,1,0,0,0,1", ""):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path / "plain", capture_output=True, text=True, timeout=60,
                           env=dict(os.environ, MFSR_CCM=bad))
        assert p.returncode != 0 and "MFSR_CCM" in p.stderr, bad
