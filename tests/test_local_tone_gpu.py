"""Local tone mapping in the finish on the GPU: the statistics kernel against the numpy restatement
(tests/local_tone_ref.py) word for word, its column chunks and contention cases, additivity over stripes and windows, the slice
against the restatement bit for bit in every kernel form, identity, crops, in place, graph capture, bursts against the chain
restatement statistics -> library fit -> restatement slice, and the CLI."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi
from tests import local_tone_ref as T
from tests import render_ref as R
from tests.kernels import guarded_upload
from tests.test_image_stats_gpu import (FBH, FBW, FH, FW, THR, _config, _finish_inputs, _frames, _inputs_unchanged, _plain)
from tests.test_render_gpu import CCM, LUTS, _pixels, _struct

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
PAD_VALUE = 1.0e9     # what the bytes between a padded row's pixels and the next row hold: never read
CANARY = 0x5A
FORMATS = [R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2]
NAMES = {R.RGB16: "rgb16", R.RGB8: "rgb8", R.RGBA8: "rgba8", R.RGB10A2: "rgb10a2"}


def _lt(cell=16, bins=16, smooth=1, shadows=0.5, highlights=0.25, pivot=0.0, max_gain=4.0):
    lt = capi.LocalTone()
    lt.cell, lt.bins, lt.smooth = cell, bins, smooth
    lt.shadows, lt.highlights, lt.pivot, lt.maxGain = shadows, highlights, pivot, max_gain
    return lt


def _m(m):
    return None if m is None else (ctypes.c_float * 9)(*[float(v) for v in m])


def _table(shape, fill=0):
    """the device table between two guards, as an int64 tensor, and its check"""
    return guarded_upload(np.full(shape, fill, np.int64))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _upload(p, pad_floats):
    """the image on the device with rows of 12 w + 4 pad_floats bytes -> (tensor, row bytes, check)"""
    h, w = p.shape[:2]
    rows = np.full((h, 3 * w + pad_floats), PAD_VALUE, np.float32)
    rows[:, :3 * w] = p.reshape(h, 3 * w)
    d, check = guarded_upload(rows)
    return d, 4 * (3 * w + pad_floats), check


def _diff(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return f"{bad.size} words differ, first {bad[:6]}: got {got.reshape(-1)[bad[:6]]}, want {want.reshape(-1)[bad[:6]]}"


def _image_stats(d_in, rb, w, h, lt, m, d_t, offset=(0, 0), full=None, stream=None):
    fw, fh = (w, h) if full is None else full
    capi.lib().toneGridStats(d_in.data_ptr() if hasattr(d_in, "data_ptr") else d_in, rb, w, h, offset[0], offset[1], fw, fh, _m(m),
                             ctypes.byref(lt), d_t.data_ptr(), stream)


def _run_stats(p, cell, bins_list=(4, 32), pads=(0, 1)):
    """mfsr_toneGridStats of p for every (NZ, matrix, padding) against the restatement; returns the number of launches"""
    h, w = p.shape[:2]
    n = 0
    ups = [_upload(p, pad) for pad in pads]
    for bins, use_m in itertools.product(bins_list, (False, True)):
        m = CCM if use_m else None
        want = T.stats(p, cell, bins, m)
        lt = _lt(cell, bins)
        for d_in, rb, _ in ups:
            d_t, check_t = _table(want.shape)
            _image_stats(d_in, rb, w, h, lt, m, d_t)
            what = f"{w}x{h} C={cell} NZ={bins} matrix={use_m} rowBytes={rb}"
            check_t(what)
            got = _host(d_t)
            assert np.array_equal(got, want), what + ": " + _diff(got, want)
            n += 1
    for (_, rb, check_in) in ups:
        check_in(f"{w}x{h} rowBytes={rb}", unchanged=True)
    return n


# ---- 1. the statistics kernel against the restatement ---------------------------------------------------------------------------
def test_toneGridStats_equals_the_restatement_on_small_images():
    """a padded pitch of 12 w + 4 bytes: rows that are not 16-byte aligned (and with no padding, rows whose alignment changes
    from one to the next unless w is a multiple of 4)"""
    n = 0
    for w, h in itertools.product((1, 3, 4, 5, 63, 65, 257), (1, 17, 33)):
        n += _run_stats(_pixels(h, w, 1000 * w + h), 16)
    assert n == 21 * 8


def test_toneGridStats_column_chunks():
    """4100 x 20 with C = 16 and NZ = 32: GX = 257 cells, three chunks of 128; and two windows whose seam is in no chunk's
    first cell add up to the whole"""
    w, h = 4100, 20
    p = _pixels(h, w, 41)
    assert _run_stats(p, 16, bins_list=(32,), pads=(0,)) == 2
    lt = _lt(16, 32)
    want = T.stats(p, 16, 32, CCM)
    d_t, check_t = _table(want.shape)
    for x0, ww in ((0, 2040), (2040, w - 2040)):
        d_in, check_in = guarded_upload(np.ascontiguousarray(p[:, x0:x0 + ww]))
        _image_stats(d_in, 12 * ww, ww, h, lt, CCM, d_t, (x0, 0), (w, h))
        check_in("window", unchanged=True)
    check_t("two windows")
    assert np.array_equal(_host(d_t), want), _diff(_host(d_t), want)


def test_toneGridStats_over_many_workgroups_with_row_blocks_below_a_cell():
    """1500 x 300 at C = 64: the host cuts the rows of a cell row into blocks of 8, so several workgroups add to one entry"""
    assert _run_stats(_pixels(300, 1500, 77), 64, bins_list=(16,), pads=(0,)) == 2


@pytest.mark.parametrize("kind", ["constant", "two_valued", "nan"])
def test_toneGridStats_contention(kind):
    h, w = 64, 512
    p = np.empty((h, w, 3), np.float32)
    if kind == "constant":
        p[:] = np.array([0.5, 0.25, 0.75], np.float32)
    elif kind == "two_valued":      # neighbouring pixels differ: both bins in every lane
        p[:] = np.array([0.2, 0.21, 0.19], np.float32)
        p[:, 1::2] = np.array([0.8, 0.79, 0.81], np.float32)
    else:
        p[:] = np.nan
    want = T.stats(p, 16, 32)
    assert np.count_nonzero(want[..., 0]) == (2 if kind == "two_valued" else 1) * 4 * 32
    assert _run_stats(p, 16) == 8


# ---- 2. the finish form -------------------------------------------------------------------------------------------------------
def _finish_stats(table, lt, m, x0=0, y0=0, w=FW, h=FH, stream=None):
    (d_fin, _), (d_wt, _), (d_fb, _) = _finish_inputs()
    o = 12 * (y0 * FW + x0)
    capi.lib().finishToneGridStats(d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * FW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0,
                                   0.0, 1.0, w, h, THR, x0, y0, FW, FH, _m(m), ctypes.byref(lt), table.data_ptr(), stream)


_lin = {}


def _linear_image():
    """the float image the plain finish writes of the shared finish inputs (no gamma): computed once"""
    if not _lin:
        (d_fin, _), (d_wt, _), (d_fb, _) = _finish_inputs()
        d_lin, check_lin = guarded_upload(np.zeros((FH, FW, 3), np.float32))
        capi.lib().finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * FW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0,
                                     1.0, d_lin.data_ptr(), 12 * FW, None, FW, FH, THR, 0, 65535.0, 0, 0, FW, FH, None)
        check_lin("float image")
        _lin["dev"], _lin["host"] = d_lin, d_lin.cpu().numpy().copy()
    return _lin["dev"], _lin["host"]


@pytest.mark.parametrize("use_m,bins", [(False, 4), (True, 32)])
def test_finishToneGridStats_equals_the_image_form_of_the_float_image(use_m, bins):
    d_lin, lin = _linear_image()
    m, lt = (CCM if use_m else None), _lt(16, bins)
    want = T.stats(lin, 16, bins, m)
    d_a, check_a = _table(want.shape)
    _image_stats(d_lin, 12 * FW, FW, FH, lt, m, d_a)
    d_b, check_b = _table(want.shape)
    _finish_stats(d_b, lt, m)
    check_a("image form")
    check_b("finish form")
    assert np.array_equal(_host(d_a), want), _diff(_host(d_a), want)        # (not a comparison of two equal mistakes)
    assert np.array_equal(_host(d_b), want), _diff(_host(d_b), want)
    _inputs_unchanged("finishToneGridStats")


def test_finishToneGridStats_stripes_and_windows_add_up_and_a_launch_adds():
    lt = _lt(16, 8)
    shape = (3, 9, 8, 2)
    d_whole, check_whole = _table(shape)
    _finish_stats(d_whole, lt, CCM)
    whole = _host(d_whole)
    assert int(whole[..., 0].sum()) == FW * FH
    for rows in (1, 7, 16):
        d_t, check_t = _table(shape)
        for y in range(0, FH, rows):
            _finish_stats(d_t, lt, CCM, 0, y, FW, min(rows, FH - y))
        check_t(f"stripes of {rows}")
        assert np.array_equal(_host(d_t), whole), f"stripes of {rows}: " + _diff(_host(d_t), whole)
    # the 64 x 16 window at (16, 16) and the four rectangles around it
    d_t, check_t = _table(shape)
    for x0, y0, w, h in ((16, 16, 64, 16), (0, 0, FW, 16), (0, 32, FW, FH - 32), (0, 16, 16, 16), (80, 16, FW - 80, 16)):
        _finish_stats(d_t, lt, CCM, x0, y0, w, h)
    check_t("window split")
    assert np.array_equal(_host(d_t), whole), _diff(_host(d_t), whole)
    # a second launch on the whole's table adds the window's
    d_win, _ = _table(shape)
    _finish_stats(d_win, lt, CCM, 16, 16, 64, 16)
    _finish_stats(d_whole, lt, CCM, 16, 16, 64, 16)
    check_whole("second launch")
    assert np.array_equal(_host(d_whole), whole + _host(d_win))
    d_t, check_t = _table(shape, fill=5)
    _finish_stats(d_t, lt, CCM)
    check_t("non-zero table")
    assert np.array_equal(_host(d_t), whole + np.uint64(5))
    _inputs_unchanged("additivity")


# ---- 3. the slice against the restatement -------------------------------------------------------------------------------------
FULL_W, FULL_H, CELL = 300, 40, 16
OFFSETS = ((0, 0), (16, 5), (32, 3))
_slice = {}


def _grid(bins):
    """random gains in [0.25, 4] for the FULL_W x FULL_H frame: (host [GY, GX, NZ], device), uploaded once, checked unchanged"""
    if ("grid", bins) not in _slice:
        gx, gy, _ = T.grid_size(FULL_W, FULL_H, CELL, bins)
        g = np.random.default_rng(bins).uniform(0.25, 4.0, (gy, gx, bins)).astype(np.float32)
        _slice["grid", bins] = (g,) + guarded_upload(g)
    return _slice["grid", bins]


def _slice_pixels(h, w, seed):
    p = _pixels(h, w, seed)
    flat = p.reshape(-1, 3)
    flat[0] = 0.0                                        # luma exactly 0
    flat[-1] = 1.0                                       # ... and exactly 1
    if flat.shape[0] > 4:
        flat[2] = np.array([np.nan, 0.5, 0.25], np.float32)
        flat[3] = np.array([0.5, np.inf, 0.25], np.float32)
    return p


def _applied(h, w, ox, oy, use_m, bins):
    """(the pixels, the restatement's p g) of one shape, offset and matrix: computed once, shared by the formats and forms"""
    key = ("applied", h, w, ox, oy, use_m, bins)
    if key not in _slice:
        p = _slice_pixels(h, w, 100 * w + h + ox)
        _slice[key] = (p, T.apply(p, _grid(bins)[0], CELL, CCM if use_m else None, (ox, oy)))
    return _slice[key]


def _out_layout(fmt, w):
    """(offset of the first byte, row bytes): RGB8 rows start on odd bytes and are an odd number of bytes apart"""
    if fmt == R.RGB8:
        return 1, 3 * w + 1 + (w & 1)
    if fmt == R.RGB16:
        return 2, 6 * w + 2
    return 4, 4 * w + 4


def _expected_bytes(packed, off, row_bytes, h):
    dense = R.as_bytes(packed)
    want = np.full(off + row_bytes * h, CANARY, np.uint8)
    rows = want[off:].reshape(h, row_bytes)
    rows[:, :dense.shape[1]] = dense
    return want


def _tone_cases():
    """(name, table, applyGamma, MFSR_RENDER_LUT)"""
    return (("table_lds", "srgb4096", 0, "lds"), ("table_cache", "srgb4096", 0, "cache"), ("gamma", "none", 1, None),
            ("neither", "none", 0, None))


@pytest.mark.parametrize("grid_form", ["lds", "cache"])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_localToneImage_equals_the_restatement(monkeypatch, fmt, grid_form):
    L = capi.lib()
    monkeypatch.setenv("MFSR_LOCAL_TONE_GRID", grid_form)
    luts = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in LUTS.items()}
    n = 0
    for (w, h), (ox, oy), use_m in itertools.product(itertools.product((1, 5, 67, 259), (1, 9)), OFFSETS, (False, True)):
        bins = 32 if use_m else 8
        m = CCM if use_m else None
        lt = _lt(CELL, bins)
        _, d_grid, check_grid = _grid(bins)
        p, o = _applied(h, w, ox, oy, use_m, bins)
        d_in, check_in = guarded_upload(p)
        off, rb = _out_layout(fmt, w)
        for name, lut_name, gam, how in _tone_cases():
            if how:
                monkeypatch.setenv("MFSR_RENDER_LUT", how)
            else:
                monkeypatch.delenv("MFSR_RENDER_LUT", raising=False)
            want_f, want_q = R.render(o, fmt, m, LUTS[lut_name], bool(gam))
            r = _struct(fmt, m, luts[lut_name])
            d_out, check_out = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
            d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
            L.localToneImage(d_in.data_ptr(), 12 * w, d_f.data_ptr(), 12 * w, d_out.data_ptr() + off, rb, w, h, ctypes.byref(r), gam,
                             d_grid.data_ptr(), ctypes.byref(lt), ox, oy, FULL_W, FULL_H, None)
            what = f"{NAMES[fmt]} grid={grid_form} {w}x{h} at ({ox}, {oy}) matrix={use_m} tone={name}"
            check_out(what)
            check_f(what)
            got_q, got_f = d_out.cpu().numpy(), d_f.cpu().numpy()
            if gam:     # numpy's powf is not the device's: the reference is mfsr_renderImage of the restatement's p g, bit for bit
                d_o, check_o = guarded_upload(o)
                d_rq, check_rq = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
                d_rf, check_rf = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
                L.renderImage(d_o.data_ptr(), 12 * w, d_rf.data_ptr(), 12 * w, d_rq.data_ptr() + off, rb, w, h, ctypes.byref(r), gam, None)
                check_rq(what)
                check_rf(what)
                check_o(what, unchanged=True)
                assert np.array_equal(got_q, d_rq.cpu().numpy()), what
                assert np.array_equal(got_f.view(np.uint32), d_rf.cpu().numpy().view(np.uint32)), what + " (float image)"
                assert np.abs(got_q.astype(np.int64) - _expected_bytes(want_q, off, rb, h).astype(np.int64)).max() <= (
                    1 if fmt in (R.RGB8, R.RGBA8) else 255), what      # (and numpy's curve within one 8-bit code)
            else:
                assert np.array_equal(got_q, _expected_bytes(want_q, off, rb, h)), what
                assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)), what + " (float image)"
            n += 1
        check_in(f"{w}x{h}", unchanged=True)
        check_grid("grid", unchanged=True)
    assert n == 8 * 3 * 2 * 4


def test_localToneImage_in_place():
    L = capi.lib()
    w, h, pitch = 67, 9, 12 * 67 + 8
    p, o = _applied(h, w, 16, 5, True, 32)
    _, d_grid, check_grid = _grid(32)
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    want_f, want_q = R.render(o, R.RGB8, CCM, LUTS["srgb4096"])
    rows = np.full((h, pitch), CANARY, np.uint8)
    rows[:, :12 * w] = p.view(np.uint8).reshape(h, 12 * w)
    r, lt = _struct(R.RGB8, CCM, lut), _lt(CELL, 32)
    for with_out in (True, False):
        d_img, check_img = guarded_upload(rows)
        d_out, check_out = guarded_upload(np.full(3 * w * h, CANARY, np.uint8))
        L.localToneImage(d_img.data_ptr(), pitch, d_img.data_ptr(), pitch, d_out.data_ptr() if with_out else None, 3 * w, w, h,
                         ctypes.byref(r), 0, d_grid.data_ptr(), ctypes.byref(lt), 16, 5, FULL_W, FULL_H, None)
        check_img("in place")
        check_out("in place")
        got = d_img.cpu().numpy()
        assert np.array_equal(got[:, :12 * w].copy().view(np.uint32).reshape(h, w, 3), want_f.view(np.uint32))
        assert (got[:, 12 * w:] == CANARY).all()
        want_bytes = _expected_bytes(want_q, 0, 3 * w, h) if with_out else np.full(3 * w * h, CANARY, np.uint8)
        assert np.array_equal(d_out.cpu().numpy(), want_bytes)
    check_grid("grid", unchanged=True)


# ---- 4. the finish form of the slice -----------------------------------------------------------------------------------------
def _finish_local(fmt, grid_dev, lt, lut_dev, x0=0, y0=0, w=FW, h=FH, local=True, stream=None, outs=None):
    """mfsr_finishLocalTone (or mfsr_finishRendered) of a window of the shared finish inputs -> (bytes [h, rb], float image)"""
    (d_fin, _), (d_wt, _), (d_fb, _) = _finish_inputs()
    L = capi.lib()
    rb = R.row_bytes(fmt, w)
    if outs is None:
        d_out, check_out = guarded_upload(np.full((h, rb), CANARY, np.uint8))
        d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, np.float32))
    else:
        d_out, d_f = outs
    r = _struct(fmt, CCM, lut_dev)
    o = 12 * (y0 * FW + x0)
    head = (d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * FW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0, d_f.data_ptr(),
            12 * w, d_out.data_ptr(), rb, ctypes.byref(r), w, h, THR, 0, x0, y0, FW, FH)
    if local:
        L.finishLocalTone(*head, grid_dev.data_ptr(), ctypes.byref(lt), stream)
    else:
        L.finishRendered(*head, stream)
    if outs is None:
        check_out("finish")
        check_f("finish")
    return d_out, d_f


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_finishLocalTone_identity_restatement_and_crops(monkeypatch, fmt):
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    lt = _lt(16, 8)
    gx, gy, nz = T.grid_size(FW, FH, 16, 8)
    _, lin = _linear_image()
    # a grid of ones: mfsr_finishRendered's bytes and float image bit for bit, in both grid forms
    ones, check_ones = guarded_upload(np.ones((gy, gx, nz), np.float32))
    want_q, want_f = (t.cpu().numpy() for t in _finish_local(fmt, None, None, lut, local=False))
    for form in ("lds", "cache"):
        monkeypatch.setenv("MFSR_LOCAL_TONE_GRID", form)
        got_q, got_f = (t.cpu().numpy() for t in _finish_local(fmt, ones, lt, lut))
        assert np.array_equal(got_q, want_q) and np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)), form
    check_ones("ones", unchanged=True)
    # a random grid: the restatement of the float image the plain finish writes
    g = np.random.default_rng(5).uniform(0.25, 4.0, (gy, gx, nz)).astype(np.float32)
    d_g, check_g = guarded_upload(g)
    ref_f, ref_q = T.render(lin, g, 16, fmt, CCM, LUTS["srgb4096"])
    for form in ("lds", "cache"):
        monkeypatch.setenv("MFSR_LOCAL_TONE_GRID", form)
        whole_q, whole_f = (t.cpu().numpy() for t in _finish_local(fmt, d_g, lt, lut))
        assert np.array_equal(whole_q, R.as_bytes(ref_q)), form
        assert np.array_equal(whole_f.view(np.uint32), ref_f.view(np.uint32)), form
        bpp = R.BYTES_PER_PIXEL[fmt]
        # stripes and windows are crops of the whole-frame launch
        for x0, y0, w, h in ((0, 0, FW, 1), (0, 1, FW, 7), (0, 8, FW, 16), (0, 24, FW, FH - 24), (16, 16, 64, 16), (80, 5, FW - 80, 30)):
            q, f = (t.cpu().numpy() for t in _finish_local(fmt, d_g, lt, lut, x0, y0, w, h))
            assert np.array_equal(q, whole_q[y0:y0 + h, bpp * x0:bpp * (x0 + w)]), (form, x0, y0, w, h)
            assert np.array_equal(f.view(np.uint32), whole_f[y0:y0 + h, x0:x0 + w].view(np.uint32)), (form, x0, y0, w, h)
    check_g("grid", unchanged=True)
    _inputs_unchanged("finishLocalTone")


def test_all_four_entry_points_capture_into_a_graph():
    L = capi.lib()
    lt = _lt(16, 8)
    gx, gy, nz = T.grid_size(FW, FH, 16, 8)
    d_lin, _ = _linear_image()
    lut = torch.from_numpy(LUTS["srgb4096"]).to(DEV)
    d_g = torch.from_numpy(np.random.default_rng(6).uniform(0.25, 4.0, (gy, gx, nz)).astype(np.float32)).to(DEV)
    table = torch.zeros(gy, gx, nz, 2, dtype=torch.int64, device=DEV)
    rb = R.row_bytes(R.RGB8, FW)
    out_a, out_b = (torch.zeros(FH, rb, dtype=torch.uint8, device=DEV) for _ in range(2))
    f_a, f_b = (torch.zeros(FH, FW, 3, dtype=torch.float32, device=DEV) for _ in range(2))
    r = _struct(R.RGB8, CCM, lut)

    def four():
        stream = torch.cuda.current_stream().cuda_stream
        table.zero_()
        _image_stats(d_lin, 12 * FW, FW, FH, lt, CCM, table, stream=stream)
        _finish_stats(table, lt, CCM, stream=stream)
        L.localToneImage(d_lin.data_ptr(), 12 * FW, f_a.data_ptr(), 12 * FW, out_a.data_ptr(), rb, FW, FH, ctypes.byref(r), 0,
                         d_g.data_ptr(), ctypes.byref(lt), 0, 0, FW, FH, stream)
        _finish_local(R.RGB8, d_g, lt, lut, stream=stream, outs=(out_b, f_b))

    four()                                           # warm-up outside capture; the eager answer
    torch.cuda.synchronize()
    eager = [t.cpu().numpy().copy() for t in (table, out_a, out_b, f_a, f_b)]
    assert int(eager[0][..., 0].sum()) == 2 * FW * FH and np.array_equal(eager[1], eager[2])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        four()
    for _ in range(2):
        for t in (table, out_a, out_b):
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for t, want in zip((table, out_a, out_b, f_a, f_b), eager):
            assert np.array_equal(t.cpu().numpy().view(np.uint8), want.view(np.uint8))
    del graph
    _inputs_unchanged("graph")


# ---- 5. bursts ---------------------------------------------------------------------------------------------------------------
HRW, HRH = 768, 512
TONE = dict(shadows=0.5, highlights=0.25, cell=32, bins=16, smooth=1)


def _chain(p, pipe, m, fmt, lut, what, offset=(0, 0)):
    """plain float image -> restatement statistics -> library fit -> restatement slice, against what the pipeline left"""
    from multi_frame_super_resolution_amd.pipeline import local_tone_fit
    lt = pipe._local_tone
    want_table = T.stats(p, lt.cell, lt.bins, m, offset, (HRW, HRH))
    got_table = _host(pipe.tone_table)
    assert np.array_equal(got_table, want_table), what + ": " + _diff(got_table, want_table)
    fit = local_tone_fit(want_table, HRW, HRH, lt)
    grid = pipe.tone_grid.cpu().numpy()
    assert np.array_equal(grid.view(np.uint32), fit.grid.numpy().view(np.uint32)), what
    want_grid, want_pivot, want_status = T.fit(want_table, lt.smooth, lt.shadows, lt.highlights, lt.pivot, lt.maxGain)
    res = pipe.local_tone_result
    ulps = np.abs(grid.view(np.int32).astype(np.int64) - want_grid.view(np.int32).astype(np.int64)).max()
    assert ulps <= 1 and res.status == want_status == 0 and abs(res.pivot - want_pivot) <= 1e-14 * want_pivot, what
    assert res.minGain == grid.min() and res.maxGain == grid.max() and res.minGain < 1.0 < res.maxGain, what
    return T.render(p, grid, lt.cell, fmt, m, lut, False, offset)


@pytest.mark.parametrize("fused", [1, 0])
def test_local_tone_burst_equals_the_chain(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    p, q_plain = _plain(fused)
    pipe = BurstPipeline(_config(fused), DEV)
    # without a render description: uint16 RGB of the gained linear image
    pipe.set_local_tone(**TONE)
    img, q = pipe.process(frames)
    want_f, want_q = _chain(p, pipe, None, R.RGB16, None, f"rgb16 fused={fused}")
    assert q.dtype == torch.int16 and np.array_equal(q.cpu().numpy().view(np.uint16), want_q)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    # RGB8 with a matrix and a table; then stripes of finish_rows equal the whole
    pipe.set_render(capi.OUT_RGB8, matrix=CCM, tone_lut=LUTS["srgb4096"])
    img, q = pipe.process(frames)
    want_f, want_q = _chain(p, pipe, CCM, R.RGB8, LUTS["srgb4096"], f"rgb8 fused={fused}")
    whole = q.cpu().numpy().copy()
    assert q.dtype == torch.uint8 and np.array_equal(whole, want_q)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    pipe.out16.zero_()
    for r0, rows in ((0, 16), (16, 1), (17, 7), (24, HRH - 24)):
        pipe.finish_rows(r0, rows)
    assert np.array_equal(pipe.out16.cpu().numpy(), whole)
    # off again: the output of the pipeline that never measured
    pipe.set_local_tone(None)
    pipe.set_render(None)
    img, q = pipe.process(frames)
    assert np.array_equal(q.cpu().numpy(), q_plain) and np.array_equal(img.cpu().numpy().view(np.uint32), p.view(np.uint32))
    pipe.close()


def test_local_tone_with_process_auto_measures_with_the_installed_matrix():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    p, _ = _plain()
    pipe = BurstPipeline(_config(), DEV)
    pipe.set_local_tone(**TONE)
    img, q = pipe.process_auto(frames, format=capi.OUT_RGB8, matrix=CCM)
    r = pipe.auto_description
    m = np.array(list(r.matrix), np.float32)
    assert r.useMatrix == 1 and not np.array_equal(m, CCM)          # the white-balance gains went in
    lut = pipe.auto_lut.cpu().numpy()
    want_f, want_q = _chain(p, pipe, m, R.RGB8, lut, "process_auto")
    assert np.array_equal(q.cpu().numpy(), want_q)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    pipe.close()


def test_local_tone_in_a_zoom_window_measures_the_window():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    x, y, w, h = 240, 96, 160, 112          # on the 16-pixel grid: the library's window is the one asked for
    p = np.ascontiguousarray(_plain()[0][y:y + h, x:x + w])
    pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
    pw.set_local_tone(**TONE)
    pw.set_render(capi.OUT_RGBA8, matrix=CCM)
    img, q = pw.process([f.to(DEV) for f in _frames()])
    want_f, want_q = _chain(p, pw, CCM, R.RGBA8, None, "window", (x, y))
    table = _host(pw.tone_table)
    assert int(table[..., 0].sum()) == w * h            # the window's pixels only, in the full frame's grid
    assert int(table[y // 32:(y + h + 31) // 32, x // 32:(x + w + 31) // 32, :, 0].sum()) == w * h
    assert np.array_equal(q.cpu().numpy(), want_q)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    pw.close()


def test_local_tone_refusals_leave_the_handle_usable():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    raw = capi.lib().raw
    set_tone, set_sharpen = raw["mfsr_burst_set_local_tone"], raw["mfsr_burst_set_sharpen"]
    lt = _lt(32, 16)
    grid = torch.ones(16, 24, 16, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    # a handle with an upload ring
    host = BurstPipeline(_config_ring(), DEV)
    assert set_tone(host._h, ctypes.byref(lt), grid.data_ptr()) == -1
    host.close()
    pipe = BurstPipeline(_config(), DEV)
    with pytest.raises(RuntimeError):
        pipe.local_tone()                                   # no description
    # whichever setter comes second is refused
    pipe.set_sharpen(1.0)
    with pytest.raises(capi.MfsrError):
        pipe.set_local_tone(0.5)
    pipe.set_sharpen(None)
    pipe.set_denoise(3.0)
    with pytest.raises(capi.MfsrError):
        pipe.set_local_tone(0.5)
    pipe.set_denoise(None)
    pipe.set_render(capi.OUT_NV12)
    with pytest.raises(capi.MfsrError):
        pipe.set_local_tone(0.5)
    pipe.set_render(None)
    assert pipe._local_tone is None
    pipe.set_local_tone(**TONE)
    with pytest.raises(capi.MfsrError):
        pipe.set_sharpen(1.0)
    with pytest.raises(capi.MfsrError):
        pipe.set_denoise(3.0)
    with pytest.raises(capi.MfsrError):
        pipe.set_render(capi.OUT_P010)
    with pytest.raises(ValueError):
        pipe.set_local_tone(0.5, cell=24)
    with pytest.raises(ValueError):
        pipe.set_local_tone(1.5)
    bad = _lt(32, 5)
    assert set_tone(pipe._h, ctypes.byref(bad), grid.data_ptr()) == -1 and set_tone(pipe._h, ctypes.byref(lt), None) == -1
    # not while a frame is pending, and no measurement before a reference
    res = capi.LocalToneResult()
    assert raw["mfsr_burst_local_tone"](pipe._h, pipe._img_out.data_ptr(), pipe._total_weights.data_ptr(), ctypes.byref(lt),
                                        pipe._tone_table.data_ptr(), pipe._tone_grid.data_ptr(), ctypes.byref(res), None) == -1
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    pipe.add_frame(frames[0], True)
    assert set_tone(pipe._h, ctypes.byref(lt), grid.data_ptr()) == -1 and set_tone(pipe._h, None, None) == -1
    pipe.flush()
    # the refused calls changed nothing: the burst still equals the chain
    pipe.set_local_tone(**TONE)
    img, q = pipe.process(frames)
    want_f, want_q = _chain(_plain()[0], pipe, None, R.RGB16, None, "after the refusals")
    assert np.array_equal(q.cpu().numpy().view(np.uint16), want_q)
    pipe.close()


def _config_ring():
    cfg = _config()
    cfg.uploadRing = 3
    return cfg


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_local_tone(tmp_path):
    import re
    from PIL import Image
    from tests.test_bundled_burst import CITY
    cli = os.path.join(ROOT, "apps", "multi_frame_sr")
    assert os.path.exists(cli), "build apps/multi_frame_sr first (__graft_entry__.build())"
    for i in range(5):          # the bundled frames with the left half darkened
        a = np.asarray(Image.open(os.path.join(CITY, f"img_{i:06d}.png"))).astype(np.float32)
        a[:, :a.shape[1] // 2] *= 0.25
        Image.fromarray(np.rint(a).astype(np.uint8)).save(tmp_path / f"img_{i:06d}.png")
    env = dict(os.environ)
    for k in ("MFSR_AUTO", "MFSR_CCM", "MFSR_SHARPEN", "MFSR_DENOISE", "MFSR_GPUS", "MFSR_LOCAL_TONE"):
        env.pop(k, None)
    outs = {}
    for name, tone in (("plain", None), ("local", "0.5,0.25,32")):
        e = dict(env, MFSR_LOCAL_TONE=tone) if tone else env
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=e)
        assert p.returncode == 0, p.stderr
        outs[name] = np.asarray(Image.open(tmp_path / "city_farneback_sr_result.png")).astype(np.float64)
        if tone:
            m = re.search(r"local tone: cell (\d+) bins (\d+) pivot (\S+) gains (\S+) \.\. (\S+) \(status (\d)\)", p.stderr)
            assert m, p.stderr
            assert (int(m.group(1)), int(m.group(2)), int(m.group(6))) == (32, 16, 0), p.stderr
            assert 0.0 < float(m.group(3)) < 1.0 and float(m.group(4)) < 1.0 < float(m.group(5)) <= 4.0, p.stderr
        else:
            assert "local tone:" not in p.stderr
    half = outs["plain"].shape[1] // 2
    assert outs["local"].shape == outs["plain"].shape
    # the dark half is lifted, and by more than the bright half
    lift = [outs["local"][:, s].mean() / outs["plain"][:, s].mean() for s in (slice(0, half), slice(half, None))]
    assert lift[0] > 1.05 and lift[0] > lift[1], lift
    for extra in (dict(MFSR_GPUS="2"), dict(MFSR_SHARPEN="1.0"), dict(MFSR_DENOISE="3")):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=60,
                           env=dict(env, MFSR_LOCAL_TONE="0.5", **extra))
        assert p.returncode != 0 and "MFSR_LOCAL_TONE" in p.stderr, extra
    for bad in ("", "x", "0.5,", "1.5", "0.5,0.25,24", "0.5,0.25,32,5", "0.5,0.25,32,16,1"):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=60,
                           env=dict(env, MFSR_LOCAL_TONE=bad))
        assert p.returncode != 0 and "MFSR_LOCAL_TONE" in p.stderr, bad
