"""The finish chain on the device: k_chainImage against the numpy composition of tests/chain_ref.py for the
single-plane and the two-plane formats, k_finishChain against the device composition of the existing entry points and against
chain_ref, stripes against the whole, the fade's skip path, chained bursts (resident, unfused, striped, windowed, host, streamed)
against chain_ref applied to the plain float image and weights of the same pipeline, and the refusals of the setters.  Every
comparison is bit for bit: uint32 views of floats, bytes of the integer outputs."""
import ctypes

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi
from tests import chain_ref as C
from tests import denoise_ref as D
from tests import local_tone_ref as LT
from tests import render_ref as R
from tests import sharpen_ref as S
from tests import test_denoise_gpu as TD
from tests import yuv_ref as Y
from tests.kernels import guarded_upload

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CANARY = 0xA5
FORMATS = (R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2)
NAMES = {R.RGB16: "RGB16", R.RGB8: "RGB8", R.RGBA8: "RGBA8", R.RGB10A2: "RGB10A2", Y.NV12: "NV12", Y.P010: "P010"}
CCM, LUT = TD.CCM, TD.LUT
f32 = np.float32
_pixels, _counts = TD._pixels, TD._counts


@pytest.fixture(scope="module", autouse=True)
def _default_accumulate_variant():
    """as tests/test_denoise_gpu.py: the bursts below share its cached plain burst, computed with the library's default"""
    L = capi.lib()
    found = L.raw["mfsr_get_accumulate_fast_exp"]()
    L.set_accumulate_fast_exp(2)
    yield
    L.set_accumulate_fast_exp(found)


# ---- descriptions: the restatement's dicts and the C struct of them ---------------------------------------------------------
def _den(radius, **kw):
    return dict(dict(radius=radius, strength=3.0, gain=4.0, alpha=0.05, beta=0.01), **kw)


def _sharp(radius, amount=1.5, threshold=0.01):
    return dict(taps=S.gaussian_taps(1.0, radius)[1], amount=amount, threshold=threshold)


def _tone(full_w, full_h, cell=16, bins=8, seed=3):
    gx, gy, gz = LT.grid_size(full_w, full_h, cell, bins)
    return dict(grid=np.random.default_rng(seed).uniform(0.5, 2.0, (gy, gx, gz)).astype(f32), cell=cell)


def _cstruct(den=None, sharp=None, tone=None):
    """(capi.FinishChain, the grid on the device or None); the stages that are off hold valid descriptions"""
    c = capi.FinishChain()
    c.denoise.gain = 1.0
    if den:
        d = c.denoise
        d.radius, d.strength, d.gain, d.alpha, d.beta = den["radius"], den["strength"], den["gain"], den["alpha"], den["beta"]
        d.wLo, d.wHi = den.get("w_lo", 0.0), den.get("w_hi", 0.0)
    if sharp:
        s = c.sharpen
        s.radius, s.amount, s.threshold = len(sharp["taps"]) - 1, sharp["amount"], sharp["threshold"]
        for k, v in enumerate(sharp["taps"]):
            s.taps[k] = float(v)
    lt = c.localTone
    lt.cell, lt.bins, lt.smooth, lt.shadows, lt.highlights, lt.maxGain = 16, 8, 1, 0.5, 0.25, 4.0
    grid = None
    if tone:
        lt.cell, lt.bins, c.useLocalTone = tone["cell"], tone["grid"].shape[2], 1
        grid = torch.from_numpy(tone["grid"]).to(DEV)
    assert capi.lib().raw["mfsr_finish_chain_validate"](ctypes.byref(c)) == 0
    return c, grid


def _render(fmt, m=None, lut_dev=None, colour=0):
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


def _expected(dense, off, row_bytes):
    """dense rows [h, n] of bytes at byte `off` of a canary-filled buffer with rows `row_bytes` apart"""
    h = dense.shape[0]
    want = np.full(off + row_bytes * h, CANARY, np.uint8)
    want[off:].reshape(h, row_bytes)[:, :dense.shape[1]] = dense
    return want


def _layouts(fmt, w):
    """(offset, row bytes) of the integer output: odd byte offsets and padded rows where the format's stores allow them"""
    if fmt == R.RGB8:
        return [(1, 3 * w + 5), (0, 3 * w), (3, 3 * w + 2)]
    if fmt == R.RGB16:
        return [(2, 6 * w + 2), (0, 6 * w)]
    if fmt == Y.NV12:
        return [(1, w + 3), (0, w), (3, w + 5), (4, w + 4)]
    if fmt == Y.P010:
        return [(2, 2 * w + 6), (0, 2 * w), (8, 2 * w + 8)]
    return [(4, 4 * w + 4), (0, 4 * w)]


def _launch(entry, args_before_outputs, args_after_outputs, w, h, fmt, off, rb):
    """one launch with guarded outputs: (float image, integer bytes, chroma bytes or None)"""
    two = fmt in (Y.NV12, Y.P010)
    d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, f32))
    d_q, check_q = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
    d_uv, check_uv = guarded_upload(np.full(off + rb * (h // 2) if two else 4, CANARY, np.uint8))
    entry(*args_before_outputs, d_f.data_ptr(), 12 * w, d_q.data_ptr() + off, rb, d_uv.data_ptr() + off if two else None, rb if two else 0,
          *args_after_outputs)
    for chk in (check_f, check_q, check_uv):
        chk(f"{NAMES[fmt]} {w}x{h}")
    return d_f.cpu().numpy(), d_q.cpu().numpy(), d_uv.cpu().numpy() if two else None


def _chain_image(L, d_in, d_cnt, w, h, c, grid, r, off, rb, offset=(0, 0), full=None):
    fw, fh = (w, h) if full is None else full
    return _launch(L.chainImage, (d_in.data_ptr(), 12 * w, None if d_cnt is None else d_cnt.data_ptr(), 12 * w),
                   (w, h, ctypes.byref(r), 0, ctypes.byref(c), None if grid is None else grid.data_ptr(), offset[0], offset[1], fw, fh, None),
                   w, h, r.format, off, rb)


def _assert_equal(got, want, fmt, off, rb, what):
    """got = (float, bytes, chroma bytes) of _launch; want = chain_ref.render's tuple"""
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what + " (float image)"
    if fmt in (Y.NV12, Y.P010):
        dense = Y.as_bytes(want[1], want[2])
        h = want[1].shape[0]
        assert np.array_equal(got[1], _expected(dense[:h], off, rb)), what + " (Y plane)"
        assert np.array_equal(got[2], _expected(dense[h:], off, rb)), what + " (chroma plane)"
    else:
        assert np.array_equal(got[1], _expected(R.as_bytes(want[1]), off, rb)), what


_inputs = {}


def _input(w, h):
    """(pixels, counts, their guarded uploads), once per size, unchanged"""
    if (w, h) not in _inputs:
        p, n = _pixels(h, w, 100 * w + h), _counts(h, w, 7 * w + h)
        _inputs[w, h] = (p, n, guarded_upload(p), guarded_upload(n))
    return _inputs[w, h]


_ts = {}


def _t(w, h, n_on, den, sharp, tone, m, offset, key):
    """chain_ref.chain of the size's input, once per (size, chain, count, matrix): the formats share it"""
    k = (w, h, n_on, key, m is not None)
    if k not in _ts:
        p, n = _input(w, h)[:2]
        _ts[k] = C.chain(p, n if n_on else None, den, sharp, tone, m, offset)
    return _ts[k]


OFFSET, PAD = (5, 3), (9, 7)      # the image's place in the full frame of the grid, and what the frame has beyond it


def _stage_set(name, w, h):
    full = (w + PAD[0], h + PAD[1])
    rd_rs = {"DS11": (1, 1), "DS34": (3, 4), "DS22": (2, 2), "DSL": (2, 2), "SL": (0, 3), "DL": (3, 0), "D": (2, 0), "S": (0, 4), "L": (0, 0)}
    rd, rs = rd_rs[name]
    return (_den(rd) if rd else None, _sharp(rs) if rs else None, _tone(*full) if "L" in name else None, full)


# ---- 1. the tile body on a float image, single-plane formats ----------------------------------------------------------------
SIZES = [(1, 1), (3, 2), (67, 19), (130, 33)]
# The inputs hold +-inf.  The denoise stage clamps them; a sharpen stage that comes first does not, and inf - inf MAKES a NaN, whose
# sign bit is the hardware's choice (the device's default NaN is positive, the host's negative): tests/test_sharpen_gpu.py keeps
# inf out of its inputs for that reason.  Here those stage sets always run with matrix + table, which clean a NaN to 0 before
# the float image is written; what is compared stays bit for bit.
NAN_MAKERS = ("SL", "S")
SETS = ["DS11", "DS34", "DS22", "DSL", "SL", "DL"]


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_chainImage_equals_the_restatement(fmt):
    """Sizes: one pixel; 3 x 2 (smaller than the reach: every tap clamps twice); 67 x 19 and 130 x 33 (ragged in both tile
    directions, no multiple of 4).  Every format runs every stage set once, on a size, with or without a count image and with
    or without matrix + table, that rotate with the format; and (R_d, R_s) = (3, 4) on every size.  (NAN_MAKERS always render.)"""
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    fi = FORMATS.index(fmt)
    cases = [(name, SIZES[(k + fi) % 4], (k + fi) % 2 == 0, (k // 2 + fi) % 2 == 0 or name in NAN_MAKERS) for k, name in enumerate(SETS)]
    cases += [("DS34", size, (j + fi) % 2 == 1, j % 2 == 0) for j, size in enumerate(SIZES)]
    for k, (name, (w, h), counted, rendered) in enumerate(cases):
        p, n, (d_in, check_in), (d_cnt, check_cnt) = _input(w, h)
        den, sharp, tone, full = _stage_set(name, w, h)
        m, lut = (CCM, LUT) if rendered else (None, None)
        want = R.render(_t(w, h, counted, den, sharp, tone, m, OFFSET, name), fmt, m, lut)
        c, grid = _cstruct(den, sharp, tone)
        off, rb = _layouts(fmt, w)[k % len(_layouts(fmt, w))]
        got = _chain_image(L, d_in, d_cnt if counted else None, w, h, c, grid, _render(fmt, m, lut_dev if rendered else None), off, rb,
                           OFFSET, full)
        what = f"{NAMES[fmt]} {name} {w}x{h} count={counted} rendered={rendered} offset={off} rowBytes={rb}"
        _assert_equal(got, want, fmt, off, rb, what)
        check_in(what, unchanged=True)
        check_cnt(what, unchanged=True)
    assert len(cases) == 10


def test_chainImage_changes_the_image_and_each_stage_counts():
    """the stage sets differ from one another and from the plain render: no stage is silently skipped"""
    w, h = 67, 19
    seen = [R.render(_input(w, h)[0], R.RGB16)[0].view(np.uint32)]
    for name in SETS:
        den, sharp, tone, _ = _stage_set(name, w, h)
        t = _t(w, h, True, den, sharp, tone, None, OFFSET, name).view(np.uint32)
        assert all(not np.array_equal(t, s) for s in seen), name
        seen.append(t)


@pytest.mark.parametrize("how", ["lds", "cache"])
def test_chainImage_lut_in_lds_and_through_the_cache_give_the_same_bytes(monkeypatch, how):
    L = capi.lib()
    w, h = 130, 33
    p, n, (d_in, _), (d_cnt, _) = _input(w, h)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    monkeypatch.setenv("MFSR_RENDER_LUT", how)
    den, sharp, tone, full = _stage_set("DSL", w, h)
    c, grid = _cstruct(den, sharp, tone)
    t = _t(w, h, True, den, sharp, tone, CCM, OFFSET, "DSL")
    for fmt in FORMATS + (Y.NV12,):
        ww, hh = (w, h) if fmt != Y.NV12 else (130, 34)
        if fmt == Y.NV12:
            p2, n2, (d_in2, _), (d_cnt2, _) = _input(ww, hh)
            den2, sharp2, tone2, full2 = _stage_set("DSL", ww, hh)
            c2, grid2 = _cstruct(den2, sharp2, tone2)
            want = C.render(p2, fmt, n2, den2, sharp2, tone2, CCM, LUT, 0, OFFSET)
            got = _chain_image(L, d_in2, d_cnt2, ww, hh, c2, grid2, _render(fmt, CCM, lut_dev), 0, ww, OFFSET, full2)
            _assert_equal(got, want, fmt, 0, ww, f"{how} NV12")
            continue
        rb = R.row_bytes(fmt, w)
        got = _chain_image(L, d_in, d_cnt, w, h, c, grid, _render(fmt, CCM, lut_dev), 0, rb, OFFSET, full)
        _assert_equal(got, R.render(t, fmt, CCM, LUT), fmt, 0, rb, f"{how} {NAMES[fmt]}")


def test_chainImage_without_a_render_description_and_one_output_at_a_time():
    """render = NULL is {RGB16, no matrix, no table}; the float image alone and the integers alone"""
    L = capi.lib()
    w, h = 67, 19
    p, n, (d_in, _), (d_cnt, _) = _input(w, h)
    den, sharp, _, _ = _stage_set("DS22", w, h)
    c, _ = _cstruct(den, sharp)
    want_f, want_q = R.render(_t(w, h, True, den, sharp, None, None, OFFSET, "DS22"), R.RGB16)
    for with_f, with_q in ((True, False), (False, True)):
        d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, f32))
        d_q, check_q = guarded_upload(np.full(6 * w * h, CANARY, np.uint8))
        L.chainImage(d_in.data_ptr(), 12 * w, d_cnt.data_ptr(), 12 * w, d_f.data_ptr() if with_f else None, 12 * w,
                     d_q.data_ptr() if with_q else None, 6 * w, None, 0, w, h, None, 0, ctypes.byref(c), None, 0, 0, w, h, None)
        check_f("one output")
        check_q("one output")
        got_f, got_q = d_f.cpu().numpy(), d_q.cpu().numpy()
        assert np.array_equal(got_f.view(np.uint32), want_f.view(np.uint32)) if with_f else (got_f == -7.0).all()
        assert np.array_equal(got_q, _expected(R.as_bytes(want_q), 0, 6 * w)) if with_q else (got_q == CANARY).all()


# ---- 2. the two-plane formats -----------------------------------------------------------------------------------------------
YUV_SIZES = [(2, 2), (6, 4), (66, 18), (130, 34)]
YUV_SETS = ["D", "S", "L", "DS34", "DSL"]
COLOURS = (Y.BT709, Y.BT2020 | Y.FULL)


@pytest.mark.parametrize("fmt", [Y.NV12, Y.P010], ids=NAMES.get)
def test_chainImage_two_plane_formats_equal_the_restatement(fmt):
    """Sizes 2 x 2, 6 x 4 (smaller than the reach), 66 x 18 and 130 x 34 (ragged tiles, a last lane of two columns); BT.709
    limited and BT.2020 full; every stage set on two sizes, so that every size and both colour descriptions meet both
    formats; the Y plane, the chroma plane and the float image."""
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    fi = 0 if fmt == Y.NV12 else 1
    cases = [(name, YUV_SIZES[(k + 2 * j + fi) % 4], COLOURS[(k + j) % 2], (k + fi) % 2 == 0, (k + j + fi) % 2 == 0 or name in NAN_MAKERS)
             for k, name in enumerate(YUV_SETS) for j in range(2)]
    assert {c[1] for c in cases} == set(YUV_SIZES) and {c[2] for c in cases} == set(COLOURS)
    for k, (name, (w, h), colour, counted, rendered) in enumerate(cases):
        p, n, (d_in, check_in), (d_cnt, check_cnt) = _input(w, h)
        den, sharp, tone, full = _stage_set(name, w, h)
        m, lut = (CCM, LUT) if rendered else (None, None)
        want = (lambda t: Y.render(t, fmt, m, lut, False, colour))(_t(w, h, counted, den, sharp, tone, m, OFFSET, name))
        c, grid = _cstruct(den, sharp, tone)
        off, rb = _layouts(fmt, w)[k % len(_layouts(fmt, w))]
        got = _chain_image(L, d_in, d_cnt if counted else None, w, h, c, grid, _render(fmt, m, lut_dev if rendered else None, colour),
                           off, rb, OFFSET, full)
        what = f"{NAMES[fmt]} {name} {w}x{h} colour={colour} count={counted} rendered={rendered} offset={off} rowBytes={rb}"
        _assert_equal(got, want, fmt, off, rb, what)
        check_in(what, unchanged=True)
        check_cnt(what, unchanged=True)


# ---- 3. the fused kernel against the device composition and the restatement -------------------------------------------------
X0, Y0, FW, FH, FBW, FBH, THR = 16, 8, 160, 50, 80, 25, 1e-3
_accs = {}


def _acc(W, H):
    """accumulators with weights on both sides of the threshold (the fallback resample runs) and their guarded uploads: once
    per size"""
    if (W, H) not in _accs:
        fin, wt, fb = TD._accumulators(W, H, FBW, FBH, THR)
        _accs[W, H] = (fin, wt, fb, [guarded_upload(a) for a in (fin, wt, fb)])
    return _accs[W, H]


def _plain_finish(L, d_fin, d_wt, d_fb, W, H, x0, y0, fw, fh):
    d_lin, chk = guarded_upload(np.zeros((H, W, 3), f32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * W, None, W, H, THR, 0, 65535.0, x0, y0, fw, fh, None)
    chk("plain finish")
    return d_lin.cpu().numpy()


def _finish_chain(L, ups, W, c, grid, r, y0, h, above, below, off, rb, place=(X0, Y0, FW, FH)):
    (d_fin, _), (d_wt, _), (d_fb, _) = ups
    o = 12 * y0 * W
    return _launch(L.finishChain, (d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * W, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0),
                   (ctypes.byref(r), W, h, THR, 0, place[0], place[1] + y0, place[2], place[3], ctypes.byref(c),
                    None if grid is None else grid.data_ptr(), above, below, None), W, h, r.format, off, rb)


FINISH_CASES = [("DS34", R.RGB8, (67, 19)), ("DS34", R.RGB8, (130, 34)), ("DSL", R.RGBA8, (67, 19)), ("DSL", R.RGBA8, (130, 34)),
                ("DS22", Y.NV12, (130, 34)), ("SL", Y.P010, (130, 34))]


@pytest.mark.parametrize("name,fmt,size", FINISH_CASES, ids=[f"{n}-{NAMES[f]}-{s[0]}x{s[1]}" for n, f, s in FINISH_CASES])
def test_finishChain_equals_the_composition_of_the_existing_entries_and_the_restatement(name, fmt, size):
    """One launch on a W x H rectangle at (16, 8) of a 160 x 50 frame against (a) mfsr_finishDenoised to a float image, then
    mfsr_sharpenImage to a float image, then mfsr_localToneImage / mfsr_renderImage / mfsr_renderImageYuv on the device, and
    (b) chain_ref on the device's plain float image and the count of the weights.  (S+L to P010: no device composition exists
    for a two-plane local tone; the restatement only.)  The two-plane formats need even extents: 130 x 34 only."""
    L = capi.lib()
    W, H = size
    fin, wt, fb, ups = _acc(W, H)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    colour = Y.BT2020 | Y.FULL if fmt == Y.P010 else 0
    r = _render(fmt, CCM, lut_dev, colour)
    den, sharp, _, _ = _stage_set(name, W, H)
    if den:
        den = dict(den, alpha=0.02, beta=0.002)
    tone = _tone(FW, FH) if "L" in name else None
    c, grid = _cstruct(den, sharp, tone)
    off, rb = _layouts(fmt, W)[0]
    got = _finish_chain(L, ups, W, c, grid, r, 0, H, 0, 0, off, rb)
    # (b) the restatement
    lin = _plain_finish(L, ups[0][0], ups[1][0], ups[2][0], W, H, X0, Y0, FW, FH)
    n = D.count_of_weight(wt, THR)
    want = C.render(lin, fmt, n, den, sharp, tone, CCM, LUT, colour, (X0, Y0))
    _assert_equal(got, want, fmt, off, rb, f"{name} {NAMES[fmt]} {W}x{H} against chain_ref")
    assert not np.array_equal(want[0].view(np.uint32), R.render_float(lin, CCM, LUT).view(np.uint32))
    # (a) the device composition
    if fmt == Y.P010:
        return
    (d_fin, _), (d_wt, _), (d_fb, _) = ups
    d_a, chk_a = guarded_upload(np.zeros((H, W, 3), f32))
    d_b, chk_b = guarded_upload(np.zeros((H, W, 3), f32))
    L.finishDenoised(d_fin.data_ptr(), d_wt.data_ptr(), 12 * W, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0, d_a.data_ptr(),
                     12 * W, None, 0, None, W, H, THR, 0, X0, Y0, FW, FH, ctypes.byref(c.denoise), 0, 0, None)
    L.sharpenImage(d_a.data_ptr(), 12 * W, d_b.data_ptr(), 12 * W, None, 0, W, H, ctypes.byref(c.sharpen), None, 0, None)
    d_f, chk_f = guarded_upload(np.full((H, W, 3), -7.0, f32))
    rbd = Y.row_bytes(fmt, W) if fmt == Y.NV12 else R.row_bytes(fmt, W)
    d_q, chk_q = guarded_upload(np.full(rbd * (H * 3 // 2 if fmt == Y.NV12 else H), CANARY, np.uint8))
    if tone:
        L.localToneImage(d_b.data_ptr(), 12 * W, d_f.data_ptr(), 12 * W, d_q.data_ptr(), rbd, W, H, ctypes.byref(r), 0, grid.data_ptr(),
                         ctypes.byref(c.localTone), X0, Y0, FW, FH, None)
    elif fmt == Y.NV12:
        L.renderImageYuv(d_b.data_ptr(), 12 * W, d_f.data_ptr(), 12 * W, d_q.data_ptr(), rbd, d_q.data_ptr() + rbd * H, rbd, W, H,
                         ctypes.byref(r), 0, None)
    else:
        L.renderImage(d_b.data_ptr(), 12 * W, d_f.data_ptr(), 12 * W, d_q.data_ptr(), rbd, W, H, ctypes.byref(r), 0, None)
    for chk in (chk_a, chk_b, chk_f, chk_q):
        chk("composition")
    assert np.array_equal(d_f.cpu().numpy().view(np.uint32), got[0].view(np.uint32)), "float image against the device composition"
    comp = d_q.cpu().numpy().reshape(-1, rbd)
    if fmt == Y.NV12:
        assert np.array_equal(_expected(comp[:H], off, rb), got[1]) and np.array_equal(_expected(comp[H:], off, rb), got[2])
    else:
        assert np.array_equal(_expected(comp, off, rb), got[1])
    for _, chk in ups:
        chk("inputs", unchanged=True)


# ---- 4. stripes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.RGB8, Y.NV12], ids=NAMES.get)
def test_stripes_add_up_to_the_whole_frame_and_a_stripe_alone_clamps_at_its_own_rows(fmt):
    """130 x 50, (R_d, R_s) = (3, 4): rows [0, 16), [16, 34), [34, 50) with rowsAbove / rowsBelow = min(7, rows available)
    equal the rows of the whole-frame launch, which equals chain_ref; with rowsAbove = rowsBelow = 0 the middle stripe equals
    chain_ref on its own rows only."""
    L = capi.lib()
    W, H = 130, 50
    fin, wt, fb, ups = _acc(W, H)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    r = _render(fmt, CCM, lut_dev)
    den, sharp = dict(_den(3), alpha=0.02, beta=0.002), _sharp(4)
    c, _ = _cstruct(den, sharp)
    place = (0, 0, W, H)
    rb = Y.row_bytes(fmt, W) if fmt == Y.NV12 else R.row_bytes(fmt, W)
    whole = _finish_chain(L, ups, W, c, None, r, 0, H, 0, 0, 0, rb, place)
    lin = _plain_finish(L, ups[0][0], ups[1][0], ups[2][0], W, H, 0, 0, W, H)
    n = D.count_of_weight(wt, THR)
    _assert_equal(whole, C.render(lin, fmt, n, den, sharp, None, CCM, LUT), fmt, 0, rb, "whole frame")
    for y0, y1 in ((0, 16), (16, 34), (34, 50)):
        got = _finish_chain(L, ups, W, c, None, r, y0, y1 - y0, min(7, y0), min(7, H - y1), 0, rb, place)
        what = f"stripe [{y0}, {y1})"
        assert np.array_equal(got[0].view(np.uint32), whole[0][y0:y1].view(np.uint32)), what
        assert np.array_equal(got[1], whole[1][rb * y0:rb * y1]), what
        if fmt == Y.NV12:
            assert np.array_equal(got[2], whole[2][rb * (y0 // 2):rb * (y1 // 2)]), what
    alone = _finish_chain(L, ups, W, c, None, r, 16, 18, 0, 0, 0, rb, place)
    want = C.render(lin, fmt, n, den, sharp, None, CCM, LUT, valid=(16, 34))
    _assert_equal(alone, want, fmt, 0, rb, "stripe alone")
    assert not np.array_equal(alone[1], whole[1][rb * 16:rb * 34])


# ---- 5. the fade ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [R.RGB8, Y.NV12], ids=NAMES.get)
def test_fade_with_wHi_below_every_count_skips_the_denoise_stage(fmt):
    """wLo = 1, wHi = 1.5 and counts >= 2: lambda = 0 everywhere, every wave skips the stencil and d = the cleaned p.  The
    result equals chain_ref with the fade, and -- on an input that the denoise's cleaning leaves as it is (no NaN, nothing
    beyond +-65536: the one thing a skipped denoise stage still does) -- the chain with the denoise stage off, bit for bit."""
    L = capi.lib()
    w, h = 130, 34
    raw = _pixels(h, w, 21)
    lut_dev = torch.from_numpy(LUT).to(DEV)
    rng = np.random.default_rng(4)
    n = rng.uniform(2.0, 9.0, (h, w, 3)).astype(f32)
    n[0, 0] = [2.0, np.inf, 1e6]
    d_cnt, _ = guarded_upload(n)
    den, sharp = _den(3, w_lo=1.0, w_hi=1.5), _sharp(4)
    c_on, _ = _cstruct(den, sharp)
    c_off, _ = _cstruct(None, sharp)
    r = _render(fmt, CCM, lut_dev)
    rb = Y.row_bytes(fmt, w) if fmt == Y.NV12 else R.row_bytes(fmt, w)
    for name, p in (("hostile", raw), ("clean", D.clean(raw))):
        d_in, _ = guarded_upload(p)
        got = _chain_image(L, d_in, d_cnt, w, h, c_on, None, r, 0, rb)
        _assert_equal(got, C.render(p, fmt, n, den, sharp, None, CCM, LUT), fmt, 0, rb, name)
        if name == "clean":
            off = _chain_image(L, d_in, None, w, h, c_off, None, r, 0, rb)
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, off) if a is not None)
    # (without the fade the same description filters: the skip is the fade's doing)
    filtered = C.render(D.clean(raw), fmt, n, _den(3), sharp, None, CCM, LUT)[0]
    assert not np.array_equal(filtered.view(np.uint32), got[0].view(np.uint32))


# ---- 6. bursts --------------------------------------------------------------------------------------------------------------
W, H = TD.W, TD.H
RENDER = TD.RENDER
BURST_DEN = dict(TD.DENOISE)                                       # set_denoise's keyword arguments
BURST_SHARP = dict(amount=1.0, taps=[float(v) for v in S.gaussian_taps(1.0, 2)[1]], threshold=0.002)
REF_DEN = dict(TD.REF_KW)
REF_SHARP = dict(taps=S.gaussian_taps(1.0, 2)[1], amount=1.0, threshold=0.002)
_wants = {}


def _want(fmt, fused=1, tone=None, colour=0):
    """chain_ref on the plain float image and weights of the same pipeline: computed once, shared, unchanged"""
    key = (fmt, fused, tone is not None, colour)
    if key not in _wants:
        lin, tw, thr = TD._plain(fused)
        _wants[key] = C.render(lin, fmt, D.count_of_weight(tw, thr), REF_DEN, REF_SHARP, tone, CCM, LUT, colour)
    return _wants[key]


def _yuv_flat(want):
    return Y.as_bytes(want[1], want[2]).reshape(-1)


@pytest.mark.parametrize("fused", [1, 0])
def test_chained_burst_equals_the_restatement_of_the_plain_burst(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in TD._frames()]
    pipe = BurstPipeline(TD._config(fused=fused), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    q0 = pipe.process(frames)[1].clone()
    assert pipe.chained_finishes() == 0                              # without a chain
    pipe.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP)
    for fmt in (R.RGB8, R.RGB10A2):
        pipe.set_render(fmt, **RENDER)
        img, q = pipe.process(frames)
        want_f, want_q = _want(fmt, fused)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)), (NAMES[fmt], fused)
        assert np.array_equal(TD._np(q), want_q), (NAMES[fmt], fused)
        assert pipe.chained_finishes() == 1 and pipe.denoised_finishes() == 0 and pipe.sharpened_finishes() == 0
    pipe.set_render(capi.OUT_NV12, yuv=capi.YUV_BT2020 | capi.YUV_FULL, **RENDER)      # a two-plane format with a stencil chain
    img, q = pipe.process(frames)
    want = _want(Y.NV12, fused, colour=Y.BT2020 | Y.FULL)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), fused
    assert np.array_equal(q.cpu().numpy(), _yuv_flat(want)), fused
    assert pipe.chained_finishes() == 1
    # ... and with the local tone behind both stencils
    tone = _tone(2 * W, 2 * H)
    lt = capi.LocalTone()
    lt.cell, lt.bins, lt.smooth, lt.shadows, lt.highlights, lt.maxGain = 16, 8, 1, 0.5, 0.25, 4.0
    pipe.set_render(capi.OUT_RGBA8, **RENDER)
    pipe.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP, local_tone=(lt, tone["grid"]))
    img, q = pipe.process(frames)
    want_f, want_q = _want(R.RGBA8, fused, tone)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32)) and np.array_equal(TD._np(q), want_q)
    # off again: the bytes of the burst without a chain
    pipe.set_finish_chain()
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    img, q = pipe.process(frames)
    assert torch.equal(q, q0) and pipe.chained_finishes() == 0
    pipe.close()


def test_chained_finish_rows_are_the_rows_of_the_whole():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in TD._frames()]
    pipe = BurstPipeline(TD._config(), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    pipe.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP)
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
    assert done.all() and pipe.chained_finishes() == 2
    pipe.close()


@pytest.mark.parametrize("fmt", [R.RGB8, Y.NV12], ids=NAMES.get)
def test_chained_host_burst_equals_the_resident_one(fmt):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    host = [f.pin_memory() for f in TD._frames()]
    pipe = BurstPipeline(TD._config(ring=4), DEV)
    pipe.set_render(fmt, **RENDER)
    pipe.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP)
    want = _want(fmt)
    want_q = _yuv_flat(want) if fmt == Y.NV12 else want[1]
    for rep in range(2):
        got = pipe.process_host(host)
        pipe.host_sync()
        assert np.array_equal(TD._np(got), want_q), (NAMES[fmt], rep)
    assert pipe.chained_finishes() > 1            # banded: one finish per band, each after the band below it was fused
    pipe.close()


def test_chained_zoom_window_is_the_crop():
    """the Python layer grows the aligned window by one 16-pixel ring (the reach is 4 < 16) and crops"""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    want_f, want_q = _want(R.RGB8)
    for x, y, w, h in ((40, 24, 100, 60), (0, 70, 90, 58)):
        pw = BurstPipeline(TD._config(), DEV, window=(x, y, w, h))
        pw.set_render(capi.OUT_RGB8, **RENDER)
        pw.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP)
        img, q = pw.process([f.to(DEV) for f in TD._frames()])
        assert tuple(q.shape[:2]) == (h, w)
        assert np.array_equal(TD._np(q), want_q[y:y + h, x:x + w]), (x, y, w, h)
        assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f[y:y + h, x:x + w].view(np.uint32)), (x, y, w, h)
        pw.close()


def test_frame_stream_chains_its_outputs():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream
    frames = [f.to(DEV) for f in TD._frames()]
    st = FrameStream(TD._config(frames=3), 1, DEV, render=dict(format=capi.OUT_RGB8, **RENDER),
                     chain=dict(denoise=BURST_DEN, sharpen=BURST_SHARP))
    outs = {}
    for f in frames:
        r = st.push(f)
        if r is not None:
            outs[r[0]] = r[1].clone()
    torch.cuda.synchronize()
    st.close()
    assert sorted(outs) == [0, 1] and outs[1].dtype == torch.uint8 and tuple(outs[1].shape) == (2 * H, 2 * W, 3)
    ref = BurstPipeline(TD._config(frames=3, reference=1), DEV)      # output 1 = frames [0, 2] around reference 1
    lin, _ = ref.process(frames)
    n = D.count_of_weight(ref.total_weights.cpu().numpy(), float(ref.cfg.weightThreshold))
    want = C.render(lin.cpu().numpy(), R.RGB8, n, REF_DEN, REF_SHARP, None, CCM, LUT)[1]
    assert np.array_equal(TD._np(outs[1]), want)
    ref.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_working_handle():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in TD._frames()]
    raw = capi.lib().raw
    set_chain, set_denoise, set_sharpen = raw["mfsr_burst_set_finish_chain"], raw["mfsr_burst_set_denoise"], raw["mfsr_burst_set_sharpen"]
    set_tone, set_render = raw["mfsr_burst_set_local_tone"], raw["mfsr_burst_set_render"]
    den = dict(radius=2, strength=3.0, gain=2.0, alpha=1.6e-3, beta=1.6e-5)
    sharp = REF_SHARP
    c, _ = _cstruct(den, sharp)
    tone = _tone(2 * W, 2 * H)
    c_tone, grid = _cstruct(den, sharp, tone)
    pipe = BurstPipeline(TD._config(), DEV)
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    pipe.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP)
    _, q = pipe.process(frames)
    before = q.clone()
    assert np.array_equal(TD._np(before), _want(R.RGB8)[1])
    h = pipe._h
    # the three setters with a description that is on are refused while the chain is installed; "off" is not
    assert set_sharpen(h, ctypes.byref(c.sharpen)) == -1 and set_denoise(h, ctypes.byref(c.denoise)) == -1
    assert set_tone(h, ctypes.byref(c_tone.localTone), grid.data_ptr()) == -1
    assert set_sharpen(h, None) == 0 and set_denoise(h, None) == 0 and set_tone(h, None, None) == 0
    # a grid if and only if useLocalTone; an invalid description
    assert set_chain(h, ctypes.byref(c), grid.data_ptr()) == -1 and set_chain(h, ctypes.byref(c_tone), None) == -1
    bad, _ = _cstruct(den, sharp)
    bad.reserved[3] = 1
    assert set_chain(h, ctypes.byref(bad), None) == -1
    # while a frame is pending
    assert pipe.group_size() > 1
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    pipe.add_frame(frames[0], True)
    assert set_chain(h, ctypes.byref(c), None) == -1 and set_chain(h, None, None) == -1
    with pytest.raises(capi.MfsrError):
        pipe.set_finish_chain(sharpen=BURST_SHARP)
    for f in frames[1:]:
        pipe.add_frame(f)
    _, q = pipe.finish()
    assert torch.equal(q, before)                                    # the refused calls changed nothing
    # the chain after set_denoise / set_sharpen / set_local_tone is refused
    assert set_chain(h, None, None) == 0
    assert set_denoise(h, ctypes.byref(c.denoise)) == 0 and set_chain(h, ctypes.byref(c), None) == -1 and set_denoise(h, None) == 0
    assert set_sharpen(h, ctypes.byref(c.sharpen)) == 0 and set_chain(h, ctypes.byref(c), None) == -1 and set_sharpen(h, None) == 0
    assert set_tone(h, ctypes.byref(c_tone.localTone), grid.data_ptr()) == 0 and set_chain(h, ctypes.byref(c), None) == -1
    assert set_tone(h, None, None) == 0
    # a two-plane format goes with a chain, and stays refused with the stencil setters
    yuv = _render(capi.OUT_NV12)
    assert set_chain(h, ctypes.byref(c), None) == 0 and set_render(h, ctypes.byref(yuv)) == 0
    assert set_chain(h, None, None) == 0 and set_sharpen(h, ctypes.byref(c.sharpen)) == -1
    pipe.set_render(capi.OUT_RGB8, **RENDER)
    pipe.set_finish_chain(denoise=BURST_DEN, sharpen=BURST_SHARP)
    _, q = pipe.process(frames)
    assert torch.equal(q, before)                                    # ... a working handle: the bytes it produced before
    pipe.close()
    # local tone in a chain on a handle with an upload ring
    ring = BurstPipeline(TD._config(ring=4), DEV)
    assert set_chain(ring._h, ctypes.byref(c_tone), grid.data_ptr()) == -1
    assert set_chain(ring._h, ctypes.byref(c), None) == 0
    ring.close()
