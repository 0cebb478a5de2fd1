"""The geometric finish on the device: k_geometryImage against the numpy restatement of
tests/geometry_ref.py for both filters and the four formats, the staged path against the slow path (MFSR_GEOMETRY_STAGE=0), a
case whose blocks fall on both sides of the stage's capacity and launches with boxes of exactly the capacity and one more, both
ways of reading the tone table, k_finishGeometry against k_geometryImage of the plain finish's float image, crops against the
whole, the identity against mfsr_finishRendered, bursts and their refusals, and the CLI.  Every comparison is bit for bit: uint32
views of floats, bytes of the integer outputs; outputs sit between canaries.  Two exceptions: the built-in gamma (powf: one LSB of
the format), and the affine ramp, which is compared with the float64 value of include/mfsr.h's mapping and
not with the restatement (tests/test_geometry_cpu.py derives the bound)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi
from tests import geometry_ref as G
from tests import render_ref as R
from tests import test_denoise_gpu as TD
from tests.kernels import guarded_upload
from tests.test_geometry_cpu import _struct

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
CANARY = 0xA5
FORMATS = (R.RGB16, R.RGB8, R.RGBA8, R.RGB10A2)
NAMES = {R.RGB16: "RGB16", R.RGB8: "RGB8", R.RGBA8: "RGBA8", R.RGB10A2: "RGB10A2"}
FILTERS = {"bilinear": G.BILINEAR, "cubic": G.CUBIC}
CCM, LUT = TD.CCM, TD.LUT
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _default_accumulate_variant():
    """as tests/test_denoise_gpu.py: kernel-level tests running before this file leave the process-wide selector at 1; the
    bursts below and the CLI they are compared with run the library's default"""
    L = capi.lib()
    found = L.raw["mfsr_get_accumulate_fast_exp"]()
    L.set_accumulate_fast_exp(2)
    yield
    L.set_accumulate_fast_exp(found)


def _render(fmt, rendered, lut_dev):
    r = capi.Render()
    r.format = fmt
    if rendered:
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*[float(v) for v in CCM])
        r.toneLut = lut_dev.data_ptr()
        r.toneSize = lut_dev.numel() - 1
    return r


def _layouts(fmt, w):
    """(offset, row bytes) of the integer output: odd byte offsets and padded rows where the format's stores allow them"""
    if fmt == R.RGB8:
        return [(1, 3 * w + 5), (0, 3 * w), (3, 3 * w + 2)]
    if fmt == R.RGB16:
        return [(2, 6 * w + 2), (0, 6 * w)]
    return [(4, 4 * w + 4), (0, 4 * w)]


def _expected(dense, off, row_bytes):
    h = dense.shape[0]
    want = np.full(off + row_bytes * h, CANARY, np.uint8)
    want[off:].reshape(h, row_bytes)[:, :dense.shape[1]] = dense
    return want


def _source(h, w, seed):
    """a ramp plus noise, seeded with NaN (cleaned to 0), negative values, values above 1 and above 65536 and 1e30; no inf (a
    weight of 0 times inf makes a NaN whose sign is the hardware's choice: see tests/test_finish_chain_gpu.py)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.15 + 0.7 * ((xx + 2 * yy) % 23) / 23.0
    p = (base[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.05, (h, w, 3))).astype(f32)
    special = np.array([np.nan, 1e30, -1e30, -3.0, 2.5, 70000.0, 0.0, -0.0, 1.0, 1e-8], f32)
    flat = p.reshape(-1)
    idx = np.arange(0, flat.size, 13)
    flat[idx] = special[np.arange(idx.size) % special.size]
    return p


_sources = {}


def _src(w, h):
    """(pixels, their guarded upload), once per size, unchanged"""
    if (w, h) not in _sources:
        p = _source(h, w, 100 * w + h)
        _sources[w, h] = (p, guarded_upload(p))
    return _sources[w, h]


def _mapping(name, sw, sh, filt):
    if name == "down":
        return G.lens(sw, sh, 53, 29, filter=filt)
    if name == "up":
        return G.lens(sw, sh, 131, 67, filter=filt)
    if name == "lens":   # the three channels land in different source pixels
        return G.lens(sw, sh, sw, sh, distortion=(0.2, -0.05, 0.0), lateral=(1.004, 0.997), filter=filt)
    if name == "clamp":  # 5 x 3 -> 9 x 7: every tap clamps
        return G.lens(sw, sh, 9, 7, filter=filt)
    if name == "one":    # 1 x 1 -> 4 x 3
        return G.lens(sw, sh, 4, 3, filter=filt)
    raise KeyError(name)


CASES = [("down", 70, 37), ("up", 70, 37), ("lens", 70, 37), ("clamp", 5, 3), ("one", 1, 1)]
_resampled = {}


def _want_o(name, sw, sh, fname):
    """the restatement's o of a case, once: the formats and both paths share it"""
    key = (name, sw, sh, fname)
    if key not in _resampled:
        _resampled[key] = G.resample(_src(sw, sh)[0], _mapping(name, sw, sh, FILTERS[fname]))
    return _resampled[key]


def _geometry_image(L, d_in, sw, sh, g, r, rect, off, rb, in_pitch=None, gamma=0):
    """one launch with guarded outputs: (float image, integer bytes)"""
    x, y, w, h = rect
    d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, f32))
    d_q, check_q = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
    L.geometryImage(d_in.data_ptr(), 12 * sw if in_pitch is None else in_pitch, sw, sh, d_f.data_ptr(), 12 * w, d_q.data_ptr() + off, rb,
                    None if r is None else ctypes.byref(r), ctypes.byref(g), gamma, x, y, w, h, None)
    check_f("float image")
    check_q("integer image")
    return d_f.cpu().numpy(), d_q.cpu().numpy()


def _assert_equal(got, o, fmt, rendered, off, rb, what):
    want_f, want_q = R.render(o, fmt, CCM if rendered else None, LUT if rendered else None)
    assert np.array_equal(got[0].view(np.uint32), want_f.view(np.uint32)), what + " (float image)"
    assert np.array_equal(got[1], _expected(R.as_bytes(want_q), off, rb)), what


# ---- 1. and 2. the tile body on a float image, staged and slow --------------------------------------------------------------
@pytest.mark.parametrize("stage", ["default", "0"])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_geometryImage_equals_the_restatement(fmt, stage, monkeypatch):
    """Source 70 x 37 (no multiple of any tile) down to 53 x 29, up to 131 x 67 (more than one block either way) and at its own
    size with k1 = 0.2, k2 = -0.05 and lateral (1.004, 0.997); 5 x 3 -> 9 x 7 (every tap clamps); 1 x 1.  Both filters, with and
    without matrix + table, the output layout cycling through the format's offsets and paddings.  Under the default and under
    MFSR_GEOMETRY_STAGE=0: both equal the restatement, hence each other."""
    if stage == "0":
        monkeypatch.setenv("MFSR_GEOMETRY_STAGE", "0")
    else:
        monkeypatch.delenv("MFSR_GEOMETRY_STAGE", raising=False)
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    k = FORMATS.index(fmt)
    for name, sw, sh in CASES:
        p, (d_in, check_in) = _src(sw, sh)
        for fname, filt in FILTERS.items():
            gd = _mapping(name, sw, sh, filt)
            g = _struct(gd)
            w, h = gd["outW"], gd["outH"]
            for rendered in (False, True):
                off, rb = _layouts(fmt, w)[k % len(_layouts(fmt, w))]
                k += 1
                got = _geometry_image(L, d_in, sw, sh, g, _render(fmt, rendered, lut_dev), (0, 0, w, h), off, rb)
                what = f"{NAMES[fmt]} {name} {fname} rendered={rendered} stage={stage} offset={off} rowBytes={rb}"
                _assert_equal(got, _want_o(name, sw, sh, fname), fmt, rendered, off, rb, what)
        check_in(name, unchanged=True)


def test_the_mappings_move_pixels_and_the_channels_apart():
    """no case is the identity in disguise: the lens case puts the three channels of some pixel into different source pixels,
    and both filters differ"""
    m = G.coords(_mapping("lens", 70, 37, G.CUBIC), 70, 37)
    assert (m["ix"][..., 0] != m["ix"][..., 2]).any() and (m["iy"][..., 0] != m["iy"][..., 2]).any()
    assert m["fx"].any() and m["fy"].any()
    for name, sw, sh in CASES[:4]:
        assert not np.array_equal(_want_o(name, sw, sh, "bilinear"), _want_o(name, sw, sh, "cubic")), name


def test_blocks_on_both_sides_of_the_stage_give_the_restatement(monkeypatch):
    """A step of 6 on a source of 8 stageW x 2 stageH and an output of 4 x 3 tiles around the same centre: the middle tiles' taps
    span far more than the stage (slow path), the outer tiles map beyond the source, where every tap clamps to the border (a box
    of one or two pixels: staged).  The default, MFSR_GEOMETRY_STAGE=0 and the restatement agree; pitched input rows."""
    L = capi.lib()
    tw, th, stw, sth = (ctypes.c_int(0) for _ in range(4))
    L.geometry_tile(*(ctypes.byref(v) for v in (tw, th, stw, sth)))
    tw, th, stw, sth = tw.value, th.value, stw.value, sth.value
    sw, sh, w, h = 8 * stw, 2 * sth, 4 * tw, 3 * th
    for fname, filt in FILTERS.items():
        gd = dict(outW=w, outH=h, filter=filt, ocx=f32(w / 2), ocy=f32(h / 2), scx=f32(sw / 2), scy=f32(sh / 2), stepX=f32(6), stepY=f32(6),
                  rnorm2=f32(1.0 / ((sw / 2) ** 2 + (sh / 2) ** 2)), k=np.array([[1.002, 0.05, 0, 0], [1, 0.05, 0, 0], [0.998, 0.05, 0, 0]], f32))
        fits = []
        for ty in range(3):
            for tx in range(4):
                x0, x1, y0, y1 = G.tap_box(gd, sw, sh, (tx * tw, ty * th, tw, th))
                fits.append(x1 - x0 + 1 <= stw and y1 - y0 + 1 <= sth)
        assert any(fits) and not all(fits), fits
        p = _source(sh, sw, 5)
        pitch = 12 * sw + 16
        rows = np.full((sh, pitch), CANARY, np.uint8)
        rows[:, :12 * sw] = p.view(np.uint8).reshape(sh, 12 * sw)
        d_in, check_in = guarded_upload(rows)
        o = G.resample(p, gd)
        g = _struct(gd)
        results = []
        for stage in (None, "0"):
            if stage is None:
                monkeypatch.delenv("MFSR_GEOMETRY_STAGE", raising=False)
            else:
                monkeypatch.setenv("MFSR_GEOMETRY_STAGE", stage)
            got = _geometry_image(L, d_in, sw, sh, g, None, (0, 0, w, h), 2, 6 * w + 2, in_pitch=pitch)
            _assert_equal(got, o, R.RGB16, False, 2, 6 * w + 2, f"{fname} stage={stage}")
            results.append(got)
        assert np.array_equal(results[0][0].view(np.uint32), results[1][0].view(np.uint32)) and np.array_equal(results[0][1], results[1][1])
        check_in(fname, unchanged=True)


# ---- 3. - 5. the finish kernel ------------------------------------------------------------------------------------------------
SW, SH, FBW, FBH, THR = 70, 37, 35, 19, 1e-3
_accs = {}


def _acc(hostile):
    """accumulators of SW x SH with weights on both sides of the threshold (the fallback resample runs) and zero weights;
    `hostile`: a NaN in an accumulator and in a weight too.  (accumulators, weights, fallback, their guarded uploads), once."""
    if hostile not in _accs:
        fin, wt, fb = TD._accumulators(SW, SH, FBW, FBH, THR)
        assert (wt == 0).any() and (wt < THR).any()
        if hostile:
            fin[3, 5, 1] = np.nan
            wt[20, 33, 2] = np.nan
            fin[36, 69, 0] = np.nan
        _accs[hostile] = (fin, wt, fb, [guarded_upload(a) for a in (fin, wt, fb)])
    return _accs[hostile]


def _finish_geometry(L, ups, g, r, rect, off, rb, dims=(SW, SH, FBW, FBH)):
    """dims: (source width, source height, fallback width, fallback height) of `ups`"""
    (d_fin, _), (d_wt, _), (d_fb, _) = ups
    sw, sh, fbw, fbh = dims
    x, y, w, h = rect
    d_f, check_f = guarded_upload(np.full((h, w, 3), -7.0, f32))
    d_q, check_q = guarded_upload(np.full(off + rb * h, CANARY, np.uint8))
    L.finishGeometry(d_fin.data_ptr(), d_wt.data_ptr(), 12 * sw, d_fb.data_ptr(), 12 * fbw, fbw, fbh, 0.0, 1.0, 0.0, 1.0, sw, sh,
                     d_f.data_ptr(), 12 * w, d_q.data_ptr() + off, rb, None if r is None else ctypes.byref(r), ctypes.byref(g), THR, 0,
                     x, y, w, h, None)
    check_f("float image")
    check_q("integer image")
    return d_f.cpu().numpy(), d_q.cpu().numpy()


def _plain_finish(L, ups, dims=(SW, SH, FBW, FBH)):
    (d_fin, _), (d_wt, _), (d_fb, _) = ups
    sw, sh, fbw, fbh = dims
    d_lin, chk = guarded_upload(np.zeros((sh, sw, 3), f32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * sw, d_fb.data_ptr(), 12 * fbw, fbw, fbh, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * sw, None, sw, sh, THR, 0, 65535.0, 0, 0, sw, sh, None)
    chk("plain finish")
    return d_lin


@pytest.mark.parametrize("stage", ["default", "0"])
@pytest.mark.parametrize("fname", list(FILTERS))
def test_finishGeometry_equals_geometryImage_of_the_plain_finish(fname, stage, monkeypatch):
    """mfsr_finishFusedWindow without gamma to a float image, then mfsr_geometryImage of it, against the one launch on the same
    accumulators: weights under the threshold (the fallback is sampled), zero weights and NaNs among the source pixels; the
    three mappings, every format once with matrix + table.  Both also equal the restatement of the plain float image."""
    if stage == "0":
        monkeypatch.setenv("MFSR_GEOMETRY_STAGE", "0")
    else:
        monkeypatch.delenv("MFSR_GEOMETRY_STAGE", raising=False)
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    fin, wt, fb, ups = _acc(True)
    d_lin = _plain_finish(L, ups)
    lin = d_lin.cpu().numpy()
    assert np.isnan(lin).any()
    for k, name in enumerate(("down", "up", "lens", "lens")):
        gd = _mapping(name, SW, SH, FILTERS[fname])
        g = _struct(gd)
        w, h = gd["outW"], gd["outH"]
        fmt = FORMATS[k]
        rendered = k % 2 == 1
        r = _render(fmt, rendered, lut_dev)
        off, rb = _layouts(fmt, w)[0]
        got = _finish_geometry(L, ups, g, r, (0, 0, w, h), off, rb)
        two = _geometry_image(L, d_lin, SW, SH, g, r, (0, 0, w, h), off, rb)
        what = f"{name} {fname} {NAMES[fmt]} stage={stage}"
        assert np.array_equal(got[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(got[1], two[1]), what
        _assert_equal(got, G.resample(lin, gd), fmt, rendered, off, rb, what)
    for _, chk in ups:
        chk("accumulators", unchanged=True)


@pytest.mark.parametrize("fname", list(FILTERS))
def test_a_rectangle_launched_on_its_own_is_the_crop_of_the_whole(fname):
    """three sub-rectangles of the 131 x 67 output: odd offsets, one single row, one single column"""
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    fin, wt, fb, ups = _acc(True)
    gd = G.lens(SW, SH, 131, 67, distortion=(0.1, 0.0, 0.0), lateral=(1.003, 0.998), filter=FILTERS[fname])
    g = _struct(gd)
    r = _render(R.RGB8, True, lut_dev)
    whole_f, whole_q = _finish_geometry(L, ups, g, r, (0, 0, 131, 67), 0, 3 * 131)
    whole_q = whole_q.reshape(67, 131, 3)
    p, (d_in, _) = _src(SW, SH)
    img_f, _ = _geometry_image(L, d_in, SW, SH, g, r, (0, 0, 131, 67), 0, 3 * 131)
    for x, y, w, h in ((67, 17, 41, 23), (3, 66, 128, 1), (129, 5, 1, 61)):
        got_f, got_q = _finish_geometry(L, ups, g, r, (x, y, w, h), 1, 3 * w + 5)
        assert np.array_equal(got_f.view(np.uint32), whole_f[y:y + h, x:x + w].view(np.uint32)), (x, y, w, h)
        assert np.array_equal(got_q, _expected(whole_q[y:y + h, x:x + w].reshape(h, 3 * w), 1, 3 * w + 5)), (x, y, w, h)
        crop_f, _ = _geometry_image(L, d_in, SW, SH, g, r, (x, y, w, h), 1, 3 * w + 5)
        assert np.array_equal(crop_f.view(np.uint32), img_f[y:y + h, x:x + w].view(np.uint32)), (x, y, w, h)


@pytest.mark.parametrize("fname", list(FILTERS))
def test_the_identity_geometry_gives_the_rendered_finish(fname):
    """positive accumulators, the identity description: mfsr_finishRendered's float image and bytes, every format"""
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    fin, wt, fb, ups = _acc(False)
    (d_fin, _), (d_wt, _), (d_fb, _) = ups
    g = capi.Geometry()
    L.geometry_defaults(SW, SH, ctypes.byref(g))
    g.filter = FILTERS[fname]
    for k, fmt in enumerate(FORMATS):
        r = _render(fmt, k % 2 == 0, lut_dev)
        rb = R.row_bytes(fmt, SW)
        d_f, check_f = guarded_upload(np.full((SH, SW, 3), -7.0, f32))
        d_q, check_q = guarded_upload(np.full(rb * SH, CANARY, np.uint8))
        L.finishRendered(d_fin.data_ptr(), d_wt.data_ptr(), 12 * SW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0,
                         d_f.data_ptr(), 12 * SW, d_q.data_ptr(), rb, ctypes.byref(r), SW, SH, THR, 0, 0, 0, SW, SH, None)
        check_f("rendered")
        check_q("rendered")
        got = _finish_geometry(L, ups, g, r, (0, 0, SW, SH), 0, rb)
        assert np.array_equal(got[0].view(np.uint32), d_f.cpu().numpy().view(np.uint32)), NAMES[fmt]
        assert np.array_equal(got[1], d_q.cpu().numpy()), NAMES[fmt]


# ---- 5b. the stage at its capacity, the table forms, the built-in gamma, and an anchor outside the restatement -----------------
@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("fname", list(FILTERS))
def test_boxes_of_exactly_the_stage_and_of_one_more_give_the_restatement(fname, axis, monkeypatch):
    """tests/test_geometry_cpu.py::capacity_edge finds, per filter, a launch in which one tile's box is exactly stageW columns
    wide and another's stageW + 1 (every box fits in height), and one with stageH and stageH + 1 rows (every box fits in width):
    the staged path at the last size it takes and the slow path at the first it must.  The default, MFSR_GEOMETRY_STAGE=0 and the
    restatement agree bit for bit, for RGB16 and RGB8 (one and four pixels a lane), for mfsr_geometryImage and for
    mfsr_finishGeometry.  (A stage that took one row too many would put row stageH of a channel's plane on row 0 of the next
    channel's; one column too many would still sit in the padded row pitch of stageW + 1 floats, two would not.)"""
    from tests.test_geometry_cpu import capacity_edge
    L = capi.lib()
    sw, sh, gd, boxes = capacity_edge(FILTERS[fname], axis)
    g = _struct(gd)
    w, h = gd["outW"], gd["outH"]
    p, (d_in, check_in) = _src(sw, sh)
    dims = (sw, sh, sw // 2 + 1, sh // 2 + 1)
    fin, wt, fb = TD._accumulators(sw, sh, dims[2], dims[3], THR)
    fin[3, 5, 1] = np.nan
    ups = [guarded_upload(a) for a in (fin, wt, fb)]
    lin = _plain_finish(L, ups, dims).cpu().numpy()
    want = {"image": G.resample(p, gd), "finish": G.resample(lin, gd)}
    assert not np.array_equal(want["image"].view(np.uint32), want["finish"].view(np.uint32))
    for fmt in (R.RGB16, R.RGB8):
        off, rb = _layouts(fmt, w)[0]
        for entry in ("image", "finish"):
            results = []
            for stage in (None, "0"):
                if stage is None:
                    monkeypatch.delenv("MFSR_GEOMETRY_STAGE", raising=False)
                else:
                    monkeypatch.setenv("MFSR_GEOMETRY_STAGE", stage)
                if entry == "image":
                    got = _geometry_image(L, d_in, sw, sh, g, _render(fmt, False, None), (0, 0, w, h), off, rb)
                else:
                    got = _finish_geometry(L, ups, g, _render(fmt, False, None), (0, 0, w, h), off, rb, dims)
                _assert_equal(got, want[entry], fmt, False, off, rb,
                              f"{fname} {axis} {NAMES[fmt]} {entry} stage={stage} boxes {sorted(set(boxes))}")
                results.append(got)
            assert np.array_equal(results[0][0].view(np.uint32), results[1][0].view(np.uint32)) and np.array_equal(results[0][1], results[1][1])
    check_in(f"{fname} {axis}", unchanged=True)
    for _, chk in ups:
        chk(f"{fname} {axis}", unchanged=True)


@pytest.mark.parametrize("how", ["lds", "cache"])
@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_geometry_with_the_table_in_lds_and_through_the_cache(fmt, how, monkeypatch):
    """MFSR_RENDER_LUT=lds | cache forces one way of reading the tone table (unset, the geometric kernels read it through the
    cache): the lens and the up case of test_geometryImage_equals_the_restatement and one mfsr_finishGeometry launch, with
    matrix + table, both filters, every format.  Both give the restatement's bits."""
    monkeypatch.setenv("MFSR_RENDER_LUT", how)
    monkeypatch.delenv("MFSR_GEOMETRY_STAGE", raising=False)
    L = capi.lib()
    lut_dev = torch.from_numpy(LUT).to(DEV)
    assert lut_dev.numel() - 1 <= 8192          # a longer table is read through the cache whatever is asked
    r = _render(fmt, True, lut_dev)
    fin, wt, fb, ups = _acc(True)
    lin = _plain_finish(L, ups).cpu().numpy()
    for fname, filt in FILTERS.items():
        for name, sw, sh in (CASES[2], CASES[1]):
            p, (d_in, check_in) = _src(sw, sh)
            gd = _mapping(name, sw, sh, filt)
            w, h = gd["outW"], gd["outH"]
            off, rb = _layouts(fmt, w)[0]
            got = _geometry_image(L, d_in, sw, sh, _struct(gd), r, (0, 0, w, h), off, rb)
            _assert_equal(got, _want_o(name, sw, sh, fname), fmt, True, off, rb, f"{how} {NAMES[fmt]} {name} {fname}")
            check_in(name, unchanged=True)
        gd = _mapping("lens", SW, SH, filt)
        off, rb = _layouts(fmt, SW)[0]
        got = _finish_geometry(L, ups, _struct(gd), r, (0, 0, SW, SH), off, rb)
        _assert_equal(got, G.resample(lin, gd), fmt, True, off, rb, f"{how} {NAMES[fmt]} finishGeometry {fname}")
    for _, chk in ups:
        chk("accumulators", unchanged=True)


def _unpack(got, fmt, w, h, off, rb):
    """the integer image of _geometry_image as [h, w, 3] int64 samples (alpha asserted opaque)"""
    rows = np.ascontiguousarray(got[off:].reshape(h, rb)[:, :R.row_bytes(fmt, w)])
    if fmt == R.RGB10A2:
        d = rows.view(np.uint32).reshape(h, w).astype(np.int64)
        assert (d >> 30 == 3).all()
        return np.stack([d & 1023, d >> 10 & 1023, d >> 20 & 1023], axis=-1)
    if fmt == R.RGB16:
        return rows.view(np.uint16).reshape(h, w, 3).astype(np.int64)
    px = rows.reshape(h, w, -1).astype(np.int64)
    assert fmt == R.RGB8 or (px[..., 3] == 255).all()
    return px[..., :3]


@pytest.mark.parametrize("fmt", FORMATS, ids=NAMES.get)
def test_geometry_builtin_gamma_within_one_lsb(fmt):
    """applyGamma = 1 without a table, as tests/test_render_gpu.py::test_renderImage_builtin_gamma_within_one_lsb: powf is the only
    inexact operation, so the integers are within one LSB of the format of numpy's pow applied to the restatement's o (DESIGN.md
    section 3.1), and equal wherever o lies on the linear segment (o <= 0.0031308; NaN and negatives included: they clamp to 0).
    The left third of the source is scaled into the linear segment."""
    L = capi.lib()
    sw, sh = 70, 37
    p = _source(sh, sw, 77)
    p[:, :24] = (np.abs(p[:, :24]) * f32(0.003)).astype(f32)
    d_in, check_in = guarded_upload(p)
    gd = _mapping("up", sw, sh, G.CUBIC if FORMATS.index(fmt) % 2 else G.BILINEAR)
    w, h = gd["outW"], gd["outH"]
    o = G.resample(p, gd)
    off, rb = _layouts(fmt, w)[0]
    got_f, got_q = _geometry_image(L, d_in, sw, sh, _struct(gd), _render(fmt, False, None), (0, 0, w, h), off, rb, gamma=1)
    check_in("gamma", unchanged=True)
    diff = np.abs(_unpack(got_q, fmt, w, h, off, rb) - R.quantise(R.gamma(o), fmt))
    with np.errstate(invalid="ignore"):
        linear = ~(o > f32(0.0031308))
        assert int((linear & (o > 0)).sum()) > 1000 and int((~linear).sum()) > 1000
    print(f"{NAMES[fmt]}: max difference {diff.max()} LSB, {int((diff > 0).sum())} of {diff.size} samples differ")
    assert diff.max() <= 1
    assert diff[linear].max() == 0
    assert np.array_equal(got_f[linear].view(np.uint32), R.gamma(o)[linear].view(np.uint32))


@pytest.mark.parametrize("fname", list(FILTERS))
def test_geometryImage_reproduces_an_affine_ramp_at_the_float64_coordinate(fname):
    """The device against the float64 value of include/mfsr.h's mapping directly, not against the restatement: an affine ramp
    under a lens mapping with distortion and a lateral scale, compared wherever no tap clamps, with the bound derived in
    tests/test_geometry_cpu.py (which holds the restatement to the same)."""
    from tests.test_geometry_cpu import ANCHOR_CASES, affine_ramp, anchor_description, assert_affine_anchor
    L = capi.lib()
    for sw, sh, ow, oh in ANCHOR_CASES:
        d_in, check_in = guarded_upload(affine_ramp(sw, sh))
        gd = anchor_description(sw, sh, ow, oh, FILTERS[fname])
        got_f, _ = _geometry_image(L, d_in, sw, sh, _struct(gd), None, (0, 0, ow, oh), 2, 6 * ow + 2)
        check_in("ramp", unchanged=True)
        assert_affine_anchor(got_f, gd, sw, sh, f"device {sw}x{sh} -> {ow}x{oh} {fname}")


# ---- 6. bursts ----------------------------------------------------------------------------------------------------------------
def _burst():
    from multi_frame_super_resolution_amd import synth
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    frames = [f.contiguous().to(DEV) for f in synth.make_burst(96, 64, 3)[0]]
    cfg = default_config(96, 64, 3, scale=2)
    cfg.applyGamma = 0
    return BurstPipeline(cfg, DEV), frames


def test_burst_finish_geometry_equals_the_restatement_of_the_plain_float_image():
    from multi_frame_super_resolution_amd.pipeline import lens_geometry
    pipe, frames = _burst()
    lin, q0 = pipe.process(frames)
    lin, q0 = lin.cpu().numpy().copy(), TD._np(q0).copy()
    assert pipe.geometry_finishes() == 0
    g = lens_geometry(192, 128, 144, 96, distortion=(0.1, 0, 0), lateral=(1.003, 0.998))
    o = G.resample(lin, G.lens(192, 128, 144, 96, distortion=(0.1, 0, 0), lateral=(1.003, 0.998)))
    # without a render description: {RGB16, no matrix, no table}
    fl, q = pipe.finish_geometry(g)
    want_f, want_q = R.render(o, R.RGB16)
    assert tuple(fl.shape) == (96, 144, 3) and tuple(q.shape) == (96, 144, 3)
    assert np.array_equal(fl.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    assert np.array_equal(TD._np(q), want_q)
    assert pipe.geometry_finishes() == 1
    # a following plain finish is unchanged
    lin2, q2 = pipe.finish()
    assert np.array_equal(lin2.cpu().numpy().view(np.uint32), lin.view(np.uint32)) and np.array_equal(TD._np(q2), q0)
    # with one: RGB8, matrix, table.  The geometric call fuses what is waiting itself (no finish before it).
    pipe.set_render(capi.OUT_RGB8, matrix=CCM, tone_lut=LUT)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for i, f in enumerate(frames):
        pipe.add_frame(f, i == 0)
    fl, q = pipe.finish_geometry(g)
    want_f, want_q = R.render(o, R.RGB8, CCM, LUT)
    assert np.array_equal(fl.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    assert q.dtype == torch.uint8 and np.array_equal(TD._np(q), want_q)
    only_q = pipe.finish_geometry(g, want_float=False)
    assert only_q[0] is None and np.array_equal(TD._np(only_q[1]), want_q)
    assert pipe.geometry_finishes() == 2
    _, q3 = pipe.finish()
    assert np.array_equal(TD._np(q3), R.render(lin, R.RGB8, CCM, LUT)[1])
    pipe.close()


def test_burst_finish_geometry_refusals_leave_the_burst_usable():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config, lens_geometry
    pipe, frames = _burst()
    g = lens_geometry(192, 128, 144, 96)
    _, q0 = pipe.process(frames)
    q0 = q0.clone()
    entry = capi.lib().raw["mfsr_burst_finish_geometry"]
    out = torch.empty(96, 144, 3, dtype=torch.float32, device=DEV)

    def refused(p):
        return entry(p._h, p._img_out.data_ptr(), p._total_weights.data_ptr(), ctypes.byref(g), out.data_ptr(), 12 * 144, None, 0, None)

    assert refused(pipe) == 0
    # an installed sharpen / denoise / chain description, a two-plane format
    for on, off in ((lambda: pipe.set_sharpen(amount=1.0), lambda: pipe.set_sharpen(None)),
                    (lambda: pipe.set_denoise(strength=3.0), lambda: pipe.set_denoise(None)),
                    (lambda: pipe.set_finish_chain(sharpen=dict(amount=1.0)), lambda: pipe.set_finish_chain()),
                    (lambda: pipe.set_render(capi.OUT_NV12), lambda: pipe.set_render(None))):
        on()
        pipe.process(frames)
        assert refused(pipe) == -1
        with pytest.raises(capi.MfsrError):
            pipe.finish_geometry(g)
        assert pipe.geometry_finishes() == 0
        off()
    # local tone
    pipe.set_local_tone(shadows=0.5)
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for i, f in enumerate(frames):
        pipe.add_frame(f, i == 0)
    pipe.local_tone()
    assert refused(pipe) == -1
    pipe.finish()
    pipe.set_local_tone(None)
    # a bad description, no output
    bad = lens_geometry(192, 128, 144, 96)
    bad.stepX = 9.0
    assert entry(pipe._h, pipe._img_out.data_ptr(), pipe._total_weights.data_ptr(), ctypes.byref(bad), out.data_ptr(), 12 * 144, None, 0, None) == -1
    assert entry(pipe._h, pipe._img_out.data_ptr(), pipe._total_weights.data_ptr(), ctypes.byref(g), None, 0, None, 0, None) == -1
    # ... and the burst is as usable as before
    _, q = pipe.process(frames)
    assert torch.equal(q, q0)
    assert refused(pipe) == 0 and pipe.geometry_finishes() == 1
    pipe.close()
    # a burst with a window
    cfg = default_config(96, 64, 3, scale=2)
    cfg.applyGamma = 0
    pw = BurstPipeline(cfg, DEV, window=(32, 16, 64, 48))
    _, qw = pw.process(frames)
    assert refused(pw) == -1
    assert torch.equal(pw.process(frames)[1], qw)
    pw.close()


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_out_size_and_lens_write_the_python_paths_bytes(tmp_path):
    """MFSR_OUT_SIZE + MFSR_LENS on the bundled city burst: _sr_result has the requested size and holds the bytes
    BurstPipeline.finish_geometry gives on the same frames with the same configuration (as
    tests/test_cli_gpu.py::test_cli_on_the_bundled_city_frames compares the plain result); the refusals."""
    import shutil
    Image = pytest.importorskip("PIL.Image", reason="tests/test_cli_gpu.py reads the CLI's PNGs with PIL")
    cli = os.path.join(ROOT, "apps", "multi_frame_sr")
    if not os.path.exists(cli):
        pytest.skip("apps/multi_frame_sr not built")
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, lens_geometry
    from tests.test_bundled_burst import CITY, _cfg, _raws
    for i in range(5):
        shutil.copy(os.path.join(CITY, f"img_{i:06d}.png"), tmp_path / f"img_{i:06d}.png")
    env = dict(os.environ, MFSR_OUT_SIZE="768x384", MFSR_LENS="0.08,-0.01,0,1.002,0.998")
    p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    out = np.asarray(Image.open(tmp_path / "city_farneback_sr_result.png"))
    assert out.shape == (384, 768, 3)
    assert np.asarray(Image.open(tmp_path / "city_farneback_sr2_result.png")).shape == (512, 1024, 3)
    raws, W, H = _raws(5)
    cfg = _cfg(W, H, 5)
    cfg.preAlign = 1
    cfg.lkIterations = 3
    pipe = BurstPipeline(cfg, DEV)
    pipe.set_render(capi.OUT_RGB8)
    pipe.process([torch.from_numpy(r.view(np.int16)).to(DEV) for r in raws])
    _, q = pipe.finish_geometry(lens_geometry(2 * W, 2 * H, 768, 384, distortion=(0.08, -0.01, 0), lateral=(1.002, 0.998)), want_float=False)
    assert np.array_equal(q.cpu().numpy(), out)
    pipe.close()
    for extra in (dict(MFSR_SHARPEN="1"), dict(MFSR_DENOISE="3"), dict(MFSR_LOCAL_TONE="0.5"), dict(MFSR_GPUS="2"), dict(MFSR_LENS="0.1,0,0,1.0"),
                  dict(MFSR_OUT_SIZE="768"), dict(MFSR_LENS="9")):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=dict(env, **extra))
        assert p.returncode != 0 and ("MFSR_LENS" in p.stderr or "MFSR_OUT_SIZE" in p.stderr), (extra, p.stderr)
