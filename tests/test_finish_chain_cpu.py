"""The finish chain without a device: the layout of mfsr_finish_chain against a compiled probe, the host
refusals of its validator and of its two launch entries (every argument is checked before any device call, so host pointers
are never dereferenced: a call that got as far as the device would not return MFSR_E_INVALID), and known answers of the numpy
composition (tests/chain_ref.py) that tests/test_finish_chain_gpu.py compares the kernels with."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi
from tests import chain_ref as C
from tests import denoise_ref as D
from tests import local_tone_ref as LT
from tests import render_ref as R
from tests import sharpen_ref as S
from tests import yuv_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
f32 = np.float32


def _chain(rd=2, rs=1, tone=False, strength=3.0, amount=1.0):
    """a valid chain: every description valid, the stages on as asked for"""
    c = capi.FinishChain()
    c.denoise.radius, c.denoise.strength, c.denoise.gain, c.denoise.alpha, c.denoise.beta = rd, strength, 2.0, 0.01, 0.001
    c.sharpen.radius, c.sharpen.amount = rs, amount
    c.sharpen.taps[0], c.sharpen.taps[1] = 0.5, 0.25
    for d in range(2, rs + 1):
        c.sharpen.taps[d] = 0.0
    lt = c.localTone
    lt.cell, lt.bins, lt.smooth, lt.shadows, lt.highlights, lt.pivot, lt.maxGain = 16, 16, 1, 0.5, 0.25, 0.0, 4.0
    c.useLocalTone = 1 if tone else 0
    return c


def test_finish_chain_struct_mirrors_the_header():
    probe = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mfsr.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu\n", sizeof(mfsr_finish_chain), offsetof(mfsr_finish_chain, denoise),
        offsetof(mfsr_finish_chain, sharpen), offsetof(mfsr_finish_chain, localTone), offsetof(mfsr_finish_chain, useLocalTone),
        offsetof(mfsr_finish_chain, reserved)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = list(map(int, subprocess.check_output([exe], text=True).split()))
    F = capi.FinishChain
    assert got == [ctypes.sizeof(F), F.denoise.offset, F.sharpen.offset, F.localTone.offset, F.useLocalTone.offset, F.reserved.offset]
    assert got == [172, 0, 48, 96, 140, 144]


def test_entry_points_resolve():
    raw = capi.lib().raw
    for name in ("mfsr_finish_chain_validate", "mfsr_finish_chain_reach", "mfsr_chain_tile", "mfsr_chainImage", "mfsr_finishChain",
                 "mfsr_burst_set_finish_chain", "mfsr_stream_set_finish_chain", "mfsr_burst_debug_chained"):
        assert name in raw, name
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    assert raw["mfsr_chain_tile"](ctypes.byref(tw), ctypes.byref(th)) == 0 and (tw.value, th.value) == (64, 16)
    assert raw["mfsr_chain_tile"](None, ctypes.byref(th)) == INVALID


def _set(path, value):
    def f(c):
        obj = c
        for name in path[:-1]:
            obj = getattr(obj, name)
        last = path[-1]
        if isinstance(last, tuple):
            getattr(obj, last[0])[last[1]] = value
        else:
            setattr(obj, last, value)
    return f


BAD = [
    ("denoise radius 4", _set(("denoise", "radius"), 4)),
    ("denoise radius -1", _set(("denoise", "radius"), -1)),
    ("denoise strength 17", _set(("denoise", "strength"), 17.0)),
    ("denoise strength 0.01", _set(("denoise", "strength"), 0.01)),
    ("denoise strength NaN", _set(("denoise", "strength"), float("nan"))),
    ("denoise gain 0", _set(("denoise", "gain"), 0.0)),
    ("denoise gain 2000", _set(("denoise", "gain"), 2000.0)),
    ("denoise alpha 2", _set(("denoise", "alpha"), 2.0)),
    ("denoise beta -1", _set(("denoise", "beta"), -1.0)),
    ("denoise wLo -1", _set(("denoise", "wLo"), -1.0)),
    ("denoise wHi inf", _set(("denoise", "wHi"), float("inf"))),
    ("denoise reserved", _set(("denoise", ("reserved", 4)), 1)),
    ("sharpen radius 5", _set(("sharpen", "radius"), 5)),
    ("sharpen radius -1", _set(("sharpen", "radius"), -1)),
    ("sharpen tap NaN", _set(("sharpen", ("taps", 1)), float("nan"))),
    ("sharpen tap 4.5", _set(("sharpen", ("taps", 0)), 4.5)),
    ("sharpen amount 17", _set(("sharpen", "amount"), 17.0)),
    ("sharpen amount -1", _set(("sharpen", "amount"), -1.0)),
    ("sharpen threshold -1", _set(("sharpen", "threshold"), -1.0)),
    ("sharpen reserved", _set(("sharpen", ("reserved", 0)), 1)),
    ("local tone cell 24", _set(("localTone", "cell"), 24)),
    ("local tone cell 8", _set(("localTone", "cell"), 8)),
    ("local tone bins 5", _set(("localTone", "bins"), 5)),
    ("local tone smooth 5", _set(("localTone", "smooth"), 5)),
    ("local tone shadows 2", _set(("localTone", "shadows"), 2.0)),
    ("local tone highlights NaN", _set(("localTone", "highlights"), float("nan"))),
    ("local tone pivot -1", _set(("localTone", "pivot"), -1.0)),
    ("local tone maxGain 0.5", _set(("localTone", "maxGain"), 0.5)),
    ("local tone reserved", _set(("localTone", ("reserved", 3)), 1)),
    ("useLocalTone 2", _set(("useLocalTone",), 2)),
    ("reserved[0]", _set((("reserved", 0),), 1)),
    ("reserved[6]", _set((("reserved", 6),), -1)),
]


@pytest.mark.parametrize("what,spoil", BAD, ids=[b[0] for b in BAD])
def test_validate_refuses_each_bad_field(what, spoil):
    raw = capi.lib().raw
    c = _chain(tone=True)
    assert raw["mfsr_finish_chain_validate"](ctypes.byref(c)) == 0
    spoil(c)
    assert raw["mfsr_finish_chain_validate"](ctypes.byref(c)) == INVALID, what
    rows = ctypes.c_int(-5)
    assert raw["mfsr_finish_chain_reach"](ctypes.byref(c), ctypes.byref(rows)) == INVALID and rows.value == -5, what
    # ... and so do the launch entries (host memory: the device is never reached)
    buf = (ctypes.c_float * (3 * 8 * 8 * 3))()
    a = ctypes.addressof(buf)
    g = a + 2 * 768
    assert raw["mfsr_chainImage"](a, 96, None, 0, a + 768, 96, None, 0, None, 0, 8, 8, None, 0, ctypes.byref(c), g, 0, 0, 8, 8,
                                  None) == INVALID, what
    assert raw["mfsr_finishChain"](a, a, 96, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, a + 768, 96, None, 0, None, 0, None, 8, 8, 1e-3, 0, 0, 0,
                                   8, 8, ctypes.byref(c), g, 0, 0, None) == INVALID, what


def test_reach_is_the_sum_of_the_radii_of_the_stages_that_are_on():
    reach = capi.lib().raw["mfsr_finish_chain_reach"]

    def of(c):
        rows = ctypes.c_int(-1)
        assert reach(ctypes.byref(c), ctypes.byref(rows)) == 0
        return rows.value

    assert of(_chain(2, 1)) == 3 and of(_chain(3, 4)) == 7 and of(_chain(1, 1, tone=True)) == 2
    assert of(_chain(0, 4)) == 4 and of(_chain(3, 0)) == 3 and of(_chain(0, 0, tone=True)) == 0
    assert of(_chain(3, 4, strength=0.0)) == 4          # strength 0: the denoise stage is off whatever its radius
    assert of(_chain(3, 4, amount=0.0)) == 3            # amount 0: the sharpen stage likewise
    assert of(_chain(3, 4, strength=0.0, amount=0.0)) == 0
    assert reach(ctypes.byref(_chain()), None) == INVALID and reach(None, ctypes.byref(ctypes.c_int())) == INVALID


def _image_call(c, w=8, h=8, out_img="free", out=None, uv=None, fmt=None, grid=None, rb=None, uvrb=None, count=None, col=0, row=0,
                full=None):
    """mfsr_chainImage on host memory: `in` at a, a free area after it"""
    buf = (ctypes.c_float * (3 * 16 * 16 * 6))()
    a = ctypes.addressof(buf)
    n = 12 * w * h
    where = {"free": a + 2 * n, "in": a, None: None}
    r = None
    if fmt is not None:
        r = capi.Render()
        r.format = fmt
    bps = 2 if fmt == capi.OUT_P010 else 1
    fw, fh = (w, h) if full is None else full
    res = capi.lib().raw["mfsr_chainImage"](a, 12 * w, None if count is None else a + count, 12 * w, where.get(out_img, out_img), 12 * w,
                                            None if out is None else a + out, (bps * w if rb is None else rb),
                                            None if uv is None else a + uv, (bps * w if uvrb is None else uvrb), w, h,
                                            None if r is None else ctypes.byref(r), 0, ctypes.byref(c),
                                            None if grid is None else a + grid, col, row, fw, fh, None)
    del buf
    return res


def test_chainImage_refusals_without_a_device():
    n = 12 * 8 * 8
    assert _image_call(_chain(0, 0)) == INVALID                               # every stage off
    assert _image_call(_chain(2, 1, strength=0.0, amount=0.0)) == INVALID     # ... by strength and amount
    assert _image_call(_chain(2, 1), out_img=None) == INVALID                 # no output
    assert _image_call(_chain(2, 1), out_img="in") == INVALID                 # in place
    # the grid if and only if the local tone is on
    assert _image_call(_chain(2, 1), grid=4 * n) == INVALID
    assert _image_call(_chain(2, 1, tone=True)) == INVALID
    assert _image_call(_chain(2, 1, tone=True), grid=4 * n + 2) == INVALID    # misaligned
    assert _image_call(_chain(0, 0, tone=True), grid=4 * n, full=(8, 4)) == INVALID     # the image outside the full frame
    assert _image_call(_chain(0, 0, tone=True), grid=4 * n, col=1) == INVALID
    # two-plane formats: even extents, both planes or neither, no plane over the input
    nv = capi.OUT_NV12
    assert _image_call(_chain(2, 1), w=7, fmt=nv, out_img=None, out=3 * n, uv=4 * n) == INVALID
    assert _image_call(_chain(2, 1), h=7, fmt=nv, out_img=None, out=3 * n, uv=4 * n) == INVALID
    assert _image_call(_chain(2, 1), fmt=nv, out_img=None, out=3 * n) == INVALID                  # the Y plane alone
    assert _image_call(_chain(2, 1), fmt=nv, out_img=None, uv=3 * n) == INVALID                   # the chroma plane alone
    assert _image_call(_chain(2, 1), fmt=nv, out_img=None, out=3 * n, uv=n - 1) == INVALID        # chroma over the input's last byte
    assert _image_call(_chain(2, 1), fmt=nv, out_img=None, out=n - 1, uv=3 * n) == INVALID        # Y likewise
    assert _image_call(_chain(2, 1), fmt=nv, out_img=None, out=3 * n, uv=4 * n, uvrb=7) == INVALID   # a short chroma row
    assert _image_call(_chain(2, 1), fmt=capi.OUT_P010, out_img=None, out=3 * n + 1, uv=4 * n) == INVALID   # a misaligned P010 plane
    assert _image_call(_chain(2, 1), fmt=capi.OUT_RGB8, out_img=None, out=3 * n, uv=4 * n, rb=24) == INVALID   # a chroma plane with one plane
    # the count image is read too: no output over it
    assert _image_call(_chain(2, 1), count=2 * n) == INVALID


def _finish_call(c, out_img=None, out=None, uv=None, fmt=None, above=2, below=2, grid=None, rows=4, w=8, first=4, full=12):
    """mfsr_finishChain on host memory: rows [first, first + rows) of accumulators of `full` rows; offsets are bytes from the
    accumulators' first byte (the weights follow them, then a free area)"""
    buf = (ctypes.c_float * (3 * w * full * 6))()
    base = ctypes.addressof(buf)
    row = 12 * w
    acc, wts = base, base + row * full
    r = None
    if fmt is not None:
        r = capi.Render()
        r.format = fmt
    bps = 2 if fmt == capi.OUT_P010 else (1 if fmt == capi.OUT_NV12 else 6)

    def at(o):
        return None if o is None else base + o

    res = capi.lib().raw["mfsr_finishChain"](acc + first * row, wts + first * row, row, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, at(out_img), row,
                                             at(out), bps * w, at(uv), bps * w, None if r is None else ctypes.byref(r), w, rows, 1e-3, 0, 0,
                                             first, w, full, ctypes.byref(c), at(grid), above, below, None)
    del buf
    return res


def test_finishChain_refusals_without_a_device():
    row, full = 96, 12
    A, W, FREE = 0, row * full, 2 * row * full           # the accumulators, the weights, a free area
    c = _chain(1, 1)
    assert _finish_call(_chain(0, 0), out_img=FREE) == INVALID               # every stage off
    assert _finish_call(c, out_img=A + 4 * row) == INVALID                   # in place on the accumulators
    assert _finish_call(c, out_img=W + 4 * row) == INVALID                   # ... on the weights
    assert _finish_call(c, out_img=A) == INVALID                             # rows 0..3: the last two are the reach above
    assert _finish_call(c, out_img=A + 8 * row) == INVALID                   # rows 8..11: the first two are the reach below
    assert _finish_call(c, out=W + 9 * row + row // 2) == INVALID            # the integers over the last row of reach
    nv = capi.OUT_NV12
    assert _finish_call(c, fmt=nv, out=FREE, uv=W + 10 * row - 8) == INVALID   # the chroma plane over the reach below (2 rows of 8 bytes)
    assert _finish_call(c, fmt=nv, out=A + 2 * row, uv=FREE) == INVALID      # the Y plane over the reach above
    assert _finish_call(c, fmt=nv, out=FREE) == INVALID                      # one plane missing
    assert _finish_call(c, fmt=nv, uv=FREE) == INVALID
    assert _finish_call(c, fmt=nv, out=FREE, uv=FREE + 512, rows=3, below=3) == INVALID    # odd rows
    assert _finish_call(c, fmt=nv, out=FREE, uv=FREE + 512, w=7) == INVALID                # odd width
    assert _finish_call(c, out_img=FREE, grid=FREE + 4096) == INVALID        # a grid without useLocalTone
    assert _finish_call(_chain(1, 1, tone=True), out_img=FREE) == INVALID    # ... and the reverse
    # a reach outside the full frame (not an overlap)
    assert _finish_call(c, out_img=FREE, above=5) == INVALID
    assert _finish_call(c, out_img=FREE, below=5) == INVALID
    assert _finish_call(c, out_img=FREE, above=-1) == INVALID and _finish_call(c, out_img=FREE, below=-1) == INVALID


# ---- known answers of the restatement ----------------------------------------------------------------------------------------
def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 0.15 + 0.7 * ((xx + 2 * yy) % 11) / 11.0
    return (base[..., None] * np.array([1.0, 0.8, 0.6]) + rng.normal(0, 0.05, (h, w, 3))).astype(f32)


DEN = dict(radius=2, strength=3.0, gain=4.0, alpha=0.05, beta=0.01)
SHARP = dict(taps=np.array([0.4, 0.2, 0.1], f32), amount=1.5, threshold=0.01)


def _grid(h, w, cell=16, bins=8, seed=3):
    gx, gy, gz = LT.grid_size(w, h, cell, bins)
    return dict(grid=np.random.default_rng(seed).uniform(0.5, 2.0, (gy, gx, gz)).astype(f32), cell=cell)


def test_a_chain_with_one_stage_is_that_stages_restatement():
    h, w = 21, 37
    p = _image(h, w, 1)
    n = np.random.default_rng(2).uniform(0.3, 6.0, (h, w, 3)).astype(f32)
    lt = _grid(h, w)
    m = np.array([1.5, -0.3, -0.2, -0.2, 1.4, -0.2, 0.0, -0.5, 1.5], f32)
    assert np.array_equal(C.chain(p, n, denoise=DEN).view(np.uint32), D.denoise(p, n, **DEN).view(np.uint32))
    assert np.array_equal(C.chain(p, n, sharpen=SHARP).view(np.uint32), S.sharpen(p, **SHARP).view(np.uint32))
    assert np.array_equal(C.chain(p, n, local_tone=lt, m=m, offset=(3, 5)).view(np.uint32),
                          LT.apply(p, lt["grid"], lt["cell"], m, (3, 5)).view(np.uint32))
    # ... and two stages are one after the other
    want = S.sharpen(D.denoise(p, n, **DEN), **SHARP)
    assert np.array_equal(C.chain(p, n, denoise=DEN, sharpen=SHARP).view(np.uint32), want.view(np.uint32))
    assert C.reach(DEN, SHARP) == 4 and C.reach(None, SHARP) == 2 and C.reach(DEN, None) == 2 and C.reach() == 0
    # the render step: render_ref's for one plane, yuv_ref's for two
    f, q = C.render(p[:20, :36], R.RGB8, n[:20, :36], denoise=DEN, sharpen=SHARP, m=m)
    wf, wq = R.render(S.sharpen(D.denoise(p[:20, :36], n[:20, :36], **DEN), **SHARP), R.RGB8, m)
    assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(q, wq)
    f, yq, uv = C.render(p[:20, :36], Y.NV12, n[:20, :36], sharpen=SHARP, colour=Y.BT2020 | Y.FULL)
    wf, wy, wuv = Y.render(S.sharpen(p[:20, :36], **SHARP), Y.NV12, colour=Y.BT2020 | Y.FULL)
    assert np.array_equal(f.view(np.uint32), wf.view(np.uint32)) and np.array_equal(yq, wy) and np.array_equal(uv, wuv)


def test_valid_rows_are_the_chain_of_those_rows_cropped():
    h, w = 30, 20
    p = _image(h, w, 5)
    whole = C.chain(p, denoise=DEN, sharpen=SHARP)
    r = C.reach(DEN, SHARP)
    # a stripe with the reach on both sides is the crop of the whole; with none it is the chain of its own rows
    got = C.chain(p, denoise=DEN, sharpen=SHARP, valid=(10 - r, 20 + r), rows=(10, 20))
    assert np.array_equal(got.view(np.uint32), whole[10:20].view(np.uint32))
    alone = C.chain(p, denoise=DEN, sharpen=SHARP, valid=(10, 20))
    assert np.array_equal(alone.view(np.uint32), C.chain(p[10:20], denoise=DEN, sharpen=SHARP).view(np.uint32))
    assert not np.array_equal(alone.view(np.uint32), whole[10:20].view(np.uint32))
    # the gain is looked up at the pixel's place in the full frame whatever the stripe
    lt = _grid(h, w, bins=4)
    t = C.chain(p, local_tone=lt, valid=(16, 30), rows=(17, 30))
    assert np.array_equal(t.view(np.uint32), C.chain(p, local_tone=lt)[17:30].view(np.uint32))


@pytest.mark.parametrize("stages", ["D", "S", "L", "DS", "DL", "SL", "DSL"])
def test_a_constant_image_stays_constant_times_the_gain(stages):
    h, w, v = 12, 18, f32(0.375)
    p = np.full((h, w, 3), v, f32)
    taps = np.array([0.5, 0.25], f32)                       # sums to 1 in exact binary fractions: the blur of a constant is exact
    lt = _grid(h, w, bins=4)
    t = C.chain(p, None, denoise=DEN if "D" in stages else None, sharpen=dict(taps=taps, amount=2.0) if "S" in stages else None,
                local_tone=lt if "L" in stages else None)
    want = p * (LT.gain(p, lt["grid"], lt["cell"])[..., None] if "L" in stages else f32(1))
    assert np.array_equal(t.view(np.uint32), want.astype(f32).view(np.uint32))


def test_the_sharpen_reads_the_denoised_value_of_the_clamped_pixel():
    """5 x 4, an impulse of 9 at (x, y) = (1, 1), three equal channels.  Denoise R = 1 with a tolerance so wide that every tap
    weighs 1 (t < 2^-25, so 1 - t rounds to 1): d is the 3 x 3 mean with replicated borders, 1 at x, y <= 2 and 0 elsewhere.
    Sharpen R = 1, taps (1/2, 1/4), amount 1: b = rf(y) cf(x) with cf = (1, 1, 3/4, 1/4, 0) and rf = (1, 1, 3/4, 1/4), because
    the tap left of column 0 reads d at the clamped column 0, which is 1.  (The denoise run AT column -1 would see the clamped
    columns 0, 0, 0 only, never the impulse, and give 0: cf(0) would be 3/4 and the corner 1.4375.)"""
    p = np.zeros((4, 5, 3), f32)
    p[1, 1] = 9.0
    n = np.full((4, 5, 3), 1e-6, f32)
    den = dict(radius=1, strength=16.0, gain=1024.0, alpha=0.0, beta=1.0)
    d = D.denoise(p, n, **den)
    d_hand = np.array([[1, 1, 1, 0, 0]] * 3 + [[0, 0, 0, 0, 0]], f32)
    assert np.array_equal(d, np.repeat(d_hand[..., None], 3, axis=2))
    t = C.chain(p, n, denoise=den, sharpen=dict(taps=np.array([0.5, 0.25], f32), amount=1.0))
    hand = np.array([[1.0, 1.0, 1.25, -0.25, 0.0],
                     [1.0, 1.0, 1.25, -0.25, 0.0],
                     [1.25, 1.25, 1.4375, -0.1875, 0.0],
                     [-0.25, -0.25, -0.1875, -0.0625, 0.0]], f32)
    assert np.array_equal(t, np.repeat(hand[..., None], 3, axis=2))
    assert t[0, 0, 0] == 1.0 and t[0, 0, 0] != 1.4375
