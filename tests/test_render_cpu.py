"""Rendered output without a device: the host arithmetic and the host refusals of the render entry points,
the layout of mfsr_render against a compiled probe, and known answers of the numpy restatement (tests/render_ref.py) that
tests/test_render_gpu.py compares the kernels with."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi
from tests import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def test_constants_mirror_the_header():
    text = open(capi.HEADER_PATH).read()
    for name, value in (("RGB16", 0), ("RGB8", 1), ("RGBA8", 2), ("RGB10A2", 3)):
        assert f"#define MFSR_OUT_{name} {value}\n" in text
        assert getattr(capi, "OUT_" + name) == value == getattr(R, name)


@pytest.mark.parametrize("fmt,bpp", [(capi.OUT_RGB16, 6), (capi.OUT_RGB8, 3), (capi.OUT_RGBA8, 4), (capi.OUT_RGB10A2, 4)])
def test_row_bytes(fmt, bpp):
    rb = capi.lib().raw["mfsr_render_row_bytes"]
    for w in (1, 5, 130, 7680):
        assert rb(fmt, w) == bpp * w == R.row_bytes(fmt, w)
    assert rb(fmt, 0) == INVALID and rb(fmt, -3) == INVALID


def test_row_bytes_of_an_unknown_format():
    rb = capi.lib().raw["mfsr_render_row_bytes"]
    assert rb(4, 16) == INVALID and rb(-1, 16) == INVALID


def test_render_struct_mirrors_the_header():
    """capi.Render has the layout of struct mfsr_render: compile a probe with gcc."""
    probe = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mfsr.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(mfsr_render), offsetof(mfsr_render, format),
        offsetof(mfsr_render, useMatrix), offsetof(mfsr_render, matrix), offsetof(mfsr_render, toneLut),
        offsetof(mfsr_render, toneSize), offsetof(mfsr_render, reserved)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = list(map(int, subprocess.check_output([exe], text=True).split()))
    C = capi.Render
    assert got == [ctypes.sizeof(C), C.format.offset, C.useMatrix.offset, C.matrix.offset, C.toneLut.offset, C.toneSize.offset,
                   C.reserved.offset]


# ---- the restatement's known answers ---------------------------------------------------------------------------------------
def test_identity_matrix_leaves_finite_values_in_range_unchanged():
    rng = np.random.default_rng(1)
    p = np.concatenate([rng.uniform(0, 1, 3000), rng.uniform(0, 65536, 2997), [0.0, 65536.0, 1.0]]).astype(np.float32).reshape(-1, 3)
    q = R.matrix(p, np.eye(3))
    assert np.array_equal(q.view(np.uint32), p.view(np.uint32))


@pytest.mark.parametrize("n", [1, 2, 4, 4096, 65536])
def test_linear_lut_reproduces_the_clamp_for_powers_of_two(n):
    """lut[k] = k/N: v*N, the subtraction of i and i/N + f/N are all exact when N is a power of two."""
    rng = np.random.default_rng(n)
    lut = (np.arange(n + 1, dtype=np.float64) / n).astype(np.float32)
    v = np.concatenate([rng.uniform(-0.5, 1.5, 4000), rng.uniform(0, 1e-6, 500), np.arange(n + 1)[:4096] / n,
                        [np.nan, np.inf, -np.inf, 1.0, 0.0]]).astype(np.float32)
    want = np.where(np.isnan(v), np.float32(0), np.clip(v, 0, 1)).astype(np.float32)
    got = R.tone_lut(v, lut)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_rgb10a2_dword_layout():
    o = np.array([[[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.5, 0.25, 1.0]]], np.float32)
    _, d = R.render(o, R.RGB10A2)
    assert d.dtype == np.uint32 and d.shape == (1, 4)
    assert [hex(int(x)) for x in d[0]] == [hex(0xC00003FF), hex(0xC00FFC00), hex(0xFFF00000),
                                           hex(3 << 30 | 1023 << 20 | 256 << 10 | 512)]
    # bytes in memory: little-endian
    assert list(R.as_bytes(d)[0, :4]) == [0xFF, 0x03, 0x00, 0xC0]


def test_layouts_and_quantisation():
    o = np.array([[[0.0, 0.5, 1.0], [2.0, -1.0, 0.2]]], np.float32)
    assert R.render(o, R.RGB16)[1].tolist() == [[[0, 32768, 65535], [65535, 0, 13107]]]
    assert R.render(o, R.RGB8)[1].tolist() == [[[0, 128, 255], [255, 0, 51]]]
    assert R.render(o, R.RGBA8)[1].tolist() == [[[0, 128, 255, 255], [255, 0, 51, 255]]]
    assert R.as_bytes(R.render(o, R.RGB8)[1]).shape == (1, 6) and R.as_bytes(R.render(o, R.RGB16)[1]).shape == (1, 12)


def test_nan_inf_and_negative_inputs():
    bad = np.array([[[np.nan, np.inf, -np.inf], [-3.0, -0.5, np.nan]]], np.float32)
    # matrix: NaN -> 0, +inf -> 65536, -inf and negatives -> 0; nothing infinite or NaN comes out
    q = R.matrix(bad, np.full(9, 256.0))
    assert np.isfinite(q).all() and q[0, 0].tolist() == [256.0 * 65536.0] * 3 and q[0, 1].tolist() == [0.0] * 3
    # tone table: NaN -> lut[0], +inf -> lut[N], -inf and negatives -> lut[0]
    lut = np.array([0.25, 0.5, 0.75], np.float32)
    assert R.tone_lut(bad, lut).tolist() == [[[0.25, 0.75, 0.25], [0.25, 0.25, 0.25]]]
    # no matrix, no table, no gamma: the float passes through, the quantiser clamps and sends NaN to 0
    o, q8 = R.render(bad, R.RGB8)
    assert np.array_equal(o.view(np.uint32), bad.view(np.uint32)) and q8.tolist() == [[[0, 255, 0], [0, 0, 0]]]
    top = (np.float32(1.0) + np.float32(0.055)) * np.float32(1.0) - np.float32(0.055)   # the curve at 1: one ulp under 1
    assert R.gamma(bad).tolist() == [[[0.0, float(top), 0.0], [0.0, 0.0, 0.0]]]


def test_srgb_table_matches_the_pipeline():
    from multi_frame_super_resolution_amd.pipeline import tone_lut_srgb

    for n in (5, 4096):
        assert np.array_equal(tone_lut_srgb(n).numpy().view(np.uint32), R.srgb_lut(n).view(np.uint32))
    assert R.srgb_lut(16)[0] == 0.0 and R.srgb_lut(16)[-1] == 1.0


# ---- host refusals: no device call ------------------------------------------------------------------------------------------
def _render(fmt=capi.OUT_RGB8, matrix=None, lut=0, n=0):
    r = capi.Render()
    r.format = fmt
    if matrix is not None:
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*matrix)
    r.toneLut = lut or None
    r.toneSize = n
    return r


def _call_render_image(r, out=0x1000, row_bytes=64 * 6, w=16, h=4, in_ptr=0x100000, in_rb=None):
    """mfsr_renderImage with pointers that are never dereferenced on the host: every case here is refused before a launch."""
    raw = capi.lib().raw["mfsr_renderImage"]
    return raw(in_ptr, 12 * w if in_rb is None else in_rb, None, 0, out, row_bytes, w, h, ctypes.byref(r), 0, None)


def _call_finish_rendered(r, out=0x1000, row_bytes=64 * 6, w=16, h=4):
    raw = capi.lib().raw["mfsr_finishRendered"]
    return raw(0x100000, 0x200000, 12 * w, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, None, 0, out, row_bytes, ctypes.byref(r), w, h, 1e-3, 0, 0, 0,
               w, h, None)


EYE = [1, 0, 0, 0, 1, 0, 0, 0, 1]


@pytest.mark.parametrize("call", [_call_render_image, _call_finish_rendered], ids=["renderImage", "finishRendered"])
def test_bad_render_descriptions_are_refused_on_the_host(call):
    for bad in (float("nan"), float("inf"), 256.5, -257.0):
        m = list(EYE)
        m[4] = bad
        assert call(_render(matrix=m)) == INVALID, bad
    assert call(_render(lut=0x3000, n=0)) == INVALID
    assert call(_render(lut=0x3000, n=65537)) == INVALID
    assert call(_render(lut=0x3000, n=-4)) == INVALID
    assert call(_render(fmt=4)) == INVALID and call(_render(fmt=-1)) == INVALID
    raw = capi.lib().raw
    assert raw["mfsr_renderImage"](0x100000, 192, None, 0, 0x1000, 384, 16, 4, None, 0, None) == INVALID   # no description


@pytest.mark.parametrize("call", [_call_render_image, _call_finish_rendered], ids=["renderImage", "finishRendered"])
def test_bad_output_rows_are_refused_on_the_host(call):
    for fmt in (capi.OUT_RGBA8, capi.OUT_RGB10A2):
        assert call(_render(fmt=fmt), out=0x1002, row_bytes=64) == INVALID      # misaligned pointer
        assert call(_render(fmt=fmt), out=0x1000, row_bytes=66) == INVALID      # row bytes not a multiple of 4
        assert call(_render(fmt=fmt), out=0x1000, row_bytes=60) == INVALID      # too short: 4 * 16 = 64
    assert call(_render(fmt=capi.OUT_RGB8), out=0x1001, row_bytes=47) == INVALID  # too short: 3 * 16 = 48
    assert call(_render(fmt=capi.OUT_RGB16), out=0x1001, row_bytes=96) == INVALID
    assert call(_render(fmt=capi.OUT_RGB16), out=0x1000, row_bytes=94) == INVALID
    assert call(_render(), w=0) == INVALID and call(_render(), h=0) == INVALID


def test_render_image_checks_its_float_rows():
    assert _call_render_image(_render(), in_rb=12 * 16 - 4) == INVALID
    assert _call_render_image(_render(), in_rb=12 * 16 + 2) == INVALID
    raw = capi.lib().raw["mfsr_renderImage"]
    r = _render()
    assert raw(0x100000, 192, None, 0, None, 0, 16, 4, ctypes.byref(r), 0, None) == INVALID   # neither output
    assert raw(None, 192, None, 0, 0x1000, 48, 16, 4, ctypes.byref(r), 0, None) == INVALID


def test_burst_and_stream_setters_check_their_handle():
    raw = capi.lib().raw
    r = _render()
    assert raw["mfsr_burst_set_render"](None, ctypes.byref(r)) == INVALID
    assert raw["mfsr_stream_set_render"](None, ctypes.byref(r)) == INVALID
