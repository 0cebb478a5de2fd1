"""Two-plane YUV 4:2:0 output without a device: the constants, the host arithmetic and the host
refusals of the entry points, and known answers of the numpy restatement (tests/yuv_ref.py) that tests/test_yuv_gpu.py compares
the kernels with: the published colour-bar codes, an anchor independent of this code."""
import ctypes

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi
from tests import yuv_ref as Y

INVALID = -1
f32 = np.float32


def test_constants_mirror_the_header():
    text = open(capi.HEADER_PATH).read()
    for name, value in (("OUT_NV12", 16), ("OUT_P010", 17), ("YUV_BT709", 0), ("YUV_BT601", 1), ("YUV_BT2020", 2), ("YUV_FULL", 4)):
        assert f"#define MFSR_{name} {value}" in text, name
        assert getattr(capi, name) == value
    assert (Y.NV12, Y.P010, Y.BT709, Y.BT601, Y.BT2020, Y.FULL) == (16, 17, 0, 1, 2, 4)
    assert "CENTRE" in text           # the header says where the chroma sample is sited


def test_entry_points_resolve():
    raw = capi.lib().raw
    for name in ("mfsr_render_image_bytes", "mfsr_renderImageYuv", "mfsr_finishRenderedYuv"):
        assert name in raw, name
    assert raw["mfsr_render_image_bytes"].restype is ctypes.c_longlong


@pytest.mark.parametrize("colour,bits", [
    (Y.BT709, "3e59b3d0 3f371759 3d93dd98 3f09f5f5 3f228f71"),
    (Y.BT601, "3e991687 3f1645a2 3de978d5 3f107833 3f3698a7"),
    (Y.BT2020, "3e86809d 3f2d9168 3d72e48f 3f0811a2 3f2d9b3d")], ids=["709", "601", "2020"])
def test_the_five_constants_have_the_stated_bit_patterns(colour, bits):
    for c in (colour, colour | Y.FULL):
        got = " ".join(f"{int(np.asarray(v, f32).view(np.uint32)):08x}" for v in Y.constants(c))
        assert got == bits


def test_row_bytes_and_image_bytes():
    rb, ib = capi.lib().raw["mfsr_render_row_bytes"], capi.lib().raw["mfsr_render_image_bytes"]
    for w in (2, 6, 130, 7680):
        assert rb(capi.OUT_NV12, w) == w == Y.row_bytes(Y.NV12, w)
        assert rb(capi.OUT_P010, w) == 2 * w == Y.row_bytes(Y.P010, w)
        for h in (2, 18, 4320):
            assert ib(capi.OUT_NV12, w, h) == w * h * 3 // 2 == Y.image_bytes(Y.NV12, w, h)
            assert ib(capi.OUT_P010, w, h) == 3 * w * h == Y.image_bytes(Y.P010, w, h)
    for fmt in (capi.OUT_NV12, capi.OUT_P010):
        for w in (0, -2, 1, 7, 131):
            assert rb(fmt, w) == INVALID and ib(fmt, w, 4) < 0, (fmt, w)
        for h in (0, -2, 1, 7):
            assert ib(fmt, 8, h) < 0, (fmt, h)
    # the single-plane formats: rowBytes * h, any positive extent
    for fmt, bpp in ((capi.OUT_RGB16, 6), (capi.OUT_RGB8, 3), (capi.OUT_RGBA8, 4), (capi.OUT_RGB10A2, 4)):
        assert ib(fmt, 5, 3) == bpp * 15 and ib(fmt, 7680, 4320) == bpp * 7680 * 4320
        assert ib(fmt, 0, 3) < 0 and ib(fmt, 5, 0) < 0
    assert ib(capi.OUT_RGB16, 65536, 65536) == 6 * 65536 * 65536      # (a long long)


def test_format_4_is_still_refused_everywhere():
    raw = capi.lib().raw
    for fmt in (4, 5, 15, 18, -1):
        assert raw["mfsr_render_row_bytes"](fmt, 16) == INVALID and raw["mfsr_render_image_bytes"](fmt, 16, 16) < 0
        r = _render(fmt)
        assert _render_image(r) == INVALID and _finish_rendered(r) == INVALID
        assert _render_image_yuv(r) == INVALID and _finish_rendered_yuv(r) == INVALID


# ---- host refusals: pointers that are never dereferenced ------------------------------------------------------------------
def _render(fmt=capi.OUT_NV12, colour=0, r1=0, r2=0):
    r = capi.Render()
    r.format = fmt
    r.reserved[0], r.reserved[1], r.reserved[2] = colour, r1, r2
    return r


def _render_image(r, out=0x1000, row_bytes=64 * 6, w=16, h=4):
    return capi.lib().raw["mfsr_renderImage"](0x100000, 12 * w, None, 0, out, row_bytes, w, h, ctypes.byref(r), 0, None)


def _finish_rendered(r, out=0x1000, row_bytes=64 * 6, w=16, h=4):
    return capi.lib().raw["mfsr_finishRendered"](0x100000, 0x200000, 12 * w, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, None, 0, out, row_bytes,
                                                  ctypes.byref(r), w, h, 1e-3, 0, 0, 0, w, h, None)


def _render_image_yuv(r, y=0x1000, y_rb=64, uv=0x8000, uv_rb=64, w=16, h=4, img=None):
    return capi.lib().raw["mfsr_renderImageYuv"](0x100000, 12 * w, img, 12 * w, y, y_rb, uv, uv_rb, w, h, ctypes.byref(r), 0, None)


def _finish_rendered_yuv(r, y=0x1000, y_rb=64, uv=0x8000, uv_rb=64, w=16, h=4, img=None):
    return capi.lib().raw["mfsr_finishRenderedYuv"](0x100000, 0x200000, 12 * w, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, img, 12 * w, y, y_rb,
                                                     uv, uv_rb, ctypes.byref(r), w, h, 1e-3, 0, 0, 0, w, h, None)


CALLS = pytest.mark.parametrize("call", [_render_image_yuv, _finish_rendered_yuv], ids=["renderImageYuv", "finishRenderedYuv"])


@CALLS
def test_odd_extents_and_missing_planes_are_refused(call):
    for fmt in (capi.OUT_NV12, capi.OUT_P010):
        r = _render(fmt)
        for w, h in ((15, 4), (16, 3), (0, 4), (16, 0), (-2, 4)):
            assert call(r, w=w, h=h) == INVALID, (fmt, w, h)
        assert call(r, y=None) == INVALID and call(r, uv=None) == INVALID       # one plane
        assert call(r, y=None, uv=None) == INVALID                              # neither, and no float image
        assert call(r, y=None, img=0x300000) == INVALID and call(r, uv=None, img=0x300000) == INVALID


@CALLS
def test_short_pitches_and_misaligned_p010_planes_are_refused(call):
    nv, p10 = _render(capi.OUT_NV12), _render(capi.OUT_P010)
    assert call(nv, y_rb=15) == INVALID and call(nv, uv_rb=15) == INVALID
    assert call(p10, y_rb=30) == INVALID and call(p10, uv_rb=30) == INVALID
    assert call(p10, y=0x1001) == INVALID and call(p10, uv=0x8001) == INVALID
    assert call(p10, y_rb=65) == INVALID and call(p10, uv_rb=67) == INVALID


@CALLS
def test_bad_colour_descriptions_are_refused(call):
    for fmt in (capi.OUT_NV12, capi.OUT_P010):
        for colour in (3, 7, 8, 16, 1 << 20, -1):
            assert call(_render(fmt, colour)) == INVALID, colour
        assert call(_render(fmt, 0, r1=1)) == INVALID and call(_render(fmt, Y.BT601 | Y.FULL, r2=-5)) == INVALID


@CALLS
def test_the_yuv_entries_refuse_the_single_plane_formats(call):
    for fmt in (capi.OUT_RGB16, capi.OUT_RGB8, capi.OUT_RGBA8, capi.OUT_RGB10A2):
        assert call(_render(fmt), y_rb=128, uv_rb=128) == INVALID, fmt
    raw = capi.lib().raw["mfsr_renderImageYuv"]
    assert raw(0x100000, 192, None, 0, 0x1000, 64, 0x8000, 64, 16, 4, None, 0, None) == INVALID       # no description


def test_the_single_plane_entries_refuse_the_yuv_formats():
    for fmt in (capi.OUT_NV12, capi.OUT_P010):
        r = _render(fmt)
        assert _render_image(r) == INVALID and _finish_rendered(r) == INVALID
        # ... also when only the float image is asked for
        raw = capi.lib().raw
        assert raw["mfsr_renderImage"](0x100000, 192, 0x300000, 192, None, 0, 16, 4, ctypes.byref(r), 0, None) == INVALID
        assert raw["mfsr_finishRendered"](0x100000, 0x200000, 192, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, 0x300000, 192, None, 0,
                                          ctypes.byref(r), 16, 4, 1e-3, 0, 0, 0, 16, 4, None) == INVALID


def test_sharpening_refuses_the_yuv_formats():
    from multi_frame_super_resolution_amd.pipeline import sharpen_gaussian
    raw = capi.lib().raw
    s = sharpen_gaussian(1.0, 2, 1.0, 0.0)
    buf = (ctypes.c_float * (3 * 8 * 8 * 3))()
    a = ctypes.addressof(buf)
    for fmt in (capi.OUT_NV12, capi.OUT_P010):
        r = _render(fmt)
        assert raw["mfsr_sharpenImage"](a, 96, a + 768, 96, a + 1536, 96, 8, 8, ctypes.byref(s), ctypes.byref(r), 0, None) == INVALID
        assert raw["mfsr_sharpenImage"](a, 96, a + 768, 96, None, 0, 8, 8, ctypes.byref(s), ctypes.byref(r), 0, None) == INVALID
        assert raw["mfsr_finishSharpened"](a, a, 96, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, a + 768, 96, None, 0, ctypes.byref(r), 8, 8,
                                           1e-3, 0, 0, 0, 8, 8, ctypes.byref(s), 0, 0, None) == INVALID
    assert raw["mfsr_burst_set_sharpen"](None, ctypes.byref(s)) == INVALID
    assert raw["mfsr_burst_set_render"](None, ctypes.byref(_render())) == INVALID


def test_python_helpers_without_a_device():
    import torch
    from multi_frame_super_resolution_amd import pipeline as P
    assert P.render_image_bytes(capi.OUT_NV12, 8, 4) == 48 and P.render_image_bytes(capi.OUT_P010, 8, 4) == 96
    assert P.render_image_bytes(capi.OUT_RGB8, 5, 3) == 45
    with pytest.raises(ValueError):
        P.render_image_bytes(capi.OUT_NV12, 7, 4)
    with pytest.raises(ValueError):
        P.render_image_bytes(4, 8, 4)
    buf = P._render_buffer(capi.OUT_NV12, 4, 8, "cpu")
    assert buf.dtype == torch.uint8 and tuple(buf.shape) == (48,)
    b16 = P._render_buffer(capi.OUT_P010, 4, 8, "cpu")
    assert b16.dtype == torch.int16 and tuple(b16.shape) == (48,)
    with pytest.raises(ValueError):
        P._render_buffer(capi.OUT_NV12, 3, 8, "cpu")
    buf.copy_(torch.arange(48, dtype=torch.uint8))
    y, uv = P.yuv_planes(buf, capi.OUT_NV12, 4, 8)
    assert tuple(y.shape) == (4, 8) and tuple(uv.shape) == (2, 4, 2)
    assert y.data_ptr() == buf.data_ptr() and uv.data_ptr() == buf.data_ptr() + 32       # views, not copies
    assert int(y[1, 2]) == 10 and uv[1, 0].tolist() == [40, 41]
    with pytest.raises(ValueError):
        P.yuv_planes(buf, capi.OUT_RGB8, 4, 8)
    with pytest.raises(ValueError):
        P.yuv_planes(buf[:47], capi.OUT_NV12, 4, 8)
    r, _ = P._render_struct(capi.OUT_P010, None, None, "cpu", yuv=capi.YUV_BT2020 | capi.YUV_FULL)
    assert r.format == 17 and list(r.reserved) == [6, 0, 0]
    assert list(P._render_struct(capi.OUT_NV12, None, None, "cpu")[0].reserved) == [0, 0, 0]
    with pytest.raises(ValueError):
        P._render_struct(capi.OUT_RGB8, None, None, "cpu", yuv=capi.YUV_BT601)
    # a zoom window with a two-plane format: whole 2 x 2 blocks only
    cfg = P.default_config(64, 48, 3, scale=2)
    P._Window(cfg, (18, 2, 40, 30)).check_yuv(capi.OUT_NV12)
    P._Window(cfg, (17, 3, 41, 31)).check_yuv(capi.OUT_RGB8)
    P._Window(cfg, None).check_yuv(capi.OUT_NV12)
    for bad in ((17, 2, 40, 30), (18, 3, 40, 30), (18, 2, 41, 30), (18, 2, 40, 31)):
        with pytest.raises(ValueError):
            P._Window(cfg, bad).check_yuv(capi.OUT_P010)
    # the crop of both planes of the aligned window's buffer
    win = P._Window(cfg, (18, 2, 40, 30))
    ax, ay, aw, ah = win.aligned
    full = torch.arange(aw * ah * 3 // 2, dtype=torch.int16)
    got = win.output(full, capi.OUT_P010)
    fy, fuv = P.yuv_planes(full, capi.OUT_P010, ah, aw)
    gy, guv = P.yuv_planes(got, capi.OUT_P010, 30, 40)
    assert torch.equal(gy, fy[2 - ay:32 - ay, 18 - ax:58 - ax])
    assert torch.equal(guv, fuv[(2 - ay) // 2:(32 - ay) // 2, (18 - ax) // 2:(58 - ax) // 2])


# ---- the restatement's known answers: the published colour-bar codes ----------------------------------------------------------
def _bar(rgb, fmt, colour):
    o = np.empty((2, 2, 3), f32)
    o[...] = np.asarray(rgb, f32)
    y, uv = Y.planes(o, fmt, colour)
    shift = 0 if fmt == Y.NV12 else 6
    assert (y == y[0, 0]).all() and y.shape == (2, 2) and uv.shape == (1, 1, 2)
    return int(y[0, 0]) >> shift, int(uv[0, 0, 0]) >> shift, int(uv[0, 0, 1]) >> shift


BARS = dict(white=(1, 1, 1), black=(0, 0, 0), red=(1, 0, 0), green=(0, 1, 0), blue=(0, 0, 1), yellow=(1, 1, 0), cyan=(0, 1, 1),
            magenta=(1, 0, 1))


@pytest.mark.parametrize("fmt,colour,want", [
    (Y.NV12, Y.BT709, dict(white=(235, 128, 128), black=(16, 128, 128), red=(63, 102, 240), green=(173, 42, 26), blue=(32, 240, 118),
                           yellow=(219, 16, 138), cyan=(188, 154, 16), magenta=(78, 214, 230))),
    (Y.NV12, Y.BT601, dict(red=(81, 90, 240), green=(145, 54, 34), blue=(41, 240, 110))),
    (Y.P010, Y.BT709, dict(red=(250, 409, 960), green=(691, 167, 105), blue=(127, 960, 471), white=(940, 512, 512))),
    (Y.NV12, Y.BT709 | Y.FULL, dict(red=(54, 99, 255), blue=(18, 255, 116)))],
    ids=["709-limited-8", "601-limited-8", "709-limited-10", "709-full-8"])
def test_colour_bars(fmt, colour, want):
    for name, codes in want.items():
        assert _bar(BARS[name], fmt, colour) == codes, name


def test_mid_grey_full_range():
    assert _bar((0.5, 0.5, 0.5), Y.NV12, Y.BT709 | Y.FULL) == (128, 128, 128)


@pytest.mark.parametrize("colour", Y.COLOURS)
def test_a_grey_ramp_has_neutral_chroma(colour):
    g = (np.arange(100000, dtype=np.float64) / 99999.0).astype(f32)
    o = np.repeat(np.repeat(np.stack([g, g, g], axis=-1)[None, :, None, :], 2, axis=0), 2, axis=2).reshape(2, 200000, 3)
    y, _, _ = Y.ycbcr(o[0, ::2], colour)
    worst = float(np.abs(y.astype(np.float64) - g.astype(np.float64)).max())
    print(f"colour {colour}: worst |Y - grey| = {worst:.3g}")
    assert worst <= 1.2e-7
    for fmt, neutral in ((Y.NV12, 128), (Y.P010, 512)):
        _, uv = Y.planes(o, fmt, colour)
        assert (uv == (neutral << (0 if fmt == Y.NV12 else 6))).all(), (fmt, colour)


def test_the_mean_adds_x_first_and_rows_second():
    """a block whose four values make the two orders differ in the last bit"""
    c = np.array([1040990127, 3194731784, 3203073413, 3203893681], np.uint32).view(f32).reshape(2, 2)
    rows_of_x = ((c[0, 0] + c[0, 1]) + (c[1, 0] + c[1, 1])) * f32(0.25)
    columns_first = ((c[0, 0] + c[1, 0]) + (c[0, 1] + c[1, 1])) * f32(0.25)
    assert rows_of_x.view(np.uint32) == 3196359545 and columns_first.view(np.uint32) == 3196359544
    got = Y.mean2x2(c)
    assert got.shape == (1, 1) and got[0, 0].view(np.uint32) == rows_of_x.view(np.uint32)
    # and through the codes: 4 x 4 pixels, block (1, 1) differs from a plain mean of four
    big = np.zeros((4, 4), f32)
    big[2:, 2:] = c
    m = Y.mean2x2(big)
    assert m.shape == (2, 2) and m[1, 1].view(np.uint32) == 3196359545 and m[0, 0] == 0


def test_p010_words_are_the_code_shifted_by_six_little_endian():
    o = np.empty((2, 2, 3), f32)
    o[...] = np.array([1.0, 0.0, 0.0], f32)               # red: (250, 409, 960)
    y, uv = Y.planes(o, Y.P010, Y.BT709)
    assert y.dtype.itemsize == 2 and int(y[0, 0]) == 250 << 6 and uv[0, 0].tolist() == [409 << 6, 960 << 6]
    b = Y.as_bytes(y, uv)
    assert b.shape == (3, 4) and b.dtype == np.uint8
    assert b[0].tolist() == [(250 << 6) & 255, (250 << 6) >> 8] * 2
    assert b[2].tolist() == [(409 << 6) & 255, (409 << 6) >> 8, (960 << 6) & 255, (960 << 6) >> 8]
    assert (y & 63 == 0).all() and (uv & 63 == 0).all()
    y8, uv8 = Y.planes(o, Y.NV12, Y.BT709)
    assert y8.dtype == np.uint8 and Y.as_bytes(y8, uv8).shape == (3, 2)


def test_nan_inf_and_out_of_range_pixels():
    o = np.array([[[np.nan, np.inf, -np.inf], [-3.0, 2.5, 0.5]], [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]], f32)
    y, cb, cr = Y.ycbcr(o)
    assert np.isfinite(y).all() and np.isfinite(cb).all() and np.isfinite(cr).all()
    kr, kg, kb, _, _ = Y.constants(0)
    assert y[0, 0] == kg and y[0, 1] == (f32(0) + kg) + kb * f32(0.5)        # NaN -> 0, inf -> 1, -inf -> 0
    yq, uv = Y.planes(o, Y.NV12)
    assert yq[1].tolist() == [16, 235]
