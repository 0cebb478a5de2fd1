"""numpy float32 restatement of the two-plane YUV 4:2:0 output (include/mfsr.h, MFSR_OUT_NV12 /
MFSR_OUT_P010): Y'CbCr from the rendered pixel, the 2 x 2 chroma mean, the codes and the layout.  Matrix and tone are
tests/render_ref.py's.  Every operation is one float32 + - * with one rounding, in the header's order, so the restatement is
bit-exact."""
from __future__ import annotations

import numpy as np

from tests import render_ref as R

NV12, P010 = 16, 17
BT709, BT601, BT2020, FULL = 0, 1, 2, 4
BITS = {NV12: 8, P010: 10}
KR_KB = {BT709: (0.2126, 0.0722), BT601: (0.299, 0.114), BT2020: (0.2627, 0.0593)}
COLOURS = (BT709, BT601, BT2020, BT709 | FULL, BT601 | FULL, BT2020 | FULL)

f32 = np.float32


def constants(colour):
    """(Kr, Kg, Kb, Sb, Sr): the float32 roundings of doubles."""
    kr, kb = KR_KB[colour & 3]
    return f32(kr), f32(1.0 - kr - kb), f32(kb), f32(0.5 / (1.0 - kb)), f32(0.5 / (1.0 - kr))


def ycbcr(o, colour=0):
    """Steps 1 and 2: (Y, Cb, Cr) float32 arrays of the pixel array o [..., 3]."""
    kr, kg, kb, sb, sr = constants(colour)
    c = R._clamp(o, 0.0, 1.0)
    c0, c1, c2 = c[..., 0], c[..., 1], c[..., 2]
    y = ((kr * c0 + kg * c1) + kb * c2).astype(f32)
    return y, ((c2 - y) * sb).astype(f32), ((c0 - y) * sr).astype(f32)


def mean2x2(c):
    """Step 3: ((C(x, y) + C(x+1, y)) + (C(x, y+1) + C(x+1, y+1))) * 0.25, x first and rows second."""
    c = np.asarray(c, f32)
    top = (c[0::2, 0::2] + c[0::2, 1::2]).astype(f32)
    bottom = (c[1::2, 0::2] + c[1::2, 1::2]).astype(f32)
    return ((top + bottom).astype(f32) * f32(0.25)).astype(f32)


def _code(v, m):
    return (np.minimum(np.maximum(np.asarray(v, f32), f32(0)), f32(m)) + f32(0.5)).astype(f32).astype(np.int64)


def codes(y, cb, cr, fmt, colour=0):
    """Step 4: integer codes (Y [h, w], UV [h/2, w/2, 2]) of luma and of the MEANED chroma."""
    n = BITS[fmt]
    m, M = f32(2 ** (n - 8)), f32(2 ** n - 1)
    if colour & FULL:
        y_off, y_scale, c_off, c_scale = f32(0), M, f32(2 ** (n - 1)), M
    else:
        y_off, y_scale, c_off, c_scale = f32(16) * m, f32(219) * m, f32(128) * m, f32(224) * m
    yq = _code(y_off + (y_scale * y).astype(f32), M)
    uv = np.stack([_code(c_off + (c_scale * cb).astype(f32), M), _code(c_off + (c_scale * cr).astype(f32), M)], axis=-1)
    return yq, uv


def planes(o, fmt, colour=0):
    """The float image o [h, w, 3] (after matrix and tone) -> (Y [h, w], UV [h/2, w/2, 2]) in the stored type: uint8, or
    uint16 words holding code << 6."""
    h, w = o.shape[:2]
    assert h % 2 == 0 and w % 2 == 0 and h > 0 and w > 0
    y, cb, cr = ycbcr(o, colour)
    yq, uv = codes(y, mean2x2(cb), mean2x2(cr), fmt, colour)
    if fmt == NV12:
        return yq.astype(np.uint8), uv.astype(np.uint8)
    return (yq << 6).astype("<u2"), (uv << 6).astype("<u2")


def render(p, fmt, m=None, lut=None, apply_gamma=False, colour=0):
    """(float image, Y plane, UV plane) of the input p [h, w, 3]."""
    o = R.render_float(p, m, lut, apply_gamma)
    return (o,) + planes(o, fmt, colour)


def row_bytes(fmt, width):
    return width * (1 if fmt == NV12 else 2)


def image_bytes(fmt, w, h):
    return row_bytes(fmt, w) * h * 3 // 2


def as_bytes(y, uv):
    """The two planes as one dense little-endian buffer [3h/2, row_bytes] of uint8: Y rows, then chroma rows."""
    h = y.shape[0]
    yb = np.ascontiguousarray(y).view(np.uint8).reshape(h, -1)
    ub = np.ascontiguousarray(uv).view(np.uint8).reshape(h // 2, -1)
    return np.concatenate([yb, ub], axis=0)


def split(buf, fmt, h, w):
    """A dense flat buffer (uint8, or 16-bit words for P010) -> (Y [h, w], UV [h/2, w/2, 2]) views."""
    flat = np.asarray(buf).reshape(-1)
    return flat[:h * w].reshape(h, w), flat[h * w:h * w * 3 // 2].reshape(h // 2, w // 2, 2)
