"""numpy float32 restatement of the rendered finish (include/mfsr.h, mfsr_render): matrix, tone, quantise,
and the four output layouts.  Every operation is one float32 + - * with one rounding, as the library computes it
(-ffp-contract=off), so the restatement is bit-exact except through the powf of the built-in gamma."""
from __future__ import annotations

import numpy as np

RGB16, RGB8, RGBA8, RGB10A2 = 0, 1, 2, 3
BYTES_PER_PIXEL = {RGB16: 6, RGB8: 3, RGBA8: 4, RGB10A2: 4}
MAX_OUT = {RGB16: 65535.0, RGB8: 255.0, RGBA8: 255.0, RGB10A2: 1023.0}

f32 = np.float32


def _clamp(v, lo, hi):
    """isnan(v) ? 0 : clamp(v, lo, hi) in float32."""
    v = np.asarray(v, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), f32(0), np.minimum(np.maximum(v, f32(lo)), f32(hi))).astype(f32)


def matrix(p, m):
    """Step 1: q_i = (m[3i] c_0 + m[3i+1] c_1) + m[3i+2] c_2 with c = clamp(p, 0, 65536)."""
    m = np.asarray(m, f32).reshape(9)
    c = _clamp(p, 0.0, 65536.0)
    q = np.empty_like(c)
    for i in range(3):
        q[..., i] = (m[3 * i] * c[..., 0] + m[3 * i + 1] * c[..., 1]) + m[3 * i + 2] * c[..., 2]
    return q


def tone_lut(q, lut):
    """Step 2 with a table of N + 1 floats."""
    lut = np.asarray(lut, f32)
    n = lut.size - 1
    v = _clamp(q, 0.0, 1.0)
    t = (v * f32(n)).astype(f32)
    i = np.minimum(t.astype(np.int32), n - 1)
    f = (t - i.astype(f32)).astype(f32)
    a, b = lut[i], lut[i + 1]
    return (a + ((b - a).astype(f32) * f).astype(f32)).astype(f32)


def gamma(q):
    """Step 2 without a table and with applyGamma: the sRGB curve, numpy's float32 pow."""
    v = _clamp(q, 0.0, 1.0)
    hi = (f32(1.0) + f32(0.055)) * np.power(v, f32(1.0) / f32(2.4), dtype=f32) - f32(0.055)
    return np.where(v <= f32(0.0031308), f32(12.92) * v, hi).astype(f32)


def quantise(o, fmt):
    """Step 3: (int)(clamp(o, 0, 1) * max + 0.5f), NaN -> 0."""
    return (_clamp(o, 0.0, 1.0) * f32(MAX_OUT[fmt]) + f32(0.5)).astype(f32).astype(np.int64)


def render_float(p, m=None, lut=None, apply_gamma=False):
    """Steps 1 and 2: the float image o."""
    q = np.asarray(p, f32) if m is None else matrix(p, m)
    if lut is not None:
        return tone_lut(q, lut)
    return gamma(q) if apply_gamma else q.copy()


def pack(qi, fmt):
    """Integers [h, w, 3] -> the format's array: uint16 [h, w, 3], uint8 [h, w, 3], uint8 [h, w, 4] or uint32 [h, w]."""
    qi = np.asarray(qi, np.int64)
    if fmt == RGB16:
        return qi.astype(np.uint16)
    if fmt == RGB8:
        return qi.astype(np.uint8)
    if fmt == RGBA8:
        return np.concatenate([qi, np.full(qi.shape[:-1] + (1,), 255, np.int64)], axis=-1).astype(np.uint8)
    if fmt == RGB10A2:
        return (qi[..., 0] | qi[..., 1] << 10 | qi[..., 2] << 20 | 3 << 30).astype(np.uint32)
    raise ValueError(fmt)


def render(p, fmt, m=None, lut=None, apply_gamma=False):
    """(float image, packed output) of steps 1-3."""
    o = render_float(p, m, lut, apply_gamma)
    return o, pack(quantise(o, fmt), fmt)


def row_bytes(fmt, width):
    return BYTES_PER_PIXEL[fmt] * width


def as_bytes(packed):
    """The packed output as dense little-endian rows [h, row_bytes] of uint8."""
    a = np.ascontiguousarray(packed)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def srgb_lut(n):
    """The sRGB curve at k/n in float64, rounded to float32 (pipeline.tone_lut_srgb)."""
    v = np.arange(n + 1, dtype=np.float64) / n
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.maximum(v, 1e-300) ** (1.0 / 2.4) - 0.055).astype(f32)
