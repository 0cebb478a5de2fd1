"""numpy restatement of the image statistics, auto white balance and auto tone (include/mfsr.h,
mfsr_imageStats): the 12-bit codes in float32 as ``render_ref.quantise`` computes them, ``render_ref.matrix`` for step 1,
``np.bincount`` for the histograms, and both fits in float64.  The table is exact; of the fits only ``pow`` and ``log`` may
differ from the library's by an ulp."""
from __future__ import annotations

import numpy as np

from tests import render_ref as R

BINS = 4096
WORDS = 8 + 2 * BINS
f32 = np.float32


def codes(p, m=None):
    """c_k = (int)(clamp(q_k, 0, 1) * 4095.0f + 0.5f), NaN -> 0, of q = p after the optional matrix: int64 [..., 3]"""
    q = np.asarray(p, f32) if m is None else R.matrix(p, m)
    return (R._clamp(q, 0.0, 1.0) * f32(4095.0) + f32(0.5)).astype(f32).astype(np.int64)


def stats(p, m=None, lo=64, hi=3967, chroma_tol=0):
    """The table of an image [h, w, 3] (any leading shape): uint64 [WORDS]."""
    c = codes(p, m).reshape(-1, 3)
    c0, c1, c2 = c[:, 0], c[:, 1], c[:, 2]
    y = (54 * c0 + 183 * c1 + 19 * c2 + 128) >> 8
    mx = c.max(axis=1)
    neutral = (lo <= c.min(axis=1)) & (mx <= hi)
    if chroma_tol > 0:
        neutral &= (256 * np.abs(c0 - c1) <= chroma_tol * c1) & (256 * np.abs(c2 - c1) <= chroma_tol * c1)
    t = np.zeros(WORDS, np.uint64)
    t[0] = c.shape[0]
    t[1] = int(neutral.sum())
    t[2:5] = c[neutral].sum(axis=0).astype(np.uint64)
    t[5:8] = c.sum(axis=0).astype(np.uint64)
    t[8:8 + BINS] = np.bincount(y, minlength=BINS).astype(np.uint64)
    t[8 + BINS:] = np.bincount(mx, minlength=BINS).astype(np.uint64)
    return t


def awb_gains(t, min_count):
    """(gains float32 [3], status) of mfsr_awb_gains."""
    n, s = int(t[1]), [int(v) for v in t[2:5]]
    g = np.ones(3, f32)
    if (min_count > 0 and n < min_count) or 0 in s:
        return g, 1
    status = 0
    for k, v in ((0, np.float64(s[1]) / np.float64(s[0])), (2, np.float64(s[1]) / np.float64(s[2]))):
        if v < 0.125 or v > 8.0:
            v, status = min(max(v, 0.125), 8.0), 2
        g[k] = f32(v)
    return g, status


def _rank(hist, target):
    """the smallest k with cum(k) >= target (4095 when the table never gets there)"""
    cum = np.cumsum(hist.astype(object))
    for k in range(BINS):
        if cum[k] >= target:
            return k
    return BINS - 1


def tone_keys(t, p_lo=0.001, p_hi=0.999):
    """(kLo, kHi, kMed)"""
    n = int(t[0])
    t_lo, t_hi = int(np.float64(p_lo) * np.float64(n)), int((np.float64(1.0) - np.float64(p_hi)) * np.float64(n))
    hy, hm = t[8:8 + BINS], t[8 + BINS:]
    return _rank(hy, t_lo + 1), _rank(hm, n - min(t_hi, n)), _rank(hy, (n + 1) // 2)


def srgb(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= 0.0031308, 12.92 * v, 1.055 * np.maximum(v, 1e-300) ** (1.0 / 2.4) - 0.055)


def tone_fit(t, p_lo=0.001, p_hi=0.999, max_gain=8.0, mid=0.18, tone_size=4096):
    """(lut float32 [tone_size + 1], black, white, gamma, status) of mfsr_tone_fit, in float64."""
    k_lo, k_hi, k_med = tone_keys(t, p_lo, p_hi)
    b = np.float64(k_lo) / 4095.0
    span, status = np.float64(k_hi) / 4095.0 - b, 0
    if span < 1.0 / np.float64(max_gain):
        span, status = 1.0 / np.float64(max_gain), 1

    def u(v):
        return np.clip((np.asarray(v, np.float64) - b) / span, 0.0, 1.0)

    um = float(u(np.float64(k_med) / 4095.0))
    g = 1.0
    if mid > 0 and 0.0 < um < 1.0:
        g = float(min(max(np.log(np.float64(mid)) / np.log(np.float64(um)), 0.5), 2.0))
    x = u(np.arange(tone_size + 1, dtype=np.float64) / np.float64(tone_size))
    lut = srgb(x if g == 1.0 else x ** g).astype(f32)
    return lut, float(b), float(b + span), g, status


def auto(measure, pixels, ccm=None, awb=True, tone=True, lo=64, hi=3967, chroma_tol=64, iterations=2, min_count=0,
         p_lo=0.001, p_hi=0.999, max_gain=8.0, mid=0.18, tone_size=4096):
    """The steps of mfsr_burst_auto_render with ``measure(matrix or None, lo, hi, chroma_tol) -> table``.  Returns a dict:
    gains (float32 [3]), matrix (float32 [9] or None), lut (or None), black, white, gamma, awb_status, tone_status, share."""
    min_count = min_count if min_count > 0 else pixels // 64
    out = dict(gains=np.ones(3, f32), lut=None, black=0.0, white=1.0, gamma=1.0, awb_status=0, tone_status=0, share=0.0)
    m = None if ccm is None else np.asarray(ccm, f32).reshape(9)
    if awb:
        g = np.ones(3, f32)
        for it in range(iterations):
            t = measure(np.diag(g).astype(f32).reshape(9) if it else None, lo, hi, chroma_tol if it else 0)
            out["share"] = float(t[1]) / float(t[0])
            c, st = awb_gains(t, min_count)
            if st == 1:
                if it == 0:
                    out["awb_status"] = 1
                continue
            if st == 2 and out["awb_status"] == 0:
                out["awb_status"] = 2
            for k in range(3):
                v = np.float64(g[k]) * np.float64(c[k])
                if v < 0.125 or v > 8.0:
                    v = min(max(v, 0.125), 8.0)
                    out["awb_status"] = out["awb_status"] or 2
                g[k] = f32(v)
        out["gains"] = g
        base = np.eye(3, dtype=np.float64) if m is None else m.astype(np.float64).reshape(3, 3)
        m = (base * g.astype(np.float64)[None, :]).astype(f32).reshape(9)
    out["matrix"] = m
    if tone:
        t = measure(m, lo, hi, 0)
        out["lut"], out["black"], out["white"], out["gamma"], out["tone_status"] = tone_fit(t, p_lo, p_hi, max_gain, mid, tone_size)
    return out
