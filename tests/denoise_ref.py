"""numpy float32 restatement of the merge-aware denoise inside the finish (include/mfsr.h, mfsr_denoise):
the cleaning, the effective count, the fade, the tolerance, the range filter with replicated borders and row-wise sums, then
steps 1-3 of tests/render_ref.py.  Every operation is one float32 + - * / with one rounding, np.fmax / np.fmin where the library
calls fmaxf / fminf, in the order the library computes it (-ffp-contract=off); the range kernel is a polynomial, so the
restatement is bit-exact."""
from __future__ import annotations

import numpy as np

from tests import render_ref as R

f32 = np.float32


def clean(p):
    """Step 1: s = isnan(p) ? 0 : fminf(fmaxf(p, -65536), 65536)."""
    p = np.asarray(p, f32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(p), f32(0), np.fmin(np.fmax(p, f32(-65536.0)), f32(65536.0))).astype(f32)


def count_of_weight(w, threshold):
    """Step 2 without its cleaning: n = (w < threshold) ? w + 1 : w, the count apply_weight_f divides by."""
    w = np.asarray(w, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(w < f32(threshold), (w + f32(1)).astype(f32), w).astype(f32)


def fade(n, w_lo=0.0, w_hi=0.0):
    """Step 3 on the cleaned count."""
    if not f32(w_hi) > f32(w_lo):
        return np.ones_like(n, dtype=f32)
    r_span = f32(1.0) / f32(f32(w_hi) - f32(w_lo))
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((f32(w_hi) - n).astype(f32) * r_span).astype(f32)
        return np.fmin(np.fmax(x, f32(0)), f32(1)).astype(f32)


def filter_sums(s, r, radius):
    """Step 5: (G [h, w], S [h, w, 3]) of the cleaned image s and the reciprocal tolerances r."""
    h, w = s.shape[:2]
    ys, xs = np.arange(h), np.arange(w)
    G = np.zeros((h, w), f32)
    S = np.zeros((h, w, 3), f32)
    with np.errstate(over="raise", invalid="raise"):
        for dy in range(-radius, radius + 1):
            Gr = np.zeros((h, w), f32)
            Sr = np.zeros((h, w, 3), f32)
            rows = s[np.clip(ys + dy, 0, h - 1)]
            for dx in range(-radius, radius + 1):
                j = rows[:, np.clip(xs + dx, 0, w - 1)]
                d = (j - s).astype(f32)
                dd = (d * d).astype(f32)
                q = (dd * r).astype(f32)
                t = ((q[..., 0] + q[..., 1]).astype(f32) + q[..., 2]).astype(f32)
                u = np.fmax((f32(1) - t).astype(f32), f32(0)).astype(f32)
                g = (u * u).astype(f32)
                Gr = (Gr + g).astype(f32)
                Sr = (Sr + (g[..., None] * j).astype(f32)).astype(f32)
            G = (G + Gr).astype(f32)
            S = (S + Sr).astype(f32)
    return G, S


def denoise(p, n=None, radius=2, strength=3.0, gain=2.0, alpha=0.0, beta=0.0, w_lo=0.0, w_hi=0.0, want_sums=False):
    """Steps 1 and 3-6: the linear float image o that takes the place of p.  n: the count image [h, w, 3] (before its NaN
    cleaning), or None for n = 1 everywhere."""
    s = clean(p)
    n = np.ones_like(s) if n is None else np.asarray(n, f32)
    n = np.where(np.isnan(n), f32(0), n).astype(f32)
    lam = fade(n, w_lo, w_hi)
    hh = f32(f32(strength) * f32(strength))
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        num = (f32(gain) * ((f32(alpha) * np.fmax(s, f32(0))).astype(f32) + f32(beta)).astype(f32)).astype(f32)
        with np.errstate(over="ignore"):
            v = np.fmax((num / np.fmax(n, f32(1e-6))).astype(f32), f32(1e-20)).astype(f32)
        r = (f32(1) / (hh * v).astype(f32)).astype(f32)
    G, S = filter_sums(s, r, radius)
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        f = (S / G[..., None]).astype(f32)
        o = np.where(lam == 0, s, (s + (lam * (f - s).astype(f32)).astype(f32)).astype(f32)).astype(f32)
    return (o, G, S) if want_sums else o


def finish_denoise(p, w, threshold, **kw):
    """Steps 1-6 of the denoised finish: p is the plain finish's linear float image, w its accumulated weights."""
    return denoise(p, count_of_weight(w, threshold), **kw)


def denoise_render(p, n, fmt, m=None, lut=None, apply_gamma=False, **kw):
    """(float image, packed output) of steps 1 and 3-7."""
    return R.render(denoise(p, n, **kw), fmt, m, lut, apply_gamma)
