"""numpy float32 restatement of the sharpened finish (include/mfsr.h, mfsr_sharpen): NaN cleaning, the
separable blur with replicated borders, coring and the unsharp mask, then steps 1-3 of tests/render_ref.py.  Every operation is
one float32 + - * with one rounding, in the order the library computes it (-ffp-contract=off), so the restatement is bit-exact."""
from __future__ import annotations

import numpy as np

from tests import render_ref as R

f32 = np.float32


def gaussian_taps(sigma, radius=0):
    """(radius, taps[radius + 1]) of mfsr_sharpen_gaussian: float64 weights, normalised in float64, rounded to float32."""
    if radius == 0:
        radius = min(4, max(1, int(np.ceil(f32(2.5) * f32(sigma)))))
    s = float(f32(sigma))
    w = np.exp(-(np.arange(radius + 1, dtype=np.float64) ** 2) / (2.0 * s * s))
    total = w[0] + 2.0 * w[1:].sum()
    return radius, (w / total).astype(f32)


def _blur_axis(s, taps, axis):
    """h = k0 * s; h = h + kd * (s(-d) + s(+d)) for d = 1..R, borders replicated along `axis`."""
    k = np.asarray(taps, f32)
    R_ = k.size - 1
    n = s.shape[axis]
    idx = np.arange(n)
    with np.errstate(invalid="ignore", over="ignore"):
        h = (k[0] * s).astype(f32)
        for d in range(1, R_ + 1):
            lo = np.take(s, np.clip(idx - d, 0, n - 1), axis=axis)
            hi = np.take(s, np.clip(idx + d, 0, n - 1), axis=axis)
            h = (h + (k[d] * (lo + hi).astype(f32)).astype(f32)).astype(f32)
    return h


def clean(p):
    """Step 1: s = isnan(p) ? 0 : p."""
    p = np.asarray(p, f32)
    return np.where(np.isnan(p), f32(0), p).astype(f32)


def blur(s, taps):
    """Steps 2 and 3: the horizontal pass, then the vertical pass on its result; s is [h, w, 3] (or [h, w])."""
    return _blur_axis(_blur_axis(s, taps, 1), taps, 0)


def sharpen(p, taps, amount, threshold=0.0):
    """Steps 1-4: the linear float image o that takes the place of p.  taps = k[0..R]."""
    s = clean(p)
    b = blur(s, taps)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (s - b).astype(f32)
        a = (np.abs(e) - f32(threshold)).astype(f32)
        g = np.where(a > 0, np.copysign(a, e), f32(0)).astype(f32)
        return (s + (f32(amount) * g).astype(f32)).astype(f32)


def sharpen_render(p, taps, amount, threshold, fmt, m=None, lut=None, apply_gamma=False):
    """(float image, packed output) of steps 1-5."""
    return R.render(sharpen(p, taps, amount, threshold), fmt, m, lut, apply_gamma)
