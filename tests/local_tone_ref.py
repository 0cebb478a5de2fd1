"""numpy restatement of local tone mapping in the finish (include/mfsr.h, mfsr_local_tone): the statistics
of the bilateral grid from the 12-bit codes of ``image_stats_ref``, the fit in float64, and the slice in float32 with one rounding
per operation, as the library computes it (-ffp-contract=off).  The table and the slice are exact; of the fit only ``pow``,
``log`` and ``exp`` may differ from the library's by the last double bit."""
from __future__ import annotations

import math

import numpy as np

from tests import image_stats_ref as S
from tests import render_ref as R

f32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def grid_size(full_w, full_h, cell, bins):
    return cdiv(full_w, cell), cdiv(full_h, cell), bins


def default_cell(w, h):
    cell = 16
    while cdiv(max(w, h), cell) > 128:
        cell *= 2
    return cell


# ---- 1. the statistics ------------------------------------------------------------------------------------------------------
def stats(p, cell, bins, m=None, offset=(0, 0), full=None):
    """The table of an image [h, w, 3] whose first pixel is ``offset`` = (x, y) of the ``full`` = (w, h) frame: uint64
    [GY, GX, NZ, 2], (count, sum of the key) per entry."""
    h, w = p.shape[:2]
    fw, fh = (w, h) if full is None else full
    gx, gy, nz = grid_size(fw, fh, cell, bins)
    c = S.codes(p, m)
    key = (54 * c[..., 0] + 183 * c[..., 1] + 19 * c[..., 2] + 128) >> 8
    X = np.arange(w)[None, :] + offset[0]
    Y = np.arange(h)[:, None] + offset[1]
    entry = ((Y // cell) * gx + (X // cell)) * nz + ((key * nz) >> 12)
    t = np.zeros((gy * gx * nz, 2), np.uint64)
    t[:, 0] = np.bincount(entry.reshape(-1), minlength=gy * gx * nz).astype(np.uint64)
    t[:, 1] = np.bincount(entry.reshape(-1), weights=key.reshape(-1).astype(np.float64), minlength=gy * gx * nz).astype(np.uint64)
    return t.reshape(gy, gx, nz, 2)


# ---- 2. the fit ---------------------------------------------------------------------------------------------------------------
def _blur(v, axis):
    """[1 2 1] / 4 with replicated borders: ((lo + 2 c) + hi) * 0.25"""
    n = v.shape[axis]
    idx = np.arange(n)
    lo = np.take(v, np.maximum(idx - 1, 0), axis=axis)
    hi = np.take(v, np.minimum(idx + 1, n - 1), axis=axis)
    return ((lo + 2.0 * v) + hi) * 0.25


def fit(t, smooth=1, shadows=0.5, highlights=0.25, pivot=0.0, max_gain=4.0):
    """(grid float32 [GY, GX, NZ], pivot, status) of mfsr_local_tone_fit.  The float arguments are the floats of the description
    widened to double, as the library reads them."""
    t = np.asarray(t, np.uint64)
    gy, gx, nz = t.shape[:3]
    N, Sm = t[..., 0].astype(np.float64), t[..., 1].astype(np.float64)
    shadows, highlights, pivot, max_gain = (float(f32(v)) for v in (shadows, highlights, pivot, max_gain))
    status = 0
    if not pivot > 0.0:
        sum_n = sum_l = 0.0
        for n, s in zip(N.reshape(-1), Sm.reshape(-1)):        # the table's order, one addition at a time
            if n > 0:
                mean = s / (4095.0 * n)
                sum_n += n
                sum_l += n * math.log(max(mean, 1.0 / 4095.0))
        if sum_n > 0.0:
            pivot = math.exp(sum_l / sum_n)
        else:
            pivot, status = 0.18, 1
    for _ in range(smooth):
        N = _blur(_blur(_blur(N, 1), 0), 2)
        Sm = _blur(_blur(_blur(Sm, 1), 0), 2)
    centre = ((np.arange(nz, dtype=np.float64) + 0.5) / nz)[None, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        B = np.where(N > 0, Sm / (4095.0 * N), centre)
    B = np.maximum(B, 1.0 / 4095.0)
    r = B / pivot
    g = np.where(r < 1.0, np.power(r, -shadows), np.power(r, -highlights))
    g = np.minimum(np.maximum(g, 1.0 / max_gain), max_gain)
    return g.astype(f32), pivot, status


# ---- 3. the slice ----------------------------------------------------------------------------------------------------------------
def _axis(X, cell, n):
    fx = ((X.astype(f32) + f32(0.5)) * f32(1.0 / cell)).astype(f32) - f32(0.5)
    fx = np.minimum(np.maximum(fx, f32(0)), f32(n - 1)).astype(f32)
    i0 = fx.astype(np.int32)
    return i0, np.minimum(i0 + 1, n - 1), (fx - i0.astype(f32)).astype(f32)


def _lerp(a, b, t):
    return (a + ((b - a).astype(f32) * t).astype(f32)).astype(f32)


def gain(p, grid, cell, m=None, offset=(0, 0)):
    """The gain of every pixel of p [h, w, 3]: float32 [h, w]."""
    grid = np.asarray(grid, f32)
    gy, gx, nz = grid.shape
    h, w = p.shape[:2]
    q = np.asarray(p, f32) if m is None else R.matrix(p, m)
    v = R._clamp(q, 0.0, 1.0)
    lum = (((f32(54) * v[..., 0] + f32(183) * v[..., 1]).astype(f32) + f32(19) * v[..., 2]).astype(f32) * f32(1.0 / 256.0)).astype(f32)
    i0, i1, ax = _axis(np.arange(w)[None, :] + offset[0], cell, gx)
    j0, j1, ay = _axis(np.arange(h)[:, None] + offset[1], cell, gy)
    fz = (lum * f32(nz)).astype(f32) - f32(0.5)
    fz = np.minimum(np.maximum(fz, f32(0)), f32(nz - 1)).astype(f32)
    k0 = fz.astype(np.int32)
    k1 = np.minimum(k0 + 1, nz - 1)
    az = (fz - k0.astype(f32)).astype(f32)

    def corner(j, i):
        j, i = np.broadcast_to(j, k0.shape), np.broadcast_to(i, k0.shape)
        return _lerp(grid[j, i, k0], grid[j, i, k1], az)

    top = _lerp(corner(j0, i0), corner(j0, i1), np.broadcast_to(ax, k0.shape))
    bot = _lerp(corner(j1, i0), corner(j1, i1), np.broadcast_to(ax, k0.shape))
    return _lerp(top, bot, np.broadcast_to(ay, k0.shape))


def apply(p, grid, cell, m=None, offset=(0, 0)):
    """o = p g: what takes the place of p in steps 1-3 of the rendered output"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(p, f32) * gain(p, grid, cell, m, offset)[..., None]).astype(f32)


def render(p, grid, cell, fmt, m=None, lut=None, apply_gamma=False, offset=(0, 0)):
    """(float image, packed output) of the local-tone finish of p"""
    return R.render(apply(p, grid, cell, m, offset), fmt, m, lut, apply_gamma)
