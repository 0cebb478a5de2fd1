"""numpy restatement of the finish chain (include/mfsr.h, mfsr_finish_chain): the composition of the five
restatements -- tests/denoise_ref.py, tests/sharpen_ref.py, tests/local_tone_ref.py, tests/render_ref.py, tests/yuv_ref.py -- and
no arithmetic of its own.  Each stage runs on the whole array of the valid rows with its own replicated borders, so a stage's
stencil at a position outside the valid pixels reads the PREVIOUS stage's result at the clamped position: the sharpen reads the
denoised value of the clamped pixel."""
from __future__ import annotations

import numpy as np

from tests import denoise_ref as D
from tests import local_tone_ref as LT
from tests import render_ref as R
from tests import sharpen_ref as S
from tests import yuv_ref as Y

f32 = np.float32


def reach(denoise=None, sharpen=None):
    """R_d + R_s; a stage that is off counts 0."""
    return (denoise["radius"] if denoise else 0) + (len(sharpen["taps"]) - 1 if sharpen else 0)


def chain(p, n=None, denoise=None, sharpen=None, local_tone=None, m=None, offset=(0, 0), valid=None, rows=None):
    """Steps 2-4: the linear float image t that takes the place of p in the rendered output.
    p [h, w, 3]: the value the finish holds; n: the count image (None: 1 everywhere), used by the denoise stage only.
    denoise: the keyword arguments of denoise_ref.denoise (radius, strength, gain, alpha, beta, w_lo, w_hi) or None = off.
    sharpen: dict(taps, amount, threshold) of sharpen_ref.sharpen or None = off.
    local_tone: dict(grid, cell) of local_tone_ref.apply or None = off; m is the render description's matrix (the luma key goes
    through it) and offset = (x, y) of p[0, 0] in the full frame the grid belongs to.
    valid = (y0, y1): the rows of p the chain may read (default: all); rows = (a, b): the rows returned (default: valid).  The
    result is the chain run on exactly the valid rows, cropped to [a, b)."""
    p = np.asarray(p, f32)
    y0, y1 = (0, p.shape[0]) if valid is None else valid
    a, b = (y0, y1) if rows is None else rows
    assert 0 <= y0 <= a < b <= y1 <= p.shape[0]
    t = p[y0:y1]
    if denoise:
        t = D.denoise(t, None if n is None else np.asarray(n, f32)[y0:y1], **denoise)
    if sharpen:
        t = S.sharpen(t, sharpen["taps"], sharpen["amount"], sharpen.get("threshold", 0.0))
    if local_tone:
        t = LT.apply(t, local_tone["grid"], local_tone["cell"], m, (offset[0], offset[1] + y0))
    return t[a - y0:b - y0]


def render(p, fmt, n=None, denoise=None, sharpen=None, local_tone=None, m=None, lut=None, colour=0, offset=(0, 0), valid=None,
           rows=None):
    """Steps 2-5.  Single-plane formats: (float image, packed output) as render_ref.render; NV12 / P010: (float image, Y plane,
    UV plane) as yuv_ref.render with the colour description `colour`."""
    t = chain(p, n, denoise, sharpen, local_tone, m, offset, valid, rows)
    if fmt in (Y.NV12, Y.P010):
        return Y.render(t, fmt, m, lut, False, colour)
    return R.render(t, fmt, m, lut)
