"""What the unsharp mask of DESIGN.md section 2.20 does to a merged image, on the CPU: the oracle pipeline on
synth.make_burst(512, 384, 6) (linear output), then the numpy restatement (tests/sharpen_ref.py) at sigma 1 and amount 0 (the
plain merge), 0.5, 1 and 2.  Reported, not asserted: the PSNR against the ground truth (16 pixels of border left out) and the
10-90 % rise width, in HR pixels, of the sharpest horizontal edge of the scene (the largest luminance step between two
neighbouring ground-truth pixels; the profile of that row, 8 pixels either side, linearly interpolated; the plateaus are the
means of the profile's outer three samples).  One JSON line.

    python tools/sharpen_quality.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def rise_width(profile):
    """10-90 % rise width of a monotone-ish edge profile (falling edges are flipped), in samples"""
    p = np.asarray(profile, np.float64)
    lo, hi = p[:3].mean(), p[-3:].mean()
    if hi < lo:
        p, lo, hi = p[::-1], hi, lo
    x = np.linspace(0, p.size - 1, (p.size - 1) * 100 + 1)
    f = np.interp(x, np.arange(p.size), p)
    a = x[np.argmax(f >= lo + 0.1 * (hi - lo))]
    b = x[np.argmax(f >= lo + 0.9 * (hi - lo))]
    return float(b - a)


def main():
    from multi_frame_super_resolution_amd import synth
    from multi_frame_super_resolution_amd.pipeline import default_config
    from tests import sharpen_ref as S
    from tests.burst_compare import psnr, run_oracle

    W, H, N = 512, 384, 6
    frames, _, gt = synth.make_burst(W, H, N)
    cfg = default_config(W, H, N, 2, False)
    cfg.applyGamma = 0
    lin = run_oracle(cfg, frames)["out"]
    truth = gt.permute(1, 2, 0).numpy().astype(np.float32)
    m = (truth.shape[0] - lin.shape[0]) // 2
    truth = truth[m:m + lin.shape[0], m:m + lin.shape[1]] if m > 0 else truth
    luma = truth.mean(axis=2)
    step = np.abs(np.diff(luma[24:-24, 24:-24], axis=1))
    y, x = np.unravel_index(np.argmax(step), step.shape)
    y, x = y + 24, x + 24
    _, taps = S.gaussian_taps(1.0, 0)
    out = {"edge_at": [int(x), int(y)], "truth_rise_px": round(rise_width(luma[y, x - 8:x + 10]), 2), "amounts": {}}
    for amount in (0.0, 0.5, 1.0, 2.0):
        img = S.sharpen(lin, taps, amount, 0.0) if amount else lin
        out["amounts"][str(amount)] = {"psnr_db": round(psnr(img[16:-16, 16:-16], truth[16:-16, 16:-16]), 2),
                                       "rise_px": round(rise_width(img.mean(axis=2)[y, x - 8:x + 10]), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
