"""What the geometric finish of DESIGN.md section 2.27 corrects, on the CPU: a synthetic grid of Gaussian dots (256 x 192, one dot
every 24 pixels) is distorted with a known barrel term (k1 = -0.03 of the forward model, r normalised by the half diagonal) and
its red and blue planes are magnified by 1.004 and 0.997 against green; the numpy restatement (tests/geometry_ref.py) then
resamples it with the same numbers (Catmull-Rom and bilinear).  Per image: the worst displacement of a dot's green centroid from
the ideal grid and the worst distance between a dot's red (or blue) and green centroid, in pixels, over the dots at least 16
pixels inside the frame; and after / before of both.  One JSON line.

    python tools/geometry_quality.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W, H, PITCH, SIGMA, WINDOW, BORDER = 256, 192, 24, 1.6, 9, 16
K1, LATERAL = -0.03, (1.004, 0.997)


def grid_points():
    xs = np.arange(PITCH / 2, W, PITCH)
    ys = np.arange(PITCH / 2, H, PITCH)
    return [(x, y) for y in ys for x in xs if BORDER <= x < W - BORDER and BORDER <= y < H - BORDER]


def distorted_dots():
    """[H, W, 3] float32: every ideal dot centre q drawn at c + (q - c) * m_c(rho(q)), the forward model per channel"""
    yy, xx = np.mgrid[0:H, 0:W]
    cx, cy = W / 2.0, H / 2.0
    rn2 = 1.0 / (cx * cx + cy * cy)
    img = np.zeros((H, W, 3), np.float64)
    k0 = (LATERAL[0], 1.0, LATERAL[1])
    for (qx, qy) in grid_points():
        dx, dy = qx - cx, qy - cy
        rho = (dx * dx + dy * dy) * rn2
        for c in range(3):
            m = K1 * rho + k0[c]
            px, py = cx + dx * m, cy + dy * m
            # pixel X covers [X, X + 1): its centre is X + 0.5
            img[..., c] += np.exp(-(((xx + 0.5) - px) ** 2 + ((yy + 0.5) - py) ** 2) / (2 * SIGMA * SIGMA))
    return (0.05 + 0.9 * img).astype(np.float32)


def centroids(img):
    """{ideal point: [3 centroids (x, y)]} of the background-free image in a window around each ideal point"""
    out = {}
    v = np.maximum(img.astype(np.float64) - 0.05, 0.0)
    for (qx, qy) in grid_points():
        x0, y0 = int(qx) - WINDOW, int(qy) - WINDOW
        win = v[y0:y0 + 2 * WINDOW + 1, x0:x0 + 2 * WINDOW + 1]
        yy, xx = np.mgrid[y0:y0 + win.shape[0], x0:x0 + win.shape[1]]
        cs = []
        for c in range(3):
            s = win[..., c].sum()
            cs.append((float(((xx + 0.5) * win[..., c]).sum() / s), float(((yy + 0.5) * win[..., c]).sum() / s)))
        out[(qx, qy)] = cs
    return out


def errors(img):
    """(worst green displacement from the grid, worst red-or-blue to green distance), pixels"""
    disp = fringe = 0.0
    for (qx, qy), cs in centroids(img).items():
        disp = max(disp, float(np.hypot(cs[1][0] - qx, cs[1][1] - qy)))
        for c in (0, 2):
            fringe = max(fringe, float(np.hypot(cs[c][0] - cs[1][0], cs[c][1] - cs[1][1])))
    return disp, fringe


def measure():
    from tests import geometry_ref as G

    src = distorted_dots()
    before = errors(src)
    out = {"width": W, "height": H, "k1": K1, "lateral": list(LATERAL), "dots": len(grid_points()),
           "before": {"displacement_px": round(before[0], 4), "fringe_px": round(before[1], 4)}}
    for name, filt in (("cubic", G.CUBIC), ("bilinear", G.BILINEAR)):
        after = errors(G.resample(src, G.lens(W, H, W, H, distortion=(K1, 0.0, 0.0), lateral=LATERAL, filter=filt)))
        out[name] = {"displacement_px": round(after[0], 4), "fringe_px": round(after[1], 4),
                     "displacement_ratio": round(after[0] / before[0], 4), "fringe_ratio": round(after[1] / before[1], 4)}
    return out


if __name__ == "__main__":
    print(json.dumps(measure()))
