"""What the merge-aware denoise of DESIGN.md section 2.24 does to a merged image, on the CPU: the oracle pipeline on
synth.make_moving_burst(256, 192, 6, alpha=1.6e-3, beta=1.6e-5, obj_size=(48, 48), obj_step=(9.0, 3.0)) (linear output) and on
its noise=False twin, then the numpy restatement (tests/denoise_ref.py) at R = 3, strength 3, gain 4, no fade, with the
burst's alpha and beta.  Pixels are split by their minimum channel weight (< 1.5, [1.5, 4), >= 4), 16 pixels of border left out.
Per class: the PSNR of the merge and of the denoised merge against the noiseless twin's merge and against the ground truth, the
gains, and the measured / predicted variance ratio (the mean over the class's samples of (merge - noiseless merge)^2 over
(alpha p + beta) / n).  `clean`: what the same filter costs on the noiseless twin's merge (the PSNR of its denoised image
against itself undenoised, and its PSNR against the ground truth before and after).  One JSON line.

    python tools/denoise_quality.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BURST = dict(width=256, height=192, frames=6, alpha=1.6e-3, beta=1.6e-5, obj_size=(48, 48), obj_step=(9.0, 3.0))
FILTER = dict(radius=3, strength=3.0, gain=4.0)
CLASSES = (("lt1.5", 0.0, 1.5), ("1.5to4", 1.5, 4.0), ("ge4", 4.0, np.inf))
BORDER = 16


def _psnr(a, b, mask):
    d = (a.astype(np.float64) - b.astype(np.float64))[mask]
    mse = float((d * d).mean())
    return 200.0 if mse == 0 else float(10 * np.log10(1.0 / mse))


def merges():
    """(noisy merge, its weights, noiseless merge, its weights, ground truth [h, w, 3], weightThreshold): oracle bursts"""
    from multi_frame_super_resolution_amd import synth
    from multi_frame_super_resolution_amd.pipeline import default_config
    from tests.burst_compare import run_oracle

    kw = dict(BURST)
    W, H, N = kw.pop("width"), kw.pop("height"), kw.pop("frames")
    cfg = default_config(W, H, N, 2, False)
    cfg.applyGamma = 0
    noisy, _, gt, _ = synth.make_moving_burst(W, H, N, **kw)
    clean, _, _, _ = synth.make_moving_burst(W, H, N, noise=False, **kw)
    a, b = run_oracle(cfg, noisy), run_oracle(cfg, clean)
    truth = gt.permute(1, 2, 0).numpy().astype(np.float32)
    return a["out"], a["tw"], b["out"], b["tw"], truth, float(cfg.weightThreshold)


def experiment(data=None):
    from tests import denoise_ref as D

    lin, tw, lin0, tw0, truth, thr = merges() if data is None else data
    alpha, beta = BURST["alpha"], BURST["beta"]
    den = D.finish_denoise(lin, tw, thr, alpha=alpha, beta=beta, **FILTER)
    den0 = D.finish_denoise(lin0, tw0, thr, alpha=alpha, beta=beta, **FILTER)
    inner = np.zeros(lin.shape[:2], bool)
    inner[BORDER:-BORDER, BORDER:-BORDER] = True
    wmin = tw.min(axis=2)
    n = np.maximum(D.count_of_weight(tw, thr), 1e-6).astype(np.float64)
    predicted = (alpha * np.maximum(lin.astype(np.float64), 0) + beta) / n
    out = {"burst": {k: v for k, v in BURST.items()}, "filter": FILTER, "classes": {}}
    for name, lo, hi in CLASSES:
        m = inner & (wmin >= lo) & (wmin < hi)
        m3 = np.broadcast_to(m[..., None], lin.shape)
        err = (lin.astype(np.float64) - lin0.astype(np.float64))[m3]
        c = {"pixels": int(m.sum()),
             "psnr_vs_noiseless": [_psnr(lin, lin0, m3), _psnr(den, lin0, m3)],
             "psnr_vs_truth": [_psnr(lin, truth, m3), _psnr(den, truth, m3)],
             "variance_measured_over_predicted": float((err * err / predicted[m3]).mean())}
        c["gain_vs_noiseless_db"] = c["psnr_vs_noiseless"][1] - c["psnr_vs_noiseless"][0]
        c["gain_vs_truth_db"] = c["psnr_vs_truth"][1] - c["psnr_vs_truth"][0]
        out["classes"][name] = c
    i3 = np.broadcast_to(inner[..., None], lin.shape)
    out["clean"] = {"psnr_denoised_vs_itself": _psnr(den0, lin0, i3),
                    "psnr_vs_truth": [_psnr(lin0, truth, i3), _psnr(den0, truth, i3)]}
    return out


def main():
    out = experiment()

    def rnd(v):
        if isinstance(v, dict):
            return {k: rnd(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [rnd(x) for x in v]
        return float(f"{v:.4g}") if isinstance(v, float) else v

    print(json.dumps(rnd(out)), flush=True)


if __name__ == "__main__":
    main()
