"""Plain numpy restatement of the certainty-mask erosion (mfsr_erodeMaskBatch), and the zones and
error measures of the ghost tests.  The checker of tests/test_ghost_cpu.py and tests/test_ghost_gpu.py."""
from __future__ import annotations

import numpy as np


def erode_ref(mask: np.ndarray, radius: int) -> np.ndarray:
    """mask [h, w, 4] float32 -> eroded mask: .x .y .z = minimum over the (2r+1)^2 window clamped to the interior
    [1, w-2] x [1, h-2], each channel alone; .w passes through; the one-cell ring is zero."""
    h, w, _ = mask.shape
    assert h >= 3 and w >= 3 and radius in (1, 2)
    ys, xs = np.arange(1, h - 1), np.arange(1, w - 1)
    res = None
    for j in range(-radius, radius + 1):
        yy = np.clip(ys + j, 1, h - 2)
        for i in range(-radius, radius + 1):
            xx = np.clip(xs + i, 1, w - 2)
            tap = mask[yy][:, xx, :3]
            res = tap if res is None else np.minimum(res, tap)
    out = np.zeros_like(mask)
    out[1:-1, 1:-1, :3] = res
    out[1:-1, 1:-1, 3] = mask[1:-1, 1:-1, 3]
    return out


def dilate_bool(a: np.ndarray, d: int) -> np.ndarray:
    """Every pixel within d pixels (Chebyshev) of a set pixel."""
    h, w = a.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), 0), 1)
    y0, y1 = np.clip(np.arange(h) - d, 0, h), np.clip(np.arange(h) + d + 1, 0, h)
    x0, x1 = np.clip(np.arange(w) - d, 0, w), np.clip(np.arange(w) + d + 1, 0, w)
    return (c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]) > 0


def ghost_zones(footprints: np.ndarray, reference: int, radius: int, scale: int):
    """(G, S) on the HR grid: G = covered by the object in some non-reference frame but not in the reference frame;
    S = at least 2*(2r+1)*scale HR pixels away from every footprint."""
    others = np.zeros_like(footprints[0])
    for k in range(footprints.shape[0]):
        if k != reference:
            others |= footprints[k]
    G = others & ~footprints[reference]
    S = ~dilate_bool(footprints.any(0), 2 * (2 * radius + 1) * scale - 1)
    return G, S


def zone_mse(img_hwc: np.ndarray, gt_chw: np.ndarray, zone: np.ndarray) -> float:
    d = img_hwc.astype(np.float64) - np.moveaxis(gt_chw, 0, -1).astype(np.float64)
    return float((d[zone] ** 2).mean())


def psnr_db(mse: float) -> float:
    return float(10.0 * np.log10(1.0 / mse))


class ErodingOracle:
    """Wraps the oracle library object of an OraclePipeline so that the numpy erosion runs on the mask right after
    ComputeRobustnessMask (between stage F and stage G); radius 0 = no erosion.  oracle/ itself is not touched."""

    def __init__(self, o, radius: int):
        self._o, self._r = o, radius

    def __getattr__(self, name):
        return getattr(self._o, name)

    def ComputeRobustnessMask(self, ref_half, mov_half, mask, *args):
        self._o.ComputeRobustnessMask(ref_half, mov_half, mask, *args)
        if self._r > 0:
            mask[...] = erode_ref(mask, self._r)


def run_oracle_eroded(cfg, frames, radius: int):
    """tests/burst_compare.py::run_oracle with the erosion between stage F and stage G: (float HR image, per-frame masks)."""
    from oracle.pipeline import OraclePipeline
    op = OraclePipeline(cfg)
    op.o = ErodingOracle(op.o, radius)
    nf = [(f.cpu().numpy() if hasattr(f, "cpu") else f).view(np.uint16) for f in frames]
    img_out = np.zeros((op.hrH, op.hrW, 3), np.float32)
    tw = np.zeros_like(img_out)
    op.set_reference(nf[cfg.reference])
    masks = []
    for k, f in enumerate(nf):
        op.add_frame(f, k == cfg.reference, img_out, tw)
        masks.append(op.mask)
    out, _ = op.finish(img_out, tw, want16=False)
    return out, masks


# ---- the scene of the quality tests ---------------------------------------------------------------------------------------------
# Chosen on the CPU oracle (tests/test_ghost_cpu.py) so that the oracle alone ghosts: a 48 x 48 LR-pixel patch (smaller than a
# tracker tile of 64 raw pixels) of saturated pixel-scale texture around mid grey, moving 70 x 13 LR pixels per frame (far
# beyond the tracker's and Lucas-Kanade's reach), in a two-frame burst, where a merged wrong frame carries half the weight.
# Low-contrast texture ghosts too weakly for the condition: the static zone S contains the output's never-written outermost
# ring, which alone puts mse0(S) near 1e-3.
GHOST_W, GHOST_H, GHOST_N, GHOST_SCALE = 1024, 768, 2, 2
# measured by test_erosion_suppresses_ghosts_on_the_oracle (which asserts that they still are what it measures)
ORACLE_RATIO_G = 0.0817     # mse2(G) / mse0(G): mse0(G) 9.861e-3 (9.88 x mse0(S) 9.985e-4), mse2(G) 8.052e-4: 10.88 dB
ORACLE_DROP_S_DB = 0.0056  # PSNR0(S) - PSNR2(S): mse2(S) 9.998e-4


def ghost_scene():
    """(cfg, frames, ground truth [3, sH, sW] numpy, footprints [N, sH, sW] numpy bool); applyGamma 0, float output."""
    from multi_frame_super_resolution_amd.pipeline import default_config
    from multi_frame_super_resolution_amd.synth import make_moving_burst
    frames, _, gt, foot = make_moving_burst(GHOST_W, GHOST_H, GHOST_N, scale=GHOST_SCALE, seed=777, max_shift=1.0, obj_size=(48, 48),
                                            obj_start=(200.0, 200.0), obj_step=(70.0, 13.0), obj_level=0.5, obj_texture=3.0)
    cfg = default_config(GHOST_W, GHOST_H, GHOST_N, GHOST_SCALE, False)
    cfg.applyGamma = 0
    return cfg, frames, gt.numpy(), foot.numpy()
