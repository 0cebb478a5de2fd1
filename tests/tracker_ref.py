"""The tile tracker's reference: the oracle's unfused chain (what cfg.fused = 0 runs) for a whole tile grid.

    convertToTilesOverlapBorder -> convertToTilesOverlapPreShift (base shift, base rotation) -> crossCorrelateTiles ->
    squaredSum -> boxFilterWithBorderX -> boxFilterWithBorderY -> normalizedCC -> findMinimum (threshold) -> addRoundedPreShift

Every fused HIP form (tests/test_tracker_inputs_gpu.py, tests/test_parity_kernels.py) is compared with its coordinates bit for bit.
Arrays are numpy "device buffers" as in tests/kernels.py: an image of width W is any C-contiguous (H, >= W) float32 array whose
row stride is the pitch, a tile grid any (tcy, >= tcx, 2) array; the columns past the width are padding that nobody may touch.
"""
import ctypes

import numpy as np

from tests.kernels import F2, pitch_of

SENTINEL = np.float32(-7777.25)   # what coordinate buffers hold before a tracker writes them


def grid(W, H, T):
    """Tiles per axis of a W x H level image (make_layout of csrc/pipeline.cpp: an image smaller than a tile has one tile)."""
    return max(W // T, 1), max(H // T, 1)


def padded(a, pad, fill=np.nan):
    """`a` (rows, cols[, 2]) inside an array of `pad` more columns, which hold `fill`."""
    a = np.asarray(a, np.float32)
    out = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


def coord_buffer(tcx, tcy, pad=1):
    return np.full((tcy, tcx + pad, 2), SENTINEL, np.float32)


def libm_cos_sin(orc, rotation):
    """cosf / sinf of the C library the oracle links (looked up through the oracle's own handle): the functions orc_tile_fetch
    calls, so a device mfsr_prealign built from them gives the oracle's whole-pixel patch origin for any rotation."""
    lib = orc.o.cdll
    out = []
    for name in ("cosf", "sinf"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ctypes.c_float, [ctypes.c_float]
        out.append(np.float32(fn(ctypes.c_float(float(np.float32(rotation))))))
    return out


def prealign_record(orc, base):
    """Device mfsr_prealign (12 x 4 bytes: shiftX, shiftY, rotation, cos, sin, 7 x int32) of base = (shiftX, shiftY, rotation,
    invScale); None for no base."""
    if base is None:
        return None
    pa = np.zeros(12, np.float32)
    c, s = libm_cos_sin(orc, base[2])
    pa[:5] = [base[0], base[1], base[2], c, s]
    return pa


def upsampled(orc, coarse, up, tcx, tcy, pad=2):
    """UpSampleShifts of the coarse grid (up = (oldLevel, newLevel, oldCountX, oldCountY, oldTileSize, newTileSize)) into a
    pre-shift grid of `pad` padding columns."""
    oldL, newL, ocx, ocy, oldT, T = up
    pre = padded(np.zeros((tcy, tcx, 2), np.float32), pad, 0.0)
    orc.call("UpSampleShifts", coarse, pre, pitch_of(coarse), pitch_of(pre), oldL, newL, ocx, ocy, tcx, tcy, oldT, T)
    return pre


def oracle_track(orc, ref, mov, W, H, T, S, pre=None, coarse=None, up=None, threshold=0.0, base=None, coord_pad=1):
    """-> (coordinates, dist, squaredSums, pre): the chain's tile shifts in a coordinate buffer of `coord_pad` sentinel columns,
    its (tiles, 2S+1, 2S+1) distance images, its sum(ref^2) per tile and the pre-shift grid it used (given, up-sampled from
    `coarse` with `up`, or zero).  base = (shiftX, shiftY, rotation, invScale) of the moved frame, None = none."""
    tcx, tcy = grid(W, H, T)
    n, L, R = tcx * tcy, T + 2 * S, 2 * S + 1
    if pre is None:
        pre = upsampled(orc, coarse, up, tcx, tcy) if coarse is not None else padded(np.zeros((tcy, tcx, 2), np.float32), 2, 0.0)
    z = F2([0, 0])
    bs, rot = z, 0.0
    if base is not None:
        # the single multiply the kernel does; the oracle takes cosf / sinf of the rotation itself
        bs = F2([np.float32(base[0]) * np.float32(base[3]), np.float32(base[1]) * np.float32(base[3])])
        rot = float(np.float32(base[2]))
    rt = np.zeros((n, L, L), np.float32)
    mt = np.zeros((n, L, L), np.float32)
    cc = np.zeros((n, L, L), np.float32)
    bx = np.zeros((n, L, L), np.float32)
    by = np.zeros((n, L, L), np.float32)
    sq = np.zeros(n, np.float32)
    dist = np.zeros((n, R, R), np.float32)
    coord = coord_buffer(tcx, tcy, coord_pad)
    orc.call("convertToTilesOverlapBorder", ref, rt, W, H, pitch_of(ref), S, T, tcx, tcy, z, 0.0)
    orc.call("convertToTilesOverlapPreShift", mov, mt, pre, pitch_of(pre), W, H, pitch_of(mov), S, T, tcx, tcy, bs, rot)
    orc.call("crossCorrelateTiles", rt, mt, cc, S, T, n)
    orc.call("squaredSum", rt, sq, S, T, n)
    orc.call("boxFilterWithBorderX", mt, bx, S, T, n)
    orc.call("boxFilterWithBorderY", bx, by, S, T, n)
    orc.call("normalizedCC", cc, sq, by, dist, S, T, n)
    orc.call("findMinimum", dist, coord, pitch_of(coord), S, n, tcx, float(np.float32(threshold)))
    orc.call("addRoundedPreShift", pre, pitch_of(pre), coord, pitch_of(coord), tcx, tcy)
    return coord, dist, sq, pre


def serial_argmin(dist_tile):
    """findMinimum's scan of one distance image: (minVal, minIdx, maxVal); the first strict minimum, -1 when nothing is below
    FLT_MAX (every value NaN)."""
    fmax = np.finfo(np.float32).max
    min_val, max_val, min_idx = fmax, -fmax, -1
    for i, v in enumerate(np.asarray(dist_tile, np.float32).reshape(-1)):
        if not np.isnan(v):
            max_val = max(max_val, v)
        if v < min_val:
            min_val, min_idx = v, i
    return np.float32(min_val), min_idx, np.float32(max_val)
