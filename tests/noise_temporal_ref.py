"""Burst noise calibration, restated in numpy: the block statistics of mfsr_noiseStatsTemporal (float32 for
h, d and r, integers after that) and the fit of mfsr_noise_fit_temporal.  Shared by tests/test_noise_temporal_cpu.py and
tests/test_noise_temporal_gpu.py; the bins and the fit are those of tests/test_noise_cpu.py."""
import numpy as np

import tests.test_noise_cpu as _noise
from tests.test_noise_cpu import BLACK, MIN_BLOCKS, NL, NQ, NV, SAT, WHITE, bin_bounds, fit_rule, var_bin  # noqa: F401

CHI2_8_MEDIAN_X4 = 29.3764      # 4 x the median of chi-square with 8 degrees of freedom
DEFAULT_TOL = 1.0 / 16.0
MAX_SHIFT = np.float32(16384.0)


def roundf(x):
    """C's roundf (halves away from zero) of a float32 array, as int64.  |x| + 0.5 is exact in float64."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(np.int64)


def placement(flow, rect, w, h):
    """(h [nby, nbx, 2] float32, placed [nby, nbx] bool) of one frame over the block rectangle; flow None = zero flow, else a
    float32 array [fh, fw, 2]."""
    bx0, by0, bx1, by1 = rect
    nby, nbx = by1 - by0, bx1 - bx0
    if flow is None:
        return np.zeros((nby, nbx, 2), dtype=np.float32), np.ones((nby, nbx), dtype=bool)
    flow = np.asarray(flow, dtype=np.float32)
    fh, fw = flow.shape[:2]
    assert (fw, fh) in ((w // 2, h // 2), (w, h))
    fx = (8 * np.arange(bx0, bx1) + 4) * fw // w
    fy = (8 * np.arange(by0, by1) + 4) * fh // h
    with np.errstate(invalid="ignore", over="ignore"):
        hh = np.float32(0.5) * flow[fy[:, None], fx[None, :]]
        placed = (np.abs(hh[..., 0]) <= MAX_SHIFT) & (np.abs(hh[..., 1]) <= MAX_SHIFT)     # (false for NaN and +-inf)
    hh = np.where(placed[..., None], hh, np.float32(0.0)).astype(np.float32)
    return hh, placed


def accepted_pairs(flows, rect, w, h, tol=DEFAULT_TOL):
    """{(j, k): number of blocks of rect at which the pair passes the phase test} (sites and saturation not looked at)."""
    tol = np.float32(tol)
    pl = [placement(f, rect, w, h) for f in flows]
    out = {}
    for j in range(len(flows)):
        for k in range(j + 1, len(flows)):
            d = pl[k][0] - pl[j][0]
            r = d - roundf(d).astype(np.float32)
            n = int((pl[j][1] & pl[k][1] & (np.abs(r[..., 0]) <= tol) & (np.abs(r[..., 1]) <= tol)).sum())
            if n:
                out[(j, k)] = n
    return out


def stats_temporal_rule(frames, flows, rect, tol=DEFAULT_TOL, black=BLACK, sat=SAT):
    """(hist [4][64][272] u32, levelSum [4][64] i64, count [4][64] i64) of mfsr_noiseStatsTemporal: u16 frames [h, w], per frame a
    flow field (float32 [fh, fw, 2]) or None, the block rectangle rect = (bx0, by0, bx1, by1), tol as the float32 it is passed as."""
    hist = np.zeros((NQ, NL, NV), dtype=np.uint32)
    level_sum = np.zeros((NQ, NL), dtype=np.int64)
    count = np.zeros((NQ, NL), dtype=np.int64)
    frames = [np.asarray(f).view(np.uint16) if np.asarray(f).dtype == np.int16 else np.asarray(f) for f in frames]
    h, w = frames[0].shape
    tol = np.float32(tol)
    bx0, by0, bx1, by1 = rect
    gy, gx = np.meshgrid(8 * np.arange(by0, by1), 8 * np.arange(bx0, bx1), indexing="ij")
    pl = [placement(f, rect, w, h) for f in flows]
    site = [roundf(p[0]) for p in pl]
    k8 = np.arange(8)
    for j in range(len(frames)):
        for k in range(j + 1, len(frames)):
            d = pl[k][0] - pl[j][0]                                   # float32
            s = roundf(d)
            r = d - s.astype(np.float32)                              # float32
            ax, ay = gx + 2 * site[j][..., 0], gy + 2 * site[j][..., 1]
            cx, cy = ax + 2 * s[..., 0], ay + 2 * s[..., 1]
            acc = pl[j][1] & pl[k][1] & (np.abs(r[..., 0]) <= tol) & (np.abs(r[..., 1]) <= tol)
            acc &= (ax >= 0) & (ax + 8 <= w) & (ay >= 0) & (ay + 8 <= h) & (cx >= 0) & (cx + 8 <= w) & (cy >= 0) & (cy + 8 <= h)
            if not acc.any():
                continue
            ax, ay, cx, cy = ax[acc], ay[acc], cx[acc], cy[acc]
            A = frames[j][(ay[:, None] + k8)[:, :, None], (ax[:, None] + k8)[:, None, :]].astype(np.int64)    # [m, 8, 8]
            B = frames[k][(cy[:, None] + k8)[:, :, None], (cx[:, None] + k8)[:, None, :]].astype(np.int64)
            usable = (A < sat).all(axis=(1, 2)) & (B < sat).all(axis=(1, 2))
            for q in range(4):
                p = A[:, q >> 1::2, q & 1::2]                          # [m][r][c]
                t = p - B[:, q >> 1::2, q & 1::2]
                S = p.sum(axis=(1, 2))
                d0, d1 = t[:, :, 0] - t[:, :, 1], t[:, :, 2] - t[:, :, 3]
                D = (d0 * d0 + d1 * d1).sum(axis=1)
                span = 16 * (sat - black[q])
                lev = np.clip(S - 16 * black[q], 0, span - 1) * 64 // span
                v = np.minimum(var_bin(D), NV - 1)
                np.add.at(hist[q], (lev[usable], v[usable]), 1)
                np.add.at(level_sum[q], lev[usable], S[usable])
                np.add.at(count[q], lev[usable], 1)
    return hist, level_sum, count


def fit_temporal_rule(hist, level_sum, count, black=BLACK, white=WHITE, min_blocks=MIN_BLOCKS):
    """(alpha, beta, status, points): fit_rule of tests/test_noise_cpu.py with var = median / 29.3764."""
    keep = _noise.CHI2_8_MEDIAN_X2
    _noise.CHI2_8_MEDIAN_X2 = CHI2_8_MEDIAN_X4
    try:
        return fit_rule(hist, level_sum, count, black, white, min_blocks)
    finally:
        _noise.CHI2_8_MEDIAN_X2 = keep


def calibrate_temporal_rule(frames, flows, tol=DEFAULT_TOL, min_blocks=MIN_BLOCKS, black=BLACK, white=WHITE, sat=SAT):
    """(alpha, beta, status, points, blocks) over the default rectangle, as mfsr_burst_calibrate_noise_temporal computes them from
    these flows."""
    h, w = np.asarray(frames[0]).shape
    st = stats_temporal_rule(frames, flows, _noise.default_rect(w, h), tol, black, sat)
    return fit_temporal_rule(*st, black, white, min_blocks) + (int(st[2][0].sum()),)


# frame k of synth.make_burst samples the scene at x + shift_k: the scene point that reference pixel p shows (shift_0 = 0) is at
# pixel p - shift_k of frame k, so in the burst's convention (reference pixel p <-> pixel p + flow) the flow is -shift_k
FLOW_SIGN = -1.0


def shifts_as_flows(shifts, w, h, mono=False):
    """The true shifts of synth.make_burst (LR = raw pixels, [N, 2]) as constant flow fields at the burst's tracking resolution,
    in the burst's convention; frame 0 gets None when its shift is zero."""
    fw, fh = (w, h) if mono else (w // 2, h // 2)
    out = []
    for k, t in enumerate(np.asarray(shifts, dtype=np.float64)):
        if k == 0 and not t.any():
            out.append(None)
            continue
        f = np.empty((fh, fw, 2), dtype=np.float32)
        f[..., 0], f[..., 1] = np.float32(FLOW_SIGN * t[0]), np.float32(FLOW_SIGN * t[1])
        out.append(f)
    return out
