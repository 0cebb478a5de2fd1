"""Noise-model calibration, the part that needs no GPU: a numpy restatement of the block statistics
(mfsr_noiseStats) and of the fit (mfsr_noise_fit), the host-side refusals of the C-ABI, the fit against the restatement on
hand-made histograms, the chi-square constant, and the synthetic chart."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = ctypes.c_int32 * 4
F4 = ctypes.c_float * 4

NQ, NL, NV = 4, 64, 272
BLACK = (256, 256, 256, 256)
WHITE = (3839.0, 3839.0, 3839.0, 3839.0)
SAT = 4095
CHI2_8_MEDIAN_X2 = 14.6882      # 2 x the median of chi-square with 8 degrees of freedom (7.3441)
MIN_BLOCKS = 200
# the recovery fixtures of tests/test_noise_gpu.py: 8 frames of 512 x 384, these noise models
CHART = dict(width=512, height=384, frames=8)
CHART_MODELS = ((1e-4, 1e-6), (1.6e-3, 1.6e-5))


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def var_bin(D):
    """Variance bin of D (int64 array, 0 <= D < 2^36): D itself below 16, then 8 sub-bins per octave."""
    D = np.asarray(D, dtype=np.int64)
    e = np.zeros(D.shape, dtype=np.int64)
    for k in range(1, 37):
        e[D >= (np.int64(1) << k)] = k                      # floor(log2 D), exact
    sh = np.maximum(e - 3, 0)
    return np.where(D < 16, D, 16 + 8 * (e - 4) + ((D >> sh) & 7))


def bin_bounds(v):
    """[lo, hi) of the D values of variance bin v."""
    if v < 16:
        return v, v + 1
    e, m = 4 + (v - 16) // 8, (v - 16) % 8
    return (8 + m) << (e - 3), (9 + m) << (e - 3)


def full_rect(w, h):
    return (0, 0, w // 8, h // 8)


def default_rect(w, h):
    """The whole block grid minus one block of border."""
    return (1, 1, w // 8 - 1, h // 8 - 1)


def stats_rule(frames, rect, black=BLACK, sat=SAT):
    """(hist [4][64][272] u32, levelSum [4][64] i64, count [4][64] i64) of u16 frames [h, w] over the block rectangle
    rect = (bx0, by0, bx1, by1)."""
    hist = np.zeros((NQ, NL, NV), dtype=np.uint32)
    level_sum = np.zeros((NQ, NL), dtype=np.int64)
    count = np.zeros((NQ, NL), dtype=np.int64)
    bx0, by0, bx1, by1 = rect
    nby, nbx = by1 - by0, bx1 - bx0
    for f in frames:
        a = np.asarray(f).view(np.uint16) if np.asarray(f).dtype == np.int16 else np.asarray(f)
        a = a[8 * by0:8 * by1, 8 * bx0:8 * bx1].astype(np.int64)
        usable = (a.reshape(nby, 8, nbx, 8) < sat).all(axis=(1, 3))
        for q in range(4):
            p = a[q >> 1::2, q & 1::2].reshape(nby, 4, nbx, 4)            # [by][r][bx][c]
            S = p.sum(axis=(1, 3))
            d0, d1 = p[:, :, :, 0] - p[:, :, :, 1], p[:, :, :, 2] - p[:, :, :, 3]
            D = (d0 * d0 + d1 * d1).sum(axis=1)
            span = 16 * (sat - black[q])
            lev = np.clip(S - 16 * black[q], 0, span - 1) * 64 // span
            v = var_bin(D)
            np.add.at(hist[q], (lev[usable], v[usable]), 1)
            np.add.at(level_sum[q], lev[usable], S[usable])
            np.add.at(count[q], lev[usable], 1)
    return hist, level_sum, count


def fit_rule(hist, level_sum, count, black=BLACK, white=WHITE, min_blocks=MIN_BLOCKS):
    """(alpha, beta, status, points) of the fit, operation by operation as DESIGN.md section 2.15 lists them (doubles)."""
    sw = sx = sy = sxx = sxy = 0.0
    n, xmin, xmax = 0, 0.0, 0.0
    for q in range(NQ):
        for lev in range(NL):
            c = int(count[q][lev])
            if c < min_blocks or c <= 0:
                continue
            rank = 0.5 * float(c)
            cum, med, found = 0.0, 0.0, False
            for v in range(NV):
                h = float(hist[q][lev][v])
                if h > 0.0 and cum + h >= rank:
                    lo, hi = bin_bounds(v)
                    med = float(lo) + (rank - cum) / h * float(hi - lo)
                    found = True
                    break
                cum += h
            if not found:
                continue
            var_dn = med / CHI2_8_MEDIAN_X2
            wq = float(np.float32(white[q]))
            x = (float(level_sum[q][lev]) / (16.0 * float(c)) - float(black[q])) / wq
            y = max(var_dn - 1.0 / 12.0, 0.0) / (wq * wq)
            w = float(c)
            sw += w
            sx += w * x
            sy += w * y
            sxx += w * x * x
            sxy += w * x * y
            xmin = x if n == 0 else min(xmin, x)
            xmax = x if n == 0 else max(xmax, x)
            n += 1
    if n < 4 or xmax - xmin < 0.125:
        return 0.0, 0.0, 2, n
    den = sw * sxx - sx * sx
    alpha = (sw * sxy - sx * sy) / den
    beta = (sy - alpha * sx) / sw
    if beta < 0.0:
        beta = 0.0
        alpha = sxy / sxx
    return alpha, beta, (0 if alpha > 0.0 else 3), n


def calibrate_rule(frames, black=BLACK, white=WHITE, sat=SAT, min_blocks=MIN_BLOCKS):
    h, w = np.asarray(frames[0]).shape
    return fit_rule(*stats_rule(frames, default_rect(w, h), black, sat), black, white, min_blocks)


def chart(alpha, beta, mono=False, seed=1234, **size):
    from multi_frame_super_resolution_amd.synth import make_chart_burst
    size = dict(CHART, **size)
    return [f.numpy().view(np.uint16) for f in make_chart_burst(size["width"], size["height"], size["frames"], alpha, beta,
                                                               mono=mono, seed=seed)]


def recovery_bound(err):
    """The bound of the GPU recovery test on |alpha_est / alpha - 1|: three times the error of THIS restatement on the same
    fixture, at least 2 %."""
    return max(3.0 * err, 0.02)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def _fit_c(hist, level_sum, count, black=BLACK, white=WHITE, min_blocks=MIN_BLOCKS):
    from multi_frame_super_resolution_amd import capi
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    level_sum = np.ascontiguousarray(level_sum, dtype=np.int64)
    count = np.ascontiguousarray(count, dtype=np.int64)
    a, b = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    st, n = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = capi.lib().raw["mfsr_noise_fit"](hist.ctypes.data, level_sum.ctypes.data, count.ctypes.data, I4(*black), F4(*white),
                                          int(min_blocks), ctypes.byref(a), ctypes.byref(b), ctypes.byref(st), ctypes.byref(n))
    return rc, a.value, b.value, st.value, n.value


def _close(a, b):
    return abs(a - b) <= 1e-9 * max(abs(a), abs(b))


def _tables():
    return (np.zeros((NQ, NL, NV), dtype=np.uint32), np.zeros((NQ, NL), dtype=np.int64), np.zeros((NQ, NL), dtype=np.int64))


def _fill(hist, level_sum, count, q, lev, sigma2, n, rng, white=WHITE, black=BLACK):
    """n blocks of variance sigma2 (DN^2) at level bin lev of position q: D = 2 sigma2 chi2_8 draws."""
    D = np.floor(2.0 * sigma2 * rng.chisquare(8, n)).astype(np.int64)
    np.add.at(hist[q][lev], var_bin(D), 1)
    span = 16 * (SAT - black[q])
    S = (lev * span + span // 2) // 64 + 16 * black[q]
    level_sum[q][lev] += n * S
    count[q][lev] += n


def test_abi_prototypes_parse():
    from multi_frame_super_resolution_amd import capi
    protos = capi.parse_header()
    for name in ("mfsr_noiseStats", "mfsr_noise_fit", "mfsr_noise_defaults", "mfsr_burst_calibrate_noise"):
        assert name in protos, name
        assert protos[name][0] == "int"
    assert [t for t, _ in protos["mfsr_noiseStats"][1]] == [
        "int", "const uint16_t*const*", "int", "int", "int", "const int32_t*", "int", "const int32_t*", "uint32_t*", "long long*",
        "long long*", "mfsr_stream_t"]
    L = capi.lib()                     # resolves every declared symbol
    assert "mfsr_noiseStats" in L.raw and "mfsr_burst_calibrate_noise" in L.raw


def test_stats_refusals_happen_on_the_host():
    """Every bad argument is MFSR_E_INVALID (-1) before any device call: there is no device here (or the pointers are not
    device pointers), so a call that got as far as the device would fail with another code, or crash."""
    from multi_frame_super_resolution_amd import capi
    f = capi.lib().raw["mfsr_noiseStats"]
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    out = ctypes.create_string_buffer(16)
    o = (ctypes.addressof(out) + 7) // 8 * 8

    def call(n=1, ptrs=None, pitch=128, w=64, h=64, black=BLACK, sat=SAT, rect=(0, 0, 8, 8), hist=o, ls=o, cnt=o):
        p = (ctypes.c_void_p * max(n, 1))(*([base] * max(n, 1))) if ptrs is None else ptrs
        return f(n, p, pitch, w, h, I4(*black), sat, I4(*rect), hist, ls, cnt, None)

    assert call(n=0) == -1 and call(n=65) == -1 and call(n=-1) == -1               # frame count
    assert call(w=63) == -1 and call(h=63) == -1 and call(w=0) == -1                # even sizes
    assert call(pitch=126) == -1 and call(pitch=129) == -1
    assert call(sat=0) == -1 and call(sat=65536) == -1 and call(sat=-5) == -1       # sat range
    assert call(black=(256, 256, 256, 4095)) == -1 and call(black=(-1, 0, 0, 0)) == -1
    assert call(rect=(2, 2, 2, 5)) == -1 and call(rect=(2, 5, 4, 5)) == -1 and call(rect=(4, 0, 2, 8)) == -1   # empty
    assert call(rect=(0, 0, 9, 8)) == -1 and call(rect=(0, 0, 8, 9)) == -1 and call(rect=(-1, 0, 8, 8)) == -1  # outside
    assert call(w=70, h=70, pitch=140, rect=(0, 0, 9, 8)) == -1                    # the partial edge block is not in the grid
    assert call(hist=None) == -1 and call(ls=None) == -1 and call(cnt=None) == -1
    assert call(ptrs=(ctypes.c_void_p * 1)(None)) == -1 and call(ptrs=(ctypes.c_void_p * 1)(base + 1)) == -1
    assert f(1, None, 128, 64, 64, I4(*BLACK), SAT, I4(0, 0, 8, 8), o, o, o, None) == -1
    g = capi.lib().raw["mfsr_burst_calibrate_noise"]
    assert g(None, 1, None, None, None, None, None, None) == -1


def test_fit_refusals():
    h, s, c = _tables()
    assert _fit_c(h, s, c, min_blocks=0)[0] == -1
    assert _fit_c(h, s, c, white=(3839.0, 0.0, 3839.0, 3839.0))[0] == -1
    assert _fit_c(h, s, c, black=(256, 256, -1, 256))[0] == -1
    from multi_frame_super_resolution_amd import capi
    assert capi.lib().raw["mfsr_noise_fit"](None, None, None, I4(*BLACK), F4(*WHITE), 200, None, None, None, None) == -1


@pytest.mark.parametrize("alpha,beta", [(1e-4, 1e-6), (1.6e-3, 1.6e-5), (5e-4, 0.0)])
def test_fit_equals_the_restatement_on_hand_made_histograms(alpha, beta):
    rng = np.random.default_rng(7)
    h, s, c = _tables()
    for q in range(4):
        for lev in range(2, 62, 3):
            x = (lev + 0.5) / 64.0 * (SAT - BLACK[q]) / WHITE[q]
            sigma2 = (alpha * x + beta) * WHITE[q] ** 2 + 1.0 / 12.0
            _fill(h, s, c, q, lev, sigma2, 400 + 37 * lev, rng)
        _fill(h, s, c, q, 63, 50.0, 150, rng)                 # below minBlocks: takes no part
    rc, a, b, st, n = _fit_c(h, s, c)
    ra, rb, rst, rn = fit_rule(h, s, c)
    assert rc == 0 and (st, n) == (rst, rn) == (0, 80)
    assert _close(a, ra) and _close(b, rb)
    assert abs(a / alpha - 1) < 0.05                          # and it is the model the histograms were drawn from
    # minBlocks is honoured
    rc, a2, b2, st2, n2 = _fit_c(h, s, c, min_blocks=100)
    r2 = fit_rule(h, s, c, min_blocks=100)
    assert rc == 0 and (st2, n2) == (r2[2], r2[3]) == (0, 84) and _close(a2, r2[0]) and _close(b2, r2[1])


def test_fit_status_2_unmeasurable():
    rng = np.random.default_rng(8)
    h, s, c = _tables()
    assert _fit_c(h, s, c)[3:] == (2, 0) and fit_rule(h, s, c)[2:] == (2, 0)          # nothing at all
    for lev in (10, 30, 50):
        _fill(h, s, c, 0, lev, 40.0, 500, rng)
    assert _fit_c(h, s, c)[3:] == (2, 3) and fit_rule(h, s, c)[2:] == (2, 3)          # three points
    h, s, c = _tables()
    for q in range(4):
        for lev in (20, 21, 22, 23):
            _fill(h, s, c, q, lev, 40.0, 500, rng)
    rc, a, b, st, n = _fit_c(h, s, c)                                                  # 16 points over 3/64 of the range
    assert (rc, a, b, st, n) == (0, 0.0, 0.0, 2, 16) and fit_rule(h, s, c) == (0.0, 0.0, 2, 16)


def test_fit_status_3_and_the_beta_clamp():
    rng = np.random.default_rng(9)
    h, s, c = _tables()
    for q in range(4):
        for lev in range(4, 60, 4):
            _fill(h, s, c, q, lev, 400.0 - 5.0 * lev, 600, rng)      # variance falls with the level
    rc, a, b, st, n = _fit_c(h, s, c)
    ra, rb, rst, rn = fit_rule(h, s, c)
    assert rc == 0 and st == rst == 3 and n == rn and a <= 0.0 and _close(a, ra) and _close(b, rb) and b > 0.0
    # a line through a negative intercept: beta clamped to 0, alpha refitted through the origin
    h, s, c = _tables()
    for q in range(4):
        for lev in range(16, 60, 4):
            x = (lev + 0.5) / 64.0 * (SAT - BLACK[q]) / WHITE[q]
            _fill(h, s, c, q, lev, (2e-3 * x - 4e-4) * WHITE[q] ** 2 + 1.0 / 12.0, 600, rng)
    rc, a, b, st, n = _fit_c(h, s, c)
    ra, rb, rst, rn = fit_rule(h, s, c)
    assert rc == 0 and st == rst == 0 and b == rb == 0.0 and _close(a, ra) and 0.0 < a < 2e-3


def test_chi_square_constant():
    """A histogram filled from exact chi-square(8) quantiles returns the variance it was built from: D = 2 sigma^2 Q(u) for u
    evenly spaced in (0, 1).  Quantiles by bisection of the closed-form CDF of an even number of degrees of freedom."""
    import math

    def cdf(x):            # chi-square, 8 degrees of freedom
        t = x / 2.0
        return 1.0 - math.exp(-t) * (1.0 + t + t * t / 2.0 + t * t * t / 6.0)

    def quantile(u):
        lo, hi = 0.0, 200.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if cdf(mid) < u else (lo, mid)
        return 0.5 * (lo + hi)

    assert abs(2.0 * quantile(0.5) - CHI2_8_MEDIAN_X2) < 1e-4
    n = 20000
    qs = np.array([quantile((i + 0.5) / n) for i in range(0, n, 20)])     # 1000 quantiles, each standing for 20 blocks
    levs = (8, 24, 40, 56)
    for base in (3.0, 47.0, 900.0, 22000.0):
        h, s, c = _tables()
        for q in range(4):
            for lev in levs:
                D = np.floor(2.0 * base * (1.0 + lev / 32.0) * qs).astype(np.int64)    # variance rising with the level
                np.add.at(h[q][lev], var_bin(D), 20)
                c[q][lev] = n
                s[q][lev] = n * (16 * BLACK[q] + (lev * 16 * (SAT - BLACK[q]) + 8 * (SAT - BLACK[q])) // 64)
        rc, a, b, st, npts = _fit_c(h, s, c)
        ra, rb, _, _ = fit_rule(h, s, c)
        assert rc == 0 and st == 0 and npts == 16 and _close(a, ra) and _close(b, rb)
        for lev in levs:
            x = (s[0][lev] / (16.0 * n) - BLACK[0]) / WHITE[0]
            got = (a * x + b) * WHITE[0] ** 2 + 1.0 / 12.0
            want = base * (1.0 + lev / 32.0)
            assert abs(got / want - 1) < 0.02, (want, got)    # the 1/8-octave bins, interpolated linearly


def test_var_bins_tile_the_range():
    assert bin_bounds(0) == (0, 1) and bin_bounds(15) == (15, 16) and bin_bounds(16) == (16, 18) and bin_bounds(271)[1] == 1 << 36
    for v in range(NV - 1):
        assert bin_bounds(v)[1] == bin_bounds(v + 1)[0]
    edges = np.array([bin_bounds(v)[0] for v in range(NV)], dtype=np.int64)
    assert np.array_equal(var_bin(edges), np.arange(NV))
    assert np.array_equal(var_bin(edges[1:] - 1), np.arange(NV - 1))
    assert int(var_bin(np.array([8 * 65535 ** 2]))[0]) <= 271


def test_noise_defaults():
    from multi_frame_super_resolution_amd.pipeline import default_config, noise_defaults
    from multi_frame_super_resolution_amd import capi
    cfg = default_config(512, 384, 8, 2, False)
    d = noise_defaults(cfg)
    assert d.black == BLACK and d.white == WHITE and d.sat == SAT and d.min_blocks == MIN_BLOCKS and d.rect == (1, 1, 63, 47)
    black, white, rect = I4(), F4(), I4()
    sat, mb = ctypes.c_int32(), ctypes.c_int32()
    assert capi.lib().raw["mfsr_noise_defaults"](ctypes.byref(cfg), black, white, ctypes.byref(sat), ctypes.byref(mb), rect) == 0
    assert (tuple(black), tuple(white), sat.value, mb.value, tuple(rect)) == (d.black, d.white, d.sat, d.min_blocks, d.rect)
    cfg = default_config(250, 130, 3, 2, True)
    assert noise_defaults(cfg).rect == (1, 1, 30, 15)
    assert capi.lib().raw["mfsr_noise_defaults"](None, None, None, None, None, None) == -1


def test_chart_burst():
    from multi_frame_super_resolution_amd.synth import make_chart_burst
    a = make_chart_burst(512, 384, 2, 1e-4, 1e-6, seed=5)
    b = make_chart_burst(512, 384, 2, 1e-4, 1e-6, seed=5)
    assert len(a) == 2 and a[0].shape == (384, 512) and all((x == y).all() for x, y in zip(a, b))
    assert not (a[0] == a[1]).all()                                   # fresh noise per frame, no motion
    flat = make_chart_burst(512, 384, 1, 0.0, 0.0, seed=5)[0].numpy().astype(np.float64)
    patches = flat.reshape(6, 64, 8, 64)
    assert (patches.max(axis=(1, 3)) == patches.min(axis=(1, 3))).all()       # 48 flat patches
    levels = np.sort((patches[:, 0, :, 0].ravel() - 256.0) / 3839.0)
    assert np.allclose(levels, np.linspace(0.05, 0.95, 48), atol=1.0 / 3839.0)
    m = make_chart_burst(250, 130, 1, 1e-4, 1e-6, mono=True)[0]
    assert m.shape == (130, 250)


def test_restatement_recovers_the_chart_and_fails_on_texture():
    """The documented reach of the rule, on the CPU restatement: the chart fixtures of the GPU test are recovered (their error
    is what the GPU test's bound is made of: printed here), the textured make_burst scene is not (section 2.15, limits)."""
    from multi_frame_super_resolution_amd.synth import make_burst
    for alpha, beta in CHART_MODELS:
        a, b, st, n = calibrate_rule(chart(alpha, beta))
        err = abs(a / alpha - 1)
        print(f"chart alpha {alpha:g} beta {beta:g}: estimated {a:.6g} {b:.6g} status {st} points {n} error {err:.4f} "
              f"bound {recovery_bound(err):.4f}")
        assert st == 0 and err < 0.10 and 0.0 <= b <= a * 0.05 + 4 * beta
    frames, _, _ = make_burst(512, 384, 4)
    a, b, st, n = calibrate_rule([f.numpy().view(np.uint16) for f in frames])
    print(f"textured scene: estimated {a:.6g} {b:.6g} status {st} points {n}")
    assert st != 0 or b > 100 * 1e-6


def test_the_package_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "multi_frame_super_resolution_amd")
    for name in ("pipeline.py", "synth.py", "capi.py", os.path.join("csrc", "noise.hip")):
        txt = open(os.path.join(pkg, name)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M) and "libmfsr_oracle" not in txt, name
