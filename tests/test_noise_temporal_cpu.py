"""Burst noise calibration, the part that needs no GPU: the prototypes, the host-side refusals of the
C-ABI, mfsr_noise_fit_temporal against the numpy restatement (tests/noise_temporal_ref.py) and against mfsr_noise_fit, and the
point of the feature on the CPU restatement: with the true shifts as flows, and with the CPU oracle's flow fields, the noise model
of a textured burst is recovered where the single-frame rule of section 2.15 is not."""
import ctypes
import functools

import numpy as np
import pytest

from tests.noise_temporal_ref import (DEFAULT_TOL, accepted_pairs, calibrate_temporal_rule, fit_temporal_rule, roundf, shifts_as_flows,
                                      stats_temporal_rule)
from tests.test_noise_cpu import (BLACK, MIN_BLOCKS, SAT, WHITE, _close, _fill, _fit_c, _tables, calibrate_rule, default_rect, fit_rule,
                                  full_rect)

I4 = ctypes.c_int32 * 4
F4 = ctypes.c_float * 4

# the fixtures of the driver tests (tests/test_noise_temporal_gpu.py): synth.make_burst(512, 384, 16) with its default seeds
# (shift_seed None), drawn with these noise models
BURST = dict(width=512, height=384, frames=16)
MODELS = ((1e-4, 1e-6), (1.6e-3, 1.6e-5))
# even-pixel shifts (LR pixels): every pair of frames is a whole number of quads apart
CRAFTED_SHIFTS = ((0, 0), (2, 0), (0, 2), (-2, 2), (4, -2), (-4, -4), (2, 4))
# quad phases (k / 8, 3k / 8 mod 1), k = 0 .. 7: no two frames within 1/16 quad of a whole number of quads on both axes
UNMATCHED_SHIFTS = tuple((k / 4.0, ((3 * k) % 8) / 4.0) for k in range(8))


def burst(alpha, beta, shifts=None, frames=None):
    """(u16 frames, shifts [N, 2]) of the fixture burst."""
    import torch
    from multi_frame_super_resolution_amd.synth import make_burst
    n = BURST["frames"] if shifts is None else len(shifts)
    n = n if frames is None else frames
    kw = {} if shifts is None else dict(shifts=torch.tensor(shifts, dtype=torch.float32))
    fr, sh, _ = make_burst(BURST["width"], BURST["height"], n, alpha=alpha, beta=beta, **kw)
    return [f.numpy().view(np.uint16) for f in fr], sh.numpy()


@functools.lru_cache(maxsize=None)
def oracle_flows(alpha, beta):
    """(frames, flows) of the fixture burst aligned by the CPU oracle to frame 0 (None for the reference)."""
    from multi_frame_super_resolution_amd.pipeline import default_config
    from oracle.pipeline import OraclePipeline
    fr, _ = burst(alpha, beta)
    op = OraclePipeline(default_config(BURST["width"], BURST["height"], BURST["frames"], 2, False))
    op.set_reference(fr[0])
    img = np.zeros((op.hrH, op.hrW, 3), np.float32)
    tw = np.zeros_like(img)
    flows = [None]
    for f in fr[1:]:
        op.add_frame(f, False, img, tw)
        flows.append(op.flow.copy())
    return fr, flows


@functools.lru_cache(maxsize=None)
def oracle_recovery(alpha, beta):
    """(alpha, beta, status, points, blocks, accepted pairs, relative error of alpha) of the restatement on the oracle's flows."""
    fr, flows = oracle_flows(alpha, beta)
    res = calibrate_temporal_rule(fr, flows)
    acc = accepted_pairs(flows, default_rect(BURST["width"], BURST["height"]), BURST["width"], BURST["height"])
    return res + (acc, abs(res[0] / alpha - 1))


def alpha_bound(err):
    """The bound of the GPU driver tests on |alpha_est / alpha - 1|: three times the error of the restatement on the CPU oracle's
    flows (the convention of recovery_bound in tests/test_noise_cpu.py), at least 5 %: the accepted set can change when a flow
    moves by 1e-5 px across tol."""
    return max(3.0 * err, 0.05)


# ---- the C-ABI ------------------------------------------------------------------------------------------------------------
def test_abi_prototypes_parse():
    from multi_frame_super_resolution_amd import capi
    protos = capi.parse_header()
    for name in ("mfsr_noiseStatsTemporal", "mfsr_noise_fit_temporal", "mfsr_burst_calibrate_noise_temporal"):
        assert name in protos, name
        assert protos[name][0] == "int"
    assert protos["mfsr_noise_temporal_scratch_bytes"][0] == "size_t"
    assert [t for t, _ in protos["mfsr_noiseStatsTemporal"][1]] == [
        "int", "const uint16_t*const*", "int", "int", "int", "const mfsr_float2*const*", "int", "int", "int", "const int32_t*", "int",
        "const int32_t*", "float", "uint32_t*", "long long*", "long long*", "mfsr_stream_t"]
    assert [t for t, _ in protos["mfsr_noise_fit_temporal"][1]] == [t for t, _ in protos["mfsr_noise_fit"][1]]
    L = capi.lib()                     # resolves every declared symbol
    for name in ("mfsr_noiseStatsTemporal", "mfsr_noise_fit_temporal", "mfsr_burst_calibrate_noise_temporal",
                 "mfsr_noise_temporal_scratch_bytes"):
        assert name in L.raw


def test_stats_refusals_happen_on_the_host():
    """Every bad argument is MFSR_E_INVALID (-1) before any device call: the frame and flow pointers are host memory (or nothing at
    all), so a call that got as far as the device would fail with another code, or crash."""
    from multi_frame_super_resolution_amd import capi
    f = capi.lib().raw["mfsr_noiseStatsTemporal"]
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    out = ctypes.create_string_buffer(16)
    o = (ctypes.addressof(out) + 7) // 8 * 8

    def call(n=2, ptrs=None, pitch=128, w=64, h=64, flows=None, fpitch=None, fw=32, fh=32, black=BLACK, sat=SAT, rect=(0, 0, 8, 8),
             tol=0.0625, hist=o, ls=o, cnt=o):
        m = max(n, 1)
        p = (ctypes.c_void_p * m)(*([base] * m)) if ptrs is None else ptrs
        fl = (ctypes.c_void_p * m)(*([base] * m)) if flows is None else flows
        return f(n, p, pitch, w, h, fl, 8 * fw if fpitch is None else fpitch, fw, fh, I4(*black), sat, I4(*rect), tol, hist, ls, cnt,
                 None)

    assert call(n=1) == -1 and call(n=0) == -1 and call(n=65) == -1 and call(n=-1) == -1          # frame count
    assert call(w=63) == -1 and call(h=63) == -1 and call(w=0) == -1                                # even sizes
    assert call(pitch=126) == -1 and call(pitch=129) == -1
    assert call(fw=31) == -1 and call(fh=64) == -1 and call(fw=64, fh=32) == -1 and call(fw=16, fh=16) == -1   # flow size
    assert call(fw=0, fh=0) == -1 and call(fw=33, fh=32) == -1
    assert call(fpitch=248) == -1 and call(fpitch=260) == -1                                        # flow rows
    assert call(flows=(ctypes.c_void_p * 2)(base, base + 4)) == -1                                  # flow alignment
    assert call(tol=-0.001) == -1 and call(tol=0.2501) == -1 and call(tol=float("nan")) == -1 and call(tol=float("inf")) == -1
    assert call(sat=0) == -1 and call(sat=65536) == -1 and call(sat=-5) == -1                       # sat range
    assert call(black=(256, 256, 256, 4095)) == -1 and call(black=(-1, 0, 0, 0)) == -1
    assert call(rect=(2, 2, 2, 5)) == -1 and call(rect=(2, 5, 4, 5)) == -1 and call(rect=(4, 0, 2, 8)) == -1   # empty
    assert call(rect=(0, 0, 9, 8)) == -1 and call(rect=(0, 0, 8, 9)) == -1 and call(rect=(-1, 0, 8, 8)) == -1  # outside
    assert call(w=70, h=70, pitch=140, fw=35, fh=35, rect=(0, 0, 9, 8)) == -1      # the partial edge block is not in the grid
    assert call(hist=None) == -1 and call(ls=None) == -1 and call(cnt=None) == -1
    assert call(ptrs=(ctypes.c_void_p * 2)(base, None)) == -1 and call(ptrs=(ctypes.c_void_p * 2)(base, base + 1)) == -1
    assert f(2, None, 128, 64, 64, (ctypes.c_void_p * 2)(), 256, 32, 32, I4(*BLACK), SAT, I4(0, 0, 8, 8), 0.0625, o, o, o, None) == -1
    assert f(2, (ctypes.c_void_p * 2)(base, base), 128, 64, 64, None, 256, 32, 32, I4(*BLACK), SAT, I4(0, 0, 8, 8), 0.0625, o, o, o,
             None) == -1
    # pairs * blocks >= 2^31: 64 frames are 2016 pairs, 1100 x 1000 blocks (the same launch with 3 frames is refused further on
    # only because its tables are no device memory: the bound is what stops this one)
    assert 2016 * 1100 * 1000 >= 1 << 31
    assert call(n=64, w=8800, h=8000, pitch=17600, fw=4400, fh=4000, rect=(0, 0, 1100, 1000)) == -1
    g = capi.lib().raw["mfsr_burst_calibrate_noise_temporal"]
    assert g(None, 2, None, 0, 0.0, 0, None, 0, None, None, None, None, None, None) == -1


def test_scratch_bytes():
    """mfsr_noise_temporal_scratch_bytes is host arithmetic: the tables, n - 1 flow fields and one mask, each rounded up to 256
    bytes; 0 for a frame count outside 2 .. 64 or an invalid config.  (The driver's refusal of a smaller scratch needs a burst
    handle, so it is in tests/test_noise_temporal_gpu.py.)"""
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import default_config
    f = capi.lib().raw["mfsr_noise_temporal_scratch_bytes"]

    def up(v):
        return (v + 255) // 256 * 256

    tables = 4 * 4 * 64 * 272 + 16 * 4 * 64
    cfg = default_config(512, 384, 16, 2, False)
    assert f(ctypes.byref(cfg), 16) == up(tables) + 15 * up(8 * 256 * 192) + up(16 * 256 * 192)
    assert f(ctypes.byref(cfg), 2) == up(tables) + up(8 * 256 * 192) + up(16 * 256 * 192)
    mono = default_config(256, 136, 5, 2, True)
    assert f(ctypes.byref(mono), 5) == up(tables) + 4 * up(8 * 256 * 136) + up(16 * 128 * 68)
    assert f(ctypes.byref(cfg), 1) == 0 and f(ctypes.byref(cfg), 65) == 0 and f(None, 4) == 0
    cfg.width = 30
    assert f(ctypes.byref(cfg), 4) == 0


# ---- the fit ----------------------------------------------------------------------------------------------------------------
def _fit_t(hist, level_sum, count, black=BLACK, white=WHITE, min_blocks=MIN_BLOCKS):
    from multi_frame_super_resolution_amd import capi
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    level_sum = np.ascontiguousarray(level_sum, dtype=np.int64)
    count = np.ascontiguousarray(count, dtype=np.int64)
    a, b = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    st, n = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = capi.lib().raw["mfsr_noise_fit_temporal"](hist.ctypes.data, level_sum.ctypes.data, count.ctypes.data, I4(*black), F4(*white),
                                                   int(min_blocks), ctypes.byref(a), ctypes.byref(b), ctypes.byref(st), ctypes.byref(n))
    return rc, a.value, b.value, st.value, n.value


def _calibrate_both(frames, flows):
    """calibrate_temporal_rule, with mfsr_noise_fit_temporal run on the same tables: (alpha, beta, status, points, blocks) of the
    restatement after the C fit has been held against it."""
    h, w = frames[0].shape
    st = stats_temporal_rule(frames, flows, default_rect(w, h))
    ra, rb, rst, rn = fit_temporal_rule(*st)
    rc, a, b, cst, n = _fit_t(*st)
    assert rc == 0 and (cst, n) == (rst, rn) and _close(a, ra) and _close(b, rb)
    return ra, rb, rst, rn, int(st[2][0].sum())


def _difference_tables(alpha, beta, seed):
    """Histograms of the D of a difference of two frames: per-sample variance sigma2 gives D = 4 sigma2 chi2_8."""
    rng = np.random.default_rng(seed)
    h, s, c = _tables()
    for q in range(4):
        for lev in range(2, 62, 3):
            x = (lev + 0.5) / 64.0 * (SAT - BLACK[q]) / WHITE[q]
            sigma2 = (alpha * x + beta) * WHITE[q] ** 2 + 1.0 / 12.0
            _fill(h, s, c, q, lev, 2.0 * sigma2, 400 + 37 * lev, rng)          # (_fill draws 2 * its variance * chi2_8)
        _fill(h, s, c, q, 63, 50.0, 150, rng)                                  # below minBlocks: takes no part
    return h, s, c


@pytest.mark.parametrize("alpha,beta", [(1e-4, 1e-6), (1.6e-3, 1.6e-5), (5e-4, 0.0)])
def test_fit_equals_the_restatement_on_hand_made_histograms(alpha, beta):
    h, s, c = _difference_tables(alpha, beta, 7)
    rc, a, b, st, n = _fit_t(h, s, c)
    ra, rb, rst, rn = fit_temporal_rule(h, s, c)
    assert rc == 0 and (st, n) == (rst, rn) == (0, 80)
    assert _close(a, ra) and _close(b, rb)
    assert abs(a / alpha - 1) < 0.05                          # and it is the model the histograms were drawn from
    rc, a2, b2, st2, n2 = _fit_t(h, s, c, min_blocks=100)     # minBlocks is honoured
    r2 = fit_temporal_rule(h, s, c, min_blocks=100)
    assert rc == 0 and (st2, n2) == (r2[2], r2[3]) == (0, 84) and _close(a2, r2[0]) and _close(b2, r2[1])


@pytest.mark.parametrize("alpha,beta", [(1e-4, 1e-6), (1.6e-3, 1.6e-5)])
def test_fit_is_the_single_frame_fit_at_half_the_variance(alpha, beta):
    """The exact relation.  On the same tables mfsr_noise_fit takes var = median / 14.6882 and mfsr_noise_fit_temporal
    var_t = median / 29.3764 = var / 2, so with one white level w for all positions, every point above the quantiser's floor
    (var_t > 1/12) and no clamp of beta, every y_t = y / 2 - 1 / (24 w^2) at the same x and weight, and the least-squares line
    follows:  alpha_t = alpha / 2,  beta_t = beta / 2 - 1 / (24 w^2).  Asserted to 1e-9 of the larger term."""
    h, s, c = _difference_tables(alpha, beta, 11)
    rc, a, b, st, n = _fit_c(h, s, c)
    rct, at, bt, stt, nt = _fit_t(h, s, c)
    assert rc == rct == 0 and st == stt == 0 and n == nt == 80 and b > 0.0 and bt > 0.0
    shift = 1.0 / (24.0 * WHITE[0] ** 2)
    assert abs(at - a / 2) <= 1e-9 * abs(a / 2)
    assert abs(bt - (b / 2 - shift)) <= 1e-9 * max(b / 2, shift)
    # mfsr_noise_fit itself is the restatement of section 2.15, as before
    ra, rb, _, _ = fit_rule(h, s, c)
    assert _close(a, ra) and _close(b, rb)


def test_fit_refusals_and_status():
    h, s, c = _tables()
    assert _fit_t(h, s, c, min_blocks=0)[0] == -1
    assert _fit_t(h, s, c, white=(3839.0, 0.0, 3839.0, 3839.0))[0] == -1
    assert _fit_t(h, s, c, black=(256, 256, -1, 256))[0] == -1
    from multi_frame_super_resolution_amd import capi
    assert capi.lib().raw["mfsr_noise_fit_temporal"](None, None, None, I4(*BLACK), F4(*WHITE), 200, None, None, None, None) == -1
    assert _fit_t(h, s, c)[1:] == (0.0, 0.0, 2, 0) and fit_temporal_rule(h, s, c) == (0.0, 0.0, 2, 0)     # nothing at all


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def test_restatement_on_two_shifted_copies():
    """Known answers of the restatement (and its roundf): frame 1 is frame 0 moved by whole quads plus a constant, so every accepted block has D = 0 and the level sums
    are those of frame 0's blocks; a half-quad shift is never accepted; saturation in A or in B drops the block."""
    x = np.array([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997, -0.49999997, 8388607.5, 0.0, -0.0, 16384.0], dtype=np.float32)
    assert roundf(x).tolist() == [1, -1, 2, 3, -3, 0, 0, 8388608, 0, 0, 16384]          # C's roundf, not numpy's half-to-even
    rng = np.random.default_rng(3)
    a = rng.integers(300, 3000, (48, 64)).astype(np.uint16)
    b = np.roll(a, (4, -6), axis=(0, 1)) + 7                      # frame 1 shows pixel p of frame 0 at p + (-6, 4): 3 and 2 quads
    flow = np.zeros((24, 32, 2), dtype=np.float32)
    flow[..., 0], flow[..., 1] = -6.0, 4.0
    hist, ls, cnt = stats_temporal_rule([a, b.astype(np.uint16)], [None, flow], full_rect(64, 48))
    # B = A's origin + (-6, 4) must stay inside: bx >= 1, by <= 4 of the 8 x 6 grid -> 7 x 5 blocks, none wrapped by the roll
    assert int(cnt[0].sum()) == 35 and all(int(hist[q][:, 0].sum()) == 35 for q in range(4)) and int(hist[:, :, 1:].sum()) == 0
    want = sum(int(a[8 * by:8 * by + 8:2, 8 * bx:8 * bx + 8:2].sum()) for by in range(5) for bx in range(1, 8))
    assert int(ls[0].sum()) == want
    assert _fit_t(hist, ls, cnt, min_blocks=1)[3:] == fit_temporal_rule(hist, ls, cnt, min_blocks=1)[2:]    # and the fit reads them alike
    flow[..., 0] = -5.0                                           # 2.5 quads: a tie of roundf, r = 0.5
    assert int(stats_temporal_rule([a, b.astype(np.uint16)], [None, flow], full_rect(64, 48), tol=0.25)[2].sum()) == 0
    flow[..., 0] = -6.0
    a2 = a.copy()
    a2[8, 16] = SAT                                               # block (2, 1) of A
    b2 = b.astype(np.uint16).copy()
    b2[4, 2] = SAT                                                # B of block (1, 0): origin (8 - 6, 0 + 4)
    assert int(stats_temporal_rule([a2, b2], [None, flow], full_rect(64, 48))[2][0].sum()) == 33


# ---- the point of the feature ---------------------------------------------------------------------------------------------------
def test_true_shifts_recover_the_model_where_the_single_frame_rule_fails():
    """make_burst(512, 384, 16) with its true shifts as flows: two pairs of frames happen to be phase-matched at tol = 1/16, and
    alpha comes out within 3 x the 2.8 % measured when the rule was proposed, while the single-frame rule on the same frames is
    off by more than a factor of 2 (or reports alpha <= 0).  beta obeys the bound of section 2.15."""
    alpha, beta = MODELS[0]
    fr, shifts = burst(alpha, beta)
    flows = shifts_as_flows(shifts, BURST["width"], BURST["height"])
    acc = accepted_pairs(flows, default_rect(BURST["width"], BURST["height"]), BURST["width"], BURST["height"])
    a, b, st, n, blocks = _calibrate_both(fr, flows)
    print(f"make_burst, true shifts: pairs {sorted(acc)} alpha {a:.6g} beta {b:.6g} status {st} points {n} terms {blocks} "
          f"error {abs(a / alpha - 1):.4f}")
    assert sorted(acc) == [(0, 1), (4, 13)] and st == 0
    assert abs(a / alpha - 1) <= 3 * 0.028
    assert 0.0 <= b <= 0.05 * alpha + 4 * beta
    sa, sb, sst, _ = calibrate_rule(fr)
    print(f"single-frame rule: alpha {sa:.6g} beta {sb:.6g} status {sst}")
    assert sst != 0 or not (alpha / 2 <= sa <= 2 * alpha)


def test_crafted_shifts_recover_the_model():
    """Even-pixel shifts: all 21 pairs of the 7 frames are phase-matched everywhere, and alpha comes out within 3 x the 0.6 %
    measured when the rule was proposed."""
    alpha, beta = MODELS[0]
    fr, shifts = burst(alpha, beta, CRAFTED_SHIFTS)
    assert np.array_equal(shifts, np.array(CRAFTED_SHIFTS, dtype=np.float32))
    flows = shifts_as_flows(shifts, BURST["width"], BURST["height"])
    acc = accepted_pairs(flows, default_rect(BURST["width"], BURST["height"]), BURST["width"], BURST["height"])
    a, b, st, n, blocks = _calibrate_both(fr, flows)
    print(f"crafted shifts: {len(acc)} pairs alpha {a:.6g} beta {b:.6g} status {st} points {n} terms {blocks} "
          f"error {abs(a / alpha - 1):.4f}")
    assert len(acc) == 21 and st == 0
    assert abs(a / alpha - 1) <= 3 * 0.006
    assert 0.0 <= b <= 0.05 * alpha + 4 * beta
    sa, _, sst, _ = calibrate_rule(fr)
    assert sst != 0 or not (alpha / 2 <= sa <= 2 * alpha)


def test_a_burst_without_a_phase_matched_pair_is_status_2():
    alpha, beta = MODELS[0]
    fr, shifts = burst(alpha, beta, UNMATCHED_SHIFTS)
    flows = shifts_as_flows(shifts, BURST["width"], BURST["height"])
    assert accepted_pairs(flows, default_rect(BURST["width"], BURST["height"]), BURST["width"], BURST["height"]) == {}
    assert calibrate_temporal_rule(fr, flows) == _calibrate_both(fr, flows) == (0.0, 0.0, 2, 0, 0)


def test_make_burst_shifts_argument_keeps_every_existing_call():
    import torch
    from multi_frame_super_resolution_amd.synth import make_burst
    a, sa, _ = make_burst(128, 96, 3, seed=9)
    b, sb, _ = make_burst(128, 96, 3, seed=9, shifts=sa)                # the drawn shifts, given back: the same burst
    assert torch.equal(sa, sb) and all(torch.equal(x, y) for x, y in zip(a, b))
    c, sc, _ = make_burst(128, 96, 3, seed=9, shifts=torch.tensor([[0.0, 0.0], [2.0, 0.0], [0.0, -2.0]]))
    assert sc.tolist() == [[0.0, 0.0], [2.0, 0.0], [0.0, -2.0]]
    assert torch.equal(c[0], a[0]) and not torch.equal(c[1], a[1])      # same scene and noise stream, other shifts


@pytest.mark.parametrize("alpha,beta", MODELS)
def test_oracle_flows_recover_the_model(alpha, beta):
    """What the GPU driver's bound is made of: the restatement on the CPU oracle's flow fields of the fixture bursts (printed; the
    figures are recorded in DESIGN.md section 2.22), and the conditions on the fixture: at least 2 accepted pairs and 30 points
    at the defaults."""
    a, b, st, n, blocks, acc, err = oracle_recovery(alpha, beta)
    assert _calibrate_both(*oracle_flows(alpha, beta)) == (a, b, st, n, blocks)
    big = {p: c for p, c in acc.items() if c >= 200}
    print(f"oracle flows, model ({alpha:g}, {beta:g}): alpha {a:.6g} beta {b:.6g} status {st} points {n} terms {blocks} "
          f"error {err:.4f} bound {alpha_bound(err):.4f}; {len(acc)} pairs accepted somewhere, with >= 200 blocks: {big}")
    assert st == 0 and len(acc) >= 2 and n >= 30
    assert alpha_bound(err) < 0.5                                        # the bound stays a bound
