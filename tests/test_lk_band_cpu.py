"""Host-side contracts of the Lucas-Kanade sweep (no GPU): the band rule behind mfsr_lucasKanadeSweepBand, the exact-division
table of mfsr_exactDivisionOk, and what tests/test_lk_sweep_gpu.py decides from the oracle alone (its inputs' conditioning)."""
import os
import time

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi

# (width, height, halfWindowSize, nFrames) -> band rows.  Evaluated from the launcher's expression as it stood BEFORE the rule
# became a function of its own (restated in band_rule below), not from the new function: the refactoring must not move a band.
BAND_TABLE = {
    (1920, 1080, 3, 4): 26,
    (1920, 1080, 3, 1): 8,
    (118, 4611, 3, 4): 10,
    (118, 4611, 3, 1): 8,
    (100, 2738, 7, 4): 9,
    (100, 2738, 7, 1): 8,
    (64, 8200, 1, 4): 9,
    (64, 8200, 1, 1): 8,
    (130, 2731, 5, 4): 9,
    (64, 32769, 7, 4): 32,      # b = 65 > 64: falls through to the first rule
    (64, 32769, 7, 1): 17,
    (63, 100, 3, 1): 0,         # refused geometries
    (64, 9, 3, 1): 0,
    (64, 100, 0, 1): 0,
    (64, 100, 8, 1): 0,
}


def band_rule(width, height, h, n):
    """The launcher's band computation as mfsr_lucasKanadeSweepBatch had it inline, in Python integers."""
    if not (1 <= n <= 4) or not (1 <= h <= 7) or width < 64 or height < 2 * (h + 2):
        return 0
    strips = -(-width // (64 - 2 * (h + 2)))
    band = height * strips * n // 8192
    band = (band + 4) & ~7
    band = min(max(band, 8), 32)
    max_bands = 1024 * [0, 8, 7, 6, 5, 4, 4, 4][h] // (strips * n)
    if max_bands >= 1:
        b = max(-(-height // max_bands), 8)
        if b <= 64:
            band = b
    return band


def _no_override():
    if os.environ.get("MFSR_LK_BAND"):
        pytest.fail("MFSR_LK_BAND is set: the band rule is overridden, its values cannot be checked")


def test_band_rule_values():
    _no_override()
    L = capi.lib()
    for (w, h, hw, n), band in BAND_TABLE.items():
        assert band_rule(w, h, hw, n) == band, (w, h, hw, n)
        got = L.lucasKanadeSweepBand(w, h, hw, n)        # through the wrapper: an int that is no status code
        assert got == band, f"mfsr_lucasKanadeSweepBand({w}, {h}, {hw}, {n}) = {got}, the rule gives {band}"
    for n in (0, 5, -1):
        assert L.lucasKanadeSweepBand(1920, 1080, 3, n) == 0


def test_band_rule_everywhere_the_restatement_goes():
    """The exported function against the restatement over a grid that crosses every branch: both rules, the 8 / 32 / 64 clamps,
    the minimum height of every half window, one to four frames."""
    _no_override()
    raw = capi.lib().raw["mfsr_lucasKanadeSweepBand"]
    seen = set()
    for hw in range(0, 9):
        for w in (63, 64, 65, 100, 640, 1920, 7680):
            for h in (2 * (hw + 2) - 1, 2 * (hw + 2), 41, 1080, 4611, 8200, 32769, 70000):
                for n in (1, 2, 3, 4):
                    want = band_rule(w, h, hw, n)
                    assert raw(w, h, hw, n) == want, (w, h, hw, n)
                    seen.add(want)
    assert {0, 8, 9, 17, 26, 32, 64} <= seen


def test_exactDivisionOk_is_wrapped_as_a_value():
    L = capi.lib()
    assert L.exactDivisionOk(1920.0) == 1        # (used to raise MfsrError(rc = 1) for exactly the divisors that pass)
    assert L.exactDivisionOk(0.0) == 0


def test_exact_division_table_keeps_every_divisor():
    """Forty distinct divisors, asked twice: the whole second pass takes less time than the fastest single first-time proof of
    the first pass (a 2^23-step loop against a table lookup), and gives the same answers."""
    raw = capi.lib().raw["mfsr_exactDivisionOk"]
    divisors = [float(10007 + 2 * i) for i in range(40)]      # (not image sizes another test of this process has asked for)
    first, t_first = [], []
    for d in divisors:
        t0 = time.perf_counter()
        first.append(raw(d))
        t_first.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    second = [raw(d) for d in divisors]
    t_second = time.perf_counter() - t0
    assert second == first and set(first) <= {0, 1}
    assert t_second < min(t_first), f"second pass {t_second * 1e3:.3f} ms, fastest first-time proof {min(t_first) * 1e3:.3f} ms"


# ---------------------------------------------------------------- the references of tests/test_lk_sweep_gpu.py
def test_warp_own_flow_is_the_oracles_warp_where_that_fetches_a_pixels_own_flow(orc):
    """The numpy restatement the sweep's planes are bit-compared with equals the oracle's WarpingKernel bit for bit at every
    pixel outside the few rows and columns whose texel centre does not round-trip (where the oracle blends a neighbour's flow in),
    for converging flows, for flows of +-3 image sizes and at a height of thousands of rows; at those rows and columns the two are
    as close as one ulp of the index times a neighbour's flow allows."""
    from tests import test_lk_sweep_gpu as S
    from tests.test_parity_kernels import assert_bitexact
    seen = 0
    for case, k in [(S.half_window_case(hw), 0) for hw in (1, 4, 7)] + [(S.hostile_case(), S.HOSTILE_FRAME), (S.LkCase(3, 118, 4611, 1, 44), 0)]:
        flow = S.oracle_chain(orc, case, k, 1)[0]
        want, got = S.oracle_warp(orc, case, k, flow), S.warp_own_flow(case.movs[k], flow)
        fetched = S.fetch_is_inexact(case.H)[:, None] | S.fetch_is_inexact(case.W)[None, :]
        assert 0 < fetched.mean() < 0.5
        assert_bitexact(want[~fetched], got[~fetched], f"{case.W}x{case.H}")
        off = want.view(np.uint32) != got.view(np.uint32)
        seen += int(off.sum())
        print(f"{case.W}x{case.H} h={case.hw}: the oracle's fetched flow moves {off.sum()} of {fetched.sum()} candidate pixels, by at most "
              f"{np.abs(want - got).max():.2e}")
        if np.abs(flow).max() < 8:
            # the fetch is at most one ulp of the index off the centre: that share of a neighbour's flow, times the image's slope
            assert np.abs(want - got).max() <= 2.0 ** -23 * max(case.W, case.H) * 4.0
    assert seen > 0


def test_minimum_geometry_seeds_exist(orc):
    """What test_lk_sweep_gpu.py::test_minimum_geometry and test_kernel_edges_gpu.py::c_lkSweep rely on, from the oracle alone: at
    every shape a seed at which the oracle's own float32 error stays under half the tolerance of one iteration."""
    from tests import test_kernel_edges_gpu as edges
    from tests import test_lk_sweep_gpu as S
    for hw in (1, 3, 7):
        for H in (2 * (hw + 2), 2 * (hw + 2) + 1):
            for nf in (1, 4):
                S.conditioned_case(orc, hw, 64, H, nf, 31 + H)
    for w, h in edges.LKS:
        S.conditioned_case(orc, 3, w, h, 4, 90 + w)       # (a frame's inputs do not depend on how many follow it)


# ---------------------------------------------------------------- the inputs of tests/test_lk_sweep_gpu.py
def test_sweep_inputs_are_well_conditioned(orc):
    """flow_difference_report's well_fraction >= 0.3 is a condition on the input, not on the kernel: at every case of
    tests/test_lk_sweep_gpu.py that asserts it, the ORACLE's flow against itself already classifies that many windows as well
    conditioned and converged (the classification uses the reference image and the oracle's flow only), and the oracle has
    converged on the true shift."""
    from tests import test_lk_sweep_gpu as S
    from tests.burst_compare import flow_difference_report
    cases = [(S.half_window_case(hw), None) for hw in range(1, 8)] + [(S.hostile_case(), [S.HOSTILE_FRAME])]
    for case, frames in cases:
        for k in (range(case.nf) if frames is None else frames):
            want = S.oracle_chain(orc, case, k, 3)[-1]
            rep = flow_difference_report(want, want, case.ref, case.hw, thr=5e-4)
            err = S.distance_to_true(case, k, want)
            print(f"h={case.hw} {case.W}x{case.H} frame {k}: well fraction {rep['well_fraction']:.2f}, oracle's mean distance to the true shift {err:.3f}")
            assert rep["well_fraction"] >= 0.3, (case.hw, case.W, case.H, k)
            assert err < 0.2, (case.hw, case.W, case.H, k)
