"""HIP kernels directly against the reference's own kernels (oracle/_ref/libmfsr_ref.so: the reference's .cu files compiled
for the host, see tests/test_reference_pin_cpu.py), closing the chain reference -> oracle -> HIP on the device.  The library
is built where the reference's sources are and travels as a file; nothing here reads those sources.  Tolerances are the
ones tests/test_parity_kernels.py states for the same kernels against the oracle."""
import numpy as np
import pytest

from tests.kernels import F3, Tex, load_ref_or_skip, pitch_of
from tests.test_parity_kernels import PATTERNS, _accum_inputs, _kernel_field, _paraboloid, assert_bitexact, rng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return load_ref_or_skip()


@pytest.mark.parametrize("pat", list(PATTERNS))
def test_deBayer_green_redblue_vs_reference(ref, hip, pat):
    H, W = 40, 72
    ref.set_cfa(PATTERNS[pat])
    hip.set_cfa(PATTERNS[pat])
    bp = F3([256, 250, 260])
    sc = F3([1 / 3839.0, 1 / 3800.0, 1 / 3850.0])
    raw16 = rng(2).integers(200, 4096, (H, W), dtype=np.uint16)
    outs = []
    for k in (ref, hip):
        rawf = raw16.astype(np.float32)
        out = np.zeros((H, W, 3), np.float32)
        k.call("deBayerGreenKernel", W, H, rawf, pitch_of(rawf), out, pitch_of(out), bp, sc)
        g = out.copy()
        k.call("deBayerRedBlueKernel", W, H, rawf, pitch_of(rawf), out, pitch_of(out), bp, sc)
        outs.append((g, out.copy()))
    assert_bitexact(outs[0][0], outs[1][0], "deBayerGreenKernel")       # BIT-EXACT, as against the oracle
    assert_bitexact(outs[0][1], outs[1][1], "deBayerRedBlueKernel")
    assert outs[0][1].max() > 0


def test_findMinimum_vs_reference(ref, hip):
    S = 4
    R = 2 * S + 1
    tcx, tcy = 5, 3
    n = tcx * tcy
    imgs = rng(28).random((n, R, R), dtype=np.float32) * 10
    imgs[0] = _paraboloid(S, 1.3, -0.6)[0]
    imgs[1] = 1.0
    imgs[2] = _paraboloid(S, 4.0, 0.0)[0]
    imgs[3, 2, 2] = imgs[3, 5, 5] = -5.0
    imgs[4] = np.nan
    res = []
    for k in (ref, hip):
        out = np.full((tcy, tcx + 1, 2), 7, np.float32)
        k.call("findMinimum", imgs.copy(), out, pitch_of(out), S, n, tcx, 0.5)
        res.append(out)
    assert_bitexact(res[0], res[1], "findMinimum")                        # BIT-EXACT, as against the oracle
    np.testing.assert_allclose(res[1][0, 0], [1.3, -0.6], atol=0.05)


def test_accumulateSuperResFull_x2_vs_reference(ref, hip):
    """The HIP full-frame kernel at x2 against the reference's centre-crop kernel where the two geometries coincide (the
    region is derived in tests/test_reference_pin_cpu.py::test_accumulateSuperResFull_x2_equals_the_reference_crop_kernel)."""
    W, H = 64, 48
    ref.set_cfa(PATTERNS["GRBG"])
    hip.set_cfa(PATTERNS["GRBG"])
    hip.L.set_accumulate_fast_exp(0)
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    raw, full_i, full_w, mask = _accum_inputs(8, W, H, 2 * W, 2 * H)
    kp = _kernel_field(7, H // 2, W // 2, 4)
    sh = rng(8).uniform(-4, 4, (H // 2, W // 2, 2)).astype(np.float32)
    y0, x0 = H // 2, W // 2
    ci = np.ascontiguousarray(full_i[y0:y0 + H, x0:x0 + W])
    cw = np.ascontiguousarray(full_w[y0:y0 + H, x0:x0 + W])
    ref.call("accumulateImagesSuperRes", raw, ci, cw, mask, Tex(kp), Tex(sh), white, black, W, H, pitch_of(ci), pitch_of(mask))
    hi, hw_ = full_i.copy(), full_w.copy()
    hip.call("accumulateSuperResFull", raw, hi, hw_, mask, Tex(kp), Tex(sh), white, black, W, H, 2, pitch_of(hi), pitch_of(mask))
    hip.L.set_accumulate_fast_exp(1)
    smax = int(np.ceil(2 * np.abs(sh).max())) + 1

    def valid(n):
        X = np.arange(n) + n // 2
        lo, hi_ = 2 * (n // 4), 2 * (n // 4 + n // 2) - 1
        return (X - 2 - smax >= lo) & (X + 2 + smax <= hi_) & (np.arange(n) >= 1) & (np.arange(n) < n - 1)

    keep = valid(H)[:, None] & valid(W)[None, :]
    assert keep.mean() > 0.25
    # the tolerance of test_accumulateSuperResFull (exp: ocml vs glibc, 25 taps of O(1) values)
    np.testing.assert_allclose(hi[y0:y0 + H, x0:x0 + W][keep], ci[keep], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(hw_[y0:y0 + H, x0:x0 + W][keep], cw[keep], rtol=2e-6, atol=2e-6)
    assert np.abs(cw[keep] - full_w[y0:y0 + H, x0:x0 + W][keep]).max() > 0.5


def test_ComputeRobustnessMask_vs_reference(ref, hip):
    H, W = 36, 52
    r = rng(60)
    refimg = r.random((H, W, 3), dtype=np.float32)
    mov = np.clip(refimg + r.normal(0, 0.02, refimg.shape).astype(np.float32), 0, 1).astype(np.float32)
    mov[5:9, 5:9] += 0.5
    uv = r.uniform(-5, 5, (H, W, 2)).astype(np.float32)
    res = []
    for k in (ref, hip):
        m = np.zeros((H, W, 4), np.float32)
        k.call("ComputeRobustnessMask", refimg, mov, m, Tex(uv), W, H, pitch_of(refimg), pitch_of(m), 1e-4, 1e-6, 0.8)
        res.append(m)
    # expf: ocml vs glibc (<= 2 ulp of an O(1) value), the tolerance of test_ComputeRobustnessMask
    np.testing.assert_allclose(res[1], res[0], atol=1e-6, rtol=1e-6)
    assert res[1][..., :3].max() > 0.5 and res[1][..., :3].min() == 0.0
