"""Merge-aware denoise inside the finish without a device: the layout of mfsr_denoise against a compiled
probe, the defaults, every bound of mfsr_denoise_validate, the host refusals of the entry points, known answers of the numpy
restatement (tests/denoise_ref.py) that tests/test_denoise_gpu.py compares the kernels with, and the quality condition of the
rule on an oracle burst with scene motion (tools/denoise_quality.py)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi
from tests import denoise_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
f32 = np.float32


def _desc(radius=2, strength=3.0, gain=2.0, alpha=1e-3, beta=1e-5, wLo=0.0, wHi=0.0):
    d = capi.Denoise()
    d.radius, d.strength, d.gain, d.alpha, d.beta, d.wLo, d.wHi = radius, strength, gain, alpha, beta, wLo, wHi
    return d


def test_denoise_struct_mirrors_the_header():
    probe = r'''
    #include <stdio.h>
    #include <stddef.h>
    #include "mfsr.h"
    int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mfsr_denoise), offsetof(mfsr_denoise, radius),
        offsetof(mfsr_denoise, strength), offsetof(mfsr_denoise, gain), offsetof(mfsr_denoise, alpha), offsetof(mfsr_denoise, beta),
        offsetof(mfsr_denoise, wLo), offsetof(mfsr_denoise, wHi), offsetof(mfsr_denoise, reserved)); return 0; }
    '''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(src, "w").write(probe)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = list(map(int, subprocess.check_output([exe], text=True).split()))
    C = capi.Denoise
    assert got == [ctypes.sizeof(C), C.radius.offset, C.strength.offset, C.gain.offset, C.alpha.offset, C.beta.offset, C.wLo.offset,
                   C.wHi.offset, C.reserved.offset]
    assert got == [48, 0, 4, 8, 12, 16, 20, 24, 28]


def test_entry_points_resolve_and_the_tile():
    raw = capi.lib().raw
    for name in ("mfsr_denoise_defaults", "mfsr_denoise_validate", "mfsr_denoise_tile", "mfsr_denoiseImage", "mfsr_finishDenoised",
                 "mfsr_burst_set_denoise", "mfsr_stream_set_denoise", "mfsr_burst_debug_denoised"):
        assert name in raw, name
    tw, th = ctypes.c_int(0), ctypes.c_int(0)
    assert raw["mfsr_denoise_tile"](ctypes.byref(tw), ctypes.byref(th)) == 0
    assert (tw.value, th.value) == (64, 16)
    assert tw.value % 4 == 0                                # an RGB8 lane's four pixels never straddle two tiles
    assert raw["mfsr_denoise_tile"](None, ctypes.byref(th)) == INVALID


def test_defaults():
    raw = capi.lib().raw
    d = capi.Denoise()
    assert raw["mfsr_denoise_defaults"](1.6e-3, 1.6e-5, ctypes.byref(d)) == 0
    assert (d.radius, d.strength, d.gain, d.wLo, d.wHi) == (2, 3.0, 2.0, 0.0, 0.0)
    assert (f32(d.alpha), f32(d.beta)) == (f32(1.6e-3), f32(1.6e-5)) and list(d.reserved) == [0] * 5
    assert raw["mfsr_denoise_validate"](ctypes.byref(d)) == 0
    assert raw["mfsr_denoise_defaults"](1.5, 0.0, ctypes.byref(d)) == INVALID
    assert raw["mfsr_denoise_defaults"](0.0, float("nan"), ctypes.byref(d)) == INVALID
    assert raw["mfsr_denoise_defaults"](0.0, 0.0, None) == INVALID
    from multi_frame_super_resolution_amd.pipeline import denoise_defaults
    assert denoise_defaults(0.25, 0.5).alpha == 0.25 and denoise_defaults().radius == 2
    with pytest.raises(ValueError):
        denoise_defaults(-1.0, 0.0)


GOOD = [
    ("the defaults' shape", dict()),
    ("radius 1", dict(radius=1)), ("radius 3", dict(radius=3)), ("radius 0 = off", dict(radius=0)),
    ("strength 1/16", dict(strength=0.0625)), ("strength 16", dict(strength=16.0)), ("strength 0 = off", dict(strength=0.0)),
    ("gain 1024", dict(gain=1024.0)), ("gain tiny", dict(gain=1e-30)),
    ("alpha = beta = 0", dict(alpha=0.0, beta=0.0)), ("alpha = beta = 1", dict(alpha=1.0, beta=1.0)),
    ("fade of 2^-10", dict(wLo=1.0, wHi=1.0 + 2.0 ** -10)), ("wHi below wLo", dict(wLo=3.0, wHi=1.0)),
    ("negative wHi, no fade", dict(wLo=0.0, wHi=-5.0)), ("a wide fade", dict(wLo=0.0, wHi=3e38)),
]
BAD = [
    ("radius 4", dict(radius=4)), ("radius -1", dict(radius=-1)),
    ("strength below 1/16", dict(strength=0.06)), ("strength above 16", dict(strength=16.5)), ("negative strength", dict(strength=-3.0)),
    ("NaN strength", dict(strength=float("nan"))), ("inf strength", dict(strength=float("inf"))),
    ("gain 0", dict(gain=0.0)), ("negative gain", dict(gain=-2.0)), ("gain above 1024", dict(gain=1025.0)),
    ("NaN gain", dict(gain=float("nan"))), ("inf gain", dict(gain=float("inf"))),
    ("negative alpha", dict(alpha=-1e-6)), ("alpha above 1", dict(alpha=1.001)), ("NaN alpha", dict(alpha=float("nan"))),
    ("negative beta", dict(beta=-1e-6)), ("beta above 1", dict(beta=1.001)), ("inf beta", dict(beta=float("inf"))),
    ("negative wLo", dict(wLo=-0.5, wHi=-1.0)), ("NaN wLo", dict(wLo=float("nan"))), ("inf wHi", dict(wHi=float("inf"))),
    ("NaN wHi", dict(wHi=float("nan"))), ("a fade narrower than 2^-10", dict(wLo=1.0, wHi=1.0 + 2.0 ** -11)),
]


@pytest.mark.parametrize("what,desc", GOOD, ids=[g[0] for g in GOOD])
def test_validate_accepts(what, desc):
    assert capi.lib().raw["mfsr_denoise_validate"](ctypes.byref(_desc(**desc))) == 0, what


@pytest.mark.parametrize("what,desc", BAD, ids=[b[0] for b in BAD])
def test_validate_and_the_entry_points_refuse(what, desc):
    raw = capi.lib().raw
    d = _desc(**desc)
    assert raw["mfsr_denoise_validate"](ctypes.byref(d)) == INVALID, what
    buf = (ctypes.c_float * (3 * 8 * 8 * 2))()
    a = ctypes.addressof(buf)
    # (the pointers are host memory: a call that got as far as the device would not return MFSR_E_INVALID)
    assert raw["mfsr_denoiseImage"](a, 96, None, 0, a + 768, 96, None, 0, 8, 8, ctypes.byref(d), None, 0, None) == INVALID, what
    assert raw["mfsr_finishDenoised"](a, a, 96, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, a + 768, 96, None, 0, None, 8, 8, 1e-3, 0, 0, 0,
                                      8, 8, ctypes.byref(d), 0, 0, None) == INVALID, what


def test_reserved_words_and_host_refusals_of_the_image_entry_points():
    raw = capi.lib().raw
    v = raw["mfsr_denoise_validate"]
    assert v(None) == INVALID
    for i in range(5):
        d = _desc()
        d.reserved[i] = 1
        assert v(ctypes.byref(d)) == INVALID, i
    buf = (ctypes.c_float * (3 * 8 * 8 * 3))()
    a = ctypes.addressof(buf)
    good = _desc()

    def image(in_=a, cnt=None, cnt_rb=0, out_img=a + 768, out=None, w=8, h=8, d=good, render=None, in_rb=96):
        return raw["mfsr_denoiseImage"](in_, in_rb, cnt, cnt_rb, out_img, 96, out, 0, w, h, ctypes.byref(d) if d else None, render, 0, None)

    def finish(out_img=a + 768, d=good, above=0, below=0, render=None, row_offset=0, full_h=8):
        return raw["mfsr_finishDenoised"](a, a, 96, None, 0, 0, 0, 0.0, 1.0, 0.0, 1.0, out_img, 96, None, 0, render, 8, 8, 1e-3, 0, 0,
                                          row_offset, 8, full_h, ctypes.byref(d) if d else None, above, below, None)

    # a description that is off is refused by both; so is none at all
    for off in (_desc(radius=0), _desc(strength=0.0)):
        assert image(d=off) == INVALID and finish(d=off) == INVALID
    assert image(d=None) == INVALID and finish(d=None) == INVALID
    # not in place, neither on the image nor on the count image; no output at all; bad extents and row bytes
    assert image(out_img=a) == INVALID and image(out_img=a + 96) == INVALID
    assert image(cnt=a + 768, cnt_rb=96, out_img=a + 768) == INVALID
    assert image(cnt=a + 1536, cnt_rb=92) == INVALID and image(cnt=a + 1537, cnt_rb=96) == INVALID
    assert image(out_img=None) == INVALID and image(w=0) == INVALID and image(h=-1) == INVALID and image(in_rb=92) == INVALID
    assert image(in_=None) == INVALID
    assert finish(out_img=a) == INVALID and finish(out_img=None) == INVALID
    # the reach must lie inside the whole image
    assert finish(above=1) == INVALID and finish(below=1) == INVALID and finish(above=-1) == INVALID
    # the two-plane formats are refused
    r = capi.Render()
    r.format = capi.OUT_NV12
    assert image(render=ctypes.byref(r)) == INVALID and finish(render=ctypes.byref(r)) == INVALID


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)

    return np.abs(key(a) - key(b))


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_a_constant_image_comes_back_within_2_ulp(radius):
    """every neighbour has d = 0, so g = 1, G = (2R + 1)^2 exactly and S = G s up to the roundings of the 2R + 1 row sums and
    their sum; the quotient lands within 2 ulp of s"""
    for value in (0.0, 1e-3, 0.18, 0.7311, 1.0, 3.3, 65536.0, -0.25):
        p = np.full((9, 11, 3), value, f32) * np.array([1.0, 0.5, 0.3333], f32)
        for n in (None, np.full_like(p, 0.37), np.full_like(p, 9.0)):
            o, G, _ = D.denoise(p, n, radius=radius, strength=3.0, gain=2.0, alpha=1.6e-3, beta=1.6e-5, want_sums=True)
            assert (G == f32((2 * radius + 1) ** 2)).all()
            assert _ulps(o, p).max() <= 2, (value, radius)


def test_lambda_zero_returns_s_bit_for_bit():
    rng = np.random.default_rng(3)
    p = rng.uniform(-0.2, 1.2, (24, 31, 3)).astype(f32)
    p[3, 4] = [np.nan, np.inf, -np.inf]
    p[7, 9] = [1e30, -1e30, -0.0]
    n = rng.uniform(2.0, 9.0, p.shape).astype(f32)            # every count at or above wHi = 2: lambda = 0
    n[5, 5] = [2.0, np.inf, 1e6]
    o = D.denoise(p, n, radius=3, strength=16.0, gain=1024.0, alpha=1.0, beta=1.0, w_lo=1.0, w_hi=2.0)
    assert np.array_equal(o.view(np.uint32), D.clean(p).view(np.uint32))
    # a mixed image: exactly the pixels and channels with n >= wHi keep s, the others move
    n[:, :16] = 1.25
    lam = D.fade(n, 1.0, 2.0)
    assert (lam[:, :16] == f32(0.75)).all() and (lam[:, 16:] == 0).all()
    o = D.denoise(p, n, radius=2, strength=3.0, gain=2.0, alpha=1e-2, beta=1e-3, w_lo=1.0, w_hi=2.0)
    s = D.clean(p)
    assert np.array_equal(o[:, 16:].view(np.uint32), s[:, 16:].view(np.uint32))
    assert (o[:, :16] != s[:, :16]).mean() > 0.1      # (white noise of width 1.4: not every pixel has a neighbour in reach)
    # the fade's ends: lambda 1 at n <= wLo, NaN counts are cleaned to 0
    assert (D.fade(np.array([0.0, 0.5, 1.0, 1.5, 2.0, 7.0, -3.0], f32), 1.0, 2.0) == np.array([1, 1, 1, 0.5, 0, 0, 1], f32)).all()
    assert (D.fade(np.array([5.0], f32), 0.0, 0.0) == 1).all()


def _hostile(h, w, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.25, 1.25, (h, w, 3)).astype(f32)
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 70000.0, -70000.0, 0.0, -0.0, 1e-30, 65536.0, 2.5, -3.0], f32)
    flat = p.reshape(-1)
    idx = np.arange(0, flat.size, 7)
    flat[idx] = special[np.arange(idx.size) % special.size]
    n = rng.uniform(0.0, 8.0, (h, w, 3)).astype(f32)
    counts = np.array([0.0, np.nan, 1e-9, 1e6, np.inf, -1.0, -np.inf, 1e-30, 3e38], f32)
    flat = n.reshape(-1)
    idx = np.arange(3, flat.size, 11)
    flat[idx] = counts[np.arange(idx.size) % counts.size]
    return p, n


@pytest.mark.parametrize("desc", [dict(radius=3, strength=16.0, gain=1024.0, alpha=1.0, beta=1.0),
                                  dict(radius=3, strength=0.0625, gain=1e-30, alpha=0.0, beta=0.0),
                                  dict(radius=2, strength=3.0, gain=2.0, alpha=1.6e-3, beta=1.6e-5, w_lo=1.0, w_hi=2.0),
                                  dict(radius=1, strength=16.0, gain=1024.0, alpha=1.0, beta=1.0, w_lo=0.0, w_hi=3e38)])
def test_hostile_values_stay_finite_and_G_is_at_least_one(desc):
    """NaN, +-inf and huge values in the image, 0 / NaN / tiny / huge / negative / infinite counts, at the corners of the
    description's bounds: the restatement raises on any overflow or invalid operation in steps 4-6 (np.errstate), G >= 1
    everywhere, and the output is finite and within the cleaned range"""
    p, n = _hostile(23, 29, 5)
    o, G, S = D.denoise(p, n, want_sums=True, **desc)
    assert np.isfinite(o).all() and np.isfinite(G).all() and np.isfinite(S).all()
    assert (G >= 1).all() and (G <= f32((2 * desc["radius"] + 1) ** 2)).all()
    assert (np.abs(o) <= 65536.0 * (1 + 2 ** -20)).all()
    o1 = D.denoise(p, None, **desc)
    assert np.isfinite(o1).all()


def test_count_of_weight_follows_the_finish():
    w = np.array([0.0, 5e-4, 9.99e-4, 1e-3, 2.0, np.nan, -1.0], f32)
    n = D.count_of_weight(w, 1e-3)
    assert np.array_equal(n[:5], np.array([1.0, f32(5e-4) + f32(1), f32(9.99e-4) + f32(1), f32(1e-3), 2.0], f32))
    assert np.isnan(n[5]) and n[6] == 0.0


def test_the_filter_narrows_where_more_was_averaged():
    """one noisy flat patch, the same noise, counts of 1 and of 16: the filter removes more where the count is smaller"""
    rng = np.random.default_rng(9)
    flat = np.full((40, 40, 3), 0.5, f32)
    noisy = (flat + rng.normal(0, np.sqrt(1e-3 * 0.5 + 1e-5), flat.shape)).astype(f32)
    res = []
    for count in (1.0, 16.0):
        o = D.denoise(noisy, np.full_like(flat, count), radius=2, strength=3.0, gain=2.0, alpha=1e-3, beta=1e-5)
        res.append(float(np.std(o[4:-4, 4:-4] - 0.5)))
    assert res[0] < 0.5 * float(np.std(noisy[4:-4, 4:-4] - 0.5)) and res[0] < res[1]


# ---- the quality condition ------------------------------------------------------------------------------------------------------
def test_quality_condition_on_the_moving_burst():
    """The oracle merge of synth.make_moving_burst(256, 192, 6, alpha=1.6e-3, beta=1.6e-5, obj_size=(48, 48), obj_step=(9, 3)),
    denoised by the restatement at R = 3, strength 3, gain 4, no fade; classes by minimum channel weight < 1.5, [1.5, 4), >= 4,
    a 16-pixel border left out.  The PSNR against the oracle merge of the noise=False twin rises by at least 1.0 dB in every
    class, and the PSNR against the ground truth falls in none.  (Measured: +1.50 / +1.73 / +1.27 dB and +1.30 / +0.76 / +0.39
    dB.)"""
    from tools import denoise_quality as Q
    out = Q.experiment()
    assert set(out["classes"]) == {"lt1.5", "1.5to4", "ge4"}
    for name, c in out["classes"].items():
        print(f"{name}: {c['pixels']} pixels, vs noiseless {c['psnr_vs_noiseless'][0]:.3f} -> {c['psnr_vs_noiseless'][1]:.3f} dB, "
              f"vs truth {c['psnr_vs_truth'][0]:.3f} -> {c['psnr_vs_truth'][1]:.3f} dB, "
              f"variance measured / predicted {c['variance_measured_over_predicted']:.2f}")
    for name, c in out["classes"].items():
        assert c["pixels"] > 500, name
        assert c["gain_vs_noiseless_db"] >= 1.0, (name, c)
        assert c["gain_vs_truth_db"] >= 0.0, (name, c)
