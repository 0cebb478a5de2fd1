"""Exposure matching, host side (no device): the numpy / Python-int restatement of the rule in include/mfsr.h (measure, gain,
apply; the GPU tests compare the kernels with it bit for bit), mfsr_exposure_gains against it, the properties of the rule on
the flicker fixture, and the five entry points refusing bad arguments before any device call."""
import ctypes

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi

DEADBAND, MIN_GAIN, MAX_GAIN = 164, 16384, 262144
BLACK, SAT, MAXV = (256, 256, 256, 256), 4095, 4095
RGGB, GRBG, GBRG, BGGR = (0, 1, 1, 2), (1, 0, 2, 1), (1, 2, 0, 1), (2, 1, 1, 0)
PHASES = (RGGB, GRBG, GBRG, BGGR)


# ---- the rule, restated (the contract in include/mfsr.h) -----------------------------------------------------------------
def measure(frame, rect, black=BLACK, sat=SAT):
    """[S0, S1, S2, S3, C] of one u16 frame [H, W] over the half-resolution rectangle (x0, y0, x1, y1)."""
    x0, y0, x1, y1 = rect
    a = frame.astype(np.int64)[2 * y0:2 * y1, 2 * x0:2 * x1]
    q = [a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]]
    ok = (q[0] < sat) & (q[1] < sat) & (q[2] < sat) & (q[3] < sat)
    return [int(np.maximum(p - b, 0)[ok].sum()) for p, b in zip(q, black)] + [int(ok.sum())]


def gains_rule(levels, reference, cfa, mono, per_colour, deadband=DEADBAND, min_gain=MIN_GAIN, max_gain=MAX_GAIN):
    """(gains [n][3], status [n]) in Python integers."""
    split = bool(per_colour) and not mono
    classes = sorted(set(cfa)) if split else [0, 1, 2]

    def total(k, c):
        return sum(levels[k][q] for q in range(4) if not split or cfa[q] == c)

    gains, status = [], []
    cr = levels[reference][4]
    for k in range(len(levels)):
        ck = levels[k][4]
        if k == reference:
            gains.append([65536] * 3)
            status.append(1)
            continue
        if ck == 0 or cr == 0 or any(total(k, c) == 0 or total(reference, c) == 0 for c in classes):
            gains.append([65536] * 3)
            status.append(2)
            continue
        g = [65536] * 3
        for c in classes:
            den = total(k, c) * cr
            g[c] = min((total(reference, c) * ck * 65536 + den // 2) // den, 2 ** 31 - 1)
        if all(abs(g[c] - 65536) <= deadband for c in classes):
            gains.append([65536] * 3)
            status.append(1)
        else:
            gains.append(g)
            status.append(0 if all(min_gain <= g[c] <= max_gain for c in classes) else 3)
    return gains, status


def apply_rule(frame, gain3, cfa, mono, black=BLACK, sat=SAT, maxv=MAXV):
    """One u16 frame [H, W] with the Q16 gains of its colours applied."""
    v = frame.astype(np.int64)
    out = v.copy()
    for q in range(4):
        sl = (slice(q >> 1, None, 2), slice(q & 1, None, 2))
        g, b = int(gain3[0 if mono else cfa[q]]), black[q]
        s = v[sl]
        new = np.minimum(b + (((s - b) * g + 32768) >> 16), maxv)
        out[sl] = np.where((s <= b) | (s >= sat), s, new)
    return out.astype(np.uint16)


def match_rule(frames, rect, reference, cfa, mono, per_colour=False, black=BLACK, sat=SAT, maxv=MAXV, **kw):
    """(matched frames, gains, status, levels): the whole of mfsr_burst_match_exposure."""
    levels = [measure(f, rect, black, sat) for f in frames]
    gains, status = gains_rule(levels, reference, cfa, mono, per_colour, **kw)
    out = [apply_rule(f, g, cfa, mono, black, sat, maxv) if s == 0 else f.copy() for f, g, s in zip(frames, gains, status)]
    return out, gains, status, levels


# ---- the fixture: the synthetic burst of the defect tests with a flicker ---------------------------------------------------
FLICKER = (1.0, 1.06, 0.94, 1.12, 0.90, 1.03)
W, H, N = 512, 384, 6
RECT = (8, 8, W // 2 - 8, H // 2 - 8)   # what sharpness_rect gives for this size

_cache = {}


def flicker(frames, factors=FLICKER, black=256, maxv=4095):
    return [np.clip(np.round((c.astype(np.float64) - black) * t + black), 0, maxv).astype(np.uint16) for c, t in zip(frames, factors)]


def fixture(mono):
    """(clean frames, flicker frames, ground truth [3, sH, sW]) as numpy uint16 arrays [H, W]."""
    if mono not in _cache:
        from multi_frame_super_resolution_amd.synth import make_burst
        fr, _, gt = make_burst(W, H, N, 2, mono=mono, seed=11)
        clean = [f.numpy().view(np.uint16).copy() for f in fr]
        _cache[mono] = (clean, flicker(clean), gt)
    return _cache[mono]


def _cfg(mono=False, cfa=RGGB, black=256.0, white=3839.0, max_val=4095.0):
    cfg = capi.Config()
    cfg.width, cfg.height, cfg.mono, cfg.scale = W, H, 1 if mono else 0, 2
    for q in range(4):
        cfg.cfa[q] = cfa[q]
    for c in range(3):
        cfg.black[c], cfg.white[c] = black, white
    cfg.maxVal = max_val
    return cfg


# ---- 3: properties of the restatement on the fixture -----------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
def test_flicker_gains_are_recovered(mono):
    _, bad, _ = fixture(mono)
    _, gains, status, _ = match_rule(bad, RECT, 0, RGGB, mono)
    rel = [abs(g[0] / 65536.0 * t - 1.0) for g, t in zip(gains, FLICKER)]
    print("gains", [round(g[0] / 65536.0, 5) for g in gains], "relative error", [f"{r:.5f}" for r in rel])
    assert status == [1, 0, 0, 0, 0, 0]
    assert max(rel[1:]) <= 0.003
    assert all(g[0] == g[1] == g[2] for g in gains)
    # per colour: each colour's gain is within the same bound
    _, gains, status, _ = match_rule(bad, RECT, 0, RGGB, mono, per_colour=True)
    assert status == [1, 0, 0, 0, 0, 0]
    assert max(abs(g[c] / 65536.0 * t - 1.0) for g, t in list(zip(gains, FLICKER))[1:] for c in range(3)) <= 0.003


@pytest.mark.parametrize("mono", [False, True])
def test_clean_burst_falls_in_the_deadband(mono):
    clean, _, _ = fixture(mono)
    out, gains, status, levels = match_rule(clean, RECT, 0, RGGB, mono)
    raw, _ = gains_rule(levels, 0, RGGB, mono, False, deadband=0)
    print("natural |gain - 1|:", [f"{abs(g[0] - 65536) / 65536:.5f}" for g in raw])
    assert status == [1] * N and gains == [[65536] * 3] * N
    assert all(np.array_equal(a, b) for a, b in zip(out, clean))


def test_status_out_of_range_and_unmeasurable():
    clean, _, _ = fixture(False)
    bright = flicker(clean[:2], (1.0, 8.0), maxv=65535)
    _, gains, status, _ = match_rule(bright, RECT, 0, RGGB, False, sat=65535, maxv=65535)
    assert status == [1, 3] and abs(gains[1][0] / 65536.0 * 8 - 1) < 0.01
    burnt = [clean[0], np.full_like(clean[1], 4095)]
    out, gains, status, levels = match_rule(burnt, RECT, 0, RGGB, False)
    assert status == [1, 2] and levels[1] == [0, 0, 0, 0, 0] and gains[1] == [65536] * 3
    assert np.array_equal(out[1], burnt[1])
    # the other way round: a reference without a usable quad makes every frame unmeasurable
    assert gains_rule(levels, 1, RGGB, False, False)[1] == [2, 1]


@pytest.mark.parametrize("mono", [False, True])
def test_apply_properties(mono):
    _, bad, _ = fixture(mono)
    f = bad[3].copy()     # the 1.12 frame: it has clipped highlights; the scene has no shadows at or below black, so add some
    f[40:44, 40:104] = np.arange(1, 257, dtype=np.uint16).reshape(4, 64)
    assert (f >= SAT).any() and (f <= 256).any()
    assert np.array_equal(apply_rule(f, [65536] * 3, RGGB, mono), f)
    for g3 in ([16384, 65536, 262144], [100000] * 3, [262144] * 3, [4096, 1048576, 70000]):
        out = apply_rule(f, g3, RGGB, mono)
        fixed = (f <= 256) | (f >= SAT)
        assert np.array_equal(out[fixed], f[fixed])
        assert out.max() <= MAXV
        assert not np.array_equal(out, f)
    # a wide range: the product (v - b) * g needs more than 32 bits
    g = np.random.default_rng(1)
    wide = g.integers(0, 65536, size=(64, 64), dtype=np.uint16)
    out = apply_rule(wide, [1048576] * 3, RGGB, mono, black=(0, 1, 2, 3), sat=65535, maxv=65535)
    assert out.max() == 65535
    out = apply_rule(wide, [1048576] * 3, RGGB, mono, black=(0, 1, 2, 3), sat=65535, maxv=60000)
    keep = (wide >= 65535) | (wide <= np.tile(np.array([[0, 1], [2, 3]]), (32, 32)))
    assert out[~keep].max() <= 60000 and np.array_equal(out[keep], wide[keep])


# ---- 2: mfsr_exposure_gains against the restatement ------------------------------------------------------------------------
def _lib_gains(levels, reference, cfa, mono, per_colour, deadband=DEADBAND, min_gain=MIN_GAIN, max_gain=MAX_GAIN):
    n = len(levels)
    flat = (ctypes.c_longlong * (5 * n))(*[v for row in levels for v in row])
    gains, status = (ctypes.c_int32 * (3 * n))(*([-7] * (3 * n))), (ctypes.c_int32 * n)(*([-7] * n))
    rc = capi.lib().raw["mfsr_exposure_gains"](n, flat, reference, (ctypes.c_int32 * 4)(*cfa), 1 if mono else 0, 1 if per_colour else 0,
                                               deadband, min_gain, max_gain, gains, status)
    assert rc == 0
    return [[gains[3 * k + c] for c in range(3)] for k in range(n)], list(status)


CASES = [(cfa, False, pc) for cfa in PHASES for pc in (False, True)] + [(RGGB, True, False), (RGGB, True, True)]


@pytest.mark.parametrize("cfa,mono,per_colour", CASES)
def test_gains_random_tables(cfa, mono, per_colour):
    g = np.random.default_rng(sum(cfa) * 7 + mono * 3 + per_colour + cfa[0])
    seen = set()
    for trial in range(60):
        n = int(g.integers(1, 17))
        big = trial % 3 == 0                                  # sums up to 2^41, counts up to 2^23: the 128-bit path
        base = int(g.integers(1, 2 ** 41 if big else 2 ** 20))
        levels = []
        for _ in range(n):
            spread = float(g.choice([0.002, 0.1, 3.0, 30.0]))          # deadband, matched and out-of-range frames
            f = float(np.exp(g.uniform(-1, 1) * np.log1p(spread)))
            s = [min(max(int(base * f * float(g.uniform(0.9, 1.1))), 0), 2 ** 41) for _ in range(4)]
            c = int(g.integers(1, 2 ** 23 + 1)) if big else int(g.integers(1, 5000))
            if g.random() < 0.06:
                s[int(g.integers(0, 4))] = 0                     # a zero sum
            if g.random() < 0.04:
                s = [0, 0, 0, 0]
            if g.random() < 0.04:
                c = 0
            levels.append(s + [c])
        ref = int(g.integers(0, n))
        want = gains_rule(levels, ref, cfa, mono, per_colour)
        assert _lib_gains(levels, ref, cfa, mono, per_colour) == want, (levels, ref)
        seen.update(want[1])
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("mono", [False, True])
def test_gains_edges(mono):
    c = 1000
    ref = [65536 * 10] * 4 + [c]

    # T[ref] = 4 * 655360; a frame with sums t each and the same count has gain round(655360 * 65536 / t)
    def lv(t):
        return [t] * 4 + [c]

    def one(t, **kw):
        got = _lib_gains([ref, lv(t)], 0, RGGB, mono, False, **kw)
        assert got == gains_rule([ref, lv(t)], 0, RGGB, mono, False, **kw)
        return got[0][1][0], got[1][1]

    # exactly at the deadband and one beyond, on both sides (t chosen so that the quotient is exact)
    for want_gain in (65536 + 164, 65536 - 164, 65536 + 165, 65536 - 165, 16384, 16383, 262144, 262145):
        levels = [[want_gain * 5] * 4 + [c], [65536 * 5] * 4 + [c]]
        got = _lib_gains(levels, 0, RGGB, mono, False)
        assert got == gains_rule(levels, 0, RGGB, mono, False)
        inside = abs(want_gain - 65536) <= 164
        assert got[0][1] == ([65536] * 3 if inside else [want_gain] * 3)
        assert got[1][1] == (1 if inside else 0 if 16384 <= want_gain <= 262144 else 3)
    assert one(655360) == (65536, 1)
    assert one(655360, deadband=0) == (65536, 1)
    assert one(1)[1] == 3 and one(1)[0] == 2 ** 31 - 1            # saturated
    assert one(0) == (65536, 2)
    assert one(655360 * 3, min_gain=65536) == (21845, 3)
    assert one(655360 // 2, max_gain=65536) == (131072, 3)
    # the count ratio enters: half the usable quads with half the sums is the same exposure
    got = _lib_gains([ref, [65536 * 5] * 4 + [c // 2]], 0, RGGB, mono, False)
    assert got == ([[65536] * 3] * 2, [1, 1])
    # rounding to nearest: den/2 is added before the division
    levels = [[3, 0, 0, 0, 1], [7, 0, 0, 0, 1]]
    assert _lib_gains(levels, 0, RGGB, mono, False) == gains_rule(levels, 0, RGGB, mono, False)
    assert _lib_gains(levels, 0, RGGB, mono, False)[0][1][0] == (3 * 65536 + 3) // 7


def test_gains_per_colour_classes():
    # red doubled, green unchanged, blue halved, in every Bayer phase
    for cfa in PHASES:
        ref = [1000 * 64] * 4 + [64]
        k = [0] * 4 + [64]
        for q in range(4):
            k[q] = ref[q] * (1, 2, 4)[cfa[q]] // 2
        gains, status = _lib_gains([ref, k], 0, cfa, False, True)
        assert (gains, status) == gains_rule([ref, k], 0, cfa, False, True)
        assert gains[1] == [131072, 65536, 32768] and status == [1, 0]
        # one colour in the deadband does not make the frame status 1; all of them do
        assert _lib_gains([ref, ref], 0, cfa, False, True)[1] == [1, 1]
        # a zero sum of one colour only: unmeasurable in per-colour mode, measurable in common mode
        z = list(ref)
        z[cfa.index(2)] = 0
        assert _lib_gains([ref, z], 0, cfa, False, True)[1] == [1, 2]
        assert _lib_gains([ref, z], 0, cfa, False, False)[1] == [1, 0]
    # mono ignores perColour
    lv = [[100, 200, 300, 400, 10], [200, 100, 400, 300, 10]]
    assert _lib_gains(lv, 0, RGGB, True, True) == _lib_gains(lv, 0, RGGB, True, False) == ([[65536] * 3] * 2, [1, 1])


# ---- 5: declarations, symbols, defaults -----------------------------------------------------------------------------------
NAMES = ("mfsr_frameLevels", "mfsr_exposure_gains", "mfsr_applyGains", "mfsr_burst_match_exposure", "mfsr_exposure_defaults")


def test_declarations_parse():
    protos = capi.parse_header()
    for name in NAMES:
        assert name in protos and protos[name][0] == "int"
    assert [a for _, a in protos["mfsr_frameLevels"][1]] == [
        "nFrames", "frames", "pitch", "width", "height", "black", "sat", "rect", "levelsDev", "stream"]
    assert [a for _, a in protos["mfsr_exposure_gains"][1]] == [
        "n", "levels", "reference", "cfa", "mono", "perColour", "deadband", "minGain", "maxGain", "gains", "status"]
    assert [a for _, a in protos["mfsr_applyGains"][1]] == [
        "nFrames", "frames", "pitch", "width", "height", "cfa", "mono", "black", "sat", "maxValue", "gains", "status", "stream"]
    assert [a for _, a in protos["mfsr_burst_match_exposure"][1]] == [
        "b", "nFrames", "frames", "reference", "perColour", "deadband", "minGain", "maxGain", "levelsDev", "gains", "status",
        "levels", "stream"]
    assert [a for _, a in protos["mfsr_exposure_defaults"][1]][0] == "cfg"


def test_symbols_resolve():
    L = capi.lib()   # (raises if the library is missing: building it is part of the contract)
    for name in NAMES:
        assert name in L.raw


def _lib_defaults(cfg):
    black = (ctypes.c_int32 * 4)()
    v = [ctypes.c_int32(-1) for _ in range(6)]
    assert capi.lib().raw["mfsr_exposure_defaults"](ctypes.byref(cfg), black, *[ctypes.byref(x) for x in v]) == 0
    return (tuple(black),) + tuple(x.value for x in v)


def test_defaults_rule():
    from multi_frame_super_resolution_amd.pipeline import exposure_defaults, sharpness_rect
    cfg = _cfg()
    d = exposure_defaults(cfg)
    assert tuple(d) == ((256,) * 4, 4095, 4095, 164, 16384, 262144, False)
    assert _lib_defaults(cfg) == ((256,) * 4, 4095, 4095, 164, 16384, 262144, 0)
    assert sharpness_rect(cfg) == RECT
    for cfa in PHASES + (RGGB,):
        cfg = _cfg(cfa=cfa)
        cfg.black[0], cfg.black[1], cfg.black[2] = 63.5, 64.49, 250.75
        cfg.white[0], cfg.white[1], cfg.white[2] = 960.25, 959.0, 700.0
        cfg.maxVal = 1023.9
        d = exposure_defaults(cfg)
        assert d.black == tuple((64, 64, 251)[c] for c in cfa) and d.sat == 950 and d.max_value == 1023
        assert _lib_defaults(cfg)[:3] == (d.black, d.sat, d.max_value)
    cfg.mono = 1
    assert exposure_defaults(cfg).black == (64,) * 4 and _lib_defaults(cfg)[0] == (64,) * 4
    # every output of the C helper is optional
    assert capi.lib().raw["mfsr_exposure_defaults"](ctypes.byref(cfg), None, None, None, None, None, None, None) == 0
    assert capi.lib().raw["mfsr_exposure_defaults"](None, None, None, None, None, None, None, None) == -1


def test_python_gains_is_host_only():
    from multi_frame_super_resolution_amd.pipeline import exposure_gains
    _, bad, _ = fixture(False)
    levels = [measure(f, RECT) for f in bad]
    want = gains_rule(levels, 0, RGGB, False, False)
    assert exposure_gains(levels, _cfg(), 0) == want
    assert exposure_gains(np.array(levels), _cfg(), 0, per_colour=True) == gains_rule(levels, 0, RGGB, False, True)
    assert exposure_gains(levels, _cfg(), 2, deadband=0, min_gain=65536, max_gain=65536 * 2) == \
        gains_rule(levels, 2, RGGB, False, False, deadband=0, min_gain=65536, max_gain=65536 * 2)


# ---- 4: host validation ------------------------------------------------------------------------------------------------------
FAKE = 0x10000  # an aligned "device" pointer: validation fails before any device call, so it is never used
I4 = ctypes.c_int32 * 4


def _frames_valid(n, frames, pitch, width, height):
    if not 1 <= n <= 64 or frames is None or any(not f or f % 2 for f in frames[:n]):
        return False
    return width > 0 and height > 0 and width % 2 == 0 and height % 2 == 0 and pitch >= 2 * width and pitch % 2 == 0


def _levels_valid(black, sat, maxv):
    return black is not None and all(0 <= b <= 65535 for b in black) and 0 < sat <= maxv <= 65535


def _rect_valid(rect, width, height):
    if rect is None:
        return False
    x0, y0, x1, y1 = rect
    return 1 <= x0 < x1 <= width // 2 - 1 and 1 <= y0 < y1 <= height // 2 - 1 and (x1 - x0) * (y1 - y0) <= 2 ** 23


def _bounds_valid(deadband, min_gain, max_gain):
    return 0 <= deadband < 65536 and 4096 <= min_gain <= 65536 <= max_gain <= 1048576


def _ptrs(n, frames):
    if isinstance(frames, str):
        return (ctypes.c_void_p * max(n, 1))(*([FAKE] * max(n, 1)))
    return frames


VW, VH = 64, 48


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=65), dict(n=-1), dict(frames=None), dict(frames=(ctypes.c_void_p * 2)(FAKE, None)),
    dict(frames=(ctypes.c_void_p * 2)(FAKE, FAKE + 1)), dict(pitch=2 * VW - 2), dict(pitch=2 * VW + 1), dict(width=0), dict(height=-2),
    dict(width=VW - 1), dict(height=VH + 1), dict(black=None), dict(black=(0, 0, -1, 0)), dict(black=(0, 65536, 0, 0)),
    dict(sat=0), dict(sat=-5), dict(sat=65536), dict(rect=None), dict(rect=(0, 1, 8, 8)), dict(rect=(1, 0, 8, 8)),
    dict(rect=(8, 1, 8, 8)), dict(rect=(1, 8, 8, 8)), dict(rect=(1, 1, VW // 2, 8)), dict(rect=(1, 1, 8, VH // 2)),
    dict(width=8192, height=8192, pitch=16384, rect=(1, 1, 4095, 4095)), dict(levels=None), dict(levels=FAKE + 4),
])
def test_frame_levels_host_validation(kw):
    a = dict(n=2, frames="ok", pitch=2 * VW, width=VW, height=VH, black=(256,) * 4, sat=4095, rect=(1, 1, VW // 2 - 1, VH // 2 - 1),
             levels=FAKE)
    a.update(kw)
    fr = _ptrs(a["n"], a["frames"])
    valid = (_frames_valid(a["n"], None if fr is None else list(fr), a["pitch"], a["width"], a["height"])
             and _levels_valid(a["black"], a["sat"], 65535) and _rect_valid(a["rect"], a["width"], a["height"])
             and bool(a["levels"]) and a["levels"] % 8 == 0)
    assert not valid, "test bug: these arguments are valid and would reach the device"
    rc = capi.lib().raw["mfsr_frameLevels"](a["n"], fr, a["pitch"], a["width"], a["height"], None if a["black"] is None else I4(*a["black"]),
                                            a["sat"], None if a["rect"] is None else I4(*a["rect"]), a["levels"], None)
    assert rc == -1


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=65), dict(frames=None), dict(frames=(ctypes.c_void_p * 2)(None, FAKE)), dict(frames=(ctypes.c_void_p * 2)(FAKE + 1, FAKE)),
    dict(pitch=2 * VW - 2), dict(pitch=2 * VW + 1), dict(width=0), dict(width=VW + 1, pitch=4 * VW), dict(height=VH - 1), dict(height=0),
    dict(cfa=None), dict(cfa=(0, 1, 1, 3)), dict(cfa=(-1, 1, 1, 2)), dict(black=None), dict(black=(-1, 0, 0, 0)),
    dict(sat=0), dict(sat=4096), dict(maxv=65536, sat=65536), dict(maxv=70000), dict(gains=None), dict(status=None),
    dict(status=(0, 4)), dict(status=(-1, 1)), dict(gains=(65536, 65536, 65536, 4095, 65536, 65536), status=(1, 0)),
    dict(gains=(1048577, 65536, 65536, 65536, 65536, 65536)), dict(gains=(65536, 0, 65536, 65536, 65536, 65536)),
])
def test_apply_gains_host_validation(kw):
    a = dict(n=2, frames="ok", pitch=2 * VW, width=VW, height=VH, cfa=RGGB, mono=0, black=(256,) * 4, sat=4095, maxv=4095,
             gains=(70000,) * 6, status=(0, 0))
    a.update(kw)
    n = a["n"]
    fr = _ptrs(n, a["frames"])
    gains_ok = a["gains"] is not None and a["status"] is not None and len(a["status"]) >= n and all(
        0 <= a["status"][k] <= 3 and (a["status"][k] != 0 or all(4096 <= a["gains"][3 * k + c] <= 1048576 for c in set(a["cfa"])))
        for k in range(max(min(n, 2), 0))) if a["cfa"] is not None and all(0 <= c <= 2 for c in a["cfa"]) else False
    valid = (_frames_valid(n, None if fr is None else list(fr), a["pitch"], a["width"], a["height"])
             and _levels_valid(a["black"], a["sat"], a["maxv"]) and gains_ok)
    assert not valid, "test bug: these arguments are valid and would reach the device"
    m = max(n, 2)
    gains = None if a["gains"] is None else (ctypes.c_int32 * (3 * m))(*(list(a["gains"]) + [65536] * (3 * m - len(a["gains"]))))
    status = None if a["status"] is None else (ctypes.c_int32 * m)(*(list(a["status"]) + [1] * (m - len(a["status"]))))
    rc = capi.lib().raw["mfsr_applyGains"](n, fr, a["pitch"], a["width"], a["height"], None if a["cfa"] is None else I4(*a["cfa"]),
                                           a["mono"], None if a["black"] is None else I4(*a["black"]), a["sat"], a["maxv"], gains,
                                           status, None)
    assert rc == -1


def test_apply_gains_without_a_status_0_frame_touches_no_device():
    """All frames untouched: the call returns before any launch (the pointers are fake; a launch would fault)."""
    fr = (ctypes.c_void_p * 3)(FAKE, FAKE, FAKE)
    gains, status = (ctypes.c_int32 * 9)(*([65536] * 9)), (ctypes.c_int32 * 3)(1, 2, 3)
    assert capi.lib().raw["mfsr_applyGains"](3, fr, 2 * VW, VW, VH, I4(*RGGB), 0, I4(*BLACK), SAT, MAXV, gains, status, None) == 0


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=-3), dict(levels=None), dict(reference=-1), dict(reference=2), dict(cfa=None), dict(cfa=(0, 1, 1, 6)),
    dict(deadband=-1), dict(deadband=65536), dict(min_gain=4095), dict(min_gain=65537), dict(max_gain=65535), dict(max_gain=1048577),
    dict(gains=None), dict(status=None), dict(levels=[[1, 1, 1, -1, 1], [1, 1, 1, 1, 1]]), dict(levels=[[1, 1, 1, 1, 1], [2 ** 48, 1, 1, 1, 1]]),
])
def test_exposure_gains_host_validation(kw):
    a = dict(n=2, levels=[[100, 100, 100, 100, 10]] * 2, reference=0, cfa=RGGB, mono=0, deadband=DEADBAND, min_gain=MIN_GAIN,
             max_gain=MAX_GAIN, gains=True, status=True)
    a.update(kw)
    flat = None if a["levels"] is None else (ctypes.c_longlong * 10)(*[v for row in a["levels"] for v in row])
    gains = (ctypes.c_int32 * 6)() if a["gains"] else None
    status = (ctypes.c_int32 * 2)() if a["status"] else None
    rc = capi.lib().raw["mfsr_exposure_gains"](a["n"], flat, a["reference"], None if a["cfa"] is None else I4(*a["cfa"]), a["mono"], 0,
                                               a["deadband"], a["min_gain"], a["max_gain"], gains, status)
    assert rc == -1
    # mono needs no CFA
    if a["cfa"] is None:
        assert capi.lib().raw["mfsr_exposure_gains"](2, flat, 0, None, 1, 0, DEADBAND, MIN_GAIN, MAX_GAIN, gains, status) == 0


def test_burst_match_exposure_host_validation():
    L = capi.lib()
    frames = (ctypes.c_void_p * 2)(FAKE, FAKE)
    # without a burst nothing can pass: every call below fails on its first check
    assert L.raw["mfsr_burst_match_exposure"](None, 2, frames, 0, 0, DEADBAND, MIN_GAIN, MAX_GAIN, FAKE, None, None, None, None) == -1
