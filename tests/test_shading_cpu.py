"""Lens-shading correction, host side (no device): the numpy / Python-int restatement of the rule in include/mfsr.h (the gain of
a sample, apply, box statistics, fit; the GPU tests compare the kernels with it bit for bit), mfsr_shading_fit and
mfsr_shading_defaults against it, the five entry points refusing bad arguments before any device call, and the recovery of a
synthetic vignette from a flat-field burst."""
import ctypes

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi

BLACK, SAT, MAXV = (256, 256, 256, 256), 4095, 4095
MIN_QUADS, MAX_GAIN = 64, 524288
KS = (3, 4, 5, 6, 7, 8)


# ---- the rule, restated (the contract in include/mfsr.h) -----------------------------------------------------------------
def grid(w, h, k):
    """(gw, gh) of a w x h frame at cell 1 << k."""
    cell = 1 << k
    return (w // 2 - 2 + cell) // cell + 1, (h // 2 - 2 + cell) // cell + 1


def gain_at(gmap, w, h, k):
    """The Q16 gain of every sample of a w x h frame under the map [4, gh, gw]: int64 [h, w]."""
    cell, cm = 1 << k, (1 << k) - 1
    gw, gh = grid(w, h, k)
    G = np.asarray(gmap).astype(np.int64)
    assert G.shape == (4, gh, gw)
    x, y = np.arange(w), np.arange(h)
    X, Y = x >> 1, y >> 1
    i, fx, j, fy = (X >> k)[None, :], (X & cm)[None, :], (Y >> k)[:, None], (Y & cm)[:, None]
    i1, j1 = np.minimum(i + 1, gw - 1), np.minimum(j + 1, gh - 1)     # (weight 0 where clamped)
    assert not ((i + 1 > gw - 1) & (fx != 0)).any() and not ((j + 1 > gh - 1) & (fy != 0)).any()
    q = 2 * (y & 1)[:, None] + (x & 1)[None, :]
    n = ((cell - fx) * (cell - fy) * G[q, j, i] + fx * (cell - fy) * G[q, j, i1] + (cell - fx) * fy * G[q, j1, i]
         + fx * fy * G[q, j1, i1])
    return (n + (1 << (2 * k - 1))) >> (2 * k)


def apply_rule(frame, gmap, k, black=BLACK, maxv=MAXV):
    """One u16 frame [H, W] with the gain map applied."""
    h, w = frame.shape
    v = frame.astype(np.int64)
    b = np.array(black, dtype=np.int64)[2 * (np.arange(h) & 1)[:, None] + (np.arange(w) & 1)[None, :]]
    new = np.minimum(b + (((v - b) * gain_at(gmap, w, h, k) + 32768) >> 16), maxv)
    return np.where(v <= b, v, new).astype(np.uint16)


def _box_sums(a, k, n_out):
    """Sums of a [hh, hw] over the boxes of the grid points: [gh, gw] (boxes the frame does not reach stay 0)."""
    cell = 1 << k
    out = np.zeros(n_out, dtype=np.int64)
    for axis in (0, 1):
        n = a.shape[axis]
        starts = [0] + list(range(cell // 2, n, cell))
        a = np.add.reduceat(a, starts, axis=axis)
    out[:a.shape[0], :a.shape[1]] = a
    return out


def stats_rule(frames, k, black=BLACK, sat=SAT):
    """(sums int64 [4, gh, gw], counts int64 [gh, gw]) over all the frames."""
    h, w = frames[0].shape
    gw, gh = grid(w, h, k)
    sums, counts = np.zeros((4, gh, gw), dtype=np.int64), np.zeros((gh, gw), dtype=np.int64)
    for f in frames:
        a = f.astype(np.int64)
        p = [a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]]
        ok = (p[0] < sat) & (p[1] < sat) & (p[2] < sat) & (p[3] < sat)
        for q in range(4):
            sums[q] += _box_sums(np.where(ok, np.maximum(p[q] - black[q], 0), 0), k, (gh, gw))
        counts += _box_sums(ok.astype(np.int64), k, (gh, gw))
    return sums, counts


def fit_rule(sums, counts, min_quads=MIN_QUADS, max_gain=MAX_GAIN):
    """(map int32 [4, gh, gw], status) in Python integers."""
    gh, gw = np.asarray(counts).shape
    n = gh * gw
    S = [[int(v) for v in np.asarray(sums)[q].reshape(-1)] for q in range(4)]
    C = [int(v) for v in np.asarray(counts).reshape(-1)]
    flat = np.full((4, gh, gw), 65536, dtype=np.int32)
    if any(C[p] < min_quads or any(S[q][p] == 0 for q in range(4)) for p in range(n)):
        return flat, 2
    T = [S[0][p] + S[1][p] + S[2][p] + S[3][p] for p in range(n)]
    a = 0
    for p in range(1, n):
        if T[p] * C[a] > T[a] * C[p]:
            a = p
    out, clamped = [], False
    for q in range(4):
        for p in range(n):
            den = S[q][p] * C[a]
            v = (S[q][a] * C[p] * 65536 + den // 2) // den
            clamped = clamped or v > max_gain
            out.append(min(max(v, 65536), max_gain))
    return np.array(out, dtype=np.int32).reshape(4, gh, gw), 3 if clamped else 0


def defaults_rule(w, h):
    """The default cell of a w x h frame."""
    m = min(w, h) // 2 - 1
    assert m >= 8
    cell = 64
    while cell > m:
        cell //= 2
    return cell


# ---- the restatement against the formula as the header writes it ---------------------------------------------------------------
@pytest.mark.parametrize("w,h,k", [(18, 18, 3), (70, 38, 3), (70, 38, 4), (258, 130, 6), (1032, 18, 3), (516, 520, 8)])
def test_gain_at_is_the_formula(w, h, k):
    g = np.random.default_rng(w + h + k)
    gw, gh = grid(w, h, k)
    G = g.integers(4096, 1048577, size=(4, gh, gw))
    got = gain_at(G, w, h, k)
    cell = 1 << k
    pts = [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1)] + [(int(g.integers(0, w)), int(g.integers(0, h))) for _ in range(300)]
    for x, y in pts:
        X, Y, q = x >> 1, y >> 1, 2 * (y & 1) + (x & 1)
        i, fx, j, fy = X >> k, X & (cell - 1), Y >> k, Y & (cell - 1)

        def at(jj, ii, weight):
            return weight * int(G[q, jj, ii]) if weight else 0       # a term of weight 0 is not read

        n = (at(j, i, (cell - fx) * (cell - fy)) + at(j, i + 1, fx * (cell - fy)) + at(j + 1, i, (cell - fx) * fy)
             + at(j + 1, i + 1, fx * fy) + (1 << (2 * k - 1)))
        assert n < 2 ** 37 and got[y, x] == n >> (2 * k)
    assert got.min() >= 4096 and got.max() <= 1048576
    # at a grid point the gain is the map's value; a flat map is flat
    for q in range(4):
        sub = got[(q >> 1)::2, (q & 1)::2][::cell, ::cell]
        assert np.array_equal(sub, G[q, :sub.shape[0], :sub.shape[1]])
    assert (gain_at(np.full((4, gh, gw), 70001), w, h, k) == 70001).all()


def test_apply_rule_properties():
    g = np.random.default_rng(5)
    w, h, k = 70, 38, 3
    gw, gh = grid(w, h, k)
    f = g.integers(0, 4096, size=(h, w)).astype(np.uint16)
    f[3:9, 5:40] = 4095
    assert np.array_equal(apply_rule(f, np.full((4, gh, gw), 65536), k), f)
    G = g.integers(65536, 4 * 65536, size=(4, gh, gw))
    out = apply_rule(f, G, k)
    assert np.array_equal(out[f <= 256], f[f <= 256]) and out.max() <= MAXV and (out >= f).all()
    # clipped samples are multiplied too (there is no sat): with room above, a clipped block rises with its neighbours
    out = apply_rule(f, G, k, maxv=65535)
    assert (out[3:9, 5:40] >= 4095).all() and (out[3:9, 5:40] > 4095).any()
    # the full range: (v - b) * g needs more than 32 bits
    wide = g.integers(0, 65536, size=(h, w)).astype(np.uint16)
    out = apply_rule(wide, np.full((4, gh, gw), 1048576), k, black=(0, 1, 2, 65535), maxv=65535)
    assert np.array_equal(out[1::2, 1::2], wide[1::2, 1::2]) and out[0::2, 0::2].max() == 65535


def test_stats_rule_boxes_tile_the_frame():
    g = np.random.default_rng(6)
    for (w, h), k in (((18, 18), 3), ((70, 38), 3), ((70, 38), 4), ((258, 130), 5), ((498, 60), 3)):
        f = [g.integers(0, 1000, size=(h, w)).astype(np.uint16) for _ in range(2)]
        sums, counts = stats_rule(f, k, black=(0, 0, 0, 0), sat=65535)
        assert counts.sum() == 2 * (w // 2) * (h // 2)
        assert [int(sums[q].sum()) for q in range(4)] == [sum(int(a[(q >> 1)::2, (q & 1)::2].sum()) for a in f) for q in range(4)]
        # brute force: the box of quad (X, Y) is ((X + cell/2) >> k, (Y + cell/2) >> k)
        cell = 1 << k
        want = np.zeros_like(counts)
        for Y in range(h // 2):
            for X in range(w // 2):
                want[(Y + cell // 2) >> k, (X + cell // 2) >> k] += 2
        assert np.array_equal(counts, want)
    # a saturated sample excludes its whole quad
    f = np.full((18, 18), 500, dtype=np.uint16)
    f[5, 7] = 4095
    sums, counts = stats_rule([f], 3)
    assert counts.sum() == 80 and sums.sum() == 4 * 80 * (500 - 256)


# ---- declarations, symbols, defaults -------------------------------------------------------------------------------------------
NAMES = ("mfsr_applyShading", "mfsr_shadingStats", "mfsr_shading_fit", "mfsr_shading_defaults", "mfsr_burst_correct_shading")


def test_declarations_parse():
    protos = capi.parse_header()
    for name in NAMES:
        assert name in protos and protos[name][0] == "int"
    assert [a for _, a in protos["mfsr_applyShading"][1]] == [
        "nFrames", "frames", "pitch", "width", "height", "mapDev", "cell", "black", "maxValue", "stream"]
    assert [a for _, a in protos["mfsr_shadingStats"][1]] == [
        "nFrames", "frames", "pitch", "width", "height", "cell", "black", "sat", "sumsDev", "countsDev", "stream"]
    assert [a for _, a in protos["mfsr_shading_fit"][1]] == ["sums", "counts", "gw", "gh", "minQuads", "maxGain", "map", "status"]
    assert [a for _, a in protos["mfsr_shading_defaults"][1]] == ["cfg", "black", "sat", "maxValue", "cell", "minQuads", "maxGain"]
    assert [a for _, a in protos["mfsr_burst_correct_shading"][1]] == ["b", "nFrames", "frames", "mapDev", "cell", "stream"]


def test_symbols_resolve():
    L = capi.lib()   # (raises if the library is missing: building it is part of the contract)
    for name in NAMES:
        assert name in L.raw


def _cfg(w, h, mono=False, black=256.0, white=3839.0, max_val=4095.0):
    cfg = capi.Config()
    cfg.width, cfg.height, cfg.mono, cfg.scale = w, h, 1 if mono else 0, 2
    for q, c in enumerate((0, 1, 1, 2)):
        cfg.cfa[q] = c
    for c in range(3):
        cfg.black[c], cfg.white[c] = black, white
    cfg.maxVal = max_val
    return cfg


def _lib_defaults(cfg):
    black = (ctypes.c_int32 * 4)()
    v = [ctypes.c_int32(-1) for _ in range(5)]
    rc = capi.lib().raw["mfsr_shading_defaults"](ctypes.byref(cfg), black, *[ctypes.byref(x) for x in v])
    return rc, (tuple(black),) + tuple(x.value for x in v)


@pytest.mark.parametrize("w,h,cell", [(18, 18, 8), (512, 384, 64), (3840, 2160, 64), (34, 18, 8), (36, 34, 16), (66, 400, 32),
                                      (130, 130, 64), (128, 130, 32)])
def test_defaults_rule(w, h, cell):
    from multi_frame_super_resolution_amd.pipeline import shading_defaults, shading_grid
    assert defaults_rule(w, h) == cell
    cfg = _cfg(w, h)
    assert tuple(shading_defaults(cfg)) == ((256,) * 4, 4095, 4095, cell, 64, 524288)
    assert _lib_defaults(cfg) == (0, ((256,) * 4, 4095, 4095, cell, 64, 524288))
    k = cell.bit_length() - 1
    gw, gh = grid(w, h, k)
    assert shading_grid(cfg) == (gw, gh) and gw >= 2 and gh >= 2


def test_defaults_refuse_small_frames_and_take_null_outputs():
    from multi_frame_super_resolution_amd.pipeline import shading_defaults
    raw = capi.lib().raw["mfsr_shading_defaults"]
    for w, h in ((16, 18), (18, 16), (16, 400), (2, 2)):
        cfg = _cfg(w, h)
        assert _lib_defaults(cfg)[0] == -1
        with pytest.raises(ValueError):
            shading_defaults(cfg)
        # the levels alone do not depend on the size
        assert raw(ctypes.byref(cfg), (ctypes.c_int32 * 4)(), None, None, None, None, None) == 0
    cfg = _cfg(512, 384)
    assert raw(ctypes.byref(cfg), None, None, None, None, None, None) == 0
    assert raw(None, None, None, None, None, None, None) == -1
    cfg.black[0], cfg.black[1], cfg.black[2] = 63.5, 64.49, 250.75
    cfg.white[0], cfg.white[1], cfg.white[2] = 960.25, 959.0, 700.0
    cfg.maxVal = 1023.9
    assert _lib_defaults(cfg)[1][:3] == ((64, 64, 64, 251), 950, 1023) == tuple(shading_defaults(cfg))[:3]


# ---- mfsr_shading_fit against the restatement --------------------------------------------------------------------------------
def _lib_fit(sums, counts, min_quads=MIN_QUADS, max_gain=MAX_GAIN):
    s, c = np.ascontiguousarray(sums, dtype=np.int64), np.ascontiguousarray(counts, dtype=np.int64)
    gh, gw = c.shape
    out = np.full((4, gh, gw), -7, dtype=np.int32)
    st = ctypes.c_int32(-7)
    rc = capi.lib().raw["mfsr_shading_fit"](s.ctypes.data, c.ctypes.data, gw, gh, min_quads, max_gain, out.ctypes.data, ctypes.byref(st))
    assert rc == 0
    return out, st.value


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1]


@pytest.mark.parametrize("k", KS)
def test_fit_random_tables(k):
    g = np.random.default_rng(100 + k)
    seen = set()
    for trial in range(40):
        w, h = 2 * int(g.integers(9, 700)), 2 * int(g.integers(9, 500))
        gw, gh = grid(w, h, k)
        big = trial % 4 == 0                                   # sums up to 2^47: the 128-bit path
        counts = g.integers(MIN_QUADS, 2 ** 22 if big else 5000, size=(gh, gw))
        level = g.integers(1, 2 ** 24 if big else 4000)
        fall = np.exp(-(0.05, 1.0, 4.0)[trial % 3] * g.random((1, gh, gw)))   # flat, within maxGain, beyond it
        sums = np.maximum((counts[None] * level * fall * g.uniform(0.9, 1.1, size=(4, gh, gw))).astype(np.int64), 1)
        if g.random() < 0.1:
            counts[int(g.integers(0, gh)), int(g.integers(0, gw))] = int(g.integers(0, MIN_QUADS))
        if g.random() < 0.1:
            sums[int(g.integers(0, 4)), int(g.integers(0, gh)), int(g.integers(0, gw))] = 0
        want = fit_rule(sums, counts)
        assert _same(_lib_fit(sums, counts), want), (w, h, k)
        assert want[0].min() >= 65536 and want[0].max() <= MAX_GAIN
        seen.add(want[1])
    assert seen == {0, 2, 3}


def test_fit_edges():
    c = np.full((3, 4), 1000, dtype=np.int64)
    s = np.full((4, 3, 4), 1000 * 700, dtype=np.int64)
    flat = np.full((4, 3, 4), 65536, dtype=np.int32)
    # a flat table: every gain 65536, status 0
    assert _same(_lib_fit(s, c), (flat, 0)) and _same(fit_rule(s, c), (flat, 0))
    # a zero count, a zero sum: unmeasurable
    for mod in (lambda s, c: c.__setitem__((1, 2), 0), lambda s, c: s.__setitem__((3, 2, 3), 0)):
        s2, c2 = s.copy(), c.copy()
        mod(s2, c2)
        s2[0, 0, 0] = 350000                   # (would be a gain of 2 if the table were measurable)
        assert _same(_lib_fit(s2, c2), (flat, 2)) and _same(fit_rule(s2, c2), (flat, 2))
    # the minQuads boundary
    s2, c2 = s.copy(), c.copy()
    c2[2, 3], s2[:, 2, 3] = 64, 64 * 350
    got = _lib_fit(s2, c2)
    assert _same(got, fit_rule(s2, c2)) and got[1] == 0 and (got[0][:, 2, 3] == 131072).all()
    c2[2, 3], s2[:, 2, 3] = 63, 63 * 350
    assert _same(_lib_fit(s2, c2), (flat, 2)) and _same(fit_rule(s2, c2), (flat, 2))
    assert _lib_fit(s2, c2, min_quads=63)[1] == 0
    # a clamp at maxGain: exactly at the bound is not clamped, one above is; the map is still returned
    for want_gain, status in ((524288, 0), (524289, 3), (1048576, 3)):
        s2 = s.copy()
        s2[1, 0, 1] = 1000 * 700 * 65536 // want_gain
        got = _lib_fit(s2, c)
        assert _same(got, fit_rule(s2, c)) and got[1] == status, want_gain
        assert got[0][1, 0, 1] == min((1000 * 700 * 1000 * 65536 + s2[1, 0, 1] * 500) // (s2[1, 0, 1] * 1000), 524288)
    assert _lib_fit(s2, c, max_gain=1048576)[1] == 0
    # a position brighter than at the anchor is clamped at 65536 without a status
    s2 = s.copy()
    s2[:, 1, 1] = 1000 * 900                  # the anchor
    s2[2, 0, 0] = 1000 * 950                  # one colour above the anchor's
    got = _lib_fit(s2, c)
    assert _same(got, fit_rule(s2, c)) and got[1] == 0 and got[0][2, 0, 0] == 65536 and got[0][0, 0, 0] == (900 * 65536 + 350) // 700
    # anchor ties go to the lowest index: two points with the same mean level but another colour balance
    s2 = s.copy()
    for p, (r, b) in (((0, 2), (800, 1000)), ((2, 1), (1000, 800))):
        s2[0][p], s2[1][p], s2[2][p], s2[3][p] = 1000 * r, 1000 * 900, 1000 * 900, 1000 * b
    got = _lib_fit(s2, c)
    assert _same(got, fit_rule(s2, c)) and (got[0][:, 0, 2] == 65536).all() and got[0][0, 2, 1] == 65536
    assert got[0][3, 2, 1] == (1000 * 65536 + 400) // 800
    # ... compared by cross-multiplication: half the quads with half the sums is the same level
    s3, c3 = s2.copy(), c.copy()
    c3[0, 2] = 500
    s3[:, 0, 2] //= 2
    assert _same(_lib_fit(s3, c3), fit_rule(s3, c3)) and (_lib_fit(s3, c3)[0][:, 0, 2] == 65536).all()
    # rounding to nearest: den/2 is added before the division
    s2 = s.copy()
    s2[:, 0, 0] = 1000 * 300
    assert _lib_fit(s2, c)[0][0, 0, 0] == (700 * 65536 + 150) // 300


def test_python_fit_is_host_only():
    from multi_frame_super_resolution_amd.pipeline import shading_fit
    g = np.random.default_rng(9)
    c = g.integers(64, 5000, size=(4, 5))
    s = (c[None] * g.integers(500, 3000, size=(4, 4, 5))).astype(np.int64)
    got = shading_fit(s, c)
    assert got[0].dtype == np.int32 and _same(got, fit_rule(s, c))
    assert _same(shading_fit(s.tolist(), c.tolist(), min_quads=1, max_gain=65536), fit_rule(s, c, 1, 65536))
    with pytest.raises(ValueError):
        shading_fit(s[:3], c)


# ---- host validation ---------------------------------------------------------------------------------------------------------
FAKE = 0x10000  # an aligned "device" pointer: validation fails before any device call, so it is never used
I4 = ctypes.c_int32 * 4
VW, VH = 64, 48


def _ptrs(n, frames):
    if isinstance(frames, str):
        return (ctypes.c_void_p * max(n, 1))(*([FAKE] * max(n, 1)))
    return frames


def _frames_valid(n, frames, pitch, width, height):
    if not 1 <= n <= 64 or frames is None or any(not f or f % 2 for f in frames[:n]):
        return False
    return width > 0 and height > 0 and width % 2 == 0 and height % 2 == 0 and pitch >= 2 * width and pitch % 2 == 0


_FRAME_CASES = [dict(n=0), dict(n=65), dict(n=-1), dict(frames=None), dict(frames=(ctypes.c_void_p * 2)(FAKE, None)),
                dict(frames=(ctypes.c_void_p * 2)(FAKE, FAKE + 1)), dict(pitch=2 * VW - 2), dict(pitch=2 * VW + 1), dict(width=0),
                dict(height=-2), dict(width=VW - 1), dict(height=VH + 1), dict(black=None), dict(black=(0, 0, -1, 0)),
                dict(black=(0, 65536, 0, 0)), dict(cell=0), dict(cell=4), dict(cell=512), dict(cell=24), dict(cell=-8), dict(cell=63)]


@pytest.mark.parametrize("kw", _FRAME_CASES + [dict(map=None), dict(map=FAKE + 2), dict(maxv=0), dict(maxv=-1), dict(maxv=65536)])
def test_apply_shading_host_validation(kw):
    a = dict(n=2, frames="ok", pitch=2 * VW, width=VW, height=VH, map=FAKE, cell=8, black=(256,) * 4, maxv=4095)
    a.update(kw)
    fr = _ptrs(a["n"], a["frames"])
    valid = (_frames_valid(a["n"], None if fr is None else list(fr), a["pitch"], a["width"], a["height"])
             and a["cell"] in (8, 16, 32, 64, 128, 256) and bool(a["map"]) and a["map"] % 4 == 0
             and a["black"] is not None and all(0 <= b <= 65535 for b in a["black"]) and 0 < a["maxv"] <= 65535)
    assert not valid, "test bug: these arguments are valid and would reach the device"
    rc = capi.lib().raw["mfsr_applyShading"](a["n"], fr, a["pitch"], a["width"], a["height"], a["map"], a["cell"],
                                             None if a["black"] is None else I4(*a["black"]), a["maxv"], None)
    assert rc == -1


@pytest.mark.parametrize("kw", _FRAME_CASES + [dict(sat=0), dict(sat=-5), dict(sat=65536), dict(sums=None), dict(sums=FAKE + 4),
                                               dict(counts=None), dict(counts=FAKE + 4)])
def test_shading_stats_host_validation(kw):
    a = dict(n=2, frames="ok", pitch=2 * VW, width=VW, height=VH, cell=8, black=(256,) * 4, sat=4095, sums=FAKE, counts=FAKE)
    a.update(kw)
    fr = _ptrs(a["n"], a["frames"])
    valid = (_frames_valid(a["n"], None if fr is None else list(fr), a["pitch"], a["width"], a["height"])
             and a["cell"] in (8, 16, 32, 64, 128, 256) and a["black"] is not None and all(0 <= b <= 65535 for b in a["black"])
             and 0 < a["sat"] <= 65535 and all(bool(a[t]) and a[t] % 8 == 0 for t in ("sums", "counts")))
    assert not valid, "test bug: these arguments are valid and would reach the device"
    rc = capi.lib().raw["mfsr_shadingStats"](a["n"], fr, a["pitch"], a["width"], a["height"], a["cell"],
                                             None if a["black"] is None else I4(*a["black"]), a["sat"], a["sums"], a["counts"], None)
    assert rc == -1


@pytest.mark.parametrize("kw", [dict(sums=None), dict(counts=None), dict(map=None), dict(status=None), dict(gw=0), dict(gh=0), dict(gw=-2),
                                dict(min_quads=0), dict(min_quads=-1), dict(max_gain=65535), dict(max_gain=1048577),
                                dict(bad_sum=-1), dict(bad_sum=2 ** 48), dict(bad_count=-1), dict(bad_count=2 ** 48)])
def test_shading_fit_host_validation(kw):
    a = dict(sums=True, counts=True, map=True, status=True, gw=3, gh=2, min_quads=64, max_gain=MAX_GAIN)
    a.update(kw)
    s, c = np.full((4, 2, 3), 70000, dtype=np.int64), np.full((2, 3), 100, dtype=np.int64)
    if "bad_sum" in a:
        s[2, 1, 1] = a["bad_sum"]
    if "bad_count" in a:
        c[1, 2] = a["bad_count"]
    out, st = np.zeros((4, 2, 3), dtype=np.int32), ctypes.c_int32()
    rc = capi.lib().raw["mfsr_shading_fit"](s.ctypes.data if a["sums"] else None, c.ctypes.data if a["counts"] else None, a["gw"], a["gh"],
                                            a["min_quads"], a["max_gain"], out.ctypes.data if a["map"] else None,
                                            ctypes.byref(st) if a["status"] else None)
    assert rc == -1


def test_burst_correct_shading_host_validation():
    frames = (ctypes.c_void_p * 2)(FAKE, FAKE)
    # without a burst nothing can pass: the call fails on its first check
    assert capi.lib().raw["mfsr_burst_correct_shading"](None, 2, frames, FAKE, 8, None) == -1


# ---- recovery of a synthetic vignette from a flat-field burst ------------------------------------------------------------------
W, H, K = 512, 384, 6
_cache = {}


def flat_fixture():
    """(flat-field frames as uint16 arrays, the vignette as a float64 array [H, W]) of the 8 x 512 x 384 calibration burst."""
    if "flat" not in _cache:
        from multi_frame_super_resolution_amd.synth import make_flat_burst, vignette
        v = vignette(W, H, 0.8, 0.05)
        flat = make_flat_burst(W, H, 8, 0.6, v, alpha=1e-4, beta=1e-6, seed=21)
        _cache["flat"] = ([f.numpy().view(np.uint16).copy() for f in flat], v.numpy())
    return _cache["flat"]


def calibrated_map():
    """(map, status) of the fixture's flat burst under the restatement."""
    if "map" not in _cache:
        flat, _ = flat_fixture()
        _cache["map"] = fit_rule(*stats_rule(flat, K))
    return _cache["map"]


def scene_fixture():
    """(clean, vig, fixed, ground truth [3, sH, sW]) of the 512 x 384 x 6 RGGB scene of the exposure tests: the clean frames, the
    frames seen through the fixture's vignette (multiplied about black in sensor coordinates), and those corrected under the
    restatement with the map calibrated from the flat burst (default cell 64); numpy uint16 arrays [H, W]."""
    if "scene" not in _cache:
        from multi_frame_super_resolution_amd.synth import make_burst
        fr, _, gt = make_burst(W, H, 6, 2, mono=False, seed=11)
        clean = [f.numpy().view(np.uint16).copy() for f in fr]
        _, v = flat_fixture()
        vig = [np.clip(np.round((c.astype(np.float64) - 256) * v + 256), 0, 4095).astype(np.uint16) for c in clean]
        gmap, _ = calibrated_map()
        fixed = [apply_rule(f, gmap, K) for f in vig]
        _cache["scene"] = (clean, vig, fixed, gt)
    return _cache["scene"]


RECOVERY = {6: (0.2598, 0.0703), 3: (0.0396, 0.0047)}   # measured: k -> (worst, mean) of |gain x vignette / (the same at the anchor) - 1|


@pytest.mark.parametrize("k", [6, 3])
def test_flat_burst_recovers_the_vignette(k):
    """gain_at x vignette is constant where the map undoes the lens; the test takes it relative to its value at the anchor.
    Measured on the 8 x 512 x 384 flat burst (level 0.6, noise (1e-4, 1e-6), vignette 1 / (1 + 0.8 r^2)^2 with a +-5 % red / blue
    tilt: 1.7 stops in the corners), worst and mean over the frame:
        cell 64 (the default for this size: a grid of 5 x 4 points)   0.2598   0.0703
        cell 32                                                       0.1351   0.0259
        cell 16                                                       0.0705   0.0086
        cell  8                                                       0.0396   0.0047
    The statistical floor (the noise of a box mean) is below 1e-3 even for the 4 x 4 x 8 quads of a corner box at cell 8.  The
    rest is the cell: bilinear interpolation of a convex gain between grid points 128 samples apart on a frame whose half-diagonal
    is 320, and, larger, the edge boxes -- the box of a grid point on the frame's edge is half a box, so its mean level is the
    level a quarter of a cell inside the frame (worst in the corners, and worst of all where the last grid point lies beyond
    the last quad).  Both shrink in proportion to the cell, as the table shows.  Asserted: three times the measured values."""
    flat, v = flat_fixture()
    assert v.max() == 1.0 and 0.28 < v.min() < 0.34
    sums, counts = stats_rule(flat, k)
    gmap, status = fit_rule(sums, counts)
    if k == K:
        assert np.array_equal(gmap, calibrated_map()[0])
    assert status == 0 and gmap.min() == 65536 and 2 * 65536 < gmap.max() < 4 * 65536     # (the corners: 1.8^2 = 3.24 at the very edge)
    a = int(np.argmax((sums.sum(axis=0) / counts).reshape(-1)))
    ja, ia = divmod(a, counts.shape[1])
    assert abs((ia << k) - W // 4) <= (1 << k) // 2 and abs((ja << k) - H // 4) <= (1 << k) // 2     # the grid point nearest the centre
    prod = gain_at(gmap, W, H, k) / 65536.0 * v
    worst, mean = 0.0, 0.0
    for q in range(4):
        p = prod[(q >> 1)::2, (q & 1)::2]
        rel = np.abs(p / p[ja << k, ia << k] - 1.0)
        worst, mean = max(worst, float(rel.max())), max(mean, float(rel.mean()))
    print(f"recovery at cell {1 << k}: worst deviation {worst:.5f}, mean {mean:.5f}; anchor ({ia}, {ja})")
    assert worst <= 3 * RECOVERY[k][0]
    assert mean <= 3 * RECOVERY[k][1]
