"""Burst noise calibration on the GPU: the tables of mfsr_noiseStatsTemporal against the numpy restatement
(tests/noise_temporal_ref.py) bit for bit on hand-made flow fields at the smallest shapes where the kernel can go wrong, and the
burst driver (mfsr_burst_calibrate_noise_temporal, BurstPipeline.calibrate_noise) against the restatement run on the flows the
burst itself produced, against the true noise model, and for what it leaves behind on the handle."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.noise_temporal_ref import DEFAULT_TOL, calibrate_temporal_rule, stats_temporal_rule
from tests.test_noise_cpu import BLACK, SAT, default_rect, full_rect
from tests.test_noise_temporal_cpu import BURST, MODELS, alpha_bound, burst, oracle_recovery

pytestmark = pytest.mark.gpu

I4 = ctypes.c_int32 * 4
DEV = "cuda:0"
POISON = 777.25          # in every flow texel the rule does not read: half of it is no whole number of quads
SIZES = ((40, 24), (72, 40), (264, 136))


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _frames_dev(host, pad=0, offset=0):
    """u16 arrays [h, w] -> device [h, w] views; pad / offset (samples) make pitched rows and base pointers off the 4- and
    16-byte grids.  Returns (views, backing tensors)."""
    views, backs = [], []
    for a in host:
        h, w = a.shape
        big = torch.full((h, w + pad + offset), 0x5A5A, dtype=torch.int16, device=DEV)
        v = big[:, offset:offset + w]
        v.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV))
        views.append(v)
        backs.append(big)
    return views, backs


def _flows_dev(flows, pad=0):
    """float32 arrays [fh, fw, 2] (or None) -> device views with rows pad texels longer."""
    out = []
    for f in flows:
        if f is None:
            out.append(None)
            continue
        fh, fw = f.shape[:2]
        big = torch.full((fh, fw + pad, 2), 12345.5, dtype=torch.float32, device=DEV)
        big[:, :fw].copy_(torch.from_numpy(np.ascontiguousarray(f)).to(DEV))
        out.append(big[:, :fw])
    return out


def _stats_gpu(dev, dflows, w, h, rect, tol, black=BLACK, sat=SAT):
    from multi_frame_super_resolution_amd import capi
    n = len(dev)
    hist = torch.full((4, 64, 272), -3, dtype=torch.int32, device=DEV)
    ls = torch.full((4, 64), -3, dtype=torch.int64, device=DEV)
    cnt = torch.full((4, 64), -3, dtype=torch.int64, device=DEV)
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in dev])
    fptrs = (ctypes.c_void_p * n)(*[None if f is None else f.data_ptr() for f in dflows])
    given = [f for f in dflows if f is not None]
    fh, fw = (given[0].shape[0], given[0].shape[1]) if given else (h // 2, w // 2)
    fpitch = given[0].stride(0) * 4 if given else 8 * fw
    capi.lib().noiseStatsTemporal(n, ptrs, dev[0].stride(0) * 2, w, h, fptrs, fpitch, fw, fh, I4(*black), sat, I4(*rect), float(tol),
                                  hist.data_ptr(), ls.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hist.cpu().numpy().view(np.uint32), ls.cpu().numpy(), cnt.cpu().numpy()


def _check(host, flows, tol=DEFAULT_TOL, rects=None, black=BLACK, sat=SAT, pad=0, offset=0, fpad=0, min_terms=1):
    """The device tables equal the restatement's for every rectangle; the frames are read only.  Returns the accepted terms of
    the last rectangle (min_terms: what at least the first rectangle must accept, so that no case is vacuous)."""
    h, w = host[0].shape
    dev, backs = _frames_dev(host, pad, offset)
    dflows = _flows_dev(flows, fpad)
    before = [b.clone() for b in backs]
    terms = 0
    for i, rect in enumerate(rects or (full_rect(w, h), default_rect(w, h))):
        want = stats_temporal_rule(host, flows, rect, tol, black, sat)
        got = _stats_gpu(dev, dflows, w, h, rect, tol, black, sat)
        for name, a, b in zip(("hist", "levelSum", "count"), got, want):
            assert np.array_equal(a, b), (name, rect, int((a != b).sum()), int(a.sum()), int(b.sum()))
        terms = int(want[2][0].sum())
        if i == 0:
            assert terms >= min_terms, (terms, min_terms)
    for x, y in zip(before, backs):
        assert torch.equal(x, y)                     # frames (and the bytes around them) are read only
    return terms


def _noise(n, w, h, seed, lo=300, hi=3000):
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, (h, w)).astype(np.uint16) for _ in range(n)]


def _block_flow(w, h, mono, quads):
    """A flow field whose texel of block (bx, by) is 2 * quads[by][bx] (raw pixels; quads: [nby, nbx, 2] float32 in quads, so
    that h = quads exactly), every other texel POISON."""
    fw, fh = (w, h) if mono else (w // 2, h // 2)
    f = np.full((fh, fw, 2), POISON, dtype=np.float32)
    nby, nbx = h // 8, w // 8
    fx = (8 * np.arange(nbx) + 4) * fw // w
    fy = (8 * np.arange(nby) + 4) * fh // h
    with np.errstate(over="ignore", invalid="ignore"):
        f[fy[:, None], fx[None, :]] = np.float32(2.0) * np.asarray(quads, dtype=np.float32).reshape(nby, nbx, 2)
    return f


def _const(w, h, qx, qy):
    q = np.empty((h // 8, w // 8, 2), dtype=np.float32)
    q[..., 0], q[..., 1] = qx, qy
    return q


def _up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


# ---- the tables, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("w,h", SIZES)
def test_translated_frames(w, h, mono):
    """n = 2, 3, 5 frames under whole-quad translations, positive and negative, with s_j.x and s.x odd (A and B off the 16-byte
    grid) and even, on dense and padded pitches, base pointers on the 16-byte grid and 2 bytes off it (the 16-bit-load kernel)."""
    shifts = ((0, 0), (1, -1), (-3, 2), (2, 1), (-1, -2))
    for n in (2, 3, 5):
        host = _noise(n, w, h, 10 * n + w)
        flows = [_block_flow(w, h, mono, _const(w, h, *shifts[k])) for k in range(n)]
        for pad, offset, fpad in ((0, 0, 0), (8, 8, 3), (6, 0, 0), (3, 1, 1)):
            terms = _check(host, flows, pad=pad, offset=offset, fpad=fpad, min_terms=n * (n - 1) // 2)
        assert terms > 0 or (w, h) == (40, 24)         # (the bordered rectangle of the smallest size is 3 x 1 blocks)


@pytest.mark.parametrize("w,h", [(40, 24), (42, 26), (72, 40)])
def test_sites_across_the_four_edges(w, h):
    """Shifts that push A (through s_j) or B (through s) across each edge of the frame, by one quad -- the smallest step a site
    takes -- and by a whole block; at 42 x 26 the last block still fits after one quad and leaves after two.  Every block has its
    own shift, so neighbouring lanes are inside and outside."""
    nby, nbx = h // 8, w // 8
    host = _noise(3, w, h, w + h)
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (2, 0), (0, 2), (4, 0), (-4, 0), (0, 4), (0, -4), (4, 4), (-1, 1)):
        moved = _block_flow(w, h, False, _const(w, h, sx, sy))
        _check(host[:2], [None, moved], min_terms=0)                              # B leaves
        _check(host[:2], [moved, None], min_terms=0)                              # A leaves (and B comes back)
        _check(host, [moved, _block_flow(w, h, False, _const(w, h, 2 * sx, 2 * sy)), None], min_terms=0)
    rng = np.random.default_rng(5)
    q1 = rng.integers(-5, 6, (nby, nbx, 2)).astype(np.float32)
    q2 = rng.integers(-5, 6, (nby, nbx, 2)).astype(np.float32)
    _check(host, [_block_flow(w, h, False, q1), None, _block_flow(w, h, False, q2)], min_terms=1)


@pytest.mark.parametrize("tol", [1.0 / 16.0, 0.125, 0.1, 0.0, 0.25])
def test_residuals_at_the_tolerance(tol):
    """Residuals exactly at tol (accepted), one ulp above it (rejected) and at 0.5 (a tie of roundf: never accepted), on both
    axes and both signs, one residual per block so that the lanes of a wave differ."""
    w, h = 264, 136
    nby, nbx = h // 8, w // 8
    t = np.float32(tol)
    res = [np.float32(0.0), t, -t, _up(t), -_up(t), np.float32(0.5), np.float32(-0.5), np.float32(0.5) * t, _up(np.float32(0.5))]
    q = np.zeros((nby, nbx, 2), dtype=np.float32)
    for by in range(nby):
        for bx in range(nbx):
            i = by * nbx + bx
            q[by, bx] = (np.float32(1.0) + res[i % len(res)], np.float32(-2.0) + res[(i // len(res)) % len(res)])
    host = _noise(3, w, h, 21)
    flow = _block_flow(w, h, False, q)
    terms = _check(host[:2], [None, flow], tol=tol, min_terms=1)
    want = sum(1 for by in range(1, nby - 1) for bx in range(1, nbx - 1)
               if abs(q[by, bx, 0] - np.float32(1.0)) <= t and abs(q[by, bx, 1] + np.float32(2.0)) <= t)
    assert terms == want
    # the same residuals between two moved frames: d = h_k - h_j is a float32 difference
    base = _block_flow(w, h, False, _const(w, h, 2.0, 3.0))
    _check(host, [base, _block_flow(w, h, False, q + np.float32(2.0)), None], tol=tol, min_terms=1)


def test_hostile_flow_texels():
    """NaN, +-inf, 1e9 and values just inside and outside |h| <= 16384 in the texels of some blocks: such a frame is not placed
    there, the pairs of the other frames go on, and no site is derived from the value."""
    w, h = 72, 40
    nby, nbx = h // 8, w // 8
    host = _noise(4, w, h, 33)
    bad = [np.nan, np.inf, -np.inf, 1e9, -1e9, 16384.5, -16385.0, 3.0e38, 16384.0, -16384.0]
    q1, q2 = _const(w, h, 1.0, 0.0), _const(w, h, -1.0, 1.0)
    for i, v in enumerate(bad):
        by, bx = divmod(2 * i + 1, nbx)
        q1[by, bx, i % 2] = v
        q2[nby - 1 - by, nbx - 1 - bx, (i + 1) % 2] = v
    for mono in (False, True):
        flows = [None, _block_flow(w, h, mono, q1), _block_flow(w, h, mono, q2), _block_flow(w, h, mono, _const(w, h, 0.0, -1.0))]
        _check(host, flows, min_terms=6)
    all_bad = _block_flow(w, h, False, _const(w, h, np.nan, 0.0))
    assert _check(host[:2], [None, all_bad], min_terms=0) == 0
    assert _check(host[:3], [None, all_bad, None], min_terms=45) == 21               # frames 0 and 2 still pair, at every block


def test_null_flows_anywhere():
    """A NULL flow at a frame index other than 0, several of them, and all of them."""
    w, h = 72, 40
    host = _noise(5, w, h, 44)
    f1, f2 = _block_flow(w, h, False, _const(w, h, 1.0, 1.0)), _block_flow(w, h, True, _const(w, h, -2.0, 0.0))
    _check(host[:3], [f1, None, f1], min_terms=3)
    _check(host, [f1, f1, None, None, f1], min_terms=10)
    _check(host[:3], [None, None, None], min_terms=3 * 45)
    _check(host[:3], [f2, f2, None], min_terms=3)


@pytest.mark.parametrize("w,h,n", [(264, 136, 5), (520, 264, 4)])
def test_flows_that_vary_from_lane_to_lane(w, h, n):
    """Every block of every frame has its own shift and residual (a rotation looks like this), so the lanes of a wave accept
    different pairs and load from different places; 520 x 264 is 2145 blocks: three workgroups."""
    nby, nbx = h // 8, w // 8
    rng = np.random.default_rng(w)
    host = _noise(n, w, h, 55)
    res = np.array([0.0, 0.0, 0.0625, -0.0625, 0.03, 0.07, -0.2, 0.5, 0.31], dtype=np.float32)
    flows = []
    for k in range(n):
        q = rng.integers(-3, 4, (nby, nbx, 2)).astype(np.float32) + res[rng.integers(0, len(res), (nby, nbx, 2))]
        flows.append(_block_flow(w, h, w == 520, q))
    flows[2] = None
    _check(host, flows, pad=2, offset=1, fpad=1, min_terms=20)
    _check(host, flows, tol=0.25, min_terms=20)


def test_saturation_in_a_only_and_in_b_only():
    """A sample at sat - 1 keeps the pair at the block, a sample at sat drops it, whether it lies in A or in B."""
    w, h = 72, 40
    flow = _block_flow(w, h, False, _const(w, h, 1.0, -1.0))                # B = A's origin + (2, -2)
    base = _noise(2, w, h, 66, 300, 3000)
    full = _check(base, [None, flow], min_terms=1, rects=(full_rect(w, h),))
    a_only = [base[0].copy(), base[1].copy()]
    a_only[0][8, 16] = SAT                                                   # A of block (2, 1); frame 1 untouched
    a_only[0][16, 40] = SAT - 1
    assert _check(a_only, [None, flow], rects=(full_rect(w, h),)) == full - 1
    b_only = [base[0].copy(), base[1].copy()]
    b_only[1][6 + 7, 18] = SAT                                               # last row, first column of B of block (2, 1): origin (18, 6)
    b_only[1][30, 50] = SAT - 1
    assert _check(b_only, [None, flow], rects=(full_rect(w, h),)) == full - 1
    other_sat = [np.minimum(f, 2000) for f in base]
    other_sat[1][20, 30] = 2000                                              # at sat = 2000: dropped; at 2001: kept
    n0 = _check(other_sat, [None, flow], sat=2001, black=(0, 10, 64, 70), rects=(full_rect(w, h),))
    assert _check(other_sat, [None, flow], sat=2000, black=(0, 10, 64, 70), min_terms=0, rects=(full_rect(w, h),)) < n0


def test_the_largest_differences_land_in_the_saturating_bin():
    """Alternating 0 / 65534 samples, inverted in the other frame (the largest values below sat = 65535): every pair difference
    is +-131068, D = 8 * 131068^2 >= 2^36 lies beyond the last bin's range and is counted in bin 271."""
    w, h = 72, 40
    a = np.zeros((h, w), dtype=np.uint16)
    a[:, 0::4] = 65534
    a[:, 1::4] = 65534
    b = (65534 - a.astype(np.int64)).astype(np.uint16)
    assert 8 * 131068 ** 2 >= 1 << 36
    _check([a, b], [None, None], sat=65535, black=(0, 0, 0, 0), min_terms=45)
    hist, _, cnt = stats_temporal_rule([a, b], [None, None], full_rect(w, h), sat=65535, black=(0, 0, 0, 0))
    assert int(hist[:, :, 271].sum()) == 4 * 45 and int(hist[:, :, :271].sum()) == 0
    rng = np.random.default_rng(77)
    wild = [rng.integers(0, 65535, (h, w)).astype(np.uint16) for _ in range(3)]
    _check(wild, [None, _block_flow(w, h, False, _const(w, h, -1.0, 1.0)), None], sat=65535, black=(0, 10, 700, 64), min_terms=45)


def test_more_updates_of_one_key_than_a_16_bit_counter_holds():
    """64 flat identical frames of 56 x 40 with NULL flows: 2016 pairs x 35 blocks = 70 560 updates of one key per position,
    from one workgroup: more than a 16-bit LDS counter holds.  The total is exact and the neighbouring bins stay zero."""
    w, h = 56, 40
    host = [np.full((h, w), 1000, dtype=np.uint16) for _ in range(64)]
    assert 2016 * 35 == 70560 > 65535
    dev, _ = _frames_dev(host)
    hist, ls, cnt = _stats_gpu(dev, [None] * 64, w, h, full_rect(w, h), DEFAULT_TOL)
    lev = (16 * 1000 - 16 * 256) * 64 // (16 * (SAT - 256))
    for q in range(4):
        assert int(hist[q][lev][0]) == 70560 and int(hist[q][lev][1]) == 0 and int(hist[q][lev][136]) == 0
        assert int(hist[q].sum()) == 70560 and int(cnt[q].sum()) == int(cnt[q][lev]) == 70560 and int(ls[q][lev]) == 70560 * 16000
    # two noisy frames alternating: many keys, bins in both halves of a row's words.  The rule is a sum over the pairs, and with
    # 32 copies of X (even indices) and of Y (odd) there are four kinds of pair (A, B): 496 x (X, X), 496 x (Y, Y), 528 x (X, Y)
    # (j = 2a < k = 2b + 1: a <= b) and 496 x (Y, X) -- the restatement of each kind once, times its multiplicity
    rng = np.random.default_rng(88)
    X, Y = (rng.integers(900, 1100, (h, w)).astype(np.uint16) for _ in range(2))
    want = None
    for A, B, times in ((X, X, 496), (Y, Y, 496), (X, Y, 528), (Y, X, 496)):
        t = stats_temporal_rule([A, B], [None, None], full_rect(w, h))
        want = [times * x for x in t] if want is None else [a + times * x for a, x in zip(want, t)]
    assert int(want[2][0].sum()) == 70560
    dev, _ = _frames_dev([X if k % 2 == 0 else Y for k in range(64)])
    got = _stats_gpu(dev, [None] * 64, w, h, full_rect(w, h), DEFAULT_TOL)
    for name, a, b in zip(("hist", "levelSum", "count"), got, want):
        assert np.array_equal(a, b.astype(a.dtype)), name


def test_python_entry_point_checks_and_equals_the_c_abi():
    from multi_frame_super_resolution_amd.pipeline import default_config, noise_fit, noise_stats_temporal
    w, h = 264, 136
    cfg = default_config(w, h, 3, 2, False)
    host = _noise(3, w, h, 99)
    flows = [None, _block_flow(w, h, False, _const(w, h, 1.0, -1.0)), _block_flow(w, h, False, _const(w, h, -2.0, 0.0))]
    dev, _ = _frames_dev(host)
    dflows = _flows_dev(flows)
    st = noise_stats_temporal(dev, dflows, cfg)
    want = stats_temporal_rule(host, flows, default_rect(w, h))
    assert np.array_equal(st.hist.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(st.count.cpu().numpy(), want[2])
    assert np.array_equal(st.level_sum.cpu().numpy(), want[1])
    from tests.noise_temporal_ref import fit_temporal_rule
    got = noise_fit(st, cfg, min_blocks=20, temporal=True)
    ref = fit_temporal_rule(*want, min_blocks=20)
    assert got[2:] == ref[2:] and all(abs(x - y) <= 1e-9 * max(abs(x), abs(y)) for x, y in zip(got[:2], ref[:2]))
    with pytest.raises(ValueError):
        noise_stats_temporal(dev, dflows[:2], cfg)
    with pytest.raises(ValueError):
        noise_stats_temporal(dev, [None, dflows[1].double(), None], cfg)


# ---- the burst driver -----------------------------------------------------------------------------------------------------------
def _cfg():
    from multi_frame_super_resolution_amd.pipeline import default_config
    return default_config(BURST["width"], BURST["height"], BURST["frames"], 2, False)


@functools.lru_cache(maxsize=None)
def _driver(alpha, beta):
    """Everything the driver tests of one noise model share, computed once: the burst, both entry points' answers (twice), the
    restatement on the flows the burst itself produced, the single-frame rule's answer."""
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, calibrate_noise
    host, _ = burst(alpha, beta)
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(DEV) for a in host]
    cfg = _cfg()
    pipe = BurstPipeline(cfg, device=DEV)
    first = pipe.calibrate_noise(dev)
    second = pipe.calibrate_noise(dev)
    # the C entry point, on a handle of its own
    other = BurstPipeline(cfg, device=DEV)
    n = len(dev)
    need = capi.lib().raw["mfsr_noise_temporal_scratch_bytes"](ctypes.byref(cfg), n)
    scratch = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    base = (scratch.data_ptr() + 255) // 256 * 256
    a, b = ctypes.c_double(), ctypes.c_double()
    st, pts, blocks = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_longlong()
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in dev])
    rc = capi.lib().raw["mfsr_burst_calibrate_noise_temporal"](other._h, n, ptrs, 0, 0.0, 0, base, need, ctypes.byref(a), ctypes.byref(b),
                                                               ctypes.byref(st), ctypes.byref(pts), ctypes.byref(blocks),
                                                               torch.cuda.current_stream().cuda_stream)
    c_abi = (rc, a.value, b.value, st.value, pts.value, blocks.value)
    # the flows of the burst itself: mfsr_burst_align_frames on a third handle, as the driver calls it
    third = BurstPipeline(cfg, device=DEV)
    third.begin_burst()
    third.set_reference(dev[0])
    prods = [third.new_frame_products() for _ in range(n - 1)]
    P = ctypes.c_void_p * (n - 1)
    capi.lib().burst_align_frames(third._h, n - 1, P(*[f.data_ptr() for f in dev[1:]]), None, P(*[p[0].data_ptr() for p in prods]),
                                  prods[0][0].stride(0) * 4, P(*[p[1].data_ptr() for p in prods]), prods[0][1].stride(0) * 4,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    flows = [None] + [p[0].cpu().numpy() for p in prods]
    rule = calibrate_temporal_rule(host, flows)
    single = calibrate_noise(dev, cfg)
    return dict(host=host, dev=dev, cfg=cfg, pipe=pipe, first=first, second=second, c_abi=c_abi, rule=rule, single=single)


def _rel(x, y):
    return abs(x - y) <= 1e-9 * max(abs(x), abs(y))


@pytest.mark.parametrize("alpha,beta", MODELS)
def test_driver_equals_the_restatement_on_its_own_flows(alpha, beta):
    d = _driver(alpha, beta)
    ra, rb, rst, rn, rblocks = d["rule"]
    print(f"model ({alpha:g}, {beta:g}): driver {d['first']}  C-ABI {d['c_abi']}  restatement on the burst's flows {d['rule']}")
    for a, b, st, n, blocks in (d["first"], d["c_abi"][1:]):
        assert st == rst == 0 and n == rn and blocks == rblocks
        assert _rel(a, ra) and _rel(b, rb)
    assert d["c_abi"][0] == 0
    assert d["second"] == d["first"]                                   # a second call on the same handle: the same bits


@pytest.mark.parametrize("alpha,beta", MODELS)
def test_driver_recovers_the_model(alpha, beta):
    """alpha within three times the error of the restatement on the CPU oracle's flow fields (at least 5 %), and at least twice as
    close as the single-frame rule on the same frames."""
    d = _driver(alpha, beta)
    bound = alpha_bound(oracle_recovery(alpha, beta)[-1])
    sa, sb, sst = d["single"]
    for a, b, st, n, blocks in (d["first"], d["c_abi"][1:]):
        err = abs(a / alpha - 1)
        serr = abs(sa / alpha - 1)
        print(f"model ({alpha:g}, {beta:g}): alpha {a:.6g} beta {b:.6g} points {n} terms {blocks} error {err:.4f} bound {bound:.4f}; "
              f"single-frame rule: alpha {sa:.6g} beta {sb:.6g} status {sst} error {serr:.4f}")
        assert st == 0 and err <= bound
        assert 2.0 * err <= serr


def test_an_ordinary_burst_on_the_handle_afterwards_is_a_fresh_handles():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    d = _driver(*MODELS[0])
    d["pipe"].calibrate_noise(d["dev"], reference=3)
    got = [t.clone() for t in d["pipe"].process(d["dev"])]
    want = BurstPipeline(d["cfg"], device=DEV).process(d["dev"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for x, y in zip(d["dev"], d["host"]):
        assert np.array_equal(x.cpu().numpy().view(np.uint16), y)       # the frames are read only


def test_refusals_of_the_driver():
    """While frames are pending the call is refused, as the setters are; a scratch that is too small, misaligned or missing, a
    reference outside the burst and a tolerance above 1/4 are refused on the host (the scratch pointer is no device memory)."""
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    d = _driver(*MODELS[0])
    dev, cfg = d["dev"], d["cfg"]
    pipe = BurstPipeline(cfg, device=DEV)
    pipe.begin_burst()
    pipe.set_reference(dev[0])
    pipe.add_frame(dev[1])                                              # waits for its group
    with pytest.raises(capi.MfsrError) as e:
        pipe.calibrate_noise(dev)
    assert e.value.code == -1
    pipe.flush()
    assert pipe.calibrate_noise(dev) == d["first"]                      # between bursts again
    n = len(dev)
    f = capi.lib().raw["mfsr_burst_calibrate_noise_temporal"]
    need = capi.lib().raw["mfsr_noise_temporal_scratch_bytes"](ctypes.byref(cfg), n)
    a, b = ctypes.c_double(), ctypes.c_double()
    st = ctypes.c_int32()
    ptrs = (ctypes.c_void_p * n)(*[x.data_ptr() for x in dev])

    def call(scratch=0x10000, nbytes=need, reference=0, tol=0.0, count=n):
        return f(pipe._h, count, ptrs, reference, tol, 0, scratch, nbytes, ctypes.byref(a), ctypes.byref(b), ctypes.byref(st), None, None,
                 None)

    assert call(nbytes=need - 1) == -1 and call(nbytes=0) == -1
    assert call(scratch=0x10010) == -1 and call(scratch=None) == -1
    assert call(reference=n) == -1 and call(reference=-1) == -1
    assert call(tol=0.26) == -1 and call(tol=float("nan")) == -1
    assert call(count=1) == -1 and call(count=65) == -1
    assert pipe.calibrate_noise(dev) == d["first"]                      # and the handle is as it was


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_noise_burst(tmp_path):
    """MFSR_NOISE=burst measures on the burst being processed through a handle of its own, reports one line on stderr and leaves
    stdout the reference's; with a status other than 0 the defaults stay, so the image is the plain run's; one GPU only."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "apps", "multi_frame_sr")
    assert os.path.exists(cli), "build apps/multi_frame_sr first (__graft_entry__.build())"
    d = tmp_path / "city"
    shutil.copytree(os.path.join(root, "tests", "golden", "city"), d)

    def run(**env):
        return subprocess.run([cli, "farneback", "city", "3"], cwd=d, capture_output=True, text=True, timeout=300,
                              env=dict(os.environ, **env))

    def result():
        return (d / "city_farneback_sr_result.png").read_bytes()

    plain = run()
    assert plain.returncode == 0 and "noise" not in plain.stderr, plain.stderr
    out_plain = result()
    got = run(MFSR_NOISE="burst")
    assert got.returncode == 0, got.stderr
    lines = [ln for ln in got.stderr.splitlines() if ln.startswith("noise: alpha ")]
    assert len(lines) == 1, got.stderr
    print(lines[0])
    words = lines[0].split()
    assert words[3] == "beta" and words[5] == "status" and words[7] == "points" and words[9] == "blocks"
    status, points, blocks = int(words[6]), int(words[8]), int(words[10])
    assert status in (0, 2, 3) and points >= 0 and blocks >= 0
    assert (float(words[2]) == 0.0 and float(words[4]) == 0.0) if status == 2 else blocks > 0
    assert "noise" not in got.stdout and " sec" in got.stdout and " FPS" in got.stdout
    if status != 0:
        assert result() == out_plain                                   # the defaults stayed
    r = run(MFSR_NOISE="burst", MFSR_GPUS="2", MFSR_VIRTUAL_RANKS="1")
    assert r.returncode != 0 and "MFSR_NOISE" in r.stderr, r.stderr
