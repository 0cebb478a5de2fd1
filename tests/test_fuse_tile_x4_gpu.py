"""The x4 warp+fuse tile kernel (accumulate_fast.hip: k_accumulate4xTile) at hostile inputs, in all of its launch forms: one
frame (frame-major, flow as ints), two frames (pixel-major, 16:16-bit flow), three and four frames (pixel-major, 8:8-bit flow
relative to the tile's centre texel, field texels aliased over the weight-sum plane-set), whole-frame and windowed.

Every case runs at 328 x 104 raw, scale 4 (tests/fuse_x4_ref.py: two whole 512-pixel tiles and a ragged one, 208 tile rows)
through mfsr_accumulateSuperResFullN on guarded buffers and, unless it says otherwise, is compared with that many oracle
accumulateSuperResFull calls in the same order at rtol = atol = 3e-5 (the bound of test_accumulate_x4_tile_kernel).  The
frames of a case do not depend on the group's size, so the oracle's accumulators after k frames serve the group of k: they
are computed once per (pattern, kernel field) and kept while that pair is being tested.
tests/test_fuse_tile_x4_cpu.py checks on the CPU that the inputs are what the cases below say they are.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import fuse_x4_ref as fx
from tests.fuse_x4_ref import FH, FW, H, HRH, HRW, W, FlowModel, form_of, live_strips, per_strip, plateau_strips
from tests.kernels import F3, Tex, guarded_upload, pitch_of
from tests.test_fuse_tile_layout_gpu import BLACK, TOL, WHITE, _smooth_kernel_field
from tests.test_parity_kernels import PATTERNS, _accum_inputs, _accumulate_group_hip, _kernel_field, rng

pytestmark = pytest.mark.gpu

S = 4
ACC_SEED = 599


@pytest.fixture(autouse=True)
def _tile_kernel_selected(hip):
    """mfsr_set_accumulate_fast_exp is process-wide and other kernel-level tests leave it at 1: the cases here are about mode 2."""
    hip.L.set_accumulate_fast_exp(2)
    yield
    hip.L.set_accumulate_fast_exp(2)


def _cfa(pat):
    return [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]


@functools.lru_cache(maxsize=None)
def _kp(which):
    # "hostile": NaN and exp-overflow texels (field (0, 0) and (1, 1)); "smooth": positive definite everywhere, so strips are
    # admitted or refused by their flow alone, as the model of fuse_x4_ref.py says
    return _kernel_field(500, FH, FW, 4) if which == "hostile" else _smooth_kernel_field(501, FH, FW)


def _phase_flow(k, alternating):
    """_parity_flow's idea in quarter-pixel steps: 4 * flow is a whole number on every texel, (3 - 5 k, -6 + 3 k), and, if
    alternating, one more on every other texel column (x) / row (y): the rounded flow between two texels takes two values
    inside one wave, so the wave's pixels differ in phase, site parity and, through qy, in the certainty rows they read."""
    yy, xx = np.mgrid[0:FH, 0:FW]
    f4x = 3 - 5 * k + ((xx & 1) if alternating else 0 * xx)
    f4y = -6 + 3 * k + ((yy & 1) if alternating else 0 * yy)
    return np.ascontiguousarray(np.stack([f4x, f4y], -1).astype(np.float32) / np.float32(4.0))


@functools.lru_cache(maxsize=None)
def _plane_masks4():
    """Four certainty fields (52 x 164 x 4, a cell is 8 HR pixels): ones with isolated texels whose three channels all differ, on
    footprint columns 0, 1, 64, 65 of the three tiles (mask column 64 b - 1 + c) and on the first and last rows and the rows
    around the middle of the frame; bands of saturated and random rows; random everywhere; ones."""
    mh, mw = (H + 1) // 2, (W + 1) // 2
    r = rng(530)
    ones = np.ones((mh, mw, 4), np.float32)
    dots = ones.copy()
    for i, gy in enumerate([0, 1, 2, 25, 26, 50, 51]):
        for j, gx in enumerate([0, 63, 64, 65, 127, 128, 129, 163]):
            if (i + j) % 3 != 2:
                dots[gy, gx, :3] = [0.25 + 0.01 * i, 0.5 + 0.01 * j, 0.75 - 0.01 * (i + j)]
    dots[3, 64, 1] = np.nan          # sanitised to 0
    rand = r.random((mh, mw, 4), dtype=np.float32)
    bands = ones.copy()
    rows = (np.arange(mh) // 3) % 2 == 1
    bands[rows] = rand[rows]
    return [dots, bands, r.random((mh, mw, 4), dtype=np.float32), ones]


@functools.lru_cache(maxsize=12)
def _frame(key):
    """(raw, certainty mask, flow) of the frame `key`; the frames are shared between cases and never written."""
    kind = key[0]
    if kind == "phase":      # (a), (f): residue blocks rotated by k, random masks with NaNs
        raw, _, _, mask = _accum_inputs(510 + key[1], W, H, HRW, HRH, nan_frac=0.01)
        flow = fx.residue_flow(key[1])
    elif kind == "plane":    # (b)
        raw, _, _, _ = _accum_inputs(531 + key[1], W, H, HRW, HRH)
        mask = _plane_masks4()[key[1] % 4]
        flow = _phase_flow(key[1] + 1, key[1] & 1)
    elif kind == "edge":     # (c): ("edge", axis, with the two-frame form's extra plateaus)
        raw, _, _, mask = _accum_inputs(551 + key[1], W, H, HRW, HRH, nan_frac=0.01)
        flow = fx.edge_flow(key[1], fx.EDGE_D2 if key[2] else fx.EDGE_D, patches=key[1] == 1)
    elif kind == "far":      # (c): ("far", which, sign)
        raw, _, _, mask = _accum_inputs(553 + key[1], W, H, HRW, HRH, nan_frac=0.01)
        flow = fx.far_flow(key[1], key[2])
    elif kind == "site":     # (d)
        raw, _, _, mask = _accum_inputs(571 + key[1], W, H, HRW, HRH, nan_frac=0.01)
        flow = fx.const_flow(*fx.SITE_SHIFTS[key[1]])
    elif kind == "refused":  # (e)
        raw, _, _, mask = _accum_inputs(591 + key[1], W, H, HRW, HRH, nan_frac=0.01)
        flow = fx.refused_group_flow(key[1])
    else:
        raise KeyError(key)
    return raw, np.ascontiguousarray(mask), np.ascontiguousarray(flow.astype(np.float32))


_chain = {"root": None, "states": {}}


def _oracle_after(orc, pat, kpk, keys):
    """The oracle's accumulators after the frames `keys` in this order, from the accumulators of ACC_SEED.  Prefixes are kept
    while (pat, kpk) stays the same; nobody writes to what this returns."""
    if _chain["root"] != (pat, kpk):
        _chain.update(root=(pat, kpk), states={})
    st = _chain["states"]
    if keys not in st:
        if not keys:
            _, oi, ow, _ = _accum_inputs(ACC_SEED, W, H, HRW, HRH)
        else:
            pi, pw = _oracle_after(orc, pat, kpk, keys[:-1])
            oi, ow = pi.copy(), pw.copy()
            raw, m, sh = _frame(keys[-1])
            orc.set_cfa(_cfa(pat))
            orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(_kp(kpk)), Tex(sh), F3(WHITE), F3(BLACK), W, H, S, pitch_of(oi), pitch_of(m))
        st[keys] = (oi, ow)
    return st[keys]


def _group_hip(hip, pat, kpk, keys, acc_i, acc_w, fresh=0):
    hip.set_cfa(_cfa(pat))
    return _accumulate_group_hip(hip, [_frame(k) for k in keys], _kp(kpk), FW, FH, W, H, S, F3(WHITE), F3(BLACK), acc_i, acc_w, fresh)


def _run(orc, hip, pat, kpk, keys):
    keys = tuple(keys)
    hi0, hw0 = _oracle_after(orc, pat, kpk, ())
    oi, ow = _oracle_after(orc, pat, kpk, keys)
    hi, hw_ = _group_hip(hip, pat, kpk, keys, hi0, hw0)
    for name, got, ref in (("weights", hw_, ow), ("values", hi, oi)):
        with np.errstate(invalid="ignore"):
            excess = np.abs(got - ref) / (TOL["atol"] + TOL["rtol"] * np.abs(ref))
        print(f"{pat} {keys}: {name}: largest error {np.nanmax(excess):.3f} of the bound")
    np.testing.assert_allclose(hw_, ow, **TOL)
    np.testing.assert_allclose(hi, oi, **TOL)
    assert np.nanmax(np.abs(hw_ - hw0)) > 0.5   # the launch accumulated something


# ---- (a) every (position in cell, phase of the first tap) pair --------------------------------------------------------
PHASE_CASES = [(n, pat) for pat in ("RGGB", "BGGR", "GRBG", "GBRG") for n in (1, 2, 3, 4)] + [(1, "MONO"), (4, "MONO")]


@pytest.mark.parametrize("n,pat", PHASE_CASES)
def test_phase_coverage(orc, hip, n, pat):
    """Residue blocks: among the admitted strips every (X & 7, qx & 7) and (Y & 7, qy & 7) pair occurs, and the frames of a
    group disagree about the phase: the K8 bodies, mx[] / my[] / flip, the raw site parity and the mask row of every tap row."""
    _run(orc, hip, pat, "hostile", [("phase", k) for k in range(n)])


# ---- (b) certainty addressing -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pat", [(n, pat) for pat in ("RGGB", "GBRG", "BGGR") for n in (1, 2, 3, 4)])
def test_plane_addressing(orc, hip, n, pat):
    """Texels whose channels all differ on the first and last columns of each tile's 66-column footprint: a read from the wrong
    cell, mask row, channel or frame cannot pass.  Frame k takes mask k of (dots, bands, random, ones)."""
    _run(orc, hip, pat, "hostile", [("plane", k) for k in range(n)])


# ---- (c) the admission window ------------------------------------------------------------------------------------------
EDGE_CASES = [(n, pat, sign) for pat in ("RGGB", "GBRG") for n in (2, 3, 4) for sign in (1, -1)]


@pytest.mark.parametrize("n,pat,sign", EDGE_CASES)
def test_admission_edge(orc, hip, n, pat, sign):
    """Frame 0 has whole strips at d = 127, 128, -128, -129 HR pixels from the tile's own flow in x, frame 1 in y (and a NaN and
    a 1e9 patch); the two-frame form, whose bound is +-2^15, gets +-127, +-128 and +-129 and admits them all.  Frames 2 and 3 sit
    as a whole on the clamp of the tile's own flow (4 * flow = +-32000, -+32001): every strip of theirs is refused, and they
    still contribute, through the straight arithmetic."""
    if n == 2:
        keys = [("edge", 0, True), ("edge", 1, True)]
    else:
        keys = [("edge", 0, False), ("edge", 1, False), ("far", 0, sign), ("far", 1, sign)][:n]
    _run(orc, hip, pat, "smooth", keys)


# ---- (d) raw sites on the frame's first and last admitted row and column ---------------------------------------------
@pytest.mark.parametrize("pat,n,first", [("RGGB", 1, 0), ("RGGB", 2, 0), ("RGGB", 4, 0), ("GRBG", 1, 1), ("BGGR", 2, 2)])
def test_raw_sites_at_the_frame_edges(orc, hip, pat, n, first):
    """Frame k's flow is SITE_SHIFTS[first + k]: (-3.5, -3.5) puts the first raw site of the first live pixel on column / row 0,
    (3.5, 3.5) the last site of the last live pixel on 4 W - 5 / 4 H - 5; (-3.75, 3.5) and (3.75, -3.75) refuse the outermost
    strips.  The raw frames sit between guards of 0xFFFF: a read one row or column outside poisons the result."""
    _run(orc, hip, pat, "smooth", [("site", first + k) for k in range(n)])


# ---- (e) the fast path ran, and a refused strip is the straight arithmetic ---------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4])
def test_fast_path_ran_and_refusals_are_the_straight_arithmetic(hip, n):
    """The group of fuse_x4_ref.refused_group_flow through the tile kernel (mode 2) and through the straight kernel frame by
    frame (mode 1): the strips the model says are refused in every frame are bit-equal (the same accumulate_pixel_core calls
    in the same order), every plateau that some frame admits holds a value that differs (the tile kernel re-associates the
    sums), and so does the live area at large.  A kernel that refused everything would be bit-equal everywhere."""
    keys = tuple(("refused", k) for k in range(n))
    _, i0, w0, _ = _accum_inputs(ACC_SEED, W, H, HRW, HRH)
    ti, tw = _group_hip(hip, "RGGB", "smooth", keys, i0, w0)
    hip.L.set_accumulate_fast_exp(1)
    try:
        si, sw = _group_hip(hip, "RGGB", "smooth", keys, i0, w0)
    finally:
        hip.L.set_accumulate_fast_exp(2)
    np.testing.assert_allclose(tw, sw, **TOL)
    np.testing.assert_allclose(ti, si, **TOL)

    live = live_strips()
    ms = [FlowModel(_frame(k)[2]) for k in keys]
    some = np.any([m.admitted(form_of(n)) for m in ms], axis=0) & live
    clear = np.min([per_strip(m.tie).min(-1) for m in ms], axis=0) >= 1.0 / 32   # no pixel of the strip near a rounding tie
    never = ~some & live & clear
    same = per_strip((ti.view(np.uint32) == si.view(np.uint32)).all(-1) & (tw.view(np.uint32) == sw.view(np.uint32)).all(-1)).all(-1)
    print(f"group of {n}: {never.sum()} strips refused in every frame, {(~same & never).sum()} of them differ; "
          f"{some.sum()} strips admitted in some frame, {(~same & some).sum()} of them differ")
    assert never.sum() >= 200 and same[never].all()
    assert (~same & some).any()
    refused_plateaus = 0
    for axis in range(2):
        for d in fx.EDGE_D:
            s = plateau_strips(fx.BLOCKS[axis][d]) & live
            if never[s].all():
                refused_plateaus += 1
            else:
                assert some[s].all() and not same[s].all(), (axis, d)
    assert refused_plateaus == (0 if n == 1 else 4)


# ---- (f) windows at the kernel level -----------------------------------------------------------------------------------
WINDOWS = [(496, 0, 32, 48),        # straddles the tile boundary at 512 and the top margin band
           (0, 16, 16, 32),         # the left margin ring only, no tile pixel
           (1008, 384, 304, 32),    # across 1024 into the ragged tile, right margin and bottom band
           (512, 208, 512, 16),     # exactly one tile, one band
           (16, 16, 1280, 384),     # the live area exactly
           (0, 0, HRW, HRH)]        # the whole frame


@pytest.mark.parametrize("undefined", [0, 1])
@pytest.mark.parametrize("n,pat", [(1, "RGGB"), (2, "RGGB"), (3, "RGGB"), (4, "RGGB"), (4, "GBRG")])
def test_kernel_window_against_cropped_full(hip, n, pat, undefined):
    """mfsr_accumulateSuperResFullWindow at scale 4 on the frames of test_phase_coverage, bit for bit the crop of
    mfsr_accumulateSuperResFullN of the same frames.  The window buffer has a pitch of 12 w + 80 bytes and three guard rows
    filled with a canary (a NaN): no byte outside the window may change.  undefined = 0: the accumulators hold values (the
    window buffer their crop); 1: the whole-frame call starts from zeros and the window buffer is canary throughout."""
    import torch
    keys = tuple(("phase", k) for k in range(n))
    _, i0, w0, _ = _accum_inputs(ACC_SEED, W, H, HRW, HRH)
    if undefined:
        i0, w0 = np.zeros_like(i0), np.zeros_like(w0)
    full = [torch.from_numpy(a) for a in _group_hip(hip, pat, "hostile", keys, i0, w0)]
    init = [torch.from_numpy(i0), torch.from_numpy(w0)]

    checks = []

    def gup(a):
        t, c = guarded_upload(a, hip.dev)
        checks.append(c)
        return t

    frames = [_frame(k) for k in keys]
    d_raw, d_mask, d_sh = [gup(f[0]) for f in frames], [gup(f[1]) for f in frames], [gup(f[2]) for f in frames]
    d_kp = gup(_kp("hostile"))
    P = ctypes.c_void_p * n
    raws, masks = P(*[t.data_ptr() for t in d_raw]), P(*[t.data_ptr() for t in d_mask])
    flows = (hip.capi.Tex2D * n)(*[hip.capi.Tex2D(t.data_ptr(), FW * 8, FW, FH) for t in d_sh])
    kp = hip.capi.Tex2D(d_kp.data_ptr(), FW * 16, FW, FH)
    white, black = hip.capi.f3(F3(WHITE).v), hip.capi.f3(F3(BLACK).v)
    hip.set_cfa(_cfa(pat))
    for x, y, w, h in WINDOWS:
        guard, padf = 3, 20  # rows before / after, extra floats per row (pitch 12 w + 80 bytes)
        pitchf = 3 * w + padf
        canary = torch.full(((h + 2 * guard) * pitchf,), 0x7FC0BEEF, dtype=torch.int32)
        buf = [canary.clone(), canary.clone()]
        if not undefined:
            for bb, a in zip(buf, init):
                bb.view(h + 2 * guard, pitchf)[guard:guard + h, :3 * w] = a[y:y + h, x:x + w].reshape(h, 3 * w).view(torch.int32)
        before = [bb.clone() for bb in buf]
        dev = [bb.to(hip.dev) for bb in buf]
        ptr = [bb.data_ptr() + guard * pitchf * 4 for bb in dev]
        hip.L.accumulateSuperResFullWindow(n, raws, ptr[0], ptr[1], masks, kp, flows, white, black, W, H, S, pitchf * 4,
                                           pitch_of(frames[0][1]), undefined, x, y, w, h, None)
        torch.cuda.synchronize()
        for bb, b0, whole in zip(dev, before, full):
            g = bb.cpu().view(h + 2 * guard, pitchf)
            inside = g[guard:guard + h, :3 * w]
            assert torch.equal(inside, whole[y:y + h, x:x + w].reshape(h, 3 * w).view(torch.int32)), (x, y, w, h)
            outside = torch.ones_like(g, dtype=torch.bool)
            outside[guard:guard + h, :3 * w] = False
            assert torch.equal(g[outside], b0.view(h + 2 * guard, pitchf)[outside]), ("bytes outside the window changed", x, y, w, h)
    for i, c in enumerate(checks):
        c(f"mfsr_accumulateSuperResFullWindow, input {i}", unchanged=True)
