"""The CPU oracle pinned to the reference's own kernels, compiled for the host.

``oracle/_ref/libmfsr_ref.so`` holds the reference's five ``.cu`` files compiled by g++ through the stand-in
headers of ``oracle/refshim/`` (one host call per GPU thread, the launch shape and the texture modes as parameters).
Every kernel the oracle restates is run here on the same seeded inputs by both, the hostile cases of
``tests/test_parity_kernels.py`` included.  The expectation is BIT FOR BIT, transcendentals included: both sides are
compiled by the same compiler with contraction off against the same libm.  No tolerance appears in this file except

  * the ``fixed8`` texture variant (documentation of the distance between the canonical float bilinear filter and
    CUDA's 8-bit interpolation weights), whose bound is derived next to the assertion;
  * pixels whose flow fetch is NaN: converting NaN to int is undefined on the host (the reference does it in plain
    C++, x86 yields INT_MIN) and defined on the device (0, PTX cvt.rzi), which the oracle follows; those pixels are
    left out of the comparison, located from the INPUT alone.

Every output lives inside a larger array filled with a canary that must survive both calls.
"""
import inspect
import subprocess
import sys

import numpy as np
import pytest

from tests.guards import Guard
from tests.kernels import F2, F3, RefBackedOracle, Tex, load_ref_or_skip, pitch_of
from tests.test_parity_kernels import (PATTERNS, RGGB, _accum_inputs, _design, _kernel_field, _paraboloid, _smooth_image, _tiles,
                                       assert_bitexact, rng)

MONO = [1, 1, 1, 1]
ALL_CFA = dict(PATTERNS, MONO=MONO)
BLOCKS_2D = [(16, 16, 1), (32, 8, 1)]
BLOCKS_1D = [(64, 1, 1), (7, 1, 1)]
BLOCKS_TILE = [(8, 8, 2), (16, 4, 1)]
TS_PAIRS = [(16, 3), (32, 4), (32, 8)]


@pytest.fixture(scope="module")
def ref():
    return load_ref_or_skip()


def pin(orc, ref, fname, make, blocks=(None,), keep=None, **kw):
    """make(guard) -> (args, outputs).  The oracle once, the reference once per block shape; outputs bit-identical
    (where ``keep`` is given, on those elements only) and every canary intact.  Returns the oracle's outputs."""
    g = Guard()
    args, outs = make(g)
    orc.call(fname, *args)
    g.check(f"{fname} (oracle)")
    want = [o.copy() for o in outs]
    for b in blocks:
        g = Guard()
        args, outs = make(g)
        ref.call(fname, *args, block=b, **kw)
        g.check(f"{fname} (reference, block {b})")
        for i, (w, o) in enumerate(zip(want, outs)):
            if keep is not None:
                w, o = w[keep], o[keep]
            assert_bitexact(w, o, f"{fname} output {i}, block {b}")
    return want


# ---------------------------------------------------------------- A: DeBayer
@pytest.mark.parametrize("pat", list(ALL_CFA))
@pytest.mark.parametrize("shape", [(32, 32), (48, 64), (19, 27)])
def test_deBayersSubSample3(orc, ref, pat, shape):
    hh, hw = shape
    orc.set_cfa(ALL_CFA[pat])
    ref.set_cfa(ALL_CFA[pat])

    def make(g):
        raw = rng(1).integers(0, 4096, (2 * hh, 2 * hw), dtype=np.uint16)
        out = g.zeros((hh, hw + 3, 3))  # odd pitch
        return (raw, out, 4095.0, hw, hh, pitch_of(out)), [out]

    (o,) = pin(orc, ref, "deBayersSubSample3", make, BLOCKS_2D)
    assert o[:, :hw].max() > 0


@pytest.mark.parametrize("pat", list(ALL_CFA))
@pytest.mark.parametrize("size", [(40, 72), (37, 51)])
def test_deBayer_green_then_redblue(orc, ref, pat, size):
    H, W = size
    orc.set_cfa(ALL_CFA[pat])
    ref.set_cfa(ALL_CFA[pat])
    bp = F3([256, 250, 260])
    sc = F3([1 / 3839.0, 1 / 3800.0, 1 / 3850.0])
    rawf = np.zeros((H, W + 3), np.float32)   # padded pitch
    rawf[:, :W] = rng(2).integers(200, 4096, (H, W), dtype=np.uint16)
    res = []
    for k, blocks in ((orc, [None]), (ref, BLOCKS_2D)):
        for b in blocks:
            g = Guard()
            out = g.zeros((H, W + 1, 3))
            kw = {} if k is orc else {"block": b}
            k.call("deBayerGreenKernel", W, H, rawf, pitch_of(rawf), out, pitch_of(out), bp, sc, **kw)
            green = out.copy()
            k.call("deBayerRedBlueKernel", W, H, rawf, pitch_of(rawf), out, pitch_of(out), bp, sc, **kw)
            g.check("deBayer chain")
            res.append((green, out.copy()))
    for green, full in res[1:]:
        assert_bitexact(res[0][0], green, "deBayerGreenKernel")
        assert_bitexact(res[0][1], full, "deBayerRedBlueKernel")
    assert (res[0][1][:2] == 0).all() and (res[0][1][:, :2] == 0).all() and res[0][1].max() > 0


# ---------------------------------------------------------------- G: accumulate
def _nan_footprint(n_out, pos, n_tex, bad):
    """Output indices whose linear-filter footprint along one axis touches a texel in ``bad`` (widened by one)."""
    xb = np.asarray(pos, np.float64) * n_tex - 0.5
    lo = np.floor(xb)
    hit = np.isin(np.clip(lo, 0, n_tex - 1), bad) | np.isin(np.clip(lo + 1, 0, n_tex - 1), bad)
    wide = hit.copy()
    wide[1:] |= hit[:-1]
    wide[:-1] |= hit[1:]
    assert wide.shape == (n_out,)
    return wide


@pytest.mark.parametrize("pat", list(ALL_CFA))
def test_accumulateImagesSuperRes(orc, ref, pat):
    """The x2 centre-crop kernel: NaN certainties, NaN / overflowing kernel parameters (the non-finite-weight rule), a wild
    flow patch (1e9: 2e9 still converts to int) and a NaN flow texel (left out, see the module docstring)."""
    W, H = 96, 64
    orc.set_cfa(ALL_CFA[pat])
    ref.set_cfa(ALL_CFA[pat])
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    fh, fw = H // 2 + 1, W // 2 + 3   # a field that is not the image's size
    ty, tx = 20, 23

    def make(g):
        raw, imgOut, tw, mask = _accum_inputs(3, W, H, W, H, nan_frac=0.01)
        kp = _kernel_field(4, fh, fw, 4)
        # the crop reads the central half of the field: hostile parameters there (exp overflow -> inf, NaN, inf)
        kp[fh // 2, fw // 2, :3] = [-50, -50, 0]
        kp[fh // 2 + 3, fw // 2 - 4, :3] = np.nan
        kp[fh // 2 - 5, fw // 2 + 5, :3] = [np.inf, 1, 0]
        sh = rng(5).uniform(-3, 3, (fh, fw, 2)).astype(np.float32)
        sh[10:14, 10:14] = 1e9
        sh[ty, tx] = np.nan
        imgOut, tw = g.new(imgOut), g.new(tw)
        return (raw, imgOut, tw, mask, Tex(kp), Tex(sh), white, black, W, H, pitch_of(imgOut), pitch_of(mask)), [imgOut, tw]

    posx = (np.arange(W) + 0.5 + W // 2) / 2.0 / W
    posy = (np.arange(H) + 0.5 + H // 2) / 2.0 / H
    bad = _nan_footprint(H, posy, fh, [ty])[:, None] & _nan_footprint(W, posx, fw, [tx])[None, :]
    assert 0 < bad.sum() < 200
    oi, ow = pin(orc, ref, "accumulateImagesSuperRes", make, BLOCKS_2D, keep=~bad)
    _, i0, w0, _ = _accum_inputs(3, W, H, W, H, nan_frac=0.01)
    assert np.abs(ow - w0).max() > 0.5 and np.isfinite(ow[~bad]).all()
    assert_bitexact(oi[0], i0[0])            # ring untouched


@pytest.mark.parametrize("pat", ["GRBG", "RGGB", "MONO"])
def test_accumulateSuperResFull_x2_equals_the_reference_crop_kernel(orc, ref, pat):
    """The oracle's full-frame generalisation (scale s, no reference line) at s = 2 against the reference's centre-crop kernel
    where the two geometries coincide: HR pixel X = x + dimX/2 whose raw and certainty sites stay inside the crop's clamp range
    [dimX/4, dimX/4 + dimX/2 - 1] for every tap and every flow of the field (|round(2u)| <= smax) -- there truncating and floor
    division agree as well.  Scales 1, 3 and 4 of that function have no reference kernel (x1 is accumulateImages, below)."""
    W, H = 64, 48
    orc.set_cfa(ALL_CFA[pat])
    ref.set_cfa(ALL_CFA[pat])
    white, black = F3([3839, 3700, 3900]), F3([256, 260, 250])
    raw, full_i, full_w, mask = _accum_inputs(8, W, H, 2 * W, 2 * H, nan_frac=0.01)
    kp = _kernel_field(7, H // 2, W // 2, 4)
    kp[H // 4, W // 4, :3] = [-50, -50, 0]      # inside the compared region: exp overflow -> inf -> axis rule
    kp[H // 4 + 2, W // 4 - 3, :3] = np.nan
    sh = rng(8).uniform(-4, 4, (H // 2, W // 2, 2)).astype(np.float32)
    y0, x0 = H // 2, W // 2
    g = Guard()
    ci, cw = g.new(full_i[y0:y0 + H, x0:x0 + W]), g.new(full_w[y0:y0 + H, x0:x0 + W])
    ref.call("accumulateImagesSuperRes", raw, ci, cw, mask, Tex(kp), Tex(sh), white, black, W, H, pitch_of(ci), pitch_of(mask))
    g.check("accumulateImagesSuperRes")
    g = Guard()
    oi, ow = g.new(full_i), g.new(full_w)
    orc.call("accumulateSuperResFull", raw, oi, ow, mask, Tex(kp), Tex(sh), white, black, W, H, 2, pitch_of(oi), pitch_of(mask))
    g.check("accumulateSuperResFull")
    smax = int(np.ceil(2 * np.abs(sh).max())) + 1

    def valid(n):   # crop coordinate x, HR coordinate X = x + n/2
        X = np.arange(n) + n // 2
        lo, hi = 2 * (n // 4), 2 * (n // 4 + n // 2) - 1
        return (X - 2 - smax >= lo) & (X + 2 + smax <= hi) & (np.arange(n) >= 1) & (np.arange(n) < n - 1)

    keep = valid(H)[:, None] & valid(W)[None, :]
    assert keep.mean() > 0.25
    assert_bitexact(oi[y0:y0 + H, x0:x0 + W][keep], ci[keep], "accumulateSuperResFull x2 image")
    assert_bitexact(ow[y0:y0 + H, x0:x0 + W][keep], cw[keep], "accumulateSuperResFull x2 weights")
    assert np.abs(cw[keep] - full_w[y0:y0 + H, x0:x0 + W][keep]).max() > 0.5


@pytest.mark.parametrize("pat", ["RGGB", "BGGR", "MONO"])
def test_accumulateImages(orc, ref, pat):
    W, H = 64, 40
    orc.set_cfa(ALL_CFA[pat])
    ref.set_cfa(ALL_CFA[pat])
    white, black = F3([3839, 3839, 3839]), F3([256, 256, 256])

    def make(g):
        raw, imgOut, tw, mask = _accum_inputs(9, W, H, W, H, nan_frac=0.01)
        kp = _kernel_field(10, H, W, 3)
        sh = rng(11).uniform(-3, 3, (H, W, 2)).astype(np.float32)
        sh[5, 5] = [300, -300]     # far outside: clamped sites
        imgOut, tw = g.new(imgOut), g.new(tw)
        return (raw, imgOut, tw, mask, kp, sh, white, black, W, H, pitch_of(imgOut), pitch_of(mask), pitch_of(sh)), [imgOut, tw]

    pin(orc, ref, "accumulateImages", make, BLOCKS_2D)


# ---------------------------------------------------------------- B: tile tracker
@pytest.mark.parametrize("T,S", TS_PAIRS)
def test_squaredSum_boxFilters_normalizedCC(orc, ref, T, S):
    n = 5
    L, R = T + 2 * S, 2 * S + 1

    def mk_sq(g):
        out = g.zeros(n)
        return (_tiles(20, n, T, S), out, S, T, n), [out]

    pin(orc, ref, "squaredSum", mk_sq, BLOCKS_1D)
    for which, blocks in (("boxFilterWithBorderX", [(L, 1, 1), (L, 1, 2)]), ("boxFilterWithBorderY", [(1, L, 1), (1, L, 2)])):
        def mk_box(g):
            out = g.new(np.full((n, L, L), -1, np.float32))
            return (_tiles(21, n, T, S), out, S, T, n), [out]

        pin(orc, ref, which, mk_box, blocks)

    def mk_ncc(g):
        out = g.zeros((n, R, R))
        return (_tiles(22, n, T, S) * 30, rng(24).random(n, dtype=np.float32) * 50, _tiles(25, n, T, S) * 50, out, S, T, n), [out]

    pin(orc, ref, "normalizedCC", mk_ncc, BLOCKS_TILE)


@pytest.mark.parametrize("rot", [0.0, 0.05])
@pytest.mark.parametrize("T,S", TS_PAIRS)
def test_convertToTiles(orc, ref, T, S, rot):
    """Odd image size, padded pitch, tiles that reach over every image border (clamped), pre-shifts with exact .5 fractions."""
    W, H = 100, 70
    tcx, tcy = W // T, H // T
    L = T + 2 * S
    img = np.zeros((H, W + 5), np.float32)
    img[:, :W] = rng(26).random((H, W), dtype=np.float32)
    base = F2([1.3, -0.7] if rot else [0, 0])

    def mk_b(g):
        out = g.new(np.full((tcx * tcy, L, L), -1, np.float32))
        return (img, out, W, H, pitch_of(img), S, T, tcx, tcy, base, rot), [out]

    pin(orc, ref, "convertToTilesOverlapBorder", mk_b, BLOCKS_TILE)
    pre = np.zeros((tcy, tcx + 1, 2), np.float32)
    pre[:, :tcx] = rng(27).uniform(-4, 4, (tcy, tcx, 2))
    pre[0, 0] = [2.5, -3.5]        # roundf ties
    pre[-1, -2] = [40.0, 60.0]     # far outside the image

    def mk_p(g):
        out = g.new(np.full((tcx * tcy, L, L), -1, np.float32))
        return (img, out, pre, pitch_of(pre), W, H, pitch_of(img), S, T, tcx, tcy, base, rot), [out]

    pin(orc, ref, "convertToTilesOverlapPreShift", mk_p, BLOCKS_TILE)


def test_findMinimum(orc, ref):
    S = 4
    R = 2 * S + 1
    tcx, tcy = 5, 3
    n = tcx * tcy
    imgs = rng(28).random((n, R, R), dtype=np.float32) * 10
    imgs[0] = _paraboloid(S, 1.3, -0.6)[0]          # analytic interior minimum
    imgs[1] = 1.0                                    # flat tile
    imgs[2] = _paraboloid(S, 4.0, 0.0)[0]            # minimum on the border ring
    imgs[3, 2, 2] = imgs[3, 5, 5] = -5.0             # tie: the first strict minimum wins
    imgs[4] = np.nan                                 # all NaN
    imgs[5, 1, 1] = -9.0                             # minimum on the first interpolable ring
    imgs[6, R - 2, R - 2] = -9.0                     # ... and on the last
    imgs[7, 0, 3] = -9.0                             # first row
    imgs[8, 4, 4] = np.nan                           # NaN next to the minimum
    imgs[8, 4, 5] = -9.0
    imgs[9] = _paraboloid(S, 0.0, 0.0)[0] * 0 + 3    # flat, then a saddle around the centre: detA < 0
    imgs[9, 4, 4], imgs[9, 4, 3], imgs[9, 4, 5], imgs[9, 3, 4], imgs[9, 5, 4] = 1.0, 5.0, 5.0, 1.5, 1.5
    for thr in (0.0, 20.0, 0.5):
        def make(g):
            out = g.new(np.full((tcy, tcx + 1, 2), 7, np.float32))
            return (imgs.copy(), out, pitch_of(out), S, n, tcx, thr), [out]

        (o,) = pin(orc, ref, "findMinimum", make, BLOCKS_1D)
    np.testing.assert_allclose(o[0, 0], [1.3, -0.6], atol=0.05)
    assert (o[0, 1] == 0).all() and (o[0, 2] == 0).all() and (o[0, 3] != 0).any()


def test_UpSampleShifts(orc, ref):
    for (ocx, ocy, ncx, ncy, oldL, newL, oldT, newT) in [(7, 5, 15, 11, 4, 2, 16, 16), (5, 3, 5, 3, 2, 1, 16, 32), (3, 2, 13, 9, 4, 1, 32, 32)]:
        inS = np.zeros((ocy, ocx + 2, 2), np.float32)
        inS[:, :ocx] = rng(29).uniform(-5, 5, (ocy, ocx, 2))

        def make(g):
            out = g.zeros((ncy, ncx + 1, 2))
            return (inS, out, pitch_of(inS), pitch_of(out), oldL, newL, ocx, ocy, ncx, ncy, oldT, newT), [out]

        pin(orc, ref, "UpSampleShifts", make, BLOCKS_2D)


@pytest.mark.parametrize("T,S", TS_PAIRS)
def test_tile_tracker_chain(orc, ref, T, S):
    """B1, B2, B3, B4x, B4y, B6, B7 chained (the correlation itself has no reference kernel: the oracle's for both), then B8
    on the result: every intermediate bit-identical, with the shapes SURVEY documents for the kernels that tie the block to
    the tile."""
    W, H = 160, 96
    tcx, tcy = W // T, H // T
    n, L, R = tcx * tcy, T + 2 * S, 2 * S + 1
    r = rng(30)
    base = r.random((H + 16, W + 16), dtype=np.float32)
    refimg = np.ascontiguousarray(base[8:8 + H, 8:8 + W])
    mov = np.ascontiguousarray(base[6:6 + H, 9:9 + W])
    pre = r.uniform(-1.4, 1.4, (tcy, tcx, 2)).astype(np.float32)
    z = F2([0, 0])
    got = {}
    for k in (orc, ref):
        g = Guard()
        rt, mt, cc, bx, by = (g.zeros((n, L, L)) for _ in range(5))
        sq, dist, coord = g.zeros(n), g.zeros((n, R, R)), g.zeros((tcy, tcx, 2))
        up = g.zeros((2 * tcy, 2 * tcx, 2))
        kx, ky = ({}, {}) if k is orc else ({"block": (L, 1, 1)}, {"block": (1, L, 1)})
        k.call("convertToTilesOverlapBorder", refimg, rt, W, H, pitch_of(refimg), S, T, tcx, tcy, z, 0.0)
        k.call("convertToTilesOverlapPreShift", mov, mt, pre, pitch_of(pre), W, H, pitch_of(mov), S, T, tcx, tcy, z, 0.0)
        orc.call("crossCorrelateTiles", rt, mt, cc, S, T, n)
        k.call("squaredSum", rt, sq, S, T, n)
        k.call("boxFilterWithBorderX", mt, bx, S, T, n, **kx)
        k.call("boxFilterWithBorderY", bx, by, S, T, n, **ky)
        k.call("normalizedCC", cc, sq, by, dist, S, T, n)
        k.call("findMinimum", dist, coord, pitch_of(coord), S, n, tcx, 0.0)
        k.call("UpSampleShifts", coord, up, pitch_of(coord), pitch_of(up), 2, 1, tcx, tcy, 2 * tcx, 2 * tcy, T, T)
        g.check("tracker chain")
        got[k.name] = [a.copy() for a in (rt, mt, sq, bx, by, dist, coord, up)]
    for nm, a, b in zip(["ref tiles", "moved tiles", "squaredSum", "boxX", "boxY", "normalizedCC", "findMinimum", "UpSampleShifts"],
                        got["oracle"], got["reference"]):
        assert_bitexact(a, b, nm)
    assert np.abs(got["oracle"][6]).max() > 0


# ---------------------------------------------------------------- C: shift minimiser
def test_checkForOutliers_to_convergence(orc, ref):
    """The outlier loop: solve (no reference kernel: the oracle's solver for both) / checkForOutliers until every tile reports -1,
    with outliers, a tile whose inversion failed and a tile that had converged before."""
    n_img, tiles = 6, 37
    pairs = [(a, b) for a in range(n_img) for b in range(a + 1, n_img)]
    n1, m = n_img - 1, len(pairs)
    r = rng(40)
    d_true = r.uniform(-3, 3, (tiles, n1, 2)).astype(np.float32)
    A1 = _design(n_img, pairs)
    meas = np.zeros((tiles, m, 2), np.float32)
    for k, (a, b) in enumerate(pairs):
        meas[:, k] = d_true[:, a:b].sum(1)
    meas += r.normal(0, 0.02, meas.shape).astype(np.float32)
    meas[3, 4] += 5.0
    meas[7, 0] -= 9.0
    meas[7, 9] += 4.0      # two outliers in one tile: dropped one per round
    res = []
    for k in (orc, ref):
        g = Guard()
        A, ms = g.new(np.tile(A1[None], (tiles, 1, 1))), g.new(meas)
        one, opt = g.zeros((tiles, n1, 2)), g.zeros((tiles, 2, m))
        info, status = g.zeros(tiles, np.int32), g.zeros(tiles, np.int32)
        status[11] = -1
        rounds = 0
        while True:
            orc.call("solveShiftsBatched", A, ms, one, opt, info, tiles, n_img, m)
            if rounds == 0:
                info[5] = 3    # a failed inversion
            k.call("checkForOutliers", ms, opt, A, status, info, tiles, n_img, m)
            rounds += 1
            if (status < 0).all() or rounds > m:
                break
        g.check("checkForOutliers")
        res.append([x.copy() for x in (A, ms, one, opt, info, status)] + [rounds])
    for i, nm in enumerate(["shiftMatrix", "measured", "oneToOne", "optimT", "info", "status"]):
        assert_bitexact(res[0][i], res[1][i], nm)
    assert res[0][6] == res[1][6] >= 3
    assert (res[0][1][3, 4] == 0).all() and (res[0][1][7, 0] == 0).all() and (res[0][1][7, 9] == 0).all()


def test_shift_glue_kernels(orc, ref):
    n_img, tcx, tcy = 5, 6, 4
    n1 = n_img - 1
    tiles = tcx * tcy
    best = rng(43).uniform(-3, 3, (tiles, n1, 2)).astype(np.float32)
    for refi, trk in [(0, 3), (4, 1), (2, 2), (0, 4), (4, 0)]:
        def make(g):
            out = g.new(np.full((tcy, tcx + 2, 2), 5, np.float32))
            return (out, best, n_img, tcx, tcy, pitch_of(out), refi, trk), [out]
        pin(orc, ref, "getOptimalShifts", make, BLOCKS_2D)
    m = 7
    mT = rng(44).random((tiles, 2, m), dtype=np.float32)
    oT = rng(45).random((tiles, 2, n1), dtype=np.float32)

    def make_t(g):
        ms, one = g.zeros((tiles, m, 2)), g.zeros((tiles, n1, 2))
        return (ms, mT, oT, one, tiles, n_img, m), [ms, one]
    pin(orc, ref, "transposeShifts", make_t, [(16, 16, 1), (5, 3, 1)])

    def make_c(g):
        mats = g.new(rng(46).random((tiles, n1, m), dtype=np.float32))
        return (mats, tiles, n_img, m), [mats]
    (o,) = pin(orc, ref, "copyShiftMatrix", make_c, BLOCKS_1D)
    assert (o == o[0]).all()


def test_concatenate_separate_setPointers(orc, ref):
    m, tcx, tcy = 3, 5, 4
    imgs = [rng(47 + i).random((tcy, tcx + i, 2), dtype=np.float32) for i in range(m)]
    ptrs = np.array([a.ctypes.data for a in imgs], np.uint64)
    pitches = np.array([pitch_of(a) for a in imgs], np.int32)

    def make(g):
        out = g.zeros((tcy * tcx, m, 2))
        return (ptrs, pitches, out, m, tcx, tcy), [out]
    (cat,) = pin(orc, ref, "concatenateShifts", make, [(4, 4, 4), (3, 5, 1)])
    for k in range(m):
        assert np.array_equal(cat[:, k].reshape(tcy, tcx, 2), imgs[k][:, :tcx])
    outs = []
    for k in (orc, ref):
        g = Guard()
        back = [g.new(np.full_like(a, 9)) for a in imgs]
        bptrs = np.array([a.ctypes.data for a in back], np.uint64)
        k.call("separateShifts", cat, bptrs, pitches, m, tcx, tcy)
        g.check("separateShifts")
        outs.append([b.copy() for b in back])
    for a, b, src in zip(outs[0], outs[1], imgs):
        assert_bitexact(a, b, "separateShifts")
        assert np.array_equal(a[:, :tcx], src[:, :tcx]) and (a[:, tcx:] == 9).all()
    tiles, n_img, mm = 9, 4, 5
    bases = [np.zeros(tiles * 64, np.float32) for _ in range(8)]
    res = []
    for k in (orc, ref):
        g = Guard()
        arrs = [g.zeros(tiles, np.uint64) for _ in range(8)]
        k.call("setPointers", *arrs, *bases, tiles, n_img, mm)
        g.check("setPointers")
        res.append([a.copy() for a in arrs])
    for a, b in zip(*res):
        assert np.array_equal(a, b) and a[1] > a[0]


# ---------------------------------------------------------------- D/E: optical flow
def _adjacent_range(a):
    """Largest difference between two texels of any 2x2 footprint (per channel maximum)."""
    a = np.asarray(a, np.float64)
    d = [np.abs(a[:, 1:] - a[:, :-1]).max(), np.abs(a[1:] - a[:-1]).max(), np.abs(a[1:, 1:] - a[:-1, :-1]).max(),
         np.abs(a[1:, :-1] - a[:-1, 1:]).max()]
    return float(max(d))


def test_WarpingKernel(orc, ref):
    H, W = 50, 70
    img = _smooth_image(50, H, W)
    uv = rng(51).uniform(-6, 6, (H, W, 2)).astype(np.float32)
    uv[0, 0] = [-30, 200]      # far outside: mirror addressing, several periods
    uv[1, 1] = [-1.5, -1.5]    # just across the border
    uv[2, 2] = [np.nan, 0]     # NaN coordinate: texel 0 on that axis

    def make(g):
        out = g.zeros((H, W + 1))
        return (W, H, pitch_of(out), Tex(uv), out, Tex(img)), [out]

    (o,) = pin(orc, ref, "WarpingKernel", make, BLOCKS_2D)
    # fixed8: CUDA's hardware filter keeps 8 fractional bits of the two interpolation weights.  Per fetch the result moves by
    # at most 2 * 2^-9 * D (each weight off by <= 2^-9, D = largest texel difference in a 2x2 footprint).  The flow fetch
    # moves each coordinate by d <= 2^-8 * D_uv texels; a bilinear surface changes by at most D_img per texel along each axis,
    # so the image fetch moves by <= 2 * d * D_img, plus its own 2^-8 * D_img.  Finite flows only.
    uvf = uv.copy()
    uvf[2, 2] = [0.25, 0.25]
    g = Guard()
    exact, fixed = g.zeros((H, W)), g.zeros((H, W))
    ref.call("WarpingKernel", W, H, pitch_of(exact), Tex(uvf), exact, Tex(img))
    ref.call("WarpingKernel", W, H, pitch_of(fixed), Tex(uvf), fixed, Tex(img), filter="fixed8")
    g.check("WarpingKernel fixed8")
    d_img, d_uv = _adjacent_range(img), max(_adjacent_range(uvf[..., 0]), _adjacent_range(uvf[..., 1]))
    bound = 2.0 ** -8 * d_img * (1.0 + 2.0 * d_uv) + 1e-6
    dist = float(np.abs(exact.astype(np.float64) - fixed).max())
    print(f"WarpingKernel: exact vs fixed8 filtering, max |d| = {dist:.3e} (bound {bound:.3e}, D_img {d_img:.3f}, D_uv {d_uv:.2f})")
    assert 0 < dist <= bound


@pytest.mark.parametrize("rot", [0.0, 0.02])
def test_CreateFlowFieldFromTiles(orc, ref, rot):
    H, W, tcx, tcy = 48, 80, 5, 3
    ts = rng(52).uniform(-3, 3, (tcy, tcx, 2)).astype(np.float32)

    def make(g):
        out = g.zeros((H, W + 3, 2))
        return (out, Tex(ts), 16, tcx, tcy, W, H, pitch_of(out), F2([0.5, -1.5] if rot else [0, 0]), rot), [out]

    pin(orc, ref, "CreateFlowFieldFromTiles", make, BLOCKS_2D)


def test_ComputeDerivatives(orc, ref):
    H, W = 40, 56
    a, b = _smooth_image(53, H, W), _smooth_image(54, H, W)

    def make(g):
        Ix, Iy, Iz = (g.zeros((H, W + 2)) for _ in range(3))
        return (W, H, pitch_of(Ix), Ix, Iy, Iz, Tex(a), Tex(b)), [Ix, Iy, Iz]

    pin(orc, ref, "ComputeDerivativesKernel", make, BLOCKS_2D)

    def make2(g):
        Ix, Iy = (g.zeros((H, W + 2)) for _ in range(2))
        return (W, H, pitch_of(Ix), Ix, Iy, Tex(a)), [Ix, Iy]

    pin(orc, ref, "ComputeDerivatives2Kernel", make2, BLOCKS_2D)
    # fixed8: four fetches with coefficients (1, 8, 8, 1) / 12, each off by <= 2^-8 * D (see test_WarpingKernel): 1.5 * 2^-8 * D
    g = Guard()
    ex, ey, fx, fy = (g.zeros((H, W)) for _ in range(4))
    ref.call("ComputeDerivatives2Kernel", W, H, pitch_of(ex), ex, ey, Tex(a))
    ref.call("ComputeDerivatives2Kernel", W, H, pitch_of(fx), fx, fy, Tex(a), filter="fixed8")
    g.check("ComputeDerivatives2Kernel fixed8")
    bound = 1.5 * 2.0 ** -8 * _adjacent_range(a) + 1e-6
    dist = float(max(np.abs(ex.astype(np.float64) - fx).max(), np.abs(ey.astype(np.float64) - fy).max()))
    print(f"ComputeDerivatives2Kernel: exact vs fixed8 filtering, max |d| = {dist:.3e} (bound {bound:.3e})")
    assert dist <= bound


@pytest.mark.parametrize("hw", [1, 3])
def test_lucasKanadeOptim(orc, ref, hw):
    H, W = 36, 52
    r = rng(55)
    fx = (r.random((H, W), dtype=np.float32) - 0.5) * 0.4
    fy = (r.random((H, W), dtype=np.float32) - 0.5) * 0.4
    ft = (r.random((H, W), dtype=np.float32) - 0.5) * 0.1
    fx[10:14, 10:14] = 0
    fy[10:14, 10:14] = 0       # singular windows
    fx[20:27, 20:27] = fy[20:27, 20:27]   # rank one
    ft[30, 30] = np.nan        # NaN update -> 0
    sh0 = r.uniform(-1, 1, (H, W, 2)).astype(np.float32)

    def make(g):
        sh = g.new(sh0)
        return (sh, fx, fy, ft, pitch_of(sh), pitch_of(fx), W, H, hw, 1e-3), [sh]

    (o,) = pin(orc, ref, "lucasKanadeOptim", make, BLOCKS_2D)
    assert_bitexact(o[:hw], sh0[:hw])
    assert np.abs(o - sh0).max() > 0.01


def test_structure_tensor_and_kernel_param(orc, ref):
    H, W = 44, 60
    img = _smooth_image(57, H, W)
    Ix, Iy = (np.zeros((H, W), np.float32) for _ in range(2))
    orc.call("ComputeDerivatives2Kernel", W, H, pitch_of(Ix), Ix, Iy, Tex(img))

    def make(g):
        out = g.zeros((H, W + 1, 3))
        return (Ix, Iy, out, W, H, pitch_of(Ix), pitch_of(out)), [out]

    (o,) = pin(orc, ref, "ComputeStructureTensor", make, BLOCKS_2D)

    def make_k(g):
        t = g.new(o)
        t[0, 0] = 0                       # lam1 + lam2 = 0 -> NaN anisotropy
        t[0, 1] = [1e-3, 1e-3, 0]         # isotropic: help = 0 -> (c, s) fallback
        t[0, 2] = [np.nan, 1, 0]
        t[0, 3] = [np.inf, 1, 0.5]
        t[0, 4] = [1, 2, -3]              # not positive semi-definite: negative eigenvalue under the root
        t[0, 5] = [2, 1, 0.7]             # the off-diagonal term with either sign
        t[0, 6] = [2, 1, -0.7]
        t[0, 7] = [0, 0, 1e-20]
        return (t, W, H, pitch_of(t), 0.005, 0.05, 0.3, 2.0, 2.0, 2.0), [t]

    (k,) = pin(orc, ref, "ComputeKernelParam", make_k, BLOCKS_2D)
    assert k[0, 5, 2] == -k[0, 6, 2] != 0


# ---------------------------------------------------------------- F: robustness
def test_ComputeRobustnessMask(orc, ref):
    H, W = 36, 52
    r = rng(60)
    refimg = r.random((H, W, 3), dtype=np.float32)
    mov = np.clip(refimg + r.normal(0, 0.02, refimg.shape).astype(np.float32), 0, 1).astype(np.float32)
    mov[5:9, 5:9] += 0.5
    refimg[20:24, 20:24] = 0.5         # flat patch: stdRef = 0
    refimg[26:30, 26:30] = 0.0         # with beta = 0 below: sigma = 0
    uv = r.uniform(-5, 5, (H, W, 2)).astype(np.float32)
    uv[3, 3] = [90, -90]               # moved patch clamped at the border
    for alpha, beta, thr in ((1e-4, 1e-6, 0.8), (1e-4, 0.0, 0.05)):
        def make(g):
            mask = g.zeros((H, W + 1, 4))
            return (refimg, mov, mask, Tex(uv), W, H, pitch_of(refimg), pitch_of(mask), alpha, beta, thr), [mask]

        (o,) = pin(orc, ref, "ComputeRobustnessMask", make, BLOCKS_2D)
    assert (o[0] == 0).all() and (o[:, W - 1] == 0).all() and o[..., :3].max() > 0.5


# ---------------------------------------------------------------- H / I
def test_ApplyWeighting_GammasRGB(orc, ref):
    H, W = 30, 44
    r = rng(61)
    fin = np.zeros((H, W + 1, 3), np.float32)
    wt = np.zeros((H, W + 1, 3), np.float32)
    fin[:, :W] = r.random((H, W, 3), dtype=np.float32) * 4
    wt[:, :W] = r.random((H, W, 3), dtype=np.float32) * 4
    wt[0, :5] = 0
    wt[1, :5] = -1          # w + 1 == 0 -> output 0
    wt[2, :5] = 1e-4        # below the threshold -> fallback blended in
    wt[3, :5] = 1e-3        # exactly the threshold: not below
    wt[4, :5] = np.nan
    io0 = np.zeros((H, W + 1, 3), np.float32)
    io0[:, :W] = rng(62).random((H, W, 3), dtype=np.float32)
    thr = float(np.float32(1e-3))

    def make(g):
        io = g.new(io0)
        return (io, fin, wt, W, H, pitch_of(io), thr), [io]

    (o,) = pin(orc, ref, "ApplyWeighting", make, BLOCKS_2D)
    assert (o[1, :5] == 0).all()

    def make_g(g):
        io = g.new((o * 1.2 - 0.1).astype(np.float32))
        io[0, 0] = np.nan
        io[0, 1] = [0.0031308, 0.0031309, np.inf]
        return (io, W, H, pitch_of(io)), [io]

    (og,) = pin(orc, ref, "GammasRGB", make_g, BLOCKS_2D)
    assert og[0, 0, 0] == 0.0 and og[0, 1, 2] > 0.9999   # inf clamps to 1


def test_fourier_helpers(orc, ref):
    H, W = 32, 48
    spec = np.zeros((H, W // 2 + 3, 2), np.float32)
    spec[:, :W // 2 + 1] = rng(64).random((H, W // 2 + 1, 2), dtype=np.float32)
    for lp, hp, lps, hps, ca in [(0.3, 0.0, 0.0, 0.0, 0), (0.3, 0.05, 0.05, 0.02, 2), (0.0, 0.0, 0.1, 0.0, 0)]:
        def make(g):
            s = g.new(spec)
            return (s, pitch_of(s), W, H, lp, hp, lps, hps, ca), [s]
        pin(orc, ref, "fourierFilter", make, BLOCKS_2D)        # kernel.cu:793

    def make_s(g):
        s = g.new(rng(65).random((H + 1, W + 1, 2), dtype=np.float32))
        return (s, W + 1, H + 1), [s]
    pin(orc, ref, "fftshift", make_s, BLOCKS_2D)               # kernel.cu:872

    def make_c(g):
        b = g.new(rng(67).random((100, 2), dtype=np.float32))
        return (rng(66).random((100, 2), dtype=np.float32), b, 100), [b]
    pin(orc, ref, "conjugateComplexMulKernel", make_c, BLOCKS_1D)


# ---------------------------------------------------------------- coverage gate
# kernel -> the test of this file that pins it (the gate checks that the test exists and names the kernel)
PINNED = {
    "deBayersSubSample3": "test_deBayersSubSample3",
    "deBayerGreenKernel": "test_deBayer_green_then_redblue",
    "deBayerRedBlueKernel": "test_deBayer_green_then_redblue",
    "accumulateImages": "test_accumulateImages",
    "accumulateImagesSuperRes": "test_accumulateImagesSuperRes",
    "squaredSum": "test_squaredSum_boxFilters_normalizedCC",
    "boxFilterWithBorderX": "test_squaredSum_boxFilters_normalizedCC",
    "boxFilterWithBorderY": "test_squaredSum_boxFilters_normalizedCC",
    "normalizedCC": "test_squaredSum_boxFilters_normalizedCC",
    "convertToTilesOverlapBorder": "test_convertToTiles",
    "convertToTilesOverlapPreShift": "test_convertToTiles",
    "findMinimum": "test_findMinimum",
    "UpSampleShifts": "test_UpSampleShifts",
    "checkForOutliers": "test_checkForOutliers_to_convergence",
    "transposeShifts": "test_shift_glue_kernels",
    "getOptimalShifts": "test_shift_glue_kernels",
    "copyShiftMatrix": "test_shift_glue_kernels",
    "concatenateShifts": "test_concatenate_separate_setPointers",
    "separateShifts": "test_concatenate_separate_setPointers",
    "setPointers": "test_concatenate_separate_setPointers",
    "WarpingKernel": "test_WarpingKernel",
    "CreateFlowFieldFromTiles": "test_CreateFlowFieldFromTiles",
    "ComputeDerivativesKernel": "test_ComputeDerivatives",
    "ComputeDerivatives2Kernel": "test_ComputeDerivatives",
    "lucasKanadeOptim": "test_lucasKanadeOptim",
    "ComputeStructureTensor": "test_structure_tensor_and_kernel_param",
    "ComputeKernelParam": "test_structure_tensor_and_kernel_param",
    "ComputeRobustnessMask": "test_ComputeRobustnessMask",
    "ApplyWeighting": "test_ApplyWeighting_GammasRGB",
    "GammasRGB": "test_ApplyWeighting_GammasRGB",
    "conjugateComplexMulKernel": "test_fourier_helpers",
    "fourierFilter": "test_fourier_helpers",
    "fftshift": "test_fourier_helpers",
}
# the only admissible reason: the oracle does not restate it
EXCLUDED = {
    "addKernel": "the oracle does not restate it (the toolkit's vector-add sample)",
    "addWithCuda": "the oracle does not restate it (host driver of that sample; never executed)",
}


def test_coverage_gate(ref):
    """Every function the reference library defines is a kernel pinned above (through its ref_<kernel> entry point), or is
    named in EXCLUDED.  Names with a leading underscore are the toolchain's and C++-mangled device helpers (inlined into the
    kernels that call them); ref_set_cfa_pattern sets c_cfaPattern for the DeBayer tests."""
    out = subprocess.run(["nm", "-D", "--defined-only", ref.path], check=True, capture_output=True, text=True).stdout
    funcs = sorted(ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TW")
    funcs = [f for f in funcs if not f.startswith("_")]
    assert len(funcs) > 60
    kernels = [f for f in funcs if not f.startswith("ref_")]
    entries = {f[4:] for f in funcs if f.startswith("ref_")} - {"set_cfa_pattern"}
    module = sys.modules[__name__]
    for k in kernels:
        if k in EXCLUDED:
            assert k not in entries and not hasattr(ref.cdll, "ref_" + k) and "does not restate" in EXCLUDED[k]
            from oracle.bindings import oracle
            assert "orc_" + k not in oracle().protos, f"{k} is excluded but the oracle restates it"
            continue
        assert k in entries, f"{k}: the reference defines it but the shim has no ref_{k}"
        assert k in PINNED, f"{k}: neither pinned by a test nor excluded"
        fn = getattr(module, PINNED[k])
        assert k in inspect.getsource(fn), f"{PINNED[k]} does not name {k}"
        assert ref.has(k)
    assert entries <= set(kernels)
    assert set(PINNED) <= set(kernels)


# ---------------------------------------------------------------- pipeline
def _run_pipeline(cfg, frames, backend=None):
    from oracle.pipeline import OraclePipeline
    op = OraclePipeline(cfg)
    if backend is not None:
        op.o = backend
    nf = [(f.cpu().numpy() if hasattr(f, "cpu") else f).view(np.uint16) for f in frames]
    img_out = np.zeros((op.hrH, op.hrW, 3), np.float32)
    tw = np.zeros_like(img_out)
    op.set_reference(nf[cfg.reference])
    for k, f in enumerate(nf):
        op.add_frame(f, k == cfg.reference, img_out, tw)
    out, q = op.finish(img_out, tw)
    return dict(img_out=img_out, tw=tw, out=out, out16=q, flow=op.flow, mask=op.mask, kparam=op.kparam4)


@pytest.mark.parametrize("scale,mono", [(2, False), (2, True), (4, False)])
def test_pipeline_on_reference_kernels(orc, ref, scale, mono):
    """The smoke() burst (3 x 256x192, seed 4321) through oracle/pipeline.py twice: as is, and with every kernel the reference
    library has answered by the reference (the fuse step, the glue stages and the correlation have no reference kernel and stay
    the oracle's).  Accumulators and the 16-bit image bit-identical."""
    from multi_frame_super_resolution_amd.pipeline import default_config
    from multi_frame_super_resolution_amd.synth import make_burst
    from oracle.bindings import oracle
    W, H, N = 256, 192, 3
    frames, _, _ = make_burst(W, H, N, scale=scale, mono=mono, seed=4321, max_shift=3.0)
    cfg = default_config(W, H, N, scale, mono)
    a = _run_pipeline(cfg, frames)
    backend = RefBackedOracle(ref, oracle())
    b = _run_pipeline(cfg, frames, backend)
    assert {"deBayersSubSample3", "deBayerGreenKernel", "deBayerRedBlueKernel", "convertToTilesOverlapBorder", "convertToTilesOverlapPreShift",
            "squaredSum", "boxFilterWithBorderX", "boxFilterWithBorderY", "normalizedCC", "findMinimum", "CreateFlowFieldFromTiles",
            "WarpingKernel", "ComputeDerivativesKernel", "ComputeDerivatives2Kernel", "lucasKanadeOptim", "ComputeStructureTensor",
            "ComputeKernelParam", "ComputeRobustnessMask", "ApplyWeighting"} <= backend.answered
    for key in ("kparam", "flow", "mask", "img_out", "tw", "out"):
        assert_bitexact(a[key], b[key], f"pipeline x{scale} mono={mono}: {key}")
    assert np.array_equal(a["out16"], b["out16"])
    assert a["tw"].max() > 1.0 and np.abs(a["flow"]).max() > 0.5
