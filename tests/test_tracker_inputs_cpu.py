"""What tests/test_tracker_inputs_gpu.py relies on, checked from the oracle alone (no GPU): its inputs are as hostile as their
comments say, so a GPU case cannot pass because its input was dull, and every row of its geometry table crosses the launch
boundary it names."""
import numpy as np
import pytest

from tests import test_tracker_inputs_gpu as trk
from tests.kernels import pitch_of
from tests.tracker_ref import grid, serial_argmin, upsampled


def _interior(idx, S):
    R = 2 * S + 1
    return 1 <= idx % R < 2 * S and 1 <= idx // R < 2 * S


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def test_geometry_rows_give_the_tile_counts_and_packings_they_claim():
    for T, S, W, H, tiles, tpw in trk.FAST_ROWS:
        assert (T, S) in trk.FAST and trk.FAST[(T, S)] == tpw
        tcx, tcy = grid(W, H, T)
        assert tcx * tcy == tiles and max(W, H) <= 300
        assert W % T or H % T, "a ragged size"
    assert {r[:2] for r in trk.FAST_ROWS} == set(trk.FAST)
    for pair in trk.FAST:      # per pair: one grid that does not fill its last workgroup or is a single tile inside/around the image
        rows = [r for r in trk.FAST_ROWS if r[:2] == pair]
        assert any(r[4] == 1 for r in rows) and any(r[4] > 1 for r in rows)
    assert trk.FAST_ROWS[1][4] % trk.FAST_ROWS[1][5] == 1                    # (32, 4) 97x45: 3 tiles, 2 per workgroup
    assert trk.FAST_ROWS[2][2] < 32 and trk.FAST_ROWS[2][3] < 32              # the image inside the tile
    for T, S, W, H, tiles, tpw in trk.GENERIC_ROWS:
        assert (T, S) not in trk.FAST and 4 <= T <= 128 and T > 2 * S and 1 <= S <= 15
        tcx, tcy = grid(W, H, T)
        assert tcx * tcy == tiles and max(W, H) <= 300
        assert W % T or H % T
        got_tpw, lds, rounds, uncut = trk.generic_launch(T, S)
        assert got_tpw == tpw and lds <= 160 * 1024
    by = {r[:2]: r for r in trk.GENERIC_ROWS}
    launch = {k: trk.generic_launch(*k) for k in by}
    assert launch[(4, 1)][0] == 14 and by[(4, 1)][4] == 10                    # one partial workgroup, T < 8
    assert launch[(8, 3)][0] == 2 and by[(8, 3)][4] % 2 == 1                  # an odd tile count: the last workgroup half empty
    assert 12 % 8 != 0 and 12 > 8 and 20 % 8 != 0                            # unrolled loop + remainder
    assert 13 * 13 > trk.TRK_THREADS and launch[(20, 6)][2] == 2             # several rounds per tile
    assert launch[(24, 5)][:1] == (1,)
    assert launch[(48, 2)][3] == 5 and launch[(48, 2)][0] == 2 and launch[(48, 2)][1] <= 56 * 1024   # the 56 KB loop
    assert 4 * 5348 * 3 > 56 * 1024                                          # ... which three tiles would exceed
    assert 64 * 1024 < launch[(64, 15)][1] <= 160 * 1024                      # needs the raised LDS limit
    assert trk.generic_launch(*trk.UNSUPPORTED_ROW[:2])[1] > 160 * 1024
    assert sorted(T for T, S in by if T % 2) == [5, 9, 17]


def test_odd_tiles_shrink_the_box_term_only(orc):
    """boxFilterWithBorderX / Y sum shift = -T/2 .. T/2 - 1: 2 * (T / 2) taps, T - 1 for odd T, starting at the candidate's own
    column; squaredSum and crossCorrelateTiles take all T x T pixels."""
    for T, S in ((5, 2), (9, 3), (17, 4), (8, 3)):
        L, R = T + 2 * S, 2 * S + 1
        taps = 2 * (T // 2)
        ones = np.ones((1, L, L), np.float32)
        bx, by = np.zeros_like(ones), np.zeros_like(ones)
        orc.call("boxFilterWithBorderX", ones, bx, S, T, 1)
        orc.call("boxFilterWithBorderY", bx, by, S, T, 1)
        c = L // 2
        assert (by[0, c - S:c + S + 1, c - S:c + S + 1] == taps * taps).all()
        # the window of candidate sx starts at column sx: a single 1 at column sx + taps is outside, at sx + taps - 1 inside
        one = np.zeros((1, L, L), np.float32)
        one[0, :, S + taps] = 1
        orc.call("boxFilterWithBorderX", one, bx, S, T, 1)
        assert bx[0, 0, c] == 0 and bx[0, 0, c + 1] == 1
        sq, cc = np.zeros(1, np.float32), np.zeros_like(ones)
        orc.call("squaredSum", ones, sq, S, T, 1)
        orc.call("crossCorrelateTiles", ones, ones, cc, S, T, 1)
        assert sq[0] == T * T and cc[0, 0, 0] == T * T


# ---- content -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", trk.FAST_ROWS + trk.GENERIC_ROWS, ids=trk.row_id)
def test_random_rows_recover_the_shift_where_they_say(orc, row):
    c = trk.random_case(row)
    want, _, _, pre = c.oracle(orc)
    assert np.isfinite(want[:, :c.tcx]).all()
    if row[:4] in trk.RECOVER_ROWS:
        ok = trk.recoverable(c, pre[:, :c.tcx], trk.true_shift(c.S))
        assert ok.any()
    if c.T % 2 == 0 and c.S >= 2:
        trk.assert_recovered(want[:, :c.tcx], trk.recoverable(c, pre[:, :c.tcx], trk.true_shift(c.S)), trk.true_shift(c.S))


@pytest.mark.parametrize("row", trk.TIE_ROWS, ids=trk.row_id)
def test_stripes_tie_at_interior_indices(orc, row):
    T, S = row[:2]
    for content in trk.TIE_CONTENTS:
        c = trk.tie_case(row, content)
        assert set(np.unique(c.ref[:, :c.W])) <= {0.0, 1.0, 2.0} and set(np.unique(c.mov[:, :c.W])) <= {0.0, 1.0, 2.0}
        _, dist, _, _ = c.oracle(orc)
        tied_tiles, interior_tiles, differing = 0, 0, 0
        for d in dist:
            mn, idx, _ = serial_argmin(d)
            at = np.flatnonzero(d.reshape(-1) == mn)
            assert at[0] == idx
            if at.size >= 2:
                tied_tiles += 1
                inner = [i for i in at if _interior(i, S)]
                if len(inner) >= 2 and _interior(idx, S):
                    interior_tiles += 1
                    differing += inner[-1] != idx
        if content != "identical":
            assert tied_tiles >= 1, content
        if content.endswith("_marked"):
            # the first strict minimum and the last equal one are both interior: another tie-break gives another shift
            assert interior_tiles >= 1 and differing >= 1, content
        if content == "identical" and T % 2 == 0:
            assert (dist.reshape(dist.shape[0], -1).min(1) == 0).any()     # an exact zero minimum


def test_half_integer_grids_hold_exact_halves(orc):
    for row in trk.HALF_ROWS:
        c = trk.half_preshift_case(row)
        pre = c.pre[:, :c.tcx]
        vals = set(np.abs(pre[trk.is_half(pre)]).tolist())
        assert vals <= {0.5, 1.5, 2.5} and len(vals) >= min(3, c.tcx * c.tcy)
        assert (~trk.is_half(pre)).any()
        assert (pre[trk.is_half(pre)] > 0).any() and (pre[trk.is_half(pre)] < 0).any()
    for row in trk.UP_ROWS:
        c = trk.half_upsample_case(row)
        assert (c.coarse[:, :c.up[2]] == np.round(c.coarse[:, :c.up[2]])).all()
        pre = upsampled(orc, c.coarse, c.up, c.tcx, c.tcy)[:, :c.tcx]
        assert trk.is_half(pre).any() and (~trk.is_half(pre)).any()


def test_off_image_preshifts_clamp(orc):
    for row in trk.OFF_ROWS:
        c = trk.off_image_case(row)
        L = c.T + 2 * c.S
        n = c.tcx * c.tcy
        mt = np.zeros((n, L, L), np.float32)
        from tests.kernels import F2
        orc.call("convertToTilesOverlapPreShift", c.mov, mt, c.pre, pitch_of(c.pre), c.W, c.H, pitch_of(c.mov), c.S, c.T, c.tcx, c.tcy,
                 F2([0, 0]), 0.0)
        assert np.isfinite(mt).all()
        last = mt[-1]
        assert (last == last[:, :1]).all() and not (mt[0] == mt[0][:, :1]).all()   # every fetch of the last tile: column 0
        assert np.abs(c.pre[:, :c.tcx]).max() >= c.T + c.S


@pytest.mark.parametrize("row", trk.NONFINITE_ROWS, ids=trk.row_id)
def test_nonfinite_cases_leave_tiles_without_a_minimum(orc, row):
    c = trk.nonfinite_case(row)
    want, dist, _, pre = c.oracle(orc)
    (ax, ay), (bx, by), (cx, cy), (dx, dy) = trk.nonfinite_tiles(c.tcx, c.tcy)
    for tx, ty in ((ax, ay), (bx, by)):       # some candidates NaN, some finite: a minimum exists
        d = dist[ty * c.tcx + tx]
        assert np.isnan(d).any() and np.isfinite(d).any() and serial_argmin(d)[1] >= 0
    for tx, ty in ((cx, cy), (dx, dy)):       # nothing below FLT_MAX
        assert serial_argmin(dist[ty * c.tcx + tx])[1] == -1
        np.testing.assert_array_equal(want[ty, tx], np.round(pre[ty, tx]))
    assert np.isinf(c.mov[:, :c.W]).sum() == 1 and np.isnan(c.ref[:, :c.W]).sum() == 1


def test_thresholds_split_the_tiles(orc):
    for row in trk.THRESHOLD_ROWS:
        c = trk.threshold_case(orc, row)
        _, dist, _, _ = c.oracle(orc)
        d = dist.reshape(dist.shape[0], -1)
        zeroed = c.threshold + d.min(1) > d.max(1)
        assert zeroed.any() and (~zeroed).any(), trk.row_id(row)
    for row in trk.TIE_ROWS:
        c = trk.exact_threshold_case(orc, row)
        want, dist, _, _ = c.oracle(orc)
        d = dist[0].reshape(-1)
        assert c.threshold == d.max() - d.min() and c.threshold > 0
        assert not (c.threshold + d.min() > d.max())          # strict: tile 0 keeps its shift ...
        assert (want[0, 0] != 0).any()                        # ... which is not zero
        assert np.nextafter(c.threshold, np.float32(np.inf)) + d.min() > d.max()


def test_rotated_corner_patches_clamp(orc):
    """The base cases: rotation moves the corner tiles' patches past the image border, and the cos / sin handed to the device
    are those of the C library the oracle calls."""
    from tests.kernels import F2
    from tests.tracker_ref import libm_cos_sin
    for rot in (0.02, -0.02, 0.1, 0.17):
        c, s = libm_cos_sin(orc, rot)
        assert abs(float(c) - np.cos(np.float32(rot))) < 1e-7 and abs(float(s) - np.sin(np.float32(rot))) < 1e-7
        assert c.dtype == np.float32
    for row in trk.BASE_ROWS:
        W, H, T, S = row[2], row[3], row[0], row[1]
        tcx, tcy = grid(W, H, T)
        L = T + 2 * S
        # an image that holds its own column index: a clamped fetch repeats the border column
        img = np.tile(np.arange(W, dtype=np.float32), (H, 1))
        mt = np.zeros((tcx * tcy, L, L), np.float32)
        pre = np.zeros((tcy, tcx, 2), np.float32)
        clamped = 0
        for base in trk.BASES:
            bs = F2([np.float32(base[0]) * np.float32(base[3]), np.float32(base[1]) * np.float32(base[3])])
            orc.call("convertToTilesOverlapPreShift", img, mt, pre, pitch_of(pre), W, H, pitch_of(img), S, T, tcx, tcy, bs, float(np.float32(base[2])))
            clamped += int((mt[:, 0, 0] == mt[:, 0, 1]).sum() + (mt[:, 0, -1] == mt[:, 0, -2]).sum())
        assert clamped >= 1, trk.row_id(row)
