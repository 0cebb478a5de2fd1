"""Coverage gate of tests/test_kernel_edges_gpu.py and tests/test_finish_edges_gpu.py: every entry point of include/mfsr.h that
takes a pitch, a width or a ``...RowBytes`` is in the edge sweep or the row-stripe tests of the first, in the sweep of the second,
or is listed here with the reason it is not.  A kernel added later without either fails this test.  Also what the sweeps decide
without a device: the robustness seeds from the oracle alone, and which path the geometric finish's tiles take."""
import re

import numpy as np

from multi_frame_super_resolution_amd.capi import parse_header
from tests import test_finish_edges_gpu as finish
from tests import test_kernel_edges_gpu as edges

PIPELINE = "burst / stream driver, covered by tests/test_pipeline_gpu.py"
BATCH = "batched form, bit-compared with the single-frame call in tests/test_batch_kernels_gpu.py"
TRACKER = ("tiles packed into workgroups: ragged sizes, every packing and padded pitches against the oracle chain in "
           "tests/test_tracker_inputs_gpu.py")
WINDOW = "zoom-window form, bit-compared with the cropped whole-frame call in tests/test_window_gpu.py"

EXCLUDED = {
    # tile tracker: the pitch is that of the whole image and the launch goes over tiles, not over pixel blocks; the fused trackers
    # pack several tiles into a workgroup and have their own sweep (TRACKER)
    "mfsr_convertToTilesOverlapBorder": "one workgroup per tile; padded image pitch in test_parity_kernels.py::test_convertToTiles",
    "mfsr_convertToTilesOverlapPreShift": "one workgroup per tile; padded image pitch in test_parity_kernels.py::test_convertToTiles",
    "mfsr_findMinimum": "one thread per tile; padded output pitch in test_parity_kernels.py::test_findMinimum",
    "mfsr_UpSampleShifts": "tile-grid kernel, test_parity_kernels.py::test_UpSampleShifts",
    "mfsr_getOptimalShifts": "tile-grid kernel; padded output pitch in test_parity_kernels.py::test_shift_glue_kernels",
    "mfsr_concatenateShifts": "pointer-array ABI on the tile grid, test_parity_kernels.py::test_concatenate_separate_setPointers",
    "mfsr_separateShifts": "pointer-array ABI on the tile grid, test_parity_kernels.py::test_concatenate_separate_setPointers",
    "mfsr_addRoundedPreShift": "tile-grid kernel, used by test_parity_kernels.py::test_trackTilesFused_equals_chain",
    "mfsr_trackTilesFused": TRACKER + "::test_every_geometry_row",
    "mfsr_trackTilesFusedBase": TRACKER + "::test_every_geometry_row, ::test_rotated_base",
    "mfsr_trackTilesFusedUp": TRACKER + "::test_half_integer_upsampled_shifts",
    "mfsr_tileSquaredSums": TRACKER + "::test_every_geometry_row (against squaredSum at every row)",
    "mfsr_trackTilesFusedBatch": TRACKER + "::test_batch_of_frames; " + BATCH,
    # Fourier helpers of the reference's tracker, not on the pipeline's path
    "mfsr_fourierFilter": "half-spectrum helper, test_parity_kernels.py::test_fourier_helpers",
    "mfsr_fftshift": "dense by contract (no pitch), test_parity_kernels.py::test_fourier_helpers",
    # other forms of swept kernels
    "mfsr_accumulateSuperResFull2": "two-frame form of mfsr_accumulateSuperResFullN, which the row-stripe test runs whole-frame",
    "mfsr_accumulateSuperResFullN": "the whole-frame side of test_kernel_edges_gpu.py::test_accumulateSuperResFullRows",
    "mfsr_accumulateSuperResFullWindow": WINDOW,
    "mfsr_CreateFlowFieldFromTilesBase": "device-prealign form, bit-compared in test_parity_kernels.py::test_lucasKanadeIterationWarped_is_bit_identical",
    "mfsr_CreateFlowFieldWarped": "bit-compared with the swept chain in test_parity_kernels.py::test_lucasKanadeIterationWarped_is_bit_identical",
    "mfsr_lucasKanadeIterationWarped": "bit-compared with mfsr_lucasKanadeIterationFused in test_parity_kernels.py::test_lucasKanadeIterationWarped_is_bit_identical",
    "mfsr_prepareFrameFusedBatch": BATCH,
    "mfsr_CreateFlowFieldWarpedBatch": BATCH,
    "mfsr_robustnessMaskFusedBatch": BATCH,
    "mfsr_zeroRing_f32x4": "ring fill called inside mfsr_robustnessMaskFused, whose sweep asserts the zero ring at every shape",
    # global pre-alignment: integer scores, identical results or not at all
    "mfsr_preAlign_pyramid_bytes": "size query",
    "mfsr_preAlignPyramid": "test_parity_kernels.py::test_preAlign_matches_oracle_exactly (four sizes, exact)",
    "mfsr_preAlign": "test_parity_kernels.py::test_preAlign_matches_oracle_exactly (four sizes, exact)",
    # raw-domain stages
    "mfsr_packed_row_bytes": "host arithmetic, tests/test_packed_cpu.py",
    "mfsr_shadingStats": "calibration statistics (not on the burst path): numpy restatement at padded, offset rows in tests/test_shading_gpu.py",
    "mfsr_noiseStats": "calibration statistics (not on the burst path): numpy restatement at padded, offset rows in tests/test_noise_gpu.py",
    # drivers and host functions
    "mfsr_config_default": "host function: fills a configuration",
    "mfsr_window_check": "host function: argument check",
    "mfsr_lucasKanadeSweepBand": "host function: the sweep's band rule, values pinned in tests/test_lk_band_cpu.py",
    "mfsr_burst_set_window": PIPELINE,
    "mfsr_burst_get_window": PIPELINE,
    "mfsr_burst_align_frame": PIPELINE,
    "mfsr_burst_align_frames": PIPELINE,
    "mfsr_burst_fuse_rows": "multi-GPU stripe driver, covered by tests/test_dist_local_gpu.py",
    "mfsr_burst_field_dims": "host function: reports sizes",
    "mfsr_stream_set_window": PIPELINE,
    "mfsr_burst_set_host_row_bytes": "host function: stores the row pitch of the host frames; " + PIPELINE,
    "mfsr_burst_finish_geometry": "burst driver of the swept mfsr_finishGeometry, tests/test_geometry_gpu.py::"
                                  "test_burst_finish_geometry_equals_the_restatement_of_the_plain_float_image",
}

GEOMETRY = re.compile(r"pitch|stride|^width$|^imgWidth$|^dimX$|^outW$|^cols$|^step|RowBytes$", re.I)


def _geometry_entries():
    out = []
    for name, (_, args) in parse_header().items():
        if any(GEOMETRY.search(a) for _, a in args):
            out.append(name)
    return out


def test_every_pitched_entry_point_is_swept_or_excluded():
    covered = set(edges.SWEEP) | set(edges.ROW_STRIPE_TESTS) | set(finish.SWEEP)
    names = _geometry_entries()
    assert len(names) > 105           # 83 by a pitch, a stride or a width, 23 more by ``...RowBytes``
    assert not set(edges.SWEEP) & set(finish.SWEEP)
    missing = [n for n in names if n not in covered and n not in EXCLUDED]
    assert not missing, f"neither in the edge sweep nor in EXCLUDED: {missing}"
    both = [n for n in EXCLUDED if n in covered]
    assert not both, f"swept and excluded at once: {both}"
    stale = [n for n in list(EXCLUDED) + sorted(covered) if n not in parse_header()]
    assert not stale, f"not in include/mfsr.h: {stale}"
    for n, why in EXCLUDED.items():
        assert isinstance(why, str) and len(why) > 8 and "\n" not in why, n
    for n, case in edges.SWEEP.items():
        assert case in edges.CASES
    for n, test in edges.ROW_STRIPE_TESTS.items():
        assert callable(getattr(edges, test))
    for n, case in finish.SWEEP.items():
        assert case in finish.CASES


def test_shapes_stay_small_and_cross_the_block():
    for name, (fn, shp) in edges.CASES.items():
        assert 1 <= len(shp) <= 14, name
        for s in shp:
            assert max(s) <= 300 and sorted(s)[-2] <= 120, (name, s)
    assert (63, 3) in edges.B64x4 and (64, 4) in edges.B64x4 and (65, 5) in edges.B64x4 and edges.B64x4[0] == (1, 1)
    for rowb, align in ((4, 4), (60, 4), (252, 4), (56, 8), (48, 16), (1, 1), (63, 1), (20, 8)):
        p = edges.padded_pitch(rowb, align)
        assert p > rowb and p % align == 0 and p % 64 != 0 and p - rowb <= 2 * align + align


def test_robustness_seeds_keep_the_oracle_off_the_threshold(orc):
    """What test_kernel_edges_gpu.py::c_robustnessFused relies on, from the oracle's output alone: at every shape of the sweep a
    seed exists at which M is nowhere within 1e-5 of thresholdM, so every cell's s = 1.5 / 0 decision can be compared."""
    for w, h in edges.ROBUST_FUSED_SHAPES:
        for uv_scale in (1, 2):
            seed, mo = edges.robustness_seed(orc, w, h, uv_scale)
            assert np.abs(mo[1:-1, 1:-1, 3] - edges.THRESHOLD_M).min(initial=1.0) > 1e-5


# ---------------------------------------------------------------- tests/test_finish_edges_gpu.py
def test_finish_shapes_stay_small_and_cross_the_tile():
    for name, (fn, shp) in finish.CASES.items():
        assert 1 <= len(shp) <= 14 and len(set(shp)) == len(shp), name
        for s in shp:
            assert max(s) <= 300 and sorted(s)[-2] <= 120, (name, s)
    # the stencil kernels' tiles are what their queries say, and every list has tile - 1, tile and tile + 1 in both axes
    for name in ("sharpen", "denoise", "chain", "geometry"):
        tw, th = finish._tile(name)[:2]
        for entry in (f"mfsr_{name}Image", {"sharpen": "mfsr_finishSharpened", "denoise": "mfsr_finishDenoised", "chain": "mfsr_finishChain",
                                           "geometry": "mfsr_finishGeometry"}[name]):
            shp = finish.CASES[finish.SWEEP[entry]][1]
            assert shp[0] == (1, 1) and {(tw + dx, th + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)} <= set(shp), entry
            assert {s[0] for s in shp} >= {4 * tw - 1, 4 * tw, 4 * tw + 1}, entry       # an RGB8 lane owns four pixels
    for entry in ("mfsr_renderImage", "mfsr_finishRendered", "mfsr_localToneImage", "mfsr_finishLocalTone"):
        shp = finish.CASES[finish.SWEEP[entry]][1]
        assert {(64 + dx, 4 + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)} <= set(shp) and {s[0] for s in shp} >= {255, 256, 257}, entry
    # the two-plane formats: even sizes on both sides of 256 columns and of 8 rows (pairs of rows of a 64 x 4 block)
    for name in ("c_renderImageYuv", "c_finishRenderedYuv", "c_chainImage_two_plane", "c_finishChain_two_plane"):
        assert all(w % 2 == 0 and h % 2 == 0 for w, h in finish.CASES[name][1]), name
    assert {(256 + dx, 8 + dy) for dx in (-2, 0, 2) for dy in (-2, 0, 2)} <= set(finish.YUV)
    # the shapes that also run both ways of reading the tone table: the smallest, tile + 1 both ways, the odd one
    for name, (fn, shp) in finish.CASES.items():
        if len(shp) >= 11 and name not in ("c_imageStats", "c_toneGridStats"):
            (w9, h9), (w0, h0) = shp[9], shp[5]                # shp[5]: exactly one tile
            assert w9 > w0 and h9 > h0 and shp[10][0] > 128 and shp[10][1] > h9, name


def test_finish_sweeps_full_geometry_tiles_take_the_staged_path():
    """What tests/test_finish_edges_gpu.py's geometry cases rely on: at every shape with a full tile, for both mappings and both
    filters, the validated description has a step of about 1.25 and every FULL tile of the launched rectangle has a tap box
    inside the stage (mfsr_geometry_tile), so the staged path runs; the lens mapping gives the channels different source pixels
    (the shared-coordinate shortcut is off) and the plain one does not."""
    from tests import geometry_ref as G
    tw, th, stw, sth = finish._tile("geometry")
    full_tiles = 0
    for w, h in finish.GEOMETRY:
        for mapping in finish.LENS:
            for filt in finish.FILTERS.values():
                sw, sh, gd, (x0, y0, _, _) = finish.geometry_case(w, h, mapping, filt)
                finish._geometry_struct(gd)                       # mfsr_geometry_validate accepts it
                assert 1.0 <= gd["stepX"] <= 1.4, (w, h, gd["stepX"])
                for ty in range(h // th):
                    for tx in range(w // tw):
                        bx0, bx1, by0, by1 = G.tap_box(gd, sw, sh, (x0 + tx * tw, y0 + ty * th, tw, th))
                        assert bx1 - bx0 + 1 <= stw and by1 - by0 + 1 <= sth, (w, h, mapping, tx, ty)
                        full_tiles += 1
                m = G.coords(gd, sw, sh, (x0, y0, w, h))
                apart = bool((m["u"][..., 0] != m["u"][..., 2]).any() or (m["v"][..., 0] != m["v"][..., 2]).any())
                assert apart == (mapping == "lens") or (w, h) == (1, 1), (w, h, mapping)
    assert full_tiles >= 2 * 2 * 8


def test_finish_sweeps_borrowed_comparisons_are_not_vacuous():
    """tests/test_robustness_group_gpu.py asserts that its planted flows put pixels outside the image, and
    tests/test_noise_temporal_gpu.py that pairs are accepted: both hold at the sweep's shapes, from the inputs alone."""
    from tests.noise_temporal_ref import DEFAULT_TOL, stats_temporal_rule
    from tests.test_noise_cpu import BLACK, SAT, full_rect
    from tests.test_noise_temporal_gpu import _block_flow, _const, _noise
    from tests.test_robustness_group_gpu import _planted_flow
    for w, h in finish.CASES["c_robustnessMaskGroup"][1]:
        if (w, h) != (3, 3):
            for n in (1, 2, 3, 4):
                assert min(_planted_flow(w, h, 31 * w + 5 * n + k)[1] for k in range(n)) > 0, (w, h, n)
    for w, h in finish.NOISE_TEMPORAL:
        host = _noise(3, w, h, 30 + w)
        flows = [_block_flow(w, h, False, _const(w, h, *s)) for s in ((0, 0), (1, -1), (-3, 2))]
        terms = int(stats_temporal_rule(host, flows, full_rect(w, h), DEFAULT_TOL, BLACK, SAT)[2][0].sum())
        assert terms >= (0 if (w, h) == (8, 8) else 3), (w, h, terms)
