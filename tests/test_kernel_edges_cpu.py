"""Coverage gate of tests/test_kernel_edges_gpu.py: every entry point of include/mfsr.h that takes a pitch or a width is in
the edge sweep or the row-stripe tests there, or is listed here with the reason it is not.  A kernel added later without
either fails this test.  Also what the sweep decides from the oracle alone (the robustness seeds), checked on the CPU."""
import re

import numpy as np

from multi_frame_super_resolution_amd.capi import parse_header
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
}

GEOMETRY = re.compile(r"pitch|stride|^width$|^imgWidth$|^dimX$|^outW$|^cols$|^step", re.I)


def _geometry_entries():
    out = []
    for name, (_, args) in parse_header().items():
        if any(GEOMETRY.search(a) for _, a in args):
            out.append(name)
    return out


def test_every_pitched_entry_point_is_swept_or_excluded():
    covered = set(edges.SWEEP) | set(edges.ROW_STRIPE_TESTS)
    names = _geometry_entries()
    assert len(names) > 60
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
