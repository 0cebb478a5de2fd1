"""bench.py's --dump-outputs writer and the plain / --full split of its legs (no GPU needed): the dumped values are the u16
samples exactly, a large image is reduced to the same seeded sample every time, and a plain run skips the legs --full adds."""
import os

import numpy as np
import pytest

import bench


def _image(h, w, seed):
    # int16 holding u16 bit patterns, as the pipeline's out16 (the full u16 range, the sign bit included)
    return np.random.default_rng(seed).integers(0, 1 << 16, size=(h, w, 3), dtype=np.uint32).astype(np.uint16).view(np.int16)


def test_small_image_is_dumped_whole_and_exact(tmp_path):
    img = _image(40, 64, 1)
    img.reshape(-1)[:2] = np.array([0, 65535], dtype=np.uint16).view(np.int16)
    bench.dump_outputs(str(tmp_path), img)
    assert os.listdir(tmp_path) == ["out16.npy"]
    got = np.load(tmp_path / "out16.npy")
    assert got.dtype == np.float32 and got.shape == img.shape
    np.testing.assert_array_equal(got, img.view(np.uint16).astype(np.float64))
    assert got.reshape(-1)[0] == 0.0 and got.reshape(-1)[1] == 65535.0


def test_large_image_is_sampled_at_fixed_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_SAMPLES", 1000)
    img = _image(50, 60, 2)                  # 9000 samples > 1000
    bench.dump_outputs(str(tmp_path / "a"), img)
    bench.dump_outputs(str(tmp_path / "b"), img.copy())
    assert os.listdir(tmp_path / "a") == ["out16_sample.npy"]
    a = np.load(tmp_path / "a" / "out16_sample.npy")
    b = np.load(tmp_path / "b" / "out16_sample.npy")
    assert a.dtype == np.float32 and a.shape == (1000,)
    np.testing.assert_array_equal(a, b)
    # the sample is the image's own values at the seeded, sorted flat positions
    idx = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).integers(0, img.size, size=1000))
    np.testing.assert_array_equal(a, img.view(np.uint16).reshape(-1)[idx].astype(np.float32))
    # a different image gives different values at the same positions
    bench.dump_outputs(str(tmp_path / "c"), _image(50, 60, 3))
    assert not np.array_equal(a, np.load(tmp_path / "c" / "out16_sample.npy"))


def test_headline_image_sample_stays_within_the_dump_limit():
    h, w, s = 2160, 3840, 2                  # the default workload's HR image
    assert h * s * w * s * 3 > bench.DUMP_MAX_SAMPLES
    assert bench.DUMP_MAX_SAMPLES * 4 <= 64 << 20


def test_plain_run_skips_the_full_legs():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_e2e and a.no_isolated


def test_full_runs_the_legs_unless_told_otherwise():
    a = bench.parse_args(["--full"])
    assert a.full and not a.no_cpu_baseline and not a.no_e2e and not a.no_isolated
    b = bench.parse_args(["--full", "--no-cpu-baseline", "--dump-outputs", "d"])
    assert b.no_cpu_baseline and not b.no_e2e and b.dump_outputs == "d"


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
