"""bench.py plain vs --full on the smallest workload: a plain run leaves the legs --full adds (CPU oracle baseline, H2D -> D2H
end-to-end leg) null, --full runs them, and both time the same bursts: same image checksum, same --dump-outputs sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "1080p5_gray_x2", "--steps", "3",
                        "--warmup", "1"] + args, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_and_full_lines_and_dumps(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--full", "--dump-outputs", str(tmp_path / "full")])
    for d in (plain, full):
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["roofline"]["launches_timed"] > 0
    assert plain["end_to_end"] is None and plain["cpu_baseline"] is None
    e2e = full["end_to_end"]
    assert e2e is not None and e2e["ms_median"] > 0 and e2e["back_to_back"]["images_identical_to_single_burst"]
    cb = full["cpu_baseline"]
    assert cb is not None and cb["value"] > 0 and "error" not in cb["parity_on_sample"], cb
    assert plain["out16_sha256_16"] and plain["out16_sha256_16"] == full["out16_sha256_16"]
    a = np.load(tmp_path / "plain" / "out16_sample.npy")
    b = np.load(tmp_path / "full" / "out16_sample.npy")
    assert a.dtype == np.float32 and a.size > 0 and a.max() > 0
    np.testing.assert_array_equal(a, b)
