"""The band logic of tests/guards.py catches a one-element overrun before and after the data.

Runs on the CPU with the oracle backend: the oracle's kernels take raw pointers and byte pitches like the HIP ones, so a
misdeclared call really writes outside the array -- into the band, which the test owns.  The same ``check_bands`` decides
for the device buffers of ``tests/kernels.py::guarded_upload``.
"""
import numpy as np
import pytest

from tests.guards import Guard, band_report, check_bands, layout
from tests.kernels import pitch_of

H, W = 5, 7


def _rgb(w):
    return np.random.default_rng(3).random((H, w, 3), dtype=np.float32)


def test_correct_call_leaves_both_bands(orc):
    g = Guard()
    rgb = _rgb(W)
    out = g.zeros((H, W))
    orc.call("rgbToGray", rgb, pitch_of(rgb), out, pitch_of(out), W, H)
    g.check("rgbToGray")
    assert out.min() > 0


def test_overrun_after_the_data_is_caught(orc):
    """Width declared one too large on a pitched output: element W of the last row is the first element of the trailing band."""
    g = Guard()
    rgb = _rgb(W + 1)
    out = g.zeros((H, W))
    orc.call("rgbToGray", rgb, pitch_of(rgb), out, pitch_of(out), W + 1, H)
    big, off, nbytes = g.bufs[0]
    assert band_report(big, off, nbytes, g.fill) == ("trailing", nbytes)
    with pytest.raises(AssertionError, match=r"rgbToGray: write outside the buffer: trailing guard changed, first at byte 140 "):
        g.check("rgbToGray")


def test_overrun_before_the_data_is_caught(orc):
    """The same misdeclared call on an output that starts one element early: its first write is the last element of the
    leading band (and the extra column of the last row is the last element of the data: the trailing band stays intact)."""
    g = Guard()
    rgb = _rgb(W + 1)
    out = g.zeros((H, W))
    big, off, nbytes = g.bufs[0]
    early = big[off - 4:off - 4 + nbytes].view(np.float32).reshape(H, W)
    orc.call("rgbToGray", rgb, pitch_of(rgb), early, pitch_of(early), W + 1, H)
    assert band_report(big, off, nbytes, g.fill) == ("leading", -4)
    with pytest.raises(AssertionError, match=r"leading guard changed, first at byte -4 "):
        g.check("rgbToGray")


def test_layout_and_single_bytes():
    off, total = layout(10, 4096, 256)
    assert off == 4096 and total == 4096 + 10 + 4096          # the trailing band starts right after the data
    off, total = layout(10, 100, 256)
    assert off == 256 and total == 256 + 10 + 100
    for pos, want in ((0, ("leading", -256)), (255, ("leading", -1)), (266, ("trailing", 10)), (total - 1, ("trailing", 109))):
        big = np.full(total, 0xFF, np.uint8)
        big[off:off + 10] = 0
        check_bands(big, off, 10, 0xFF, "untouched")
        big[pos] ^= 1
        assert band_report(big, off, 10, 0xFF) == want
