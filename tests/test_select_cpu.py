"""Frame selection, host side (no device): the selection rule of mfsr_select_frames against a table, and the host validation
of mfsr_frameSharpness / mfsr_burst_select_frames, which must refuse bad arguments before any device call."""
import ctypes

import pytest

from multi_frame_super_resolution_amd import capi


def _lib():
    try:
        return capi.lib()
    except ImportError as e:
        pytest.skip(str(e))


def _select(sums, candidates=0, ratio=0.0, with_keep=True):
    L = _lib()
    n = len(sums)
    arr = (ctypes.c_longlong * max(n, 1))(*sums)
    ref = ctypes.c_int(-7)
    keep = (ctypes.c_int32 * max(n, 1))(*([9] * max(n, 1)))
    rc = L.raw["mfsr_select_frames"](n, arr, candidates, ctypes.c_float(ratio), ctypes.byref(ref), keep if with_keep else None)
    return rc, ref.value, [keep[k] for k in range(n)]


@pytest.mark.parametrize("sums,candidates,ratio,ref,keep", [
    ([5, 9, 9, 2], 0, 0.0, 1, [1, 1, 1, 1]),          # tie -> lowest index; ratio 0 keeps everything
    ([9, 9, 9], 0, 1.0, 0, [1, 1, 1]),                # ratio 1 keeps the ties (>=)
    ([3, 7, 10, 1], 0, 1.0, 2, [0, 0, 1, 0]),         # ratio 1: only the reference (and equals)
    ([50, 100, 49, 51], 0, 0.5, 1, [1, 1, 0, 1]),     # exact equality at 0.5 keeps the frame
    ([1, 2, 3, 4, 5], 1, 0.0, 0, [1, 1, 1, 1, 1]),    # candidates 1: frame 0, whatever the others score
    ([1, 8, 3, 9, 5], 3, 0.0, 1, [1, 1, 1, 1, 1]),    # candidates k: argmax over the first k
    ([1, 8, 3, 9, 5], 3, 0.9, 1, [0, 1, 0, 1, 0]),    # a later frame sharper than the reference is kept
    ([1, 8, 3, 9, 5], 5, 0.0, 3, [1, 1, 1, 1, 1]),    # candidates == n: all
    ([1, 8, 3, 9, 5], 99, 0.0, 3, [1, 1, 1, 1, 1]),   # candidates > n: all
    ([42], 0, 1.0, 0, [1]),                           # n = 1
    ([0, 0, 0], 0, 0.5, 0, [1, 1, 1]),                # all-zero scores (flat frames): 0 >= 0.5 * 0
    ([2**62 - 1, 2**62 - 2, 2**61], 0, 1.0, 0, [1, 1, 0]),  # large sums compare as doubles
])
def test_select_frames_table(sums, candidates, ratio, ref, keep):
    rc, r, k = _select(sums, candidates, ratio)
    assert rc == 0
    assert r == ref
    assert k == keep


def test_select_frames_keep_may_be_null():
    rc, r, _ = _select([4, 6, 5], 0, 0.5, with_keep=False)
    assert rc == 0 and r == 1


@pytest.mark.parametrize("n,candidates,ratio", [
    (0, 0, 0.0), (-1, 0, 0.0),                        # invalid n
    (3, -1, 0.0),                                     # negative candidates
    (3, 0, -0.01), (3, 0, 1.01), (3, 0, float("nan")), (3, 0, float("inf")),
])
def test_select_frames_invalid(n, candidates, ratio):
    L = _lib()
    arr = (ctypes.c_longlong * 4)(1, 2, 3, 4)
    ref, keep = ctypes.c_int(), (ctypes.c_int32 * 4)()
    assert L.raw["mfsr_select_frames"](n, arr, candidates, ctypes.c_float(ratio), ctypes.byref(ref), keep) == -1


def test_select_frames_null_outputs():
    L = _lib()
    arr = (ctypes.c_longlong * 2)(1, 2)
    keep = (ctypes.c_int32 * 2)()
    assert L.raw["mfsr_select_frames"](2, None, 0, ctypes.c_float(0.0), ctypes.byref(ctypes.c_int()), keep) == -1
    assert L.raw["mfsr_select_frames"](2, arr, 0, ctypes.c_float(0.0), None, keep) == -1


# ---- mfsr_frameSharpness: every case has a bad argument, so the fake pointers are never handed to the device ----
W, H = 260, 196
RGGB = (0, 1, 1, 2)
FAKE = 0x10000  # an aligned "device" pointer: validation fails before any device call, so it is never used


def _valid(n, frames, pitch, width, height, cfa, mono, rect, sums):
    """The argument contract of mfsr_frameSharpness, restated: a guard so that these tests never hand the fake pointers to a
    call that would pass validation and reach the device."""
    if n < 1 or frames is None or rect is None or sums is None:
        return False
    if any(not f or f % 2 for f in frames[:n]):
        return False
    if width <= 0 or height <= 0 or width % 2 or height % 2 or pitch < 2 * width or pitch % 2:
        return False
    if not mono and (cfa is None or sum(1 for c in cfa if c == 1) != 2):
        return False
    x0, y0, x1, y1 = rect
    if not (1 <= x0 < x1 <= width // 2 - 1 and 1 <= y0 < y1 <= height // 2 - 1):
        return False
    return (x1 - x0) * (y1 - y0) <= 1 << 23


def _sharp(n=2, frames="ok", pitch=2 * W, width=W, height=H, cfa=RGGB, mono=0, rect=(1, 1, W // 2 - 1, H // 2 - 1), sums=FAKE):
    L = _lib()
    if frames == "ok":
        frames = (ctypes.c_void_p * max(n, 1))(*([FAKE] * max(n, 1)))
    assert not _valid(n, None if frames is None else list(frames), pitch, width, height, cfa, mono, rect, sums), \
        "test bug: these arguments are valid and would reach the device"
    cfa_arr = None if cfa is None else (ctypes.c_int32 * 4)(*cfa)
    rect_arr = None if rect is None else (ctypes.c_int32 * 4)(*rect)
    return L.raw["mfsr_frameSharpness"](n, frames, pitch, width, height, cfa_arr, mono, rect_arr, sums, None)


@pytest.mark.parametrize("kw", [
    dict(n=0), dict(n=-3),
    dict(frames=None), dict(frames=(ctypes.c_void_p * 2)(FAKE, None)), dict(frames=(ctypes.c_void_p * 2)(FAKE, FAKE + 1)),
    dict(sums=None), dict(rect=None), dict(cfa=None),
    dict(pitch=2 * W - 2), dict(pitch=2 * W + 1), dict(pitch=0),
    dict(width=W + 1, pitch=2 * W + 2), dict(height=H + 1), dict(width=0), dict(height=-2),
    dict(cfa=(0, 1, 2, 2)), dict(cfa=(1, 1, 1, 2)), dict(cfa=(0, 2, 2, 0)), dict(cfa=(1, 1, 1, 1)),
    dict(rect=(0, 1, 10, 10)), dict(rect=(1, 0, 10, 10)),                        # touching column / row 0
    dict(rect=(1, 1, W // 2, 10)), dict(rect=(1, 1, 10, H // 2)),                # touching column / row W/2-1 (exclusive end past it)
    dict(rect=(5, 5, 5, 10)), dict(rect=(5, 5, 10, 5)), dict(rect=(9, 5, 5, 10)),  # empty / reversed
])
def test_frame_sharpness_host_validation(kw):
    assert _sharp(**kw) == -1


def test_frame_sharpness_area_limit():
    # 2^23 + 1 half-resolution pixels: refused; 2^23 exactly is the limit (not run here: it would launch)
    w, h = 2 * 4100, 2 * 2052
    assert _sharp(width=w, height=h, pitch=2 * w, rect=(1, 1, 1 + 4097, 1 + 2048)) == -1   # 4097 * 2048 = 2^23 + 2048
    assert _sharp(width=w, height=h, pitch=2 * w, rect=(1, 1, 1 + 4096, 1 + 2049)) == -1   # 4096 * 2049
    assert _valid(2, [FAKE, FAKE], 2 * w, w, h, RGGB, 0, (1, 1, 1 + 4096, 1 + 2048), FAKE)  # 2^23: the guard's own limit


def test_frame_sharpness_mono_ignores_cfa():
    # with mono the CFA is not read (NULL allowed): the only bad argument left is the empty rectangle
    assert _sharp(mono=1, cfa=None, rect=(5, 5, 5, 10)) == -1
    assert _sharp(mono=1, cfa=(0, 0, 0, 0), rect=(5, 5, 5, 10)) == -1


def test_burst_select_frames_host_validation():
    L = _lib()
    ref = ctypes.c_int()
    frames = (ctypes.c_void_p * 2)(FAKE, FAKE)
    assert L.raw["mfsr_burst_select_frames"](None, 2, frames, 0, ctypes.c_float(0.0), FAKE, ctypes.byref(ref), None, None, None,
                                             None) == -1


def test_select_declarations_parse():
    protos = capi.parse_header()
    for name in ("mfsr_frameSharpness", "mfsr_select_frames", "mfsr_burst_select_frames"):
        assert name in protos and protos[name][0] == "int"
    args = protos["mfsr_burst_select_frames"][1]
    assert [a for _, a in args] == ["b", "nFrames", "frames", "candidates", "keepRatio", "sumsDev", "reference", "keep", "sums",
                                    "rect", "stream"]
