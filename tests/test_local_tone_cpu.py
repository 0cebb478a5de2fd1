"""Local tone mapping in the finish without a device: the numpy restatement's own properties, the host
fit of the library against it, validation, the defaults, and the direction of the effect against a global curve."""
import ctypes

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi, synth
from tests import local_tone_ref as T

INVALID = -1
CCM = np.array([1.62, -0.41, -0.21, -0.33, 1.55, -0.22, 0.05, -0.61, 1.56], np.float32)


def _lt(cell=16, bins=16, smooth=1, shadows=0.5, highlights=0.25, pivot=0.0, max_gain=4.0):
    lt = capi.LocalTone()
    lt.cell, lt.bins, lt.smooth = cell, bins, smooth
    lt.shadows, lt.highlights, lt.pivot, lt.maxGain = shadows, highlights, pivot, max_gain
    return lt


def _image(h, w, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.1, 1.1, (h, w, 3)).astype(np.float32)
    p[::7, ::5] = np.array([np.nan, 2.0, -1.0], np.float32)
    p[: h // 2, : w // 3] *= np.float32(0.05)          # a dark corner: entries far below the pivot
    return p


def _ulps(a, b):
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


def _lib_fit(table, fw, fh, lt):
    L = capi.lib()
    gx, gy, gz = T.grid_size(fw, fh, lt.cell, lt.bins)
    t = np.ascontiguousarray(table, np.uint64).reshape(-1)
    assert t.size == 2 * gx * gy * gz
    grid = np.full((gy, gx, gz), np.nan, np.float32)
    pivot, st = ctypes.c_double(-1.0), ctypes.c_int32(-1)
    L.local_tone_fit(t.ctypes.data, fw, fh, ctypes.byref(lt), grid.ctypes.data, ctypes.byref(pivot), ctypes.byref(st))
    return grid, pivot.value, st.value


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [None, CCM], ids=["plain", "matrix"])
def test_restatement_stripes_and_windows_add_up_to_the_whole(m):
    h, w, cell, bins = 75, 133, 16, 8
    p = _image(h, w, 3)
    whole = T.stats(p, cell, bins, m)
    assert whole.shape == (5, 9, 8, 2) and int(whole[..., 0].sum()) == h * w
    for rows in (1, 7, 16):
        t = np.zeros_like(whole)
        for y in range(0, h, rows):
            t += T.stats(p[y:y + rows], cell, bins, m, (0, y), (w, h))
        assert np.array_equal(t, whole), rows
    t = np.zeros_like(whole)
    for x0, y0, ww, hh in ((16, 16, 64, 32), (0, 0, w, 16), (0, 48, w, h - 48), (0, 16, 16, 32), (80, 16, w - 80, 32)):
        t += T.stats(p[y0:y0 + hh, x0:x0 + ww], cell, bins, m, (x0, y0), (w, h))
    assert np.array_equal(t, whole)


def test_restatement_slice_of_a_crop_is_the_crop_of_the_slice():
    h, w, cell = 40, 90, 16
    p = _image(h, w, 5)
    grid = np.random.default_rng(1).uniform(0.25, 4.0, (3, 6, 8)).astype(np.float32)
    whole = T.gain(p, grid, cell, CCM)
    part = T.gain(p[5:33, 16:70], grid, cell, CCM, (16, 5))
    assert np.array_equal(part.view(np.uint32), whole[5:33, 16:70].view(np.uint32))
    ones = T.gain(p, np.ones_like(grid), cell)
    assert np.array_equal(ones.view(np.uint32), np.ones((h, w), np.float32).view(np.uint32))


# ---- the library's fit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,smooth,pivot", [(16, 1, 0.0), (4, 0, 0.0), (32, 4, 0.0), (8, 2, 0.3)])
def test_fit_equals_the_restatement(bins, smooth, pivot):
    h, w = 75, 133
    table = T.stats(_image(h, w, bins), 16, bins, CCM)
    lt = _lt(16, bins, smooth, 0.5, 0.25, pivot, 4.0)
    got, piv, st = _lib_fit(table, w, h, lt)
    want, wpiv, wst = T.fit(table, smooth, 0.5, 0.25, pivot, 4.0)
    assert st == wst == 0 and abs(piv - wpiv) <= 1e-14 * wpiv
    assert (piv == float(np.float32(pivot))) if pivot > 0 else (0.0 < piv < 1.0)
    assert _ulps(got, want) <= 1, _ulps(got, want)
    assert got.min() < 1.0 < got.max()                 # both exponents act on this image


def test_fit_with_zero_exponents_is_exactly_one():
    table = T.stats(_image(40, 50, 2), 16, 16)
    got, _, st = _lib_fit(table, 50, 40, _lt(shadows=0.0, highlights=0.0))
    assert st == 0 and np.all(got.view(np.uint32) == 0x3F800000)


def test_fit_of_an_empty_table_sets_the_status():
    table = np.zeros((3, 4, 16, 2), np.uint64)
    got, piv, st = _lib_fit(table, 50, 40, _lt())
    want, wpiv, wst = T.fit(table)
    assert st == wst == 1 and piv == wpiv == 0.18
    assert _ulps(got, want) <= 1
    # every entry holds the gain of its bin's centre: the same along x and y
    assert np.all(got == got[:1, :1])


def test_fit_clamps_at_max_gain():
    h, w = 64, 64
    p = np.full((h, w, 3), 1e-3, np.float32)
    p[:, 32:] = 1.0
    table = T.stats(p, 16, 16)
    lt = _lt(smooth=0, shadows=1.0, highlights=1.0, pivot=0.25, max_gain=2.0)
    got, _, _ = _lib_fit(table, w, h, lt)
    want, _, _ = T.fit(table, 0, 1.0, 1.0, 0.25, 2.0)
    assert _ulps(got, want) <= 1
    assert got.max() == 2.0 and got.min() == 0.5
    assert np.all(got[:, :2, 0] == 2.0) and np.all(got[:, 2:, 15] == 0.5)       # the dark half's bin, the bright half's bin


# ---- validation, defaults, grid size --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,value", [
    ("cell", 8), ("cell", 24), ("cell", 1024), ("cell", 0), ("bins", 0), ("bins", 5), ("bins", 64), ("smooth", -1), ("smooth", 5),
    ("shadows", -0.1), ("shadows", 1.5), ("shadows", float("nan")), ("highlights", -0.1), ("highlights", 1.1),
    ("highlights", float("inf")), ("pivot", -0.1), ("pivot", 1.5), ("pivot", float("nan")), ("maxGain", 0.5), ("maxGain", 65.0),
    ("maxGain", float("nan")), ("reserved", 1)])
def test_validation_refuses_each_bad_field(field, value):
    raw = capi.lib().raw
    lt = _lt()
    assert raw["mfsr_local_tone_validate"](ctypes.byref(lt)) == 0
    if field == "reserved":
        lt.reserved[3] = value
    else:
        setattr(lt, field, value)
    assert raw["mfsr_local_tone_validate"](ctypes.byref(lt)) == INVALID
    g = ctypes.c_int()
    assert raw["mfsr_local_tone_grid"](64, 64, ctypes.byref(lt), ctypes.byref(g), ctypes.byref(g), ctypes.byref(g)) == INVALID
    st = ctypes.c_int32()
    table, grid = np.zeros(2 * 4096, np.uint64), np.zeros(4096, np.float32)
    assert raw["mfsr_local_tone_fit"](table.ctypes.data, 16, 16, ctypes.byref(lt), grid.ctypes.data, None, ctypes.byref(st)) == INVALID
    # the device entry points refuse it before any device call (the pointers are never dereferenced)
    r = capi.Render()
    assert raw["mfsr_toneGridStats"](0x100000, 192, 16, 4, 0, 0, 16, 4, None, ctypes.byref(lt), 0x200000, None) == INVALID
    assert raw["mfsr_localToneImage"](0x100000, 192, None, 0, 0x1000, 96, 16, 4, ctypes.byref(r), 0, 0x200000, ctypes.byref(lt),
                                      0, 0, 16, 4, None) == INVALID
    assert raw["mfsr_burst_set_local_tone"](None, ctypes.byref(lt), 0x200000) == INVALID


def test_entry_points_check_their_arguments_on_the_host():
    raw = capi.lib().raw
    lt, r = _lt(), capi.Render()
    assert raw["mfsr_local_tone_validate"](None) == INVALID
    img, tab, grid, out = 0x100000, 0x200000, 0x300000, 0x400000
    stats_ok = [img, 192, 16, 4, 0, 0, 16, 4, None, ctypes.byref(lt), tab, None]
    for pos, bad in ((0, None), (1, 188), (2, 0), (3, 0), (4, -1), (5, -1), (6, 15), (7, 3), (9, None), (10, None), (10, tab + 4)):
        a = list(stats_ok)
        a[pos] = bad
        assert raw["mfsr_toneGridStats"](*a) == INVALID, pos
    bad_m = (ctypes.c_float * 9)(*([1.0] * 8 + [float("nan")]))
    assert raw["mfsr_toneGridStats"](*(stats_ok[:8] + [bad_m] + stats_ok[9:])) == INVALID
    image_ok = [img, 192, None, 0, out, 96, 16, 4, ctypes.byref(r), 0, grid, ctypes.byref(lt), 0, 0, 16, 4, None]
    for pos, bad in ((0, None), (4, None), (5, 90), (8, None), (10, None), (10, grid + 2), (11, None), (12, 1), (13, -1), (14, 15)):
        a = list(image_ok)
        a[pos] = bad
        assert raw["mfsr_localToneImage"](*a) == INVALID, pos
    yuv = capi.Render()
    yuv.format = capi.OUT_NV12
    a = list(image_ok)
    a[8] = ctypes.byref(yuv)
    assert raw["mfsr_localToneImage"](*a) == INVALID
    res = capi.LocalToneResult()
    assert raw["mfsr_burst_local_tone"](None, img, img, None, tab, grid, ctypes.byref(res), None) == INVALID


@pytest.mark.parametrize("w,h,cell", [(1, 1, 16), (2049, 16, 32), (7680, 4320, 64), (2048, 2048, 16), (16, 65536, 512)])
def test_defaults_cell_rule(w, h, cell):
    lt = capi.LocalTone()
    capi.lib().local_tone_defaults(w, h, ctypes.byref(lt))
    assert lt.cell == cell == T.default_cell(w, h)
    assert (lt.bins, lt.smooth, lt.shadows, lt.highlights, lt.pivot, lt.maxGain) == (16, 1, 0.5, 0.25, 0.0, 4.0)
    assert list(lt.reserved) == [0, 0, 0, 0] and T.cdiv(max(w, h), lt.cell) <= 128
    gx, gy, gz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    capi.lib().local_tone_grid(w, h, ctypes.byref(lt), ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(gz))
    assert (gx.value, gy.value, gz.value) == T.grid_size(w, h, cell, 16)


def test_struct_sizes():
    assert ctypes.sizeof(capi.LocalTone) == 44 and ctypes.sizeof(capi.LocalToneResult) == 24


# ---- the direction of the effect -------------------------------------------------------------------------------------------------
def _patch_contrast(lum):
    """standard deviation of log-luma inside 8 x 8 patches, averaged over the patches"""
    h, w = lum.shape
    lg = np.log(np.maximum(lum.astype(np.float64), 1e-6)).reshape(h // 8, 8, w // 8, 8)
    return float(lg.std(axis=(1, 3)).mean())


def _luma(p):
    p = np.clip(p.astype(np.float64), 0.0, 1.0)
    return (54 * p[..., 0] + 183 * p[..., 1] + 19 * p[..., 2]) / 256.0


def local_and_global_contrast_ratios():
    """(local, global): the ratio after / before of the local contrast of the dark left half of a 256 x 192 synthetic scene,
    under the local operator with shadows = 0.5 and under the global power curve with the same mean lift of that half"""
    gen = torch.Generator().manual_seed(7)
    scene = synth._scene(192, 256, gen, "cpu").permute(1, 2, 0).numpy().astype(np.float32).copy()
    scene[:, :128] *= np.float32(1.0 / 16.0)
    grid, _, _ = T.fit(T.stats(scene, 16, 16), smooth=1, shadows=0.5, highlights=0.0, pivot=0.0, max_gain=64.0)
    local = T.apply(scene, grid, 16)
    left = (slice(None), slice(0, 128))
    before, lifted = _luma(scene)[left], _luma(local)[left]
    lift = lifted.mean() / before.mean()
    assert lift > 1.5
    # the global curve v -> v^e with the same mean luma over the left half: bisection on e in (0, 1]
    lo, hi = 0.05, 1.0
    for _ in range(60):
        e = 0.5 * (lo + hi)
        if _luma(np.clip(scene, 0, 1) ** e)[left].mean() > lifted.mean():
            lo = e
        else:
            hi = e
    glob = _luma(np.clip(scene, 0, 1) ** (0.5 * (lo + hi)))[left]
    assert abs(glob.mean() / lifted.mean() - 1.0) < 1e-6
    c0 = _patch_contrast(before)
    return _patch_contrast(lifted) / c0, _patch_contrast(glob) / c0


def test_local_operator_keeps_more_local_contrast_than_the_global_curve():
    local, glob = local_and_global_contrast_ratios()
    print(f"local contrast kept in the lifted shadows: local operator {local:.3f}, global curve {glob:.3f}")
    assert local > glob
