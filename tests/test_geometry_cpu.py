"""The geometric finish without a device: the numpy restatement (tests/geometry_ref.py) on the identity,
mfsr_geometry_lens / _defaults / _validate (host-only entry points of the library) against a double-precision recomputation and
every refusal the header lists, the header's no-NaN / no-overflow claim at the extreme corners, and what the correction does to
a distorted dot grid (tools/geometry_quality.py)."""
import ctypes
import itertools

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi
from tests import geometry_ref as G

f32 = np.float32


def _image(h, w, seed):
    return np.random.default_rng(seed).uniform(0.01, 4.0, (h, w, 3)).astype(f32)


# ---- 1. identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", [G.BILINEAR, G.CUBIC], ids=["bilinear", "cubic"])
@pytest.mark.parametrize("w,h", [(8, 5), (70, 37)])
def test_the_restatement_on_the_identity_returns_its_input(w, h, filt):
    p = _image(h, w, 10 * w + h)
    g = G.identity(w, h, filt)
    m = G.coords(g, w, h)
    assert np.array_equal(m["ix"], np.broadcast_to(np.arange(w)[None, :, None], (h, w, 3)))
    assert np.array_equal(m["iy"], np.broadcast_to(np.arange(h)[:, None, None], (h, w, 3)))
    assert not m["fx"].any() and not m["fy"].any()
    assert np.array_equal(G.resample(p, g).view(np.uint32), p.view(np.uint32))
    # ... and a rectangle of the output is the crop
    rect = (1, 2, w - 3, h - 2)
    assert np.array_equal(G.resample(p, g, rect).view(np.uint32), p[2:h, 1:w - 2].view(np.uint32))


# ---- 2. the host entry points -----------------------------------------------------------------------------------------------
def _struct(d):
    g = capi.Geometry()
    for key in ("outW", "outH", "filter", "ocx", "ocy", "scx", "scy", "stepX", "stepY", "rnorm2"):
        setattr(g, key, d[key] if isinstance(d[key], int) else float(d[key]))
    for c in range(3):
        for i in range(4):
            g.k[c][i] = float(d["k"][c][i])
    return g


def _as_dict(g):
    return dict(outW=g.outW, outH=g.outH, filter=g.filter, ocx=f32(g.ocx), ocy=f32(g.ocy), scx=f32(g.scx), scy=f32(g.scy),
                stepX=f32(g.stepX), stepY=f32(g.stepY), rnorm2=f32(g.rnorm2), k=np.array([[g.k[c][i] for i in range(4)] for c in range(3)], f32))


LENS_CASES = [(192, 128, 144, 96, 1.0, (0.1, 0.0, 0.0), (1.003, 0.998), "cubic"),
              (4032, 3024, 3840, 2160, 1.0, (0.0, 0.0, 0.0), (1.0, 1.0), "bilinear"),
              (7680, 4320, 5760, 3240, 1.25, (-0.21, 0.043, -0.0071), (1.0021, 0.9983), "cubic"),
              (1, 1, 1, 1, 1.0, (0.0, 0.0, 0.0), (1.0, 1.0), "cubic"),
              (5, 3, 9, 7, 1.0, (0.2, -0.05, 0.0), (1.004, 0.997), "bilinear")]


@pytest.mark.parametrize("case", LENS_CASES, ids=lambda c: f"{c[0]}x{c[1]}to{c[2]}x{c[3]}")
def test_lens_geometry_equals_a_double_precision_recomputation(case):
    from multi_frame_super_resolution_amd.pipeline import lens_geometry
    sw, sh, ow, oh, zoom, k, lat, filt = case
    g = lens_geometry(sw, sh, ow, oh, zoom=zoom, distortion=k, lateral=lat, filter=filt)
    want = G.lens(sw, sh, ow, oh, zoom, k, lat, G.CUBIC if filt == "cubic" else G.BILINEAR)
    got = _as_dict(g)
    for key, v in want.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(v)), key
    assert got["stepX"] == f32(min(np.float64(sw) / ow, np.float64(sh) / oh) / zoom)
    assert all(v == 0 for v in g.reserved)
    assert capi.lib().raw["mfsr_geometry_validate"](ctypes.byref(g)) == 0


def test_geometry_defaults_is_the_identity():
    g = capi.Geometry()
    assert capi.lib().raw["mfsr_geometry_defaults"](70, 37, ctypes.byref(g)) == 0
    want = G.identity(70, 37)
    got = _as_dict(g)
    for key, v in want.items():
        assert np.array_equal(np.asarray(got[key]), np.asarray(v)), key
    assert (g.outW, g.outH, g.filter, g.stepX, g.k[0][0], g.k[2][0]) == (70, 37, capi.GEO_CUBIC, 1.0, 1.0, 1.0)
    tw, th, sw, sh = (ctypes.c_int(0) for _ in range(4))
    assert capi.lib().raw["mfsr_geometry_tile"](*(ctypes.byref(v) for v in (tw, th, sw, sh))) == 0
    # the stage holds an identity tile's taps: the default takes the staged path
    assert tw.value > 0 and th.value > 0 and sw.value >= tw.value + 3 and sh.value >= th.value + 3


def _bad(**changes):
    d = G.lens(192, 128, 144, 96, distortion=(0.1, 0.0, 0.0), lateral=(1.003, 0.998))
    d["k"] = d["k"].copy()
    for key, v in changes.items():
        if key.startswith("k"):
            d["k"][int(key[1]), int(key[2])] = v
        else:
            d[key] = v
    return _struct(d)


REFUSALS = [dict(outW=0), dict(outW=32769), dict(outH=0), dict(outH=32769), dict(filter=2), dict(filter=-1),
            dict(ocx=np.nan), dict(ocy=np.inf), dict(scx=-np.inf), dict(scy=np.nan), dict(stepX=np.nan), dict(stepY=np.inf),
            dict(rnorm2=np.inf), dict(rnorm2=np.nan), dict(k00=np.nan), dict(k13=np.inf), dict(k22=-np.inf),
            dict(stepX=0.124), dict(stepX=8.01), dict(stepY=0.0), dict(stepY=-1.0), dict(stepY=9.0),
            dict(rnorm2=0.0), dict(rnorm2=-1e-6), dict(rnorm2=4.5),
            dict(k00=1.26), dict(k10=0.74), dict(k20=-1.0),
            dict(k01=4.01), dict(k12=-4.01), dict(k23=5.0),
            dict(ocx=-144.5), dict(ocx=288.5), dict(ocy=-96.5), dict(ocy=192.5), dict(scx=-32769.0), dict(scy=65537.0)]


@pytest.mark.parametrize("changes", REFUSALS, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_geometry_validate_refuses(changes):
    validate = capi.lib().raw["mfsr_geometry_validate"]
    assert validate(ctypes.byref(_bad())) == 0
    assert validate(ctypes.byref(_bad(**changes))) == -1


def test_geometry_validate_refuses_null_reserved_and_accepts_the_bounds():
    validate = capi.lib().raw["mfsr_geometry_validate"]
    assert validate(None) == -1
    for i in range(10):
        g = _bad()
        g.reserved[i] = 1
        assert validate(ctypes.byref(g)) == -1, i
    edge = _bad(outW=32768, outH=1, ocx=-32768.0, ocy=2.0, stepX=0.125, stepY=8.0, rnorm2=4.0, k00=1.25, k10=0.75, k01=4.0, k12=-4.0,
                k23=4.0)
    assert validate(ctypes.byref(edge)) == 0
    # the launch bounds the source centre by ITS source, and a rectangle by the output, on the host and before any device call
    # (the pointers are host memory that is never touched)
    src = np.zeros((128, 192, 3), f32)
    dst = np.zeros((96, 144, 3), f32)
    image = capi.lib().raw["mfsr_geometryImage"]
    for g, rect in ((_bad(scx=385.0), (0, 0, 144, 96)), (_bad(scy=-129.0), (0, 0, 144, 96)), (_bad(), (1, 0, 144, 96)),
                    (_bad(), (0, 90, 10, 7)), (_bad(), (-1, 0, 10, 7)), (_bad(), (0, 0, 0, 7))):
        assert image(src.ctypes.data, 12 * 192, 192, 128, dst.ctypes.data, 12 * 144, None, 0, None, ctypes.byref(g), 0, *rect, None) == -1
    yuv = capi.Render()
    yuv.format = capi.OUT_NV12
    assert image(src.ctypes.data, 12 * 192, 192, 128, dst.ctypes.data, 12 * 144, None, 0, ctypes.byref(yuv), ctypes.byref(_bad()), 0,
                 0, 0, 144, 96, None) == -1
    assert image(src.ctypes.data, 12 * 192, 192, 128, src.ctypes.data + 12, 12 * 144, None, 0, None, ctypes.byref(_bad()), 0, 0, 0, 144, 96,
                 None) == -1   # the output overlaps the input


def test_no_nan_and_no_overflow_at_the_extreme_corners():
    """include/mfsr.h: with validate's bounds m is finite (so dx * m is never 0 * inf = NaN), u lies in [-1, srcW] after the clamp,
    ix in [-1, srcW], the fraction in [0, 1).  A 32768-wide output and source, every coefficient at its bound with every
    combination of signs, the centres at both ends of their ranges, the four corner pixels."""
    validate = capi.lib().raw["mfsr_geometry_validate"]
    n = 32768
    worst_m = 0.0
    for oc, sc, k0, (s1, s2, s3), step, rn in itertools.product((-float(n), 2.0 * n), (-float(n), 2.0 * n), (0.75, 1.25),
                                                                 itertools.product((-4.0, 4.0), repeat=3), (0.125, 8.0), (4.0, 1e-30)):
        k = np.array([[k0, s1, s2, s3]] * 3, f32)
        d = dict(outW=n, outH=n, filter=G.CUBIC, ocx=f32(oc), ocy=f32(oc), scx=f32(sc), scy=f32(sc), stepX=f32(step), stepY=f32(step),
                 rnorm2=f32(rn), k=k)
        assert validate(ctypes.byref(_struct(d))) == 0
        for x, y in ((0, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 1)):
            m = G.coords(d, n, n, (x, y, 1, 1))
            assert np.isfinite(m["rho"]).all() and np.isfinite(m["m"]).all()
            worst_m = max(worst_m, float(np.abs(m["m"]).max()))
            for key, lim in (("u", n), ("v", n)):
                assert not np.isnan(m[key]).any() and (m[key] >= -1.0).all() and (m[key] <= lim).all()
            for key in ("ix", "iy"):
                assert (m[key] >= -1).all() and (m[key] <= n).all()
            for key in ("fx", "fy"):
                assert (m[key] >= 0.0).all() and (m[key] < 1.0).all()
    assert 2.0 ** 124 < worst_m < 2.0 ** 126   # the bound the header derives is reached, and holds


# ---- 3. quality -------------------------------------------------------------------------------------------------------------
def test_correcting_a_distorted_dot_grid_moves_the_dots_back_and_closes_the_fringes():
    """tools/geometry_quality.py: the worst dot displacement from the ideal grid and the worst red / blue to green centroid
    distance both fall, for both filters.  (Measured: README.md and DESIGN.md section 2.27 quote the figures.)"""
    from tools import geometry_quality as Q
    r = Q.measure()
    print(r)
    for filt in ("cubic", "bilinear"):
        assert r[filt]["displacement_px"] < r["before"]["displacement_px"], (filt, r)
        assert r[filt]["fringe_px"] < r["before"]["fringe_px"], (filt, r)
