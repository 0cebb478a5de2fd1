"""The geometric finish without a device: the numpy restatement (tests/geometry_ref.py) on the identity,
mfsr_geometry_lens / _defaults / _validate (host-only entry points of the library) against a double-precision recomputation and
every refusal the header lists, the header's no-NaN / no-overflow claim at the extreme corners, what the correction does to
a distorted dot grid (tools/geometry_quality.py), an affine ramp against the float64 value of the header's mapping (an anchor
that does not share the restatement's coordinate code; tests/test_geometry_gpu.py holds the device to the same), and the search
for launches whose boxes of source taps are exactly the stage's capacity and one more."""
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


# ---- 4. an anchor outside the restatement: affine ramps ----------------------------------------------------------------------
# Both kernels reproduce an affine function exactly wherever no tap clamps (the bilinear weights and the Catmull-Rom weights
# sum to 1 and have the first moment f), so there the output is the ramp at the source coordinate, whatever the restatement
# says.  Dyadic coefficients: the ramp is exact in float32 on every source used here.
RAMP_A, RAMP_B, RAMP_C = (0.5, 1.0, 0.25), (1 / 64, -1 / 128, 1 / 32), (1 / 128, 1 / 64, -1 / 64)
ANCHOR_CASES = [(70, 37, 131, 67), (70, 37, 53, 29), (300, 200, 257, 129)]


def affine_ramp(sw, sh):
    yy, xx = np.mgrid[0:sh, 0:sw].astype(np.float64)
    p = np.stack([a + b * xx + c * yy for a, b, c in zip(RAMP_A, RAMP_B, RAMP_C)], axis=-1)
    assert np.array_equal(p.astype(f32).astype(np.float64), p)
    return p.astype(f32)


def anchor_description(sw, sh, ow, oh, filt):
    return G.lens(sw, sh, ow, oh, distortion=(0.2, -0.05, 0.0), lateral=(1.004, 0.997), filter=filt)


def anchor_expected(g, sw, sh):
    """include/mfsr.h's mapping in float64 from the float32 fields of the description, without the clamp:
    (the ramp at (u, v) [outH, outW, 3], the mask of pixels whose taps all lie inside the source by 0.01 px, the bound)."""
    d = np.float64
    X, Y = np.arange(g["outW"], dtype=d) + 0.5, np.arange(g["outH"], dtype=d) + 0.5
    dx = ((X - d(g["ocx"])) * d(g["stepX"]))[None, :, None]
    dy = ((Y - d(g["ocy"])) * d(g["stepY"]))[:, None, None]
    rho = (dx * dx + dy * dy) * d(g["rnorm2"])
    k = np.asarray(g["k"], d)
    m = ((k[:, 3] * rho + k[:, 2]) * rho + k[:, 1]) * rho + k[:, 0]
    u, v = d(g["scx"]) + dx * m - 0.5, d(g["scy"]) + dy * m - 0.5
    want = np.asarray(RAMP_A) + np.asarray(RAMP_B) * u + np.asarray(RAMP_C) * v
    before, after = (1, 2) if g["filter"] == G.CUBIC else (0, 1)       # the taps are floor(u) - before .. floor(u) + after
    inside = ((u >= before + 0.01) & (u <= sw - after - 0.01) & (v >= before + 0.01) & (v <= sh - after - 0.01)).all(axis=-1)
    slope = max(abs(b) + abs(c) for b, c in zip(RAMP_B, RAMP_C))
    pmax = np.abs(affine_ramp(sw, sh)).max()
    bound = slope * 32 * float(np.spacing(f32(max(sw, sh)))) + 16 * float(np.spacing(f32(pmax)))
    return want, inside, bound


def assert_affine_anchor(o, g, sw, sh, what):
    """o [outH, outW, 3] float32 against the ramp at the float64 coordinate; returns (share compared, largest error, bound)"""
    want, inside, bound = anchor_expected(g, sw, sh)
    share = float(inside.mean())
    err = float(np.abs(o.astype(np.float64) - want)[inside].max())
    print(f"{what}: {share:.2f} of the output compared, largest error {err:.2e}, bound {bound:.2e}")
    assert share >= 0.7, (what, share)
    assert err <= bound, (what, err, bound)
    return share, err, bound


@pytest.mark.parametrize("filt", [G.BILINEAR, G.CUBIC], ids=["bilinear", "cubic"])
@pytest.mark.parametrize("sw,sh,ow,oh", ANCHOR_CASES, ids=lambda v: str(v))
def test_the_restatement_reproduces_an_affine_ramp_at_the_float64_coordinate(sw, sh, ow, oh, filt):
    """A lens mapping with distortion (0.2, -0.05, 0) and lateral (1.004, 0.997): at every pixel none of whose taps clamps (at
    least 70 % of the output) the restatement's output is a + b u + c v at the coordinate of include/mfsr.h evaluated in float64,
    within max(|b| + |c|) * 32 ulp32(max(srcW, srcH)) + 16 ulp32(max |p|): the dozen float32 roundings of the coordinate chain,
    each at most half an ulp of a quantity no larger than twice the source extent, times the ramp's slope, plus the
    interpolation sums.  A wrong half-pixel convention moves the output by half a slope (4e-3 .. 2e-2), a wrong sign in a
    Catmull-Rom weight by more: both are hundreds of bounds away."""
    g = anchor_description(sw, sh, ow, oh, filt)
    o = G.resample(affine_ramp(sw, sh), g)
    share, err, bound = assert_affine_anchor(o, g, sw, sh, f"{sw}x{sh} -> {ow}x{oh} filter {filt}")
    # the test can fail: half a pixel off is far outside the bound
    shifted = dict(g, scx=f32(g["scx"] + 0.5))
    want, inside, _ = anchor_expected(shifted, sw, sh)
    assert np.abs(o.astype(np.float64) - want)[inside].max() > 100 * bound


# ---- 5. launches at the capacity of the stage -------------------------------------------------------------------------------
def geometry_tile():
    v = [ctypes.c_int(0) for _ in range(4)]
    assert capi.lib().raw["mfsr_geometry_tile"](*(ctypes.byref(x) for x in v)) == 0
    return tuple(x.value for x in v)


def capacity_edge(filt, axis):
    """A launch in which one tile's box of source taps is exactly the stage's capacity along `axis` ("x": stageW columns, "y":
    stageH rows), another tile's is one more, and every box fits along the other axis: (source width, source height, the
    description, the (columns, rows) of every tile's box).  Centres at the middle, k = (1, 0, 0, 0), a step of 1 along the other
    axis; the step along `axis` is the first of 1.300, 1.305 .. 2.495 that does it (the steps differ per filter: the cubic's
    box is two taps wider).  Raises AssertionError when there is none."""
    tw, th, stw, sth = geometry_tile()
    (ow, oh), (fx, fy) = ((4 * tw, 3 * th), (1.5625, 2.5)) if axis == "x" else ((tw, 8 * th), (1.5625, 2.34375))
    sw, sh = int(np.ceil(ow * fx)), int(np.ceil(oh * fy))
    for step in np.arange(1.3, 2.5, 0.005):
        g = dict(outW=ow, outH=oh, filter=filt, ocx=f32(ow / 2), ocy=f32(oh / 2), scx=f32(sw / 2), scy=f32(sh / 2),
                 stepX=f32(step if axis == "x" else 1), stepY=f32(step if axis == "y" else 1),
                 rnorm2=f32(1.0 / ((sw / 2) ** 2 + (sh / 2) ** 2)), k=np.array([[1, 0, 0, 0]] * 3, f32))
        boxes = []
        for ty in range(oh // th):
            for tx in range(ow // tw):
                x0, x1, y0, y1 = G.tap_box(g, sw, sh, (tx * tw, ty * th, tw, th))
                boxes.append((x1 - x0 + 1, y1 - y0 + 1))
        along, across = ([b[0] for b in boxes], [b[1] for b in boxes]) if axis == "x" else ([b[1] for b in boxes], [b[0] for b in boxes])
        cap, other = (stw, sth) if axis == "x" else (sth, stw)
        if cap in along and cap + 1 in along and max(across) <= other:
            return sw, sh, g, boxes
    raise AssertionError(f"no step puts boxes of {cap} and {cap + 1} along {axis} into one launch")


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("filt", [G.BILINEAR, G.CUBIC], ids=["bilinear", "cubic"])
def test_a_launch_with_boxes_at_the_capacity_of_the_stage_and_one_beyond_exists(filt, axis):
    """what tests/test_geometry_gpu.py's capacity-edge test launches: found, valid, and on both sides of `fits`"""
    tw, th, stw, sth = geometry_tile()
    sw, sh, g, boxes = capacity_edge(filt, axis)
    print(f"filter {filt} axis {axis}: source {sw} x {sh}, output {g['outW']} x {g['outH']}, step ({g['stepX']}, {g['stepY']}), "
          f"boxes {sorted(set(boxes))}")
    assert capi.lib().raw["mfsr_geometry_validate"](ctypes.byref(_struct(g))) == 0
    fits = [bw <= stw and bh <= sth for bw, bh in boxes]
    assert any(fits) and not all(fits)
    assert (stw, sth)[axis == "y"] in [b[axis == "y"] for b, f in zip(boxes, fits) if f]
    assert (stw, sth)[axis == "y"] + 1 in [b[axis == "y"] for b, f in zip(boxes, fits) if not f]
