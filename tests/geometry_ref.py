"""numpy float32 restatement of the geometric finish (include/mfsr.h, mfsr_geometry): per output pixel and
per channel a source coordinate and a bilinear or Catmull-Rom kernel over the NaN-cleaned source.  Every statement is one float32
operation with one rounding, in the header's order, so the result is bit-exact; tests/render_ref.py takes it from there (matrix,
tone, store)."""
from __future__ import annotations

import numpy as np

BILINEAR, CUBIC = 0, 1
f32 = np.float32


def lens(src_w, src_h, out_w, out_h, zoom=1.0, distortion=(0.0, 0.0, 0.0), lateral=(1.0, 1.0), filter=CUBIC):
    """mfsr_geometry_lens: doubles, rounded once.  A dict with the struct's field names; k is float32 [3, 4]."""
    k = np.zeros((3, 4), f32)
    k[:, 0] = [f32(lateral[0]), f32(1.0), f32(lateral[1])]
    k[:, 1:] = np.asarray(distortion, np.float64).astype(f32)
    step = f32(min(src_w / out_w, src_h / out_h) / zoom)
    return dict(outW=int(out_w), outH=int(out_h), filter=int(filter), ocx=f32(out_w / 2.0), ocy=f32(out_h / 2.0), scx=f32(src_w / 2.0),
                scy=f32(src_h / 2.0), stepX=step, stepY=step, rnorm2=f32(1.0 / ((src_w / 2.0) ** 2 + (src_h / 2.0) ** 2)), k=k)


def identity(src_w, src_h, filter=CUBIC):
    """mfsr_geometry_defaults (with a choice of filter)"""
    return lens(src_w, src_h, src_w, src_h, filter=filter)


def _axis(centre, d, m, n):
    """u, clamped; its floor as int64 and the fraction"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = (d * m).astype(f32)
        u = (f32(centre) + t).astype(f32)
        u = (u - f32(0.5)).astype(f32)
    u = np.fmin(np.fmax(u, f32(-1.0)), f32(n)).astype(f32)   # fmaxf / fminf: a NaN gives the other argument
    i = np.floor(u).astype(np.int64)
    f = (u - i.astype(f32)).astype(f32)
    return u, i, f


def coords(g, src_w, src_h, rect=None):
    """The mapping of the rectangle (x, y, w, h) of the full output (None: all of it): a dict of float32 / int64 arrays
    [h, w, 3] -- u, v, ix, iy, fx, fy -- and m [h, w, 3], rho [h, w]."""
    x0, y0, w, h = (0, 0, g["outW"], g["outH"]) if rect is None else rect
    X = (np.arange(x0, x0 + w, dtype=np.int64).astype(f32) + f32(0.5)).astype(f32)
    Y = (np.arange(y0, y0 + h, dtype=np.int64).astype(f32) + f32(0.5)).astype(f32)
    dx = ((X - f32(g["ocx"])).astype(f32) * f32(g["stepX"])).astype(f32)[None, :]
    dy = ((Y - f32(g["ocy"])).astype(f32) * f32(g["stepY"])).astype(f32)[:, None]
    k = np.asarray(g["k"], f32)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
        rho = (r2 * f32(g["rnorm2"])).astype(f32)
        out = {key: [] for key in ("u", "v", "ix", "iy", "fx", "fy", "m")}
        for c in range(3):
            m = (k[c, 3] * rho).astype(f32)
            m = (m + k[c, 2]).astype(f32)
            m = (m * rho).astype(f32)
            m = (m + k[c, 1]).astype(f32)
            m = (m * rho).astype(f32)
            m = (m + k[c, 0]).astype(f32)
            u, ix, fx = _axis(g["scx"], np.broadcast_to(dx, m.shape), m, src_w)
            v, iy, fy = _axis(g["scy"], np.broadcast_to(dy, m.shape), m, src_h)
            for key, val in (("u", u), ("v", v), ("ix", ix), ("iy", iy), ("fx", fx), ("fy", fy), ("m", m)):
                out[key].append(val)
    res = {key: np.stack(val, axis=-1) for key, val in out.items()}
    res["rho"] = rho
    return res


def _cubic_weights(f):
    w0 = (f32(-0.5) * f).astype(f32)
    w0 = (w0 + f32(1.0)).astype(f32)
    w0 = (w0 * f).astype(f32)
    w0 = (w0 - f32(0.5)).astype(f32)
    w0 = (w0 * f).astype(f32)
    w1 = (f32(1.5) * f).astype(f32)
    w1 = (w1 - f32(2.5)).astype(f32)
    w1 = (w1 * f).astype(f32)
    w1 = (w1 * f).astype(f32)
    w1 = (w1 + f32(1.0)).astype(f32)
    w2 = (f32(-1.5) * f).astype(f32)
    w2 = (w2 + f32(2.0)).astype(f32)
    w2 = (w2 * f).astype(f32)
    w2 = (w2 + f32(0.5)).astype(f32)
    w2 = (w2 * f).astype(f32)
    w3 = (f32(0.5) * f).astype(f32)
    w3 = (w3 - f32(0.5)).astype(f32)
    w3 = (w3 * f).astype(f32)
    w3 = (w3 * f).astype(f32)
    return w0, w1, w2, w3


def resample(p, g, rect=None):
    """o of the rectangle (x, y, w, h) of the full output (None: all of it) from the source image p [srcH, srcW, 3]."""
    p = np.asarray(p, f32)
    src_h, src_w = p.shape[:2]
    s = np.where(np.isnan(p), f32(0), p).astype(f32)
    m = coords(g, src_w, src_h, rect)
    o = np.empty(m["ix"].shape, f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(3):
            ix, iy, fx, fy = m["ix"][..., c], m["iy"][..., c], m["fx"][..., c], m["fy"][..., c]
            sc = s[..., c]

            def tap(i, j):
                return sc[np.clip(j, 0, src_h - 1), np.clip(i, 0, src_w - 1)]

            if g["filter"] == BILINEAR:
                h = []
                for j in (iy, iy + 1):
                    a, b = tap(ix, j), tap(ix + 1, j)
                    d = (b - a).astype(f32)
                    d = (d * fx).astype(f32)
                    h.append((a + d).astype(f32))
                d = (h[1] - h[0]).astype(f32)
                d = (d * fy).astype(f32)
                o[..., c] = (h[0] + d).astype(f32)
            else:
                w = _cubic_weights(fx)
                wy = _cubic_weights(fy)
                h = []
                for dj in range(-1, 3):
                    t = [(w[i] * tap(ix - 1 + i, iy + dj)).astype(f32) for i in range(4)]
                    h.append(((t[0] + t[1]).astype(f32) + (t[2] + t[3]).astype(f32)).astype(f32))
                t = [(wy[j] * h[j]).astype(f32) for j in range(4)]
                o[..., c] = ((t[0] + t[1]).astype(f32) + (t[2] + t[3]).astype(f32)).astype(f32)
    return o


def tap_box(g, src_w, src_h, rect):
    """(x0, x1, y0, y1): the bounding box of the clamped source taps of the output rectangle (what a workgroup stages)"""
    m = coords(g, src_w, src_h, rect)
    before, after = (1, 2) if g["filter"] == CUBIC else (0, 1)
    cl = lambda v, n: int(min(max(v, 0), n - 1))   # noqa: E731
    return (cl(m["ix"].min() - before, src_w), cl(m["ix"].max() + after, src_w), cl(m["iy"].min() - before, src_h),
            cl(m["iy"].max() + after, src_h))
