"""The robustness masks of a group in one pass, bit for bit against what it replaces:

* mfsr_prepareFrameMeansBatch against mfsr_prepareFrameFusedBatch: the means image is the numpy float32 restatement of the mask
  kernel's sum (from 0.0f, row-major over the individually clamped coordinates) and its exact division by 9, applied to the
  existing call's half-resolution image; both pyramid levels are the existing call's.
* mfsr_robustnessMaskGroup against mfsr_robustnessMaskFusedBatch on whole mask planes, ring and row padding included, with
  flows that put the displaced position on, next to and beyond every edge, on the round-half rule, and on NaN / Inf / -0.0.
* a 7-frame burst through BurstPipeline with the switch on and off: accumulators and out16.

Everything is compared on uint32 views, so NaN payloads and zero signs count."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(3, 3), (33, 9), (64, 16), (65, 17), (130, 35)]     # half-resolution (w, h): below, on and over the 64 x 8 / 64 x 16 tiles
TAPS = {5: [0.0625, 0.25, 0.375, 0.25, 0.0625], 3: [0.25, 0.5, 0.25]}
MAXVAL = 4095.0
ALPHA, BETA, THRESHOLD_M = 1e-4, 1e-6, 0.8
SENTINEL = 7.0
UNSUPPORTED = -2


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _raw_frames(w, h, n, seed):
    """n + 1 raw frames (reference first) of 2w x 2h samples: one smooth scene, shifted a little and with its own noise per frame"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:2 * h + 8, 0:2 * w + 8].astype(np.float64)
    scene = 1800.0 + 900.0 * np.sin(xx / 7.3 + 0.4) * np.cos(yy / 5.1) + 500.0 * np.sin((xx + 2 * yy) / 11.0)
    out = []
    for k in range(n + 1):
        dy, dx = (0, 0) if k == 0 else (2 * ((k + 1) // 2), 2 * (k // 2))
        f = scene[dy:dy + 2 * h, dx:dx + 2 * w] + r.normal(0.0, 25.0, (2 * h, 2 * w))
        out.append(torch.from_numpy(np.clip(np.rint(f), 0, 4095).astype(np.uint16).view(np.int16)).to("cuda:0"))
    return out


class _Prepared:
    """The products of both prepare calls for n moved frames, in buffers with padded rows filled with a sentinel."""

    def __init__(self, L, capi, raws, w, h, ntaps, means):
        dev = raws[0].device
        n = len(raws)
        self.half = [torch.full((h, w + 3, 3), SENTINEL, device=dev) for _ in range(n)]
        self.p0 = [torch.full((h, w + 5), SENTINEL, device=dev) for _ in range(n)]
        self.p1 = [torch.full((max(h // 2, 1), w // 2 + 3), SENTINEL, device=dev) for _ in range(n)]
        taps = (ctypes.c_float * ntaps)(*TAPS[ntaps])
        arr = (capi.PrepareFrame * n)(*[capi.PrepareFrame(r.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr())
                                        for r, a, b, c in zip(raws, self.half, self.p0, self.p1)])
        fn = L.prepareFrameMeansBatch if means else L.prepareFrameFusedBatch
        fn(n, arr, (w + 3) * 12, MAXVAL, w, h, (w + 5) * 4, (w // 2 + 3) * 4, taps, ntaps, None)
        torch.cuda.synchronize()
        self.half_row_bytes = (w + 3) * 12


def _numpy_means(half):
    """half: float32 [h, w, 3] -> the 3 x 3 patch means as the mask kernel forms them"""
    h, w, _ = half.shape
    p = np.pad(half, ((1, 1), (1, 1), (0, 0)), mode="edge")          # the individually clamped coordinates
    m = np.zeros_like(half)                                          # the sum starts from 0.0f
    for y in range(3):
        for x in range(3):                                           # row-major, y outer
            m = m + p[y:y + h, x:x + w]
            assert m.dtype == np.float32
    return m / np.float32(9)                                         # the correctly rounded quotient (div9)


@pytest.mark.parametrize("w,h", SIZES)
def test_prepare_with_means_equals_prepare_and_numpy(w, h):
    from multi_frame_super_resolution_amd import capi
    L = capi.lib()
    for ntaps in (5, 3):
        for n in (1, 2, 3, 4):
            raws = _raw_frames(w, h, n, 100 * w + 10 * n + ntaps)[1:]
            old = _Prepared(L, capi, raws, w, h, ntaps, means=False)
            new = _Prepared(L, capi, raws, w, h, ntaps, means=True)
            for k in range(n):
                what = f"{w}x{h} taps={ntaps} frames={n} frame {k}"
                assert _same_bits(new.p0[k], old.p0[k]), what + ": pyramid level 0"
                assert _same_bits(new.p1[k], old.p1[k]), what + ": pyramid level 1"
                half = old.half[k].cpu().numpy()
                assert np.all(half[:, w:] == np.float32(SENTINEL)), what
                want = half.copy()
                want[:, :w] = _numpy_means(np.ascontiguousarray(half[:, :w]))
                got = new.half[k].cpu().numpy()
                bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
                assert bad.size == 0, f"{what}: {len(bad)} values of the means image differ, first (y, x, c) = {bad[0].tolist()}"
    # no halo, no patch: one tap is refused and nothing is launched
    raws = _raw_frames(w, h, 1, 1)[1:]
    half, p0, p1 = torch.zeros(h, w, 3, device="cuda:0"), torch.zeros(h, w, device="cuda:0"), torch.zeros(max(h // 2, 1), max(w // 2, 1), device="cuda:0")
    arr = (capi.PrepareFrame * 1)(capi.PrepareFrame(raws[0].data_ptr(), half.data_ptr(), p0.data_ptr(), p1.data_ptr()))
    one = (ctypes.c_float * 1)(1.0)
    assert L.raw["mfsr_prepareFrameMeansBatch"](1, arr, w * 12, MAXVAL, w, h, w * 4, max(w // 2, 1) * 4, one, 1, None) == UNSUPPORTED
    torch.cuda.synchronize()


def _planted_flow(w, h, seed):
    """A smooth random flow within +-3 px with planted texels.  Returns (flow float32 [h, w, 2], count of interior pixels that the
    planted displacements alone put outside the image)."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = r.uniform(0, 2 * np.pi, 4)
    f = np.stack([3.0 * np.sin(xx / 9.0 + ph[0]) * np.cos(yy / 6.0 + ph[1]), 3.0 * np.cos(xx / 7.0 + ph[2]) * np.sin(yy / 8.0 + ph[3])],
                 axis=-1).astype(np.float32)
    planted = np.zeros((h, w, 2), dtype=bool)   # components holding an exact even integer 2 d: round(0.5 f) = d whatever the 1-ulp bilinear weights
    tx, ty = [-2, -1, 0, w - 1, w, w + 1], [-2, -1, 0, h - 1, h, h + 1]
    # q = p + round(0.5 * flow): every target column from both edge columns (corners included), every target row from both edge rows
    for px in {1, w - 2}:
        for py in range(1, h - 1):
            f[py, px, 0] = 2.0 * (tx[(py + px) % 6] - px)
            planted[py, px, 0] = True
    for py in {1, h - 2}:
        for px in range(1, w - 1):
            f[py, px, 1] = 2.0 * (ty[(px + py) % 6] - py)
            planted[py, px, 1] = True
    special = np.zeros((h, w), dtype=bool)
    if w >= 16 and h >= 9:
        row = h // 2
        vals = [5.0, -5.0, 3.0, -3.0, 1.0, -1.0, 7.0,                # 2 d + 1: the round-half rule
                0.0, -0.0, np.nan, np.inf, -np.inf]
        for i, v in enumerate(vals):
            x = 3 + 2 * i
            if x < w - 3:
                f[row, x, i % 2] = np.float32(v)
                special[row, x] = not np.isfinite(v)
        if w >= 40:   # the same non-finite values in the other component
            for i, v in enumerate([np.nan, np.inf, -np.inf]):
                f[row, 30 + 2 * i, (i + 1) % 2] = np.float32(v)
                special[row, 30 + 2 * i] = True
    # pixels whose planted displacement leaves the image, judged from the planted numbers alone: the bilinear fetch reads the
    # texel's 3 x 3 neighbourhood at most, so a finite neighbourhood keeps an exact even integer within 1e-2 of itself
    outside = 0
    for py in range(1, h - 1):
        for px in range(1, w - 1):
            if special[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2].any():
                continue
            ox = planted[py, px, 0] and not 0 <= px + int(f[py, px, 0]) // 2 < w
            oy = planted[py, px, 1] and not 0 <= py + int(f[py, px, 1]) // 2 < h
            outside += bool(ox or oy)
    return f, outside


@pytest.mark.parametrize("w,h", SIZES)
def test_group_masks_equal_the_fused_batch(w, h):
    from multi_frame_super_resolution_amd import capi
    L = capi.lib()
    dev = torch.device("cuda:0")
    nonzero = False
    for n in (1, 2, 3, 4):
        raws = _raw_frames(w, h, n, 7 * w + n)
        ref = _Prepared(L, capi, raws[:1], w, h, 5, means=False).half[0]
        plain = _Prepared(L, capi, raws[1:], w, h, 5, means=False)
        means = _Prepared(L, capi, raws[1:], w, h, 5, means=True)
        flows, outside = [], []
        for k in range(n):
            f, cnt = _planted_flow(w, h, 31 * w + 5 * n + k)
            pad = np.full((h, w + 2, 2), SENTINEL, dtype=np.float32)
            pad[:, :w] = f
            flows.append(torch.from_numpy(pad).to(dev))
            outside.append(cnt)
        if (w, h) != (3, 3):
            assert min(outside) > 0, f"{w}x{h}: the planted flows of a frame put no pixel outside the image: {outside}"
        want = [torch.full((h, w + 1, 4), SENTINEL, device=dev) for _ in range(n)]
        got = [torch.full((h, w + 1, 4), SENTINEL, device=dev) for _ in range(n)]
        flow_rb, mask_rb, img_rb = (w + 2) * 8, (w + 1) * 16, plain.half_row_bytes
        old = (capi.RobustnessFrame * n)(*[capi.RobustnessFrame(plain.half[k].data_ptr(), want[k].data_ptr(), flows[k].data_ptr())
                                           for k in range(n)])
        L.robustnessMaskFusedBatch(n, old, ref.data_ptr(), flow_rb, w, h, w, h, img_rb, mask_rb, ALPHA, BETA, THRESHOLD_M, None)
        new = (capi.RobustnessGroupFrame * n)(*[capi.RobustnessGroupFrame(means.half[k].data_ptr(), raws[k + 1].data_ptr(), got[k].data_ptr(),
                                                                           flows[k].data_ptr()) for k in range(n)])
        L.robustnessMaskGroup(n, new, ref.data_ptr(), img_rb, flow_rb, means.half_row_bytes, mask_rb, w, h, MAXVAL, ALPHA, BETA,
                              THRESHOLD_M, None)
        torch.cuda.synchronize()
        for k in range(n):
            a, b = got[k].cpu().numpy(), want[k].cpu().numpy()
            bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
            assert bad.size == 0, (f"{w}x{h} frames={n} frame {k}: {len(bad)} mask values differ, first (y, x, c) = {bad[0].tolist()}: "
                                   f"{a[tuple(bad[0])]!r} for {b[tuple(bad[0])]!r}")
            assert np.all(b[:, w:] == np.float32(SENTINEL))                                   # row padding untouched
            ring = np.ones((h, w), dtype=bool)
            ring[1:-1, 1:-1] = False
            assert np.all(b[:, :w][ring].view(np.uint32) == 0)                                 # the ring is +0.0
            nonzero = nonzero or bool((b[1:-1, 1:w - 1, :3] > 0).any())
    if (w, h) != (3, 3):
        assert nonzero, "every mask of the comparison is zero: the frames do not resemble the reference"


def _burst(cfg, frames, group, window=None):
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    L = capi.lib()
    L.set_robustness_group(group)
    try:
        pipe = BurstPipeline(cfg, torch.device("cuda:0"), window=window)
        img, out16 = pipe.process(frames)
        res = dict(img=img.clone(), out16=out16.clone(), acc=pipe.img_out.clone(), weights=pipe.total_weights.clone(),
                   launches=pipe.robust_group_launches(), paths=pipe.debug_paths())
        torch.cuda.synchronize()
        pipe.close()
        return res
    finally:
        L.set_robustness_group(1)


@pytest.mark.parametrize("erode,window", [(0, None), (1, None), (0, (100, 60, 200, 150))], ids=["plain", "erode1", "window"])
def test_burst_is_bit_identical_with_the_switch_on_and_off(erode, window):
    from multi_frame_super_resolution_amd.pipeline import default_config
    from multi_frame_super_resolution_amd.synth import make_burst
    W, H, N = 256, 192, 7
    frames, _, _ = make_burst(W, H, N, scale=2, mono=False, seed=977, max_shift=3.0)
    frames = [f.to("cuda:0") for f in frames]
    cfg = default_config(W, H, N, 2, False)
    cfg.maskErode = erode
    on, off = _burst(cfg, frames, 1, window), _burst(cfg, frames, 0, window)
    for name in ("acc", "weights", "img", "out16"):
        a, b = on[name], off[name]
        assert a.shape == b.shape and (torch.equal(a, b) if a.dtype != torch.float32 else _same_bits(a, b)), name
    assert float(on["weights"].max()) > 1.0                                     # frames were merged
    # one launch per aligned group that has moved frames: the reference's group (three moved frames) and the group of three
    assert on["paths"]["robust_batch"] == 2 and on["launches"] == 2, (on["launches"], on["paths"])
    assert off["paths"]["robust_batch"] == 2 and off["launches"] == 0, (off["launches"], off["paths"])
