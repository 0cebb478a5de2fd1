"""The fused reference setup against the launches it replaces, bit for bit (uint32 views, NaNs included):

  * mfsr_kernelParamField against the five-call chain ComputeDerivatives2Kernel -> ComputeStructureTensor ->
    separableFilter(chan = 3) -> ComputeKernelParam -> float3ToFloat4 run on the WHOLE image;
  * mfsr_tileSquaredSumsLevels against mfsr_tileSquaredSums level by level;
  * mfsr_deBayerFusedRing against a zero-filled image followed by mfsr_deBayerFused;
  * whole bursts with mfsr_set_reference_fused(0) and (1).

Every device array sits between the guards of tests/kernels.py::guarded_upload (HipKernels.call checks them and that read-only
inputs are left alone); outputs have padded pitches, and the padding and the rows outside a row window must keep their
sentinel.  The new entry points take their images as mfsr_tex2d descriptors, so the argument-name gate of
tests/test_kernel_edges_cpu.py does not see them: their padded-pitch and launch-edge cases are the ones here.
"""
import ctypes

import numpy as np
import pytest

from multi_frame_super_resolution_amd import capi
from tests.kernels import F3, Host, Tex

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3
UNSUPPORTED = -2
KF_TX, KF_TY, KF_MAXH = 64, 16, 5      # csrc/kernel_field.hip: the tile and the largest ntaps / 2
PARAMS = (0.005, 0.05, 0.3, 2.0, 2.0, 2.0)     # Dth, Dtr, kDetail, kDenoise, kStretch, kShrink (mfsr_config_default's)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sentinel(shape):
    """a float32 array whose every byte is SENTINEL"""
    return np.full(int(np.prod(shape)) * 4, SENTINEL, np.uint8).view(np.float32).reshape(shape)


def gaussian(hip, sigma):
    buf = np.zeros(99, np.float32)
    n = hip.L.raw["mfsr_gaussin_filter_1D"](ctypes.c_float(sigma), buf.ctypes.data)
    return buf[:n].copy()


def tap_sets(hip):
    """1, 3, the pipeline's own (sigmaTensor = 1: 5), the supported maximum (11) and maximum + 2"""
    sets = [np.ones(1, np.float32), gaussian(hip, 0.5), gaussian(hip, 1.0), gaussian(hip, 2.7), gaussian(hip, 3.3)]
    assert [len(t) for t in sets] == [1, 3, 5, 2 * KF_MAXH + 1, 2 * KF_MAXH + 3]
    return sets


def image(w, h, content):
    r = np.random.default_rng(w * 1000 + h)
    if content == "random":
        img = r.random((h, w), dtype=np.float32)
    elif content == "constant":      # tensor == 0 everywhere: norm == 0, lam1 + lam2 == 0, A = 1 + sqrt(0 / 0)
        img = np.zeros((h, w), np.float32)
    elif content == "ramp":          # a pure horizontal ramp
        img = np.broadcast_to(np.arange(w, dtype=np.float32) / np.float32(w), (h, w)).copy()
    else:                            # random, with constant blocks (0 and 0.25) and a ramp block
        img = r.random((h, w), dtype=np.float32)
        img[h // 8:h // 8 + h // 2, w // 16:w // 16 + w // 3] = 0.0
        img[h // 2:, :w // 4] = 0.25
        x0 = w // 2
        img[h // 4:h // 4 + h // 2, x0:x0 + w // 3] = np.arange(w // 3, dtype=np.float32) / np.float32(64)
    img.flags.writeable = False
    return img


def chain(hip, img, taps):
    """the five launches on the whole image, dense"""
    h, w = img.shape
    ix, iy = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    hip.call("ComputeDerivatives2Kernel", w, h, 4 * w, ix, iy, Tex(img))
    ten = np.zeros((h, w, 3), np.float32)
    hip.call("ComputeStructureTensor", ix, iy, ten, w, h, 4 * w, 12 * w)
    tmp, sm = np.zeros_like(ten), np.zeros_like(ten)
    hip.call("separableFilter", ten, 12 * w, tmp, sm, 12 * w, w, h, 3, Host(taps), len(taps))
    hip.call("ComputeKernelParam", sm, w, h, 12 * w, *PARAMS)
    out = np.zeros((h, w, 4), np.float32)
    hip.call("float3ToFloat4", sm, 12 * w, out, 16 * w, w, h)
    return out


def field(hip, img, taps, row0, rows):
    """mfsr_kernelParamField into a sentinel-filled image with a padded pitch -> the whole buffer [h, w + 3, 4]"""
    h, w = img.shape
    buf = sentinel((h, w + 3, 4))
    hip.call("kernelParamField", Tex(img), Tex(buf, w, h, 16 * (w + 3)), row0, rows, Host(taps), len(taps), *PARAMS)
    return buf


def windows(h):
    """whole image, middle, touching row 0, touching the last row, single rows (in the middle, and where the mirrored stencil
    rows all stay near the window: rows h - 4 and h - 3), a band one row longer than a tile"""
    return [(0, h), (h // 3, max(h // 3, 2)), (0, 5), (h - 6, 6), (h // 2, 1), (h - 4, 1), (h - 3, 1), (0, min(h, KF_TY + 1))]


def fallbacks(hip, reset=False):
    """workgroups of mfsr_kernelParamField that left the LDS path since the last reset"""
    n = ctypes.c_int(-1)
    hip.L.kernelParamFieldFallbacks(ctypes.byref(n), 1 if reset else 0)
    return n.value


@pytest.mark.parametrize("content", ["random", "blocks", "constant", "ramp"])
@pytest.mark.parametrize("w,h", [(200, 70), (67, 19), (KF_TX, KF_TY), (KF_TX + 1, 20), (2 * KF_TX + 1, KF_TY + 1)])
def test_kernel_field_equals_the_chain(hip, w, h, content):
    """(widths 64 k + 1 and heights / bands 16 k + 1: with one tap the last tile column / row is one pixel wide)"""
    img = image(w, h, content)
    fallbacks(hip, reset=True)
    for taps in tap_sets(hip):
        if len(taps) // 2 > KF_MAXH:
            with pytest.raises(capi.MfsrError) as e:
                field(hip, img, taps, 0, h)
            assert e.value.code == UNSUPPORTED
            continue
        want = chain(hip, img, taps)
        assert (bits(want[..., 3]) == 0).all()
        if content == "constant":
            assert np.isnan(want[..., :3]).all()          # the 0 / 0 of A reaches every component
        if content == "blocks" and h >= 64 and len(taps) <= 5:   # (the zero block is larger than stencil + smoothing there)
            assert np.isnan(want).any() and np.isfinite(want).any()
        for row0, rows in windows(h):
            got = field(hip, img, taps, row0, rows)
            expect = sentinel(got.shape)
            expect[row0:row0 + rows, :w] = want[row0:row0 + rows]
            assert np.array_equal(bits(got), bits(expect)), \
                f"{w}x{h} {content} taps {len(taps)} rows [{row0}, {row0 + rows}): first at {np.argwhere(bits(got) != bits(expect))[0]}"
    assert fallbacks(hip) == 0        # every workgroup took the staged LDS path


@pytest.mark.parametrize("w,h", [(KF_TX - 1, KF_TY), (KF_TX, KF_TY - 1)])
def test_kernel_field_declines_images_below_one_tile(hip, w, h):
    with pytest.raises(capi.MfsrError) as e:
        field(hip, image(w, h, "random"), gaussian(hip, 1.0), 0, h)
    assert e.value.code == UNSUPPORTED


# ---------------------------------------------------------------- tile sums
def _levels_case(hip, dims, tile, shift):
    """dims: (w, h) per level; tile counts as make_layout takes them (w / T, at least 1)"""
    r = np.random.default_rng(7)
    imgs = [r.standard_normal((h, w)).astype(np.float32) for w, h in dims]
    tcx = [max(w // t, 1) for (w, h), t in zip(dims, tile)]
    tcy = [max(h // t, 1) for (w, h), t in zip(dims, tile)]
    want = []
    for im, t, s, cx, cy in zip(imgs, tile, shift, tcx, tcy):
        o = np.zeros(cx * cy, np.float32)
        hip.call("tileSquaredSums", im, o, im.shape[1], im.shape[0], 4 * im.shape[1], s, t, cx, cy)
        want.append(o)
    # the levels call: device arrays between guards, pointer tables in host memory
    from tests.kernels import guarded_upload
    ups = []
    for im in imgs:
        im.flags.writeable = False
        ups.append(guarded_upload(im))
    outs = [guarded_upload(sentinel((cx * cy,))) for cx, cy in zip(tcx, tcy)]
    n = len(dims)
    texs = (capi.Tex2D * n)(*[capi.Tex2D(t.data_ptr(), 4 * im.shape[1], im.shape[1], im.shape[0]) for (t, _), im in zip(ups, imgs)])
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in outs])
    I = ctypes.c_int * n
    hip.L.tileSquaredSumsLevels(n, texs, ptrs, I(*shift), I(*tile), I(*tcx), I(*tcy), None)
    hip.torch.cuda.synchronize()
    for l in range(n):
        ups[l][1](f"level {l} image", unchanged=True)
        outs[l][1](f"level {l} sums")
        assert np.array_equal(bits(outs[l][0].cpu().numpy()), bits(want[l])), f"level {l}"


def test_tile_sums_of_all_levels_equal_the_per_level_launches(hip):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(256, 160, 3, 2, False)
    tw, th = 128, 80
    dims = [(tw // cfg.levelFactor[l], th // cfg.levelFactor[l]) for l in range(cfg.levels)]
    assert cfg.levels >= 2
    _levels_case(hip, dims, [cfg.tileSize[l] for l in range(cfg.levels)], [cfg.maxShift[l] for l in range(cfg.levels)])
    # two levels with different tile sizes; the first one's only tile is ragged (the image ends inside the tile)
    _levels_case(hip, [(13, 29), (83, 61)], [16, 24], [4, 5])
    _levels_case(hip, [(83, 61)], [8], [3])


# ---------------------------------------------------------------- ring debayer
CFAS = {"RGGB": (0, 1, 1, 2), "BGGR": (2, 1, 1, 0), "GRBG": (1, 0, 2, 1), "GBRG": (1, 2, 0, 1), "MONO": (1, 1, 1, 1)}


@pytest.mark.parametrize("pat", list(CFAS))
@pytest.mark.parametrize("w,h", [(70, 22), (6, 6)])
def test_ring_debayer_equals_clear_then_debayer(hip, pat, w, h):
    hip.set_cfa(CFAS[pat])
    try:
        bp, sc = F3([256, 250, 260]), F3([1 / 3839.0, 1 / 3800.0, 1 / 3850.0])
        raw = np.random.default_rng(5).integers(200, 4096, (h, w), dtype=np.uint16)
        raw.flags.writeable = False
        wins = [(0, h)] + ([(4, 12), (h - 8, 8)] if h > 12 else [])        # row windows start on an even row (the CFA phase)
        for r0, rows in wins:
            sub = np.ascontiguousarray(raw[r0:r0 + rows])
            sub.flags.writeable = False
            want = np.zeros((rows, w, 3), np.float32)
            hip.call("deBayerFused", sub, want, 12 * w, w, rows, bp, sc)
            assert (bits(want[:2]) == 0).all() and (bits(want[:, -2:]) == 0).all()
            got = sentinel((rows, w + 1, 3))
            hip.call("deBayerFusedRing", sub, Tex(got, w, rows, 12 * (w + 1)), bp, sc)
            expect = sentinel(got.shape)
            expect[:, :w] = want
            assert np.array_equal(bits(got), bits(expect)), f"{pat} {w}x{h} rows [{r0}, {r0 + rows})"
    finally:
        hip.set_cfa(CFAS["RGGB"])


# ---------------------------------------------------------------- whole bursts
def _burst(W, H, mono):
    import torch
    from multi_frame_super_resolution_amd.synth import make_burst
    frames, _, _ = make_burst(W, H, 3, scale=2, mono=mono, seed=77, max_shift=2.0)
    return [f.to(torch.device("cuda:0")) for f in frames]


def _run_whole(hip, cfg, frames, fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    hip.L.set_reference_fused(fused)
    try:
        pipe = BurstPipeline(cfg, hip.dev)
        _, out16 = pipe.process(frames)
        res = dict(out16=out16.cpu().numpy().copy(), img=pipe.img_out.cpu().numpy().copy(),
                   tw=pipe.total_weights.cpu().numpy().copy(), paths=pipe.debug_paths())
        pipe.close()
        return res
    finally:
        hip.L.set_reference_fused(1)


@pytest.mark.parametrize("W,H,mono", [(256, 160, False), (128, 96, True)])
def test_burst_is_the_same_with_and_without_the_fused_reference_setup(hip, W, H, mono):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, 3, 2, mono)
    frames = _burst(W, H, mono)
    fallbacks(hip, reset=True)
    a, b = _run_whole(hip, cfg, frames, 0), _run_whole(hip, cfg, frames, 1)
    assert fallbacks(hip) == 0
    assert a["paths"]["ref_field_fused"] == 0 and b["paths"]["ref_field_fused"] == 1
    assert {k: v for k, v in a["paths"].items() if k != "ref_field_fused"} == \
           {k: v for k, v in b["paths"].items() if k != "ref_field_fused"}
    assert np.array_equal(a["out16"], b["out16"])
    assert np.array_equal(bits(a["img"]), bits(b["img"])) and np.array_equal(bits(a["tw"]), bits(b["tw"]))
    assert a["out16"].any()


def test_row_stripe_reference_is_the_same_with_and_without_the_fused_setup(hip):
    """The calls of one rank of a two-rank burst (mfsr_burst_set_reference_rows, fuse and finish of its stripe), for either
    rank: the stripe's rows of out16 and of both accumulators."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    W, H = 256, 160
    cfg = default_config(W, H, 3, 2, False)
    frames = _burst(W, H, False)
    torch = hip.torch
    pipe = BurstPipeline(cfg, hip.dev)
    st = torch.cuda.current_stream().cuda_stream
    flows, masks = zip(*[pipe.new_frame_products() for _ in frames])
    pipe.set_reference(frames[cfg.reference])
    for k, f in enumerate(frames):
        pipe.align_frame(f, k == cfg.reference, flows[k], masks[k])
    torch.cuda.synchronize()
    try:
        for rank in (0, 1):
            plan = pipe.stripe_plan(2, rank, 64)
            res = []
            for fused in (0, 1):
                hip.L.set_reference_fused(fused)
                pipe.L.burst_begin(pipe._h, pipe._img_out.data_ptr(), pipe._total_weights.data_ptr(), st)
                pipe.L.burst_set_reference_rows(pipe._h, frames[cfg.reference].data_ptr(), plan.rowBegin, plan.rowEnd, st)
                assert pipe.debug_paths()["ref_field_fused"] == fused
                pipe.fuse_rows(frames, flows, masks, plan.rowBegin, plan.rowEnd, True)
                out16 = pipe.finish_rows(plan.rowBegin, plan.rowEnd - plan.rowBegin)
                torch.cuda.synchronize()
                rows = slice(plan.rowBegin, plan.rowEnd)
                res.append((out16[rows].cpu().numpy().copy(), pipe._img_out[rows].cpu().numpy().copy(),
                            pipe._total_weights[rows].cpu().numpy().copy()))
            assert plan.rowEnd - plan.rowBegin == H and res[0][0].any()
            assert np.array_equal(res[0][0], res[1][0]), f"out16, rank {rank}"
            assert np.array_equal(bits(res[0][1]), bits(res[1][1])), f"imgOut, rank {rank}"
            assert np.array_equal(bits(res[0][2]), bits(res[1][2])), f"totalWeights, rank {rank}"
    finally:
        hip.L.set_reference_fused(1)
        pipe.close()
