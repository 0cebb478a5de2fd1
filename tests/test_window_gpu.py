"""Zoom windows on the GPU: a windowed burst's u16 image, float image and flushed accumulators are bit for bit the
rectangle cut from the whole-frame burst of the same frames (which the other GPU tests check against the oracle)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

W, H, N = 260, 196, 4  # HR grids that are not multiples of 16 at x2 / x3 / x1: windows may end at a ragged edge
GBRG = (1, 2, 0, 1)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _equal(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cfg(scale, kind, pair=1, async_fuse=0, frames=N, width=W, height=H):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(width, height, frames, scale, kind == "mono")
    if kind == "gbrg":
        for i, c in enumerate(GBRG):
            cfg.cfa[i] = c
    cfg.pairFrames = pair
    cfg.asyncFuse = async_fuse
    return cfg


def _frames(scale, kind, n=N, seed=11, width=W, height=H, device="cuda:0"):
    from multi_frame_super_resolution_amd.synth import make_burst
    fr, _, _ = make_burst(width, height, n, scale=scale, mono=kind == "mono", seed=seed, max_shift=3.0, device=device)
    return [f.to("cuda:0") for f in fr]


def _burst(cfg, frames, window=None, setup=None):
    """(float image, u16 image, accumulators, weights) of one burst, copied to the host."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    pipe = BurstPipeline(cfg, window=window)
    if setup is not None:
        setup(pipe)
    out, out16 = pipe.process(frames)
    res = (out.clone().cpu(), out16.clone().cpu(), pipe.img_out.clone().cpu(), pipe.total_weights.clone().cpu())
    pipe.close()
    return res


def _windows(hr_w, hr_h):
    bx, by = (hr_w - 40) // 16 * 16, (hr_h - 40) // 16 * 16
    return {
        "interior": (64, 48, 96, 64),
        "top_left": (0, 0, 48, 32),
        "bottom_right_edge": (bx, by, hr_w - bx, hr_h - by),
        "whole_explicit": (0, 0, hr_w, hr_h),
        "16x16": (128, 96, 16, 16),
        "tile_column_and_margin": (240, 0, min(32, hr_w - 240), 32),  # x2: crosses the 256-px tile edge, rows in the top band
    }


def _assert_crop(whole, got, win, what):
    x, y, w, h = win
    names = ("float image", "u16 image", "accumulators", "weights")
    for i, name in enumerate(names):
        assert _equal(whole[i][y:y + h, x:x + w], got[i]), f"{what}: {name} differs from the whole-frame crop"


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("async_fuse", [0, 1])
@pytest.mark.parametrize("scale,kind", [(2, "rggb"), (2, "gbrg"), (2, "mono"), (4, "rggb"), (3, "rggb"), (1, "rggb")])
def test_window_equals_whole_frame_crop(scale, kind, pair, async_fuse):
    cfg = _cfg(scale, kind, pair, async_fuse)
    frames = _frames(scale, kind)
    whole = _burst(cfg, frames)
    hr_w, hr_h = W * scale, H * scale
    for name, win in _windows(hr_w, hr_h).items():
        _assert_crop(whole, _burst(cfg, frames, win), win, name)
    # the whole frame through the C-ABI's 0, 0, 0, 0
    got = _burst(cfg, frames, setup=lambda p: p.L.burst_set_window(p._h, 0, 0, 0, 0))
    _assert_crop(whole, got, (0, 0, hr_w, hr_h), "0,0,0,0")


def test_python_window_returns_exactly_the_rectangle():
    """BurstPipeline(window=...) takes any rectangle: the library works on the aligned window around it, the result is the
    rectangle asked for."""
    cfg = _cfg(2, "rggb")
    frames = _frames(2, "rggb")
    whole = _burst(cfg, frames)
    for x, y, w, h in [(37, 21, 101, 55), (500, 370, 100, 100)]:
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        pipe = BurstPipeline(cfg, window=(x, y, w, h))
        out, out16 = pipe.process(frames)
        x1, y1 = min(x + w, 2 * W), min(y + h, 2 * H)
        assert _equal(out.cpu(), whole[0][y:y1, x:x1])
        assert _equal(out16.cpu(), whole[1][y:y1, x:x1])
        pipe.close()


def test_window_host_bursts_source_and_joint():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    cfg = _cfg(2, "rggb")
    cfg.uploadRing = 3
    frames = _frames(2, "rggb")
    host = [f.cpu().pin_memory() for f in frames]
    win = (240, 96, 160, 112)
    x, y, w, h = win

    # uploadRing + prefetch_host + finish_host, twice back to back (the second burst overlaps the first one's download)
    ref = BurstPipeline(cfg)
    want = ref.process_host(host)
    ref.host_sync()
    want = want.clone()
    pw = BurstPipeline(cfg, window=win)
    for _ in range(2):
        got = pw.process_host(host)
        pw.host_sync()
        assert _equal(got, want[y:y + h, x:x + w]), "process_host"

    # process_source (frame-source callback) and process_joint
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    NEXT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
    RESET = ctypes.CFUNCTYPE(None, ctypes.c_void_p)

    class Source(ctypes.Structure):
        _fields_ = [("next_frame", NEXT), ("reset", RESET), ("user", ctypes.c_void_p)]

    state = {"i": 0}

    def next_frame(user, dst, stream):
        if state["i"] >= len(frames):
            return 0
        f = frames[state["i"]]
        state["i"] += 1
        return 1 if hip.hipMemcpyAsync(dst, f.data_ptr(), W * H * 2, 3, stream) == 0 else -1

    def reset(user):
        state["i"] = 0

    src = Source(NEXT(next_frame), RESET(reset), None)
    used = ctypes.c_int(0)
    st = torch.cuda.current_stream().cuda_stream
    for p in (ref, pw):
        p.L.burst_process_source(p._h, ctypes.byref(src), p._img_out.data_ptr(), p._total_weights.data_ptr(), p.out_img.data_ptr(),
                                 p.out16.data_ptr(), ctypes.byref(used), st)
    torch.cuda.synchronize()
    assert _equal(pw.out16.cpu(), ref.out16.cpu()[y:y + h, x:x + w]), "process_source"
    assert _equal(pw.out_img.cpu(), ref.out_img.cpu()[y:y + h, x:x + w]), "process_source"

    jo, j16 = (t.clone().cpu() for t in ref.process_joint(frames))
    wo, w16 = (t.clone().cpu() for t in pw.process_joint(frames))
    assert _equal(w16, j16[y:y + h, x:x + w]) and _equal(wo, jo[y:y + h, x:x + w]), "process_joint"
    ref.close()
    pw.close()


def test_window_frame_stream():
    from multi_frame_super_resolution_amd.pipeline import FrameStream
    cfg = _cfg(2, "rggb")
    frames = _frames(2, "rggb", n=5, seed=5)
    win = (128, 64, 176, 96)
    x, y, w, h = win
    full, part = FrameStream(cfg, radius=1), FrameStream(cfg, radius=1, window=win)

    def run(s):
        outs = {}
        for f in frames:
            r = s.push(f)
            if r is not None:
                outs[r[0]] = r[1].clone().cpu()
        for t, img in s.drain():
            outs[t] = img.clone().cpu()
        return outs

    a, b = run(full), run(part)
    assert sorted(a) == sorted(b) == list(range(len(frames)))
    for t in a:
        assert _equal(b[t], a[t][y:y + h, x:x + w]), t
    full.close()
    part.close()


@pytest.mark.parametrize("nframes", [1, 2, 3, 4])
def test_kernel_window_against_cropped_full(nframes):
    """mfsr_accumulateSuperResFullWindow against the crop of mfsr_accumulateSuperResFullN on the same products; the window
    buffer has a pitch above 12 w and guard rows, filled with a canary: no byte outside the window changes."""
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    cfg = _cfg(2, "rggb", pair=1)
    frames = _frames(2, "rggb")
    pipe = BurstPipeline(cfg)
    pipe.process(frames)  # the frames' flows and masks stay in the burst's ring
    kp = pipe.debug_views()[2]
    views = [pipe.frame_views(N - 1 - k) for k in range(N)]  # (flow, mask) of frame k
    L = capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    hr_w, hr_h = 2 * W, 2 * H
    P = ctypes.c_void_p * nframes
    raws = P(*[f.data_ptr() for f in frames[:nframes]])
    masks = P(*[views[k][1].ptr for k in range(nframes)])
    flows = (capi.Tex2D * nframes)(*[views[k][0] for k in range(nframes)])
    mpitch = views[0][1].pitch
    white, black = capi.f3(cfg.white), capi.f3(cfg.black)
    for undefined in (0, 1):
        acc = torch.zeros(hr_h, hr_w, 3, dtype=torch.float32, device="cuda:0")
        wts = torch.zeros_like(acc)
        L.accumulateSuperResFullN(nframes, raws, acc.data_ptr(), wts.data_ptr(), masks, kp, flows, white, black, W, H, 2, 12 * hr_w,
                                  mpitch, 0, st)
        for x, y, w, h in [(240, 0, 32, 48), (64, 48, 96, 64), (496, 368, 24, 24), (0, 0, hr_w, hr_h)]:
            guard, padf = 3, 20  # rows before / after, extra floats per row (pitch 12 w + 80 bytes)
            pitchf = 3 * w + padf
            canary = torch.full(((h + 2 * guard) * pitchf,), 0x7FC0BEEF, dtype=torch.int32, device="cuda:0")
            buf = [canary.clone(), canary.clone()]
            if not undefined:
                for bb in buf:
                    bb.view(h + 2 * guard, pitchf)[guard:guard + h, :3 * w] = 0
            before = [bb.clone() for bb in buf]
            ptr = [bb.data_ptr() + guard * pitchf * 4 for bb in buf]
            L.accumulateSuperResFullWindow(nframes, raws, ptr[0], ptr[1], masks, kp, flows, white, black, W, H, 2, pitchf * 4, mpitch,
                                           undefined, x, y, w, h, st)
            torch.cuda.synchronize()
            for bb, b0, full in zip(buf, before, (acc, wts)):
                g = bb.view(h + 2 * guard, pitchf)
                inside = g[guard:guard + h, :3 * w]
                assert torch.equal(inside, full[y:y + h, x:x + w].reshape(h, 3 * w).view(torch.int32)), (x, y, w, h, undefined)
                mask = torch.ones_like(g, dtype=torch.bool)
                mask[guard:guard + h, :3 * w] = False
                assert torch.equal(g[mask], b0.view(h + 2 * guard, pitchf)[mask]), ("bytes outside the window changed", x, y, w, h, undefined)
    # refusals: a misaligned window, one outside the frame, a pitch below 12 w
    raw = L.raw["mfsr_accumulateSuperResFullWindow"]
    dummy = torch.zeros(64, 64, 3, device="cuda:0")
    for x, y, w, h, pitch in [(8, 0, 16, 16, 12 * 16), (512, 0, 16, 16, 12 * 16), (0, 0, 32, 16, 12 * 16)]:
        assert raw(nframes, raws, dummy.data_ptr(), dummy.data_ptr(), masks, kp, flows, white, black, W, H, 2, pitch, mpitch, 1,
                   x, y, w, h, st) == -1
    pipe.close()


def test_window_refusals_and_switching_back():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    cfg = _cfg(2, "rggb", pair=1)
    frames = _frames(2, "rggb")
    pipe = BurstPipeline(cfg)
    sw = pipe.L.raw["mfsr_burst_set_window"]
    assert sw(pipe._h, 8, 0, 32, 32) == -1
    assert sw(pipe._h, 0, 0, 16, 400) == -1
    assert sw(pipe._h, 496, 0, 32, 16) == -1
    # a frame waiting for its group
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    pipe.add_frame(frames[0], True)
    assert sw(pipe._h, 16, 16, 32, 32) == -1
    pipe.finish()
    # the unfused chain has no window kernels
    cfg0 = _cfg(2, "rggb")
    cfg0.fused = 0
    p0 = BurstPipeline(cfg0)
    assert p0.L.raw["mfsr_burst_set_window"](p0._h, 16, 16, 32, 32) == -2
    assert p0.L.raw["mfsr_burst_set_window"](p0._h, 0, 0, 0, 0) == 0
    p0.close()
    # window, then back to the whole frame on the same burst: the bits of a fresh burst
    fresh = _burst(cfg, frames)
    assert sw(pipe._h, 64, 48, 96, 64) == 0
    v = [ctypes.c_int() for _ in range(4)]
    pipe.L.burst_get_window(pipe._h, *[ctypes.byref(i) for i in v])
    assert [i.value for i in v] == [64, 48, 96, 64]
    pipe.process(frames)  # (window-sized data in the first bytes of the whole-frame buffers)
    assert sw(pipe._h, 0, 0, 0, 0) == 0
    out, out16 = pipe.process(frames)
    assert _equal(out16.cpu(), fresh[1]) and _equal(out.cpu(), fresh[0])
    assert _equal(pipe.img_out.cpu(), fresh[2]) and _equal(pipe.total_weights.cpu(), fresh[3])
    pipe.close()


def test_window_4k_x4_central_quarter():
    """At the size the feature is for: 4K x4 RGGB, four frames, the central quarter of the area."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    w4, h4 = 3840, 2160
    cfg = _cfg(4, "rggb", frames=4, width=w4, height=h4)
    frames = _frames(4, "rggb", n=4, seed=3, width=w4, height=h4, device="cuda:0")
    hr_w, hr_h = 4 * w4, 4 * h4
    win = (hr_w // 4 // 16 * 16, hr_h // 4 // 16 * 16, hr_w // 2, hr_h // 2)
    x, y, w, h = win
    pipe = BurstPipeline(cfg, window=win)
    out, out16 = pipe.process(frames)
    got16, got = out16.clone(), out.clone()
    pipe.close()
    del pipe
    full = BurstPipeline(cfg)
    fo, f16 = full.process(frames)
    assert torch.equal(f16[y:y + h, x:x + w], got16)
    assert torch.equal(fo[y:y + h, x:x + w].contiguous().view(torch.int32), got.view(torch.int32))
    full.close()
