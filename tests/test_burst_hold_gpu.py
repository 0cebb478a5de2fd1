"""The burst hold of the driver (mfsr_burst_hold_fuse, BurstPipeline.hold_fuse): complete groups are aligned as they fill and
their warp+fuse leaves as ONE launch at flush / finish / a full slot ring.  Whole bursts at 256 x 192 through BurstPipeline,
hold on against hold off: accumulators and the u16 image bit for bit, and the launches counted by mfsr_burst_fuse_stats."""
import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
from multi_frame_super_resolution_amd.synth import make_burst

pytestmark = pytest.mark.gpu

W, H = 256, 192
NMAX = 17


@pytest.fixture(scope="module")
def frames(hip):
    fr, _, _ = make_burst(W, H, NMAX, scale=2, mono=False, seed=777, max_shift=3.0)
    return [f.to(hip.dev) for f in fr]


def _burst(hip, frames, n, hold, cfg_frames=None, flush_after=(), setup=None, window=None):
    """One burst of the first n frames -> (imgOut, totalWeights, out16, accumulators at each flush, stats)"""
    cfg = default_config(W, H, n if cfg_frames is None else cfg_frames, 2, False)
    if setup:
        setup(cfg)
    pipe = BurstPipeline(cfg, hip.dev, window=window)
    try:
        pipe.hold_fuse(hold)
        pipe.begin_burst()
        pipe.set_reference(frames[0])
        mid = []
        for k in range(n):
            pipe.add_frame(frames[k], k == 0)
            if k + 1 in flush_after:
                mid.append((pipe.img_out.cpu().numpy().copy(), pipe.total_weights.cpu().numpy().copy()))   # (the accessors flush)
        _, out16 = pipe.finish(want_float=False)
        torch.cuda.synchronize()
        return (pipe._img_out.cpu().numpy(), pipe._total_weights.cpu().numpy(), out16.cpu().numpy().copy(), mid, pipe.fuse_stats())
    finally:
        pipe.close()


def _same(a, b):
    assert np.array_equal(a[0], b[0]), "imgOut"
    assert np.array_equal(a[1], b[1]), "totalWeights"
    assert np.array_equal(a[2], b[2]), "out16"


@pytest.fixture(scope="module")
def plain(hip, frames):
    """the bursts without the hold, once per frame count"""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = _burst(hip, frames, n, False)
            assert cache[n][4] == (0, 0)
        return cache[n]
    return get


@pytest.mark.parametrize("n,launches,groups", [(8, 1, 2), (9, 1, 2), (12, 1, 3), (16, 1, 4), (17, 1, 4)])
def test_hold_equals_group_launches(hip, frames, plain, n, launches, groups):
    """floor(n / 4) groups in one burst launch, the remainder as an ordinary launch.  17 frames: the ring holds 16 slots, so the
    17th frame sends the four held groups off (one burst launch) and follows alone."""
    held = _burst(hip, frames, n, True)
    _same(held, plain(n))
    assert held[4] == (launches, groups)


def test_more_frames_than_the_ring_holds(hip, frames, plain):
    """cfg.frames = 8: a ring of eight slots.  Of 17 frames the first eight leave when the ninth needs a slot, the next eight
    when the seventeenth does: two burst launches of two groups each."""
    held = _burst(hip, frames, 17, True, cfg_frames=8)
    _same(held, plain(17))
    assert held[4] == (2, 4)


def test_flush_in_the_middle_of_a_burst(hip, frames):
    """A flush after 6 and after 10 frames: the accumulators at those points and at the end equal the path without the hold.
    Six frames: one held group and two waiting frames, two ordinary launches.  Ten: the second group alone, then two frames."""
    off = _burst(hip, frames, 16, False, flush_after=(6, 10))
    on = _burst(hip, frames, 16, True, flush_after=(6, 10))
    for (ai, aw), (bi, bw) in zip(on[3], off[3]):
        assert np.array_equal(ai, bi) and np.array_equal(aw, bw)
    _same(on, off)
    assert on[4] == (0, 0)       # never two complete groups between flushes ...
    on = _burst(hip, frames, 16, True, flush_after=(6,))
    _same(on, off)
    assert on[4] == (1, 2)       # ... frames 7 .. 16: groups (7 .. 10) and (11 .. 14) in one launch, then two frames


def test_two_bursts_on_one_context(hip, frames, plain):
    cfg = default_config(W, H, 16, 2, False)
    pipe = BurstPipeline(cfg, hip.dev)
    try:
        pipe.hold_fuse(True)
        for n in (12, 16):
            _, out16 = pipe.process(frames[:n])
            torch.cuda.synchronize()
            assert np.array_equal(out16.cpu().numpy(), plain(n)[2]), n
            assert np.array_equal(pipe.img_out.cpu().numpy(), plain(n)[0]), n
            assert pipe.fuse_stats() == (1, n // 4)
    finally:
        pipe.close()


def test_seven_frames_of_a_sixteen_frame_configuration(hip, frames):
    """Fewer than two complete groups: today's launches."""
    on = _burst(hip, frames, 7, True, cfg_frames=16)
    _same(on, _burst(hip, frames, 7, False, cfg_frames=16))
    assert on[4] == (0, 0)


def test_process_wide_switch(hip, frames, plain):
    hip.L.set_burst_fuse(0)
    try:
        off = _burst(hip, frames, 12, True)
    finally:
        hip.L.set_burst_fuse(1)
    _same(off, plain(12))
    assert off[4] == (0, 0)


def _mixed_burst(hip, dev_frames, host_frames, upload_ring):
    """20 frames on one handle with the hold on and cfg.uploadRing set: frames 0-7 resident, a flush, frames 8-11 resident, frames
    12-19 from the host.  Frames 0-7 are then in the accumulators, frames 8-11 wait in the burst hold, frames 12-15 become the
    host burst's held group and frames 16-19 the filling group.  -> (imgOut, totalWeights, downloaded u16 image, fuse_stats)"""
    cfg = default_config(W, H, 20, 2, False)
    cfg.uploadRing = upload_ring
    pipe = BurstPipeline(cfg, hip.dev)
    try:
        L, h, st = pipe.L, pipe._h, pipe._stream()
        acc = (pipe._img_out.data_ptr(), pipe._total_weights.data_ptr())
        out16_host = torch.empty_like(pipe.out16, device="cpu").pin_memory()
        pipe.hold_fuse(True)
        pipe.begin_burst()
        L.burst_set_reference_host(h, host_frames[0].data_ptr(), st)
        for k in range(8):
            pipe.add_frame(dev_frames[k], k == 0)
        pipe.flush()
        for k in range(8, 12):
            pipe.add_frame(dev_frames[k])
        for k in range(12, 20):
            L.burst_add_frame_host(h, host_frames[k].data_ptr(), 0, *acc, st)
        L.burst_finish_host(h, *acc, pipe.out16.data_ptr(), out16_host.data_ptr(), st)
        pipe.host_sync()
        torch.cuda.synchronize()
        return (pipe._img_out.cpu().numpy(), pipe._total_weights.cpu().numpy(), out16_host.numpy().copy(), pipe.fuse_stats())
    finally:
        pipe.close()


@pytest.fixture(scope="module")
def frames20(hip):
    fr, _, _ = make_burst(W, H, 20, scale=2, mono=False, seed=778, max_shift=3.0)
    return [f.to(hip.dev) for f in fr], [f.cpu().pin_memory() for f in fr]


@pytest.mark.parametrize("upload_ring", [4, 8])
def test_groups_fuse_in_arrival_order_on_a_mixed_handle(hip, frames20, upload_ring):
    """Resident and host frames on one handle with the hold on: a group of the burst hold (frames 8-11) and the host burst's held
    group (12-15) wait at the same time.  The hold's group arrived first, so it is fused first: the accumulators and the
    downloaded image are, bit for bit, those of the same calls under mfsr_set_burst_fuse(0), where every resident group is
    fused the moment it is complete -- arrival order by construction.  (The driver used to fuse the held group before a single
    hold group there: (x + held) + g where arrival order is (x + g) + held.)  The flush sends frames 0-7 off as one burst
    launch of two groups; the third held group leaves alone.
    uploadRing = 4: frame 16 needs the upload slot of frame 12, so both waiting groups leave there, inside
    mfsr_burst_add_frame_host (the old driver kept the order on that path).  uploadRing = 8: both are still waiting when
    mfsr_burst_finish_host is called, which sends the hold's group off and fuses the held and the filling group band by band
    (where the old driver did not)."""
    dev, host = frames20
    on = _mixed_burst(hip, dev, host, upload_ring)
    hip.L.set_burst_fuse(0)
    try:
        off = _mixed_burst(hip, dev, host, upload_ring)
    finally:
        hip.L.set_burst_fuse(1)
    assert off[3] == (0, 0)
    assert on[3] == (1, 2)
    _same(on, off)


def _async(cfg):
    cfg.asyncFuse = 1


@pytest.mark.parametrize("what", ["asyncFuse", "window", "host"])
def test_other_paths_are_not_held(hip, frames, what):
    """cfg.asyncFuse, a zoom window and a host burst keep their launches: zero burst launches with the hold switched on, and
    the results of the same burst with it off."""
    if what == "host":
        cfg = default_config(W, H, 12, 2, False)
        cfg.uploadRing = 4
        host = [f.cpu().pin_memory() for f in frames[:12]]
        outs = []
        for hold in (True, False):
            pipe = BurstPipeline(cfg, hip.dev)
            try:
                pipe.hold_fuse(hold)
                out = pipe.process_host(host)
                pipe.host_sync()
                outs.append(out.numpy().copy())
                assert pipe.fuse_stats() == (0, 0)
            finally:
                pipe.close()
        assert np.array_equal(outs[0], outs[1])
        return
    kw = dict(setup=_async) if what == "asyncFuse" else dict(window=(64, 48, 200, 120))
    on, off = _burst(hip, frames, 12, True, **kw), _burst(hip, frames, 12, False, **kw)
    _same(on, off)
    assert on[4] == (0, 0)
