"""Packed 10 / 12-bit raw frames on the device: k_unpackRaw against the numpy restatement of
tests/packed_ref.py for equality, and packed host bursts (cfg.rawPacking) against the resident burst of the same samples, bit
for bit.  Nothing here has a tolerance."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi, synth
from tests import packed_ref as R

pytestmark = pytest.mark.gpu

CANARY = 0xA5


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
def _samples(kind, n, h, w, bits, rng):
    if kind == "counter":       # every sample of a lane, and of a group, distinct
        return (np.arange(n * h * w).reshape(n, h, w) % (1 << bits)).astype(np.uint16)
    if kind == "ones":
        return np.full((n, h, w), (1 << bits) - 1, np.uint16)
    return rng.integers(0, 1 << bits, (n, h, w)).astype(np.uint16)


@pytest.mark.parametrize("packing", R.ALL)
def test_unpack_kernel_equals_the_restatement(packing):
    """Widths: one group, an odd dense row size (12 samples are 15 / 18 bytes), one group either side of a full wave of
    16-sample lanes (1024), more than one workgroup per row... of lanes (2052 x 5 rows).  Source rows dense and padded by 1, 3,
    16 bytes of 0xFF; source bases at byte offsets 0, 1, 2 (only offset 0 with a stride that is a multiple of 4 takes the dword
    path); destination pitch dense and + 32 bytes.  Heights, frame counts and the sample data cycle through all their 27
    combinations under that grid.  The whole destination allocation is compared: the gaps between rows and frames and the
    guards around them keep their canary bytes."""
    from multi_frame_super_resolution_amd.pipeline import unpack_raw
    dev = torch.device("cuda:0")
    bits = R.BITS[packing]
    rng = np.random.default_rng(7 + packing)
    rest = list(itertools.product((1, 2, 5), (1, 3, 64), ("counter", "ones", "random")))
    grid = itertools.product((4, 8, 12, 1020, 1024, 1028, 2052), (0, 1, 3, 16), (0, 1, 2), (0, 32))
    for i, (w, pad, off, gap) in enumerate(grid):
        h, n, kind = rest[(7 * i) % len(rest)]     # 7 and 27 are coprime: every combination comes up
        dense = R.dense_row_bytes(packing, w)
        rb, pitch = dense + pad, 2 * w + gap
        want = _samples(kind, n, h, w, bits, rng)
        # sources: frame k at 64 * ceil + off inside one buffer of 0xFF
        span = (rb * h + off + 63) // 64 * 64 + 64
        src = np.full(n * span, 0xFF, np.uint8)
        for k in range(n):
            a = k * span + off
            src[a:a + rb * h] = R.pack_ref(want[k], packing, rb, fill=0xFF).reshape(-1)
        # destinations: frame k at a multiple of 64 inside one buffer of canaries, 64 bytes of guard before and after each
        dspan = (pitch * h + 63) // 64 * 64 + 64
        expect = np.full(64 + n * dspan, CANARY, np.uint8)
        for k in range(n):
            rows = expect[64 + k * dspan:64 + k * dspan + pitch * h].reshape(h, pitch)
            rows[:, :2 * w] = want[k].view(np.uint8).reshape(h, 2 * w)
        dsrc = torch.from_numpy(src).to(dev)
        ddst = torch.full((expect.size,), CANARY, dtype=torch.uint8, device=dev)
        ins = [dsrc[k * span + off:k * span + off + rb * h].view(h, rb) for k in range(n)]
        outs = [ddst[64 + k * dspan:64 + k * dspan + pitch * h].view(torch.int16).view(h, pitch // 2)[:, :w] for k in range(n)]
        unpack_raw(ins, packing, w, out=outs)
        got = ddst.cpu().numpy()
        assert np.array_equal(got, expect), (packing, w, pad, off, gap, h, n, kind)
        assert torch.equal(dsrc.cpu(), torch.from_numpy(src))
    # the default output, one tensor in and out
    one = unpack_raw(torch.from_numpy(R.pack_ref(want[0], packing)).to(dev), packing, w)
    assert one.dtype == torch.uint16 and np.array_equal(one.cpu().view(torch.int16).numpy().view(np.uint16), want[0])


@pytest.mark.parametrize("packing", R.ALL)
def test_unpack_kernel_dword_path_with_a_cut_last_lane(packing):
    """The dword path needs a source stride that is a multiple of 4 and a destination pitch that is a multiple of 16; with the
    widths above only 1024 (whole lanes) meets both for the 10-bit packings.  Widths 24 and 1032 leave the last lane of a row 8
    samples: that lane goes group by group inside the dword kernel.  The rows are padded to the next multiple of 4 bytes (10
    bits: 30 -> 32, 1290 -> 1292; 12 bits are dense), every kind of sample data on each width, and 1024 with random data."""
    from multi_frame_super_resolution_amd.pipeline import unpack_raw
    dev = torch.device("cuda:0")
    bits = R.BITS[packing]
    rng = np.random.default_rng(70 + packing)
    for w, kind, gap in itertools.product((24, 1032, 1024), ("counter", "ones", "random"), (0, 32)):
        h, n = 3, 2
        dense = R.dense_row_bytes(packing, w)
        rb, pitch = dense + (-dense) % 4, 2 * w + gap
        assert rb % 4 == 0 and pitch % 16 == 0
        want = _samples(kind, n, h, w, bits, rng)
        span = (rb * h + 63) // 64 * 64 + 64
        src = np.full(n * span, 0xFF, np.uint8)
        for k in range(n):
            src[k * span:k * span + rb * h] = R.pack_ref(want[k], packing, rb, fill=0xFF).reshape(-1)
        dspan = (pitch * h + 63) // 64 * 64 + 64
        expect = np.full(64 + n * dspan, CANARY, np.uint8)
        for k in range(n):
            rows = expect[64 + k * dspan:64 + k * dspan + pitch * h].reshape(h, pitch)
            rows[:, :2 * w] = want[k].view(np.uint8).reshape(h, 2 * w)
        dsrc = torch.from_numpy(src).to(dev)
        ddst = torch.full((expect.size,), CANARY, dtype=torch.uint8, device=dev)
        assert dsrc.data_ptr() % 4 == 0 and ddst.data_ptr() % 16 == 0
        ins = [dsrc[k * span:k * span + rb * h].view(h, rb) for k in range(n)]
        outs = [ddst[64 + k * dspan:64 + k * dspan + pitch * h].view(torch.int16).view(h, pitch // 2)[:, :w] for k in range(n)]
        unpack_raw(ins, packing, w, out=outs)
        assert np.array_equal(ddst.cpu().numpy(), expect), (packing, w, kind, gap)


# ---- packed host bursts -------------------------------------------------------------------------------------------------------
W, H, N = 384, 256, 7
_cache = {}


def _burst(bits):
    """the burst of the existing host-burst tests, its samples shifted right to fit 10 bits for the 10-bit packings"""
    if ("frames", bits) not in _cache:
        frames, _, _ = synth.make_burst(W, H, N, seed=29, device="cpu")
        if bits == 10:
            frames = [(f.view(torch.int16).to(torch.int32) >> 2).to(torch.int16).view(f.dtype) for f in frames]
        _cache["frames", bits] = [f.contiguous() for f in frames]
    return _cache["frames", bits]


def _config(bits, ref=0, pair=1, async_fuse=0, ring=0, packing=0):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, N, scale=2)
    if bits == 10:                       # the levels describe the samples' range, as for any other sensor
        for i in range(3):
            cfg.black[i], cfg.white[i] = 64.0, 1023.0 - 64.0
        cfg.maxVal = 1023.0
    cfg.reference, cfg.pairFrames, cfg.asyncFuse, cfg.uploadRing, cfg.rawPacking = ref, pair, async_fuse, ring, packing
    return cfg


def _resident(bits, ref, pair=1, async_fuse=0):
    """the resident burst of the same samples under the same config (the group size decides how the frames' contributions are
    summed, so it belongs to the config that is compared): computed once per config, shared and left unchanged"""
    key = ("want", bits, ref, pair, async_fuse)
    if key not in _cache:
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        dev = torch.device("cuda:0")
        plain = BurstPipeline(_config(bits, ref, pair, async_fuse), dev)
        _, want = plain.process([f.to(dev) for f in _burst(bits)])
        _cache[key] = want.cpu().clone()
        plain.close()
    return _cache[key]


def _pinned_packed(bits, packing, row_bytes=None):
    return [p.pin_memory() for p in synth.pack_raw(_burst(bits), packing, row_bytes=row_bytes)]


def _three_bursts(cfg, host, want, what):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    pipe = BurstPipeline(cfg, torch.device("cuda:0"))
    for rep in range(3):                 # slot re-use, the reference double buffer, staging buffers refilled
        got = pipe.process_host(host)
        pipe.host_sync()
        assert torch.equal(got, want), (what, rep)
        got.zero_()
    pipe.close()


@pytest.mark.parametrize("packing", [capi.PACK_MIPI10, capi.PACK_BE12])
@pytest.mark.parametrize("ring,ref,async_fuse,pair", list(itertools.product((4, 16), (0, 3), (0, 1), (0, 1))))
def test_packed_host_burst_equals_resident_burst(packing, ring, ref, async_fuse, pair):
    bits = R.BITS[packing]
    host = _pinned_packed(bits, packing)
    assert np.array_equal(R.unpack_ref(host[1].numpy(), packing, W), _burst(bits)[1].view(torch.int16).numpy().view(np.uint16))
    _three_bursts(_config(bits, ref, pair, async_fuse, ring, packing), host, _resident(bits, ref, pair, async_fuse),
                  (packing, ring, ref, async_fuse, pair))


@pytest.mark.parametrize("packing", [capi.PACK_MIPI12, capi.PACK_BE10])
def test_the_other_packings_once(packing):
    bits = R.BITS[packing]
    _three_bursts(_config(bits, 3, 1, 1, 4, packing), _pinned_packed(bits, packing), _resident(bits, 3, 1, 1), packing)


def test_packed_host_burst_with_padded_lines():
    """CSI-2 lines padded to 512 bytes (480 are samples); the padding is 0xFF and must not reach a sample"""
    packing, bits = capi.PACK_MIPI10, 10
    host = _pinned_packed(bits, packing, row_bytes=512)
    for p in host:
        p[:, 480:] = 0xFF
    _three_bursts(_config(bits, 3, 1, 0, 4, packing), host, _resident(bits, 3), "padded MIPI10")
    # a stride that is no multiple of 4: the byte path inside the library is not needed (the staging rows are dense), the
    # 2-D copy takes any pitch
    host = _pinned_packed(12, capi.PACK_BE12, row_bytes=576 + 3)
    _three_bursts(_config(12, 0, 1, 0, 4, capi.PACK_BE12), host, _resident(12, 0), "padded BE12")


def test_unpacked_host_burst_with_padded_rows():
    """mfsr_burst_set_host_row_bytes without a packing: uint16_t rows W + 24 samples apart"""
    frames = _burst(12)
    host = []
    for f in frames:
        buf = torch.full((H, W + 24), -1, dtype=torch.int16).pin_memory()
        buf[:, :W] = f.view(torch.int16)
        host.append(buf[:, :W])
    _three_bursts(_config(12, 3, 1, 0, 4, 0), host, _resident(12, 3), "padded uint16 rows")


def test_host_row_bytes_refusals_and_dense_again():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    dev = torch.device("cuda:0")
    set_rows = capi.lib().raw["mfsr_burst_set_host_row_bytes"]
    packing = capi.PACK_MIPI10
    pipe = BurstPipeline(_config(10, 0, 1, 0, 4, packing), dev)
    assert set_rows(pipe._h, 479) == -1 and set_rows(pipe._h, -1) == -1          # below the dense row (480)
    assert set_rows(pipe._h, 481) == 0 and set_rows(pipe._h, 0) == 0 and set_rows(pipe._h, 480) == 0
    # frames pending: a group waits for its rest
    host = _pinned_packed(10, packing)
    st = torch.cuda.current_stream().cuda_stream
    pipe.begin_burst()
    pipe.L.burst_set_reference_host(pipe._h, host[0].data_ptr(), st)
    pipe.L.burst_add_frame_host(pipe._h, host[0].data_ptr(), 1, pipe._img_out.data_ptr(), pipe._total_weights.data_ptr(), st)
    assert set_rows(pipe._h, 512) == -1
    pipe.flush()
    assert set_rows(pipe._h, 512) == 0 and set_rows(pipe._h, 0) == 0
    # a padded burst and a dense one on the same pipeline
    padded = _pinned_packed(10, packing, row_bytes=496)
    for frames in (padded, host, padded):
        got = pipe.process_host(frames)
        pipe.host_sync()
        assert torch.equal(got, _resident(10, 0))
    with pytest.raises(ValueError):
        pipe.process_host([f.view(torch.int16) for f in host])                    # unpacked frames on a packed pipeline
    pipe.close()
    plain = BurstPipeline(_config(12, 0, 1, 0, 4, 0), dev)
    assert set_rows(plain._h, 2 * W - 2) == -1 and set_rows(plain._h, 2 * W + 1) == -1 and set_rows(plain._h, 2 * W + 2) == 0
    plain.close()
    none = BurstPipeline(_config(12), dev)
    assert set_rows(none._h, 0) == -1                                             # no upload ring
    none.close()


def test_packed_host_burst_with_a_zoom_window_is_the_crop():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    packing, bits = capi.PACK_BE12, 12
    host = _pinned_packed(bits, packing)
    win = (240, 96, 160, 112)
    x, y, w, h = win
    pw = BurstPipeline(_config(bits, 0, 1, 0, 4, packing), torch.device("cuda:0"), window=win)
    for _ in range(2):
        got = pw.process_host(host)
        pw.host_sync()
        assert torch.equal(got, _resident(bits, 0)[y:y + h, x:x + w])
    pw.close()


def test_row_bytes_between_bursts_that_left_announced_frames_unconsumed():
    """A burst that announces its frames (prefetch_host) and consumes only some of them leaves uploads that are never unpacked;
    they are not frames pending: the stride can be set for the next burst, and that burst is right."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, _ptr_table
    packing = capi.PACK_MIPI10
    pipe = BurstPipeline(_config(10, 0, 1, 0, 4, packing), torch.device("cuda:0"))
    set_rows = capi.lib().raw["mfsr_burst_set_host_row_bytes"]
    host = _pinned_packed(10, packing)
    out_host = torch.empty_like(pipe.out16, device="cpu").pin_memory()
    st = torch.cuda.current_stream().cuda_stream
    acc = (pipe._img_out.data_ptr(), pipe._total_weights.data_ptr())
    pipe.begin_burst()
    pipe.L.burst_set_reference_host(pipe._h, host[0].data_ptr(), st)
    pipe.L.burst_prefetch_host(pipe._h, _ptr_table(host), len(host), st)
    for k in range(2):                           # the reference and one of the four announced frames
        pipe.L.burst_add_frame_host(pipe._h, host[k].data_ptr(), 1 if k == 0 else 0, *acc, st)
    assert set_rows(pipe._h, 496) == -1          # frames are pending here
    pipe.L.burst_finish_host(pipe._h, *acc, pipe.out16.data_ptr(), out_host.data_ptr(), st)
    pipe.host_sync()
    assert set_rows(pipe._h, 496) == 0 and set_rows(pipe._h, 0) == 0
    for frames in (_pinned_packed(10, packing, row_bytes=496), host):
        got = pipe.process_host(frames)
        pipe.host_sync()
        assert torch.equal(got, _resident(10, 0))
    pipe.close()


def test_process_source_refuses_a_packed_burst():
    """the frame source fills the uint16_t slots itself: a packed burst is refused before the source is asked for anything"""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    pipe = BurstPipeline(_config(10, 0, 1, 0, 4, capi.PACK_MIPI10), torch.device("cuda:0"))
    NEXT = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
    RESET = ctypes.CFUNCTYPE(None, ctypes.c_void_p)

    class Source(ctypes.Structure):
        _fields_ = [("next_frame", NEXT), ("reset", RESET), ("user", ctypes.c_void_p)]

    calls = []
    src = Source(NEXT(lambda user, dst, stream: calls.append("next") or 0), RESET(lambda user: calls.append("reset")), None)
    used = ctypes.c_int(0)
    rc = capi.lib().raw["mfsr_burst_process_source"](pipe._h, ctypes.byref(src), pipe._img_out.data_ptr(), pipe._total_weights.data_ptr(),
                                                     None, pipe.out16.data_ptr(), ctypes.byref(used),
                                                     torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and not calls
    pipe.close()


_UPLOAD_1D_CHILD = """
import torch
from multi_frame_super_resolution_amd import capi
from tests import test_packed_gpu as T
from multi_frame_super_resolution_amd.pipeline import BurstPipeline
dev = torch.device("cuda:0")
set_rows = capi.lib().raw["mfsr_burst_set_host_row_bytes"]
pipe = BurstPipeline(T._config(10, 0, 1, 0, 4, capi.PACK_MIPI10), dev)
assert set_rows(pipe._h, 512) == -1 and set_rows(pipe._h, 481) == -1       # a non-dense stride with 1-D uploads
assert set_rows(pipe._h, 480) == 0 and set_rows(pipe._h, 0) == 0           # the dense one, either way of saying it
got = pipe.process_host(T._pinned_packed(10, capi.PACK_MIPI10))
pipe.host_sync()
assert torch.equal(got, T._resident(10, 0))                                # a dense packed burst through 1-D uploads
pipe.close()
plain = BurstPipeline(T._config(12, 0, 1, 0, 4, 0), dev)
assert set_rows(plain._h, 2 * T.W + 48) == -1 and set_rows(plain._h, 2 * T.W) == 0
plain.close()
print("1D-OK")
"""


def test_upload_1d_refuses_a_non_dense_stride():
    """MFSR_UPLOAD_1D is read once per process: a child process with it set (this test is about that process)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MFSR_UPLOAD_1D="1")
    r = subprocess.run([sys.executable, "-c", _UPLOAD_1D_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "1D-OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("packing", [capi.PACK_MIPI10, capi.PACK_NONE])
def test_host_burst_captured_as_a_graph_equals_the_eager_one(packing):
    """The shape of tests/test_hipgraph_gpu.py: eager results of two bursts; a second pipeline warmed up, one host burst captured
    on fixed (pinned) host buffers, replayed on each burst's data.  The uploads, the unpack and the download are nodes of the
    graph: the image is in host memory when the replay has completed.  Then the same pipeline runs eagerly again."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    dev = torch.device("cuda:0")
    bits = 10 if packing else 12
    second, _, _ = synth.make_burst(W, H, N, seed=31, device="cpu")
    if bits == 10:
        second = [(f.view(torch.int16).to(torch.int32) >> 2).to(torch.int16).view(f.dtype) for f in second]
    bursts = [_burst(bits), [f.contiguous() for f in second]]
    if packing:
        bursts = [synth.pack_raw(b, packing) for b in bursts]
    cfg = _config(bits, 0, 1, 0, 4, packing)
    pipe = BurstPipeline(cfg, dev)
    eager = []
    for frames in bursts:
        got = pipe.process_host([f.pin_memory() for f in frames])
        pipe.host_sync()
        eager.append(got.clone())
    pipe.close()
    assert torch.equal(eager[0], _resident(bits, 0)) and not torch.equal(eager[0], eager[1])

    static = [torch.empty_like(f).pin_memory() for f in bursts[0]]           # graph inputs live at fixed addresses
    for dst, src in zip(static, bursts[0]):
        dst.copy_(src)
    gpipe = BurstPipeline(cfg, dev)
    gpipe.process_host(static)                                               # warm-up outside capture
    gpipe.host_sync()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g16 = gpipe.process_host(static)
    for k in (1, 0, 1):
        for dst, src in zip(static, bursts[k]):
            dst.copy_(src)
        g16.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g16, eager[k]), f"burst {k}: graph replay differs from the eager host burst"
    for k in (0, 1):                                                         # and eagerly again on the same pipeline
        for dst, src in zip(static, bursts[k]):
            dst.copy_(src)
        got = gpipe.process_host(static)
        gpipe.host_sync()
        assert torch.equal(got, eager[k]), f"burst {k}: eager after the capture"
    del graph
    gpipe.close()
