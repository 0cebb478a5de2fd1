"""Ghost suppression, host side (no device): the ABI of the new option, the argument checks of
mfsr_erodeMaskBatch, the numpy restatement of the erosion (tests/ghost_ref.py; the GPU tests compare the kernel with it bit for
bit), the moving-object burst generator, and the quality claim on the CPU oracle, where the scene of the GPU test was chosen
and its margins come from."""
import ctypes

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi
from multi_frame_super_resolution_amd.synth import make_burst, make_moving_burst
from tests import ghost_ref
from tests.ghost_ref import erode_ref


# ---- 1. the ABI ----------------------------------------------------------------------------------------------------------------
def test_config_layout_is_unchanged_and_mask_erode_defaults_to_zero():
    class Before(ctypes.Structure):       # mfsr_config as it was: the new field took the first of two reserved ints
        _fields_ = [f for f in capi.Config._fields_ if f[0] not in ("maskErode", "reserved")] + [("reserved", ctypes.c_int32 * 2)]

    assert ctypes.sizeof(capi.Config) == ctypes.sizeof(Before) == 220
    for name, _ in Before._fields_[:-1]:
        assert getattr(capi.Config, name).offset == getattr(Before, name).offset, name
    assert capi.Config.maskErode.offset == Before.reserved.offset
    assert capi.Config.reserved.offset == Before.reserved.offset + 4

    class Guarded(ctypes.Structure):
        _fields_ = [("cfg", capi.Config), ("guard", ctypes.c_uint8 * 64)]

    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
    capi.lib().config_default(ctypes.byref(g.cfg), 512, 384, 8, 2, 0)
    assert g.cfg.maskErode == 0 and g.cfg.reserved[0] == 0
    assert bytes(g.guard) == b"\xa5" * 64          # the library's sizeof(mfsr_config) is the binding's
    assert g.cfg.uploadRing == 0 and g.cfg.preAlignMaxAngle == 20.0


def test_workspace_is_unchanged_when_off_and_grows_by_the_scratch_masks_when_on():
    L = capi.lib()
    cfg = capi.Config()
    L.config_default(ctypes.byref(cfg), 512, 384, 8, 2, 0)
    base, sbase = L.burst_workspace_bytes(ctypes.byref(cfg)), L.stream_workspace_bytes(ctypes.byref(cfg), 1)
    assert base > 0 and sbase > 0
    cfg.maskErode = 0
    assert L.burst_workspace_bytes(ctypes.byref(cfg)) == base and L.stream_workspace_bytes(ctypes.byref(cfg), 1) == sbase
    group = L.raw["mfsr_burst_group_size"](ctypes.byref(cfg))
    one = 256 * 16 * 192                                     # one half-resolution float4 mask, rows padded to 64 bytes
    for r in (1, 2):
        cfg.maskErode = r
        assert L.burst_workspace_bytes(ctypes.byref(cfg)) == base + group * one
        assert L.stream_workspace_bytes(ctypes.byref(cfg), 1) == sbase + group * one
    for bad in (-1, 3, 5):
        cfg.maskErode = bad                                  # what mfsr_burst_create / mfsr_stream_create validate with
        assert L.burst_workspace_bytes(ctypes.byref(cfg)) == 0 and L.stream_workspace_bytes(ctypes.byref(cfg), 1) == 0


# ---- 2. argument checks before any device call ---------------------------------------------------------------------------------
def test_erode_rejects_bad_arguments_without_a_device():
    f = capi.lib().raw["mfsr_erodeMaskBatch"]
    INVALID = -1
    W, H, P = 40, 30, 16 * 40
    span = P * H
    a, b = 0x10000, 0x10000 + 4 * span          # never dereferenced: every call below fails its host check

    def call(n=1, ins=(a,), outs=(b,), w=W, h=H, ip=P, op=P, r=2, null_in=False, null_out=False):
        pi = None if null_in else (ctypes.c_void_p * len(ins))(*ins)
        po = None if null_out else (ctypes.c_void_p * len(outs))(*outs)
        return f(n, pi, po, w, h, ip, op, r, None)

    for r in (0, 3, -1):
        assert call(r=r) == INVALID
    assert call(w=2) == INVALID and call(h=2) == INVALID
    assert call(ip=P - 16) == INVALID and call(op=P - 16) == INVALID        # pitch < 16 * width
    assert call(ip=P + 8) == INVALID and call(op=P + 4) == INVALID          # not a multiple of 16
    assert call(null_in=True) == INVALID and call(null_out=True) == INVALID
    assert call(ins=(None,)) == INVALID and call(outs=(None,)) == INVALID
    assert call(ins=(a + 4,)) == INVALID and call(outs=(b + 8,)) == INVALID  # misaligned cells
    assert call(outs=(a,)) == INVALID                                        # in place
    assert call(outs=(a + span - 16,)) == INVALID                            # overlapping
    assert call(n=2, ins=(a, a + span), outs=(b, b)) == INVALID              # two outputs on one buffer
    assert call(n=2, ins=(a, a + span), outs=(b, a)) == INVALID              # an output on another frame's input
    assert call(n=0) == INVALID and call(n=5, ins=(a,) * 5, outs=(b,) * 5) == INVALID


# ---- 3. the numpy restatement ----------------------------------------------------------------------------------------------------
def _field(h, w, value):
    m = np.zeros((h, w, 4), np.float32)
    m[1:-1, 1:-1, :3] = value
    m[..., 3] = np.random.default_rng(3).random((h, w), dtype=np.float32)
    return m


@pytest.mark.parametrize("r", [1, 2])
def test_reference_erosion_properties(r):
    h, w = 21, 27
    m = _field(h, w, 1.0)
    m[10, 12, 1] = 0.0                                   # a lone 0 in a field of ones: a (2r+1)^2 block, in its channel only
    e = erode_ref(m, r)
    want = np.ones((h - 2, w - 2), np.float32)
    want[9 - r:10 + r, 11 - r:12 + r] = 0.0
    assert np.array_equal(e[1:-1, 1:-1, 1], want)
    assert (e[1:-1, 1:-1, 0] == 1).all() and (e[1:-1, 1:-1, 2] == 1).all()
    # cells next to the ring are not pulled to zero by it; the ring itself is zero in all four components
    assert e[1, 1, 0] == 1 and e[h - 2, w - 2, 2] == 1 and e[1, w - 2, 0] == 1
    ring = np.ones((h, w), bool)
    ring[1:-1, 1:-1] = False
    assert (e[ring] == 0).all()
    assert np.array_equal(e[1:-1, 1:-1, 3], m[1:-1, 1:-1, 3])       # .w passes through
    z = _field(h, w, 0.0)
    z[7, 7, :3] = 1.0                                    # a lone 1 in zeros vanishes
    assert (erode_ref(z, r)[..., :3] == 0).all()
    small = _field(3, 3, 0.5)                            # the smallest mask: one interior cell, its own window
    assert np.array_equal(erode_ref(small, r)[1, 1], small[1, 1])


def test_reference_erosion_is_not_idempotent():
    """Two passes of r = 1 equal one of r = 2 (and differ from one of r = 1): what an in-place kernel would get wrong."""
    rng = np.random.default_rng(11)
    m = _field(30, 41, 0.0)
    m[1:-1, 1:-1, :3] = rng.random((28, 39, 3), dtype=np.float32)
    once, twice, two = erode_ref(m, 1), erode_ref(erode_ref(m, 1), 1), erode_ref(m, 2)
    assert np.array_equal(twice, two)                    # (clamped windows compose: also at the border)
    assert not np.array_equal(once, twice)


# ---- 4. the moving-object burst ----------------------------------------------------------------------------------------------------
def test_moving_burst_generator():
    W, H, N, s = 128, 96, 4, 2
    kw = dict(scale=s, seed=31, max_shift=2.0)
    a = make_moving_burst(W, H, N, obj_size=(10, 8), obj_start=(20.0, 30.0), obj_step=(7.0, -2.5), **kw)
    b = make_moving_burst(W, H, N, obj_size=(10, 8), obj_start=(20.0, 30.0), obj_step=(7.0, -2.5), **kw)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    plain = make_burst(W, H, N, **kw)
    none = make_moving_burst(W, H, N, obj_size=None, **kw)
    assert all(torch.equal(x, y) for x, y in zip(plain[0], none[0]))          # no object: make_burst's bytes
    assert torch.equal(plain[1], none[1]) and torch.equal(plain[2], none[2]) and not none[3].any()
    assert torch.equal(a[1], plain[1])                                        # the object draws nothing from the scene's stream
    frames, _, gt, foot = a
    assert foot.shape == (N, s * H, s * W) and foot.dtype == torch.bool
    for k in range(N):
        ys, xs = torch.nonzero(foot[k], as_tuple=True)
        x0, y0 = round((20.0 + 7.0 * k) * s), round((30.0 - 2.5 * k) * s)
        assert (int(xs.min()), int(ys.min())) == (x0, y0)                     # footprints move by the requested step
        assert (int(xs.max()), int(ys.max())) == (x0 + 10 * s - 1, y0 + 8 * s - 1)
        assert int(foot[k].sum()) == 10 * s * 8 * s
    # ground truth: the object at the reference frame's position, the plain scene elsewhere
    assert torch.equal(gt[:, ~foot[0]], plain[2][:, ~foot[0]])
    assert not torch.equal(gt[:, foot[0]], plain[2][:, foot[0]])
    assert (gt[0][foot[0]] == gt[1][foot[0]]).all()                           # the patch is grey
    for k in range(N):                                                        # ... and every frame shows it
        assert not torch.equal(frames[k], plain[0][k])


# ---- 5. the quality claim on the CPU oracle ------------------------------------------------------------------------------------------
def test_erosion_suppresses_ghosts_on_the_oracle():
    """The scene of the GPU test (tests/ghost_ref.py::ghost_scene), through oracle.pipeline.OraclePipeline with the numpy
    erosion between stage F and stage G.  It must ghost (mse0(G) >= 4 mse0(S)), the erosion must help on G, and the figures
    the GPU test takes its margins from (ghost_ref.ORACLE_*) must be the ones measured here."""
    cfg, frames, gt, foot = ghost_ref.ghost_scene()
    G, S = ghost_ref.ghost_zones(foot, cfg.reference, 2, cfg.scale)
    assert G.sum() > 1000 and S.sum() > 100000
    mse = {}
    for r in (0, 2):
        out, _ = ghost_ref.run_oracle_eroded(cfg, frames, r)
        mse[r] = (ghost_ref.zone_mse(out, gt, G), ghost_ref.zone_mse(out, gt, S))
    ratio = mse[2][0] / mse[0][0]
    drop = ghost_ref.psnr_db(mse[0][1]) - ghost_ref.psnr_db(mse[2][1])
    gain = ghost_ref.psnr_db(mse[2][0]) - ghost_ref.psnr_db(mse[0][0])
    print(f"oracle: mse0(G) {mse[0][0]:.4e} mse0(S) {mse[0][1]:.4e} (x{mse[0][0] / mse[0][1]:.2f}); mse2(G) {mse[2][0]:.4e} "
          f"mse2(S) {mse[2][1]:.4e}; ratio G {ratio:.4f} (gain {gain:.2f} dB); PSNR0(S) - PSNR2(S) {drop:.4f} dB")
    assert mse[0][0] >= 4.0 * mse[0][1]           # condition: the scene ghosts
    assert mse[2][0] < mse[0][0]                  # claim
    assert abs(ratio - ghost_ref.ORACLE_RATIO_G) <= 0.002
    assert abs(drop - ghost_ref.ORACLE_DROP_S_DB) <= 0.002
