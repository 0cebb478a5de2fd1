"""The slot ring of the burst hold (mfsr_burst_hold_fuse) in mfsr_burst_workspace_bytes: host arithmetic only.

The ring of per-frame products (two flow images of the Lucas-Kanade ping-pong and one certainty mask per slot) has
max(8, min(cfg.frames, 16)) slots, so that the complete groups of a burst of up to 16 frames can wait for one warp+fuse launch.
The slots beyond the eighth are appended at the end of the layout: configurations of at most 8 frames keep their workspace
byte for byte (tests/golden/workspace_layout.json pins eight of them), every frame from the 9th to the 16th adds exactly one
slot, and more frames add nothing."""
import ctypes

import pytest

from multi_frame_super_resolution_amd import capi


def _bytes(width, height, frames, scale=2, mono=0, **fields):
    raw = capi.lib().raw
    cfg = capi.Config()
    assert raw["mfsr_config_default"](ctypes.byref(cfg), width, height, frames, scale, mono) == 0
    for k, v in fields.items():
        setattr(cfg, k, v)
    n = raw["mfsr_burst_workspace_bytes"](ctypes.byref(cfg))
    assert n > 0
    return n


def _up(v, a):
    return (v + a - 1) // a * a


def _slot_bytes(width, height, mono):
    """one ring slot as Bump::image places it: rows padded to 64 bytes, every image at a multiple of 256 bytes"""
    hw, hh = width // 2, height // 2
    tw, th = (width, height) if mono else (hw, hh)
    flow = _up(_up(tw * 8, 64) * th, 256)
    mask = _up(_up(hw * 16, 64) * hh, 256)
    return 2 * flow + mask


@pytest.mark.parametrize("width,height,scale,mono,fields", [
    (256, 192, 2, 0, {}),
    (328, 104, 2, 0, {"preAlign": 1}),
    (200, 136, 4, 0, {"maskErode": 1}),
    (128, 96, 2, 1, {}),
    (256, 160, 2, 0, {"uploadRing": 4, "rawPacking": capi.PACK_MIPI10}),
])
def test_ring_slots_follow_the_frame_count(width, height, scale, mono, fields):
    size = {n: _bytes(width, height, n, scale, mono, **fields) for n in range(1, 21)}
    # frames <= 8: the ring of eight slots, as before the hold existed
    assert len({size[n] for n in range(1, 9)}) == 1
    # 9 .. 16 frames: exactly one slot per frame (the sizes are multiples of 256, so is a slot: no rounding in between)
    slot = _slot_bytes(width, height, mono)
    for n in range(9, 17):
        assert size[n] - size[n - 1] == slot, n
    # more than 16 frames: the ring stays at 16 slots
    assert len({size[n] for n in range(16, 21)}) == 1
    assert size[16] - size[8] == 8 * slot
