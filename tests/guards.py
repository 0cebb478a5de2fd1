"""Canary bands around test buffers: one band logic for host arrays (the CPU pin tests) and device buffers (HipKernels).

A buffer is laid out ``[leading band | data | trailing band]`` in one byte array.  The trailing band starts at the first
byte after the data (never rounded up), so an overrun by one element lands in it; the data offset is rounded up to
``align`` only.  ``check_bands`` is the single place that decides whether a band survived.
"""
from __future__ import annotations

import numpy as np


def layout(nbytes: int, guard: int, align: int = 1):
    """(offset of the data, total bytes) of ``[guard | data | guard]`` with the data at a multiple of ``align``."""
    off = -(-guard // align) * align
    return off, off + nbytes + guard


def first_changed(band: np.ndarray, fill: int):
    """Offset of the first byte of ``band`` that is not ``fill``, or None."""
    bad = np.flatnonzero(band != fill)
    return int(bad[0]) if bad.size else None


def band_report(big: np.ndarray, off: int, nbytes: int, fill: int):
    """None when both bands of the byte array ``big`` are intact, else (which, first changed byte offset).  The offset counts
    from the start of the data: negative in the leading band, >= nbytes in the trailing one."""
    big = big.reshape(-1).view(np.uint8)
    for which, lo, hi in (("leading", 0, off), ("trailing", off + nbytes, big.size)):
        d = first_changed(big[lo:hi], fill)
        if d is not None:
            return which, lo + d - off
    return None


def check_bands(big: np.ndarray, off: int, nbytes: int, fill: int, what: str):
    rep = band_report(big, off, nbytes, fill)
    assert rep is None, (f"{what}: write outside the buffer: {rep[0]} guard changed, first at byte {rep[1]} "
                         f"relative to the data ({nbytes} bytes)")


class Guard:
    """Host buffers that sit between two canary bands."""

    PAD = 256
    FILL = 0xA5

    def __init__(self, pad=None, fill=None):
        self.pad = self.PAD if pad is None else pad
        self.fill = self.FILL if fill is None else fill
        self.bufs = []

    def new(self, init):
        init = np.ascontiguousarray(init)
        off, total = layout(init.nbytes, self.pad)
        big = np.full(total, self.fill, np.uint8)
        v = big[off:off + init.nbytes].view(init.dtype).reshape(init.shape)
        v[...] = init
        self.bufs.append((big, off, init.nbytes))
        return v

    def zeros(self, shape, dtype=np.float32):
        return self.new(np.zeros(shape, dtype))

    def check(self, what):
        for big, off, nbytes in self.bufs:
            check_bands(big, off, nbytes, self.fill, what)
