"""Host-side mirror of the burst driver in ``csrc/pipeline.cpp`` (C-ABI
``mfsr_burst_*``): N raw frames in -> one x-s frame out, the contract of the
reference CLI ``finalProject/Project/multi_frame_sr.cpp:146-209``.

torch only owns device memory and streams here; all arithmetic is in the HIP
library.  No CPU fallback: constructing a pipeline without a HIP device raises.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Iterable, Optional, Sequence, Tuple

import torch

from . import capi


def default_config(width: int, height: int, frames: int, scale: int = 2, mono: bool = False) -> capi.Config:
    cfg = capi.Config()
    capi.lib().config_default(ctypes.byref(cfg), width, height, frames, scale, 1 if mono else 0)
    return cfg


WINDOW_GRID = 16  # zoom windows start on this HR grid and span multiples of it (or reach the frame's edge)


def align_window(cfg: capi.Config, x: int, y: int, w: int, h: int) -> Tuple[int, int, int, int]:
    """Smallest window the kernels take (mfsr_window_check) that covers the HR rectangle [x, x+w) x [y, y+h), clipped to
    the frame: the origin rounded down to the 16-pixel grid, the far edges rounded up to it or to the frame's edge.
    Pure Python (no device)."""
    hr_w, hr_h = cfg.width * cfg.scale, cfg.height * cfg.scale
    if w <= 0 or h <= 0:
        raise ValueError("window must not be empty")
    x1, y1 = min(x + w, hr_w), min(y + h, hr_h)
    x, y = max(x, 0), max(y, 0)
    if x >= x1 or y >= y1:
        raise ValueError(f"window ({x}, {y}, {w}, {h}) lies outside the {hr_w}x{hr_h} output")
    g = WINDOW_GRID
    ax, ay = x // g * g, y // g * g
    ax1, ay1 = min(-(-x1 // g) * g, hr_w), min(-(-y1 // g) * g, hr_h)
    return ax, ay, ax1 - ax, ay1 - ay


class _Window:
    """A requested HR rectangle, the aligned window the library works on, and the crop of it the caller asked for."""

    def __init__(self, cfg: capi.Config, window: Optional[Sequence[int]]):
        hr_w, hr_h = cfg.width * cfg.scale, cfg.height * cfg.scale
        self._frame = (hr_w, hr_h)
        if window is None:
            self.aligned = (0, 0, hr_w, hr_h)
            self.crop = (slice(None), slice(None))
            self.on = False
            self._rect = None
            return
        x, y, w, h = (int(v) for v in window)
        self._asked = (x, y, w, h)
        self._base = align_window(cfg, x, y, w, h)
        self._rect = (max(x, 0), max(y, 0), min(x + w, hr_w), min(y + h, hr_h))
        self.grow(0)

    def grow(self, ring: int) -> bool:
        """The aligned window grown by ``ring`` pixels (a multiple of 16) on every side and clipped to the frame, with the crop
        that still returns the rectangle asked for: a stencil of up to ``ring`` pixels in the finish then sees the pixels the
        whole-frame burst sees.  Returns whether the aligned window changed."""
        if self._rect is None:
            return False
        hr_w, hr_h = self._frame
        bx, by, bw, bh = self._base
        ax, ay = max(bx - ring, 0), max(by - ring, 0)
        ax1, ay1 = min(bx + bw + ring, hr_w), min(by + bh + ring, hr_h)
        aligned = (ax, ay, ax1 - ax, ay1 - ay)
        changed = aligned != getattr(self, "aligned", None)
        self.aligned = aligned
        cx, cy, cx1, cy1 = self._rect
        self.crop = (slice(cy - ay, cy1 - ay), slice(cx - ax, cx1 - ax))
        self.on = self.aligned != (0, 0, hr_w, hr_h)
        return changed

    def apply(self, setter, handle):
        if self.on:
            setter(handle, *self.aligned)

    def __call__(self, img: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        return None if img is None else img[self.crop]

    def check_yuv(self, fmt: int):
        """A two-plane 4:2:0 format needs a rectangle of whole 2 x 2 blocks."""
        if fmt in capi.YUV_FORMATS and self._rect is not None and any(v % 2 for v in self._asked):
            raise ValueError(f"window {self._asked}: x, y, w and h must be even for a two-plane YUV 4:2:0 output")

    def output(self, buf: Optional[torch.Tensor], fmt: int) -> Optional[torch.Tensor]:
        """The integer output of the rectangle asked for: the crop of the image, or for a two-plane format the crop of both
        planes of the aligned window's flat buffer, as one flat tensor again (a copy; the buffer itself without a window)."""
        if buf is None or fmt not in capi.YUV_FORMATS:
            return self(buf)
        if self._rect is None:
            return buf
        ys, xs = self.crop
        y, uv = yuv_planes(buf, fmt, self.aligned[3], self.aligned[2])
        return torch.cat([y[ys, xs].reshape(-1), uv[ys.start // 2:ys.stop // 2, xs.start // 2:xs.stop // 2].reshape(-1)])


Selection = namedtuple("Selection", "reference kept sums rect")
Selection.__doc__ = """What BurstPipeline.process_selected chose: the reference frame, the kept frame indices (index order), the
sharpness score of every frame (mfsr_frameSharpness) and the half-resolution rectangle (x0, y0, x1, y1) that was scored."""


def sharpness_rect(cfg: capi.Config, window: Optional[Sequence[int]] = None) -> Tuple[int, int, int, int]:
    """The half-resolution rectangle (x0, y0, x1, y1) mfsr_burst_select_frames scores: without a window the frame less an
    8-pixel margin (1 pixel if 8 leave nothing); with an aligned zoom window (x, y, w, h) its raw footprint, clipped to the
    scorable part [1, W/2-1) x [1, H/2-1).  Pure Python (no device)."""
    hw, hh = cfg.width // 2, cfg.height // 2
    if window is None:
        m = 8 if hw - 8 > 8 and hh - 8 > 8 else 1
        return m, m, hw - m, hh - m
    x, y, w, h = (int(v) for v in window)
    s2 = 2 * cfg.scale
    lo, hi, lim = [x // s2, y // s2], [-(-(x + w) // s2), -(-(y + h) // s2)], [hw - 1, hh - 1]
    for d in range(2):
        lo[d], hi[d] = max(lo[d], 1), min(hi[d], lim[d])
        if hi[d] <= lo[d]:
            lo[d] = min(lo[d], lim[d] - 1)
            hi[d] = lo[d] + 1
    return lo[0], lo[1], hi[0], hi[1]


def _raw_frames(frames: Sequence[torch.Tensor], cfg: capi.Config):
    """Check a list of raw device frames (one device, one row stride); returns (device, pitch in bytes)."""
    if not frames:
        raise ValueError("at least one frame is needed")
    dev = frames[0].device
    pitch = frames[0].stride(0) * 2
    for f in frames:
        if (f.device != dev or not f.is_cuda or f.dtype not in (torch.int16, torch.uint16) or f.dim() != 2
                or tuple(f.shape) != (cfg.height, cfg.width) or f.stride(1) != 1 or f.stride(0) * 2 != pitch):
            raise ValueError(f"frames must be 16-bit {cfg.height}x{cfg.width} tensors on one HIP device with contiguous rows "
                             "and one row stride")
    return dev, pitch


def _ptr_table(frames: Sequence[torch.Tensor]):
    """The frame pointer table of a C-ABI call (``const uint16_t* const*``)."""
    return (ctypes.c_void_p * len(frames))(*[f.data_ptr() for f in frames])


def _i4(seq):
    """Four integers as the ``int32_t[4]`` of a C-ABI call (a CFA, black levels, a rectangle)."""
    return (ctypes.c_int32 * 4)(*seq)


def frame_sharpness(frames: Sequence[torch.Tensor], cfg: capi.Config,
                    rect: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Sharpness score of every frame (mfsr_frameSharpness): an int64 device tensor, exact.  ``frames``: 16-bit [H, W]
    device tensors of cfg's size, rows contiguous and all with the same row stride (pitched views are fine).  ``rect``:
    the half-resolution rectangle (x0, y0, x1, y1) to score; None = the whole-frame rule of ``sharpness_rect``."""
    frames = list(frames)
    dev, pitch = _raw_frames(frames, cfg)
    r = sharpness_rect(cfg) if rect is None else tuple(int(v) for v in rect)
    n = len(frames)
    with torch.cuda.device(dev):
        sums = torch.empty(n, dtype=torch.int64, device=dev)
        capi.lib().frameSharpness(n, _ptr_table(frames), pitch, cfg.width, cfg.height, _i4(cfg.cfa), 1 if cfg.mono else 0, _i4(r),
                                  sums.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return sums


def defect_defaults(cfg: capi.Config, n_frames: int) -> Tuple[int, int, int]:
    """(threshold, spread, min_votes) the defect vote uses when none are given: a 64th of the white level, half the local
    range of the neighbours on top of it (spread 2, in quarters), and three quarters of the frames but always a strict
    majority.  Pure Python (no device)."""
    threshold = max(1, int(max(cfg.white)) // 64)
    min_votes = max(n_frames // 2 + 1, -(-3 * n_frames // 4))
    return threshold, 2, min_votes


def detect_defects(frames: Sequence[torch.Tensor], cfg: capi.Config, threshold: Optional[int] = None, spread: int = 2,
                   min_votes: Optional[int] = None):
    """Defect map of a burst (mfsr_detectDefects): (uint8 [H, W] device tensor, 0 = good, 1 = hot, 2 = cold; (hot, cold)
    pixel counts).  ``frames`` as for ``frame_sharpness`` (pitched views are fine); they are only read.  threshold /
    min_votes None = ``defect_defaults``."""
    frames = list(frames)
    dev, pitch = _raw_frames(frames, cfg)
    n = len(frames)
    t0, _, v0 = defect_defaults(cfg, n)
    threshold = t0 if threshold is None else int(threshold)
    min_votes = v0 if min_votes is None else int(min_votes)
    with torch.cuda.device(dev):
        dmap = torch.empty(cfg.height, cfg.width, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        capi.lib().detectDefects(n, _ptr_table(frames), pitch, cfg.width, cfg.height, 1 if cfg.mono else 0, threshold, int(spread), min_votes,
                                 dmap.data_ptr(), dmap.stride(0), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        hot, cold = counts.cpu().tolist()
    return dmap, (hot, cold)


def repair_defects(frames: Sequence[torch.Tensor], defect_map: torch.Tensor, cfg: capi.Config):
    """The frames repaired under ``defect_map`` (mfsr_repairDefects; any uint8 [H, W] device map, non-zero = defective): a
    list of new contiguous tensors, the caller's frames stay untouched."""
    frames = list(frames)
    dev, _ = _raw_frames(frames, cfg)
    if (defect_map.device != dev or defect_map.dtype != torch.uint8 or tuple(defect_map.shape) != (cfg.height, cfg.width)
            or defect_map.stride(1) != 1):
        raise ValueError(f"defect_map must be a uint8 {cfg.height}x{cfg.width} tensor on the frames' device with contiguous rows")
    out = [f.clone(memory_format=torch.contiguous_format) for f in frames]
    with torch.cuda.device(dev):
        capi.lib().repairDefects(len(out), _ptr_table(out), 2 * cfg.width, cfg.width, cfg.height, 1 if cfg.mono else 0, defect_map.data_ptr(),
                                 defect_map.stride(0), torch.cuda.current_stream().cuda_stream)
    return out


Exposure = namedtuple("Exposure", "reference gains status levels gains_q16")
Exposure.__doc__ = """What BurstPipeline.process_matched measured and applied: the frame the others were matched to, the gain of
every frame and colour as floats (``gains_q16`` / 65536; [n][3]), the status of every frame (0 matched, 1 within the deadband or
the reference, 2 unmeasurable, 3 out of range: only status 0 frames were changed), the level sums [n][5] (S[q], q = 0..3, and
the usable-quad count C) and the raw Q16 gains."""

ExposureDefaults = namedtuple("ExposureDefaults", "black sat max_value deadband min_gain max_gain per_colour")


def exposure_defaults(cfg: capi.Config) -> ExposureDefaults:
    """The levels and bounds of exposure matching when none are given (the rule of mfsr_exposure_defaults, restated): black
    level of every quad position (its colour's cfg.black rounded to nearest; mono: cfg.black[0]), sat = the smallest
    floor(black + white) of the channels, max_value = int(cfg.maxVal), deadband 164 (0.25 %), gains within [16384, 262144]
    (+-2 EV), one common gain.  Pure Python (no device)."""
    import math
    colour = [0] * 4 if cfg.mono else [int(c) for c in cfg.cfa]
    if any(c < 0 or c > 2 for c in colour):
        raise ValueError("exposure matching needs a CFA of red, green and blue")
    black = tuple(int(math.floor(float(cfg.black[c]) + 0.5)) for c in colour)
    sat = min(int(math.floor(float(cfg.black[c]) + float(cfg.white[c]))) for c in range(3))
    return ExposureDefaults(black, sat, int(cfg.maxVal), 164, 16384, 262144, False)


def frame_levels(frames: Sequence[torch.Tensor], cfg: capi.Config, rect: Optional[Sequence[int]] = None,
                 sat: Optional[int] = None) -> torch.Tensor:
    """Level sums of every frame (mfsr_frameLevels): an int64 [n, 5] device tensor, exact -- per frame the sums S[q] of
    max(v - black[q], 0) over the usable quads (all four samples < sat) of the half-resolution rectangle, q = 0..3, and the
    number of usable quads.  ``frames`` as for ``frame_sharpness`` (pitched views are fine); they are only read.  rect None =
    ``sharpness_rect(cfg)``; sat None = ``exposure_defaults``."""
    frames = list(frames)
    dev, pitch = _raw_frames(frames, cfg)
    d = exposure_defaults(cfg)
    r = sharpness_rect(cfg) if rect is None else tuple(int(v) for v in rect)
    n = len(frames)
    with torch.cuda.device(dev):
        levels = torch.empty(n, 5, dtype=torch.int64, device=dev)
        capi.lib().frameLevels(n, _ptr_table(frames), pitch, cfg.width, cfg.height, _i4(d.black),
                               d.sat if sat is None else int(sat), _i4(r), levels.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return levels


def exposure_gains(levels, cfg: capi.Config, reference: int, per_colour: bool = False, deadband: Optional[int] = None,
                   min_gain: Optional[int] = None, max_gain: Optional[int] = None):
    """(gains, status) of mfsr_exposure_gains: Q16 gains [n][3] (65536 = 1.0) and the status of every frame, as lists of Python
    ints.  ``levels``: [n, 5] integers (a tensor on any device, an array or nested lists).  Host only: no device is needed."""
    if isinstance(levels, torch.Tensor):
        levels = levels.cpu().tolist()
    rows = [[int(v) for v in row] for row in levels]
    n = len(rows)
    if n == 0 or any(len(row) != 5 for row in rows):
        raise ValueError("levels must be [n, 5] with n >= 1")
    d = exposure_defaults(cfg)
    flat = (ctypes.c_longlong * (5 * n))(*[v for row in rows for v in row])
    gains, status = (ctypes.c_int32 * (3 * n))(), (ctypes.c_int32 * n)()
    capi.lib().exposure_gains(n, flat, int(reference), _i4(cfg.cfa), 1 if cfg.mono else 0, 1 if per_colour else 0,
                              d.deadband if deadband is None else int(deadband), d.min_gain if min_gain is None else int(min_gain),
                              d.max_gain if max_gain is None else int(max_gain), gains, status)
    return [[int(gains[3 * k + c]) for c in range(3)] for k in range(n)], [int(s) for s in status]


def apply_gains(frames: Sequence[torch.Tensor], gains, status, cfg: capi.Config):
    """The frames with their gains applied (mfsr_applyGains; ``gains`` [n][3] Q16, ``status`` [n]: only status 0 frames
    change): a list of new contiguous tensors, the caller's frames stay untouched."""
    frames = list(frames)
    dev, _ = _raw_frames(frames, cfg)
    n = len(frames)
    if len(gains) != n or len(status) != n:
        raise ValueError("one gain triple and one status per frame are needed")
    d = exposure_defaults(cfg)
    out = [f.clone(memory_format=torch.contiguous_format) for f in frames]
    with torch.cuda.device(dev):
        capi.lib().applyGains(n, _ptr_table(out), 2 * cfg.width, cfg.width, cfg.height, _i4(cfg.cfa), 1 if cfg.mono else 0,
                              _i4(d.black), d.sat, d.max_value,
                              (ctypes.c_int32 * (3 * n))(*[int(g) for row in gains for g in row]),
                              (ctypes.c_int32 * n)(*[int(s) for s in status]), torch.cuda.current_stream().cuda_stream)
    return out


NoiseDefaults = namedtuple("NoiseDefaults", "black white sat min_blocks rect")
NoiseStats = namedtuple("NoiseStats", "hist level_sum count")
NoiseStats.__doc__ = """The tables of mfsr_noiseStats as device tensors: hist int32 [4, 64, 272] (u32 bit patterns), level_sum and
count int64 [4, 64]."""


def noise_defaults(cfg: capi.Config) -> NoiseDefaults:
    """The levels and bounds of noise calibration when none are given (the rule of mfsr_noise_defaults, restated): black and sat
    as ``exposure_defaults``, white level of every quad position (its colour's cfg.white; mono: cfg.white[0]), min_blocks 200,
    rect = the whole grid of 8x8-sample blocks less one block of border.  Pure Python (no device)."""
    d = exposure_defaults(cfg)
    colour = [0] * 4 if cfg.mono else [int(c) for c in cfg.cfa]
    if cfg.width < 24 or cfg.height < 24:
        raise ValueError("noise calibration needs frames of at least 24 x 24 samples")
    return NoiseDefaults(d.black, tuple(float(cfg.white[c]) for c in colour), d.sat, 200,
                         (1, 1, cfg.width // 8 - 1, cfg.height // 8 - 1))


def noise_stats(frames: Sequence[torch.Tensor], cfg: capi.Config, rect: Optional[Sequence[int]] = None,
                sat: Optional[int] = None) -> NoiseStats:
    """Block statistics of raw frames (mfsr_noiseStats), exact: per quad position and level bin the histogram of the blocks'
    pair-difference energies D, the sum of their level sums S and their number.  ``frames`` as for ``frame_sharpness`` (pitched
    views are fine, at most 64); they are only read.  rect None / sat None = ``noise_defaults``; rect is (bx0, by0, bx1, by1) in
    blocks of 8 x 8 samples."""
    frames = list(frames)
    dev, pitch = _raw_frames(frames, cfg)
    d = noise_defaults(cfg)
    r = d.rect if rect is None else tuple(int(v) for v in rect)
    n = len(frames)
    with torch.cuda.device(dev):
        hist = torch.empty(4, 64, 272, dtype=torch.int32, device=dev)
        level_sum = torch.empty(4, 64, dtype=torch.int64, device=dev)
        count = torch.empty(4, 64, dtype=torch.int64, device=dev)
        capi.lib().noiseStats(n, _ptr_table(frames), pitch, cfg.width, cfg.height, _i4(d.black),
                              d.sat if sat is None else int(sat), _i4(r), hist.data_ptr(), level_sum.data_ptr(), count.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    return NoiseStats(hist, level_sum, count)


NOISE_TEMPORAL_TOL = 1.0 / 16.0   # the default phase tolerance of burst noise calibration, in quads


def noise_stats_temporal(frames: Sequence[torch.Tensor], flows: Sequence[Optional[torch.Tensor]], cfg: capi.Config,
                         tol: float = NOISE_TEMPORAL_TOL, rect: Optional[Sequence[int]] = None,
                         sat: Optional[int] = None) -> NoiseStats:
    """Block statistics of the DIFFERENCES of the frames of a burst (mfsr_noiseStatsTemporal), exact:
    wherever two frames are displaced against each other by a whole number of quads to within ``tol`` (0 .. 0.25 quads), the
    tables of ``noise_stats`` are taken on frame j (levels) and on the difference of the two frames (variances).  ``frames``:
    2 .. 64 frames as for ``noise_stats``.  ``flows``: per frame its flow field in the burst's convention -- a float32 device
    tensor [fh, fw, 2] with contiguous texels and one row stride, (fh, fw) = ``BurstPipeline.field_dims()[0]`` -- or None for
    zero flow (the reference).  rect / sat None = ``noise_defaults``.  Fit the result with ``noise_fit(..., temporal=True)``."""
    frames, flows = list(frames), list(flows)
    dev, pitch = _raw_frames(frames, cfg)
    if len(flows) != len(frames):
        raise ValueError("one flow field (or None) per frame is needed")
    given = [f for f in flows if f is not None]
    shape = tuple(given[0].shape) if given else (cfg.height // 2, cfg.width // 2, 2)
    fpitch = given[0].stride(0) * 4 if given else 8 * shape[1]
    for f in given:
        if (f.device != dev or f.dtype != torch.float32 or f.dim() != 3 or tuple(f.shape) != shape or shape[2] != 2
                or f.stride(2) != 1 or f.stride(1) != 2 or f.stride(0) * 4 != fpitch):
            raise ValueError("flows must be float32 [fh, fw, 2] tensors of one shape and row stride on the frames' device")
    d = noise_defaults(cfg)
    r = d.rect if rect is None else tuple(int(v) for v in rect)
    n = len(frames)
    with torch.cuda.device(dev):
        hist = torch.empty(4, 64, 272, dtype=torch.int32, device=dev)
        level_sum = torch.empty(4, 64, dtype=torch.int64, device=dev)
        count = torch.empty(4, 64, dtype=torch.int64, device=dev)
        fptrs = (ctypes.c_void_p * n)(*[None if f is None else f.data_ptr() for f in flows])
        capi.lib().noiseStatsTemporal(n, _ptr_table(frames), pitch, cfg.width, cfg.height, fptrs, fpitch, shape[1], shape[0],
                                      _i4(d.black), d.sat if sat is None else int(sat), _i4(r), float(tol), hist.data_ptr(),
                                      level_sum.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return NoiseStats(hist, level_sum, count)


def noise_fit(stats, cfg: capi.Config, min_blocks: Optional[int] = None, temporal: bool = False):
    """(alpha, beta, status, points) of mfsr_noise_fit on the tables of ``noise_stats`` (tensors on any device or arrays):
    the least-squares line through (level, variance) of every well-filled level bin, as Python floats (doubles).  status 0 ok,
    2 unmeasurable (alpha = beta = 0), 3 alpha <= 0.  Host only: no device is needed.  ``temporal=True``: the tables are those of
    ``noise_stats_temporal`` (mfsr_noise_fit_temporal: the variances are those of a difference of two frames)."""
    import numpy as np

    def host(t, dtype):
        a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        return np.ascontiguousarray(a.view(dtype) if a.dtype.itemsize == np.dtype(dtype).itemsize else a.astype(dtype))

    hist, level_sum, count = host(stats[0], np.uint32), host(stats[1], np.int64), host(stats[2], np.int64)
    if hist.shape != (4, 64, 272) or level_sum.shape != (4, 64) or count.shape != (4, 64):
        raise ValueError("stats must be (hist [4, 64, 272], level_sum [4, 64], count [4, 64])")
    d = noise_defaults(cfg)
    a, b = ctypes.c_double(), ctypes.c_double()
    st, n = ctypes.c_int32(), ctypes.c_int32()
    fit = capi.lib().noise_fit_temporal if temporal else capi.lib().noise_fit
    fit(hist.ctypes.data, level_sum.ctypes.data, count.ctypes.data, _i4(d.black),
        (ctypes.c_float * 4)(*d.white), d.min_blocks if min_blocks is None else int(min_blocks),
        ctypes.byref(a), ctypes.byref(b), ctypes.byref(st), ctypes.byref(n))
    return a.value, b.value, st.value, n.value


def calibrate_noise(frames: Sequence[torch.Tensor], cfg: capi.Config):
    """(alpha, beta, status) of the noise model var = alpha * I + beta measured on raw device frames: ``noise_stats`` with the
    defaults, then ``noise_fit``.  alpha and beta are construction-time configuration, so the use is two steps::

        alpha, beta, status = calibrate_noise(chart_frames, cfg)
        if status == 0:
            cfg.alpha, cfg.beta = alpha, beta
        pipe = BurstPipeline(cfg)

    The frames must show flat areas at many levels (a chart capture per sensor gain, or a natural image with flat regions):
    a single frame cannot tell pixel-scale texture from noise."""
    a, b, st, _ = noise_fit(noise_stats(frames, cfg), cfg)
    return a, b, st


ShadingDefaults = namedtuple("ShadingDefaults", "black sat max_value cell min_quads max_gain")


def shading_defaults(cfg: capi.Config) -> ShadingDefaults:
    """The levels and bounds of lens-shading correction when none are given (the rule of mfsr_shading_defaults, restated): black,
    sat and max_value as ``exposure_defaults``; cell = the largest power of two up to 64 that is at most min(W/2, H/2) - 1, never
    below 8 (frames smaller than 18 x 18 are refused); min_quads 64; max_gain 524288 (3 stops).  Pure Python (no device)."""
    d = exposure_defaults(cfg)
    m = min(cfg.width, cfg.height) // 2 - 1
    if cfg.width % 2 or cfg.height % 2 or m < 8:
        raise ValueError("lens-shading correction needs frames of at least 18 x 18 samples, width and height even")
    cell = 64
    while cell > m:
        cell //= 2
    return ShadingDefaults(d.black, d.sat, d.max_value, cell, 64, 524288)


def shading_grid(cfg: capi.Config, cell: Optional[int] = None) -> Tuple[int, int]:
    """(gw, gh): the grid points of a gain map of cell ``cell`` quads (None = ``shading_defaults``) over cfg's frame; the map is
    int32 [4, gh, gw].  Pure Python (no device)."""
    cell = shading_defaults(cfg).cell if cell is None else int(cell)
    if cell not in (8, 16, 32, 64, 128, 256):
        raise ValueError("cell must be a power of two in [8, 256]")
    return (cfg.width // 2 - 2 + cell) // cell + 1, (cfg.height // 2 - 2 + cell) // cell + 1


def shading_stats(frames: Sequence[torch.Tensor], cfg: capi.Config, cell: Optional[int] = None, sat: Optional[int] = None):
    """Box statistics of flat-field frames (mfsr_shadingStats), exact: (sums int64 [4, gh, gw], counts int64 [gh, gw]) device
    tensors -- per grid point of the gain map the sums of max(v - black[q], 0) over the usable quads (all four samples < sat) of
    its box in all frames, and their number.  ``frames`` as for ``frame_sharpness`` (pitched views are fine, at most 64); they
    are only read.  cell None / sat None = ``shading_defaults``."""
    frames = list(frames)
    dev, pitch = _raw_frames(frames, cfg)
    d = shading_defaults(cfg)
    cell = d.cell if cell is None else int(cell)
    gw, gh = shading_grid(cfg, cell)
    n = len(frames)
    with torch.cuda.device(dev):
        sums = torch.empty(4, gh, gw, dtype=torch.int64, device=dev)
        counts = torch.empty(gh, gw, dtype=torch.int64, device=dev)
        capi.lib().shadingStats(n, _ptr_table(frames), pitch, cfg.width, cfg.height, cell, _i4(d.black),
                                d.sat if sat is None else int(sat), sums.data_ptr(), counts.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
    return sums, counts


def shading_fit(sums, counts, min_quads: int = 64, max_gain: int = 524288):
    """(map, status) of mfsr_shading_fit on the tables of ``shading_stats`` (tensors on any device or arrays): the Q16 gain map
    as a numpy int32 array [4, gh, gw], relative to the brightest grid point.  status 0 ok, 2 unmeasurable (every gain 65536),
    3 some gain was clamped at ``max_gain``.  Host only: no device is needed."""
    import numpy as np

    def host(t):
        return np.ascontiguousarray((t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.int64))

    s, c = host(sums), host(counts)
    if s.ndim != 3 or s.shape[0] != 4 or c.shape != s.shape[1:]:
        raise ValueError("sums must be [4, gh, gw] and counts [gh, gw]")
    gh, gw = c.shape
    gain_map = np.empty((4, gh, gw), dtype=np.int32)
    st = ctypes.c_int32()
    capi.lib().shading_fit(s.ctypes.data, c.ctypes.data, gw, gh, int(min_quads), int(max_gain), gain_map.ctypes.data, ctypes.byref(st))
    return gain_map, st.value


def calibrate_shading(flat_frames: Sequence[torch.Tensor], cfg: capi.Config, cell: Optional[int] = None):
    """(gain map, status) measured on raw device frames of a uniformly lit diffuser: ``shading_stats``, then ``shading_fit``
    with the defaults.  The map is an int32 [4, gh, gw] device tensor, what ``apply_shading`` and
    ``BurstPipeline.process_shaded`` take; status as for ``shading_fit``."""
    d = shading_defaults(cfg)
    gain_map, st = shading_fit(*shading_stats(flat_frames, cfg, cell), min_quads=d.min_quads, max_gain=d.max_gain)
    return torch.from_numpy(gain_map).to(flat_frames[0].device), st


def _shading_map(gain_map: torch.Tensor, cfg: capi.Config, cell: Optional[int], dev) -> int:
    """Check a gain map against cfg's frame and the cell (None = ``shading_defaults``); returns the cell."""
    cell = shading_defaults(cfg).cell if cell is None else int(cell)
    gw, gh = shading_grid(cfg, cell)
    if (not isinstance(gain_map, torch.Tensor) or gain_map.device != dev or gain_map.dtype != torch.int32
            or tuple(gain_map.shape) != (4, gh, gw) or not gain_map.is_contiguous()):
        raise ValueError(f"gain_map must be a contiguous int32 [4, {gh}, {gw}] tensor on the frames' device (cell {cell})")
    return cell


def apply_shading(frames: Sequence[torch.Tensor], gain_map: torch.Tensor, cfg: capi.Config, cell: Optional[int] = None):
    """The frames with the gain map applied (mfsr_applyShading; ``gain_map`` int32 [4, gh, gw] on the frames' device, Q16, every
    value in [4096, 1048576] -- not checked): a list of new contiguous tensors, the caller's frames stay untouched.  cell None =
    ``shading_defaults``."""
    frames = list(frames)
    dev, _ = _raw_frames(frames, cfg)
    cell = _shading_map(gain_map, cfg, cell, dev)
    d = shading_defaults(cfg)
    out = [f.clone(memory_format=torch.contiguous_format) for f in frames]
    with torch.cuda.device(dev):
        capi.lib().applyShading(len(out), _ptr_table(out), 2 * cfg.width, cfg.width, cfg.height, gain_map.data_ptr(), cell,
                                _i4(d.black), d.max_value, torch.cuda.current_stream().cuda_stream)
    return out


def packed_row_bytes(packing: int, width: int) -> int:
    """Bytes of a dense packed row of ``width`` samples (mfsr_packed_row_bytes): width * bits / 8.  ValueError for an unknown
    packing or a width that is not a whole number of groups (4 samples at 10 bits, 2 at 12)."""
    n = capi.lib().raw["mfsr_packed_row_bytes"](int(packing), int(width))
    if n < 0:
        raise ValueError(f"packing {packing} does not take rows of {width} samples")
    return n


def unpack_raw(packed, packing: int, width: int, out=None):
    """Packed 10 / 12-bit frames widened to 16-bit samples on the device (mfsr_unpackRaw; the layouts of
    ``capi.PACK_*`` are stated in include/mfsr.h).  ``packed``: a uint8 device tensor [height, rowBytes] or a sequence of such
    tensors of one shape and row stride, rowBytes >= ``packed_row_bytes(packing, width)`` (bytes beyond the dense row are line
    padding and are not read); rows contiguous, the tensors may be pitched views at any byte offset.  ``out``: int16 / uint16
    device tensors [height, width] (one, or a sequence), rows contiguous, one row stride; by default fresh dense uint16
    tensors.  Samples come out as they are (0..1023 / 0..4095).  One launch per 64 frames on the current stream.  Returns
    ``out`` (a tensor for a tensor, a list for a sequence)."""
    single = isinstance(packed, torch.Tensor)
    ins = [packed] if single else list(packed)
    if not ins:
        raise ValueError("at least one frame is needed")
    dense = packed_row_bytes(packing, width)
    dev, h, row_bytes = ins[0].device, int(ins[0].shape[0]), ins[0].stride(0)
    for t in ins:
        if not (t.is_cuda and t.device == dev and t.dtype == torch.uint8 and t.dim() == 2 and t.shape[0] == h and h > 0
                and t.shape[1] >= dense and t.stride(1) == 1 and t.stride(0) == row_bytes):
            raise ValueError(f"packed frames must be uint8 [height, >= {dense}] tensors on one HIP device with contiguous rows "
                             "and one row stride")
    if out is None:
        outs = [torch.empty(h, width, dtype=torch.uint16, device=dev) for _ in ins]
        ret = outs[0] if single else outs
    else:
        outs = [out] if isinstance(out, torch.Tensor) else list(out)
        ret = out
        if len(outs) != len(ins):
            raise ValueError("out must have as many frames as the input")
    pitch = outs[0].stride(0) * 2
    for t in outs:
        if not (t.is_cuda and t.device == dev and t.dtype in (torch.int16, torch.uint16) and tuple(t.shape) == (h, width)
                and t.stride(1) == 1 and t.stride(0) * 2 == pitch):
            raise ValueError(f"out: 16-bit {h}x{width} tensors on the input's device with contiguous rows and one row stride")
    with torch.cuda.device(dev):
        for k0 in range(0, len(ins), 64):
            n = min(64, len(ins) - k0)
            capi.lib().unpackRaw(n, _ptr_table(ins[k0:k0 + n]), row_bytes, int(packing), _ptr_table(outs[k0:k0 + n]), pitch,
                                 int(width), h, torch.cuda.current_stream().cuda_stream)
    return ret


def erode_mask(masks, radius: int, out=None):
    """Erosion of certainty masks (mfsr_erodeMaskBatch): every colour certainty (.x .y .z) becomes its
    minimum over the (2*radius+1)^2 neighbourhood clamped to the interior, .w passes through, the one-cell ring is zero.
    ``masks``: a float32 device tensor [h, w, 4] or [n, h, w, 4], or a sequence of [h, w, 4] tensors of one size; rows may be
    pitched (a row stride that is a multiple of 4 floats), cells are dense.  ``out``: the same form as ``masks``, must not
    overlap it; by default fresh dense tensors.  Returns ``out``.  radius 1 or 2; up to MFSR_MAX_FUSE_GROUP masks go into one
    launch on the current stream.  What ``cfg.maskErode`` makes the burst pipeline do to every moved frame's mask."""
    single = isinstance(masks, torch.Tensor) and masks.dim() == 3
    ins = [masks] if single else list(masks)
    if not ins:
        raise ValueError("no masks")
    h, w = int(ins[0].shape[0]), int(ins[0].shape[1])

    def check(t, what):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (h, w, 4)
                and t.stride(2) == 1 and t.stride(1) == 4 and t.device == ins[0].device):
            raise ValueError(f"{what}: float32 device tensors [h, w, 4] of one size with dense cells expected")

    for t in ins:
        check(t, "masks")
    if out is None:
        res = torch.empty(len(ins), h, w, 4, dtype=torch.float32, device=ins[0].device)
        outs = list(res) if not single else [res[0]]
        ret = outs[0] if single else (res if isinstance(masks, torch.Tensor) else outs)
    else:
        outs = [out] if single else list(out)
        if len(outs) != len(ins):
            raise ValueError("out must have as many masks as the input")
        for t in outs:
            check(t, "out")
        ret = out
    in_pitch, out_pitch = ins[0].stride(0) * 4, outs[0].stride(0) * 4
    if any(t.stride(0) * 4 != in_pitch for t in ins) or any(t.stride(0) * 4 != out_pitch for t in outs):
        raise ValueError("all masks of a call share one row pitch")
    G = 4  # MFSR_MAX_FUSE_GROUP
    with torch.cuda.device(ins[0].device):
        for k0 in range(0, len(ins), G):
            n = min(G, len(ins) - k0)
            P = ctypes.c_void_p * n
            capi.lib().erodeMaskBatch(n, P(*[t.data_ptr() for t in ins[k0:k0 + n]]), P(*[t.data_ptr() for t in outs[k0:k0 + n]]),
                                      w, h, in_pitch, out_pitch, int(radius), torch.cuda.current_stream().cuda_stream)
    return ret


# ---- rendered output (include/mfsr.h, mfsr_render) --------------------------------------------------
def tone_lut_srgb(n: int = 4096) -> torch.Tensor:
    """The sRGB curve sampled at k/n, k = 0..n, in float64 and rounded to float32: a CPU tensor of n + 1 floats for
    ``set_render(tone_lut=...)``."""
    if not 1 <= n <= 65536:
        raise ValueError("1 <= n <= 65536")
    v = torch.arange(n + 1, dtype=torch.float64) / n
    return torch.where(v <= 0.0031308, 12.92 * v, 1.055 * v.clamp_min(1e-300) ** (1.0 / 2.4) - 0.055).to(torch.float32)


def render_row_bytes(fmt: int, width: int) -> int:
    """Bytes of a dense rendered row (mfsr_render_row_bytes); ValueError for an unknown format."""
    n = capi.lib().raw["mfsr_render_row_bytes"](int(fmt), int(width))
    if n < 0:
        raise ValueError(f"unknown output format {fmt} or width {width}")
    return n


def render_image_bytes(fmt: int, w: int, h: int) -> int:
    """Bytes of a dense rendered image (mfsr_render_image_bytes): rows of ``render_row_bytes``, h of them, or 3h/2 for the
    two-plane formats; ValueError for an unknown format or an extent the format does not take (NV12 / P010: even w and h)."""
    n = capi.lib().raw["mfsr_render_image_bytes"](int(fmt), int(w), int(h))
    if n < 0:
        raise ValueError(f"unknown output format {fmt} or extent {w} x {h}")
    return n


def yuv_planes(buf: torch.Tensor, fmt: int, h: int, w: int):
    """(Y [h, w], UV [h/2, w/2, 2]) views of the flat buffer of a two-plane output (``capi.OUT_NV12``: uint8, ``capi.OUT_P010``:
    int16 words holding code << 6), without a copy: the chroma plane follows the Y plane."""
    if fmt not in capi.YUV_FORMATS:
        raise ValueError(f"format {fmt} has one plane")
    if h % 2 or w % 2 or buf.dim() != 1 or buf.numel() != h * w * 3 // 2:
        raise ValueError("yuv_planes: a flat tensor of 3hw/2 elements, h and w even")
    return buf[:h * w].view(h, w), buf[h * w:].view(h // 2, w // 2, 2)


def _render_struct(fmt: int, matrix, tone_lut, device, yuv: int = 0):
    """(capi.Render, the device tensor of the table or None): the caller keeps the tensor alive as long as the struct is used.
    ``yuv``: the colour description of a two-plane format (``capi.YUV_BT709 | YUV_BT601 | YUV_BT2020``, ``| capi.YUV_FULL``)."""
    r = capi.Render()
    r.format = int(fmt)
    if yuv:
        if int(fmt) not in capi.YUV_FORMATS:
            raise ValueError("yuv: a colour description goes with OUT_NV12 / OUT_P010 only")
        r.reserved[0] = int(yuv)
    if matrix is not None:
        m = [float(v) for v in torch.as_tensor(matrix, dtype=torch.float64).reshape(-1).tolist()]
        if len(m) != 9:
            raise ValueError("matrix: 3 x 3 coefficients, row-major")
        r.useMatrix = 1
        r.matrix = (ctypes.c_float * 9)(*m)
    lut = None
    if tone_lut is not None:
        lut = torch.as_tensor(tone_lut).to(device=device, dtype=torch.float32).contiguous()
        if lut.dim() != 1 or not 2 <= lut.numel() <= 65537:
            raise ValueError("tone_lut: N + 1 floats, 1 <= N <= 65536")
        r.toneLut = lut.data_ptr()
        r.toneSize = lut.numel() - 1
    return r, lut


def _render_buffer(fmt: int, h: int, w: int, device) -> torch.Tensor:
    """The tensor typed for the format: int16 [h, w, 3], uint8 [h, w, 3], uint8 [h, w, 4] or int32 [h, w]; for the two-plane
    formats one flat tensor of 3hw/2 elements, uint8 (NV12) or int16 (P010): ``yuv_planes`` gives the planes."""
    if fmt in capi.YUV_FORMATS:
        if h % 2 or w % 2:
            raise ValueError(f"a two-plane YUV 4:2:0 output needs an even width and height, not {w} x {h}")
        return torch.empty(h * w * 3 // 2, dtype=torch.uint8 if fmt == capi.OUT_NV12 else torch.int16, device=device)
    if fmt == capi.OUT_RGB16:
        return torch.empty(h, w, 3, dtype=torch.int16, device=device)
    if fmt == capi.OUT_RGB8:
        return torch.empty(h, w, 3, dtype=torch.uint8, device=device)
    if fmt == capi.OUT_RGBA8:
        return torch.empty(h, w, 4, dtype=torch.uint8, device=device)
    if fmt == capi.OUT_RGB10A2:
        return torch.empty(h, w, dtype=torch.int32, device=device)
    raise ValueError(f"unknown output format {fmt}")


def render_image(img: torch.Tensor, format: int = capi.OUT_RGB16, matrix=None, tone_lut=None, apply_gamma: bool = False,
                 want_float: bool = False, yuv: int = 0):
    """Matrix, tone curve and quantisation of an existing float image [h, w, 3] on the device (mfsr_renderImage, or
    mfsr_renderImageYuv for ``capi.OUT_NV12`` / ``OUT_P010`` with the colour description ``yuv``): the pixel body of the
    rendered finish on its own.  Returns the tensor typed for the format (two planes: the flat tensor of ``yuv_planes``), and
    with ``want_float`` also the float image the integers quantise."""
    if not (img.is_cuda and img.dtype == torch.float32 and img.dim() == 3 and img.shape[2] == 3 and img.stride(2) == 1
            and img.stride(1) == 3):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    h, w = int(img.shape[0]), int(img.shape[1])
    with torch.cuda.device(img.device):
        r, lut = _render_struct(format, matrix, tone_lut, img.device, yuv)
        out = _render_buffer(format, h, w, img.device)
        fl = torch.empty(h, w, 3, dtype=torch.float32, device=img.device) if want_float else None
        if format in capi.YUV_FORMATS:
            rb = render_row_bytes(format, w)
            capi.lib().renderImageYuv(img.data_ptr(), img.stride(0) * 4, fl.data_ptr() if want_float else None, 12 * w, out.data_ptr(),
                                      rb, out.data_ptr() + rb * h, rb, w, h, ctypes.byref(r), 1 if apply_gamma else 0,
                                      torch.cuda.current_stream().cuda_stream)
            return (out, fl) if want_float else out
        capi.lib().renderImage(img.data_ptr(), img.stride(0) * 4, fl.data_ptr() if want_float else None, 12 * w, out.data_ptr(),
                               render_row_bytes(format, w), w, h, ctypes.byref(r), 1 if apply_gamma else 0,
                               torch.cuda.current_stream().cuda_stream)
        del lut  # (the launch is on the current stream: the caching allocator keeps the table until the stream has passed it)
    return (out, fl) if want_float else out


# ---- sharpening inside the finish (include/mfsr.h, mfsr_sharpen) ----------------------------------------
def sharpen_gaussian(sigma: float = 1.0, radius: int = 0, amount: float = 1.0, threshold: float = 0.0) -> capi.Sharpen:
    """A sharpen description with Gaussian taps (mfsr_sharpen_gaussian; host arithmetic, no device): radius 0 chooses
    min(4, max(1, ceil(2.5 sigma)))."""
    s = capi.Sharpen()
    if capi.lib().raw["mfsr_sharpen_gaussian"](float(sigma), int(radius), float(amount), float(threshold), ctypes.byref(s)) != 0:
        raise ValueError("sharpen: sigma > 0, 0 <= radius <= 4, 0 <= amount <= 16, threshold >= 0, all finite")
    return s


def _sharpen_struct(amount, sigma=1.0, radius=0, threshold=0.0, taps=None) -> Optional[capi.Sharpen]:
    """The description of ``BurstPipeline.set_sharpen``'s arguments; None = off."""
    if amount is None:
        return None
    if taps is None:
        return sharpen_gaussian(sigma, radius, amount, threshold)
    k = [float(v) for v in taps]
    if not 1 <= len(k) <= 5:
        raise ValueError("taps: k[0] (centre), k[1..R], R <= 4")
    s = capi.Sharpen()
    s.radius = int(radius) if radius else len(k) - 1
    if s.radius > len(k) - 1:
        raise ValueError("taps: radius + 1 coefficients are needed")
    s.taps = (ctypes.c_float * 5)(*(k + [0.0] * (5 - len(k))))
    s.amount, s.threshold = float(amount), float(threshold)
    if capi.lib().raw["mfsr_sharpen_validate"](ctypes.byref(s)) != 0:
        raise ValueError("sharpen: |taps| <= 4, 0 <= amount <= 16, threshold >= 0, all finite")
    return s


def sharpen_image(img: torch.Tensor, amount: float = 1.0, sigma: float = 1.0, radius: int = 0, threshold: float = 0.0, taps=None,
                  format: Optional[int] = None, matrix=None, tone_lut=None, apply_gamma: bool = False, want_float: bool = True):
    """The unsharp mask of a sharpened finish on an existing linear float image [h, w, 3] on the device (mfsr_sharpenImage),
    followed by the steps of ``render_image`` when ``format`` is given.  Returns the float image, or with ``format`` the tensor
    typed for it (and with ``want_float`` the pair (integers, float image))."""
    if not (img.is_cuda and img.dtype == torch.float32 and img.dim() == 3 and img.shape[2] == 3 and img.stride(2) == 1
            and img.stride(1) == 3):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    s = _sharpen_struct(amount, sigma, radius, threshold, taps)
    if s is None or s.radius == 0 or s.amount == 0:
        raise ValueError("sharpen_image: amount and radius must not be 0")
    h, w = int(img.shape[0]), int(img.shape[1])
    with torch.cuda.device(img.device):
        r, lut, out = None, None, None
        if format is not None:
            r, lut = _render_struct(format, matrix, tone_lut, img.device)
            out = _render_buffer(format, h, w, img.device)
        fl = torch.empty(h, w, 3, dtype=torch.float32, device=img.device) if (want_float or out is None) else None
        capi.lib().sharpenImage(img.data_ptr(), img.stride(0) * 4, None if fl is None else fl.data_ptr(), 12 * w,
                                None if out is None else out.data_ptr(), 0 if out is None else render_row_bytes(format, w), w, h,
                                ctypes.byref(s), None if r is None else ctypes.byref(r), 1 if apply_gamma else 0,
                                torch.cuda.current_stream().cuda_stream)
        del lut
    if out is None:
        return fl
    return (out, fl) if want_float else out


# ---- merge-aware denoise inside the finish (include/mfsr.h, mfsr_denoise) -----------------------------
def denoise_defaults(alpha: float = 0.0, beta: float = 0.0) -> capi.Denoise:
    """The default denoise description (mfsr_denoise_defaults; host arithmetic, no device): radius 2, strength 3, gain 2, no
    fade, and the noise model alpha, beta of one raw sample (``cfg.alpha`` / ``cfg.beta``)."""
    d = capi.Denoise()
    if capi.lib().raw["mfsr_denoise_defaults"](float(alpha), float(beta), ctypes.byref(d)) != 0:
        raise ValueError("denoise: alpha and beta in [0, 1], finite")
    return d


def _denoise_struct(strength, radius=2, gain=2.0, alpha=0.0, beta=0.0, fade=None) -> Optional[capi.Denoise]:
    """The description of ``BurstPipeline.set_denoise``'s arguments; None = off.  fade = (w_lo, w_hi) or None."""
    if strength is None:
        return None
    d = capi.Denoise()
    d.radius, d.strength, d.gain, d.alpha, d.beta = int(radius), float(strength), float(gain), float(alpha), float(beta)
    if fade is not None:
        d.wLo, d.wHi = float(fade[0]), float(fade[1])
    if capi.lib().raw["mfsr_denoise_validate"](ctypes.byref(d)) != 0:
        raise ValueError("denoise: radius 0..3, strength 0 or 1/16..16, 0 < gain <= 1024, alpha and beta in [0, 1], "
                         "fade = (w_lo >= 0, w_hi) with w_hi <= w_lo or w_hi - w_lo >= 2^-10, all finite")
    return d


def denoise_image(img: torch.Tensor, count: Optional[torch.Tensor] = None, strength: float = 3.0, radius: int = 2, gain: float = 2.0,
                  alpha: float = 0.0, beta: float = 0.0, fade=None, format: Optional[int] = None, matrix=None, tone_lut=None,
                  apply_gamma: bool = False, want_float: bool = True):
    """The range filter of a denoised finish on an existing linear float image [h, w, 3] on the device (mfsr_denoiseImage),
    followed by the steps of ``render_image`` when ``format`` is given.  ``count``: a float image [h, w, 3] of how many samples
    each value averaged (the tolerance is gain * (alpha * p + beta) / count), or None for one everywhere, the single-frame
    case.  Returns the float image, or with ``format`` the tensor typed for it (and with ``want_float`` the pair (integers,
    float image))."""
    def dense(t):
        return t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[2] == 3 and t.stride(2) == 1 and t.stride(1) == 3
    if not dense(img):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    if count is not None and not (dense(count) and count.shape == img.shape and count.device == img.device):
        raise ValueError("count: a float32 device tensor of img's shape with dense pixels")
    d = _denoise_struct(strength, radius, gain, alpha, beta, fade)
    if d is None or d.radius == 0 or d.strength == 0:
        raise ValueError("denoise_image: strength and radius must not be 0")
    h, w = int(img.shape[0]), int(img.shape[1])
    with torch.cuda.device(img.device):
        r, lut, out = None, None, None
        if format is not None:
            r, lut = _render_struct(format, matrix, tone_lut, img.device)
            out = _render_buffer(format, h, w, img.device)
        fl = torch.empty(h, w, 3, dtype=torch.float32, device=img.device) if (want_float or out is None) else None
        capi.lib().denoiseImage(img.data_ptr(), img.stride(0) * 4, None if count is None else count.data_ptr(),
                                0 if count is None else count.stride(0) * 4, None if fl is None else fl.data_ptr(), 12 * w,
                                None if out is None else out.data_ptr(), 0 if out is None else render_row_bytes(format, w), w, h,
                                ctypes.byref(d), None if r is None else ctypes.byref(r), 1 if apply_gamma else 0,
                                torch.cuda.current_stream().cuda_stream)
        del lut
    if out is None:
        return fl
    return (out, fl) if want_float else out


# ---- image statistics, auto white balance, auto tone (include/mfsr.h, mfsr_imageStats) ---------------
ToneFit = namedtuple("ToneFit", "lut black white gamma status")


def auto_defaults(pixels: int = 0) -> capi.AutoParams:
    """The defaults of auto white balance and auto tone (mfsr_auto_defaults; host only): neutral set lo 64, hi 3967, chromaTol
    64, 2 passes, minCount = pixels / 64 (0: decided from the pixels measured), pLo 0.001, pHi 0.999, maxGain 8, mid 0.18, a
    table of 4096 intervals."""
    ap = capi.AutoParams()
    capi.lib().auto_defaults(int(pixels), ctypes.byref(ap))
    return ap


def _stats_params(matrix, lo, hi, chroma_tol) -> capi.ImageStatsParams:
    p = capi.ImageStatsParams()
    p.lo, p.hi, p.chromaTol = int(lo), int(hi), int(chroma_tol)
    if matrix is not None:
        m = [float(v) for v in torch.as_tensor(matrix, dtype=torch.float64).reshape(-1).tolist()]
        if len(m) != 9:
            raise ValueError("matrix: 3 x 3 coefficients, row-major")
        p.useMatrix = 1
        p.matrix = (ctypes.c_float * 9)(*m)
    return p


def image_stats(img: torch.Tensor, matrix=None, lo: int = 64, hi: int = 3967, chroma_tol: int = 0) -> torch.Tensor:
    """The statistics table of a float image [h, w, 3] on the device (mfsr_imageStats), exact: a CPU int64 tensor of
    ``capi.IMAGE_STATS_WORDS`` words -- pixels, neutral pixels, the three code sums over the neutral set and over all pixels, the
    histogram of the luma key and the histogram of the channel maximum, of the 12-bit codes of the pixel after ``matrix`` (None:
    the pixel itself).  Rows may be pitched; the image is only read."""
    if not (img.is_cuda and img.dtype == torch.float32 and img.dim() == 3 and img.shape[2] == 3 and img.stride(2) == 1
            and img.stride(1) == 3):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    h, w = int(img.shape[0]), int(img.shape[1])
    p = _stats_params(matrix, lo, hi, chroma_tol)
    with torch.cuda.device(img.device):
        table = torch.zeros(capi.IMAGE_STATS_WORDS, dtype=torch.int64, device=img.device)
        capi.lib().imageStats(img.data_ptr(), img.stride(0) * 4, w, h, ctypes.byref(p), table.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
        return table.cpu()


def _stats_host(stats):
    import numpy as np
    a = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    a = np.ascontiguousarray(a.astype(np.uint64, copy=False) if a.dtype != np.int64 else a.view(np.uint64))
    if a.shape != (capi.IMAGE_STATS_WORDS,):
        raise ValueError(f"stats: the table of image_stats, {capi.IMAGE_STATS_WORDS} words")
    return a


def awb_gains(stats, min_count: Optional[int] = None):
    """((g_r, 1, g_b), status) of mfsr_awb_gains on a table of ``image_stats``: grey-world gains over the neutral set.  status 0
    ok, 1 unmeasurable (gains 1, 1, 1), 2 clamped to [1/8, 8].  min_count None = 1/64 of the pixels measured.  Host only."""
    a = _stats_host(stats)
    g, st = (ctypes.c_float * 3)(), ctypes.c_int32()
    capi.lib().awb_gains(a.ctypes.data, int(a[0]) // 64 if min_count is None else int(min_count), g, ctypes.byref(st))
    return tuple(g), st.value


def tone_fit(stats, p_lo: float = 0.001, p_hi: float = 0.999, max_gain: float = 8.0, mid: float = 0.18,
             tone_size: int = 4096) -> ToneFit:
    """Black point, white point, mid-tone gamma and the tone table of them (mfsr_tone_fit) from a table of ``image_stats``:
    ``ToneFit(lut, black, white, gamma, status)`` with ``lut`` a CPU float32 tensor of tone_size + 1 floats for
    ``set_render(tone_lut=...)``.  status 1: the span was floored at 1 / max_gain.  Host only."""
    import numpy as np
    a = _stats_host(stats)
    tp = capi.ToneParams(float(p_lo), float(p_hi), float(max_gain), float(mid))
    lut = np.empty(int(tone_size) + 1, np.float32)
    b, w, g, st = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int32()
    capi.lib().tone_fit(a.ctypes.data, ctypes.byref(tp), int(tone_size), lut.ctypes.data, ctypes.byref(b), ctypes.byref(w),
                        ctypes.byref(g), ctypes.byref(st))
    return ToneFit(torch.from_numpy(lut), b.value, w.value, g.value, st.value)


# ---- local tone mapping in the finish (include/mfsr.h, mfsr_local_tone) ------------------------------
LocalToneFit = namedtuple("LocalToneFit", "grid pivot status")


def local_tone_defaults(w: int, h: int) -> capi.LocalTone:
    """The default description for a w x h frame (mfsr_local_tone_defaults; host only): cell = the smallest power of two >= 16
    with at most 128 cells along the longer side, 16 bins, one smoothing pass, shadows 0.5, highlights 0.25, a measured pivot,
    gains within [1/4, 4]."""
    lt = capi.LocalTone()
    if capi.lib().raw["mfsr_local_tone_defaults"](int(w), int(h), ctypes.byref(lt)) != 0:
        raise ValueError("local_tone_defaults: 1 <= w, h <= 65536")
    return lt


def _local_tone_struct(w, h, shadows, highlights, cell=None, bins=16, smooth=1, pivot=0.0, max_gain=4.0) -> capi.LocalTone:
    lt = local_tone_defaults(w, h)
    lt.shadows, lt.highlights, lt.pivot, lt.maxGain = float(shadows), float(highlights), float(pivot), float(max_gain)
    lt.bins, lt.smooth = int(bins), int(smooth)
    if cell is not None:
        lt.cell = int(cell)
    if capi.lib().raw["mfsr_local_tone_validate"](ctypes.byref(lt)) != 0:
        raise ValueError("local tone: cell a power of two 16..512, bins 4, 8, 16 or 32, smooth 0..4, shadows and highlights "
                         "in [0, 1], pivot in [0, 1], max_gain in [1, 64], all finite")
    return lt


def local_tone_grid(full_w: int, full_h: int, lt: capi.LocalTone) -> Tuple[int, int, int]:
    """(GX, GY, GZ) of the grid of a full_w x full_h frame (mfsr_local_tone_grid): the statistics table has 2 GX GY GZ words and
    the gain grid GX GY GZ floats, luma fastest, then x, then y."""
    gx, gy, gz = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if capi.lib().raw["mfsr_local_tone_grid"](int(full_w), int(full_h), ctypes.byref(lt), ctypes.byref(gx), ctypes.byref(gy),
                                              ctypes.byref(gz)) != 0:
        raise ValueError("local_tone_grid: a positive extent and a valid description")
    return gx.value, gy.value, gz.value


def _dense_f3(img: torch.Tensor) -> bool:
    return (img.is_cuda and img.dtype == torch.float32 and img.dim() == 3 and img.shape[2] == 3 and img.stride(2) == 1
            and img.stride(1) == 3)


def _matrix9(matrix):
    if matrix is None:
        return None
    m = [float(v) for v in torch.as_tensor(matrix, dtype=torch.float64).reshape(-1).tolist()]
    if len(m) != 9:
        raise ValueError("matrix: 3 x 3 coefficients, row-major")
    return (ctypes.c_float * 9)(*m)


def tone_grid_stats(img: torch.Tensor, lt: capi.LocalTone, matrix=None, offset=(0, 0), full=None,
                    table: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The statistics of the bilateral grid of a float image [h, w, 3] on the device (mfsr_toneGridStats), exact: a device int64
    tensor [GY, GX, GZ, 2] of (count, sum of the luma key) per grid entry.  ``offset`` = (x, y) of the image's first pixel in
    the ``full`` = (w, h) frame the grid belongs to (default: the image is the frame).  ``table``: add to this table instead of
    a zeroed one (stripes and windows add up to the whole)."""
    if not _dense_f3(img):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    h, w = int(img.shape[0]), int(img.shape[1])
    fw, fh = (w, h) if full is None else (int(full[0]), int(full[1]))
    gx, gy, gz = local_tone_grid(fw, fh, lt)
    with torch.cuda.device(img.device):
        if table is None:
            table = torch.zeros(gy, gx, gz, 2, dtype=torch.int64, device=img.device)
        elif table.shape != (gy, gx, gz, 2) or table.dtype != torch.int64 or not table.is_contiguous():
            raise ValueError(f"table: a contiguous int64 tensor [{gy}, {gx}, {gz}, 2]")
        capi.lib().toneGridStats(img.data_ptr(), img.stride(0) * 4, w, h, int(offset[0]), int(offset[1]), fw, fh, _matrix9(matrix),
                                 ctypes.byref(lt), table.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return table


def local_tone_fit(stats, full_w: int, full_h: int, lt: capi.LocalTone) -> LocalToneFit:
    """The gains of a table of ``tone_grid_stats`` (mfsr_local_tone_fit; host only): ``LocalToneFit(grid, pivot, status)`` with
    ``grid`` a CPU float32 tensor [GY, GX, GZ].  status 1: the table was empty (pivot 0.18)."""
    import numpy as np
    gx, gy, gz = local_tone_grid(full_w, full_h, lt)
    a = stats.cpu().numpy() if isinstance(stats, torch.Tensor) else np.asarray(stats)
    a = np.ascontiguousarray(a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64, copy=False)).reshape(-1)
    if a.size != 2 * gx * gy * gz:
        raise ValueError(f"stats: the table of tone_grid_stats, {2 * gx * gy * gz} words")
    grid = np.empty((gy, gx, gz), np.float32)
    pivot, st = ctypes.c_double(), ctypes.c_int32()
    capi.lib().local_tone_fit(a.ctypes.data, int(full_w), int(full_h), ctypes.byref(lt), grid.ctypes.data, ctypes.byref(pivot),
                              ctypes.byref(st))
    return LocalToneFit(torch.from_numpy(grid), pivot.value, st.value)


def local_tone_image(img: torch.Tensor, grid: torch.Tensor, lt: capi.LocalTone, format: int = capi.OUT_RGB16, matrix=None,
                     tone_lut=None, apply_gamma: bool = False, want_float: bool = False, offset=(0, 0), full=None):
    """``render_image`` with the gain of the bilateral ``grid`` ([GY, GX, GZ] floats, device or host) applied to every pixel
    before the matrix (mfsr_localToneImage).  ``offset`` / ``full`` as for ``tone_grid_stats``.  Returns the tensor typed for
    the format, and with ``want_float`` also the float image the integers quantise."""
    if not _dense_f3(img):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    if format in capi.YUV_FORMATS:
        raise ValueError("local_tone_image: single-plane formats only")
    h, w = int(img.shape[0]), int(img.shape[1])
    fw, fh = (w, h) if full is None else (int(full[0]), int(full[1]))
    gx, gy, gz = local_tone_grid(fw, fh, lt)
    with torch.cuda.device(img.device):
        g = torch.as_tensor(grid).to(device=img.device, dtype=torch.float32).contiguous()
        if g.numel() != gx * gy * gz:
            raise ValueError(f"grid: {gy} x {gx} x {gz} floats")
        r, lut = _render_struct(format, matrix, tone_lut, img.device)
        out = _render_buffer(format, h, w, img.device)
        fl = torch.empty(h, w, 3, dtype=torch.float32, device=img.device) if want_float else None
        capi.lib().localToneImage(img.data_ptr(), img.stride(0) * 4, fl.data_ptr() if want_float else None, 12 * w, out.data_ptr(),
                                  render_row_bytes(format, w), w, h, ctypes.byref(r), 1 if apply_gamma else 0, g.data_ptr(),
                                  ctypes.byref(lt), int(offset[0]), int(offset[1]), fw, fh, torch.cuda.current_stream().cuda_stream)
        del lut, g
    return (out, fl) if want_float else out


# ---- the finish chain (include/mfsr.h, mfsr_finish_chain) --------------------------------------------
def _chain_struct(full_w: int, full_h: int, denoise: Optional[dict], sharpen: Optional[dict], local_tone, device,
                  alpha: float = 0.0, beta: float = 0.0):
    """(capi.FinishChain or None when every stage is off, the device tensor of the grid or None, reach) of the arguments of
    ``BurstPipeline.set_finish_chain``.  The stages that are off hold valid descriptions that are off (a zero radius)."""
    c = capi.FinishChain()
    den = None
    if denoise is not None:
        kw = dict(denoise)
        kw["alpha"] = alpha if kw.get("alpha") is None else kw["alpha"]
        kw["beta"] = beta if kw.get("beta") is None else kw["beta"]
        den = _denoise_struct(**kw)
    if den is None:
        den = denoise_defaults(0.0, 0.0)
        den.radius = 0
    c.denoise = den
    sh = None if sharpen is None else _sharpen_struct(**sharpen)
    if sh is not None:
        c.sharpen = sh
    grid = None
    if local_tone is not None:
        lt, g = local_tone
        gx, gy, gz = local_tone_grid(full_w, full_h, lt)
        grid = torch.as_tensor(g).to(device=device, dtype=torch.float32).contiguous()
        if grid.numel() != gx * gy * gz:
            raise ValueError(f"local_tone: a grid of {gy} x {gx} x {gz} floats")
        c.localTone, c.useLocalTone = lt, 1
    else:
        c.localTone = local_tone_defaults(full_w, full_h)
    reach = ctypes.c_int(-1)
    if capi.lib().raw["mfsr_finish_chain_reach"](ctypes.byref(c), ctypes.byref(reach)) != 0:
        raise ValueError("finish chain: an invalid denoise, sharpen or local-tone description")
    if reach.value == 0 and grid is None:
        return None, None, 0
    return c, grid, reach.value


def finish_chain_image(img: torch.Tensor, count: Optional[torch.Tensor] = None, denoise: Optional[dict] = None,
                       sharpen: Optional[dict] = None, local_tone=None, format: Optional[int] = None, matrix=None, tone_lut=None,
                       apply_gamma: bool = False, want_float: bool = True, yuv: int = 0, offset=(0, 0), full=None):
    """The finish chain on an existing linear float image [h, w, 3] on the device (mfsr_chainImage): denoise, then sharpen, then
    the local-tone gain, then the steps of ``render_image`` when ``format`` is given (any format, ``capi.OUT_NV12`` /
    ``OUT_P010`` with the colour description ``yuv`` included), in one launch.  ``denoise`` / ``sharpen``: dicts of the keyword
    arguments of ``denoise_image`` / ``sharpen_image``'s descriptions (strength, radius, gain, alpha, beta, fade; amount, sigma,
    radius, threshold, taps); ``local_tone``: a ``(capi.LocalTone, grid)`` pair; None = that stage is off, and one stage at
    least must be on.  ``count`` as for ``denoise_image``.  ``offset`` / ``full`` as for ``local_tone_image``.  Returns the float
    image, or with ``format`` the tensor typed for it (and with ``want_float`` the pair (integers, float image))."""
    if not _dense_f3(img):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    if count is not None and not (_dense_f3(count) and count.shape == img.shape and count.device == img.device):
        raise ValueError("count: a float32 device tensor of img's shape with dense pixels")
    h, w = int(img.shape[0]), int(img.shape[1])
    fw, fh = (w, h) if full is None else (int(full[0]), int(full[1]))
    with torch.cuda.device(img.device):
        c, grid, _ = _chain_struct(fw, fh, denoise, sharpen, local_tone, img.device)
        if c is None:
            raise ValueError("finish_chain_image: one stage at least must be on")
        r, lut, out = None, None, None
        if format is not None:
            r, lut = _render_struct(format, matrix, tone_lut, img.device, yuv)
            out = _render_buffer(format, h, w, img.device)
        two = format in capi.YUV_FORMATS
        fl = torch.empty(h, w, 3, dtype=torch.float32, device=img.device) if (want_float or out is None) else None
        rb = 0 if out is None else render_row_bytes(format, w)
        capi.lib().chainImage(img.data_ptr(), img.stride(0) * 4, None if count is None else count.data_ptr(),
                              0 if count is None else count.stride(0) * 4, None if fl is None else fl.data_ptr(), 12 * w,
                              None if out is None else out.data_ptr(), rb, out.data_ptr() + rb * h if two else None, rb if two else 0,
                              w, h, None if r is None else ctypes.byref(r), 1 if apply_gamma else 0, ctypes.byref(c),
                              None if grid is None else grid.data_ptr(), int(offset[0]), int(offset[1]), fw, fh,
                              torch.cuda.current_stream().cuda_stream)
        del lut, grid
    if out is None:
        return fl
    return (out, fl) if want_float else out


# ---- the geometric finish (include/mfsr.h, mfsr_geometry) --------------------------------------------
_GEO_FILTERS = {"bilinear": capi.GEO_BILINEAR, "cubic": capi.GEO_CUBIC}


def lens_geometry(src_w: int, src_h: int, out_w: int, out_h: int, zoom: float = 1.0, distortion=(0, 0, 0), lateral=(1, 1),
                  filter: str = "cubic") -> capi.Geometry:
    """The description of a geometric finish from a lens profile (mfsr_geometry_lens; host arithmetic in double, rounded once):
    an ``out_w`` x ``out_h`` output of a ``src_w`` x ``src_h`` source around the two image centres, step = min(src_w / out_w,
    src_h / out_h) / ``zoom``, ``distortion`` = (k1, k2, k3) of the forward radial model in r^2 normalised by the source's half
    diagonal, ``lateral`` = the magnifications of red and blue against green, ``filter`` = "bilinear" or "cubic" (Catmull-Rom)."""
    if filter not in _GEO_FILTERS:
        raise ValueError('filter: "bilinear" or "cubic"')
    k = [float(v) for v in distortion]
    lat = [float(v) for v in lateral]
    if len(k) != 3 or len(lat) != 2:
        raise ValueError("distortion: (k1, k2, k3); lateral: (red, blue)")
    g = capi.Geometry()
    if capi.lib().raw["mfsr_geometry_lens"](int(src_w), int(src_h), int(out_w), int(out_h), float(zoom), (ctypes.c_double * 3)(*k),
                                            (ctypes.c_double * 2)(*lat), _GEO_FILTERS[filter], ctypes.byref(g)) != 0:
        raise ValueError("lens_geometry: extents 1 .. 32768, step in [1/8, 8], |lateral - 1| <= 0.25, |k| <= 4, all finite")
    return g


def geometry_image(img: torch.Tensor, geometry: capi.Geometry, format: Optional[int] = None, matrix=None, tone_lut=None, rect=None,
                   apply_gamma: bool = False, want_float: bool = True):
    """The geometric finish on an existing linear float image [h, w, 3] on the device (mfsr_geometryImage): resample by
    ``geometry`` (``lens_geometry``), then the steps of ``render_image`` when ``format`` is given (single-plane formats).
    ``rect`` = (x, y, w, h): that rectangle of the geometry's output only (None: all of it), bit for bit the crop.  Returns the
    float image, or with ``format`` the tensor typed for it (and with ``want_float`` the pair (integers, float image)).  This is
    how the other stages combine with it: ``finish_chain_image`` (or a burst's float image) first, then this."""
    if not _dense_f3(img):
        raise ValueError("img: a float32 device tensor [h, w, 3] with dense pixels")
    src_h, src_w = int(img.shape[0]), int(img.shape[1])
    x, y, w, h = (0, 0, geometry.outW, geometry.outH) if rect is None else (int(v) for v in rect)
    with torch.cuda.device(img.device):
        r, lut, out = None, None, None
        if format is not None:
            r, lut = _render_struct(format, matrix, tone_lut, img.device)
            out = _render_buffer(format, h, w, img.device)
        fl = torch.empty(h, w, 3, dtype=torch.float32, device=img.device) if (want_float or out is None) else None
        capi.lib().geometryImage(img.data_ptr(), img.stride(0) * 4, src_w, src_h, None if fl is None else fl.data_ptr(), 12 * w,
                                 None if out is None else out.data_ptr(), 0 if out is None else render_row_bytes(format, w),
                                 None if r is None else ctypes.byref(r), ctypes.byref(geometry), 1 if apply_gamma else 0, x, y, w, h,
                                 torch.cuda.current_stream().cuda_stream)
        del lut
    if out is None:
        return fl
    return (out, fl) if want_float else out


class BurstPipeline:
    """One burst context on one device (ctx-per-device, not thread-safe; the
    reference is single-device/single-stream, kernel.cu:45)."""

    def __init__(self, cfg: capi.Config, device: Optional[torch.device] = None, window: Optional[Sequence[int]] = None):
        """window = (x, y, w, h): super-resolve only that rectangle of the HR output (a zoom).  Any rectangle: the library
        works on the 16-pixel-aligned window around it (``align_window``; ``img_out`` / ``total_weights`` are that size) and
        ``finish`` / ``process`` / ``process_host`` return exactly the rectangle asked for, bit for bit the same pixels as
        the whole-frame burst.  Needs cfg.fused = 1."""
        if not torch.cuda.is_available():
            raise RuntimeError("multi_frame_super_resolution_amd needs a HIP device (MI355X); there is no CPU fallback")
        self.L = capi.lib()
        self.cfg = cfg
        self.window = _Window(cfg, window)
        self._sharpen_on = self._denoise_on = False   # a stencil in the finish (set_sharpen, set_denoise) grows the window
        self._chain_reach = 0           # ... and so does a chain with a stencil stage (set_finish_chain)
        self._chain = self._chain_grid = None
        self._local_tone = None         # the description of set_local_tone; its grid and table live as long as it is installed
        self.local_tone_result = None   # capi.LocalToneResult of the last measurement
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        nbytes = self.L.burst_workspace_bytes(ctypes.byref(cfg))
        if nbytes == 0:
            raise ValueError("invalid mfsr_config")
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            base = self.workspace.data_ptr()
            self._ws_ptr = (base + 255) // 256 * 256
            self.hr_w, self.hr_h = cfg.width * cfg.scale, cfg.height * cfg.scale
            # accumulators: float3 HR (the window's size when one is set), pitch 12*width (caller-owned, RMW across
            # frames, reference DeBayerKernels.cu:306-307,374-375)
            out_h, out_w = self.window.aligned[3], self.window.aligned[2]
            self._img_out = torch.zeros(out_h, out_w, 3, dtype=torch.float32, device=self.device)
            self._total_weights = torch.zeros_like(self._img_out)
            self.out_img = torch.empty_like(self._img_out)
            self.out16 = torch.empty(out_h, out_w, 3, dtype=torch.int16, device=self.device)
            self._fmt = capi.OUT_RGB16   # the format of out16 (set_render)
            handle = ctypes.c_void_p()
            self.L.burst_create(ctypes.byref(handle), ctypes.byref(cfg), self._ws_ptr, nbytes)
            self._h = handle
            self.window.apply(self.L.burst_set_window, self._h)
        self._hold = None        # mfsr_burst_hold_fuse is on for this context (None: not decided, begin_burst applies HOLD_FUSE)
        self._held_frames = []   # ... and these frame tensors wait for the burst launch: referenced until flush / finish

    def close(self):
        if getattr(self, "_h", None):
            self.L.burst_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream() -> int:
        return torch.cuda.current_stream().cuda_stream

    def set_render(self, format: Optional[int] = capi.OUT_RGB16, matrix=None, tone_lut=None, yuv: int = 0):
        """Render the output inside the finish (mfsr_burst_set_render): ``matrix`` = 3 x 3 colour matrix
        (row-major, display = matrix * camera), ``tone_lut`` = N + 1 floats of a tone curve sampled at k/N (``tone_lut_srgb``;
        without one cfg.applyGamma decides), ``format`` = ``capi.OUT_*``.  ``finish`` and ``process*`` then return the integer
        image as a tensor typed for the format: int16 [h, w, 3], uint8 [h, w, 3], uint8 [h, w, 4] or int32 [h, w]; the float
        image is the rendered one.  ``format=None`` turns rendering off.  Between bursts only.
        ``capi.OUT_NV12`` / ``OUT_P010``: two-plane YUV 4:2:0 with the colour description ``yuv``
        (``capi.YUV_BT709 | YUV_BT601 | YUV_BT2020``, ``| capi.YUV_FULL``; 0 = BT.709 limited range); the integer image is one
        flat tensor, uint8 or int16, of which ``yuv_planes`` gives the Y and the (Cb, Cr) plane.  A zoom window must then have
        even x, y, w and h (ValueError), and sharpening cannot be on."""
        if format is not None:
            self.window.check_yuv(int(format))
        out_h, out_w = self.window.aligned[3], self.window.aligned[2]
        with torch.cuda.device(self.device):
            if format is None:
                self.L.burst_set_render(self._h, None)
                self._render_lut, fmt = None, capi.OUT_RGB16
            else:
                r, lut = _render_struct(format, matrix, tone_lut, self.device, yuv)
                self.L.burst_set_render(self._h, ctypes.byref(r))
                self._render_lut, fmt = lut, int(format)   # the table is the caller's memory: alive as long as the description
            self.out16 = _render_buffer(fmt, out_h, out_w, self.device)
            self._out16_host = None
            self._fmt = fmt

    _AUTO_KEYS = {"lo": "lo", "hi": "hi", "chroma_tol": "chromaTol", "iterations": "iterations", "min_count": "minCount",
                  "tone_size": "toneSize"}
    _TONE_KEYS = {"p_lo": "pLo", "p_hi": "pHi", "max_gain": "maxGain", "mid": "mid"}

    def auto_render(self, format: int = capi.OUT_RGB8, matrix=None, awb: bool = True, tone: bool = True, yuv: int = 0,
                    tone_lut=None, **params) -> capi.AutoResult:
        """Measure the burst and render by the measurement (mfsr_burst_auto_render): after the last
        ``add_frame`` and before ``finish``.  ``awb``: white-balance gains from the near-grey pixels of the merged image go into
        the colour matrix (``matrix`` times diag(gains), or diag(gains)).  ``tone``: black point, white point and a mid-tone
        gamma from the image's histograms become the tone table.  With both off this is ``set_render(format, matrix, tone_lut,
        yuv)``; ``tone_lut`` is used only when ``tone`` is off.  ``params``: lo, hi, chroma_tol, iterations, min_count, p_lo,
        p_hi, max_gain, mid, tone_size (``auto_defaults``).  The statistics are those of the output, or of the aligned zoom window.
        ``finish`` then returns the integer image typed for ``format`` as after ``set_render``; the description stays installed
        until ``set_render`` changes it.  Returns the ``capi.AutoResult``; the installed description is ``self.auto_description``
        (a ``capi.Render``) and the table behind it ``self.auto_lut`` (a device tensor or None)."""
        self.window.check_yuv(int(format))
        out_h, out_w = self.window.aligned[3], self.window.aligned[2]
        ap = auto_defaults(out_h * out_w)
        ap.awb, ap.tone = int(bool(awb)), int(bool(tone))
        for k, v in params.items():
            if k in self._AUTO_KEYS:
                setattr(ap, self._AUTO_KEYS[k], int(v))
            elif k in self._TONE_KEYS:
                setattr(ap.toneParams, self._TONE_KEYS[k], float(v))
            else:
                raise TypeError(f"auto_render: unknown parameter {k!r}")
        if not 1 <= ap.toneSize <= 65536:
            raise ValueError("tone_size: 1 .. 65536")
        res = capi.AutoResult()
        with torch.cuda.device(self.device):
            r, lut = _render_struct(format, matrix, None if tone else tone_lut, self.device, yuv)
            table = torch.empty(capi.IMAGE_STATS_WORDS, dtype=torch.int64, device=self.device)
            if tone:
                lut = torch.empty(ap.toneSize + 1, dtype=torch.float32, device=self.device)
            self.L.burst_auto_render(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(), ctypes.byref(ap),
                                     table.data_ptr(), lut.data_ptr() if tone else None, ctypes.byref(r), ctypes.byref(res),
                                     self._stream())
            self._held_frames.clear()
            # the table is the caller's memory: alive as long as the description; the statistics table with it
            self._render_lut, self._auto_table = lut, table
            self.auto_description, self.auto_lut = r, lut
            self.out16 = _render_buffer(int(format), out_h, out_w, self.device)
            self._out16_host = None
            self._fmt = int(format)
        return res

    def process_auto(self, frames: Sequence[torch.Tensor], frame_ids: Optional[Iterable[int]] = None, **auto):
        """Whole burst on this device, rendered by its own measurement: reference products, every frame, ``auto_render(**auto)``,
        finish.  Returns (float image, integer image) like ``process`` after ``set_render``; the outcome of the measurement is
        left in ``self.auto_result`` (a ``capi.AutoResult``)."""
        r = self.cfg.reference
        self.begin_burst()
        self.set_reference(frames[r])
        for k in (range(len(frames)) if frame_ids is None else frame_ids):
            self.add_frame(frames[k], k == r)
        self.auto_result = self.auto_render(**auto)
        if self._local_tone is not None:     # measured with the matrix auto_render has just installed
            self.local_tone()
        return self.finish()

    def set_local_tone(self, shadows: Optional[float] = 0.5, highlights: float = 0.25, cell: Optional[int] = None, bins: int = 16,
                       smooth: int = 1, pivot: float = 0.0, max_gain: float = 4.0):
        """Local tone mapping inside the finish (mfsr_burst_set_local_tone): a gain per pixel from a
        bilateral grid over (x, y, luma) of the merged image, applied before the colour matrix, the same for the three
        channels.  Regions darker than the ``pivot`` (0 = the image's log-average luma) are lifted by (B / pivot)^-shadows,
        brighter ones lowered by (B / pivot)^-highlights, B the mean luma of the grid cell and luma bin around the pixel;
        gains stay within [1 / max_gain, max_gain].  ``cell`` = HR pixels per grid cell (None: chosen from the frame),
        ``bins`` luma bins, ``smooth`` blur passes over the grid.  ``shadows=None`` turns it off.  Between bursts only; not
        together with ``set_sharpen`` / ``set_denoise`` or a two-plane format.  ``process`` and ``process_auto`` then measure the
        burst before they finish it (``local_tone``; the outcome is ``self.local_tone_result``); until a burst has been measured
        the installed grid holds ones."""
        with torch.cuda.device(self.device):
            if shadows is None:
                self.L.burst_set_local_tone(self._h, None, None)
                self._local_tone = self._tone_grid = self._tone_table = None
                return
            lt = _local_tone_struct(self.hr_w, self.hr_h, shadows, highlights, cell, bins, smooth, pivot, max_gain)
            gx, gy, gz = local_tone_grid(self.hr_w, self.hr_h, lt)
            grid = torch.ones(gy, gx, gz, dtype=torch.float32, device=self.device)
            torch.cuda.current_stream().synchronize()   # (the library may read the grid on another stream than the fill's)
            self.L.burst_set_local_tone(self._h, ctypes.byref(lt), grid.data_ptr())
            self._local_tone, self._tone_grid = lt, grid
            self._tone_table = torch.zeros(gy, gx, gz, 2, dtype=torch.int64, device=self.device)

    def local_tone(self) -> capi.LocalToneResult:
        """Measure the burst's accumulators and install the fitted grid (mfsr_burst_local_tone): after the last ``add_frame``
        (and after ``auto_render``, whose matrix the measurement then uses) and before ``finish``.  Needs ``set_local_tone``.
        The table is left in ``self.tone_table`` (int64 [GY, GX, GZ, 2]), the grid in ``self.tone_grid``."""
        if self._local_tone is None:
            raise RuntimeError("local_tone: call set_local_tone first")
        res = capi.LocalToneResult()
        with torch.cuda.device(self.device):
            self.L.burst_local_tone(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(), ctypes.byref(self._local_tone),
                                    self._tone_table.data_ptr(), self._tone_grid.data_ptr(), ctypes.byref(res), self._stream())
            self._held_frames.clear()
        self.local_tone_result = res
        return res

    @property
    def tone_grid(self) -> Optional[torch.Tensor]:
        return self._tone_grid if self._local_tone is not None else None

    @property
    def tone_table(self) -> Optional[torch.Tensor]:
        return self._tone_table if self._local_tone is not None else None

    def set_sharpen(self, amount: Optional[float] = None, sigma: float = 1.0, radius: int = 0, threshold: float = 0.0, taps=None):
        """Sharpen inside the finish (mfsr_burst_set_sharpen): an unsharp mask of strength ``amount`` on
        the linear float value, before the colour matrix and the tone curve, in the finish's own launch.  The blur is a
        Gaussian of ``sigma`` (``radius`` 0 = chosen from sigma, at most 4), or the symmetric ``taps`` k[0], k[1..R];
        differences below ``threshold`` (linear units) are left alone.  ``amount=None`` turns it off.  Between bursts only.
        With a zoom window the library works on the aligned window grown by one 16-pixel ring (clipped to the frame), so the
        rectangle asked for stays bit for bit the crop of the whole-frame sharpened result; ``img_out`` and
        ``total_weights`` are reallocated at that size."""
        s = _sharpen_struct(amount, sigma, radius, threshold, taps)
        on = s is not None and s.radius != 0 and s.amount != 0
        with torch.cuda.device(self.device):
            self.L.burst_set_sharpen(self._h, None if s is None else ctypes.byref(s))
            self._sharpen_on = on
            self._grow_window()

    def _grow_window(self):
        """A stencil in the finish (sharpen, denoise): the aligned window grows by one 16-pixel ring, or shrinks back."""
        if self.window.grow(WINDOW_GRID if (self._sharpen_on or self._denoise_on or self._chain_reach > 0) else 0):
            self.L.burst_set_window(self._h, *self.window.aligned)
            out_h, out_w = self.window.aligned[3], self.window.aligned[2]
            self._img_out = torch.zeros(out_h, out_w, 3, dtype=torch.float32, device=self.device)
            self._total_weights = torch.zeros_like(self._img_out)
            self.out_img = torch.empty_like(self._img_out)
            self.out16 = _render_buffer(self._fmt, out_h, out_w, self.device)
            self._out16_host = None

    def set_denoise(self, strength: Optional[float] = None, radius: int = 2, gain: float = 2.0, alpha: Optional[float] = None,
                    beta: Optional[float] = None, fade=None):
        """Denoise inside the finish (mfsr_burst_set_denoise): a range filter of ``radius`` 1..3 on the
        linear float value, before the colour matrix and the tone curve, in the finish's own launch.  Its tolerance is
        ``strength``^2 * ``gain`` * (alpha * p + beta) / n with n the pixel's accumulated weight, so it is wide where the merge
        averaged few samples and narrows by itself where it averaged many.  ``alpha`` / ``beta``: the noise model of one raw
        sample, None = ``cfg.alpha`` / ``cfg.beta``.  ``fade`` = (w_lo, w_hi): full strength at n <= w_lo, none at n >= w_hi.
        ``strength=None`` turns it off.  Between bursts only; not together with ``set_sharpen`` or a two-plane format.  With a
        zoom window the aligned window grows by one 16-pixel ring, as for ``set_sharpen``."""
        d = _denoise_struct(strength, radius, gain, self.cfg.alpha if alpha is None else alpha,
                            self.cfg.beta if beta is None else beta, fade)
        on = d is not None and d.radius != 0 and d.strength != 0
        with torch.cuda.device(self.device):
            self.L.burst_set_denoise(self._h, None if d is None else ctypes.byref(d))
            self._denoise_on = on
            self._grow_window()

    def set_finish_chain(self, denoise: Optional[dict] = None, sharpen: Optional[dict] = None, local_tone=None):
        """The finish chain (mfsr_burst_set_finish_chain): denoise, then sharpen, then the local-tone
        gain, then matrix, tone and the store of ``set_render``'s format -- ``capi.OUT_NV12`` / ``OUT_P010`` included -- in the
        finish's one launch.  ``denoise`` / ``sharpen``: dicts of the keyword arguments of ``set_denoise`` / ``set_sharpen``
        (alpha / beta default to cfg's); ``local_tone``: a ``(capi.LocalTone, grid)`` pair, the grid [GY, GX, GZ] of the full HR
        frame as ``local_tone_fit`` returns it (measured on the plain value, before denoise and sharpen).  All three None turns
        the chain off.  Between bursts only; not while ``set_sharpen``, ``set_denoise`` or ``set_local_tone`` is on, which are
        refused in turn while a chain is installed.  With a zoom window and a stencil stage the aligned window grows by one
        16-pixel ring (the reach is at most 7), as for ``set_sharpen``."""
        with torch.cuda.device(self.device):
            c, grid, reach = _chain_struct(self.hr_w, self.hr_h, denoise, sharpen, local_tone, self.device, self.cfg.alpha,
                                           self.cfg.beta)
            if grid is not None:
                torch.cuda.current_stream().synchronize()   # (the library may read the grid on another stream than the copy's)
            self.L.burst_set_finish_chain(self._h, None if c is None else ctypes.byref(c), None if grid is None else grid.data_ptr())
            self._chain, self._chain_grid, self._chain_reach = c, grid, reach   # the grid is alive as long as it is installed
            self._grow_window()

    def chained_finishes(self) -> int:
        """Launches of mfsr_finishChain since ``begin_burst`` (mfsr_burst_debug_chained): 1 for a resident burst, one per band
        for a host burst, 0 without a chain."""
        n = ctypes.c_int(-1)
        self.L.burst_debug_chained(self._h, ctypes.byref(n))
        return n.value

    def finish_geometry(self, geometry: capi.Geometry, want_float: bool = True, want_int: bool = True):
        """(float image, integer image) of the burst through the geometric finish (mfsr_burst_finish_geometry; DESIGN.md section
        2.27): tensors of the geometry's output extent, [outH, outW, 3] float32 and the tensor typed for ``set_render``'s format
        (int16 RGB without one).  An explicit call beside ``finish``, which may follow and returns what it always did.  Refused
        (capi.MfsrError) with a zoom window, with ``set_sharpen`` / ``set_denoise`` / ``set_local_tone`` / ``set_finish_chain``
        on, and with a two-plane format; ``geometry_image`` on a chained float image is the way to combine them."""
        if not (want_float or want_int):
            raise ValueError("finish_geometry: one output at least")
        w, h = int(geometry.outW), int(geometry.outH)
        with torch.cuda.device(self.device):
            fl = torch.empty(h, w, 3, dtype=torch.float32, device=self.device) if want_float else None
            out = None
            if want_int:
                if self._fmt in capi.YUV_FORMATS:   # (no buffer for it; the library's refusal names the reason)
                    out = torch.empty(1, dtype=torch.uint8, device=self.device)
                else:
                    out = _render_buffer(self._fmt, h, w, self.device)
            rb = 0 if out is None or self._fmt in capi.YUV_FORMATS else render_row_bytes(self._fmt, w)
            self.L.burst_finish_geometry(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(), ctypes.byref(geometry),
                                         None if fl is None else fl.data_ptr(), 12 * w, None if out is None else out.data_ptr(), rb,
                                         self._stream())
        self._held_frames.clear()
        return fl, out

    def geometry_finishes(self) -> int:
        """Launches of mfsr_finishGeometry since ``begin_burst`` (mfsr_burst_debug_geometry): one per ``finish_geometry``."""
        n = ctypes.c_int(-1)
        self.L.burst_debug_geometry(self._h, ctypes.byref(n))
        return n.value

    def denoised_finishes(self) -> int:
        """Launches of mfsr_finishDenoised since ``begin_burst`` (mfsr_burst_debug_denoised): 1 for a resident burst, one per
        band for a host burst, 0 when denoising is off."""
        n = ctypes.c_int(-1)
        self.L.burst_debug_denoised(self._h, ctypes.byref(n))
        return n.value

    def robust_group_launches(self) -> int:
        """Launches of mfsr_robustnessMaskGroup since ``begin_burst`` (mfsr_burst_debug_robust_group): one per aligned group
        whose masks came from the patch-mean path, 0 after ``capi.lib().set_robustness_group(0)`` / MFSR_ROBUST_GROUP=0."""
        n = ctypes.c_int(-1)
        self.L.burst_debug_robust_group(self._h, ctypes.byref(n))
        return n.value

    def fused_finishes(self) -> int:
        """Finishes taken inside the burst launch since ``begin_burst`` (mfsr_burst_debug_finish_fused): 1 where ``finish``
        asked for the plain whole-frame uint16 image only and the hold's 8, 12 or 16 frames were the burst's last fuse, else 0
        (also after ``capi.lib().set_finish_fuse(0)`` / MFSR_FINISH_FUSE=0)."""
        n = ctypes.c_int(-1)
        self.L.burst_debug_finish_fused(self._h, ctypes.byref(n))
        return n.value

    def sharpened_finishes(self) -> int:
        """Launches of mfsr_finishSharpened since ``begin_burst`` (mfsr_burst_debug_sharpened): 1 for a resident burst, one per
        band for a host burst, 0 when sharpening is off."""
        n = ctypes.c_int(-1)
        self.L.burst_debug_sharpened(self._h, ctypes.byref(n))
        return n.value

    # With cfg.pairFrames (the default) add_frame defers the warp+fuse of every other frame until its
    # partner is aligned (mfsr.h, mfsr_burst_add_frame): readers of the accumulators flush first.
    def flush(self):
        self.L.burst_flush(self._h, self._stream())
        self._held_frames.clear()

    # Burst hold (mfsr.h, mfsr_burst_hold_fuse): the complete groups of a burst leave as ONE warp+fuse launch at flush / finish
    # instead of one launch per group; bit-identical results.  The library then reads the frames' raw buffers as late as that,
    # so add_frame keeps the tensors referenced until the launch has been enqueued.
    HOLD_FUSE = True    # what begin_burst() opts into; DESIGN.md section 5 has the measurement behind the default

    def hold_fuse(self, enable: bool = True):
        self.L.burst_hold_fuse(self._h, 1 if enable else 0)
        self._hold = bool(enable)

    def fuse_stats(self):
        """(burst launches, four-frame groups they fused) since ``begin_burst`` (mfsr_burst_fuse_stats)."""
        n, g = ctypes.c_int(-1), ctypes.c_int(-1)
        self.L.burst_fuse_stats(self._h, ctypes.byref(n), ctypes.byref(g))
        return n.value, g.value

    @property
    def img_out(self) -> torch.Tensor:
        self.flush()
        return self._img_out

    @property
    def total_weights(self) -> torch.Tensor:
        self.flush()
        return self._total_weights

    def reset_accumulators(self):
        self.flush()
        self._img_out.zero_()
        self._total_weights.zero_()

    def begin_burst(self):
        """Start a burst without zeroing: the first warp+fuse launch overwrites the accumulators
        (mfsr_burst_begin).  Equivalent to reset_accumulators() for every reader (flush zeroes them if no
        frame was added).  Opts into the burst hold where ``HOLD_FUSE`` says so."""
        if self._hold is None and self.HOLD_FUSE:
            self.hold_fuse(True)
        self.L.burst_begin(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(), self._stream())
        self._held_frames.clear()

    def set_reference(self, raw: torch.Tensor):
        self._check_raw(raw)
        self.L.burst_set_reference(self._h, raw.data_ptr(), self._stream())
        self._held_frames.clear()

    def add_frame(self, raw: torch.Tensor, is_reference: bool = False):
        self._check_raw(raw)
        self.L.burst_add_frame(self._h, raw.data_ptr(), 1 if is_reference else 0, self._img_out.data_ptr(),
                               self._total_weights.data_ptr(), self._stream())
        if self._hold:
            self._held_frames.append(raw)

    def finish(self, want_float: bool = True, want_u16: bool = True):
        """(float image, u16 image) of the burst: the whole HR frame, or the rectangle given as ``window``.  After
        ``set_render`` the second one is the rendered image, typed for its format, and the float image the one it quantises."""
        self.L.burst_finish(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(),
                            self.out_img.data_ptr() if want_float else None,
                            self.out16.data_ptr() if want_u16 else None, self._stream())
        self._held_frames.clear()
        return self.window(self.out_img if want_float else None), self.window.output(self.out16 if want_u16 else None, self._fmt)

    def finish_rows(self, row0: int, rows: int) -> torch.Tensor:
        """Finish only HR rows [row0, row0+rows) (reduce-scatter mode); returns the
        full-size u16 buffer (after ``set_render``: the rendered image's buffer) with that stripe filled."""
        self.L.burst_finish_rows(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(), None,
                                 self.out16.data_ptr(), row0, rows, self._stream())
        self._held_frames.clear()
        return self.out16

    # ---- the raw-domain steps, in the order DESIGN.md sections 2.14 and 2.17 fix: repair, shade, select, match, then the burst.
    #      ``work``: checked frames the step may write (clones of the caller's) ----
    def _checked(self, frames: Sequence[torch.Tensor], clone: bool):
        for f in frames:
            self._check_raw(f)
        return [f.clone() for f in frames] if clone else list(frames)

    def _repair(self, work, threshold: Optional[int], spread: int, min_votes: Optional[int]):
        """mfsr_burst_repair_defects on ``work``, in place; sets ``defects`` and ``defect_map``."""
        n = len(work)
        t0, _, v0 = defect_defaults(self.cfg, n)
        self.defect_map = torch.empty(self.cfg.height, self.cfg.width, dtype=torch.uint8, device=self.device)
        counts_dev = torch.empty(2, dtype=torch.int32, device=self.device)
        counts = (ctypes.c_uint32 * 2)()
        self.L.burst_repair_defects(self._h, n, _ptr_table(work), t0 if threshold is None else int(threshold), int(spread),
                                    v0 if min_votes is None else int(min_votes), self.defect_map.data_ptr(),
                                    counts_dev.data_ptr(), counts, self._stream())
        self.defects = (int(counts[0]), int(counts[1]))

    def _shade(self, work, gain_map: torch.Tensor, cell: Optional[int]):
        """mfsr_burst_correct_shading on ``work``, in place."""
        cell = _shading_map(gain_map, self.cfg, cell, self.device)
        self.L.burst_correct_shading(self._h, len(work), _ptr_table(work), gain_map.data_ptr(), cell, self._stream())

    def _select(self, work, candidates: int, keep_ratio: float):
        """mfsr_burst_select_frames on ``work``: (reference, kept frame indices); sets ``selection``."""
        n = len(work)
        sums_dev = torch.empty(n, dtype=torch.int64, device=self.device)
        ref, keep = ctypes.c_int(-1), (ctypes.c_int32 * n)()
        sums, rect = (ctypes.c_longlong * n)(), (ctypes.c_int32 * 4)()
        self.L.burst_select_frames(self._h, n, _ptr_table(work), int(candidates), float(keep_ratio), sums_dev.data_ptr(),
                                   ctypes.byref(ref), keep, sums, rect, self._stream())
        r = ref.value
        kept = [k for k in range(n) if keep[k]]
        self.selection = Selection(r, kept, list(sums), tuple(rect))
        return r, kept

    def _match(self, work, r: int, per_colour: bool, deadband: Optional[int], min_gain: Optional[int], max_gain: Optional[int]):
        """mfsr_burst_match_exposure of ``work`` to frame ``r``, in place; sets ``exposure``."""
        n = len(work)
        d = exposure_defaults(self.cfg)
        levels_dev = torch.empty(n, 5, dtype=torch.int64, device=self.device)
        gains, status, levels = (ctypes.c_int32 * (3 * n))(), (ctypes.c_int32 * n)(), (ctypes.c_longlong * (5 * n))()
        self.L.burst_match_exposure(self._h, n, _ptr_table(work), r, 1 if per_colour else 0,
                                    d.deadband if deadband is None else int(deadband),
                                    d.min_gain if min_gain is None else int(min_gain),
                                    d.max_gain if max_gain is None else int(max_gain), levels_dev.data_ptr(), gains, status, levels,
                                    self._stream())
        q16 = [[int(gains[3 * k + c]) for c in range(3)] for k in range(n)]
        self.exposure = Exposure(r, [[g / 65536.0 for g in row] for row in q16], [int(s) for s in status],
                                 [[int(levels[5 * k + i]) for i in range(5)] for k in range(n)], q16)

    def calibrate_noise(self, frames: Sequence[torch.Tensor], reference: int = 0, tol: Optional[float] = None,
                        min_blocks: Optional[int] = None):
        """(alpha, beta, status, points, blocks) of the noise model var = alpha * I + beta measured on the burst itself
        (mfsr_burst_calibrate_noise_temporal): the frames are aligned to ``frames[reference]`` and the
        statistics are taken on the differences of frames that are a whole number of quads apart, so scene texture cancels
        where the single-frame ``calibrate_noise`` function reads it as noise.  tol None = 1/16 quad, min_blocks None =
        ``noise_defaults``.  status 0 ok, 2 unmeasurable (no phase-matched pair of frames, too few levels: alpha = beta = 0),
        3 alpha <= 0; points = points of the fit, blocks = accepted (block, pair) terms.  Between bursts only.  Nothing is
        fused and neither the frames nor cfg change: alpha and beta are construction-time configuration, so write them into the
        config of the pipeline created next."""
        frames = self._checked(frames, clone=False)
        n = len(frames)
        nbytes = self.L.noise_temporal_scratch_bytes(ctypes.byref(self.cfg), n)
        if nbytes == 0:
            raise ValueError("burst noise calibration needs 2 .. 64 frames")
        with torch.cuda.device(self.device):
            scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            base = (scratch.data_ptr() + 255) // 256 * 256
            a, b = ctypes.c_double(), ctypes.c_double()
            st, pts, blocks = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_longlong()
            self.L.burst_calibrate_noise_temporal(self._h, n, _ptr_table(frames), int(reference), 0.0 if tol is None else float(tol),
                                                  0 if min_blocks is None else int(min_blocks), base, nbytes, ctypes.byref(a),
                                                  ctypes.byref(b), ctypes.byref(st), ctypes.byref(pts), ctypes.byref(blocks),
                                                  self._stream())
        return a.value, b.value, st.value, pts.value, blocks.value

    def _run(self, work, r: int, kept: Iterable[int]):
        """The burst itself: reference products of frame ``r``, the ``kept`` frames, finish."""
        self.begin_burst()
        self.set_reference(work[r])
        for k in kept:
            self.add_frame(work[k], k == r)
        if self._local_tone is not None:
            self.local_tone()
        return self.finish()

    def process(self, frames: Sequence[torch.Tensor], frame_ids: Optional[Iterable[int]] = None):
        """Whole burst on this device: reference products, every frame, finish."""
        return self._run(frames, self.cfg.reference, range(len(frames)) if frame_ids is None else frame_ids)

    def process_selected(self, frames: Sequence[torch.Tensor], candidates: int = 0, keep_ratio: float = 0.0):
        """Whole burst with the reference chosen by sharpness (mfsr_burst_select_frames): the sharpest of the first
        ``candidates`` frames (0 = all) is the reference, and only frames scoring at least ``keep_ratio`` times its score
        are fused.  Then exactly what ``process`` does with that reference and those frames.  With a window the score is
        taken over the window's footprint.  Returns (float image, u16 image) like ``process``; the choice is left in
        ``self.selection`` (a ``Selection``)."""
        work = self._checked(frames, clone=False)
        return self._run(work, *self._select(work, candidates, keep_ratio))

    def process_shaded(self, frames: Sequence[torch.Tensor], gain_map: torch.Tensor, cell: Optional[int] = None):
        """Whole burst with the lens shading corrected first (mfsr_burst_correct_shading on clones: the caller's frames stay
        untouched), then exactly ``process`` of the corrected frames.  ``gain_map``: an int32 [4, gh, gw] device tensor of Q16
        gains (``calibrate_shading``; ``shading_grid`` gives gw, gh); cell None = ``shading_defaults``."""
        work = self._checked(frames, clone=True)
        self._shade(work, gain_map, cell)
        return self._run(work, self.cfg.reference, range(len(work)))

    def process_repaired(self, frames: Sequence[torch.Tensor], threshold: Optional[int] = None, spread: int = 2,
                         min_votes: Optional[int] = None, select: bool = False, candidates: int = 0, keep_ratio: float = 0.0,
                         shading: Optional[torch.Tensor] = None, shading_cell: Optional[int] = None):
        """Whole burst with its defective pixels repaired first (mfsr_burst_repair_defects on clones: the caller's frames
        stay untouched), then exactly ``process`` of the repaired frames, or ``process_selected`` (``candidates``,
        ``keep_ratio``) with ``select=True``: repair goes before selection.  threshold / min_votes None =
        ``defect_defaults``.  The (hot, cold) pixel counts are left in ``self.defects``, the map in ``self.defect_map``.
        ``shading`` (a gain map as for ``process_shaded``, with ``shading_cell``): the lens shading is corrected after the
        repair and before the selection."""
        work = self._checked(frames, clone=True)
        self._repair(work, threshold, spread, min_votes)
        if shading is not None:
            self._shade(work, shading, shading_cell)
        r, kept = self._select(work, candidates, keep_ratio) if select else (self.cfg.reference, range(len(work)))
        return self._run(work, r, kept)

    def process_matched(self, frames: Sequence[torch.Tensor], select: bool = False, repair: bool = False, per_colour: bool = False,
                        deadband: Optional[int] = None, min_gain: Optional[int] = None, max_gain: Optional[int] = None,
                        candidates: int = 0, keep_ratio: float = 0.0, threshold: Optional[int] = None, spread: int = 2,
                        min_votes: Optional[int] = None, shading: Optional[torch.Tensor] = None, shading_cell: Optional[int] = None):
        """Whole burst with the exposure of its frames matched to the reference first (mfsr_burst_match_exposure on clones:
        the caller's frames stay untouched).  Order of the raw-domain steps: repair defects (``repair=True``; threshold /
        spread / min_votes as for ``process_repaired``), correct the lens shading (``shading`` = a gain map as for
        ``process_shaded``, with ``shading_cell``), select the reference and the kept frames (``select=True``;
        candidates / keep_ratio as for ``process_selected``), match every frame to that reference, then the ordinary burst.
        deadband / min_gain / max_gain None = ``exposure_defaults``; ``per_colour``: one gain per colour instead of one per
        frame.  With a window the levels are measured over the window's footprint.  Returns (float image, u16 image) like
        ``process``; the outcome is left in ``self.exposure`` (an ``Exposure``), and ``self.defects`` / ``self.defect_map`` /
        ``self.selection`` are set by the steps that ran."""
        work = self._checked(frames, clone=True)
        if repair:
            self._repair(work, threshold, spread, min_votes)
        if shading is not None:
            self._shade(work, shading, shading_cell)
        r, kept = self._select(work, candidates, keep_ratio) if select else (self.cfg.reference, range(len(work)))
        self._match(work, r, per_colour, deadband, min_gain, max_gain)
        return self._run(work, r, kept)

    def host_sync(self):
        """Block the host until the image of the last process_host has landed in host memory."""
        self.L.burst_host_sync(self._h)

    def process_joint(self, frames: Sequence[torch.Tensor]):
        """Whole burst with the joint shift minimiser in the loop (mfsr_burst_process_joint: every neighbouring pair is
        measured besides the (reference, k) pairs; per-tile least squares with outlier rejection gives the tile shifts)."""
        if len(frames) != self.cfg.frames:
            raise ValueError("process_joint needs exactly cfg.frames frames")
        for f in frames:
            self._check_raw(f)
        nbytes = self.L.burst_joint_workspace_bytes(ctypes.byref(self.cfg))
        if nbytes == 0:
            raise ValueError("the joint mode needs 2 <= frames <= 64")
        if getattr(self, "_joint_ws", None) is None or self._joint_ws.numel() < nbytes + 256:
            self._joint_ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        base = (self._joint_ws.data_ptr() + 255) // 256 * 256
        self.L.burst_process_joint(self._h, _ptr_table(frames), base, nbytes, self._img_out.data_ptr(), self._total_weights.data_ptr(),
                                   self._stream())
        return self.finish()

    # ---- building blocks of stripe-sharded (multi-GPU) bursts: mfsr_burst_align_frame / mfsr_burst_fuse_rows ----
    def field_dims(self):
        """((flow_h, flow_w), (mask_h, mask_w)) of the per-frame products."""
        v = [ctypes.c_int() for _ in range(4)]
        self.L.burst_field_dims(self._h, *[ctypes.byref(x) for x in v])
        return (v[1].value, v[0].value), (v[3].value, v[2].value)

    def new_frame_products(self):
        """(flow [fh, fw, 2] f32, mask [mh, mw, 4] f32) device tensors with dense rows (a row range = one message)."""
        (fh, fw), (mh, mw) = self.field_dims()
        return (torch.empty(fh, fw, 2, dtype=torch.float32, device=self.device),
                torch.empty(mh, mw, 4, dtype=torch.float32, device=self.device))

    def align_frame(self, raw: torch.Tensor, is_reference: bool, flow: torch.Tensor, mask: torch.Tensor):
        self._check_raw(raw)
        self.L.burst_align_frame(self._h, raw.data_ptr(), 1 if is_reference else 0, flow.data_ptr(), flow.stride(0) * 4,
                                 mask.data_ptr(), mask.stride(0) * 4, self._stream())

    def group_size(self) -> int:
        """Frames per warp+fuse launch cfg.pairFrames stands for (mfsr_burst_group_size)."""
        return int(self.L.raw["mfsr_burst_group_size"](ctypes.byref(self.cfg)))

    def fuse_rows(self, raws, flows, masks, row_begin: int, row_end: int, fresh: bool):
        n = len(raws)
        P = ctypes.c_void_p * n
        self.L.burst_fuse_rows(self._h, n, P(*[r.data_ptr() for r in raws]), P(*[f.data_ptr() for f in flows]),
                               flows[0].stride(0) * 4, P(*[m.data_ptr() for m in masks]), masks[0].stride(0) * 4,
                               self._img_out.data_ptr(), self._total_weights.data_ptr(), 1 if fresh else 0, row_begin, row_end,
                               self._stream())

    def check_flow_bound(self, flow_rows: torch.Tensor, bound: float, flag: torch.Tensor):
        """flag |= 1 if a vertical flow of these rows exceeds ``bound`` (mfsr_checkFlowBound)."""
        self.L.checkFlowBound(flow_rows.data_ptr(), flow_rows.stride(0) * 4, flow_rows.shape[1], flow_rows.shape[0], bound,
                              flag.data_ptr(), self._stream())

    def stripe_plan(self, world: int, rank: int, raw_halo: int = 64) -> "capi.StripePlan":
        plan = capi.StripePlan()
        self.L.dist_stripe_plan(ctypes.byref(self.cfg), world, rank, raw_halo, ctypes.byref(plan))
        return plan

    # ---- frames in (pinned) host memory: the library uploads them on its own copy stream (cfg.uploadRing > 0) ----
    def process_host(self, host_frames: Sequence[torch.Tensor], out16_host: Optional[torch.Tensor] = None):
        """Whole burst from HOST frames (pin them: ``t.pin_memory()``) to the u16 HR image in host memory:
        mfsr_burst_set_reference_host / add_frame_host / finish_host.  Returns the (pinned) host image; it is complete
        after ``host_sync()`` (the download runs on a stream of its own so that the next burst overlaps it).
        With ``cfg.rawPacking`` the frames are uint8 tensors [height, rowBytes] of packed bytes (``capi.PACK_*``, rowBytes >=
        ``packed_row_bytes``: what lies beyond the dense row is line padding and is not uploaded); the library unpacks them on
        the device.  Rows may be padded either way (views with a row stride larger than the row): one stride for the burst.
        The call may be captured into a graph (``torch.cuda.graph``) after one eager call, ``host_sync()`` and a device
        synchronisation: the uploads and the download are then nodes of the graph, the pinned host frames its inputs, and the
        image is in host memory when a replay has completed."""
        if self.cfg.uploadRing <= 0:
            raise ValueError("cfg.uploadRing must be > 0 for host-frame bursts")
        if not host_frames:
            raise ValueError("at least one frame is needed")
        if self.cfg.rawPacking:
            dense, dtypes, elem = packed_row_bytes(self.cfg.rawPacking, self.cfg.width), (torch.uint8,), 1
        else:
            dense, dtypes, elem = 2 * self.cfg.width, (torch.int16, torch.uint16), 2
        row_bytes = host_frames[0].stride(0) * elem if host_frames[0].dim() == 2 else -1
        for f in host_frames:
            ok = not f.is_cuda and f.dtype in dtypes and f.dim() == 2 and f.shape[0] == self.cfg.height and f.stride(1) == 1 \
                and f.stride(0) * elem == row_bytes >= dense
            if ok and self.cfg.rawPacking:
                ok = f.shape[1] * elem >= dense
            elif ok:
                ok = f.shape[1] == self.cfg.width
            if not ok:
                raise ValueError("host frames must be CPU tensors with contiguous rows and one row stride: 16-bit of the configured "
                                 f"size, or with cfg.rawPacking uint8 [height, >= {dense}]")
        if row_bytes != getattr(self, "_host_row_bytes", dense):
            self.L.burst_set_host_row_bytes(self._h, row_bytes)
        self._host_row_bytes = row_bytes
        if out16_host is None:
            if getattr(self, "_out16_host", None) is None:
                self._out16_host = torch.empty_like(self.out16, device="cpu").pin_memory()
            out16_host = self._out16_host
        st = self._stream()
        self.begin_burst()
        ref = self.cfg.reference
        self.L.burst_set_reference_host(self._h, host_frames[ref].data_ptr(), st)
        # every copy queued before the first kernel: the copy engine then runs them back to back (mfsr_burst_prefetch_host)
        self.L.burst_prefetch_host(self._h, _ptr_table(host_frames), len(host_frames), st)
        for k, f in enumerate(host_frames):
            self.L.burst_add_frame_host(self._h, f.data_ptr(), 1 if k == ref else 0, self._img_out.data_ptr(),
                                        self._total_weights.data_ptr(), st)
        self.L.burst_finish_host(self._h, self._img_out.data_ptr(), self._total_weights.data_ptr(), self.out16.data_ptr(),
                                 out16_host.data_ptr(), st)
        return self.window.output(out16_host, self._fmt)

    def debug_views(self):
        """(flow, mask, kernel_param, tracking) descriptors of the last add_frame."""
        t = [capi.Tex2D() for _ in range(4)]
        self.L.burst_debug_views(self._h, *[ctypes.byref(x) for x in t])
        return t

    def frame_views(self, frames_back: int):
        """(flow, mask) descriptors of the frame aligned ``frames_back`` frames before the last one (mfsr_burst_debug_frame_views).
        With frame-batched alignment a frame is aligned when its group is complete (or on flush / finish), not by add_frame."""
        f, m = capi.Tex2D(), capi.Tex2D()
        self.L.burst_debug_frame_views(self._h, int(frames_back), ctypes.byref(f), ctypes.byref(m))
        return f, m

    def debug_paths(self) -> dict:
        """{name: count} of the driver branches taken since ``begin_burst`` (mfsr_burst_debug_paths; names:
        ``capi.path_names()``).  Host-side counters of launches: read them after ``flush`` / ``finish``, when every frame of
        the burst has been aligned."""
        names = capi.path_names()
        counts, n = (ctypes.c_int32 * len(names))(), ctypes.c_int(0)
        self.L.burst_debug_paths(self._h, counts, len(names), ctypes.byref(n))
        if n.value != len(names):
            raise RuntimeError(f"libmfsr_hip.so counts {n.value} paths, include/mfsr.h names {len(names)}: rebuild the library")
        return {k: int(v) for k, v in zip(names, counts)}

    def _check_raw(self, raw: torch.Tensor):
        if raw.device != self.device or raw.dtype not in (torch.int16, torch.uint16) or not raw.is_contiguous():
            raise ValueError("raw frame must be a contiguous 16-bit tensor on the pipeline's device")
        if tuple(raw.shape) != (self.cfg.height, self.cfg.width):
            raise ValueError(f"raw frame must be {self.cfg.height}x{self.cfg.width}, got {tuple(raw.shape)}")


class FrameStream:
    """Sliding-window stream (C-ABI ``mfsr_stream_*``; the reference's ``setTemporalAreaRadius``,
    finalProject/Project/multi_frame_sr.cpp:182): output t fuses frames [t-radius, t+radius] around reference t.  Every
    frame is uploaded and prepared once.  ``host_frames``: frames are pinned CPU tensors, uploaded by the library's
    copy stream."""

    def __init__(self, cfg: capi.Config, radius: int = 1, device: Optional[torch.device] = None, host_frames: bool = False,
                 window: Optional[Sequence[int]] = None, render: Optional[dict] = None, sharpen: Optional[dict] = None,
                 denoise: Optional[dict] = None, chain: Optional[dict] = None):
        """chain: the keyword arguments of ``BurstPipeline.set_finish_chain`` (denoise, sharpen, local_tone): every output's
        finish runs the chain; a window grows as for sharpen when the chain has a stencil stage.
        window: every output is that HR rectangle (see BurstPipeline).  render: the keyword arguments of
        ``BurstPipeline.set_render`` (format, matrix, tone_lut, yuv): every output is rendered, typed for the format.  sharpen: the
        keyword arguments of ``BurstPipeline.set_sharpen``: every output is sharpened inside its finish; with a window the
        library works on the aligned window grown by one 16-pixel ring, as ``BurstPipeline`` does, so the rectangle asked for
        is the crop of the whole-frame sharpened output.  denoise: the keyword arguments of ``BurstPipeline.set_denoise``
        (alpha / beta default to cfg's): every output is denoised inside its finish; a window grows in the same way."""
        if not torch.cuda.is_available():
            raise RuntimeError("multi_frame_super_resolution_amd needs a HIP device (MI355X); there is no CPU fallback")
        self.L = capi.lib()
        self.cfg = cfg
        self.radius = radius
        self.host_frames = host_frames
        self.window = _Window(cfg, window)
        sharp = None if sharpen is None else _sharpen_struct(**sharpen)
        den = None
        if denoise is not None:
            kw = dict(denoise)
            kw["alpha"] = cfg.alpha if kw.get("alpha") is None else kw["alpha"]
            kw["beta"] = cfg.beta if kw.get("beta") is None else kw["beta"]
            den = _denoise_struct(**kw)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        ch, self._chain_grid, reach = None, None, 0
        if chain is not None:
            with torch.cuda.device(self.device):
                ch, self._chain_grid, reach = _chain_struct(cfg.width * cfg.scale, cfg.height * cfg.scale, chain.get("denoise"),
                                                            chain.get("sharpen"), chain.get("local_tone"), self.device, cfg.alpha,
                                                            cfg.beta)
                torch.cuda.current_stream().synchronize()
        if (sharp is not None and sharp.radius != 0 and sharp.amount != 0) or (
                den is not None and den.radius != 0 and den.strength != 0) or reach > 0:
            self.window.grow(WINDOW_GRID)
        nbytes = self.L.stream_workspace_bytes(ctypes.byref(cfg), radius)
        if nbytes == 0:
            raise ValueError("invalid mfsr_config / radius")
        with torch.cuda.device(self.device):
            self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
            base = (self.workspace.data_ptr() + 255) // 256 * 256
            self.hr_w, self.hr_h = cfg.width * cfg.scale, cfg.height * cfg.scale
            self.out16 = torch.empty(self.window.aligned[3], self.window.aligned[2], 3, dtype=torch.int16, device=self.device)
            h = ctypes.c_void_p()
            self.L.stream_create(ctypes.byref(h), ctypes.byref(cfg), radius, 1 if host_frames else 0, base, nbytes)
            self._h = h
            self.window.apply(self.L.stream_set_window, self._h)
            self._fmt = capi.OUT_RGB16
            if render is not None:
                fmt = int(render.get("format", capi.OUT_RGB16))
                self.window.check_yuv(fmt)
                r, self._render_lut = _render_struct(fmt, render.get("matrix"), render.get("tone_lut"), self.device,
                                                     int(render.get("yuv", 0)))
                self.L.stream_set_render(self._h, ctypes.byref(r))
                self.out16 = _render_buffer(fmt, self.window.aligned[3], self.window.aligned[2], self.device)
                self._fmt = fmt
            if sharp is not None:
                self.L.stream_set_sharpen(self._h, ctypes.byref(sharp))
            if den is not None:
                self.L.stream_set_denoise(self._h, ctypes.byref(den))
            if ch is not None:
                self.L.stream_set_finish_chain(self._h, ctypes.byref(ch),
                                               None if self._chain_grid is None else self._chain_grid.data_ptr())

    def close(self):
        if getattr(self, "_h", None):
            self.L.stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, frame: torch.Tensor):
        """Hand over the next frame; returns (t, u16 HR image) once output t is produced (the image is this object's
        buffer, valid until the next push / drain), else None."""
        if frame.is_cuda == self.host_frames or not frame.is_contiguous() or tuple(frame.shape) != (self.cfg.height, self.cfg.width):
            raise ValueError("frame must be a contiguous 16-bit tensor of the configured size, on the "
                             + ("host" if self.host_frames else "device"))
        produced = ctypes.c_longlong(-1)
        self.L.stream_push(self._h, frame.data_ptr(), None, self.out16.data_ptr(), ctypes.byref(produced),
                           torch.cuda.current_stream().cuda_stream)
        return (produced.value, self.window.output(self.out16, self._fmt)) if produced.value >= 0 else None

    def drain(self):
        """End of the stream: yields the outstanding (t, u16 HR image) outputs."""
        while True:
            produced = ctypes.c_longlong(-1)
            self.L.stream_drain(self._h, None, self.out16.data_ptr(), ctypes.byref(produced), torch.cuda.current_stream().cuda_stream)
            if produced.value < 0:
                return
            yield produced.value, self.window.output(self.out16, self._fmt)


def view_as_tensor(t: capi.Tex2D, channels: int, device) -> torch.Tensor:
    """Copy a device image described by a Tex2D into a fresh [H, W, C] float tensor (tests)."""
    L = capi.lib()
    out = torch.empty(t.height, t.width, channels, dtype=torch.float32, device=device)
    # hipMemcpy2D through torch: build a strided view over the raw pointer is not possible
    # without owning it, so go through the C-ABI's resample-free path: a 1:1 float copy
    # kernel is not exported; use ctypes + hipMemcpy2DAsync from libamdhip64 instead.
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                ctypes.c_size_t, ctypes.c_int]
    rc = hip.hipMemcpy2D(out.data_ptr(), t.width * channels * 4, t.ptr, t.pitch, t.width * channels * 4, t.height, 3)
    if rc != 0:
        raise RuntimeError(f"hipMemcpy2D failed: {rc}")
    torch.cuda.synchronize()
    return out
