"""Synthetic bursts (after the reference's own burst
generator test_opencv/main.cpp:1877-1913: one scene, per-frame random shifts
in U(-5,5) LR pixels, down-sampling, crops).

Scene = band-limited noise + hard edges on an HR grid of (s*W+64*s) x (s*H+64*s);
frame k = scene shifted by a sub-pixel offset t_k (bilinear), box-averaged by s,
plus signal-dependent noise (variance alpha*I + beta), then either kept as a
12-bit gray frame or mosaicked to a 12-bit RGGB raw frame
(u16 = round(I * white + black)).  Frame 0 is the reference (zero shift).

torch is used only as an array library (works on cpu and on cuda); nothing here
is part of the measured path.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F


def _scene(hr_h: int, hr_w: int, gen: torch.Generator, device) -> torch.Tensor:
    """[3, H, W] float in [0.05, 0.95]."""
    def noise(div):
        h, w = max(hr_h // div, 2), max(hr_w // div, 2)
        n = torch.rand(1, 1, h, w, generator=gen, device=device)
        return F.interpolate(n, size=(hr_h, hr_w), mode="bicubic", align_corners=False)[0, 0]

    lum = 0.5 * noise(32) + 0.3 * noise(8) + 0.2 * noise(3)
    # hard edges: random axis-aligned boxes and a diagonal stripe pattern
    yy, xx = torch.meshgrid(torch.arange(hr_h, device=device), torch.arange(hr_w, device=device), indexing="ij")
    nbox = 24
    bx = torch.rand(nbox, 4, generator=gen, device=device)
    for i in range(nbox):
        x0, y0 = int(bx[i, 0] * hr_w), int(bx[i, 1] * hr_h)
        w, h = int(20 + bx[i, 2] * hr_w * 0.15), int(20 + bx[i, 3] * hr_h * 0.15)
        lum[y0:y0 + h, x0:x0 + w] = lum[y0:y0 + h, x0:x0 + w] * 0.5 + (0.15 if i % 2 else 0.6)
    stripes = (((xx + 2 * yy) // 23) % 2).float()
    lum = lum * (0.85 + 0.15 * stripes)
    lum = (lum - lum.min()) / (lum.max() - lum.min() + 1e-9)
    chroma = torch.stack([noise(16), noise(16), noise(16)]) - 0.5
    rgb = (0.1 + 0.8 * lum)[None] + 0.15 * chroma
    return rgb.clamp(0.05, 0.95)


def _shifted(scene: torch.Tensor, tx: float, ty: float) -> torch.Tensor:
    """scene sampled at (x + tx, y + ty), bilinear (tx,ty in scene pixels)."""
    ix, iy = math.floor(tx), math.floor(ty)
    fx, fy = tx - ix, ty - iy
    s = torch.roll(scene, shifts=(-iy, -ix), dims=(1, 2))
    s10 = torch.roll(s, shifts=-1, dims=2)
    s01 = torch.roll(s, shifts=-1, dims=1)
    s11 = torch.roll(s01, shifts=-1, dims=2)
    return (1 - fx) * (1 - fy) * s + fx * (1 - fy) * s10 + (1 - fx) * fy * s01 + fx * fy * s11


def _shifted_crop(scene: torch.Tensor, tx: float, ty: float, m: int, hh: int, ww: int) -> torch.Tensor:
    """_shifted(scene, tx, ty)[:, m:m + hh, m:m + ww] without moving the whole scene four times: while the shift stays inside
    the margin m the rolled scene's wrap-around never reaches the crop, so the four neighbours are plain slices -- the same
    elements in the same arithmetic, bit for bit (a 16-frame 4K burst: 27 -> 15 s on the CPU)."""
    ix, iy = math.floor(tx), math.floor(ty)
    if not (m + iy >= 0 and m + ix >= 0 and m + iy + hh + 1 <= scene.shape[1] and m + ix + ww + 1 <= scene.shape[2]):
        return _shifted(scene, tx, ty)[:, m:m + hh, m:m + ww]
    fx, fy = tx - ix, ty - iy
    y0, x0 = m + iy, m + ix
    s = scene[:, y0:y0 + hh, x0:x0 + ww]
    s10 = scene[:, y0:y0 + hh, x0 + 1:x0 + 1 + ww]
    s01 = scene[:, y0 + 1:y0 + 1 + hh, x0:x0 + ww]
    s11 = scene[:, y0 + 1:y0 + 1 + hh, x0 + 1:x0 + 1 + ww]
    return (1 - fx) * (1 - fy) * s + fx * (1 - fy) * s10 + (1 - fx) * fy * s01 + fx * fy * s11


def _rotated(scene: torch.Tensor, tx: float, ty: float, angle_deg: float) -> torch.Tensor:
    """scene sampled at c + R(angle) (p - c) + (tx, ty), bilinear, c = image centre (the rotation stress variant of
    SURVEY.md section 8d; the reference's generator rotates its crops the same way, test_opencv/main.cpp:1896-1907)."""
    _, h, w = scene.shape
    a = math.radians(angle_deg)
    ca, sa = math.cos(a), math.sin(a)
    dev = scene.device
    yy, xx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32),
                            indexing="ij")
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    dx, dy = xx - cx, yy - cy
    qx = cx + ca * dx - sa * dy + tx
    qy = cy + sa * dx + ca * dy + ty
    grid = torch.stack([(qx + 0.5) / w * 2 - 1, (qy + 0.5) / h * 2 - 1], -1)[None]
    return F.grid_sample(scene[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0]


def make_burst(width: int, height: int, frames: int, scale: int = 2, mono: bool = False, seed: int = 1234,
               device="cpu", max_shift: float = 5.0, noise: bool = True, alpha: float = 1e-4, beta: float = 1e-6,
               black: float = 256.0, white: float = 4095.0 - 256.0, shift_seed: Optional[int] = None,
               first_is_reference: bool = True,
               angles_deg: Optional[List[float]] = None,
               keep: Optional[Sequence[int]] = None, _composite=None,
               shifts: Optional[torch.Tensor] = None) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """Returns (raw frames [H,W] int16 holding u16 bit patterns, shifts [N,2] in LR px, ground truth [3,sH,sW]).

    ``seed`` fixes the scene; ``shift_seed`` (default: same stream) fixes the per-frame shifts and
    noise, so ranks of a sharded burst can draw different frames of the SAME scene.  ``angles_deg`` (one per frame)
    additionally rotates frame k about the frame centre (needs cfg.preAlign beyond a degree or two).  ``keep``: only
    these frame numbers are rendered (the others come back as None) while the random stream advances as if all were -- a
    rank of a sharded burst gets exactly the frames the one-GPU burst has at those positions.  ``_composite(scene, k)``
    (``make_moving_burst``): the HR scene frame k is rendered from (k = None: the ground truth's); it draws nothing from the
    random stream.  ``shifts``: an [N, 2] tensor of per-frame shifts in LR pixels that replaces the drawn ones, row 0 included
    (the random stream advances as if they had been used, so the noise of every frame is the one of the call without it)."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    s = scale
    m = 32 * s
    hr_h, hr_w = s * height + 2 * m, s * width + 2 * m
    scene = _scene(hr_h, hr_w, gen, device)
    if shift_seed is not None:
        gen = torch.Generator(device=device)
        gen.manual_seed(shift_seed)
    drawn = (torch.rand(frames, 2, generator=gen, device=device) * 2 - 1) * max_shift
    if first_is_reference:
        drawn[0] = 0
    shifts = drawn if shifts is None else torch.as_tensor(shifts, dtype=drawn.dtype, device=device).reshape(frames, 2).clone()
    out = []
    yy, xx = torch.meshgrid(torch.arange(height, device=device), torch.arange(width, device=device), indexing="ij")
    cfa_idx = ((yy % 2) + (xx % 2))  # RGGB: (0,0)->R=0, (0,1)/(1,0)->G=1, (1,1)->B=2
    keep_set = None if keep is None else set(int(k) for k in keep)
    for k in range(frames):
        if keep_set is not None and k not in keep_set:
            if noise:  # the draw the frame would have made
                torch.randn((3, height, width), generator=gen, device=device)
            out.append(None)
            continue
        tx, ty = float(shifts[k, 0]) * s, float(shifts[k, 1]) * s
        ang = float(angles_deg[k]) if angles_deg is not None else 0.0
        src = scene if _composite is None else _composite(scene, k)
        if ang == 0.0:
            sh = _shifted_crop(src, tx, ty, m, s * height, s * width)
        else:
            sh = _rotated(src, tx, ty, ang)[:, m:m + s * height, m:m + s * width]
        lr = F.avg_pool2d(sh[None], s)[0] if s > 1 else sh
        if noise:
            lr = lr + torch.randn(lr.shape, generator=gen, device=device) * torch.sqrt(alpha * lr + beta)
        if mono:
            img = 0.299 * lr[0] + 0.587 * lr[1] + 0.114 * lr[2]
        else:
            img = torch.gather(lr, 0, cfa_idx[None])[0]
        raw = torch.round(img * white + black).clamp(0, 4095).to(torch.int16)
        out.append(raw.contiguous())
    gt = (scene if _composite is None else _composite(scene, None))[:, m:m + s * height, m:m + s * width].contiguous()
    return out, shifts, gt


def make_moving_burst(width: int, height: int, frames: int, scale: int = 2, obj_size: Optional[Tuple[int, int]] = (24, 24),
                      obj_start: Optional[Tuple[float, float]] = None, obj_step: Tuple[float, float] = (6.0, 0.0),
                      obj_level: float = 0.9, obj_texture: float = 0.15, obj_seed: int = 99, **kwargs):
    """``make_burst`` with something in the scene that moves: a textured rectangular patch of ``obj_size`` = (w, h) LR pixels,
    composited into the HR scene BEFORE the per-frame shift, box average and noise, whose top-left corner is at
    ``obj_start + k * obj_step`` (x, y in LR pixels of the reference frame's grid, rounded to the HR grid) in frame k.  Frame 0
    is the reference (``first_is_reference``), so ``obj_start`` is where the ground truth shows the object; default: the
    frame's centre.  The patch's luminance is ``obj_level`` + ``obj_texture`` * (uniform noise of one value per LR pixel - 0.5),
    equal in the three channels, drawn from a generator of its own (``obj_seed``): the scene's random stream does not see it.
    Every other argument is ``make_burst``'s; ``obj_size=None`` renders no object and returns exactly ``make_burst``'s frames.

    Returns (frames, shifts, ground truth [3, sH, sW] with the object at the reference frame's position, footprints
    [N, sH, sW] bool: the HR pixels of the ground truth's grid the object covers in frame k)."""
    s = scale
    m = 32 * s
    device = kwargs.get("device", "cpu")
    if obj_size is None:
        out, shifts, gt = make_burst(width, height, frames, scale=scale, **kwargs)
        return out, shifts, gt, torch.zeros(frames, s * height, s * width, dtype=torch.bool, device=device)
    ow, oh = int(obj_size[0]), int(obj_size[1])
    if obj_start is None:
        obj_start = ((width - ow) / 2.0, (height - oh) / 2.0)
    g = torch.Generator(device=device)
    g.manual_seed(obj_seed)
    lum = obj_level + obj_texture * (torch.rand(oh, ow, generator=g, device=device) - 0.5)
    patch = lum.repeat_interleave(s, 0).repeat_interleave(s, 1).clamp(0.05, 0.95)[None].expand(3, -1, -1)

    def corner(k):  # HR pixel of the object's top-left corner in frame k, on the cropped (ground truth) grid
        return (int(round((obj_start[0] + k * obj_step[0]) * s)), int(round((obj_start[1] + k * obj_step[1]) * s)))

    def composite(scene, k):
        x, y = corner(0 if k is None else k)
        x0, y0 = max(x + m, 0), max(y + m, 0)
        x1, y1 = min(x + m + ow * s, scene.shape[2]), min(y + m + oh * s, scene.shape[1])
        if x1 <= x0 or y1 <= y0:
            return scene
        c = scene.clone()
        c[:, y0:y1, x0:x1] = patch[:, y0 - (y + m):y1 - (y + m), x0 - (x + m):x1 - (x + m)]
        return c

    out, shifts, gt = make_burst(width, height, frames, scale=scale, _composite=composite, **kwargs)
    foot = torch.zeros(frames, s * height, s * width, dtype=torch.bool, device=device)
    for k in range(frames):
        x, y = corner(k)
        foot[k, max(y, 0):max(min(y + oh * s, s * height), 0), max(x, 0):max(min(x + ow * s, s * width), 0)] = True
    return out, shifts, gt, foot


def make_chart_burst(width: int, height: int, frames: int, alpha: float, beta: float, mono: bool = False, seed: int = 1234,
                     device="cpu", patch: int = 64, black: float = 256.0, white: float = 4095.0 - 256.0) -> List[torch.Tensor]:
    """A noise-calibration chart: ``frames`` raw frames [H, W] (int16 holding u16 bit patterns) of one static scene of flat grey
    patches, ``patch`` x ``patch`` raw samples each, whose levels cover 0.05 .. 0.95 evenly in a seeded random order (the part
    of a patch the frame cuts off is simply missing).  No motion; the same noise (variance alpha*I + beta), quantisation and
    clamp as ``make_burst``, and the same RGGB / mono layout -- every channel of a grey patch has the patch's level.  512x384
    gives 8 x 6 = 48 patches."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    ny, nx = -(-height // patch), -(-width // patch)
    n = ny * nx
    levels = torch.linspace(0.05, 0.95, n, device=device) if n > 1 else torch.full((1,), 0.5, device=device)
    levels = levels[torch.randperm(n, generator=gen, device=device)].reshape(ny, nx)
    img = levels.repeat_interleave(patch, 0).repeat_interleave(patch, 1)[:height, :width].contiguous()
    out = []
    for _ in range(frames):
        noisy = img + torch.randn(img.shape, generator=gen, device=device) * torch.sqrt(alpha * img + beta)
        out.append(torch.round(noisy * white + black).clamp(0, 4095).to(torch.int16).contiguous())
    return out


def vignette(width: int, height: int, strength: float = 0.8, colour_tilt: float = 0.05, device="cpu") -> torch.Tensor:
    """The transmission of a lens over a ``width`` x ``height`` RGGB sensor, a float64 [H, W] tensor in (0, 1]: 1 / (1 +
    strength * r^2)^2 with r the distance from the frame centre in half-diagonals (r = 1 in the corners), times a colour shading
    that grows with r^2: red samples lose ``colour_tilt`` at r = 1, blue samples gain it (green: none), normalised so that no
    value exceeds 1.  Sensor coordinates: the same for every frame of a burst, whatever the scene does."""
    yy, xx = torch.meshgrid(torch.arange(height, device=device, dtype=torch.float64),
                            torch.arange(width, device=device, dtype=torch.float64), indexing="ij")
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    r2 = ((xx - cx) ** 2 + (yy - cy) ** 2) / (cx * cx + cy * cy)
    colour = (yy.long() % 2) + (xx.long() % 2)  # RGGB: 0 red, 1 green, 2 blue
    tilt = 1.0 + colour_tilt * (colour.double() - 1.0) * r2
    v = tilt / (1.0 + strength * r2) ** 2
    return v / v.max()


def make_flat_burst(width: int, height: int, frames: int, level: float = 0.6, vignette: Optional[torch.Tensor] = None,
                    alpha: float = 1e-4, beta: float = 1e-6, seed: int = 1234, device="cpu", black: float = 256.0,
                    white: float = 4095.0 - 256.0) -> List[torch.Tensor]:
    """Flat-field frames for ``calibrate_shading``: ``frames`` raw frames [H, W] (int16 holding u16 bit patterns) of a uniformly
    lit diffuser at ``level`` seen through ``vignette`` (a [H, W] transmission as the function of that name makes it; None = no lens),
    with the noise (variance alpha*I + beta at the shaded level I), quantisation and clamp of ``make_burst``."""
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    img = torch.full((height, width), float(level), dtype=torch.float64, device=device)
    if vignette is not None:
        img = img * vignette.to(device=device, dtype=torch.float64)
    out = []
    for _ in range(frames):
        noisy = img + torch.randn(img.shape, generator=gen, device=device, dtype=torch.float64) * torch.sqrt(alpha * img + beta)
        out.append(torch.round(noisy * white + black).clamp(0, 4095).to(torch.int16).contiguous())
    return out


def pack_raw(frames, packing: int, row_bytes: Optional[int] = None):
    """Pack 16-bit frames into the 10 / 12-bit layouts of ``capi.PACK_*`` (CPU only; the inverse of ``pipeline.unpack_raw``,
    for tests and tools: the library itself has no packer).  ``frames``: an integer tensor [height, width] or a sequence of
    them; every sample must fit the packing's bits and the width be a whole number of groups (4 samples at 10 bits, 2 at 12).
    ``row_bytes``: the row stride of the result, at least width * bits / 8 (the default); the padding bytes are zero.
    Returns uint8 CPU tensor(s) [height, row_bytes]: a tensor for a tensor, a list for a sequence."""
    from .capi import PACK_BE10, PACK_BE12, PACK_BITS, PACK_MIPI10, PACK_MIPI12

    if packing not in PACK_BITS:
        raise ValueError(f"unknown packing {packing}")
    bits = PACK_BITS[packing]
    single = isinstance(frames, torch.Tensor)
    out = []
    for f in ([frames] if single else list(frames)):
        if f.dim() != 2 or f.is_floating_point():
            raise ValueError("frames must be integer tensors [height, width]")
        p = f.cpu()
        p = (p.view(torch.int16) if p.dtype == torch.uint16 else p).to(torch.int32) & 0xffff
        h, w = p.shape
        if w == 0 or w % (4 if bits == 10 else 2) != 0:
            raise ValueError(f"width {w} is not a whole number of {bits}-bit groups")
        if int(p.max()) >= (1 << bits):
            raise ValueError(f"a sample does not fit {bits} bits")
        dense = w * bits // 8
        rb = dense if row_bytes is None else int(row_bytes)
        if rb < dense:
            raise ValueError(f"row_bytes {rb} is below the dense row size {dense}")
        if bits == 10:
            p0, p1, p2, p3 = (p[:, j::4] for j in range(4))
            if packing == PACK_MIPI10:
                b = [p0 >> 2, p1 >> 2, p2 >> 2, p3 >> 2, (p0 & 3) | (p1 & 3) << 2 | (p2 & 3) << 4 | (p3 & 3) << 6]
            else:
                assert packing == PACK_BE10
                b = [p0 >> 2, (p0 & 3) << 6 | p1 >> 4, (p1 & 15) << 4 | p2 >> 6, (p2 & 63) << 2 | p3 >> 8, p3 & 255]
        else:
            p0, p1 = p[:, 0::2], p[:, 1::2]
            if packing == PACK_MIPI12:
                b = [p0 >> 4, p1 >> 4, (p0 & 15) | (p1 & 15) << 4]
            else:
                assert packing == PACK_BE12
                b = [p0 >> 4, (p0 & 15) << 4 | p1 >> 8, p1 & 255]
        rows = torch.zeros(h, rb, dtype=torch.uint8)
        rows[:, :dense] = torch.stack(b, dim=2).reshape(h, dense).to(torch.uint8)
        out.append(rows)
    return out[0] if single else out
