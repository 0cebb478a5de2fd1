"""A float32 numpy model of which strips the x4 warp+fuse tile kernel may take on its fast path, and the hostile inputs that
tests/test_fuse_tile_x4_cpu.py (what the inputs are) and tests/test_fuse_tile_x4_gpu.py (what the kernel does with them) share.

The model is written from the definition of the operation (the texture stand-in `tex_coord` + `lerp4`
in float32 at the pixel's normalised centre, then roundf(4 u), NaN -> 0, saturating), not from the kernel: nothing here
imports the code under test.  Per HR pixel of a 4 W x 4 H frame with fields at HR / 8 it gives

    sx, sy      the rounded flow in HR pixels
    qx, qy      X + sx - 2, Y + sy - 2: the first tap; the 5 x 5 taps fall on the raw sites (qx >> 2 .. +1, qy >> 2 .. +1)
    inside      0 <= qx <= 4 W - 5 and 0 <= qy <= 4 H - 5: every tap is a raw site of the frame, nothing is clamped
    dx, dy      sx, sy relative to the rounded flow of the tile's centre texel (field column 64 b + 32 of tile column
                b = X // 512, field row Y >> 3), that one clamped to +-32000

and per strip of four pixels whether a launch form may take it: every pixel inside the frame and
    form 1 (one frame per launch)              -2^20 <= sx, sy < 2^20
    form 2 (two frames)                        -2^15 <= sx, sy < 2^15
    form 3, 4 (three and four frames)          form 2's bound, and -128 <= dx, dy <= 127 (the flow is kept in 8:8 bits)
The kernel also asks for positive semi-definite kernel parameters on the strip's four texels; that is a property of
another input, so the cases that rely on the model use a kernel field that is positive definite everywhere.

`tie` is the distance of 4 u from the nearest half-integer.  The inputs below keep it at 1/16 or more, so that no float32
rounding can move a pixel's rounded flow, everywhere but in the 8 x 8-pixel corner zones of the +-128 plateaus (4 u = k +- 128 a b
with a, b odd sixteenths is a half-integer there); the model, the oracle and the kernels evaluate lerp4 unfused in the same
order and agree there too, but no assertion about admission rests on those strips.
"""
import numpy as np

W, H, S = 328, 104, 4               # raw frame; HR 1312 x 416: two whole 512-pixel tiles and a ragged one of 288, 208 tile rows
HRW, HRH = W * S, H * S
FW, FH = HRW // 8, HRH // 8         # flow / kernel fields (and, at these sizes, the certainty masks): 164 x 52
MARGIN = 16                         # the frame's border ring belongs to the margin kernel
TILE_W = 512
CLAMP = 32000
F32 = np.float32


def form_of(n):
    return min(int(n), 3)           # 3 and 4 frames per launch are one code form


def round2i(f):
    """roundf (half away from zero) then float -> int as the hardware converts: NaN -> 0, saturating."""
    f = np.asarray(f, F32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        r = np.sign(f) * np.floor(np.abs(f) + 0.5)
    r = np.where(np.isnan(f), 0.0, r)
    return np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def tex_axis(n_out, n_tex):
    """One axis of tex_coord (clamp addressing) at the centres of n_out pixels over n_tex texels: i0, i1, fraction (float32)."""
    x = np.arange(n_out, dtype=F32)
    pos = (x + F32(0.5)) / F32(n_out)
    xb = pos * F32(n_tex) - F32(0.5)
    f = np.floor(xb)
    i = f.astype(np.int64)
    return np.clip(i, 0, n_tex - 1), np.clip(i + 1, 0, n_tex - 1), (xb - f).astype(F32)


def lerp_field(t):
    """lerp4 of the field t (FH x FW, float32) at every HR pixel, in float32 and in lerp4's order of operations."""
    i0, i1, a = tex_axis(HRW, t.shape[1])
    j0, j1, b = tex_axis(HRH, t.shape[0])
    a, b, one = a[None, :], b[:, None], F32(1.0)
    t = np.asarray(t, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((((one - a) * (one - b)) * t[j0][:, i0] + (a * (one - b)) * t[j0][:, i1]) + ((one - a) * b) * t[j1][:, i0]) + \
            (a * b) * t[j1][:, i1]


class FlowModel:
    def __init__(self, flow):
        flow = np.asarray(flow, F32)
        assert flow.shape == (FH, FW, 2)
        yy, xx = np.mgrid[0:HRH, 0:HRW]
        u4 = [lerp_field(flow[..., c]) * F32(4.0) for c in range(2)]
        self.sx, self.sy = round2i(u4[0]), round2i(u4[1])
        self.qx, self.qy = xx + self.sx - 2, yy + self.sy - 2
        self.inside = (self.qx >= 0) & (self.qx <= HRW - 5) & (self.qy >= 0) & (self.qy <= HRH - 5)
        cc = np.minimum(64 * (xx // TILE_W) + 32, FW - 1)
        centre = flow[yy >> 3, cc] * F32(4.0)
        self.bsx = np.clip(round2i(centre[..., 0]), -CLAMP, CLAMP)
        self.bsy = np.clip(round2i(centre[..., 1]), -CLAMP, CLAMP)
        self.dx, self.dy = self.sx - self.bsx, self.sy - self.bsy
        tie = np.full((HRH, HRW), np.inf)
        for v in u4:
            v = v.astype(np.float64)
            with np.errstate(invalid="ignore"):
                ok = np.abs(v) < 2.0 ** 22
                tie = np.where(ok, np.minimum(tie, np.abs(np.abs(v) % 1.0 - 0.5)), tie)
        self.tie = tie

    def pixel_ok(self, form):
        bound = 1 << 20 if form == 1 else 1 << 15
        ok = self.inside & (self.sx >= -bound) & (self.sx < bound) & (self.sy >= -bound) & (self.sy < bound)
        if form >= 3:
            ok &= (self.dx >= -128) & (self.dx <= 127) & (self.dy >= -128) & (self.dy <= 127)
        return ok

    def admitted(self, form):
        """(HRH, HRW / 4) bool: the strip X0 = 4 j of row Y may take the fast path of launch form `form`."""
        return self.pixel_ok(form).reshape(HRH, HRW // 4, 4).all(-1)


def live_strips():
    """The strips the tile kernel owns: clear of the 16-pixel border ring."""
    m = np.zeros((HRH, HRW // 4), bool)
    m[MARGIN:HRH - MARGIN, MARGIN // 4:(HRW - MARGIN) // 4] = True
    return m


def per_strip(a):
    return a.reshape(HRH, HRW // 4, 4)


# ---- the inputs ----------------------------------------------------------------------------------------------------
def const_flow(fx, fy):
    return np.ascontiguousarray(np.zeros((FH, FW, 2), F32) + F32([fx, fy]))


def residue_flow(k=0):
    """4 fx = ((col // 20 + k) % 8) - 3, 4 fy = ((row // 6 + 3 k) % 8) - 4: blocks of 160 x 48 HR pixels over which the rounded
    flow takes every residue modulo 8 on either axis; frame k's blocks are rotated, so the frames of a group disagree about
    the phase at every pixel but a few where the blocks wrap from +4 to -3."""
    fx4 = ((np.arange(FW) // 20 + k) % 8) - 3
    fy4 = ((np.arange(FH) // 6 + 3 * k) % 8) - 4
    f = np.zeros((FH, FW, 2), F32)
    f[..., 0] = (fx4 / 4.0)[None, :]
    f[..., 1] = (fy4 / 4.0)[:, None]
    return f


# plateaus of texels that put whole strips at d HR pixels from the flow of their tile's centre texel (columns 32 and 96 stay
# on the base flow).  x axis: positive offsets on the left, negative ones in the second tile, so every tap stays inside the
# frame; y axis: positive ones at the top, negative ones at the bottom.  Blocks of +-127, 128 / -128, -129 are at the texels
# of the x2 test_admission_edge; the third row / column block is for the two-frame form (its bound is +-2^15, not 8 bits).
X_BLOCKS = {127: (slice(6, 10), slice(8, 11)), 128: (slice(12, 16), slice(8, 11)), 129: (slice(18, 22), slice(8, 11)),
            -128: (slice(6, 10), slice(70, 73)), -129: (slice(12, 16), slice(70, 73)), -127: (slice(18, 22), slice(70, 73))}
Y_BLOCKS = {127: (slice(5, 8), slice(4, 8)), 128: (slice(5, 8), slice(40, 44)), 129: (slice(5, 8), slice(76, 80)),
            -128: (slice(40, 43), slice(4, 8)), -129: (slice(40, 43), slice(40, 44)), -127: (slice(40, 43), slice(76, 80))}
BLOCKS = (X_BLOCKS, Y_BLOCKS)
BASE = ((1.0, -0.5), (-1.5, 1.0))
EDGE_D = (127, 128, -128, -129)             # d = 4 * (+31.75, +32.0, -32.0, -32.25)
EDGE_D2 = EDGE_D + (129, -127)              # the two-frame form: +-127, +-128, +-129
NAN_PATCH, HUGE_PATCH = (slice(20, 23), slice(60, 63)), (slice(30, 33), slice(20, 23))


def edge_flow(axis, ds=EDGE_D, patches=False):
    """Base flow BASE[axis] with the plateaus `ds` (HR pixels, multiples of a quarter LR pixel) on that axis."""
    f = const_flow(*BASE[axis])
    for d in ds:
        f[BLOCKS[axis][d] + (axis,)] += F32(d / 4.0)
    if patches:
        f[NAN_PATCH] = np.nan
        f[HUGE_PATCH] = 1e9
    return f


def far_flow(which, sign):
    """Whole frames at the clamp of the tile's own flow: 4 * flow = +-32000 and -+32001; every tap is outside the frame."""
    return const_flow(sign * 8000.0, -sign * 8000.25) if which == 0 else const_flow(-sign * 8000.25, sign * 8000.0)


def plateau_strips(block):
    """The strips whose four pixels interpolate between texels of the block only (texel c is centred on HR pixel 8 c + 4)."""
    rows, cols = block
    m = np.zeros((HRH, HRW // 4), bool)
    m[8 * rows.start + 4:8 * (rows.stop - 1) + 4, (8 * cols.start + 4) // 4:(8 * (cols.stop - 1) + 4) // 4] = True
    return m


def refused_group_flow(k):
    """Frame k of the group that shows the fast path ran: frame 0 carries the admitted x plateaus (d = 127, -128), frame 1 the
    admitted y plateaus, frames 2 and 3 are off the frame as a whole; EVERY frame carries plateaus at the texels of d = 128 and
    d = -129 of both axes, at d = 128 + k and -129 - k: the three- and four-frame forms refuse those strips in every frame.
    Every frame also has the 1e9 patch (refused by every form) and the NaN patch (NaN rounds to 0: admitted)."""
    f = edge_flow(k, (127, -128)) if k < 2 else far_flow(k - 2, 1)
    for axis in range(2):
        f[BLOCKS[axis][128] + (axis,)] += F32((128 + k) / 4.0)
        f[BLOCKS[axis][-129] + (axis,)] += F32((-129 - k) / 4.0)
    f[NAN_PATCH] = np.nan
    f[HUGE_PATCH] = 1e9
    return f


# constant flows that put the first raw site of the first live pixel on column / row 0 (-3.5: qx = 16 - 14 - 2) and the last
# site of the last live pixel on the frame's last column / row (+3.5: qx = 4 W - 17 + 14 - 2 = 4 W - 5); a quarter pixel more
# and the outermost strips are refused
SITE_SHIFTS = ((-3.5, -3.5), (3.5, 3.5), (-3.75, 3.5), (3.75, -3.75))
