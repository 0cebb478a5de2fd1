"""The warp+fuse tile kernel's LDS certainty layout, raw-site addressing and fast-path admission (accumulate_fast.hip:
certainty as one plane per CFA position, raw sites at 32-bit lane offsets, the 16-bit range test implied by the 8-bit window) against the oracle's frame-by-frame accumulateSuperResFull.

Every case goes through mfsr_accumulateSuperResFullN on guarded buffers at the ragged shape of
test_accumulate_groups_of_three_and_four (328 x 104: the last 256-pixel tile is partial, the rows are no multiple of 16), with
that test's tolerance (rtol = atol = 3e-5).  What the cases add is inputs chosen so that a wrong certainty plane, a wrong
mask row or column, a wrong raw row or a wrong admission decision changes the result:
  * flows whose rounded HR value changes parity from texel to texel and row to row (a wave then reads two certainty planes
    at once) next to flows that are constant over a frame (one plane per wave), over all four parity combinations;
  * certainty texels whose channels all differ, saturated rows next to unsaturated ones, isolated texels on the first and
    last columns of a tile's 66-column footprint;
  * strips exactly on and one past the 8-bit window around the tile's own flow, frames shifted by +-32000 / +-32001 HR
    pixels, non-finite and huge flows;
  * raw sites on the first and last admitted rows and columns of the frame.
"""
import numpy as np
import pytest

from tests.kernels import F3, Tex, pitch_of
from tests.test_parity_kernels import PATTERNS, _accum_inputs, _accumulate_group_hip, _kernel_field, rng

pytestmark = pytest.mark.gpu

W, H = 328, 104
TOL = dict(rtol=3e-5, atol=3e-5)
WHITE, BLACK = [3839, 3700, 3900], [256, 260, 250]


def _field_size(field, s):
    return (H // 2, W // 2) if (field == "quarter" or s == 4) else (H, W)


def _run(orc, hip, pat, frames, kp, field, s, seed):
    """frames: (raw, mask, flow) -> both accumulator sets of the oracle and of the group launch, compared."""
    cfa = [1, 1, 1, 1] if pat == "MONO" else PATTERNS[pat]
    orc.set_cfa(cfa)
    hip.set_cfa(cfa)
    white, black = F3(WHITE), F3(BLACK)
    fh, fw = _field_size(field, s)
    _, oi, ow, _ = _accum_inputs(seed, W, H, W * s, H * s)
    hi0, hw0 = oi.copy(), ow.copy()
    for raw, m, sh in frames:
        orc.call("accumulateSuperResFull", raw, oi, ow, m, Tex(kp), Tex(sh), white, black, W, H, s, pitch_of(oi), pitch_of(m))
    hi, hw_ = _accumulate_group_hip(hip, frames, kp, fw, fh, W, H, s, white, black, hi0, hw0, 0)
    np.testing.assert_allclose(hw_, ow, **TOL)
    np.testing.assert_allclose(hi, oi, **TOL)
    assert np.abs(hw_ - hw0).max() > 0.5   # the launch accumulated something


def _smooth_kernel_field(seed, fh, fw):
    # every texel positive definite: the strips are admitted or not by their flow alone
    r = rng(seed)
    k = np.zeros((fh, fw, 4), np.float32)
    k[..., 0] = r.uniform(0.05, 3.0, (fh, fw))
    k[..., 1] = r.uniform(0.05, 3.0, (fh, fw))
    k[..., 2] = r.uniform(-0.2, 0.2, (fh, fw))
    return k


def _parity_flow(k, alternating, fh, fw):
    """Frame k's flow.  2 * flow is a whole number on every texel: base parity (k & 1, (k >> 1) & 1), and, if alternating, one
    more HR pixel on every other texel column (x) / texel row (y) -- so the rounded value of the pixels between two texels
    takes both parities inside one wave.  Otherwise the frame's flow is one constant."""
    yy, xx = np.mgrid[0:fh, 0:fw]
    bx, by = 1.0 - 2.0 * k + 0.5 * (k & 1), -2.0 + 1.0 * k + 0.5 * ((k >> 1) & 1)
    fx = np.full((fh, fw), bx) + (0.5 * (xx & 1) if alternating else 0.0)
    fy = np.full((fh, fw), by) + (0.5 * (yy & 1) if alternating else 0.0)
    return np.ascontiguousarray(np.stack([fx, fy], -1).astype(np.float32))


PARITY_CASES = [(n, "quarter", 2, pat) for pat in ("RGGB", "GBRG", "BGGR") for n in (1, 2, 3, 4)] + \
               [(3, "half", 2, "MONO"), (4, "half", 2, "MONO"), (4, "quarter", 4, "RGGB")]


@pytest.mark.parametrize("n,field,s,pat", PARITY_CASES)
def test_parity_mix(orc, hip, n, field, s, pat):
    """Every certainty plane, both polarities of each parity offset, one and two planes per wave."""
    fh, fw = _field_size(field, s)
    kp = _kernel_field(410, fh, fw, 4)
    frames = []
    for k in range(n):
        raw, _, _, mask = _accum_inputs(411 + k, W, H, W * s, H * s, nan_frac=0.01)
        frames.append((raw, mask, _parity_flow(k, (k + n) & 1, fh, fw)))
    _run(orc, hip, pat, frames, kp, field, s, 419)


def _plane_masks():
    """Four certainty fields (mh x mw x 4, channels R G B _): ones with isolated three-valued texels on the footprint edges of
    the tiles; bands of saturated and random rows; random everywhere; ones."""
    mh, mw = (H + 1) // 2, (W + 1) // 2
    r = rng(430)
    ones = np.ones((mh, mw, 4), np.float32)
    dots = ones.copy()
    # footprint column c of tile column b is mask column 64 b - 1 + c: c = 0, 1, 64, 65 for b = 0, 1, 2 (inside the field)
    cols = [0, 63, 64, 65, 127, 128, 129, mw - 1]
    for i, gy in enumerate([0, 4, 5, 6, 25, 26, mh - 6, mh - 5, mh - 1]):
        for j, gx in enumerate(cols):
            if (i + j) % 3 != 2:
                dots[gy, gx, :3] = [0.25 + 0.01 * i, 0.5 + 0.01 * j, 0.75 - 0.01 * (i + j)]
    dots[7, 64, 1] = np.nan          # sanitised to 0
    rand = r.random((mh, mw, 4), dtype=np.float32)
    bands = ones.copy()
    rows = (np.arange(mh) // 3) % 2 == 1
    bands[rows] = rand[rows]
    return [dots, bands, r.random((mh, mw, 4), dtype=np.float32), ones]


@pytest.mark.parametrize("n,pat", [(4, "RGGB"), (3, "GBRG"), (2, "BGGR"), (1, "RGGB")])
def test_plane_addressing(orc, hip, n, pat):
    """Texels whose channels all differ: a read from the wrong plane, mask row, frame or column cannot pass.  Saturated waves
    (strip_pixel_sat) sit next to waves that read the planes."""
    fh, fw = _field_size("quarter", 2)
    kp = _kernel_field(431, fh, fw, 4)
    masks = _plane_masks()
    frames = []
    for k in range(n):
        raw, _, _, _ = _accum_inputs(432 + k, W, H, W * 2, H * 2)
        frames.append((raw, masks[(k + n) % 4], _parity_flow(k + 1, k & 1, fh, fw)))
    _run(orc, hip, pat, frames, kp, "quarter", 2, 439)


def _plateau(flow, rows, cols, dx, dy):
    flow[rows, cols, 0] += dx
    flow[rows, cols, 1] += dy


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("n,pat", [(4, "RGGB"), (3, "GBRG")])
def test_admission_edge(orc, hip, n, pat, sign):
    """The four-workgroup kernels keep a strip's rounded flow in 8 bits relative to the rounded flow of the tile's centre
    texel (field column 64 b + 32) and admit d in [-128, 127].  Plateaus of three texels put whole strips at d = 127, 128,
    -128 and -129 on either axis, clear of the centre texels and with every tap still inside the frame; two frames are
    shifted as a whole by +-32000 and +-32001 HR pixels (the clamp of the tile's own flow); one patch is NaN, one 1e9.
    Those two frames put every tap outside the frame: they exercise the clamp and the refusal (the straight arithmetic for the
    whole frame), and what the launch accumulates on the fast path comes from the first two frames."""
    fh, fw = _field_size("quarter", 2)
    kp = _smooth_kernel_field(450, fh, fw)
    flows = []
    # x axis: positive offsets on the left (X + 129 stays inside 656 pixels), negative ones on the right
    f = np.zeros((fh, fw, 2), np.float32) + np.float32([1.0, -0.5])
    _plateau(f, slice(6, 10), slice(8, 11), 63.5, 0.0)      # d = +127
    _plateau(f, slice(12, 16), slice(8, 11), 64.0, 0.0)     # d = +128
    _plateau(f, slice(6, 10), slice(70, 73), -64.0, 0.0)    # d = -128
    _plateau(f, slice(12, 16), slice(70, 73), -64.5, 0.0)   # d = -129
    flows.append(f)
    # y axis: positive offsets at the top (Y + 129 stays inside 208 rows), negative ones at the bottom
    f = np.zeros((fh, fw, 2), np.float32) + np.float32([-1.5, 1.0])
    _plateau(f, slice(5, 8), slice(4, 8), 0.0, 63.5)
    _plateau(f, slice(5, 8), slice(40, 44), 0.0, 64.0)
    _plateau(f, slice(40, 43), slice(4, 8), 0.0, -64.0)
    _plateau(f, slice(40, 43), slice(40, 44), 0.0, -64.5)
    f[20:23, 60:63] = np.nan
    f[30:33, 20:23] = 1e9
    flows.append(f)
    # whole frames at the clamp of the tile's own flow: round(2 * flow) = +-32000 and +-32001
    flows.append(np.zeros((fh, fw, 2), np.float32) + np.float32([sign * 16000.0, -sign * 16000.5]))
    flows.append(np.zeros((fh, fw, 2), np.float32) + np.float32([-sign * 16000.5, sign * 16000.0]))
    frames = []
    for k in range(n):
        raw, _, _, mask = _accum_inputs(451 + k, W, H, W * 2, H * 2, nan_frac=0.01)
        frames.append((raw, mask, np.ascontiguousarray(flows[k])))
    _run(orc, hip, pat, frames, kp, "quarter", 2, 459)


@pytest.mark.parametrize("n,pat", [(4, "RGGB"), (2, "BGGR"), (1, "GBRG")])
def test_raw_sites_at_the_frame_edges(orc, hip, n, pat):
    """A strip is admitted when X + sx - 2 lies in [0, 2 W - 5] (and the same in y).  The tile kernel's first live pixel is
    16: a flow of -7 puts its first raw site on column / row 0, +7 puts the last site of the last live pixel on the frame's
    last column / row; half a pixel more and the same strips are refused.  The raw frames sit between guard bands."""
    fh, fw = _field_size("quarter", 2)
    kp = _smooth_kernel_field(470, fh, fw)
    shifts = [(-7.0, -7.0), (7.0, 7.0), (-7.5, 7.0), (7.5, -7.5)]
    frames = []
    for k in range(n):
        raw, _, _, mask = _accum_inputs(471 + k, W, H, W * 2, H * 2, nan_frac=0.01)
        frames.append((raw, mask, np.ascontiguousarray(np.zeros((fh, fw, 2), np.float32) + np.float32(shifts[(k + n) % 4]))))
    _run(orc, hip, pat, frames, kp, "quarter", 2, 479)
