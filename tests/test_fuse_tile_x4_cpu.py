"""The inputs of tests/test_fuse_tile_x4_gpu.py do what they claim: conditions on the inputs alone, checked with the float32
model of the admission rule (tests/fuse_x4_ref.py) and, for the frames that lie off the frame as a whole, with the oracle.
No GPU.  The figures in the comments were computed with exactly these inputs."""
import numpy as np
import pytest

from tests import fuse_x4_ref as fx
from tests.fuse_x4_ref import FH, FW, H, HRH, HRW, W, FlowModel, form_of, live_strips, per_strip, plateau_strips
from tests.kernels import F3, Tex, pitch_of
from tests.test_fuse_tile_layout_gpu import BLACK, WHITE, _smooth_kernel_field
from tests.test_parity_kernels import PATTERNS, _accum_inputs

LIVE = live_strips()
FORMS = (1, 2, 3)
NO_TIE = 1.0 / 32      # 4 u is at least this far from a half-integer: no rounding of the interpolation can move the result


def _pixels_of(strips):
    return np.repeat(strips, 4, axis=1)


def test_the_model_on_exact_fields():
    """A constant field is interpolated exactly, round2i is roundf with the hardware's conversion, and the tile's centre texel is
    field column 64 b + 32 of the pixel's own field row."""
    m = FlowModel(fx.const_flow(1.25, -0.75))
    assert np.all(m.sx == 5) and np.all(m.sy == -3) and np.all(m.dx == 0) and np.all(m.dy == 0)
    assert list(fx.round2i(np.float32([0.5, -0.5, 1.5, -2.5, 0.49999997, np.nan, 1e10, -1e10, np.inf]))) == \
        [1, -1, 2, -3, 0, 0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1]
    f = fx.const_flow(0.0, 0.0)
    f[3, 32], f[3, 96], f[3, 160] = (1.0, 2.0), (3.0, 4.0), (9000.0, -9000.0)
    m = FlowModel(f)
    for X, bs in ((0, (4, 8)), (511, (4, 8)), (512, (12, 16)), (1023, (12, 16)), (1024, (32000, -32000)), (1311, (32000, -32000))):
        assert (m.bsx[24, X], m.bsy[31, X]) == bs and m.bsx[23, X] == 0 and m.bsx[32, X] == 0
    # the texel centres: pixel 8 c + 4 is 1/16 past texel c, and the fractions are the odd sixteenths
    i0, i1, a = fx.tex_axis(HRW, FW)
    assert i0[8 * 5 + 4] == 5 and i1[8 * 5 + 4] == 6 and i0[8 * 5 + 3] == 4
    assert np.allclose(a[16:HRW - 16] * 16 % 2, 1.0, atol=1e-3)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_residue_blocks_cover_every_phase(k):
    """Among the strips that every form admits, each position in the certainty cell meets each phase of the first tap modulo 8,
    on both axes: the 64 (X & 7, qx & 7) pairs select among the compile-time K8 bodies and the runtime mx[] masks and raw
    column parity, the 64 (Y & 7, qy & 7) pairs among the mask rows, my[] and flip.  Computed: 64 and 64 for k = 0..3, every
    live strip admitted by every form (122880 of 122880), 4 u at least 0.0625 from a tie."""
    m = FlowModel(fx.residue_flow(k))
    assert m.tie.min() >= NO_TIE
    for form in FORMS:
        adm = m.admitted(form) & LIVE
        print(f"residue blocks, frame {k}, form {form}: {adm.sum()} of {LIVE.sum()} live strips admitted")
        assert adm.sum() >= 0.9 * LIVE.sum()
    sel = _pixels_of(m.admitted(3) & LIVE)
    yy, xx = np.mgrid[0:HRH, 0:HRW]
    pairs_x = set(zip((xx[sel] & 7).tolist(), (m.qx[sel] & 7).tolist()))
    pairs_y = set(zip((yy[sel] & 7).tolist(), (m.qy[sel] & 7).tolist()))
    assert len(pairs_x) == 64 and len(pairs_y) == 64


def test_residue_frames_of_a_group_disagree():
    """Frame k's blocks are rotated by k in x and 3 k in y: two frames of a group have different phases modulo 8 on both axes
    at every live pixel but a few in the 8-pixel zone where the blocks wrap from +4 to -3 (computed: 0.16 % in x, 0.52 % in y)."""
    ms = [FlowModel(fx.residue_flow(k)) for k in range(4)]
    live = _pixels_of(LIVE)
    for i in range(4):
        for j in range(i + 1, 4):
            assert np.mean(((ms[i].sx - ms[j].sx) & 7)[live] == 0) < 0.01 and np.mean(((ms[i].sy - ms[j].sy) & 7)[live] == 0) < 0.01


@pytest.mark.parametrize("ds", [fx.EDGE_D, fx.EDGE_D2])
@pytest.mark.parametrize("axis", [0, 1])
def test_plateaus_sit_on_the_admission_edge(axis, ds):
    """Each of d = 127, 128, -128, -129 (and 129, -127 for the two-frame form) has 96 live strips whose four pixels are all at
    exactly d on that axis with every tap inside the frame.  Forms 3 / 4 take d in [-128, 127] only; forms 1 and 2 take all.
    The only pixels near a rounding tie are in the corner zones of the +-128 plateaus (128 a b with a, b odd sixteenths is a
    half-integer): 0.13 % of the live strips (0.16 % with the two-frame form's plateaus), none of them a plateau strip."""
    m = FlowModel(fx.edge_flow(axis, ds, patches=axis == 1))
    d_own, d_other = ((m.dx, m.dy), (m.dy, m.dx))[axis]
    tie = per_strip(m.tie).min(-1)
    for d in ds:
        s = plateau_strips(fx.BLOCKS[axis][d]) & LIVE
        assert s.sum() == 96 > 0
        assert np.all(per_strip(d_own)[s] == d) and np.all(per_strip(d_other)[s] == 0)
        assert per_strip(m.inside)[s].all()
        assert tie[s].min() >= NO_TIE
        assert m.admitted(1)[s].all() and m.admitted(2)[s].all()
        assert m.admitted(3)[s].all() if -128 <= d <= 127 else not m.admitted(3)[s].any()
    near = (tie < NO_TIE) & LIVE
    print(f"axis {axis}: {near.sum()} of {LIVE.sum()} live strips hold a pixel within {NO_TIE} of a tie")
    assert near.sum() <= 0.002 * LIVE.sum()


def test_frame_edges_admit_the_outermost_sites():
    """(-3.5, -3.5) and (+3.5, +3.5) admit every live strip, and the admitted first taps reach 0 and exactly 4 W - 5 = 1307 /
    4 H - 5 = 411; a quarter pixel more refuses the outermost strips (computed: 0.31 % for (-3.75, 3.5), 0.57 % for (3.75, -3.75))."""
    lo, hi = FlowModel(fx.const_flow(*fx.SITE_SHIFTS[0])), FlowModel(fx.const_flow(*fx.SITE_SHIFTS[1]))
    for form in FORMS:
        assert np.array_equal(lo.admitted(form) & LIVE, LIVE) and np.array_equal(hi.admitted(form) & LIVE, LIVE)
    live = _pixels_of(LIVE)
    assert lo.qx[live].min() == 0 and lo.qy[live].min() == 0
    assert hi.qx[live].max() == 4 * W - 5 == 1307 and hi.qy[live].max() == 4 * H - 5 == 411
    for sh in fx.SITE_SHIFTS[2:]:
        m = FlowModel(fx.const_flow(*sh))
        for form in FORMS:
            refused = LIVE & ~m.admitted(form)
            print(f"flow {sh}, form {form}: {refused.sum() / LIVE.sum():.4%} of the live strips refused")
            assert 0 < refused.sum() < 0.01 * LIVE.sum()
        assert m.tie.min() >= NO_TIE


@pytest.mark.parametrize("sign", [1, -1])
def test_far_frames_sit_on_the_clamp_and_are_refused(sign):
    """4 * flow = +-32000 is the clamp itself (d = 0), -+32001 one past it (d = -+1): both pass the 8-bit window and the 2^15
    bound, and every strip is refused because its taps are outside the frame."""
    for which in (0, 1):
        m = FlowModel(fx.far_flow(which, sign))
        assert set(np.unique(np.abs(m.bsx))) == {32000} and set(np.unique(np.abs(m.bsy))) == {32000}
        assert sorted(np.unique(np.abs(np.concatenate([m.dx.ravel(), m.dy.ravel()])))) == [0, 1]
        assert not m.inside.any()
        for form in FORMS:
            assert not (m.admitted(form) & LIVE).any()


@pytest.mark.parametrize("n", [1, 3, 4])
def test_refused_group_is_refused_in_every_frame(n):
    """The group that shows the fast path ran: the plateaus at the texels of d = 128 and -129 are refused in every frame of a
    three- or four-frame group (640 strips with the 1e9 patch's), every other plateau is admitted in some frame; the one-frame
    form has no 8-bit window, admits every plateau, and refuses the 1e9 patch only (256 strips).  A NaN flow rounds to 0: admitted."""
    ms = [FlowModel(fx.refused_group_flow(k)) for k in range(n)]
    some = np.any([m.admitted(form_of(n)) for m in ms], axis=0)
    never = ~some & LIVE
    print(f"group of {n}: {never.sum()} live strips refused in every frame")
    assert never.sum() == (256 if n == 1 else 640)
    for axis in range(2):
        for d in fx.EDGE_D:
            s = plateau_strips(fx.BLOCKS[axis][d]) & LIVE
            assert s.sum() == 96
            if n > 1 and d in (128, -129):
                assert never[s].all()
                for k, m in enumerate(ms[:2]):
                    assert np.all(per_strip((m.dx, m.dy)[axis])[s] == (128 + k if d > 0 else -129 - k)) and per_strip(m.inside)[s].all()
            else:
                assert some[s].all()
    huge = plateau_strips(fx.HUGE_PATCH) & LIVE
    nan = plateau_strips(fx.NAN_PATCH) & LIVE
    assert huge.sum() > 0 and never[huge].all() and nan.sum() > 0 and some[nan].all()


@pytest.mark.parametrize("flow", [(8000.0, -8000.25), (-8000.25, 8000.0), (-8000.0, 8000.25), (1e9, 1e9), (np.nan, np.nan)])
def test_a_frame_off_the_frame_still_contributes(orc, flow):
    """The oracle clamps every tap to the frame: a frame whose flow is +-8000 or +-8000.25 LR pixels, 1e9 or NaN changes the
    accumulators.  No case may treat such a frame as contributing nothing."""
    orc.set_cfa(PATTERNS["RGGB"])
    raw, oi, ow, mask = _accum_inputs(451, W, H, HRW, HRH)
    i0, w0 = oi.copy(), ow.copy()
    kp = _smooth_kernel_field(450, FH, FW)
    sh = fx.const_flow(*flow)
    orc.call("accumulateSuperResFull", raw, oi, ow, mask, Tex(kp), Tex(sh), F3(WHITE), F3(BLACK), W, H, 4, pitch_of(oi), pitch_of(mask))
    live = np.s_[16:HRH - 16, 16:HRW - 16]
    changed = (ow[live] != w0[live]).any(-1)
    print(f"flow {flow}: {changed.mean():.2%} of the live pixels' weight sums changed, by up to {np.abs(ow - w0)[live].max():.3g}")
    assert changed.mean() > 0.5 and np.abs(ow - w0)[live].max() > 0.5 and (oi[live] != i0[live]).any()
