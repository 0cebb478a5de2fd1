"""k_lkSweep (csrc/lk_fused.hip, behind mfsr_lucasKanadeSweepBatch) in guarded, padded buffers.

One harness, ``run_sweep``: mfsr_CreateFlowFieldWarped and then the sweep iterations of 1 .. 4 frames, with EVERY buffer a guarded
upload (tests/kernels.py::guarded_upload) whose rows are padded to three different pitches -- pitchShift, pitchImg and pitchSD
differ, pitchSD the smaller of the two image pitches, so one taken for another reads other pixels but stays inside the
allocation.  Input padding is 0xFF (NaN: a read of it shows in np.isfinite and in every bit comparison), outputs start as the
sentinel byte everywhere, so a pixel the kernel leaves unwritten is found as well as one written twice in the wrong place.
After the last launch: every guard, the read-only inputs unchanged, all output padding intact, and every output buffer holding
byte for byte what its last writer left (the planes no launch was given still all sentinel).

The oracle side is the chain of tests/test_parity_kernels.py::test_lucasKanadeSweepBatch_vs_oracle_chain on dense arrays:
CreateFlowFieldFromTiles, then per iteration WarpingKernel -> ComputeDerivativesKernel -> lucasKanadeOptim.

Bands are never set from here: they come from the shapes and are confirmed through mfsr_lucasKanadeSweepBand; with MFSR_LK_BAND
in the environment those assertions fail, which is intended.
"""
import numpy as np
import pytest

from tests.burst_compare import flow_difference_report
from tests.kernels import F2, Tex
from tests.test_kernel_edges_gpu import POISON, SENTINEL, DevBufs, _pad2d, padded_pitch
from tests.test_parity_kernels import _smooth_image, assert_bitexact, rng

pytestmark = pytest.mark.gpu

UNWRITTEN = np.uint32(SENTINEL * 0x01010101)
SHIFTS = [(10, 7), (6, 9), (11, 8), (7, 6)]      # crop offsets (dx, dy) of the moved frames: the true flow is (8 - dx, 8 - dy)
TCX, TCY = 5, 4                                  # tile-shift grid every case interpolates its first flow from
MIN_DET = 1e-4
E_INVALID, E_UNSUPPORTED = -1, -2


# ---------------------------------------------------------------- inputs
class LkCase:
    """A reference image, ``nf`` moved crops of the same smooth image and their tile shifts (the true translation +- 0.4 px)."""

    def __init__(self, hw, W, H, nf, seed, image_seed=63):
        r = rng(seed)
        base = _smooth_image(image_seed, H + 16, W + 16)
        self.hw, self.W, self.H, self.nf = hw, W, H, nf
        self.ref = np.ascontiguousarray(base[8:8 + H, 8:8 + W])
        self.movs, self.tiles, self.true = [], [], []
        for k in range(nf):
            dx, dy = SHIFTS[k]
            self.movs.append(np.ascontiguousarray(base[dy:dy + H, dx:dx + W]))
            self.true.append(np.array([8 - dx, 8 - dy], np.float32))       # ref(p) = moved(p + u)
            self.tiles.append((self.true[k] + r.uniform(-0.4, 0.4, (TCY, TCX, 2))).astype(np.float32))


def vw(hw):
    return 64 - 2 * (hw + 2)          # columns a wavefront produces


# h -> (H, seed): three strips, the last owning one column (W = 2 VW + 1); five or nine bands of 8 rows, the last one row.  H and
# the seed are whatever tests/test_lk_band_cpu.py::test_sweep_inputs_are_well_conditioned accepts, from the oracle alone.
HALF_WINDOWS = {1: (41, 11), 2: (73, 12), 3: (41, 13), 4: (73, 14), 5: (41, 15), 6: (73, 16), 7: (41, 17)}


def half_window_case(hw):
    H, seed = HALF_WINDOWS[hw]
    return LkCase(hw, 2 * vw(hw) + 1, H, (hw - 1) % 4 + 1, seed)


HOSTILE_FRAME = 2


def hostile_case():
    """Four frames at 109 x 41, h = 3.  The first two tiles of frame 2's top tile row carry flows of up to +-3 image sizes: they
    are interpolated into columns 0 .. 54 of rows 0 .. 14, so every lane of the first strip's waves (columns 0 .. 53) samples
    the moved image through MIRROR addressing there, rows away from the border."""
    c = LkCase(3, 109, 41, 4, 23)
    c.tiles[HOSTILE_FRAME][0, 0] = [3.0 * c.W, -3.0 * c.H]
    c.tiles[HOSTILE_FRAME][0, 1] = [-2.5 * c.W, 1.5 * c.H]
    return c


def calm(case, k, reach=0):
    """Pixels of frame ``k`` farther than ``reach`` px from every pixel a hostile tile shift (more than 1 px off the true shift)
    is interpolated into: all of them in every case but hostile_case()."""
    ty, tx = (np.arange(case.H) + 0.5) / case.H * TCY - 0.5, (np.arange(case.W) + 0.5) / case.W * TCX - 0.5
    dev = np.abs(case.tiles[k] - case.true[k]).max(-1) > 1.0
    near = np.zeros((case.H, case.W), bool)
    for j, i in np.argwhere(dev):
        near |= (np.abs(ty - j) < 1.0 + reach * TCY / case.H)[:, None] & (np.abs(tx - i) < 1.0 + reach * TCX / case.W)[None, :]
    return ~near


def distance_to_true(case, k, flow):
    """Mean |flow - true shift| over the interior (12 px from the border, as the sibling test) -- of the pixels no hostile first
    flow can have reached in three iterations (h + 2 px each): convergence is a statement about flows that start near the truth."""
    m = calm(case, k, 3 * (case.hw + 2))[12:-12, 12:-12]
    assert m.mean() > 0.25
    return float(np.abs(flow[12:-12, 12:-12] - case.true[k])[m].mean())


def oracle_chain(orc, case, k, iters, flow0=None):
    """-> the flow after each of ``iters`` oracle iterations of frame ``k`` (unscaled), from CreateFlowFieldFromTiles or flow0."""
    W, H = case.W, case.H
    flow = np.zeros((H, W, 2), np.float32)
    if flow0 is None:
        orc.call("CreateFlowFieldFromTiles", flow, Tex(case.tiles[k]), 16, TCX, TCY, W, H, W * 8, F2([0, 0]), 0.0)
    else:
        flow[...] = flow0
    out = []
    for _ in range(iters):
        warped = oracle_warp(orc, case, k, flow)
        Ix, Iy, Iz = (np.zeros((H, W), np.float32) for _ in range(3))
        orc.call("ComputeDerivativesKernel", W, H, W * 4, Ix, Iy, Iz, Tex(warped), Tex(case.ref))
        orc.call("lucasKanadeOptim", flow, Ix, Iy, Iz, W * 8, W * 4, W, H, case.hw, MIN_DET)
        out.append(flow.copy())
    return out


def oracle_warp(orc, case, k, flow):
    warped = np.zeros((case.H, case.W), np.float32)
    orc.call("WarpingKernel", case.W, case.H, case.W * 4, Tex(np.ascontiguousarray(flow)), warped, Tex(case.movs[k]))   # MIRROR (REF_TEX_ADDRESS)
    return warped


# The oracle's WarpingKernel does not read a pixel's flow, it FETCHES it: a bilinear sample of the flow texture at the pixel's
# centre, ((i + 0.5) / n) * n - 0.5 in float32 (opticalFlow.cu:36).  At most indices that is i again and the sample is the
# pixel's own flow, bit for bit.  At a few it is one ulp off i, and the exact-float bilinear of the oracle then mixes ~1e-5 of
# the neighbour's flow in (the reference's texture unit, with its 8-bit fraction, does not).  The LK kernels warp a pixel by
# the flow they hold for it, so at those rows and columns -- known from the image size alone -- the planes differ from the
# oracle's by some 1e-7 (Lucas-Kanade section).  ``warp_own_flow`` is the same warp with the flow read, not fetched.
def fetch_is_inexact(n):
    """-> bool[n]: indices whose texel centre does not come back from ((i + 0.5) / n) * n - 0.5 in float32."""
    i = np.arange(n, dtype=np.float32)
    return ((i + np.float32(0.5)) / np.float32(n) * np.float32(n) - np.float32(0.5)).astype(np.float32) != i


def warp_own_flow(img, flow):
    """WarpingKernel's arithmetic (opticalFlow.cu:38-43 through the MIRROR texture stand-in, oracle/oracle_common.h) in numpy
    float32, one rounding per operation, with every pixel's OWN flow.  tests/test_lk_band_cpu.py pins it to the oracle's
    WarpingKernel, bit for bit wherever that fetches a pixel's own flow.  Finite flows only."""
    f32, one, half = np.float32, np.float32(1.0), np.float32(0.5)
    H, W = img.shape
    gx, gy = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))

    def mirror(x):
        f = np.floor(x)
        fr = x - f
        return np.where((f.astype(np.int64) & 1) == 1, one - fr, fr)

    u = mirror(((gx + half) + flow[..., 0]) / f32(W))
    v = mirror(((gy + half) + flow[..., 1]) / f32(H))
    xB, yB = u * f32(W) - half, v * f32(H) - half
    fx, fy = np.floor(xB), np.floor(yB)
    a, b = xB - fx, yB - fy
    ix, iy = fx.astype(np.int64), fy.astype(np.int64)
    i0, i1, j0, j1 = np.clip(ix, 0, W - 1), np.clip(ix + 1, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iy + 1, 0, H - 1)
    r = (((one - a) * (one - b) * img[j0, i0] + a * (one - b) * img[j0, i1]) + (one - a) * b * img[j1, i0]) + a * b * img[j1, i1]
    assert r.dtype == np.float32
    return r


def own_error_of_the_oracle(orc, case, k):
    """max |the oracle's flow after one iteration - the same update evaluated in float64| over frame ``k``: how far ONE float32
    evaluation order is from the exact value of opticalFlow.cu:215-320 on these inputs (the oracle's own float32 derivative
    images taken as given).  M = sum of grad grad^T over the window is symmetric, so V S^+ U^T is its pseudo-inverse."""
    W, H, h = case.W, case.H, case.hw
    flow = np.zeros((H, W, 2), np.float32)
    orc.call("CreateFlowFieldFromTiles", flow, Tex(case.tiles[k]), 16, TCX, TCY, W, H, W * 8, F2([0, 0]), 0.0)
    warped = oracle_warp(orc, case, k, flow)
    Ix, Iy, It = (np.zeros((H, W), np.float32) for _ in range(3))
    orc.call("ComputeDerivativesKernel", W, H, W * 4, Ix, Iy, It, Tex(warped), Tex(case.ref))
    got = flow.copy()
    orc.call("lucasKanadeOptim", got, Ix, Iy, It, W * 8, W * 4, W, H, h, MIN_DET)
    x, y, t = Ix.astype(np.float64), Iy.astype(np.float64), It.astype(np.float64)

    def box(p):
        c = np.cumsum(np.cumsum(np.pad(p, ((1, 0), (1, 0))), 0), 1)
        n = 2 * h + 1
        return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]        # window sums of the pixels h .. size - h - 1

    a, b, d, p, q = box(x * x), box(x * y), box(y * y), box(x * t), box(y * t)
    det = a * d - b * b
    l1 = (a + d) / 2 + np.sqrt(((a - d) / 2) ** 2 + b * b)
    ok = (l1 >= MIN_DET) & (det > 0)
    det = np.where(ok, det, 1.0)
    want = flow.astype(np.float64)
    want[h:H - h, h:W - h, 0] += np.where(ok, (d * p - b * q) / det, 0.0)
    want[h:H - h, h:W - h, 1] += np.where(ok, (a * q - b * p) / det, 0.0)
    return float(np.abs(got - want).max())


def conditioned_case(orc, hw, W, H, nf, seed0):
    """The first seed from ``seed0`` at which the oracle's own float32 error (above) stays under HALF the tolerance of one
    iteration (atol 1e-4, c_lkFused's) at every pixel of every frame: where one float32 evaluation order is off the exact
    value by more, two correct ones can differ by the tolerance, and the input cannot tell a wrong kernel from a right one.
    Decided from the oracle alone (3 x 3 windows at a handful of rows are where it matters)."""
    for seed in range(seed0, seed0 + 40):
        case = LkCase(hw, W, H, nf, seed, image_seed=seed)
        if max(own_error_of_the_oracle(orc, case, k) for k in range(nf)) <= 0.5e-4:
            return case
    raise AssertionError(f"no seed from {seed0} for h={hw} {W}x{H} x{nf}")


# ---------------------------------------------------------------- the harness
def sweep_pitches(W):
    """-> (pitchShift, pitchImg, pitchSD): three different padded pitches, pitchSD < pitchImg, none a multiple of 64."""
    sd = padded_pitch(4 * W, 4)
    img = sd + 4                      # padded_pitch would make the two equal: one more alignment step
    while img % 64 == 0:
        img += 4
    sh = padded_pitch(8 * W, 8)
    while sh in (sd, img) or sh % 64 == 0:
        sh += 8
    assert len({sh, img, sd}) == 3 and sd < img and sd > 4 * W and sh > 8 * W
    return sh, img, sd


def _blank(shape):
    return np.full(shape, UNWRITTEN, np.uint32).view(np.float32)


class SweepRun:
    """What ``run_sweep`` returns, by frame index of the case: flow0 / S0 / D0 (what the iterations start from), and per iteration
    ``it`` flow[it][k], S[it][k], D[it][k] (the planes only where that iteration wrote them)."""

    def __init__(self):
        self.flow0, self.S0, self.D0 = {}, {}, {}
        self.flow, self.S, self.D = [], [], []


class _Bufs:
    """Guarded, padded device buffers by name, with mid-run downloads."""

    def __init__(self, hip):
        self.hip, self.D, self.by = hip, DevBufs(hip), {}

    def up(self, name, a, pitch=None, readonly=False):
        buf, p, rowb = _pad2d(a, POISON if readonly else SENTINEL, pitch=pitch)
        ptr = self.D.up(buf, readonly)
        self.by[name] = dict(t=self.D.items[-1][1], buf=buf, rowb=rowb, shape=a.shape, last=buf.copy(), ptr=ptr, pitch=p)
        return ptr

    def get(self, name, what):
        """Download an output: its padding intact, no pixel left as uploaded -> the dense float array."""
        b = self.by[name]
        full = b["t"].cpu().numpy().reshape(b["buf"].shape)
        bad = np.argwhere(full[:, b["rowb"]:] != SENTINEL)
        assert bad.size == 0, f"{what}: pitch padding of {name} changed, first at row {bad[0][0]}, byte {b['rowb'] + bad[0][1]} of the row"
        b["last"] = full
        dense = full[:, :b["rowb"]].copy().view(np.float32).reshape(b["shape"])
        left = np.argwhere(dense.view(np.uint32) == UNWRITTEN)
        assert left.size == 0, f"{what}: {len(left)} elements of {name} were never written, first at {tuple(left[0])}"
        return dense

    def put(self, name, a):
        b = self.by[name]
        buf, _, _ = _pad2d(a, SENTINEL, pitch=b["pitch"])
        b["t"].copy_(self.hip.torch.from_numpy(buf).reshape(b["t"].shape))
        b["last"] = buf

    def finish(self, what):
        self.D.finish(what)          # every guard; read-only inputs unchanged; outputs downloaded
        for name, b in self.by.items():
            bad = np.argwhere(b["buf"] != b["last"])
            assert bad.size == 0, (f"{what}: {name} no longer holds what its last writer left (never written: the sentinel), first at row "
                                   f"{bad[0][0]}, byte {bad[0][1]} of {b['rowb']} row bytes")


def run_sweep(hip, case, schedule, order=None, hostile=None, orc=None):
    """mfsr_CreateFlowFieldWarped per frame, then one mfsr_lucasKanadeSweepBatch per entry (outScale, planes out) of ``schedule``
    over the frames ``order`` (slot -> frame index of the case; default all, in order).  ``hostile``: {frame: function(flow) ->
    flow} applied to that frame's first flow field; where it changed the flow the planes are recomputed on the host by the
    oracle's warp (``orc``)."""
    L, capi, torch = hip.L, hip.capi, hip.torch
    W, H, hw = case.W, case.H, case.hw
    order = list(range(case.nf)) if order is None else list(order)
    n = len(order)
    assert all(p and s == 1.0 for s, p in schedule[:-1]), "every iteration but the last hands planes to the next"
    what = f"k_lkSweep h={hw} {W}x{H} frames {order}"
    pSh, pImg, pSD = sweep_pitches(W)
    B = _Bufs(hip)
    ref = B.up("ref", case.ref, pImg, True)
    mov, til, f, S, Dd = {}, {}, {}, {}, {}
    for k in order:
        mov[k] = B.up(f"moved{k}", case.movs[k], pImg, True)
        til[k] = B.up(f"tiles{k}", case.tiles[k], None, True)
        f[k] = [B.up(f"flow{k}.{j}", _blank((H, W, 2)), pSh) for j in range(2)]
        S[k] = [B.up(f"sum{k}.{j}", _blank((H, W)), pSD) for j in range(2)]
        Dd[k] = [B.up(f"diff{k}.{j}", _blank((H, W)), pSD) for j in range(2)]
    res = SweepRun()
    for k in order:
        L.CreateFlowFieldWarped(f[k][0], capi.Tex2D(til[k], B.by[f"tiles{k}"]["pitch"], TCX, TCY), W, H, pSh, capi.f2([0, 0]), 0.0, None,
                                ref, mov[k], pImg, S[k][0], Dd[k][0], pSD, None)
    torch.cuda.synchronize()
    for k in order:
        res.flow0[k], res.S0[k], res.D0[k] = (B.get(f"{nm}{k}.0", what + " first flow") for nm in ("flow", "sum", "diff"))
        if hostile and k in hostile:
            new = np.ascontiguousarray(hostile[k](res.flow0[k].copy()), np.float32)
            changed = (new.view(np.uint32) != res.flow0[k].view(np.uint32)).any(-1)
            warped = oracle_warp(orc, case, k, new)      # (orc_f2i is defined for NaN and saturates, as v_cvt_i32_f32 does)
            res.flow0[k] = new
            res.S0[k], res.D0[k] = np.where(changed, warped + case.ref, res.S0[k]), np.where(changed, warped - case.ref, res.D0[k])
            for nm, a in (("flow", res.flow0[k]), ("sum", res.S0[k]), ("diff", res.D0[k])):
                B.put(f"{nm}{k}.0", a)
    for it, (scale, planes) in enumerate(schedule):
        i, o = it & 1, (it & 1) ^ 1
        arr = (capi.LkFrame * n)()
        for slot, k in enumerate(order):
            arr[slot] = capi.LkFrame(f[k][i], f[k][o], mov[k], S[k][i], Dd[k][i], S[k][o] if planes else None, Dd[k][o] if planes else None)
        L.lucasKanadeSweepBatch(n, arr, ref, pSh, pImg, pSD, W, H, hw, MIN_DET, scale, None)
        torch.cuda.synchronize()
        w = f"{what} iteration {it}"
        res.flow.append({k: B.get(f"flow{k}.{o}", w) for k in order})
        res.S.append({k: B.get(f"sum{k}.{o}", w) for k in order} if planes else None)
        res.D.append({k: B.get(f"diff{k}.{o}", w) for k in order} if planes else None)
    B.finish(what)
    return res


# ---------------------------------------------------------------- assertions
def assert_planes(orc, case, k, flow, S, D, what):
    """(b) the planes an iteration hands on are the warp of the moved image under the kernel's OWN flow, + and - the reference, bit
    for bit at every pixel (ring rows and columns, each strip's first and last column): against warp_own_flow everywhere, and
    against the oracle's WarpingKernel fed that flow wherever its flow fetch is exact."""
    own = warp_own_flow(case.movs[k], flow)
    assert_bitexact(own + case.ref, S, f"{what} frame {k}: sumOut against warped + ref")
    assert_bitexact(own - case.ref, D, f"{what} frame {k}: diffOut against warped - ref")
    # ... and the oracle's WarpingKernel itself wherever it fetches a pixel's own flow (all but a few rows and columns)
    warped = oracle_warp(orc, case, k, flow)
    fetched = fetch_is_inexact(case.H)[:, None] | fetch_is_inexact(case.W)[None, :]
    assert fetched.mean() < 0.25
    n_off, d_off = 0, 0.0
    for nm, want, got in (("sumOut", warped + case.ref, S), ("diffOut", warped - case.ref, D)):
        off = want.view(np.uint32) != got.view(np.uint32)
        bad = np.argwhere(off & ~fetched)
        assert bad.size == 0, f"{what} frame {k}: {nm} against the oracle's WarpingKernel: {len(bad)} pixels differ, first at {tuple(bad[0])}"
        n_off, d_off = n_off + int(off.sum()), max(d_off, float(np.abs(want - got).max()))
    print(f"{what} frame {k}: planes bit-exact; the oracle's WarpingKernel, which fetches the flow inexactly at {fetched.sum()} of {fetched.size} "
          f"pixels, differs at {n_off} plane values there, by at most {d_off:.2e}")


def assert_ring(case, got, flow_in, scale, what):
    h = case.hw
    want = flow_in * np.float32(scale)          # exact for 1 and 2
    for nm, sl in (("top rows", np.s_[:h]), ("bottom rows", np.s_[-h:]), ("left columns", np.s_[:, :h]), ("right columns", np.s_[:, -h:])):
        assert_bitexact(want[sl], got[sl], f"{what}: ring {nm} keep the input flow x {scale}")


def tile_kernel_chain(hip, case, k, iters):
    """mfsr_lucasKanadeIterationWarped (the tile kernel) on the same input, dense: the final flow, x 2 on the last iteration."""
    W, H = case.W, case.H
    f = [np.zeros((H, W, 2), np.float32) for _ in range(2)]
    S = [np.full((H, W), np.nan, np.float32) for _ in range(2)]
    D = [np.full((H, W), np.nan, np.float32) for _ in range(2)]
    hip.call("CreateFlowFieldWarped", f[0], Tex(case.tiles[k]), W, H, W * 8, F2([0, 0]), 0.0, None, case.ref, case.movs[k], W * 4, S[0], D[0], W * 4)
    for it in range(iters):
        i, o, last = it & 1, (it & 1) ^ 1, it == iters - 1
        hip.call("lucasKanadeIterationWarped", f[i], f[o], W * 8, case.ref, case.movs[k], W * 4, S[i], D[i], None if last else S[o],
                 None if last else D[o], W * 4, W, H, case.hw, MIN_DET, 2.0 if last else 1.0)
    return f[iters & 1]


def assert_like_the_oracle(hip, case, k, got2, want, what):
    """(a) the assertions of test_lucasKanadeSweepBatch_vs_oracle_chain on the final flow (x outScale 2) against the oracle's,
    plus a bound on EVERY pixel (max_rest < 2e-2).  For h = 1 alone, where the two maxima are over the bounds, the tile kernel
    on the same input is the yardstick: the sweep is at most twice as far from the oracle.  -> the figures."""
    assert np.isfinite(got2).all(), what
    got = got2 / 2.0
    rep = flow_difference_report(got, want, case.ref, case.hw, thr=5e-4)
    d = np.abs(got - want)
    err = distance_to_true(case, k, got)
    print(f"{what} frame {k}/{case.nf}: |flow(k_lkSweep) - flow(oracle chain)| well-conditioned windows ({rep['well_fraction']:.0%}) max "
          f"{rep['max_well']:.2e} px, rest max {rep['max_rest']:.2e} px, median {np.median(d):.1e}, > 5e-4: {rep['n_big']}; "
          f"mean distance to the true shift {err:.3f} px")
    assert rep["well_fraction"] >= 0.3
    if case.hw == 1 and (rep["max_well"] > 5e-4 or rep["max_rest"] >= 2e-2):
        tile = tile_kernel_chain(hip, case, k, 3) / 2.0
        rt = flow_difference_report(tile, want, case.ref, case.hw, thr=5e-4)
        print(f"   h = 1: the tile kernel against the oracle on the same input: well-conditioned max {rt['max_well']:.2e} px, rest max {rt['max_rest']:.2e} px")
        assert rep["max_well"] <= max(5e-4, 2 * rt["max_well"]) and rep["max_rest"] < max(2e-2, 2 * rt["max_rest"])
    else:
        assert rep["max_well"] <= 5e-4
        assert rep["max_rest"] < 2e-2
    assert np.median(d) <= 2e-5
    assert err < 0.25
    np.testing.assert_allclose(got2[:case.hw], 2.0 * want[:case.hw], rtol=0, atol=1e-6)
    return rep, float(np.median(d))


THREE = [(1.0, True), (1.0, True), (2.0, False)]      # three iterations, outScale 2 on the last


# ---------------------------------------------------------------- a + b: every half window
@pytest.mark.parametrize("hw", range(1, 8))
def test_every_half_window_against_the_oracle(orc, hip, hw):
    """Each of the seven template instances (its own register ring and lane bounds) against three chained oracle iterations:
    three strips with the last owning one column, bands of 8 rows with the last owning one row, 1 .. 4 frames per launch.  After
    the first iteration the planes handed to the next are the oracle's warp under the kernel's own flow, bit for bit.

    Measured on an MI355X, worst frame per h -- well-conditioned windows max / rest max / median, px:
        h = 1: 1.1e-4 / 7.5e-4 / 1.3e-6      h = 2: 1.4e-5 / 4.6e-5 / 4.2e-7      h = 3: 3.8e-6 / 4.2e-5 / 2.4e-7
        h = 4: 3.1e-6 / 1.8e-5 / 2.4e-7      h = 5: 2.7e-6 / 5.1e-6 / 1.2e-7      h = 6: 2.3e-6 / 2.5e-6 / 1.2e-7
        h = 7: 1.3e-6 / 3.6e-6 / 0
    h = 1 (3 x 3 windows, never measured against the oracle before) is inside the bounds of the larger windows: the tile-kernel
    yardstick of assert_like_the_oracle was not needed.  The planes are bit-exact at every pixel."""
    case = half_window_case(hw)
    assert hip.L.lucasKanadeSweepBand(case.W, case.H, hw, case.nf) == 8, "MFSR_LK_BAND is set, or the band rule moved"
    res = run_sweep(hip, case, THREE)
    for k in range(case.nf):
        what = f"h={hw} {case.W}x{case.H}"
        assert_planes(orc, case, k, res.flow[0][k], res.S[0][k], res.D[0][k], what)
        assert_ring(case, res.flow[0][k], res.flow0[k], 1.0, what)
        assert_like_the_oracle(hip, case, k, res.flow[2][k], oracle_chain(orc, case, k, 3)[-1], what)


# ---------------------------------------------------------------- c: minimum geometry
def one_iteration_against_the_oracle(orc, hip, case, what):
    """One iteration with planes out (outScale 1) and one as a last iteration (outScale 2, no planes: the idle planes keep the
    sentinel), each against the oracle at c_lkFused's tolerance; ring rows and columns bit for bit; the planes as in (b)."""
    first = run_sweep(hip, case, [(1.0, True)])
    last = run_sweep(hip, case, [(2.0, False)])
    for k in range(case.nf):
        want = oracle_chain(orc, case, k, 1)[0]
        np.testing.assert_allclose(first.flow[0][k], want, rtol=0, atol=1e-4, err_msg=f"{what} frame {k}")
        np.testing.assert_allclose(last.flow[0][k] / 2.0, want, rtol=0, atol=1e-4, err_msg=f"{what} frame {k}, outScale 2")
        assert_bitexact(first.flow[0][k] * np.float32(2.0), last.flow[0][k], f"{what} frame {k}: outScale 2 is the same flow doubled")
        assert_ring(case, first.flow[0][k], first.flow0[k], 1.0, f"{what} frame {k}")
        assert_ring(case, last.flow[0][k], last.flow0[k], 2.0, f"{what} frame {k}")
        assert_planes(orc, case, k, first.flow[0][k], first.S[0][k], first.D[0][k], what)


@pytest.mark.parametrize("hw", [1, 3, 7])
def test_minimum_geometry(orc, hip, hw):
    """width == 64 (two strips at h = 7: the second all halo but a few columns) with height == 2 (h + 2) and one row more: the
    band's halo is the whole image, mirrored at both ends; one frame and four."""
    for H in (2 * (hw + 2), 2 * (hw + 2) + 1):
        for nf in (1, 4):
            one_iteration_against_the_oracle(orc, hip, conditioned_case(orc, hw, 64, H, nf, 31 + H), f"minimum geometry h={hw} 64x{H} x{nf}")


# ---------------------------------------------------------------- d: results do not depend on the band
def assert_same_bits(a, b, what, band):
    same = a.view(np.uint32) == b.view(np.uint32)
    if not same.all():
        y, x = np.argwhere(~same)[0][:2]
        raise AssertionError(f"{what}: {np.count_nonzero(~same)} of {a.size} elements differ, first at row {y} (row {y % band} of its "
                             f"{band}-row band), column {x}")


LAST = [(1.0, True), (2.0, False)]       # one iteration with planes out, a last one with outScale 2 and none


# (W, H, h, band of the four-frame launch, band of a frame alone, frames also launched alone, a permuted launch as well)
BANDS = [(118, 4611, 3, 10, 8, (0, 1, 2, 3), True),      # the last band of the four-frame launch is 1 row
         (100, 2738, 7, 9, 8, (0, 1, 2, 3), True),       # ... 2 rows, shorter than the halo; 3660 and 1029 tiles: surplus workgroups in the XCD remap
         (64, 8200, 1, 9, 8, (0, 1, 2, 3), True),
         (64, 32769, 7, 32, 17, (0, 3), False)]          # the rule's fall-through branch (b = 65 > 64); bit identity only, first and last slot


@pytest.mark.parametrize("W,H,hw,band4,band1,alone,permute", BANDS)
def test_results_do_not_depend_on_the_band(orc, hip, W, H, hw, band4, band1, alone, permute):
    """A pixel's window is summed from the same rows in the same order whatever band it falls in, so the flow and both planes
    of a frame are bit-identical whether it is launched alone or as one of four, in whichever slot (the four frames differ, one
    launch permutes them: a frame index taken from the wrong term of the remapped tile number shows).  At 118 x 4611 frame 0
    of the four-frame launch also meets the oracle chain: the first oracle comparison at a band other than 8 (measured: 1.7e-4 px
    over the well-conditioned windows, 1.2e-3 over the rest, median 1.5e-6).  At 64 x 32769 (2.1 M pixels a frame, the largest
    case of the module) the frames of the first and the last slot are launched alone and no permuted launch is made: seconds."""
    L = hip.L
    msg = "MFSR_LK_BAND is set, or the band rule moved"
    assert L.lucasKanadeSweepBand(W, H, hw, 4) == band4 and L.lucasKanadeSweepBand(W, H, hw, 1) == band1 and band4 != band1, msg
    case = LkCase(hw, W, H, 4, 41 + hw)
    four = run_sweep(hip, case, LAST)
    runs = [(f"alone (band {band1})", run_sweep(hip, case, LAST, order=[k]), [k]) for k in alone]
    if permute:
        runs.append(("in permuted slots", run_sweep(hip, case, LAST, order=[2, 0, 3, 1]), range(4)))
    for nm, other, frames in runs:
        for k in frames:
            w = f"h={hw} {W}x{H} frame {k} as one of four (band {band4}) and {nm}"
            assert_same_bits(four.flow0[k], other.flow0[k], w + ": first flow", band4)
            assert_same_bits(four.flow[0][k], other.flow[0][k], w + ": flow of the first iteration", band4)
            assert_same_bits(four.S[0][k], other.S[0][k], w + ": sumOut", band4)
            assert_same_bits(four.D[0][k], other.D[0][k], w + ": diffOut", band4)
            assert_same_bits(four.flow[1][k], other.flow[1][k], w + ": flow of the last iteration", band4)
    if (W, H) == (118, 4611):
        want = oracle_chain(orc, case, 0, 2)
        assert_planes(orc, case, 0, four.flow[0][0], four.S[0][0], four.D[0][0], f"h={hw} {W}x{H} band {band4}")
        assert_like_the_oracle(hip, case, 0, four.flow[1][0], want[-1], f"h={hw} {W}x{H} band {band4}")


# ---------------------------------------------------------------- e: hostile flows stay in their frame
def _hostile_flow(flow):
    """NaN, +-Inf and 1e9 in blocks of the left 13 columns: the first rows, a band seam (rows 7 / 8), the last rows."""
    flow[0:3, 0:4] = np.nan
    flow[6:10, 9:13] = [np.inf, -np.inf]
    flow[20:22, 2:5] = [1e9, -1e9]
    flow[38:41, 0:3] = [np.nan, 1e9]
    flow[30, 12] = [-np.inf, np.nan]
    return flow


def test_hostile_flows_stay_in_their_frame(orc, hip):
    """Frame 2 of four carries tile shifts of up to +-3 image sizes: against the oracle as in (a) and (b) -- the convergence
    figure over the pixels whose first flow was near the true shift, as everywhere.  Then its first flow field gets NaN, +-Inf
    and 1e9 in a few blocks (its planes recomputed for that flow by the oracle's warp): every guard and every byte of padding
    intact (run_sweep), the three other frames bit-identical to the run without, and in frame 2 every pixel farther than
    2 (h + 2) rows or columns per iteration from a hostile pixel as well."""
    case = hostile_case()
    hw, k2 = case.hw, HOSTILE_FRAME
    what = f"hostile tile shifts h={hw} {case.W}x{case.H}"
    clean = run_sweep(hip, case, THREE)
    assert (~calm(case, k2)).mean() > 0.1 and np.abs(clean.flow0[k2]).max() > 2 * case.W
    assert_planes(orc, case, k2, clean.flow[0][k2], clean.S[0][k2], clean.D[0][k2], what)
    assert_like_the_oracle(hip, case, k2, clean.flow[2][k2], oracle_chain(orc, case, k2, 3)[-1], what)
    run = run_sweep(hip, case, THREE, hostile={k2: _hostile_flow}, orc=orc)
    bad = ~np.isfinite(run.flow0[k2]).all(-1) | (np.abs(run.flow0[k2]).max(-1) >= 1e9)
    assert 40 < bad.sum() < 80
    for k in (0, 1, 3):
        for it in range(3):
            assert_same_bits(clean.flow[it][k], run.flow[it][k], f"frame {k} next to a hostile frame, flow of iteration {it}", 8)
            if it < 2:
                assert_same_bits(clean.S[it][k], run.S[it][k], f"frame {k} next to a hostile frame, sumOut of iteration {it}", 8)
                assert_same_bits(clean.D[it][k], run.D[it][k], f"frame {k} next to a hostile frame, diffOut of iteration {it}", 8)
    yy, xx = np.argwhere(bad).T
    for it in range(3):
        R = 2 * (hw + 2) * (it + 1)
        near = np.zeros(bad.shape, bool)
        for y, x in zip(yy, xx):
            near[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1] = True
        far = ~near
        assert far.mean() > 0.4 and far[:, 54].any() and far[:, 108].any()       # a strip seam and the last strip's one column among them
        for nm, a, b in (("flow", clean.flow[it][k2], run.flow[it][k2]),) + ((("sumOut", clean.S[it][k2], run.S[it][k2]),
                                                                               ("diffOut", clean.D[it][k2], run.D[it][k2])) if it < 2 else ()):
            same = (a.view(np.uint32) == b.view(np.uint32)).reshape(bad.shape + (-1,)).all(-1)
            off = np.argwhere(far & ~same)
            assert off.size == 0, (f"hostile frame, {nm} of iteration {it}: {len(off)} pixels farther than {R} from every hostile pixel "
                                   f"differ from the clean run, first at {tuple(off[0])}")


# ---------------------------------------------------------------- f: refusals touch nothing
def test_refusals_touch_nothing(hip):
    """Every MFSR_REQUIRE / MFSR_E_UNSUPPORTED of the entry: the status, and every buffer, guards included, as uploaded."""
    capi = hip.capi
    raw = hip.L.raw["mfsr_lucasKanadeSweepBatch"]
    hw, W, H = 3, 64, 12
    case = LkCase(hw, W, H, 1, 51)
    pSh, pImg, pSD = sweep_pitches(W)

    def attempt(nm, status, n=1, h=hw, w=W, height=H, psh=pSh, pimg=pImg, scale=1.0, edit=None):
        D = DevBufs(hip)
        up = lambda a, pitch: D.up(_pad2d(a, SENTINEL, pitch=pitch)[0], True)      # noqa: E731  (read-only: must come back as uploaded)
        ref, mov = up(case.ref, pImg), up(case.movs[0], pImg)
        fl = [up(_blank((H, W, 2)), pSh) for _ in range(2)]
        S = [up(_blank((H, W)), pSD) for _ in range(2)]
        Dp = [up(_blank((H, W)), pSD) for _ in range(2)]
        fr = dict(shiftsIn=fl[0], shiftsOut=fl[1], movedImg=mov, sumIn=S[0], diffIn=Dp[0], sumOut=S[1], diffOut=Dp[1])
        if edit:
            edit(fr)
        arr = (capi.LkFrame * 5)(*[capi.LkFrame(**fr) for _ in range(5)])
        rc = raw(n, arr, ref, psh, pimg, pSD, w, height, h, MIN_DET, scale, None)
        D.finish(f"refused mfsr_lucasKanadeSweepBatch ({nm})")
        assert rc == status, f"{nm}: status {rc}, expected {status}"

    attempt("nFrames 0", E_INVALID, n=0)
    attempt("nFrames 5", E_INVALID, n=5)
    attempt("halfWindowSize 0", E_UNSUPPORTED, h=0)
    attempt("halfWindowSize 8", E_UNSUPPORTED, h=8)
    attempt("width 63", E_UNSUPPORTED, w=63)
    attempt("height 2 (h + 2) - 1", E_UNSUPPORTED, height=2 * (hw + 2) - 1)
    attempt("shiftsIn == shiftsOut", E_INVALID, edit=lambda f: f.update(shiftsOut=f["shiftsIn"]))
    attempt("sumOut without diffOut", E_INVALID, edit=lambda f: f.update(diffOut=None))
    attempt("sumOut == sumIn", E_INVALID, edit=lambda f: f.update(sumOut=f["sumIn"]))
    attempt("sumOut with outScale 2", E_INVALID, scale=2.0)
    attempt("pitchShift no multiple of 8", E_INVALID, psh=pSh + 4)
    attempt("pitchImg < 4 * width", E_INVALID, pimg=4 * W - 4)
    attempt("misaligned shiftsOut", E_INVALID, edit=lambda f: f.update(shiftsOut=f["shiftsOut"] + 4))
    # (the same arguments unedited are accepted: test_minimum_geometry launches them)
