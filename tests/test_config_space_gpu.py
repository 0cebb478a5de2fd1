"""The burst driver's non-default configurations against the CPU oracle ("Configuration space").

validate() in csrc/pipeline.cpp accepts wide ranges for mfsr_config's fields, and the driver chooses its kernels from them:
the warped Lucas-Kanade path against mfsr_lucasKanadeIterationFused, the sweep kernel against its fallback for half windows
outside 1..7, the frame-batched alignment, the batched per-frame stages, the compile-time tracker against the generic one,
the fused prepare kernel against the chain, which buffer of the flow ping-pong holds the result.  Every case below changes a
few fields of default_config, runs the burst through the oracle pipeline once and through the HIP driver twice
(pairFrames = 1: the frame-batched alignment where it applies; pairFrames = 0: frame by frame), and asserts

  * the project's own contract of HIP against oracle (tests/burst_compare.py::assert_parity, nothing loosened per case);
  * the reference products bit for bit where the suite already states that (tracking image at 256 x 192 with the default
    prefilter; kernel parameters always), the tracking image to 1e-6 elsewhere, as test_burst_matches_oracle_ragged_sizes;
  * that the alignment locks: median flow of every moved frame's central half within 0.15 px of the true shift (the
    tolerance of test_burst_matches_oracle) -- otherwise both sides could agree while failing to align;
  * the branch the case exists for, from the driver's own counters (mfsr_burst_debug_paths): a threshold changed later makes
    the case fail instead of silently testing another branch.

test_every_path_counter_is_taken_and_not_taken holds the table against the counters: a branch added to the driver fails it
until a case reaches it.

Not asserted: the final tile shifts of the chain / plain fused tracker (bit-equal by DESIGN.md sections 2.1 and 2.5): the
debug views expose flow, mask, kernel parameters and tracking image only, not the tile grids.

Half windows 0 and 1 are deliberately not swept at pipeline level: test_parity_kernels.py::
test_lucasKanadeIterationFused_equals_chain documents that their normal matrices are near-singular in the reference itself, so
a flip-set contract would measure the oracle's conditioning, not the driver; `lk_hw8` already takes the branch they would take
(half window 0) and `lk_hw2` sits next to the sweep range's lower edge.
"""
import numpy as np
import pytest

from tests.burst_compare import assert_parity, classify, flow_difference_report, run_hip, run_oracle

pytestmark = pytest.mark.gpu

LEVELS3 = dict(levels=3, levelFactor=(4, 2, 1), tileSize=(16, 16, 32), maxShift=(3, 3, 4))


def _case(fields=None, W=256, H=192, N=5, max_shift=3.0, mono=False, scale=2, both=None, batched=None, framewise=None):
    """fields: what the case changes of default_config.  both / batched / framewise: the path counters the case exists for, as
    {name: exact count}: in both HIP runs / with pairFrames = 1 / with pairFrames = 0."""
    return dict(fields=fields or {}, W=W, H=H, N=N, max_shift=max_shift, mono=mono, scale=scale, both=both or {},
                batched=batched or {}, framewise=framewise or {})


def _small(W, H, fields=None, mono=False, **kw):
    return _case(fields, W=W, H=H, N=3, max_shift=2.0, mono=mono, **kw)


# The base burst has 5 frames, reference 1: with pairFrames = 1 one full group of four (three moved frames and the reference)
# and one frame aligned alone on flush -- 2 batches, 4 moved frames.  The default path, which the cases that change no branch
# (a kernel's parameter only) must stay on:
DEFAULT_BATCHED = dict(frames_deferred=5, frames_immediate=0, align_batches=2, stage_batches=2, prepare_fused=1, prepare_batch=2,
                       prepare_chain=0, track_fused_batch=4, track_fused_up=0, track_fused_base=0, flow_warped_batch=2,
                       flow_warped=0, lk_sweep_batch=6, lk_sweep_single=0, robust_batch=2, robust_fused=0, scale_flow=0)
DEFAULT_FRAMEWISE = dict(frames_deferred=0, frames_immediate=5, align_batches=0, stage_batches=0, prepare_fused=5, prepare_batch=0,
                         track_fused_up=4, track_fused_base=4, track_fused_batch=0, track_fast_pair=8, track_generic_pair=0,
                         flow_warped=4, flow_warped_batch=0, flow_plain=0, lk_sweep_single=12, lk_sweep_batch=0,
                         lk_iteration_warped=0, lk_iteration_fused=0, lk_chain=0, robust_fused=4, robust_batch=0, robust_chain=0,
                         scale_flow=0)
# the sweep refuses the half window: frame by frame in both runs, mfsr_lucasKanadeIterationWarped for every iteration
NO_SWEEP = dict(frames_deferred=0, frames_immediate=5, lk_sweep_batch=0, lk_sweep_single=0, lk_iteration_warped=12,
                lk_iteration_fused=0, flow_warped=4, scale_flow=0)
# deferred, but (T, S) is not one of the compile-time tracker's pairs: the generic tracker frame by frame, batched LK only
GENERIC_BATCHED = dict(frames_deferred=5, align_batches=2, stage_batches=0, prepare_batch=0, prepare_fused=5, track_fused_batch=0,
                       track_fused_base=4, track_fused_up=4, track_fast_pair=0, track_generic_pair=8, flow_warped=4,
                       flow_warped_batch=0, lk_sweep_batch=6, robust_fused=4, robust_batch=0)
GENERIC_FRAMEWISE = dict(frames_deferred=0, track_fused_base=4, track_fused_up=4, track_fast_pair=0, track_generic_pair=8,
                         lk_sweep_single=12)
# below the tw >= 64 / th >= 32 threshold (3 frames, 2 moved): mfsr_lucasKanadeIterationFused from a plain flow field
BELOW = dict(frames_deferred=0, frames_immediate=3, flow_warped=0, flow_warped_batch=0, flow_plain=2, lk_iteration_fused=6,
             lk_sweep_single=0, lk_sweep_batch=0, lk_iteration_warped=0, scale_flow=0, prepare_fused=3, robust_fused=2)


def _lk_it(it):
    return _case(dict(lkIterations=it), batched=dict(frames_deferred=5, lk_sweep_batch=2 * it, robust_batch=2, scale_flow=0),
                 framewise=dict(frames_deferred=0, lk_sweep_single=4 * it, robust_fused=4, scale_flow=0))


CASES = {
    # ---- Lucas-Kanade -------------------------------------------------------------------------------------------------------
    "lk_it0": _case(dict(lkIterations=0), both=dict(frames_deferred=0, frames_immediate=5, flow_plain=4, flow_warped=0,
                                                    flow_warped_batch=0, scale_flow=4, lk_sweep_batch=0, lk_sweep_single=0,
                                                    lk_iteration_warped=0, lk_iteration_fused=0, lk_chain=0, robust_fused=4)),
    "lk_it1": _lk_it(1),
    "lk_it2": _lk_it(2),
    "lk_it4": _lk_it(4),
    "lk_hw2": _case(dict(lkHalfWindow=2), batched=DEFAULT_BATCHED, framewise=DEFAULT_FRAMEWISE),
    "lk_hw7": _case(dict(lkHalfWindow=7), batched=DEFAULT_BATCHED, framewise=DEFAULT_FRAMEWISE),
    "lk_hw8": _case(dict(lkHalfWindow=8), both=NO_SWEEP),
    "lk_hw15": _case(dict(lkHalfWindow=15), both=NO_SWEEP),
    # ---- tile tracker -------------------------------------------------------------------------------------------------------
    "levels1_T16S4": _case(dict(levels=1, levelFactor=(1,), tileSize=(16,), maxShift=(4,)),
                           batched=dict(stage_batches=2, track_fused_batch=2, track_fused_up=0, track_fused_base=0, track_fast_pair=2),
                           framewise=dict(track_fused_up=0, track_fused_base=4, track_fast_pair=4, track_generic_pair=0)),
    "levels3": _case(LEVELS3, batched=dict(stage_batches=2, track_fused_batch=6, track_fast_pair=6, track_generic_pair=0),
                     framewise=dict(track_fused_up=8, track_fused_base=4, track_fast_pair=12, track_generic_pair=0)),
    "lf4_skip": _case(dict(levelFactor=(4, 1)), batched=dict(stage_batches=2, track_fused_batch=4),
                      framewise=dict(track_fused_up=4, track_fused_base=4, track_fast_pair=8)),
    "T24S5": _case(dict(tileSize=(24, 24), maxShift=(5, 5)), batched=GENERIC_BATCHED, framewise=GENERIC_FRAMEWISE),
    "T32S8": _case(dict(maxShift=(8, 8)), batched=dict(stage_batches=2, track_fused_batch=4, track_fast_pair=4, track_generic_pair=0),
                   framewise=dict(track_fast_pair=8, track_generic_pair=0)),
    "T8S3": _case(dict(tileSize=(8, 8), maxShift=(3, 3)), batched=GENERIC_BATCHED, framewise=GENERIC_FRAMEWISE),
    "T64S15": _case(dict(tileSize=(64, 64), maxShift=(15, 15)), max_shift=6.0, batched=GENERIC_BATCHED, framewise=GENERIC_FRAMEWISE),
    # ---- prepare ------------------------------------------------------------------------------------------------------------
    "sigma_trk_2": _case(dict(sigmaTracking=2.0), batched=DEFAULT_BATCHED, framewise=DEFAULT_FRAMEWISE),
    "sigma_trk_6": _case(dict(sigmaTracking=6.0), both=dict(prepare_chain=5, prepare_fused=0, prepare_batch=0, stage_batches=0),
                         batched=dict(frames_deferred=5, align_batches=2, lk_sweep_batch=6, track_fused_batch=0, track_fused_base=4,
                                      robust_fused=4, robust_batch=0),
                         framewise=dict(frames_deferred=0, lk_sweep_single=12)),
    # ---- parameters of kernels on the default path ----------------------------------------------------------------------------
    "sigma_tensor_2": _case(dict(sigmaTensor=2.0), batched=DEFAULT_BATCHED, framewise=DEFAULT_FRAMEWISE),
    "min_thr": _case(dict(minimumThreshold=0.05), batched=DEFAULT_BATCHED, framewise=DEFAULT_FRAMEWISE),
    "gamma": _case(dict(applyGamma=1), batched=DEFAULT_BATCHED, framewise=DEFAULT_FRAMEWISE),
    "levels_rgb": _case(dict(black=(200.0, 256.0, 300.0), white=(3000.0, 3839.0, 3500.0)), batched=DEFAULT_BATCHED,
                        framewise=DEFAULT_FRAMEWISE),
    # ---- the other drivers of the same stages -----------------------------------------------------------------------------------
    "unfused_levels3_hw8": _case(dict(fused=0, lkHalfWindow=8, **LEVELS3),
                                 both=dict(frames_deferred=0, frames_immediate=5, prepare_chain=5, prepare_fused=0, track_chain=12,
                                           track_fused_up=0, track_fused_base=0, track_fused_batch=0, flow_plain=4, flow_warped=0,
                                           lk_chain=12, lk_sweep_single=0, lk_iteration_warped=0, lk_iteration_fused=0, scale_flow=4,
                                           robust_chain=4, robust_fused=0, robust_batch=0)),
    # mono: groups of two -- (0, 1), (2, 3), (4); tw == W, so the flow needs no scaling and the stages never batch
    "mono_it2_T16": _case(dict(lkIterations=2, tileSize=(16, 16), maxShift=(3, 3)), mono=True,
                          both=dict(prepare_chain=5, prepare_fused=0, prepare_batch=0, stage_batches=0, scale_flow=0, track_fast_pair=8,
                                    track_fused_batch=0, track_fused_base=4, track_fused_up=4, robust_fused=4, flow_warped=4),
                          batched=dict(frames_deferred=5, align_batches=3, lk_sweep_batch=6, lk_sweep_single=0),
                          framewise=dict(frames_deferred=0, lk_sweep_single=8, lk_sweep_batch=0)),
    "x4_it1": _case(dict(lkIterations=1), scale=4, batched=dict(frames_deferred=5, stage_batches=2, lk_sweep_batch=2, robust_batch=2),
                    framewise=dict(frames_deferred=0, lk_sweep_single=4, robust_fused=4)),
    # ---- small frames: 3 frames, reference 1, the default configuration unless noted -------------------------------------------
    # tw = 64, th = 32: the smallest frame still on the warped / sweep path (one batch of three frames on flush)
    "min_warped": _small(128, 64, batched=dict(frames_deferred=3, align_batches=1, stage_batches=1, flow_warped_batch=1,
                                               lk_sweep_batch=3, lk_iteration_fused=0, flow_plain=0),
                         framewise=dict(frames_deferred=0, flow_warped=2, lk_sweep_single=6, lk_iteration_fused=0, flow_plain=0)),
    "below_w": _small(124, 64, both=BELOW),     # tw = 62
    # global pre-alignment off the warped path: the one way to mfsr_CreateFlowFieldFromTilesBase (default trackers; without
    # Lucas-Kanade iterations the oracle's own flow is off by up to a pixel, so lkIterations = 0 cannot serve here)
    "prealign_below_w": _small(124, 64, dict(preAlign=1), both=dict(BELOW, flow_base=2, flow_plain=0)),
    # global pre-alignment ON the warped path: the frames are deferred, but pre-alignment keeps the stages from batching -- the one
    # way to the frame-by-frame stages INSIDE a deferred batch, where every frame of the group works in its own intermediates
    # (moved half image, pyramids, search pyramid, estimate) and only the Lucas-Kanade launches are shared
    "prealign_warped": _case(dict(preAlign=1),
                             batched=dict(frames_deferred=5, align_batches=2, stage_batches=0, prepare_batch=0, flow_warped=4,
                                          flow_warped_batch=0, lk_sweep_batch=6, robust_fused=4, robust_batch=0, track_fused_up=4,
                                          track_fused_base=4),
                             framewise=DEFAULT_FRAMEWISE),
    # the smallest legal frame: tracking image 32 x 32, the coarse level's 32-pixel tile on a 16 x 16 image
    "smallest": _small(64, 64, both=dict(BELOW, track_fused_up=2, track_fused_base=2, track_fast_pair=4)),
    "smallest_T16": _small(64, 64, dict(levels=1, levelFactor=(1,), tileSize=(16,), maxShift=(3,)),
                           both=dict(BELOW, track_fused_up=0, track_fused_base=2, track_fast_pair=2)),
    # tw = 64 because the frame is mono: warped path, groups of two -- (0, 1), (2)
    "smallest_mono": _small(64, 64, mono=True, both=dict(prepare_chain=3, flow_plain=0, lk_iteration_fused=0, stage_batches=0),
                            batched=dict(frames_deferred=3, align_batches=2, lk_sweep_batch=6, flow_warped=2),
                            framewise=dict(frames_deferred=0, lk_sweep_single=6, flow_warped=2)),
}

# the same sweep through the other drivers (host bursts, zoom windows, frame streams): HIP against HIP, bit for bit
DRIVER_CASES = ["lk_it2", "lk_hw8", "levels3", "T24S5", "sigma_trk_6", "prealign_warped"]
REFERENCE = 1
SEED = 20240611


def _set(cfg, fields):
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(cfg, k)[i] = x
        else:
            setattr(cfg, k, v)


def _config(name, pair=1, frames=None, reference=REFERENCE):
    from multi_frame_super_resolution_amd.pipeline import default_config
    c = CASES[name]
    cfg = default_config(c["W"], c["H"], c["N"] if frames is None else frames, c["scale"], c["mono"])
    _set(cfg, c["fields"])
    cfg.reference = reference
    cfg.pairFrames = pair
    return cfg


_BURSTS = {}


def _burst_of(name):
    """(frames, shifts) of the case's burst: made once, shared by every test of the case, never written to."""
    from multi_frame_super_resolution_amd.synth import make_burst
    c = CASES[name]
    key = (c["W"], c["H"], c["N"], c["scale"], c["mono"], c["max_shift"])
    if key not in _BURSTS:
        frames, shifts, _ = make_burst(c["W"], c["H"], c["N"], scale=c["scale"], mono=c["mono"], seed=SEED, max_shift=c["max_shift"])
        _BURSTS[key] = (frames, shifts.numpy())
    return _BURSTS[key]


_PATHS = {}   # (case, pairFrames) -> the driver's counters, kept for test_every_path_counter_is_taken_and_not_taken


def _expected(name, pair):
    c = CASES[name]
    return dict(c["both"], **(c["batched"] if pair else c["framewise"]))


def _assert_paths(name, pair, paths):
    want = _expected(name, pair)
    got = {k: paths[k] for k in want}
    assert got == want, f"{name} pairFrames={pair}: the driver took other branches than the case is for: " \
                        f"{ {k: (got[k], want[k]) for k in want if got[k] != want[k]} } (got, expected); all counters {paths}"


def _assert_locks(name, flows, shifts, what):
    """median flow over the central half of every moved frame ~ -(its shift against the reference's), raw pixels"""
    for k, f in enumerate(flows):
        if k == REFERENCE:
            continue
        c = f[f.shape[0] // 4: -(f.shape[0] // 4), f.shape[1] // 4: -(f.shape[1] // 4)]
        med = np.median(c.reshape(-1, 2), 0)
        true = -(shifts[k] - shifts[REFERENCE])
        print(f"[{name} {what}] frame {k}: median flow {med}, true {true}")
        np.testing.assert_allclose(med, true, atol=0.15, err_msg=f"{name} {what} frame {k}")


@pytest.mark.parametrize("name", list(CASES))
def test_config_matches_oracle(name):
    c = CASES[name]
    frames, shifts = _burst_of(name)
    cfg = _config(name)
    o = run_oracle(cfg, frames)
    _assert_locks(name, o["flows"], shifts, "oracle")     # (a case whose ORACLE does not align says nothing about the driver)
    default_prepare = (c["W"], c["H"]) == (256, 192) and "sigmaTracking" not in c["fields"]
    for pair in (1, 0):
        cfg = _config(name, pair)
        h = run_hip(cfg, frames)
        what = f"{name} pairFrames={pair}"
        _PATHS[(name, pair)] = h["paths"]
        _assert_paths(name, pair, h["paths"])
        if default_prepare:
            assert np.array_equal(h["tracking"], o["tracking"]), what
        else:
            np.testing.assert_allclose(h["tracking"], o["tracking"], atol=1e-6, err_msg=what)
        assert np.array_equal(h["kparam"], o["kparam"], equal_nan=True), what
        rep = classify(cfg, h, o)
        well = max(flow_difference_report(h["flows"][k], o["flows"][k], o["tracking"], cfg.lkHalfWindow)["max_well"]
                   for k in range(c["N"]) if k != REFERENCE)
        # (the record of DESIGN.md section 3's table; not a threshold)
        print(f"CONFIGSPACE | {name} | {pair} | {rep['flip_fraction']:.2e} | {rep['psnr_db_vs_oracle']:.1f} | {well:.1e}")
        _assert_locks(name, h["flows"], shifts, f"pairFrames={pair}")
        assert_parity(rep, what)


def test_below_the_height_threshold_is_not_a_legal_frame():
    """lk_warped_path also asks for th >= 32.  No accepted configuration goes below it: validate() wants height >= 64, so a Bayer
    frame's tracking image has at least 32 rows and a mono frame's 64 -- a 128 x 60 frame (th = 30) is refused at create, with
    either sensor type, and the height half of the threshold has no case in the table above (`below_w`, `smallest` and
    `smallest_T16` are below it by width)."""
    import ctypes
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import default_config
    for mono in (False, True):
        assert capi.lib().raw["mfsr_burst_workspace_bytes"](ctypes.byref(default_config(128, 60, 3, 2, mono))) == 0
        assert capi.lib().raw["mfsr_burst_workspace_bytes"](ctypes.byref(default_config(128, 64, 3, 2, mono))) > 0


def _paths_of(name, pair):
    if (name, pair) not in _PATHS:       # (the case's own test did not run in this session: the HIP burst alone)
        _PATHS[(name, pair)] = run_hip(_config(name, pair), _burst_of(name)[0])["paths"]
    return _PATHS[(name, pair)]


def test_every_path_counter_is_taken_and_not_taken():
    """Over the whole table (both HIP runs of every case) every counter of mfsr_burst_debug_paths is non-zero at least once
    and zero at least once: no branch the driver counts is left without a case, none is taken by every case."""
    from multi_frame_super_resolution_amd import capi
    names = capi.path_names()
    taken, not_taken = set(), set()
    for name in CASES:
        for pair in (1, 0):
            p = _paths_of(name, pair)
            assert sorted(p) == sorted(names)
            taken |= {k for k in names if p[k] > 0}
            not_taken |= {k for k in names if p[k] == 0}
    assert not set(names) - taken, f"no case takes: {sorted(set(names) - taken)}"
    assert not set(names) - not_taken, f"every case takes: {sorted(set(names) - not_taken)}"
    for name in CASES:       # every counter a case names exists
        for pair in (1, 0):
            assert set(_expected(name, pair)) <= set(names), name


def test_path_counters_restart_with_the_burst():
    """mfsr_burst_begin zeroes the counters: a second burst on the same context reports its own launches, not the sum."""
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to("cuda:0") for f in _burst_of("lk_it2")[0]]
    pipe = BurstPipeline(_config("lk_it2", 0), torch.device("cuda:0"))
    pipe.process(frames)
    first = pipe.debug_paths()
    pipe.process(frames)
    assert pipe.debug_paths() == first and first["lk_sweep_single"] == 8
    pipe.begin_burst()
    assert set(pipe.debug_paths().values()) == {0}
    pipe.close()


def _prealign_floats(pipe):
    """(shiftX, shiftY, rotation) of mfsr_burst_prealign_result, as their bits"""
    import ctypes
    import struct
    from multi_frame_super_resolution_amd import capi
    pa = capi.PreAlign()
    pipe.L.burst_prealign_result(pipe._h, ctypes.byref(pa), None)
    return struct.pack("<3f", pa.shiftX, pa.shiftY, pa.rotation)


def test_prealign_result_names_the_last_aligned_frame():
    """mfsr_burst_prealign_result is the estimate of the frame aligned last.  `prealign_warped` cut to 4 frames with reference 0
    is one group of four with pairFrames = 1: the last frame is aligned at batch position 3, in the last of the group's
    per-frame intermediates.  The call after process() returns, bit for bit, the three floats of the frame-by-frame burst
    (pairFrames = 0), where every frame is aligned in the same buffers.  (Batch position 0 is the reference frame here, which
    has no estimate: the group's first entry is never written in this burst, so it cannot stand in for the last one.)"""
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to("cuda:0") for f in _burst_of("prealign_warped")[0][:4]]
    got = {}
    for pair in (1, 0):
        pipe = BurstPipeline(_config("prealign_warped", pair, frames=4, reference=0), torch.device("cuda:0"))
        pipe.process(frames)
        got[pair] = _prealign_floats(pipe)
        if pair:
            assert pipe.debug_paths()["align_batches"] == 1 and pipe.debug_paths()["frames_deferred"] == 4
        pipe.close()
    print(f"prealign_result: pairFrames=1 {np.frombuffer(got[1], np.float32)}, pairFrames=0 {np.frombuffer(got[0], np.float32)}")
    assert got[1] == got[0]


def test_context_survives_joint_mode():
    """After mfsr_burst_process_joint the reference's alignment products name the caller's joint workspace: add_frame without a
    new reference is refused (invalid argument), and an ordinary process() on the same context -- which sets its reference
    again -- gives the u16 image, the accumulators and the weights of a fresh context, bit for bit."""
    import torch
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    dev = torch.device("cuda:0")
    frames = [f.to(dev) for f in _burst_of("lk_it2")[0]]     # (the 256 x 192 x 5 burst every case of that size shares)
    cfg = default_config(256, 192, 5, 2, False)
    cfg.reference = REFERENCE
    fresh = BurstPipeline(cfg, dev)
    _, o16 = fresh.process(frames)
    want = (o16.clone().cpu(), fresh.img_out.clone().cpu(), fresh.total_weights.clone().cpu())
    fresh.close()
    pipe = BurstPipeline(cfg, dev)
    pipe.process_joint(frames)
    with pytest.raises(capi.MfsrError) as e:
        pipe.add_frame(frames[0], False)
    assert e.value.code == -1     # MFSR_E_INVALID
    _, o16 = pipe.process(frames)
    got = (o16.cpu(), pipe.img_out.cpu(), pipe.total_weights.cpu())
    pipe.close()
    for i, what in enumerate(("u16 image", "accumulators", "weights")):
        assert torch.equal(_bits(want[i]), _bits(got[i])), f"after process_joint: {what} differs from a fresh context's"


# ---------------------------------------------------------------------------------------------------------------------------
# the same configurations through the host-burst, zoom-window and frame-stream drivers
# ---------------------------------------------------------------------------------------------------------------------------
_RESIDENT = {}


def _resident(name, pair=1):
    """(float image, u16 image, accumulators, weights) of the resident whole-frame burst, on the host; once per case."""
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    if (name, pair) not in _RESIDENT:
        pipe = BurstPipeline(_config(name, pair), torch.device("cuda:0"))
        out, out16 = pipe.process([f.to("cuda:0") for f in _burst_of(name)[0]])
        _RESIDENT[(name, pair)] = (out.clone().cpu(), out16.clone().cpu(), pipe.img_out.clone().cpu(), pipe.total_weights.clone().cpu())
        pipe.close()
    return _RESIDENT[(name, pair)]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_host_burst_equals_resident_burst(name):
    """The statement of test_host_frame_burst_equals_device_frame_burst (uploadRing = 4) at configurations that flip
    can_defer_alignment, the batched stages and the prepare path.  Three bursts on one context: the first alone (its frames are
    aligned as they come off the link), the second and, into another host buffer, the third enqueued back to back (the third
    while the second is still in flight: the driver then batches every group)."""
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    want = _resident(name)[1]
    cfg = _config(name)
    cfg.uploadRing = 4
    pipe = BurstPipeline(cfg, torch.device("cuda:0"))
    pinned = [f.pin_memory() for f in _burst_of(name)[0]]
    first = pipe.process_host(pinned)
    pipe.host_sync()
    assert torch.equal(first, want), (name, "first burst")
    first.zero_()
    other = torch.zeros_like(first).pin_memory()
    second = pipe.process_host(pinned)
    third = pipe.process_host(pinned, other)
    pipe.host_sync()
    assert torch.equal(second, want), (name, "second burst")
    assert torch.equal(third, want), (name, "third burst, enqueued behind the second")
    pipe.close()


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_window_equals_whole_frame_crop(name):
    """The statement of tests/test_window_gpu.py: the window (64, 48, 96, 64) is bit for bit the rectangle of the whole frame."""
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    x, y, w, h = win = (64, 48, 96, 64)
    whole = _resident(name)
    pipe = BurstPipeline(_config(name), torch.device("cuda:0"), window=win)
    out, out16 = pipe.process([f.to("cuda:0") for f in _burst_of(name)[0]])
    got = (out.cpu(), out16.cpu(), pipe.img_out.cpu(), pipe.total_weights.cpu())
    pipe.close()
    for i, what in enumerate(("float image", "u16 image", "accumulators", "weights")):
        crop = whole[i][y:y + h, x:x + w]
        assert crop.shape == got[i].shape and torch.equal(_bits(crop), _bits(got[i])), f"{name}: {what} differs from the whole-frame crop"


@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("name", DRIVER_CASES)
def test_frame_stream_equals_burst_per_window(name, pair):
    """The bit-identity test_frame_stream_matches_oracle_per_window states: every output t of FrameStream(radius = 1) is the HIP
    burst of its own window (frames [t-1, t+1] clipped, reference t) under the same configuration -- although the stream
    prepares each frame once and always aligns frame by frame.  pairFrames = 0: both sides fuse frame by frame; 1: the burst
    aligns its window as one batch where the configuration allows it."""
    import torch
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, FrameStream
    dev = torch.device("cuda:0")
    frames = [f.to(dev) for f in _burst_of(name)[0]]
    N, R = len(frames), 1
    st = FrameStream(_config(name, pair, frames=2 * R + 1, reference=0), R, dev)
    outs = {}
    for f in frames:
        r = st.push(f)
        if r is not None:
            outs[r[0]] = r[1].clone()
    for t, o in st.drain():
        outs[t] = o.clone()
    torch.cuda.synchronize()
    st.close()
    assert sorted(outs) == list(range(N))
    for t in range(N):
        lo, hi = max(0, t - R), min(N - 1, t + R)
        ref = BurstPipeline(_config(name, pair, frames=hi - lo + 1, reference=t - lo), dev)
        _, o16 = ref.process(frames[lo:hi + 1])
        assert torch.equal(o16, outs[t]), f"{name} pairFrames={pair} t={t}"
        ref.close()
    assert not torch.equal(outs[1], outs[2])
