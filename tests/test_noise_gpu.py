"""Noise-model calibration on the GPU: mfsr_noiseStats against the numpy restatement for equality,
recovery of the model on the synthetic chart, the effect on a high-gain burst, the documented limit on texture, bit-safety and
the CLI switch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.test_noise_cpu import (BLACK, CHART_MODELS, SAT, WHITE, calibrate_rule, chart, default_rect, fit_rule, full_rect,
                                  recovery_bound, stats_rule)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "apps", "multi_frame_sr")
I4 = ctypes.c_int32 * 4


def _to_dev(host, pad=0, offset=0):
    """u16 arrays [h, w] -> device [h, w] views; pad / offset make pitched, shifted rows.  Returns (views, backing tensors)."""
    views, backs = [], []
    for a in host:
        h, w = a.shape
        big = torch.full((h, w + pad + offset), 0x5A5A, dtype=torch.int16, device="cuda:0")
        v = big[:, offset:offset + w]
        v.copy_(torch.from_numpy(a.view(np.int16)).to("cuda:0"))
        views.append(v)
        backs.append(big)
    return views, backs


def _dense(host):
    return [torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to("cuda:0") for a in host]


def _stats_gpu(dev, w, h, rect, black=BLACK, sat=SAT):
    from multi_frame_super_resolution_amd import capi
    n = len(dev)
    hist = torch.full((4, 64, 272), -3, dtype=torch.int32, device="cuda:0")
    ls = torch.full((4, 64), -3, dtype=torch.int64, device="cuda:0")
    cnt = torch.full((4, 64), -3, dtype=torch.int64, device="cuda:0")
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in dev])
    capi.lib().noiseStats(n, ptrs, dev[0].stride(0) * 2, w, h, I4(*black), sat, I4(*rect), hist.data_ptr(), ls.data_ptr(),
                          cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return hist.cpu().numpy().view(np.uint32), ls.cpu().numpy(), cnt.cpu().numpy()


def _check(host, rects=None, black=BLACK, sat=SAT, pad=0, offset=0):
    h, w = host[0].shape
    dev, backs = _to_dev(host, pad, offset)
    before = [b.clone() for b in backs]
    for rect in rects or (full_rect(w, h), default_rect(w, h)):
        want = stats_rule(host, rect, black, sat)
        got = _stats_gpu(dev, w, h, rect, black, sat)
        for name, a, b in zip(("hist", "levelSum", "count"), got, want):
            assert np.array_equal(a, b), (name, rect, int((a != b).sum()))
    for x, y in zip(before, backs):
        assert torch.equal(x, y)                     # frames (and the bytes around them) are read only


def _noise(n, w, h, seed, lo=0, hi=4096):
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, (h, w)).astype(np.uint16) for _ in range(n)]


def _scene(n, w, h, mono, seed=77):
    from multi_frame_super_resolution_amd.synth import make_burst
    frames, _, _ = make_burst(w, h, n, mono=mono, seed=seed)
    return [f.numpy().view(np.uint16) for f in frames]


# ---- equality -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
def test_scene_and_chart_bursts(mono):
    _check(_scene(3, 256, 192, mono))
    _check(chart(1e-4, 1e-6, mono=mono, width=256, height=192, frames=2))


@pytest.mark.parametrize("w,h", [(250, 130), (64, 24), (24, 64), (1026, 70)])
def test_sizes_with_partial_edge_blocks(w, h):
    _check(_scene(2, w, h, False, seed=w), rects=(full_rect(w, h), default_rect(w, h)))


@pytest.mark.parametrize("pad,offset", [(6, 0), (3, 1), (8, 8), (24, 0), (5, 3)])
def test_unaligned_pitch_and_pointer(pad, offset):
    """Pitches and row starts that are not multiples of 16 bytes take the 16-bit-load kernel; (8, 8) and (24, 0) stay aligned."""
    _check(_scene(2, 256, 136, False), pad=pad, offset=offset)
    _check(_noise(1, 250, 130, 5, 200, 3000), pad=pad, offset=offset)


@pytest.mark.parametrize("n", [1, 17, 64])
def test_frame_counts(n):
    _check(_noise(n, 128, 72, n, 256, 4000), rects=(full_rect(128, 72),))


def test_rectangles():
    host = _scene(2, 512, 384, False)
    _check(host, rects=((5, 7, 6, 8), (0, 0, 64, 1), (63, 0, 64, 48), (10, 3, 41, 29), (0, 47, 64, 48)))


def test_full_range_levels_and_saturated_region():
    """Blocks that hold a sample at or above sat are excluded whole; black levels and sat other than the defaults."""
    host = _scene(3, 256, 192, False)
    host[1][40:75, 100:171] = 4095                    # a clipped region, not on block boundaries
    host[2][5, 5] = 4095
    host[0][100:108, 8:16] = 4094                      # just below sat: stays
    _check(host)
    _check(_noise(2, 256, 192, 11, 0, 65536), black=(0, 10, 700, 64), sat=65535)
    _check(_noise(2, 256, 192, 12, 0, 4096), black=(60, 64, 64, 70), sat=3000)
    _check(_noise(2, 256, 192, 13, 0, 4096), black=(0, 0, 0, 0), sat=1)      # nothing usable: all-zero tables
    host = _noise(1, 128, 64, 14, 0, 2)
    host[0][:, ::4] = 65534                            # the largest pair differences: D up to 8 * 65534^2
    _check(host, sat=65535)


def test_all_equal_frames_land_on_one_address():
    """The contention case: every update of a position goes to one counter; the counts must still be exact."""
    for value in (1000, 256, 0, 4094):
        host = [np.full((384, 512), value, dtype=np.uint16) for _ in range(5)]
        _check(host)
    big = [np.full((2160, 3840), 777, dtype=np.uint16) for _ in range(4)]
    _check(big, rects=(full_rect(3840, 2160),))
    hist, ls, cnt = stats_rule(big[:1], full_rect(3840, 2160))
    assert int(cnt.sum()) == 4 * 480 * 270 and int((hist != 0).sum()) == 4


def test_4k_16_frames():
    host = _scene(2, 3840, 2160, False)
    host = [host[k % 2] if k % 3 else np.roll(host[k % 2], 8 * k, axis=1) for k in range(16)]
    _check(host, rects=(default_rect(3840, 2160),))


# ---- recovery -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,beta", CHART_MODELS)
def test_chart_recovery(alpha, beta):
    """8 frames of the 512 x 384 chart.  The bound on |alpha_est / alpha - 1| is three times the error of the numpy restatement
    on this very fixture (measured on the CPU: 0.10 % for (1e-4, 1e-6), 0.40 % for (1.6e-3, 1.6e-5)), at least 2 %: so 2 % for
    both.  beta is ill-conditioned: only 0 <= beta_est <= 0.05 alpha_est + 4 beta.  The device stage equals numpy bit for bit,
    so the GPU's values equal the restatement's to 1e-9."""
    from multi_frame_super_resolution_amd.pipeline import calibrate_noise, default_config, noise_fit, noise_stats
    host = chart(alpha, beta)
    ra, rb, rst, rn = calibrate_rule(host)
    bound = recovery_bound(abs(ra / alpha - 1))
    cfg = default_config(512, 384, 8, 2, False)
    dev = _dense(host)
    a, b, st = calibrate_noise(dev, cfg)
    print(f"chart ({alpha:g}, {beta:g}): numpy {ra:.6g} {rb:.6g} (error {abs(ra / alpha - 1):.4f}), HIP {a:.6g} {b:.6g}, bound {bound:.4f}")
    assert st == rst == 0
    assert abs(a - ra) <= 1e-9 * abs(ra) and abs(b - rb) <= 1e-9 * abs(rb)
    assert abs(a / alpha - 1) <= bound
    assert 0.0 <= b <= a * 0.05 + 4 * beta
    assert noise_fit(noise_stats(dev, cfg), cfg) == (a, b, st, rn)
    want = stats_rule(host, default_rect(512, 384))
    got = noise_stats(dev, cfg)
    assert np.array_equal(got.hist.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(got.count.cpu().numpy(), want[2])


def test_burst_calibrate_noise_c_abi():
    from multi_frame_super_resolution_amd import capi
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    alpha, beta = CHART_MODELS[1]
    host = chart(alpha, beta)
    ra, rb, rst, _ = calibrate_rule(host)
    cfg = default_config(512, 384, 8, 2, False)
    dev = _dense(host)
    p = BurstPipeline(cfg)
    scratch = torch.empty(4 * 4 * 64 * 272 + 16 * 256, dtype=torch.uint8, device="cuda:0")
    a, b, st = ctypes.c_float(), ctypes.c_float(), ctypes.c_int32(-1)
    ptrs = (ctypes.c_void_p * 8)(*[f.data_ptr() for f in dev])
    capi.lib().burst_calibrate_noise(p._h, 8, ptrs, scratch.data_ptr(), ctypes.byref(a), ctypes.byref(b), ctypes.byref(st),
                                     torch.cuda.current_stream().cuda_stream)
    assert st.value == rst == 0 and a.value == np.float32(ra) and b.value == np.float32(rb)
    raw = capi.lib().raw["mfsr_burst_calibrate_noise"]
    assert raw(p._h, 0, ptrs, scratch.data_ptr(), ctypes.byref(a), ctypes.byref(b), ctypes.byref(st), None) == -1
    assert raw(p._h, 8, ptrs, None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(st), None) == -1
    p.close()


# ---- the documented limit -------------------------------------------------------------------------------------------------
def test_textured_scene_is_not_recovered():
    """A single frame cannot tell pixel-scale texture from noise: on the make_burst scene (default noise, alpha 1e-4, beta
    1e-6) the estimate is either refused or far off.  Checked with the numpy restatement on the CPU first (4 frames of 512 x
    384: alpha 6.07e-4, beta 1.31e-3, status 0)."""
    from multi_frame_super_resolution_amd.pipeline import calibrate_noise, default_config
    host = _scene(4, 512, 384, False, seed=1234)
    ra, rb, rst, _ = calibrate_rule(host)
    assert rst != 0 or rb > 100 * 1e-6
    a, b, st = calibrate_noise(_dense(host), default_config(512, 384, 4, 2, False))
    print(f"textured scene: alpha {a:.6g} beta {b:.6g} status {st}")
    assert st == rst and (st != 0 or b > 100 * 1e-6)
    assert abs(a - ra) <= 1e-9 * abs(ra) and abs(b - rb) <= 1e-9 * abs(rb)


# ---- effect ---------------------------------------------------------------------------------------------------------------
def test_calibration_opens_the_masks_of_a_high_gain_burst():
    """A make_burst(512, 384, 6) scene drawn with alpha 1.6e-3, beta 1.6e-5 (a high-gain sensor), processed with the default
    config (alpha 1e-4, beta 1e-6) and with the values calibrate_noise measures on a chart burst of the same noise.  Asserted:
    the mean robustness mask of frames 1..5 rises, and PSNR against the scene (16-pixel margin) is higher with calibration.
    Only the ordering is asserted; the values are printed and recorded in DESIGN.md section 2.15.  Measured on an MI355X (the
    CPU oracle pipeline gives the same figures): PSNR default 31.579 dB, calibrated 31.582 dB; masks default 0.9924 0.9781
    0.9596 0.9765 0.9884, calibrated 0.9996 0.9959 0.9889 0.9957 0.9989 -- the masks open, the PSNR barely moves: the default
    model already merges 96-99 % of this burst."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, calibrate_noise, default_config, view_as_tensor
    from multi_frame_super_resolution_amd.synth import make_burst
    alpha, beta = 1.6e-3, 1.6e-5
    frames, _, gt = make_burst(512, 384, 6, alpha=alpha, beta=beta)
    truth = gt.permute(1, 2, 0).numpy().astype(np.float64)
    dev = [f.to("cuda:0") for f in frames]

    def run(cfg):
        pipe = BurstPipeline(cfg)
        pipe.begin_burst()
        pipe.set_reference(dev[0])
        for k in range(6):
            pipe.add_frame(dev[k], k == 0)
        pipe.flush()
        masks = []
        for k in range(1, 6):
            _, m = pipe.frame_views(5 - k)
            masks.append(float(view_as_tensor(m, 4, pipe.device)[4:-4, 4:-4, :3].mean()))
        out, _ = pipe.finish()
        d = out.cpu().numpy().astype(np.float64)[16:-16, 16:-16] - truth[16:-16, 16:-16]
        pipe.close()
        return float(10 * np.log10(1.0 / np.mean(d * d))), masks

    cfg = default_config(512, 384, 6, 2, False)
    p_default, m_default = run(cfg)
    a, b, st = calibrate_noise(_dense(chart(alpha, beta)), cfg)
    assert st == 0
    cfg.alpha, cfg.beta = a, b
    p_cal, m_cal = run(cfg)
    print(f"calibrated alpha {a:.6g} beta {b:.6g}")
    print(f"PSNR default {p_default:.3f} dB, calibrated {p_cal:.3f} dB")
    print("masks default   ", [round(m, 4) for m in m_default])
    print("masks calibrated", [round(m, 4) for m in m_cal])
    assert float(np.mean(m_cal)) > float(np.mean(m_default))
    assert p_cal > p_default


# ---- bit-safety -----------------------------------------------------------------------------------------------------------
def test_calibration_changes_nothing():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, calibrate_noise, default_config
    host = _scene(4, 256, 192, False)
    cfg = default_config(256, 192, 4, 2, False)
    dev = _dense(host)
    keep = [f.clone() for f in dev]
    p = BurstPipeline(cfg)
    before = p.process(dev)[1].clone()
    calibrate_noise(dev, cfg)
    for x, y in zip(keep, dev):
        assert torch.equal(x, y)
    assert (cfg.alpha, cfg.beta) == (np.float32(1e-4), np.float32(1e-6))
    after = p.process(dev)[1].clone()
    assert torch.equal(before, after)
    p.close()


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def _run_cli(d, **env):
    return subprocess.run([CLI, "farneback", "city", "3"], cwd=d, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, **env))


def test_cli_noise(tmp_path):
    import shutil
    assert os.path.exists(CLI), "build apps/multi_frame_sr first (__graft_entry__.build())"
    d = tmp_path / "city"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "city"), d)

    def result():
        return (d / "city_farneback_sr_result.png").read_bytes()

    plain = _run_cli(d)
    assert plain.returncode == 0 and "noise" not in plain.stderr, plain.stderr
    out_plain = result()
    given = _run_cli(d, MFSR_NOISE="1e-4,1e-6")
    assert given.returncode == 0 and "noise:" not in given.stderr, given.stderr
    assert result() == out_plain                                      # the defaults, spelled out
    other = _run_cli(d, MFSR_NOISE="3e-3,1e-4")
    assert other.returncode == 0 and result() != out_plain
    auto = _run_cli(d, MFSR_NOISE="auto")
    assert auto.returncode == 0, auto.stderr
    lines = [ln for ln in auto.stderr.splitlines() if ln.startswith("noise: alpha ")]
    assert len(lines) == 1, auto.stderr
    words = lines[0].split()
    assert words[3] == "beta" and words[5] == "status" and int(words[6]) in (0, 2, 3)
    assert float(words[2]) >= 0.0 or int(words[6]) == 3
    assert "noise" not in auto.stdout and " sec" in auto.stdout and " FPS" in auto.stdout
    print(lines[0])
    for bad in (dict(MFSR_NOISE="yes"), dict(MFSR_NOISE="1e-4"), dict(MFSR_NOISE="1e-4,"), dict(MFSR_NOISE="-1,0"),
                dict(MFSR_NOISE="auto", MFSR_GPUS="2", MFSR_VIRTUAL_RANKS="1")):
        r = _run_cli(d, **bad)
        assert r.returncode != 0 and "MFSR_NOISE" in r.stderr, (bad, r.stderr)
