"""Frame selection on the GPU: mfsr_frameSharpness equals a numpy int64 restatement of the score exactly, the selection picks the
sharp frame of a burst whose other frames are blurred, process_selected is bit for bit the plain burst with the chosen
reference and frames, and the CLI's MFSR_SELECT reports and uses the sharp frame."""
import os
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "apps", "multi_frame_sr")

CFAS = {"rggb": (0, 1, 1, 2), "bggr": (2, 1, 1, 0), "grbg": (1, 0, 2, 1), "gbrg": (1, 2, 0, 1)}


# ---- the score, restated in numpy int64 (the contract in include/mfsr.h) ------------------------------------------------
def np_score(raw: np.ndarray, cfa, mono: bool, rect) -> int:
    r = raw.astype(np.uint16).astype(np.int64)
    greens = [(0, 1), (1, 0)] if mono else [(i >> 1, i & 1) for i in range(4) if cfa[i] == 1]
    assert len(greens) == 2
    (ay, ax), (by, bx) = greens
    G = r[ay::2, ax::2] + r[by::2, bx::2]
    x0, y0, x1, y1 = rect
    P = G[y0 - 1:y1 + 1, x0 - 1:x1 + 1]
    gx = (P[:-2, 2:] + 2 * P[1:-1, 2:] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[1:-1, :-2] + P[2:, :-2])
    gy = (P[2:, :-2] + 2 * P[2:, 1:-1] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[:-2, 1:-1] + P[:-2, 2:])
    return int((gx * gx + gy * gy).sum())


def _cfg(w, h, n=4, scale=2, kind="rggb"):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(w, h, n, scale, kind == "mono")
    if kind != "mono":
        for i, c in enumerate(CFAS[kind]):
            cfg.cfa[i] = c
    return cfg


def _random_frames(n, w, h, seed, pad=0, offset=0):
    """n random full-range u16 frames on the device as [h, w] views; pad / offset make pitched, shifted rows."""
    g = np.random.default_rng(seed)
    host = [g.integers(0, 65536, size=(h, w), dtype=np.uint16) for _ in range(n)]
    out = []
    for a in host:
        big = torch.zeros(h, w + pad + offset, dtype=torch.int16, device="cuda:0")
        v = big[:, offset:offset + w]
        v.copy_(torch.from_numpy(a.view(np.int16)).to("cuda:0"))
        out.append(v)
    return host, out


def _check(cfg, host, dev, rect, mono=False):
    from multi_frame_super_resolution_amd.pipeline import frame_sharpness, sharpness_rect
    got = frame_sharpness(dev, cfg, rect).cpu().tolist()
    r = sharpness_rect(cfg) if rect is None else rect
    want = [np_score(a, list(cfg.cfa), mono, r) for a in host]
    assert got == want


@pytest.mark.parametrize("kind", ["rggb", "bggr", "grbg", "gbrg", "mono"])
@pytest.mark.parametrize("pad,offset", [(0, 0), (12, 0), (3, 0), (0, 2), (5, 1)])
def test_sums_equal_numpy_small(kind, pad, offset):
    W, H = 260, 196  # half-res 130 x 98: not multiples of the 4 x 64-column strips nor of the row bands
    cfg = _cfg(W, H, kind=kind)
    host, dev = _random_frames(5, W, H, seed=100 * len(kind) + 10 * pad + offset, pad=pad, offset=offset)
    for rect in (None, (1, 1, W // 2 - 1, H // 2 - 1), (1, 1, 2, 2), (W // 2 - 2, H // 2 - 2, W // 2 - 1, H // 2 - 1),
                 (5, 90, 6, 97), (63, 17, 71, 50), (1, 40, W // 2 - 1, 41), (64, 1, 65, H // 2 - 1)):
        _check(cfg, host, dev, rect, kind == "mono")


# the even sizes the exposure tests sweep (test_exposure_gpu._SIZES): the score shares its loader and band planner with
# mfsr_frameLevels.  6 x 6 is the smallest frame a rectangle fits in (hw = 3: no 16-byte loads, every lane but one clamped);
# 2056 x 12 has five strips and one band
_SIZES = [(70, 38), (258, 130), (1000, 602), (500, 8), (498, 60), (6, 6), (8, 6), (6, 16), (1032, 18), (1026, 40), (2056, 12)]


@pytest.mark.parametrize("w,h", _SIZES)
def test_geometry_noise(w, h):
    cfg = _cfg(w, h)
    hw, hh = w // 2, h // 2
    # the whole scorable rectangle and the single quads at its two corners (one and the same where hw = 3 or hh = 3)
    rects = list(dict.fromkeys([(1, 1, hw - 1, hh - 1), (1, 1, 2, 2), (hw - 2, hh - 2, hw - 1, hh - 1)]))
    for pad, offset in ((0, 0), (8, 0), (3, 1)):
        host, dev = _random_frames(3, w, h, seed=w * 7 + h, pad=pad, offset=offset)
        for rect in rects:
            _check(cfg, host, dev, rect)


@pytest.mark.parametrize("n", [1, 5, 70])
def test_sums_equal_numpy_frame_counts(n):
    W, H = 260, 196
    cfg = _cfg(W, H)
    host, dev = _random_frames(n, W, H, seed=n)
    _check(cfg, host, dev, None)
    _check(cfg, host, dev, (3, 2, 127, 95))


@pytest.mark.parametrize("kind,pad", [("rggb", 0), ("gbrg", 8)])
def test_sums_equal_numpy_4k(kind, pad):
    W, H = 3840, 2160
    cfg = _cfg(W, H, kind=kind)
    host, dev = _random_frames(2, W, H, seed=7, pad=pad)
    _check(cfg, host, dev, None)
    _check(cfg, host, dev, (1, 1, W // 2 - 1, H // 2 - 1))
    _check(cfg, host, dev, (777, 333, 1500, 1001))


def test_max_gradient_at_max_area_is_exact():
    """Columns of 65535 / 0 four raw columns wide: every half-res column has |gx| = 4 * 131070, gy = 0, over exactly 2^23
    pixels -- the largest sum the contract admits (just under 2^61.3), exact, no overflow."""
    from multi_frame_super_resolution_amd.pipeline import frame_sharpness
    hw, hh = 4096 + 2, 2048 + 2
    W, H = 2 * hw, 2 * hh
    cols = np.where((np.arange(W) // 2) % 4 < 2, 65535, 0).astype(np.uint16)
    raw = np.broadcast_to(cols, (H, W)).copy()
    cfg = _cfg(W, H, n=1)
    rect = (1, 1, hw - 1, hh - 1)
    assert (rect[2] - rect[0]) * (rect[3] - rect[1]) == 1 << 23
    dev = torch.from_numpy(raw.view(np.int16)).to("cuda:0")
    got = int(frame_sharpness([dev], cfg, rect).cpu()[0])
    assert got == (1 << 23) * (4 * 131070) ** 2
    assert got == np_score(raw, list(cfg.cfa), False, rect)


# ---- selection on a real burst ----------------------------------------------------------------------------------------
def _blur_cfa(raw: torch.Tensor) -> torch.Tensor:
    """3x3 box blur of every CFA plane (edge-replicated), rounded back to integers."""
    out = raw.clone()
    x = raw.to(torch.float32)
    for dy in (0, 1):
        for dx in (0, 1):
            p = x[dy::2, dx::2][None, None]
            p = torch.nn.functional.pad(p, (1, 1, 1, 1), mode="replicate")
            out[dy::2, dx::2] = torch.round(torch.nn.functional.avg_pool2d(p, 3, stride=1)[0, 0]).to(raw.dtype)
    return out


def _burst(n, sharp, W=256, H=192, seed=5):
    from multi_frame_super_resolution_amd.synth import make_burst
    fr, _, _ = make_burst(W, H, n, scale=2, seed=seed, max_shift=3.0)
    return [(f if k in sharp else _blur_cfa(f)).to("cuda:0").contiguous() for k, f in enumerate(fr)]


@pytest.mark.parametrize("k", [0, 2, 4])
def test_selection_picks_the_sharp_frame(k):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, frame_sharpness
    W, H, N = 256, 192, 5
    frames = _burst(N, {k}, W, H)
    cfg = _cfg(W, H, N)
    sums = frame_sharpness(frames, cfg).cpu().tolist()
    pipe = BurstPipeline(cfg)
    pipe.process_selected(frames)
    assert pipe.selection.reference == k and pipe.selection.kept == list(range(N)) and pipe.selection.sums == sums
    if k > 0:  # the sharp frame is not among the candidates
        for c in range(1, k + 1):
            pipe.process_selected(frames, candidates=c)
            assert pipe.selection.reference == int(np.argmax(sums[:c])) != k
    blurred = max(s for i, s in enumerate(sums) if i != k)
    ratio = (blurred / sums[k] + 1.0) / 2.0
    pipe.process_selected(frames, keep_ratio=ratio)
    assert pipe.selection.reference == k and pipe.selection.kept == [k]
    pipe.close()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("window", [None, (64, 48, 160, 96), (0, 0, 48, 32)])
def test_process_selected_equals_plain_burst(window):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, sharpness_rect
    W, H, N = 256, 192, 6
    frames = _burst(N, {1, 3, 4}, W, H, seed=9)   # frames 0, 2, 5 blurred
    cfg = _cfg(W, H, N)
    sel = BurstPipeline(cfg, window=window)
    # keep the sharp frames only: a ratio between the best blurred and the worst sharp score over the scored rectangle
    sel.process_selected(frames)
    s = sel.selection.sums
    ratio = (max(s[i] for i in (0, 2, 5)) + min(s[i] for i in (1, 3, 4))) / 2.0 / max(s)
    out, out16 = sel.process_selected(frames, keep_ratio=ratio)
    out, out16 = out.clone(), out16.clone()
    r, kept = sel.selection.reference, sel.selection.kept
    assert r in (1, 3, 4) and kept == [1, 3, 4]
    assert sel.selection.rect == sharpness_rect(cfg, None if window is None else sel.window.aligned)
    cfg_r = _cfg(W, H, N)
    cfg_r.reference = r
    plain = BurstPipeline(cfg_r, window=window)
    want, want16 = plain.process(frames, frame_ids=kept)
    assert torch.equal(_bits(out), _bits(want)) and torch.equal(out16, want16)
    sel.close()
    plain.close()


def test_window_footprint_rule():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, sharpness_rect
    W, H, N = 256, 192, 3
    frames = _burst(N, {0, 1, 2}, W, H)
    for scale, window, want in ((2, (64, 48, 160, 96), (16, 12, 56, 36)),
                                (2, (0, 0, 48, 32), (1, 1, 12, 8)),
                                (2, (480, 352, 32, 32), (120, 88, 127, 95)),
                                (4, (96, 32, 48, 16), (12, 4, 18, 6))):
        cfg = _cfg(W, H, N, scale)
        assert sharpness_rect(cfg, window) == want
        p = BurstPipeline(cfg, window=window)
        p.process_selected(frames)
        assert p.selection.rect == want
        p.close()
    cfg = _cfg(W, H, N)
    p = BurstPipeline(cfg)
    p.process_selected(frames)
    assert p.selection.rect == (8, 8, W // 2 - 8, H // 2 - 8) == sharpness_rect(cfg)
    p.close()


# ---- CLI: MFSR_SELECT ------------------------------------------------------------------------------------------------
def _city(tmp_path, sharp_index):
    from PIL import Image
    from multi_frame_super_resolution_amd.synth import _scene, _shifted
    gen = torch.Generator().manual_seed(3)
    scene = _scene(256 * 2 + 64, 512 * 2 + 64, gen, "cpu")
    shifts = [(0, 0), (1.3, -2.1), (-3.2, 0.6), (2.4, 2.9), (-1.1, -1.7)]
    for i, (dx, dy) in enumerate(shifts):
        sh = _shifted(scene, dx * 2, dy * 2)[:, 32:32 + 512, 32:32 + 1024]
        lr = torch.nn.functional.avg_pool2d(sh[None], 2)[0]
        if i != sharp_index:
            lr = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(lr[None], (1, 1, 1, 1), mode="replicate"), 3, stride=1)[0]
        img = (lr.permute(1, 2, 0).clamp(0, 1) * 255).round().byte().numpy()
        Image.fromarray(img).save(tmp_path / f"img_{i + 1:06d}.png")


def test_cli_select_reports_the_sharp_frame(tmp_path):
    assert os.path.exists(CLI), "build apps/multi_frame_sr first (__graft_entry__.build())"
    _city(tmp_path, 2)  # img_000003.png (index 2) is the only sharp frame
    env = dict(os.environ, MFSR_SELECT="0")
    p = subprocess.run([CLI, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    assert "reference 2, kept 5 of 5" in p.stderr
    assert "reference" not in p.stdout and " sec" in p.stdout and " FPS" in p.stdout
    assert (tmp_path / "city_farneback_sr_result.png").exists() and (tmp_path / "city_farneback_sr2_result.png").exists()
    # a keep ratio of 1 keeps the reference only
    env["MFSR_KEEP_RATIO"] = "1"
    p = subprocess.run([CLI, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    assert "reference 2, kept 1 of 5" in p.stderr


def test_cli_select_refuses_multi_gpu(tmp_path):
    assert os.path.exists(CLI), "build apps/multi_frame_sr first (__graft_entry__.build())"
    _city(tmp_path, 2)
    env = dict(os.environ, MFSR_SELECT="0", MFSR_GPUS="2", MFSR_VIRTUAL_RANKS="1")
    p = subprocess.run([CLI, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode != 0
    assert "MFSR_SELECT" in p.stderr
    assert not (tmp_path / "city_farneback_sr_result.png").exists()
