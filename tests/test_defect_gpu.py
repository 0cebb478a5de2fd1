"""Defective pixels on the GPU: mfsr_detectDefects and mfsr_repairDefects equal the numpy restatement of the rule
(tests/test_defect_cpu.py) bit for bit, process_repaired is bit for bit the plain burst of numpy-repaired frames, the repair
lowers the error around the defects, and the CLI's MFSR_DEFECTS reports and repairs them.  All comparisons are equalities."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.test_defect_cpu import FIXTURES, default_votes, defect_positions, detect, fixture, repair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "apps", "multi_frame_sr")
PAD_BYTE = 0xAB


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


def _np16(t):
    return t.cpu().numpy().view(np.uint16)


def _detect_gpu(dev, w, h, mono, threshold, spread, votes, map_pad=0):
    """(map [h, w] numpy, (hot, cold)) through the C-ABI with a pitched map; checks that the map's padding is untouched."""
    from multi_frame_super_resolution_amd import capi
    n = len(dev)
    big = torch.full((h, w + map_pad), PAD_BYTE, dtype=torch.uint8, device="cuda:0")
    counts = torch.full((2,), 77, dtype=torch.int32, device="cuda:0")
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in dev])
    capi.lib().detectDefects(n, ptrs, dev[0].stride(0) * 2, w, h, 1 if mono else 0, threshold, spread, votes, big.data_ptr(),
                             big.stride(0), counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    m = big.cpu().numpy()
    assert (m[:, w:] == PAD_BYTE).all(), "the map's pitch padding was written"
    return m[:, :w].copy(), tuple(counts.cpu().tolist())


def _repair_gpu(dev, w, h, mono, dmap, map_pad=0):
    """In place on `dev` through the C-ABI with a pitched map."""
    from multi_frame_super_resolution_amd import capi
    n = len(dev)
    big = torch.full((h, w + map_pad), PAD_BYTE, dtype=torch.uint8, device="cuda:0")
    big[:, :w].copy_(torch.from_numpy(dmap).to("cuda:0"))
    ptrs = (ctypes.c_void_p * n)(*[f.data_ptr() for f in dev])
    capi.lib().repairDefects(n, ptrs, dev[0].stride(0) * 2, w, h, 1 if mono else 0, big.data_ptr(), big.stride(0),
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(big.cpu().numpy()[:, :w], dmap) and (big.cpu().numpy()[:, w:] == PAD_BYTE).all()


def _check(host, mono, threshold, spread, votes, pad=0, offset=0, map_pad=0, need_both=False, check_repair=True):
    h, w = host[0].shape
    d = 1 if mono else 2
    dev, backs = _to_dev(host, pad, offset)
    before = [b.clone() for b in backs]
    got, counts = _detect_gpu(dev, w, h, mono, threshold, spread, votes, map_pad)
    want = detect(host, d, threshold, spread, votes)
    nh, nc = int((want == 1).sum()), int((want == 2).sum())
    print(f"{w}x{h} n={len(host)} d={d} thr={threshold} spread={spread} votes={votes}: {nh} hot, {nc} cold")
    assert np.array_equal(got, want)
    assert counts == (nh, nc)
    if need_both:
        assert nh > 0 and nc > 0
    for a, b in zip(before, backs):
        assert torch.equal(a, b), "detection wrote to a frame"
    if check_repair:
        _repair_gpu(dev, w, h, mono, want, map_pad)
        for k, a in enumerate(host):
            assert np.array_equal(_np16(dev[k]), repair(a, want, d)), f"frame {k}"
        for a, b in zip(before, backs):  # the frames' pitch padding
            if pad or offset:
                assert torch.equal(a[:, :offset], b[:, :offset]) and torch.equal(a[:, offset + w:], b[:, offset + w:])


def _noise(n, w, h, seed, shared=0.0):
    """n full-range u16 noise frames; `shared`: the fraction of pixels every frame takes from one common pattern, so that
    many pixels collect a majority of votes."""
    g = np.random.default_rng(seed)
    base = g.integers(0, 65536, size=(h, w), dtype=np.uint16)
    out = []
    for _ in range(n):
        a = g.integers(0, 65536, size=(h, w), dtype=np.uint16)
        keep = g.random((h, w)) < shared
        a[keep] = base[keep]
        out.append(a)
    return out


# ---- 5 / 6: detection and repair against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("w,h,n,mono", FIXTURES)
def test_fixture_bursts(w, h, n, mono):
    _, bad, want, _ = fixture(w, h, n, mono)
    _check(bad, mono, 59, 2, default_votes(n))
    dev, _ = _to_dev(bad)
    got, counts = _detect_gpu(dev, w, h, mono, 59, 2, default_votes(n))
    assert np.array_equal(got, want) and counts == (150, 150)


# the smallest Bayer frame is 5 x 5; 248 m + 1 / + 2 wide: the last output column of the last strip but one has its right
# neighbour outside the frame
_SIZES = [(70, 38), (258, 130), (1000, 602), (5, 5), (12, 5), (496, 9), (500, 8), (249, 12), (497, 60), (498, 11), (745, 60),
          (993, 40)]


@pytest.mark.parametrize("w,h,mono", [(w, h, False) for w, h in _SIZES] + [(w, h, True) for w, h in _SIZES + [(3, 3), (3, 7)]])
def test_geometry_noise(w, h, mono):
    n = 5
    host = _noise(n, w, h, seed=w * 7 + h, shared=0.5)
    big = w * h > 2000
    _check(host, mono, 0, 0, n // 2 + 1, need_both=big)
    _check(host, mono, 59, 2, n // 2 + 1, pad=6, map_pad=5)
    _check(host, mono, 0, 16, n // 2 + 1, pad=3, offset=1, map_pad=1)
    _check(host, mono, 65535, 0, n, pad=8, map_pad=16)
    _check(host[:1], mono, 0, 0, 1, need_both=big)               # one frame: a densely populated map
    _check(host[:1], mono, 1000, 1, 1, pad=4, offset=2, map_pad=3)


@pytest.mark.parametrize("mono", [False, True])
def test_frame_counts_1_and_64(mono):
    w, h = 258, 130
    host = _noise(64, w, h, seed=64, shared=0.7)
    _check(host, mono, 0, 0, 33, need_both=True)
    _check(host, mono, 0, 0, 64)
    _check(host, mono, 300, 2, 48, pad=2)
    _check(host[:1], mono, 0, 0, 1, need_both=True)
    _check(host[:2], mono, 0, 0, 2, need_both=True)


def test_4k_pair():
    w, h = 3840, 2160
    host = _noise(2, w, h, seed=4, shared=0.6)
    _check(host, False, 0, 1, 2, need_both=True)


@pytest.mark.parametrize("mono", [False, True])
def test_repair_hand_made_map(mono):
    w, h, d = 70, 38, 1 if mono else 2
    host = _noise(3, w, h, seed=9)
    m = np.zeros((h, w), np.uint8)
    m[10, 10] = m[10, 10 + d] = 1                       # flagged same-colour neighbours next to each other
    m[20 - d:20 + d + 1:d, 30 - d:30 + d + 1:d] = 2     # a fully flagged 3 x 3 lattice neighbourhood: the centre stays
    m[0, 0] = m[0, w - 1] = m[h - 1, 0] = m[h - 1, w - 1] = 1
    m[0, d] = 2                                         # a corner with a flagged neighbour
    m[5, 40] = 200                                      # any non-zero entry is a defect
    for pad, map_pad in ((0, 0), (5, 3)):
        dev, _ = _to_dev(host, pad)
        _repair_gpu(dev, w, h, mono, m, map_pad)
        for k, a in enumerate(host):
            want = repair(a, m, d)
            assert want[20, 30] == a[20, 30]
            assert np.array_equal(_np16(dev[k]), want)


def test_python_entry_points():
    from multi_frame_super_resolution_amd.pipeline import default_config, detect_defects, repair_defects
    w, h, n, mono = FIXTURES[2]
    _, bad, want, _ = fixture(w, h, n, mono)
    cfg = default_config(w, h, n, 2, mono)
    dev, _ = _to_dev(bad, pad=4)
    dmap, counts = detect_defects(dev, cfg)
    assert np.array_equal(dmap.cpu().numpy(), want) and counts == (150, 150)
    fixed = repair_defects(dev, dmap, cfg)
    for k, a in enumerate(bad):
        assert np.array_equal(_np16(dev[k]), a)                      # the caller's frames stay
        assert np.array_equal(_np16(fixed[k]), repair(a, want, 2))


# ---- 7: process_repaired --------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _dense(host):
    return [torch.from_numpy(a.view(np.int16).copy()).to("cuda:0") for a in host]


@pytest.mark.parametrize("window,select", [(None, False), ((64, 48, 160, 96), False), (None, True), ((0, 0, 48, 32), True)])
def test_process_repaired_equals_plain_burst_of_repaired_frames(window, select):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    w, h, n, mono = FIXTURES[2]
    _, bad, want, _ = fixture(w, h, n, mono)
    cfg = default_config(w, h, n, 2, mono)
    bad_dev = _dense(bad)
    fixed_dev = _dense([repair(a, want, 2) for a in bad])
    a = BurstPipeline(cfg, window=window)
    out, out16 = a.process_repaired(bad_dev, select=select, keep_ratio=0.5 if select else 0.0)
    got = (out.clone(), out16.clone(), a.img_out.clone(), a.total_weights.clone())
    assert a.defects == (150, 150)
    assert np.array_equal(a.defect_map.cpu().numpy(), want)
    for k, f in enumerate(bad):
        assert np.array_equal(_np16(bad_dev[k]), f)                  # the caller's frames stay
    b = BurstPipeline(cfg, window=window)
    if select:
        o, o16 = b.process_selected(fixed_dev, keep_ratio=0.5)
        assert a.selection == b.selection
    else:
        o, o16 = b.process(fixed_dev)
    ref = (o, o16, b.img_out, b.total_weights)
    for x, y in zip(got, ref):
        assert x.shape == y.shape and torch.equal(_bits(x), _bits(y))
    a.close()
    b.close()


# ---- 8: the point of the feature ------------------------------------------------------------------------------------------
def test_repair_lowers_the_error_around_the_defects():
    """e(X) = mean squared error of the finished float image of burst X against the synthetic scene's ground truth over the
    HR pixels within 2 s of an injected defect's footprint (512 x 384 x 8 RGGB at x2, 300 stuck pixels).  The fixed condition
    is the strict ordering e(repaired) < e(bad); the three values are printed (and recorded in DESIGN.md section 2.13).
    Measured on an MI355X: e(clean) = 1.816716e-03, e(repaired) = 1.837826e-03, e(bad) = 3.887326e-03 over 29404 HR pixels."""
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline, default_config
    w, h, n, mono = FIXTURES[2]
    s = 2
    clean, bad, want, gt = fixture(w, h, n, mono)
    cfg = default_config(w, h, n, s, mono)
    near = np.zeros((s * h, s * w), bool)
    for x, y, _ in defect_positions(w, h):   # footprint [s x, s x + s) x [s y, s y + s), grown by 2 s
        near[max(0, s * y - 2 * s):s * y + s + 2 * s, max(0, s * x - 2 * s):s * x + s + 2 * s] = True
    truth = gt.permute(1, 2, 0).numpy().astype(np.float64)
    pipe = BurstPipeline(cfg)

    def err(out):
        img = out.cpu().numpy().astype(np.float64)
        assert img.shape == truth.shape
        return float(((img - truth) ** 2)[near].mean())

    e_clean = err(pipe.process(_dense(clean))[0])
    e_bad = err(pipe.process(_dense(bad))[0])
    e_rep = err(pipe.process_repaired(_dense(bad))[0])
    pipe.close()
    print(f"e(clean) = {e_clean:.6e}, e(repaired) = {e_rep:.6e}, e(bad) = {e_bad:.6e} over {int(near.sum())} HR pixels")
    assert e_rep < e_bad


# ---- 9: CLI ----------------------------------------------------------------------------------------------------------------
def _write_burst(d, frames):
    """Five 12-bit RGGB mosaics as 16-bit single-channel TIFFs under the CLI's fixed `city` names (content is sniffed)."""
    from PIL import Image
    d.mkdir()
    for i, a in enumerate(frames):
        Image.fromarray((a.astype(np.uint16) << 4)).save(d / f"img_{i + 1:06d}.png", format="TIFF")


def _run_cli(d, **env):
    return subprocess.run([CLI, "farneback", "city", "3"], cwd=d, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, **env))


def test_cli_defects(tmp_path):
    from PIL import Image
    assert os.path.exists(CLI), "build apps/multi_frame_sr first (__graft_entry__.build())"
    w, h, n, mono = 512, 384, 8, False
    _, bad, want, _ = fixture(w, h, n, mono)
    bad = bad[:5]
    # the CLI's white level for 16-bit input is 4095: threshold 4095 // 64 = 63; 5 frames: 4 votes
    m = detect(bad, 2, 63, 2, 4)
    nh, nc = int((m == 1).sum()), int((m == 2).sum())
    assert np.array_equal(m, want) and (nh, nc) == (150, 150)   # the injected defects, all of them and nothing else
    _write_burst(tmp_path / "bad", bad)
    _write_burst(tmp_path / "fixed", [repair(a, m, 2) for a in bad])
    p = _run_cli(tmp_path / "bad", MFSR_DEFECTS="1")
    assert p.returncode == 0, p.stderr
    assert f"defects: {nh} hot, {nc} cold" in p.stderr
    assert "defects" not in p.stdout and " sec" in p.stdout and " FPS" in p.stdout
    repaired = {k: (tmp_path / "bad" / f"city_farneback_{k}_result.png").read_bytes() for k in ("sr", "sr2")}
    q = _run_cli(tmp_path / "fixed")
    assert q.returncode == 0, q.stderr
    assert "defects" not in q.stderr
    for k in ("sr", "sr2"):
        assert repaired[k] == (tmp_path / "fixed" / f"city_farneback_{k}_result.png").read_bytes()
    # MFSR_DEFECTS=0 and no variable at all: the same output, and not the repaired one
    q0 = _run_cli(tmp_path / "bad", MFSR_DEFECTS="0")
    plain0 = (tmp_path / "bad" / "city_farneback_sr_result.png").read_bytes()
    q1 = _run_cli(tmp_path / "bad")
    assert q0.returncode == 0 and q1.returncode == 0 and "defects" not in q1.stderr
    assert plain0 == (tmp_path / "bad" / "city_farneback_sr_result.png").read_bytes() != repaired["sr"]
    # explicit parameters reach the library: all five frames must agree, no spread
    m2 = detect(bad, 2, 100, 0, 5)
    p = _run_cli(tmp_path / "bad", MFSR_DEFECTS="1", MFSR_DEFECT_THRESHOLD="100", MFSR_DEFECT_SPREAD="0", MFSR_DEFECT_VOTES="5")
    assert p.returncode == 0 and f"defects: {int((m2 == 1).sum())} hot, {int((m2 == 2).sum())} cold" in p.stderr
    for bad_env in (dict(MFSR_DEFECTS="yes"), dict(MFSR_DEFECTS="1", MFSR_DEFECT_VOTES="2"),
                    dict(MFSR_DEFECTS="1", MFSR_DEFECT_SPREAD="17"), dict(MFSR_DEFECTS="1", MFSR_DEFECT_THRESHOLD="-1")):
        r = _run_cli(tmp_path / "bad", **bad_env)
        assert r.returncode != 0 and "MFSR_DEFECT" in r.stderr


def test_cli_defects_refuses_multi_gpu(tmp_path):
    assert os.path.exists(CLI), "build apps/multi_frame_sr first (__graft_entry__.build())"
    _, bad, _, _ = fixture(256, 192, 8, True)
    _write_burst(tmp_path / "b", bad[:5])
    p = _run_cli(tmp_path / "b", MFSR_DEFECTS="1", MFSR_GPUS="2", MFSR_VIRTUAL_RANKS="1")
    assert p.returncode != 0
    assert "MFSR_DEFECTS" in p.stderr
    assert not (tmp_path / "b" / "city_farneback_sr_result.png").exists()
