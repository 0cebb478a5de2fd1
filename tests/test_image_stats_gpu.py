"""Image statistics, auto white balance and auto tone on the GPU: the statistics kernel against the numpy
restatement (tests/image_stats_ref.py) word for word, its contention cases, additivity over stripes and windows, the finish form
against the image form, the burst driver against the restatement's fits, a cast burst, and the CLI."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from multi_frame_super_resolution_amd import capi, synth
from tests import image_stats_ref as S
from tests import render_ref as R
from tests import yuv_ref as Y
from tests.kernels import guarded_upload
from tests.test_render_gpu import CCM, _pixels

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
WORDS = S.WORDS
PAD_VALUE = 1.0e9     # what the bytes between a padded row's pixels and the next row hold: never read


def _params(m=None, lo=64, hi=3967, chroma_tol=0):
    p = capi.ImageStatsParams()
    p.lo, p.hi, p.chromaTol = lo, hi, chroma_tol
    if m is not None:
        p.useMatrix = 1
        p.matrix = (ctypes.c_float * 9)(*[float(v) for v in m])
    return p


def _table(fill=0):
    """the device table between two guards, as an int64 tensor, and its check"""
    return guarded_upload(np.full(WORDS, fill, np.int64))


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _upload(p, pad_floats):
    """the image on the device with rows of 12 w + 4 pad_floats bytes -> (tensor, row bytes, check)"""
    h, w = p.shape[:2]
    rows = np.full((h, 3 * w + pad_floats), PAD_VALUE, np.float32)
    rows[:, :3 * w] = p.reshape(h, 3 * w)
    d, check = guarded_upload(rows)
    return d, 4 * (3 * w + pad_floats), check


def _diff(got, want):
    bad = np.flatnonzero(got != want)
    return f"{bad.size} words differ, first {bad[:6]}: got {got[bad[:6]]}, want {want[bad[:6]]}"


def _run_image(p, combos=None):
    """mfsr_imageStats of p for every (matrix, chromaTol, padding) against the restatement; returns the number of launches"""
    L = capi.lib()
    h, w = p.shape[:2]
    n = 0
    wants = {}
    for pad in (0, 2):
        d_in, rb, check_in = _upload(p, pad)
        for use_m, tol in combos or itertools.product((False, True), (0, 64)):
            m = CCM if use_m else None
            if (use_m, tol) not in wants:
                wants[use_m, tol] = S.stats(p, m, 64, 3967, tol)
            d_t, check_t = _table()
            par = _params(m, chroma_tol=tol)
            L.imageStats(d_in.data_ptr(), rb, w, h, ctypes.byref(par), d_t.data_ptr(), None)
            what = f"{w}x{h} matrix={use_m} chromaTol={tol} rowBytes={rb}"
            check_t(what)
            got = _host(d_t)
            assert np.array_equal(got, wants[use_m, tol]), what + ": " + _diff(got, wants[use_m, tol])
            n += 1
        check_in(f"{w}x{h} rowBytes={rb}", unchanged=True)
    return n


# ---- 1. the kernel against the restatement ---------------------------------------------------------------------------------
def test_imageStats_equals_the_restatement_on_small_images():
    n = 0
    for w, h in itertools.product((1, 2, 3, 5, 63, 64, 65, 130, 257), (1, 3, 37)):
        n += _run_image(_pixels(h, w, 1000 * w + h))
    assert n == 27 * 8


def test_imageStats_equals_the_restatement_over_several_workgroups():
    """1024 x 513: 256 quads per row, so a workgroup's chunk is at least 4 rows and the launch has more than a hundred
    workgroups whose chunk boundaries fall inside the image; the last chunk is a single row"""
    assert _run_image(_pixels(513, 1024, 77)) == 8


# ---- 2. contention: every lane of a wave on one counter, on two, and on counter 0 --------------------------------------------------
@pytest.mark.parametrize("kind", ["constant", "two_valued", "nan"])
def test_imageStats_contention(kind):
    h, w = 513, 1024
    p = np.empty((h, w, 3), np.float32)
    if kind == "constant":
        p[:] = np.array([0.5, 0.25, 0.75], np.float32)
    elif kind == "two_valued":      # neighbouring pixels differ: both keys in every wave
        p[:] = np.array([0.2, 0.21, 0.19], np.float32)
        p[:, 1::2] = np.array([0.8, 0.79, 0.81], np.float32)
    else:
        p[:] = np.nan
    want = S.stats(p, None, 64, 3967, 64)
    assert np.count_nonzero(want[8:]) == (4 if kind == "two_valued" else 2)
    assert _run_image(p, combos=[(False, 64), (True, 0)]) == 4


# ---- 3. the finish form: additivity, and equality with the image form --------------------------------------------------------------
FW, FH, FBW, FBH, THR = 130, 37, 65, 19, 1e-3
_fin = {}


def _finish_inputs():
    """the construction of test_render_gpu.test_finishRendered_equals_the_chain: the left 64 columns of rows 0..19 above the
    threshold, a checkerboard of sub-threshold weights elsewhere; uploaded once, checked unchanged by every user"""
    if not _fin:
        rng = np.random.default_rng(11)
        fin = rng.uniform(0, 2, (FH, FW, 3)).astype(np.float32)
        wt = rng.uniform(0.5, 2, (FH, FW, 3)).astype(np.float32)
        low = ((np.add.outer(np.arange(FH), np.arange(FW)) % 3) == 0)
        low[:20, :64] = False
        wt[low] = np.array([0.0, 5e-4, 0.7], np.float32)
        fb = rng.uniform(0, 1, (FBH, FBW, 3)).astype(np.float32)
        _fin["dev"] = [guarded_upload(a) for a in (fin, wt, fb)]
    return _fin["dev"]


def _finish_stats(table, par, x0=0, y0=0, w=FW, h=FH):
    (d_fin, _), (d_wt, _), (d_fb, _) = _finish_inputs()
    o = 12 * (y0 * FW + x0)
    capi.lib().finishStats(d_fin.data_ptr() + o, d_wt.data_ptr() + o, 12 * FW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0,
                           w, h, THR, x0, y0, FW, FH, ctypes.byref(par), table.data_ptr(), None)


def _inputs_unchanged(what):
    for _, check in _finish_inputs():
        check(what, unchanged=True)


@pytest.mark.parametrize("use_m,tol", [(False, 0), (True, 64)])
def test_finishStats_equals_imageStats_of_the_float_image(use_m, tol):
    L = capi.lib()
    (d_fin, _), (d_wt, _), (d_fb, _) = _finish_inputs()
    d_lin, check_lin = guarded_upload(np.zeros((FH, FW, 3), np.float32))
    L.finishFusedWindow(d_fin.data_ptr(), d_wt.data_ptr(), 12 * FW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0,
                        d_lin.data_ptr(), 12 * FW, None, FW, FH, THR, 0, 65535.0, 0, 0, FW, FH, None)
    check_lin("float image")
    par = _params(CCM if use_m else None, chroma_tol=tol)
    d_a, check_a = _table()
    L.imageStats(d_lin.data_ptr(), 12 * FW, FW, FH, ctypes.byref(par), d_a.data_ptr(), None)
    d_b, check_b = _table()
    _finish_stats(d_b, par)
    check_a("image form")
    check_b("finish form")
    want = S.stats(d_lin.cpu().numpy(), CCM if use_m else None, 64, 3967, tol)
    assert np.array_equal(_host(d_a), want), _diff(_host(d_a), want)        # (not a comparison of two equal mistakes)
    assert np.array_equal(_host(d_b), want), _diff(_host(d_b), want)
    assert 0 < int(want[1]) < FW * FH
    _inputs_unchanged("finishStats")


def test_finishStats_stripes_and_windows_add_up_and_a_launch_adds():
    par = _params(CCM, chroma_tol=64)
    d_whole, check_whole = _table()
    _finish_stats(d_whole, par)
    whole = _host(d_whole)
    assert int(whole[0]) == FW * FH and int(whole[8:8 + S.BINS].sum()) == FW * FH and int(whole[8 + S.BINS:].sum()) == FW * FH
    # two row stripes into one table
    d_t, check_t = _table()
    _finish_stats(d_t, par, 0, 0, FW, 16)
    _finish_stats(d_t, par, 0, 16, FW, FH - 16)
    check_t("stripes")
    assert np.array_equal(_host(d_t), whole), _diff(_host(d_t), whole)
    # the 64 x 16 window at (16, 16) and the four rectangles around it
    d_t, check_t = _table()
    for x0, y0, w, h in ((16, 16, 64, 16), (0, 0, FW, 16), (0, 32, FW, FH - 32), (0, 16, 16, 16), (80, 16, FW - 80, 16)):
        _finish_stats(d_t, par, x0, y0, w, h)
    check_t("window split")
    assert np.array_equal(_host(d_t), whole), _diff(_host(d_t), whole)
    # the window alone is the restatement of the crop: a second launch on the whole's table adds it
    d_win, _ = _table()
    _finish_stats(d_win, par, 16, 16, 64, 16)
    _finish_stats(d_whole, par, 16, 16, 64, 16)
    check_whole("second launch")
    assert np.array_equal(_host(d_whole), whole + _host(d_win))
    # ... and a table that did not start at zero keeps what it held
    d_t, check_t = _table(fill=5)
    _finish_stats(d_t, par)
    check_t("non-zero table")
    assert np.array_equal(_host(d_t), whole + np.uint64(5))
    _inputs_unchanged("additivity")


def test_both_entry_points_capture_into_a_graph():
    """asynchronous, nothing allocated: the clearing of the table and both launches captured on the capture stream and replayed
    twice on the same inputs give the eager table (the second replay starts from the cleared table again)"""
    L = capi.lib()
    (d_fin, _), (d_wt, _), (d_fb, _) = _finish_inputs()
    p = _pixels(37, 130, 9)
    d_in = torch.from_numpy(p).to(DEV)
    par = _params(CCM, chroma_tol=64)
    table = torch.zeros(WORDS, dtype=torch.int64, device=DEV)

    def both():
        stream = torch.cuda.current_stream().cuda_stream
        table.zero_()
        L.imageStats(d_in.data_ptr(), 12 * 130, 130, 37, ctypes.byref(par), table.data_ptr(), stream)
        L.finishStats(d_fin.data_ptr(), d_wt.data_ptr(), 12 * FW, d_fb.data_ptr(), 12 * FBW, FBW, FBH, 0.0, 1.0, 0.0, 1.0, FW, FH, THR,
                      0, 0, FW, FH, ctypes.byref(par), table.data_ptr(), stream)

    both()                                           # warm-up outside capture; the eager answer
    torch.cuda.synchronize()
    eager = table.cpu().numpy().copy()
    assert int(eager[0]) == 2 * 130 * 37
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(2):
        table.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(table.cpu().numpy(), eager)
    del graph
    _inputs_unchanged("graph")


# ---- 4. bursts --------------------------------------------------------------------------------------------------------------
W, H, N = 384, 256, 7
_cache = {}


def _frames(cast=None):
    if ("frames", cast) not in _cache:
        if cast is None:
            frames, _, _ = synth.make_burst(W, H, N, seed=29, device="cpu")
            _cache["frames", cast] = [f.contiguous() for f in frames]
        else:       # raw R and B sites scaled about the black level, in numpy
            out = []
            for f in _frames():
                a = f.numpy().view(np.uint16).astype(np.float64)
                a[0::2, 0::2] = np.rint((a[0::2, 0::2] - 256.0) * cast[0] + 256.0)
                a[1::2, 1::2] = np.rint((a[1::2, 1::2] - 256.0) * cast[1] + 256.0)
                out.append(torch.from_numpy(np.clip(a, 0, 4095).astype(np.uint16).view(np.int16)))
            _cache["frames", cast] = out
    return _cache["frames", cast]


def _config(fused=1):
    from multi_frame_super_resolution_amd.pipeline import default_config
    cfg = default_config(W, H, N, scale=2)
    cfg.applyGamma, cfg.fused = 0, fused
    return cfg


def _plain(fused=1, cast=None):
    """the plain float image and integer image of the burst (no render description, a pipeline that never measured): once per
    configuration, shared and left unchanged"""
    key = ("plain", fused, cast)
    if key not in _cache:
        from multi_frame_super_resolution_amd.pipeline import BurstPipeline
        pipe = BurstPipeline(_config(fused), DEV)
        img, q = pipe.process([f.to(DEV) for f in _frames(cast)])
        _cache[key] = (img.cpu().numpy().copy(), q.cpu().numpy().copy())
        pipe.close()
    return _cache[key]


def _fits(p, ccm=None, **kw):
    """the restatement's fits of the statistics of the float image p"""
    return S.auto(lambda m, lo, hi, ct: S.stats(p, m, lo, hi, ct), p.shape[0] * p.shape[1], ccm, **kw)


def _ulps(a, b):
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


def _check_installed(pipe, want, what):
    """the installed matrix and table against the restatement's: the matrix exact, the table within one float ulp (pow, log)"""
    r, res = pipe.auto_description, pipe.auto_result
    m = np.array(list(r.matrix), np.float32)
    assert r.useMatrix == 1 and np.array_equal(m.view(np.uint32), want["matrix"].view(np.uint32)), (what, m, want["matrix"])
    assert np.array_equal(np.array(list(res.gains), np.float32).view(np.uint32), want["gains"].view(np.uint32)), what
    lut = pipe.auto_lut.cpu().numpy()
    assert r.toneSize == lut.size - 1 == want["lut"].size - 1 and _ulps(lut, want["lut"]) <= 1, (what, _ulps(lut, want["lut"]))
    assert (res.black, res.white) == (want["black"], want["white"]) and abs(res.gamma - want["gamma"]) <= 1e-14, what
    assert (res.awbStatus, res.toneStatus) == (want["awb_status"], want["tone_status"]) and res.neutralShare == want["share"], what
    return m, lut


@pytest.mark.parametrize("fused", [1, 0])
def test_auto_burst_equals_the_restatement(fused):
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    p, q_plain = _plain(fused)
    pipe = BurstPipeline(_config(fused), DEV)
    # RGB8, with a colour matrix of the caller's
    img, q = pipe.process_auto(frames, format=capi.OUT_RGB8, matrix=CCM)
    want = _fits(p, CCM)
    assert want["awb_status"] == 0 and want["tone_status"] == 0 and want["black"] < want["white"]
    m, lut = _check_installed(pipe, want, f"RGB8 fused={fused}")
    want_f, want_q = R.render(p, R.RGB8, m, lut)
    assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy(), want_q)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    # NV12, without one
    img, q = pipe.process_auto(frames, format=capi.OUT_NV12)
    m, lut = _check_installed(pipe, _fits(p), f"NV12 fused={fused}")
    want_f, want_y, want_uv = Y.render(p, Y.NV12, m, lut)
    assert q.dtype == torch.uint8 and np.array_equal(q.cpu().numpy().reshape(3 * H, 2 * W), Y.as_bytes(want_y, want_uv))
    # both measurements off: bit for bit set_render with the caller's matrix
    res = None
    img, q = (t.clone() for t in pipe.process_auto(frames, format=capi.OUT_RGB8, matrix=CCM, awb=False, tone=False))
    res = pipe.auto_result
    assert tuple(res.gains) == (1.0, 1.0, 1.0) and (res.black, res.white, res.gamma) == (0.0, 1.0, 1.0)
    assert list(pipe.auto_description.matrix) == [float(v) for v in CCM] and not pipe.auto_description.toneLut
    pipe.set_render(capi.OUT_RGB8, matrix=CCM)
    img2, q2 = pipe.process(frames)
    assert torch.equal(q, q2) and torch.equal(img.view(torch.int32), img2.view(torch.int32))
    # set_render(None) turns it off again: the output of the pipeline that never measured
    pipe.set_render(None)
    img3, q3 = pipe.process(frames)
    assert q3.dtype == torch.int16 and np.array_equal(q3.cpu().numpy(), q_plain)
    assert np.array_equal(img3.cpu().numpy().view(np.uint32), p.view(np.uint32))
    pipe.close()


def test_auto_burst_in_a_zoom_window_measures_the_window():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    x, y, w, h = 240, 96, 160, 112          # on the 16-pixel grid, even extents: the library's window is the one asked for
    p = np.ascontiguousarray(_plain()[0][y:y + h, x:x + w])
    pw = BurstPipeline(_config(), DEV, window=(x, y, w, h))
    img, q = pw.process_auto([f.to(DEV) for f in _frames()], format=capi.OUT_NV12, matrix=CCM)
    m, lut = _check_installed(pw, _fits(p, CCM), "window")
    want_f, want_y, want_uv = Y.render(p, Y.NV12, m, lut)
    assert np.array_equal(q.cpu().numpy().reshape(3 * h // 2, w), Y.as_bytes(want_y, want_uv))
    assert np.array_equal(img.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    pw.close()


def test_auto_render_refuses_what_the_library_refuses():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    frames = [f.to(DEV) for f in _frames()]
    pipe = BurstPipeline(_config(), DEV)
    with pytest.raises(capi.MfsrError):      # no reference yet
        pipe.auto_render()
    pipe.begin_burst()
    pipe.set_reference(frames[0])
    for k, f in enumerate(frames):
        pipe.add_frame(f, k == 0)
    for bad in (dict(iterations=0), dict(iterations=5), dict(lo=-1), dict(hi=4096), dict(chroma_tol=70000), dict(max_gain=0.5),
                dict(matrix=[300, 0, 0, 0, 1, 0, 0, 0, 1]), dict(format=7)):
        with pytest.raises((capi.MfsrError, ValueError)):
            pipe.auto_render(**bad)
    with pytest.raises(TypeError):
        pipe.auto_render(no_such_parameter=1)
    _, q = pipe.finish()
    assert q.dtype == torch.int16 and np.array_equal(q.cpu().numpy(), _plain()[1])   # the refused calls changed nothing
    pipe.close()


# ---- 5. a cast burst --------------------------------------------------------------------------------------------------------
CAST = (0.6, 0.75)
# The restatement on the CPU oracle's merge of the plain and of the cast burst (tests/burst_compare.run_oracle, applyGamma 0)
# recovers the inverse cast with a relative error of 7.1e-7 on R and 4.11e-5 on B; twice the larger:
CAST_BOUND = 2 * 4.11e-5


def test_cast_burst_gains_recover_the_cast():
    from multi_frame_super_resolution_amd.pipeline import BurstPipeline
    gains = {}
    for cast in (None, CAST):
        pipe = BurstPipeline(_config(), DEV)
        pipe.process_auto([f.to(DEV) for f in _frames(cast)], format=capi.OUT_RGB8, tone=False)
        res = pipe.auto_result
        want = _fits(_plain(cast=cast)[0], tone=False)     # the restatement on the GPU's own float image: exactly equal
        got = np.array(list(res.gains), np.float32)
        assert res.awbStatus == 0 and np.array_equal(got.view(np.uint32), want["gains"].view(np.uint32)), (cast, got, want["gains"])
        assert res.neutralShare == want["share"] and res.neutralShare > 1 / 64
        gains[cast] = got.astype(np.float64)
        pipe.close()
    rel = gains[CAST] / gains[None]
    err = max(abs(rel[0] * CAST[0] - 1.0), abs(rel[2] * CAST[1] - 1.0))
    print(f"cast burst: gains {gains[CAST]} against {gains[None]}, relative error {err:.3g} (bound {CAST_BOUND:.3g})")
    assert rel[1] == 1.0 and err <= CAST_BOUND


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------
def test_cli_auto(tmp_path):
    import re
    from PIL import Image
    from tests.test_bundled_burst import CITY
    cli = os.path.join(ROOT, "apps", "multi_frame_sr")
    assert os.path.exists(cli), "build apps/multi_frame_sr first (__graft_entry__.build())"
    for i in range(5):          # the bundled frames with a cast on R and B
        a = np.asarray(Image.open(os.path.join(CITY, f"img_{i:06d}.png"))).astype(np.float32)
        a[..., 0] *= CAST[0]
        a[..., 2] *= CAST[1]
        Image.fromarray(np.rint(a).astype(np.uint8)).save(tmp_path / f"img_{i:06d}.png")
    env = dict(os.environ)
    for k in ("MFSR_AUTO", "MFSR_CCM", "MFSR_SHARPEN", "MFSR_GPUS"):
        env.pop(k, None)
    outs = {}
    for name, auto in (("plain", None), ("auto", "wb,tone")):
        e = dict(env, MFSR_AUTO=auto) if auto else env
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=300, env=e)
        assert p.returncode == 0, p.stderr
        outs[name] = np.asarray(Image.open(tmp_path / "city_farneback_sr_result.png")).copy()
        if auto:
            m = re.search(r"auto: gains (\S+) (\S+) (\S+) .*black (\S+) white (\S+) gamma (\S+)", p.stderr)
            assert m, p.stderr
            g = [float(v) for v in m.groups()]
            assert g[0] > 1.0 and g[1] == 1.0 and g[2] > 1.0 and 0.0 <= g[3] < g[4] and 0.5 <= g[5] <= 2.0, p.stderr
        else:
            assert "auto:" not in p.stderr
    assert outs["auto"].shape == outs["plain"].shape and not np.array_equal(outs["auto"], outs["plain"])
    # the cast is gone from the balanced image: its channel means are closer together than the plain run's
    spread = {k: np.ptp(v.reshape(-1, 3).mean(axis=0)) for k, v in outs.items()}
    assert spread["auto"] < spread["plain"], spread
    p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=60,
                       env=dict(env, MFSR_AUTO="wb,tone", MFSR_GPUS="2"))
    assert p.returncode != 0 and "MFSR_AUTO" in p.stderr
    for bad in ("", "wb,", "tone,wb,x", "white"):
        p = subprocess.run([cli, "farneback", "city", "3"], cwd=tmp_path, capture_output=True, text=True, timeout=60,
                           env=dict(env, MFSR_AUTO=bad))
        assert p.returncode != 0 and "MFSR_AUTO" in p.stderr, bad
