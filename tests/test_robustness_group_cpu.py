"""Host-side checks of the group robustness path (no GPU needed): mfsr_prepareFrameMeansBatch and mfsr_robustnessMaskGroup
validate their arguments before any device call, and the switch is callable through capi.  Every call below carries exactly
one bad argument (the pointers are made-up addresses that the host never dereferences), so nothing is ever launched."""
import ctypes

from multi_frame_super_resolution_amd import capi

INVALID, UNSUPPORTED = -1, -2
W, H = 40, 24
A = 0x10000          # an address aligned for every buffer
TAPS = (ctypes.c_float * 5)(0.0625, 0.25, 0.375, 0.25, 0.0625)


def _prepare(**kw):
    a = dict(n=2, frames="ok", meansRowBytes=12 * W, maxVal=4095.0, w=W, h=H, pyr0RowBytes=4 * W, pyr1RowBytes=4 * (W // 2), taps=TAPS,
             ntaps=5, dataIn=A, halfOut=A, pyr0=A, pyr1=A)
    a.update(kw)
    fr = None
    if a["frames"] == "ok":
        fr = (capi.PrepareFrame * 4)(*[capi.PrepareFrame(a["dataIn"] if k == 1 else A, a["halfOut"] if k == 1 else A,
                                                         a["pyr0"] if k == 1 else A, a["pyr1"] if k == 1 else A) for k in range(4)])
    return capi.lib().raw["mfsr_prepareFrameMeansBatch"](a["n"], fr, a["meansRowBytes"], a["maxVal"], a["w"], a["h"], a["pyr0RowBytes"],
                                                         a["pyr1RowBytes"], a["taps"], a["ntaps"], None)


def test_prepare_means_checks_its_arguments_on_the_host():
    assert _prepare(frames=None) == INVALID
    assert _prepare(n=0) == INVALID and _prepare(n=5) == INVALID
    assert _prepare(taps=None) == INVALID
    assert _prepare(dataIn=None) == INVALID and _prepare(halfOut=None) == INVALID and _prepare(pyr0=None) == INVALID
    assert _prepare(pyr1=None) == INVALID                       # a second pyramid level for all frames or for none
    assert _prepare(dataIn=A + 2) == INVALID                     # raw quads are read as 4-byte words
    assert _prepare(meansRowBytes=12 * W - 4) == INVALID and _prepare(meansRowBytes=12 * W + 2) == INVALID
    assert _prepare(pyr0RowBytes=4 * W - 4) == INVALID and _prepare(pyr1RowBytes=4 * (W // 2) - 4) == INVALID
    assert _prepare(w=0) == INVALID and _prepare(h=0) == INVALID
    assert _prepare(ntaps=4) == INVALID and _prepare(ntaps=0) == INVALID
    # no halo to take the patch from / more taps than the tile's halo holds: refused, nothing launched
    assert _prepare(ntaps=1) == UNSUPPORTED
    assert _prepare(ntaps=19, taps=(ctypes.c_float * 19)()) == UNSUPPORTED


def _group(**kw):
    a = dict(n=3, frames="ok", ref=A, refRowBytes=12 * W, flowRowBytes=8 * W, meansRowBytes=12 * W, maskRowBytes=16 * W, w=W, h=H, means=A,
             raw=A, mask=A, flow=A)
    a.update(kw)
    fr = None
    if a["frames"] == "ok":
        fr = (capi.RobustnessGroupFrame * 4)(*[capi.RobustnessGroupFrame(a["means"] if k == 2 else A, a["raw"] if k == 2 else A,
                                                                          a["mask"] if k == 2 else A, a["flow"] if k == 2 else A)
                                               for k in range(4)])
    return capi.lib().raw["mfsr_robustnessMaskGroup"](a["n"], fr, a["ref"], a["refRowBytes"], a["flowRowBytes"], a["meansRowBytes"],
                                                      a["maskRowBytes"], a["w"], a["h"], 4095.0, 1e-4, 1e-6, 0.8, None)


def test_mask_group_checks_its_arguments_on_the_host():
    assert _group(frames=None) == INVALID and _group(ref=None) == INVALID
    assert _group(n=0) == INVALID and _group(n=5) == INVALID
    for field in ("means", "raw", "mask", "flow"):
        assert _group(**{field: None}) == INVALID, field
    assert _group(mask=A + 8) == INVALID                         # float4 stores
    assert _group(flow=A + 4) == INVALID                         # float2 loads
    assert _group(means=A + 2) == INVALID and _group(raw=A + 2) == INVALID and _group(ref=A + 2) == INVALID
    assert _group(refRowBytes=12 * W - 4) == INVALID and _group(meansRowBytes=12 * W - 4) == INVALID
    assert _group(maskRowBytes=16 * W - 16) == INVALID and _group(flowRowBytes=8 * W - 8) == INVALID
    assert _group(refRowBytes=12 * W + 2) == INVALID and _group(meansRowBytes=12 * W + 2) == INVALID
    assert _group(maskRowBytes=16 * W + 8) == INVALID and _group(flowRowBytes=8 * W + 4) == INVALID
    assert _group(w=2) == INVALID and _group(h=2) == INVALID


def test_switch_and_structs():
    L = capi.lib()
    try:
        assert L.set_robustness_group(0) == 0
        assert L.set_robustness_group(1) == 0
    finally:
        L.raw["mfsr_set_robustness_group"](1)
    assert L.raw["mfsr_burst_debug_robust_group"](None, None) == INVALID
    n = ctypes.c_int(5)
    assert L.raw["mfsr_burst_debug_robust_group"](None, ctypes.byref(n)) == INVALID and n.value == 5
    assert ctypes.sizeof(capi.RobustnessGroupFrame) == 4 * ctypes.sizeof(ctypes.c_void_p)
    protos = capi.parse_header()
    assert [a for _, a in protos["mfsr_robustnessMaskGroup"][1]] == ["nFrames", "frames", "refHalf", "refRowBytes", "flowRowBytes",
                                                                     "meansRowBytes", "maskRowBytes", "w", "h", "maxVal", "alpha", "beta",
                                                                     "thresholdM", "stream"]
    assert [a for _, a in protos["mfsr_prepareFrameMeansBatch"][1]] == ["nFrames", "frames", "meansRowBytes", "maxVal", "w", "h",
                                                                        "pyr0RowBytes", "pyr1RowBytes", "taps", "ntaps", "stream"]
