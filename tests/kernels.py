"""Uniform numpy-level access to the CPU oracle and to the HIP C-ABI.

Both runners expose ``call(name, *args)`` with the SAME argument list (the
reference kernel's argument order); numpy arrays are device buffers that the
kernel may update in place.  Marker classes cover the places where the two
C signatures differ only in spelling:

    F3(v)          float3 by value (HIP)        / const float[3] (oracle)
    F2(v)          float2 by value (HIP)        / two floats (oracle)
    Tex(a, w, h)   mfsr_tex2d by value (HIP)    / ptr, pitch, w, h (oracle); address="clamp" | "mirror" is
                   read by RefKernels only (the other two fix the mode per kernel)
    Host(a)        host array on both sides (e.g. filter taps)

``OracleKernels`` is test infrastructure; ``HipKernels`` is the product path
(torch is used only to own device memory).  ``RefKernels`` runs the reference's
own kernels, compiled for the host (oracle/_ref/libmfsr_ref.so, oracle/refshim/):
what the reference leaves open -- block shape, texture address mode and filter
variant -- are its parameters, with this project's decisions as defaults.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np


class F3:
    def __init__(self, v):
        self.v = np.asarray(v, np.float32).copy()


class F2:
    def __init__(self, v):
        self.v = np.asarray(v, np.float32).copy()


class Tex:
    def __init__(self, arr, width=None, height=None, pitch=None, address=None):
        self.arr = arr
        self.address = address
        self.height = arr.shape[0] if height is None else height
        self.width = arr.shape[1] if width is None else width
        self.pitch = arr.strides[0] if pitch is None else pitch


class Host:
    def __init__(self, arr):
        self.arr = np.ascontiguousarray(arr)


def pitch_of(a: np.ndarray) -> int:
    return int(a.strides[0])


class OracleKernels:
    name = "oracle"

    def __init__(self):
        from oracle.bindings import oracle

        self.o = oracle()

    def call(self, fname, *args):
        conv = []
        keep = []
        for a in args:
            if isinstance(a, F3):
                keep.append(a.v)
                conv.append(a.v)
            elif isinstance(a, F2):
                conv.extend([float(a.v[0]), float(a.v[1])])
            elif isinstance(a, Tex):
                conv.extend([a.arr, int(a.pitch), int(a.width), int(a.height)])
            elif isinstance(a, Host):
                conv.append(a.arr)
            elif a is None:
                conv.append(None)
            else:
                conv.append(a)
        return getattr(self.o, fname)(*conv)

    def set_cfa(self, pattern):
        self.o.set_cfa_pattern(np.asarray(pattern, np.int32))


# ---- guarded device buffers ---------------------------------------------------------------------------------------
# Every array a test hands to the HIP library lives in a larger device byte buffer [guard | data | guard] (tests/guards.py).
# The guards hold 0xFF: NaN as float, 0xFFFF as uint16_t, -1 as int, so a read outside the array poisons what it feeds, and
# a write outside it is found when the guards are read back.  The data offset is a multiple of 256 (what the entry points
# may require of a pointer); the trailing guard starts at the first byte after the data.
DEVICE_GUARD = 4096
DEVICE_ALIGN = 256
DEVICE_FILL = 0xFF


def guarded_upload(arr: np.ndarray, dev="cuda:0"):
    """-> (tensor_view, check): ``arr`` on the device between two guards, as a tensor of its shape and type (uint16 as
    int16).  ``check(what, unchanged=False)`` downloads the buffer once and asserts that both guards are intact (naming
    which one and the first changed byte) and, with ``unchanged``, that the data still equals what was uploaded."""
    import torch

    from tests.guards import check_bands, layout

    a = np.ascontiguousarray(arr)
    raw = a.reshape(-1).view(np.uint8)
    off, total = layout(a.nbytes, DEVICE_GUARD, DEVICE_ALIGN)
    big = np.full(total, DEVICE_FILL, np.uint8)
    big[off:off + a.nbytes] = raw
    d_big = torch.from_numpy(big).to(dev)
    assert d_big.data_ptr() % DEVICE_ALIGN == 0
    tdt = a.dtype if a.dtype != np.uint16 else np.dtype(np.int16)
    view = d_big[off:off + a.nbytes].view(torch.from_numpy(np.zeros(1, tdt)).dtype).reshape(a.shape)
    sent = raw.copy()

    def check(what, unchanged=False):
        h = d_big.cpu().numpy()
        check_bands(h, off, a.nbytes, DEVICE_FILL, what)
        if unchanged:
            bad = np.flatnonzero(h[off:off + a.nbytes] != sent)
            assert bad.size == 0, f"{what}: a read-only input was changed, first at byte {int(bad[0])}"

    return view, check


class HipKernels:
    name = "hip"

    def __init__(self):
        import torch

        from multi_frame_super_resolution_amd import capi

        self.torch = torch
        self.capi = capi
        self.L = capi.lib()
        self.dev = torch.device("cuda:0")

    def set_cfa(self, pattern):
        arr = (ctypes.c_int32 * 4)(*[int(p) for p in pattern])
        self.L.set_cfa_pattern(arr)

    def call(self, fname, *args):
        torch = self.torch
        uploaded = {}

        def up(a: np.ndarray, index: int):
            key = id(a)
            if key not in uploaded:
                assert a.flags["C_CONTIGUOUS"]
                t, check = guarded_upload(a, self.dev)
                uploaded[key] = (a, t, check, index)
            return uploaded[key][1]

        conv = []
        for i, a in enumerate(args):
            if isinstance(a, F3):
                conv.append(self.capi.f3(a.v))
            elif isinstance(a, F2):
                conv.append(self.capi.f2(a.v))
            elif isinstance(a, Tex):
                t = up(a.arr, i)
                conv.append(self.capi.Tex2D(t.data_ptr(), int(a.pitch), int(a.width), int(a.height)))
            elif isinstance(a, Host):
                conv.append(a.arr.ctypes.data)
            elif isinstance(a, np.ndarray):
                conv.append(up(a, i).data_ptr())
            elif a is None:
                conv.append(None)
            else:
                conv.append(a)
        conv.append(None)  # stream: default
        rc = getattr(self.L, fname)(*conv)
        torch.cuda.synchronize()
        for a, t, check, index in uploaded.values():
            check(f"mfsr_{fname}, argument {index}", unchanged=not a.flags["WRITEABLE"])
        for a, t, check, index in uploaded.values():
            if a.flags["WRITEABLE"]:
                h = t.cpu().numpy()
                if a.dtype == np.uint16:
                    h = h.view(np.uint16)
                np.copyto(a, h)
        return rc


# ---- the reference's kernels on the host ------------------------------------------------------------------------
CLAMP, MIRROR = 0, 1
# texture address modes per kernel, textures in argument order: this project's decisions
REF_TEX_ADDRESS = {
    "accumulateImagesSuperRes": (CLAMP, CLAMP),
    "WarpingKernel": (CLAMP, MIRROR),
    "CreateFlowFieldFromTiles": (CLAMP,),
    "ComputeDerivativesKernel": (MIRROR, MIRROR),
    "ComputeDerivatives2Kernel": (MIRROR,),
    "ComputeRobustnessMask": (CLAMP,),
}
_REF_1D = {"squaredSum", "findMinimum", "conjugateComplexMulKernel", "copyShiftMatrix", "setPointers", "checkForOutliers"}
_REF_TILE3D = {"normalizedCC", "convertToTilesOverlapBorder", "convertToTilesOverlapPreShift"}
REF_ERRORS = {1: "__syncthreads() in a kernel run as a loop", 2: "dynamic shared memory request too large",
              4: "write past the block's dynamic shared memory", 8: "bad block shape"}


class RefMissing(RuntimeError):
    pass


class RefKernels:
    """``call(name, *args, block=(bx, by, bz), filter="exact" | "fixed8")``: the same argument list as
    ``OracleKernels.call``.  ``flat(name, *args)`` takes the oracle's C argument list (what ``oracle.bindings``
    passes), so that an object of this class can stand in for the oracle inside ``oracle.pipeline``."""
    name = "reference"

    def __init__(self, path=None):
        from oracle.bindings import _SCALAR, _parse
        from oracle.refbuild import ref_lib_path

        self.path = path or ref_lib_path()
        if not os.path.exists(self.path):
            raise RefMissing(self.path)
        self.cdll = ctypes.CDLL(self.path)
        self.fns = {}
        for oname, (_, args) in _parse().items():
            name = oname[len("orc_"):]
            try:
                fn = getattr(self.cdll, "ref_" + name)
            except AttributeError:
                continue
            at = [ctypes.c_void_p if "*" in t else _SCALAR[t.replace("const", "").strip()] for t, _ in args]
            if name != "set_cfa_pattern":
                at += [ctypes.c_int] * (4 if name in REF_TEX_ADDRESS else 3)
            fn.argtypes = at
            fn.restype = ctypes.c_int
            self.fns[name] = (fn, [n for _, n in args])

    def has(self, name):
        return name in self.fns

    def default_block(self, name, flat):
        names = self.fns[name][1]
        if name in ("boxFilterWithBorderX", "boxFilterWithBorderY"):
            side = flat[names.index("tileSize")] + 2 * flat[names.index("maxShift")]
            return (side, 1, 1) if name.endswith("X") else (1, side, 1)   # the kernels' own constraint
        if name in _REF_1D:
            return (64, 1, 1)
        if name in _REF_TILE3D:
            return (8, 8, 2)
        if name in ("concatenateShifts", "separateShifts"):
            return (4, 4, 4)
        return (16, 16, 1)

    def flat(self, name, *flat, block=None, address=None, filter="exact"):
        fn, _ = self.fns[name]
        conv = []
        for v in flat:
            if isinstance(v, np.ndarray):
                assert v.flags["C_CONTIGUOUS"], "reference arrays must be C-contiguous"
                conv.append(v.ctypes.data)
            else:
                conv.append(v)
        if name == "set_cfa_pattern":
            return fn(*conv)
        conv += list(block or self.default_block(name, flat))
        if name in REF_TEX_ADDRESS:
            modes = list(REF_TEX_ADDRESS[name])
            for i, a in enumerate(address or ()):
                if a is not None:
                    modes[i] = {"clamp": CLAMP, "mirror": MIRROR}.get(a, a)
            fbit = {"exact": 0, "fixed8": 1}[filter]
            conv.append(sum((m | (fbit << 1)) << (4 * i) for i, m in enumerate(modes)))
        rc = fn(*conv)
        assert rc == 0, f"reference shim, {name}: " + ", ".join(v for k, v in REF_ERRORS.items() if rc & k)
        return rc

    def call(self, fname, *args, block=None, filter="exact"):
        conv, address = [], []
        for a in args:
            if isinstance(a, F3):
                conv.append(a.v)
            elif isinstance(a, F2):
                conv.extend([float(a.v[0]), float(a.v[1])])
            elif isinstance(a, Tex):
                conv.extend([a.arr, int(a.pitch), int(a.width), int(a.height)])
                address.append(a.address)
            elif isinstance(a, Host):
                conv.append(a.arr)
            else:
                conv.append(a)
        return self.flat(fname, *conv, block=block, address=address, filter=filter)

    def set_cfa(self, pattern):
        self.flat("set_cfa_pattern", np.asarray(pattern, np.int32))


def load_ref_or_skip():
    """What the ``ref`` fixture of the reference-pin test modules returns: the library; a failure when it is missing although
    the reference's sources are on this machine (build() should have made it); a skip when neither is here."""
    import pytest

    from oracle.refbuild import find_reference_dir
    try:
        return RefKernels()
    except RefMissing as e:
        if find_reference_dir() is not None:
            pytest.fail(f"{e} is missing although the reference's sources are on this machine: run __graft_entry__.build()")
        pytest.skip("neither oracle/_ref/libmfsr_ref.so nor the reference's sources are on this machine")


class RefBackedOracle:
    """Stands in for ``oracle.bindings.oracle()``: every function the reference library has is answered by the
    reference's kernel, everything else (glue stages, solver, pre-alignment) by the oracle."""

    def __init__(self, ref, oracle_obj):
        self._ref, self._orc = ref, oracle_obj
        self.answered = set()

    def __getattr__(self, name):
        ref, orc = self.__dict__["_ref"], self.__dict__["_orc"]
        if name == "set_cfa_pattern":
            def both(p):
                ref.flat("set_cfa_pattern", p)
                return orc.set_cfa_pattern(p)
            return both
        if ref.has(name):
            self.__dict__["answered"].add(name)
            return lambda *a: ref.flat(name, *a)
        return getattr(orc, name)
