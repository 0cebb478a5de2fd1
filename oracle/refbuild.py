"""Builds oracle/_ref/libmfsr_ref.so: the reference's own kernels compiled for the host.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  The reference's sources are not part of
this repository; the recipe (oracle/Makefile, target ``ref``, and oracle/refshim/) is.  The
directory that holds the reference's five ``.cu`` files is taken from the environment variable
``MFSR_REFERENCE_DIR`` or, failing that, from a checkout named ``reference`` next to (or
above) this repository or in the home directory.
"""
from __future__ import annotations

import os
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
REF_LIB_PATH = os.path.join(_DIR, "_ref", "libmfsr_ref.so")
REF_FILES = ("kernel.cu", "DeBayerKernels.cu", "opticalFlow.cu", "RobustnessModell.cu", "ShiftMinimizerKernels.cu")


def _has_sources(d: str) -> bool:
    return all(os.path.isfile(os.path.join(d, f)) for f in REF_FILES)


def find_reference_dir() -> str | None:
    """The directory with the reference's kernels, or None when there is none on this machine."""
    cands = []
    env = os.environ.get("MFSR_REFERENCE_DIR")
    if env:
        cands += [env, os.path.join(env, "test_opencv")]
    d = os.path.dirname(_DIR)
    while True:
        up = os.path.dirname(d)
        if up == d:
            break
        d = up
        cands.append(os.path.join(d, "reference", "test_opencv"))
    cands.append(os.path.join(os.path.expanduser("~"), "reference", "test_opencv"))
    for c in cands:
        try:
            if _has_sources(c):
                return os.path.abspath(c)
        except OSError:
            pass
    return None


def ref_lib_path() -> str:
    """The library the tests load: MFSR_REF_LIB (e.g. the sanitizer build) or oracle/_ref/libmfsr_ref.so."""
    return os.environ.get("MFSR_REF_LIB") or REF_LIB_PATH


def build_ref(target: str = "ref") -> str | None:
    """make -C oracle <target>.  Returns the library's path, or None when the reference is absent."""
    ref = find_reference_dir()
    if ref is None:
        return None
    subprocess.check_call(["make", "-s", "-C", _DIR, target, "REFERENCE_DIR=" + ref])
    return REF_LIB_PATH if target == "ref" else os.path.join(_DIR, "_ref", "libmfsr_ref_asan.so")
