"""ctypes loader for libaptai_hip.so (the C ABI in include/aptai_hip.h).

There is NO CPU fallback: every product op goes through this library and raises if it is missing
or if the call fails.  The library is built in-tree by ``__graft_entry__.build()`` /
``make -C aptai_amd/csrc`` (hipcc cross-compiles gfx950 without a GPU).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

import torch  # noqa: F401  -- MUST precede the CDLL below: torch's bundled HIP runtime has to be the one this process
#                              initialises; loading libaptai_hip.so first pulls in a second runtime that sees no device

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# APTAI_HIP_LIB: A/B a second in-tree build of the same sources (tools/, never a different implementation)
LIB_PATH = os.environ.get("APTAI_HIP_LIB") or os.path.join(CSRC, "libaptai_hip.so")

_lib = None
_lock = threading.Lock()

_P, _I64, _I, _F, _U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64
# argument and return types of every entry point, as include/aptai_hip.h declares them (_abi reads the header once per process)
ABI = _abi.header()
ARGTYPES = {name: args for name, (_, args) in ABI.prototypes.items()}


class AptaiHipError(RuntimeError):
    pass


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile every HIP source for gfx950 and link libaptai_hip.so in-tree."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC, f"-j{jobs}"], check=True)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise AptaiHipError(
                        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"or `make -C {CSRC}` — aptai_amd has no CPU fallback")
                L = ctypes.CDLL(LIB_PATH)
                for name, (restype, _) in ABI.prototypes.items():
                    fn = getattr(L, name)
                    fn.restype, fn.argtypes = restype, ARGTYPES[name]
                _lib = L
    return _lib


def call(name: str, *args) -> None:
    """Call an int-returning entry point with its declared argtypes and raise on a non-zero status."""
    check(getattr(lib(), name)(*args), name)


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().aptai_last_error().decode(errors="replace")
        raise AptaiHipError(f"{what or 'aptai_hip call'} failed (status {rc}): {msg}")


def declared_symbols() -> list:
    """Every function name declared in include/aptai_hip.h (used by the CPU export test)."""
    return sorted(ABI.prototypes)
