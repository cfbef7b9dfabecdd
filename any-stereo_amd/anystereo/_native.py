"""What the ctypes bindings share: opening a library of `_srchash.LIBRARIES`, describing it, and turning a failed call into an
exception.  `_scenes_lib`, `_augment_lib` and `_spatial_lib` load through it.  It serves the `hip` row as well
(tests/test_native_cpu.py), but `_lib.py` still carries the copy of these steps it always had: the full-size cfg-4 training test
keeps meeting a GPU fault of unknown cause in whole-suite runs ("One table, one recipe, one loader"), and until that
cause is known nothing that test executes is rewritten.

Only the slow path lives here.  A binding keeps its own cached `load()` and its own `check()`: `ops.py` issues about 1500
`L.check(L.load().fn(...))` per training step, so on success those two touch one module global and one integer and never reach
this module.  There is no fallback anywhere: a missing file, a missing symbol or a library built from other sources raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _srchash

_LABEL = {"hip": "HIP"}   # "anystereo HIP call ...", "anystereo scenes call ..."


def lib_path(key: str) -> str:
    """The in-tree build of the library, or the file its override variable names (A/B timing of kernel variants)."""
    row = _srchash.LIBRARIES[key]
    return os.environ.get(row.override) or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", row.file)


def _compiled_hash(key: str, lib: C.CDLL) -> str:
    return getattr(lib, _srchash.LIBRARIES[key].prefix + "_source_hash")().decode()


def open_library(key: str, signatures: dict, path: str | None = None) -> C.CDLL:
    """Load the file and bind every name of `signatures` (name -> (restype, argtypes)); refuse a library whose compiled-in source
    hash is not the tree's."""
    row = _srchash.LIBRARIES[key]
    path = lib_path(key) if path is None else path
    if not os.path.exists(path):
        raise RuntimeError(f"{row.file} not found at {path}: build it with `python any-stereo_amd/build.py` (or __graft_entry__.build())."
                           + (" There is no CPU fallback for the hot path." if key == "hip" else ""))
    lib = C.CDLL(path)
    for name, (res, args) in signatures.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    want, have = _srchash.source_hash(key), _compiled_hash(key, lib)
    if want is not None and want != have and os.environ.get("ANYSTEREO_ALLOW_STALE_LIB", "0") != "1":
        raise RuntimeError(f"{path} was built from other sources (library {have}, tree {want}): run `python any-stereo_amd/build.py` "
                           "(ANYSTEREO_ALLOW_STALE_LIB=1 overrides)")
    return lib


def library_info(key: str, lib: C.CDLL) -> dict:
    """What is loaded: path, ABI version, the source hash compiled into it and whether it matches the tree."""
    have, want = _compiled_hash(key, lib), _srchash.source_hash(key)
    return {"path": os.path.relpath(lib._name), "abi": int(getattr(lib, _srchash.LIBRARIES[key].prefix + "_abi_version")()), "src_hash": have,
            "matches_sources": None if want is None else have == want}


def raise_for(key: str, rc: int, what: str, lib: C.CDLL):
    """The body of a binding's check(): the library's own message for the code it returned."""
    msg = getattr(lib, _srchash.LIBRARIES[key].prefix + "_last_error_string")().decode("utf-8", "replace")
    raise RuntimeError(f"anystereo {_LABEL.get(key, key)} call {what} failed (code {rc}): {msg}")
