"""ctypes binding of libanystereo_spatial.so (C ABI: include/anystereo_spatial.h): the spatial augmentation's library.

Modelled on `_augment_lib.py`: every declared symbol is bound at load, a library built from other sources is refused, and there is
no fallback — `harness.spatial` calls the host restatement for CPU tensors because they are CPU tensors, never because a kernel
is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (pins the HIP runtime this library binds to, as in _lib.py)

SPT_MAX_BATCH = 8
SPT_MIN_SCALE, SPT_MAX_SCALE = 0.125, 8.0
SPT_OK, SPT_ERR_BAD_ARG, SPT_ERR_BAD_SHAPE, SPT_ERR_LAUNCH, SPT_ERR_CROP, SPT_ERR_ALIAS = 0, -1, -2, -3, -4, -5
SPT_U8, SPT_F32 = 0, 1
SPT_FLIP_NONE, SPT_FLIP_HF, SPT_FLIP_H, SPT_FLIP_V = 0, 1, 2, 3

LIB_PATH = os.environ.get("ANYSTEREO_SPATIAL_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libanystereo_spatial.so")

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double


class Sample(C.Structure):
    """spt_sample (include/anystereo_spatial.h)."""
    _fields_ = [("scale_x", _d), ("scale_y", _d), ("rescale", _i), ("flip", _i), ("y0", _i), ("x0", _i), ("ch", _i), ("cw", _i), ("dy2", _i),
                ("reserved", _i)]


# name -> (restype, argtypes); every symbol include/anystereo_spatial.h declares
SIGNATURES = {
    "spt_abi_version": (_i, []),
    "spt_last_error_string": (C.c_char_p, []),
    "spt_source_hash": (C.c_char_p, []),
    "spt_frame_size": (_i, [_i, _i, _i, _d, _d, C.POINTER(_i), C.POINTER(_i)]),
    "spt_validate": (_i, [C.POINTER(Sample), _i, _i, _i, _i, _i]),
    "spt_spatial_pair": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, C.POINTER(Sample), _vp, _vp, _i, _i, _i, C.POINTER(_vp), C.POINTER(_vp), _vp]),
}
# the entries that launch kernels (tests/test_spatial_gpu.py runs each of them under a guarded allocator)
LAUNCHING = ("spt_spatial_pair",)

_lib = None


def load() -> C.CDLL:
    """Load the library (once) and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libanystereo_spatial.so not found at {LIB_PATH}: build it with `python any-stereo_amd/build.py` "
                           "(or __graft_entry__.build()).")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    from ._srchash import spatial_source_hash
    want, have = spatial_source_hash(), lib.spt_source_hash().decode()
    if want is not None and want != have and os.environ.get("ANYSTEREO_ALLOW_STALE_LIB", "0") != "1":
        raise RuntimeError(f"{LIB_PATH} was built from other sources (library {have}, tree {want}): run `python any-stereo_amd/build.py` "
                           "(ANYSTEREO_ALLOW_STALE_LIB=1 overrides)")
    _lib = lib
    return lib


def library_info() -> dict:
    from ._srchash import spatial_source_hash
    lib = load()
    have, want = lib.spt_source_hash().decode(), spatial_source_hash()
    return {"path": os.path.relpath(LIB_PATH), "abi": int(lib.spt_abi_version()), "src_hash": have,
            "matches_sources": None if want is None else have == want}


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().spt_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(f"anystereo spatial call {what} failed (code {rc}): {msg}")
