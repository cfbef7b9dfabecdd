"""ctypes binding of libanystereo_spatial.so (C ABI: include/anystereo_spatial.h): the spatial augmentation's library.

Loaded like `_lib.py`, by `_native.open_library`: every declared symbol is bound at load, a library built from other sources is
refused, and there is no fallback — `harness.spatial` calls the host restatement for CPU tensors because they are CPU tensors,
never because a kernel is missing.
"""
from __future__ import annotations

import ctypes as C

import torch  # noqa: F401  (pins the HIP runtime this library binds to, as in _lib.py)

from . import _native

SPT_MAX_BATCH = 8
SPT_MIN_SCALE, SPT_MAX_SCALE = 0.125, 8.0
SPT_OK, SPT_ERR_BAD_ARG, SPT_ERR_BAD_SHAPE, SPT_ERR_LAUNCH, SPT_ERR_CROP, SPT_ERR_ALIAS = 0, -1, -2, -3, -4, -5
SPT_U8, SPT_F32 = 0, 1
SPT_FLIP_NONE, SPT_FLIP_HF, SPT_FLIP_H, SPT_FLIP_V = 0, 1, 2, 3

LIB_PATH = _native.lib_path("spatial")

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
    if _lib is None:
        _lib = _native.open_library("spatial", SIGNATURES, LIB_PATH)
    return _lib


def library_info() -> dict:
    return _native.library_info("spatial", load())


def check(rc: int, what: str) -> None:
    if rc != 0:
        _native.raise_for("spatial", rc, what, load())
