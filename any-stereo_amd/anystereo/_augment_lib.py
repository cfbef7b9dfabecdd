"""ctypes binding of libanystereo_augment.so (C ABI: include/anystereo_augment.h): the photometric augmentation's library.

Loaded like `_lib.py`, by `_native.open_library`: every declared symbol is bound at load, a library built from other sources is
refused, and there is no fallback — `harness.augment` calls the host restatement for CPU tensors because they are CPU tensors,
never because a kernel is missing.
"""
from __future__ import annotations

import ctypes as C

import torch  # noqa: F401  (pins the HIP runtime this library binds to, as in _lib.py)

from . import _native

AUG_MAX_BATCH = 8
AUG_MAX_RECTS = 2
AUG_TILE = 2048
AUG_MAX_PARTS = 1024
AUG_OK, AUG_ERR_BAD_ARG, AUG_ERR_BAD_SHAPE, AUG_ERR_LAUNCH, AUG_ERR_WORKSPACE, AUG_ERR_ALIAS = 0, -1, -2, -3, -4, -5
AUG_U8, AUG_F32 = 0, 1

LIB_PATH = _native.lib_path("augment")

_vp, _i = C.c_void_p, C.c_int


class ImageParams(C.Structure):
    """aug_image_params (include/anystereo_augment.h)."""
    _fields_ = [("order", C.c_int * 4), ("factor", C.c_float * 3), ("hue_shift", C.c_int)]


class Sample(C.Structure):
    """aug_sample (include/anystereo_augment.h)."""
    _fields_ = [("img", ImageParams * 2), ("shared", C.c_int), ("n_rects", C.c_int), ("rect", (C.c_int * 4) * AUG_MAX_RECTS)]


# name -> (restype, argtypes); every symbol include/anystereo_augment.h declares
SIGNATURES = {
    "aug_abi_version": (_i, []),
    "aug_last_error_string": (C.c_char_p, []),
    "aug_source_hash": (C.c_char_p, []),
    "aug_workspace_bytes": (C.c_int64, [_i, _i, _i]),
    "aug_photometric_pair": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, C.POINTER(Sample), _vp, _vp, C.c_int64, _vp]),
}
# the entries that launch kernels (tests/test_augment_gpu.py runs each of them under a guarded allocator)
LAUNCHING = ("aug_photometric_pair",)

_lib = None


def load() -> C.CDLL:
    """Load the library (once) and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is None:
        _lib = _native.open_library("augment", SIGNATURES, LIB_PATH)
    return _lib


def library_info() -> dict:
    return _native.library_info("augment", load())


def check(rc: int, what: str) -> None:
    if rc != 0:
        _native.raise_for("augment", rc, what, load())
