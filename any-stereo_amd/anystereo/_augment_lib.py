"""ctypes binding of libanystereo_augment.so (C ABI: include/anystereo_augment.h): the photometric augmentation's library.

Modelled on `_scenes_lib.py`: every declared symbol is bound at load, a library built from other sources is refused, and there is
no fallback — `harness.augment` calls the host restatement for CPU tensors because they are CPU tensors, never because a kernel
is missing.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (pins the HIP runtime this library binds to, as in _lib.py)

AUG_MAX_BATCH = 8
AUG_MAX_RECTS = 2
AUG_TILE = 2048
AUG_MAX_PARTS = 1024
AUG_OK, AUG_ERR_BAD_ARG, AUG_ERR_BAD_SHAPE, AUG_ERR_LAUNCH, AUG_ERR_WORKSPACE, AUG_ERR_ALIAS = 0, -1, -2, -3, -4, -5
AUG_U8, AUG_F32 = 0, 1

LIB_PATH = os.environ.get("ANYSTEREO_AUGMENT_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libanystereo_augment.so")

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
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"libanystereo_augment.so not found at {LIB_PATH}: build it with `python any-stereo_amd/build.py` "
                           "(or __graft_entry__.build()).")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    from ._srchash import augment_source_hash
    want, have = augment_source_hash(), lib.aug_source_hash().decode()
    if want is not None and want != have and os.environ.get("ANYSTEREO_ALLOW_STALE_LIB", "0") != "1":
        raise RuntimeError(f"{LIB_PATH} was built from other sources (library {have}, tree {want}): run `python any-stereo_amd/build.py` "
                           "(ANYSTEREO_ALLOW_STALE_LIB=1 overrides)")
    _lib = lib
    return lib


def library_info() -> dict:
    from ._srchash import augment_source_hash
    lib = load()
    have, want = lib.aug_source_hash().decode(), augment_source_hash()
    return {"path": os.path.relpath(LIB_PATH), "abi": int(lib.aug_abi_version()), "src_hash": have,
            "matches_sources": None if want is None else have == want}


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().aug_last_error_string().decode("utf-8", "replace")
        raise RuntimeError(f"anystereo augment call {what} failed (code {rc}): {msg}")
