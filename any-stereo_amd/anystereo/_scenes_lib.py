"""ctypes binding of libanystereo_scenes.so (C ABI: include/anystereo_scenes.h): the procedural scenes' library.

Loaded like `_lib.py`, by `_native.open_library`: every declared symbol is bound at load, a library built from other sources is
refused, and there is no fallback — `harness.scenes` calls the host restatements for CPU tensors because they are CPU tensors,
never because a kernel is missing.
"""
from __future__ import annotations

import ctypes as C

import torch  # noqa: F401  (pins the HIP runtime this library binds to, as in _lib.py)

from . import _native

SCN_MAX_LAYERS = 8
SCN_MAX_OCTAVES = 6
SCN_MAX_BATCH = 8
SCN_LAYER_FLOATS = 16
SCN_OK, SCN_ERR_BAD_ARG, SCN_ERR_BAD_SHAPE, SCN_ERR_LAUNCH = 0, -1, -2, -3
KIND_PLANE, KIND_ELLIPSE, KIND_PARALLELOGRAM = 0, 1, 2

LIB_PATH = _native.lib_path("scenes")

_vp, _i = C.c_void_p, C.c_int


class Spec(C.Structure):
    """scn_spec (include/anystereo_scenes.h)."""
    _fields_ = [("n_layers", C.c_int), ("octaves", C.c_int)] + [(n, C.c_float) for n in (
        "aspect", "bg_min", "bg_max", "bg_slope", "d_min", "d_max", "slope_max", "size_min", "size_max", "shear_max", "lattice", "contrast",
        "noise")]


class GtSample(C.Structure):
    """scn_gt_sample (include/anystereo_scenes.h)."""
    _fields_ = [("disp", C.c_void_p), ("disp_right", C.c_void_p), ("noc", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("index", C.c_int)]


# name -> (restype, argtypes); every symbol include/anystereo_scenes.h declares
SIGNATURES = {
    "scn_abi_version": (_i, []),
    "scn_last_error_string": (C.c_char_p, []),
    "scn_source_hash": (C.c_char_p, []),
    "scn_layers": (_i, [C.POINTER(Spec), C.c_uint64, _i, C.POINTER(C.c_float)]),
    "scn_render_pair": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(Spec), C.c_uint64, _i, _vp]),
    "scn_ground_truth": (_i, [C.POINTER(GtSample), _i, C.POINTER(Spec), C.c_uint64, _vp]),
    "scn_disparity_at": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(C.c_float), C.POINTER(C.c_int), _i, C.POINTER(Spec), C.c_uint64, _vp]),
}
# the entries that launch kernels (tests/test_scenes_gpu.py runs each of them under a guarded allocator)
LAUNCHING = ("scn_render_pair", "scn_ground_truth", "scn_disparity_at")

_lib = None


def load() -> C.CDLL:
    """Load the library (once) and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is None:
        _lib = _native.open_library("scenes", SIGNATURES, LIB_PATH)
    return _lib


def library_info() -> dict:
    return _native.library_info("scenes", load())


def check(rc: int, what: str) -> None:
    if rc != 0:
        _native.raise_for("scenes", rc, what, load())
