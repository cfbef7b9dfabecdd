"""Content hash of the native sources (csrc/*.hip, csrc/*.h, include/anystereo_hip.h).  build.py compiles it into the library
(`as_source_hash()`), `_lib.load()` recomputes it from the tree and refuses a library built from other sources: the built `.so`
is git-ignored but travels with the repo snapshot, so a stale binary would otherwise run silently on the GPU box."""
import hashlib
import os

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "..", "csrc")
HEADER = os.path.join(PKG, "..", "..", "include", "anystereo_hip.h")


def source_hash() -> str | None:
    """None when the sources are not there (an installed library without its tree)."""
    if not (os.path.isdir(CSRC) and os.path.exists(HEADER)):
        return None
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(open(HEADER, "rb").read())
    return h.hexdigest()[:16]


SCENES_CSRC = os.path.join(CSRC, "scenes")
SCENES_HEADER = os.path.join(PKG, "..", "..", "include", "anystereo_scenes.h")


def scenes_source_hash() -> str | None:
    """The same for libanystereo_scenes.so: csrc/scenes/* and include/anystereo_scenes.h (`scn_source_hash()`).  `source_hash()` above
    lists the top level of csrc/ only, so the scene sources are no part of the main library's hash."""
    if not (os.path.isdir(SCENES_CSRC) and os.path.exists(SCENES_HEADER)):
        return None
    h = hashlib.sha256()
    for f in sorted(os.listdir(SCENES_CSRC)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(SCENES_CSRC, f), "rb").read())
    h.update(open(SCENES_HEADER, "rb").read())
    return h.hexdigest()[:16]


AUGMENT_CSRC = os.path.join(CSRC, "augment")
AUGMENT_HEADER = os.path.join(PKG, "..", "..", "include", "anystereo_augment.h")


def augment_source_hash() -> str | None:
    """The same for libanystereo_augment.so: csrc/augment/* and include/anystereo_augment.h only (`aug_source_hash()`)."""
    if not (os.path.isdir(AUGMENT_CSRC) and os.path.exists(AUGMENT_HEADER)):
        return None
    h = hashlib.sha256()
    for f in sorted(os.listdir(AUGMENT_CSRC)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(AUGMENT_CSRC, f), "rb").read())
    h.update(open(AUGMENT_HEADER, "rb").read())
    return h.hexdigest()[:16]


SPATIAL_CSRC = os.path.join(CSRC, "spatial")
SPATIAL_HEADER = os.path.join(PKG, "..", "..", "include", "anystereo_spatial.h")
SPATIAL_SHARED = (os.path.join(CSRC, "cubic.h"),)   # top-level headers csrc/spatial/ includes: the final resize's arithmetic


def spatial_source_hash() -> str | None:
    """The same for libanystereo_spatial.so: csrc/spatial/*, include/anystereo_spatial.h and the one header it shares with the main
    library, csrc/cubic.h (`spt_source_hash()`)."""
    if not (os.path.isdir(SPATIAL_CSRC) and os.path.exists(SPATIAL_HEADER) and all(os.path.exists(f) for f in SPATIAL_SHARED)):
        return None
    h = hashlib.sha256()
    for f in sorted(os.listdir(SPATIAL_CSRC)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(SPATIAL_CSRC, f), "rb").read())
    for f in SPATIAL_SHARED:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    h.update(open(SPATIAL_HEADER, "rb").read())
    return h.hexdigest()[:16]
