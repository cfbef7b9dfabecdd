"""Build libanystereo_hip.so, libanystereo_scenes.so, libanystereo_augment.so and libanystereo_spatial.so (gfx950 only) in-tree with hipcc.

    python any-stereo_amd/build.py [--force]

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so is
git-ignored but travels to the GPU box with the repo snapshot.
"""
from __future__ import annotations

import concurrent.futures as cf
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIBDIR = os.path.join(HERE, "anystereo", "lib")
LIB = os.path.join(LIBDIR, "libanystereo_hip.so")
HEADER = os.path.join(HERE, "..", "include", "anystereo_hip.h")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function",
         "-Wno-pass-failed"]


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def _newer(src_list, target) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in src_list)


def _srchash():
    import importlib.util
    spec = importlib.util.spec_from_file_location("anystereo_srchash", os.path.join(HERE, "anystereo", "_srchash.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _source_hash() -> str:
    return _srchash().source_hash()


# libanystereo_scenes.so (include/anystereo_scenes.h): the procedural scenes' library, a build of its own — csrc/scenes/ is no part of
# libanystereo_hip.so, its source hash or its ABI
SCENES_CSRC = os.path.join(CSRC, "scenes")
SCENES_OBJ = os.path.join(OBJ, "scenes")
SCENES_LIB = os.path.join(LIBDIR, "libanystereo_scenes.so")
SCENES_HEADER = os.path.join(HERE, "..", "include", "anystereo_scenes.h")


def build_scenes(force: bool = False, verbose: bool = True) -> str:
    """The same recipe as the main library: the same flags, objects under build/scenes/, the source hash compiled in
    (`scn_source_hash`; `_scenes_lib.load()` refuses a stale binary)."""
    os.makedirs(SCENES_OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = sorted(f for f in os.listdir(SCENES_CSRC) if f.endswith(".hip"))
    stamp_src = os.path.join(SCENES_OBJ, "stamp.cpp")
    stamp = 'extern "C" const char* scn_source_hash(void) { return "%s"; }\n' % _srchash().scenes_source_hash()
    if not os.path.exists(stamp_src) or open(stamp_src).read() != stamp:
        open(stamp_src, "w").write(stamp)
    deps = [os.path.join(SCENES_CSRC, f) for f in sorted(os.listdir(SCENES_CSRC)) if f.endswith(".h")] + [SCENES_HEADER]
    hipcc = _hipcc()
    objs, compiled = [], False
    for s in srcs:
        src, obj = os.path.join(SCENES_CSRC, s), os.path.join(SCENES_OBJ, s[:-4] + ".o")
        objs.append(obj)
        if force or _newer([src] + deps, obj):
            r = subprocess.run([hipcc] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
            if verbose and (r.stderr.strip() or r.returncode):
                sys.stderr.write(r.stderr)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}")
            compiled = True
            if verbose:
                print(f"[build] compiled scenes/{s}")
    if force or compiled or _newer(objs + [stamp_src], SCENES_LIB):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SCENES_LIB] + objs + [stamp_src], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise RuntimeError("link failed")
        if verbose:
            print(f"[build] linked {SCENES_LIB}")
    return SCENES_LIB


# libanystereo_augment.so (include/anystereo_augment.h): the photometric augmentation's library, a build of its own like the scenes'
AUGMENT_CSRC = os.path.join(CSRC, "augment")
AUGMENT_OBJ = os.path.join(OBJ, "augment")
AUGMENT_LIB = os.path.join(LIBDIR, "libanystereo_augment.so")
AUGMENT_HEADER = os.path.join(HERE, "..", "include", "anystereo_augment.h")


def build_augment(force: bool = False, verbose: bool = True) -> str:
    """The recipe of `build_scenes` with the same flags: objects under build/augment/, the source hash compiled in
    (`aug_source_hash`; `_augment_lib.load()` refuses a stale binary)."""
    os.makedirs(AUGMENT_OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = sorted(f for f in os.listdir(AUGMENT_CSRC) if f.endswith(".hip"))
    stamp_src = os.path.join(AUGMENT_OBJ, "stamp.cpp")
    stamp = 'extern "C" const char* aug_source_hash(void) { return "%s"; }\n' % _srchash().augment_source_hash()
    if not os.path.exists(stamp_src) or open(stamp_src).read() != stamp:
        open(stamp_src, "w").write(stamp)
    deps = [os.path.join(AUGMENT_CSRC, f) for f in sorted(os.listdir(AUGMENT_CSRC)) if f.endswith(".h")] + [AUGMENT_HEADER]
    hipcc = _hipcc()
    objs, compiled = [], False
    for s in srcs:
        src, obj = os.path.join(AUGMENT_CSRC, s), os.path.join(AUGMENT_OBJ, s[:-4] + ".o")
        objs.append(obj)
        if force or _newer([src] + deps, obj):
            r = subprocess.run([hipcc] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
            if verbose and (r.stderr.strip() or r.returncode):
                sys.stderr.write(r.stderr)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}")
            compiled = True
            if verbose:
                print(f"[build] compiled augment/{s}")
    if force or compiled or _newer(objs + [stamp_src], AUGMENT_LIB):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", AUGMENT_LIB] + objs + [stamp_src], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise RuntimeError("link failed")
        if verbose:
            print(f"[build] linked {AUGMENT_LIB}")
    return AUGMENT_LIB


# libanystereo_spatial.so (include/anystereo_spatial.h): the spatial augmentation's library, a build of its own like the two above; it
# includes csrc/cubic.h, which is therefore one of its dependencies and part of its source hash
SPATIAL_CSRC = os.path.join(CSRC, "spatial")
SPATIAL_OBJ = os.path.join(OBJ, "spatial")
SPATIAL_LIB = os.path.join(LIBDIR, "libanystereo_spatial.so")
SPATIAL_HEADER = os.path.join(HERE, "..", "include", "anystereo_spatial.h")


def build_spatial(force: bool = False, verbose: bool = True) -> str:
    """The recipe of `build_augment`: objects under build/spatial/, the source hash compiled in (`spt_source_hash`;
    `_spatial_lib.load()` refuses a stale binary)."""
    os.makedirs(SPATIAL_OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = sorted(f for f in os.listdir(SPATIAL_CSRC) if f.endswith(".hip"))
    stamp_src = os.path.join(SPATIAL_OBJ, "stamp.cpp")
    stamp = 'extern "C" const char* spt_source_hash(void) { return "%s"; }\n' % _srchash().spatial_source_hash()
    if not os.path.exists(stamp_src) or open(stamp_src).read() != stamp:
        open(stamp_src, "w").write(stamp)
    deps = ([os.path.join(SPATIAL_CSRC, f) for f in sorted(os.listdir(SPATIAL_CSRC)) if f.endswith(".h")] + [SPATIAL_HEADER]
            + list(_srchash().SPATIAL_SHARED))
    hipcc = _hipcc()
    objs, compiled = [], False
    for s in srcs:
        src, obj = os.path.join(SPATIAL_CSRC, s), os.path.join(SPATIAL_OBJ, s[:-4] + ".o")
        objs.append(obj)
        if force or _newer([src] + deps, obj):
            r = subprocess.run([hipcc] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
            if verbose and (r.stderr.strip() or r.returncode):
                sys.stderr.write(r.stderr)
            if r.returncode != 0:
                raise RuntimeError(f"hipcc failed on {src}")
            compiled = True
            if verbose:
                print(f"[build] compiled spatial/{s}")
    if force or compiled or _newer(objs + [stamp_src], SPATIAL_LIB):
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SPATIAL_LIB] + objs + [stamp_src], capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise RuntimeError("link failed")
        if verbose:
            print(f"[build] linked {SPATIAL_LIB}")
    return SPATIAL_LIB


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    # the hash of every native source, compiled into the library (as_source_hash): _lib.load() refuses a stale binary
    stamp_src = os.path.join(OBJ, "stamp.cpp")
    stamp = 'extern "C" const char* as_source_hash(void) { return "%s"; }\n' % _source_hash()
    if not os.path.exists(stamp_src) or open(stamp_src).read() != stamp:
        open(stamp_src, "w").write(stamp)
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")] + [HEADER]
    hipcc = _hipcc()
    jobs = []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s[:-4] + ".o")
        if force or _newer([src] + deps, obj):
            jobs.append((src, obj))

    def compile_one(job):
        src, obj = job
        cmd = [hipcc] + FLAGS + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        return job, r

    if jobs:
        with cf.ThreadPoolExecutor(max_workers=min(4, len(jobs))) as ex:
            for (src, obj), r in ex.map(compile_one, jobs):
                if verbose and (r.stderr.strip() or r.returncode):
                    sys.stderr.write(r.stderr)
                if r.returncode != 0:
                    raise RuntimeError(f"hipcc failed on {src}")
                if verbose:
                    print(f"[build] compiled {os.path.basename(src)}")
    objs = [os.path.join(OBJ, s[:-4] + ".o") for s in srcs]
    if force or jobs or _newer(objs + [stamp_src], LIB):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs + [stamp_src]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            raise RuntimeError("link failed")
        if verbose:
            print(f"[build] linked {LIB}")
    build_scenes(force=force, verbose=verbose)
    build_augment(force=force, verbose=verbose)
    build_spatial(force=force, verbose=verbose)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
