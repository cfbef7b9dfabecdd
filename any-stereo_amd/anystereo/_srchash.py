"""The table of the native libraries and the content hash of each one's sources.

build.py compiles `source_hash(key)` into the library (`<prefix>_source_hash()`), `_native.open_library` recomputes it from the
tree and refuses a library built from other sources: the built `.so` is git-ignored but travels with the repo snapshot, so a stale
binary would otherwise run silently on the GPU box.  Each library has a hash of its own: the sources are the TOP LEVEL of its
directory, so csrc/scenes/ is no part of the main library's hash, and an edit there rebuilds the scenes' library alone.

build.py loads this file by path, without importing the package: nothing here imports anystereo or torch.
"""
import collections
import hashlib
import os

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")   # the repository
ERRSTATE = "any-stereo_amd/csrc/host/errstate.h"   # err_buf / fail / REQUIRE / check_launch of the three small libraries

# file: in anystereo/lib/; sources, header, shared: paths below the repository root; shared: headers from outside `sources` that
# its files include; prefix: of every exported symbol; override: the environment variable that names another build of the file
Library = collections.namedtuple("Library", "file sources header shared prefix override")
LIBRARIES = {
    "hip": Library("libanystereo_hip.so", "any-stereo_amd/csrc", "include/anystereo_hip.h", (), "as", "ANYSTEREO_LIB"),
    "scenes": Library("libanystereo_scenes.so", "any-stereo_amd/csrc/scenes", "include/anystereo_scenes.h", (ERRSTATE,), "scn",
                      "ANYSTEREO_SCENES_LIB"),
    "augment": Library("libanystereo_augment.so", "any-stereo_amd/csrc/augment", "include/anystereo_augment.h", (ERRSTATE,), "aug",
                       "ANYSTEREO_AUGMENT_LIB"),
    # cubic.h: the final resize's arithmetic, shared with the main library
    "spatial": Library("libanystereo_spatial.so", "any-stereo_amd/csrc/spatial", "include/anystereo_spatial.h",
                       ("any-stereo_amd/csrc/cubic.h", ERRSTATE), "spt", "ANYSTEREO_SPATIAL_LIB"),
}


def source_hash(key: str, root: str = ROOT) -> str | None:
    """16 hex digits over the *.hip and *.h files in the top level of the library's directory (sorted; name, then bytes), its shared
    headers in the table's order (base name, then bytes) and its header's bytes.  None when any of them is not there (an installed
    library without its tree)."""
    lib = LIBRARIES[key]
    csrc, header, shared = (os.path.join(root, lib.sources), os.path.join(root, lib.header), [os.path.join(root, f) for f in lib.shared])
    if not (os.path.isdir(csrc) and all(os.path.exists(f) for f in [header] + shared)):
        return None
    h = hashlib.sha256()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(csrc, f), "rb").read())
    for f in shared:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    h.update(open(header, "rb").read())
    return h.hexdigest()[:16]
