"""The one loader, the one source hash and the table behind them (anystereo/_native.py, anystereo/_srchash.py), for each of the four
libraries alike: all of them load and answer their host-only entries without a GPU."""
import ctypes as C
import importlib
import os

import pytest

from _headers import declared_symbols
from anystereo import _native, _srchash

MODULES = {"hip": "_lib", "scenes": "_scenes_lib", "augment": "_augment_lib", "spatial": "_spatial_lib"}
KEYS = list(_srchash.LIBRARIES)


def _binding(key):
    return importlib.import_module("anystereo." + MODULES[key])


def test_every_row_has_a_binding():
    assert KEYS == list(MODULES) == ["hip", "scenes", "augment", "spatial"]   # build.py builds them in this order
    assert len({row.prefix for row in _srchash.LIBRARIES.values()}) == len({row.file for row in _srchash.LIBRARIES.values()}) == 4


@pytest.mark.parametrize("key", KEYS)
def test_load_binds_every_symbol_and_describes_the_library(key):
    L, row = _binding(key), _srchash.LIBRARIES[key]
    lib = L.load()
    assert L.load() is lib
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    info = L.library_info()
    assert set(info) == {"path", "abi", "src_hash", "matches_sources"}
    assert info["matches_sources"] is True and len(info["src_hash"]) == 16
    assert info["abi"] == getattr(lib, row.prefix + "_abi_version")()
    assert os.path.samefile(info["path"], L.LIB_PATH) and os.path.basename(L.LIB_PATH) == row.file


@pytest.mark.parametrize("key", KEYS)
def test_a_library_built_from_other_sources_is_refused(key, monkeypatch):
    """The .so is git-ignored but travels with the snapshot: a stale binary must not run silently on the GPU box."""
    L = _binding(key)
    L.load()
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(_srchash, "source_hash", lambda key, root=None: "0" * 16)
    with pytest.raises(RuntimeError, match="built from other sources"):
        L.load()
    assert L._lib is None
    monkeypatch.setenv("ANYSTEREO_ALLOW_STALE_LIB", "1")
    assert L.load() is L._lib is not None


@pytest.mark.parametrize("key", KEYS)
def test_a_missing_file_names_the_build(key, monkeypatch, tmp_path):
    L = _binding(key)
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", str(tmp_path / "nowhere.so"))
    with pytest.raises(RuntimeError, match=r"%s not found at .*nowhere\.so: build it with `python any-stereo_amd/build\.py`"
                       % _srchash.LIBRARIES[key].file.replace(".", r"\.")):
        L.load()


@pytest.mark.parametrize("key", KEYS)
def test_a_symbol_that_is_not_exported_is_an_error(key):
    L = _binding(key)
    bogus = _srchash.LIBRARIES[key].prefix + "_no_such_entry"
    with pytest.raises(AttributeError, match=bogus):
        _native.open_library(key, {**L.SIGNATURES, bogus: (C.c_int, [])})
    assert isinstance(_native.open_library(key, L.SIGNATURES), C.CDLL)


@pytest.mark.parametrize("key", KEYS)
def test_a_failed_call_raises_with_the_library_s_message(key):
    L = _binding(key)
    L.check(0, "x")
    label = {"hip": "HIP"}.get(key, key)
    with pytest.raises(RuntimeError, match=r"anystereo %s call x failed \(code -7\): " % label):
        L.check(-7, "x")


@pytest.mark.parametrize("key", KEYS)
def test_signatures_are_what_the_header_declares(key):
    L = _binding(key)
    declared = declared_symbols(key)
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)


# ---- what feeds which hash, on a synthetic tree in the table's layout --------------------------------------------------------------

def _tree(root):
    for key, row in _srchash.LIBRARIES.items():
        for rel in (row.sources + "/%s.hip" % key, row.sources + "/%s_local.h" % key, row.header) + row.shared:
            path = os.path.join(root, rel)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            if not os.path.exists(path):
                open(path, "w").write("// %s\n" % rel)


def _hashes(root):
    return {key: _srchash.source_hash(key, str(root)) for key in KEYS}


def _changed(root, rel, edit):
    before = _hashes(root)
    edit(os.path.join(root, rel))
    after = _hashes(root)
    return {key for key in KEYS if after[key] != before[key]}, after


def _append(path):
    open(path, "a").write("// edited\n")


def test_what_feeds_which_hash(tmp_path):
    _tree(tmp_path)
    first = _hashes(tmp_path)
    assert all(isinstance(h, str) and len(h) == 16 and int(h, 16) >= 0 for h in first.values()) and len(set(first.values())) == 4
    assert _hashes(tmp_path) == first
    csrc = _srchash.LIBRARIES["hip"].sources
    assert _changed(tmp_path, csrc + "/scenes/scenes.hip", _append)[0] == {"scenes"}
    assert _changed(tmp_path, csrc + "/scenes/scenes_local.h", _append)[0] == {"scenes"}
    assert _changed(tmp_path, csrc + "/cubic.h", _append)[0] == {"hip", "spatial"}
    assert _changed(tmp_path, _srchash.ERRSTATE, _append)[0] == {"scenes", "augment", "spatial"}
    assert _changed(tmp_path, csrc + "/hip.hip", _append)[0] == {"hip"}
    assert _changed(tmp_path, csrc + "/notes.txt", _append)[0] == set()      # neither *.hip nor *.h
    for key, row in _srchash.LIBRARIES.items():
        assert _changed(tmp_path, row.header, _append)[0] == {key}
    # a missing header, shared header or directory: no hash (an installed library without its tree)
    for key, row in _srchash.LIBRARIES.items():
        changed, after = _changed(tmp_path, row.header, os.remove)
        assert changed == {key} and after[key] is None
        _tree(tmp_path)
    changed, after = _changed(tmp_path, _srchash.ERRSTATE, os.remove)
    assert changed == {"scenes", "augment", "spatial"} and [after[k] for k in KEYS[1:]] == [None] * 3
    assert _srchash.source_hash("hip", str(tmp_path / "nowhere")) is None


def test_the_tree_s_hashes_follow_the_rule():
    """The rule written out once more, independently, on the real tree: sorted top-level sources as name + bytes, shared headers as
    base name + bytes, then the header's bytes."""
    import hashlib
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    for key, row in _srchash.LIBRARIES.items():
        h = hashlib.sha256()
        d = os.path.join(root, row.sources)
        for f in sorted(os.listdir(d)):
            if os.path.isfile(os.path.join(d, f)) and (f.endswith(".hip") or f.endswith(".h")):
                h.update(f.encode() + open(os.path.join(d, f), "rb").read())
        for f in row.shared:
            h.update(os.path.basename(f).encode() + open(os.path.join(root, f), "rb").read())
        h.update(open(os.path.join(root, row.header), "rb").read())
        assert _srchash.source_hash(key) == h.hexdigest()[:16], key
