"""Compare the gfx950 machine code of every kernel between two source trees.

    python tools/codegen_diff.py OLD_TREE NEW_TREE [file.hip ...]

Each named csrc/*.hip (default: every one whose text, or any csrc/*.h, differs between the trees) is compiled
for the device only with build.py's FLAGS in both trees, to gfx950 assembly rather than to a linked code object:
in the linked ELF every kernel that touches a __device__ variable carries a pc-relative distance to it, which
moves whenever ANY kernel of the file changes size.  Per function (kernels, and device functions left out of
line) the text from its label to its end, kernel descriptor (register counts, LDS size) included, is hashed with
the file-wide numbering of local labels removed; the line says identical / DIFFERS, or only-old / only-new when
a name appears in one tree alone.  Needs hipcc, no GPU.
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile


def _build_py(tree):
    spec = importlib.util.spec_from_file_location("as_build", os.path.join(tree, "any-stereo_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+")  # .LBB12_3 -> .LBB_3: the function's index in the file is not part of its code
_LOOPREF = re.compile(r"\bBB\d+_")             # the same index in the loop comments ("Parent Loop BB12_3 Depth=1")
_PAD = re.compile(r"[ \t]+")                   # ... whose column padding shrinks when the index gains a digit


def symbols(path):
    """{name: sha1 of the function's assembly} for every function of a device .s file (kernel descriptor included)."""
    out, name, lines = {}, None, []
    for line in open(path):
        if "-- Begin function " in line:
            name, lines = line.split("-- Begin function ")[1].strip(), []
        elif "-- End function" in line and name:
            out[name] = hashlib.sha1(_PAD.sub(" ", _LOOPREF.sub("BB_", _LOCAL.sub(r".L\1", "".join(lines)))).encode()).hexdigest()
            name = None
        elif name:
            lines.append(line)
    return out


def compile_device(tree, name, outdir):
    b = _build_py(tree)
    asm = os.path.join(outdir, name + ".s")
    cmd = [b._hipcc()] + b.FLAGS + ["--cuda-device-only", "-S", os.path.join(b.CSRC, name), "-o", asm]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {tree}/{name}:\n{r.stderr}")
    return symbols(asm)


def _read(tree, name):
    p = os.path.join(tree, "any-stereo_amd", "csrc", name)
    return open(p, "rb").read() if os.path.exists(p) else None


def main(argv):
    old, new = os.path.abspath(argv[0]), os.path.abspath(argv[1])
    names = argv[2:]
    if not names:
        csrc = sorted(os.listdir(os.path.join(new, "any-stereo_amd", "csrc")))
        hdr = any(_read(old, h) != _read(new, h) for h in csrc if h.endswith(".h"))
        names = [f for f in csrc if f.endswith(".hip") and _read(old, f) is not None and (hdr or _read(old, f) != _read(new, f))]
    differing = 0
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new, cf.ThreadPoolExecutor(8) as ex:
        jobs = [(n, ex.submit(compile_device, old, n, t_old), ex.submit(compile_device, new, n, t_new)) for n in names]
        for n, fo, fn in jobs:
            so, sn = fo.result(), fn.result()
            rows = [(s, "identical" if so.get(s) == sn.get(s) else "only-new" if s not in so else "only-old" if s not in sn else "DIFFERS")
                    for s in sorted(set(so) | set(sn))]
            bad = [r for r in rows if r[1] != "identical"]
            differing += len(bad)
            print(f"== {n}: {len(rows)} symbols, {len(rows) - len(bad)} identical, {len(bad)} not")
            for s, verdict in rows:
                print(f"  {verdict:9s} {s}")
    print(f"total not identical: {differing}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
