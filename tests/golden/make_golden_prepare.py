"""Regenerates tests/golden/prepare_pair.npz from the reference's own pad_for_multi_train (needs the reference checkout):

    python tests/golden/make_golden_prepare.py

evaluation.py cannot be imported (see make_golden.py: missing packages, a dangling model import), so the single function is compiled
from its AST node, with the reference's InputPadder and make_coord; InputPadder.get_pad_num is undefined in the reference and is
supplied with the only meaning its call site allows ([top, bottom, left, right]).

Per case k of CASES = (H, W, scale, divis_by) — the reference chooses divis_by by model name: 32 for *IGEVStereo*, 16 otherwise —
with B = 2 seeded 8-bit-valued images per side (all four images differ):
    c{k}_image1, c{k}_image2   uint8 [2,3,H,W]      the inputs (the reference receives them as float32)
    c{k}_pad1, c{k}_pad2       fp32 [2,3,h_pad,w_pad]  the reference's image1_pad / image2_pad
    c{k}_coord                 fp32 [H*W,2]           the reference's hr_coord
    cases                      fp64 [5,4]             CASES
The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
from __future__ import annotations

import argparse
import ast
import io
import math
import os
import sys
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, import_reference  # noqa: E402

CASES = [(40, 64, 1.0, 32), (64, 96, 2.0, 32), (37, 53, 1.5, 32), (45, 70, 1.3, 16), (33, 65, 2.95, 32)]
BATCH = 2


def reference_pad_for_multi_train():
    import_reference()
    import models.coreContinuous_IGEV.liif as rliif
    from models.coreContinuous_IGEV.utils.utils import InputPadder as RefPadder
    RefPadder.get_pad_num = lambda self: [self._pad[2], self._pad[3], self._pad[0], self._pad[1]]
    tree = ast.parse(open(os.path.join(REF, "evaluation.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "pad_for_multi_train"][0]
    ns = {"math": math, "F": F, "torch": torch, "InputPadder": RefPadder, "make_coord": rliif.make_coord}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "evaluation.py", "exec"), ns)
    return ns["pad_for_multi_train"]


def main():
    torch.set_num_threads(1)  # the bits of ATen's CPU kernels do not depend on it; one thread keeps it that way
    ref = reference_pad_for_multi_train()
    arrs = {"cases": np.asarray(CASES, dtype=np.float64)}
    for k, (h, w, s, div) in enumerate(CASES):
        g = torch.Generator().manual_seed(4100 + k)
        im1 = torch.randint(0, 256, (BATCH, 3, h, w), generator=g, dtype=torch.uint8)
        im2 = torch.randint(0, 256, (BATCH, 3, h, w), generator=g, dtype=torch.uint8)
        args = argparse.Namespace(scale_test=s, model="continuous_IGEVStereo" if div == 32 else "continuous_RAFTStereo")
        p1, p2, coord = ref(args, im1.float(), im2.float())
        assert p1.dtype == torch.float32 and coord.dtype == torch.float32 and tuple(coord.shape) == (h * w, 2)
        assert p1.shape[-2] % div == 0 and p1.shape[-1] % div == 0
        arrs.update({f"c{k}_image1": im1, f"c{k}_image2": im2, f"c{k}_pad1": p1, f"c{k}_pad2": p2, f"c{k}_coord": coord})
        print(f"case {k} {(h, w, s, div)}: padded {tuple(p1.shape[-2:])}, values {float(p1.min()):.1f} .. {float(p1.max()):.1f}")

    path = os.path.join(HERE, "prepare_pair.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrs):
            a = arrs[name]
            a = np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a)
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))  # fixed: the file regenerates bit for bit
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"wrote prepare_pair.npz ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
