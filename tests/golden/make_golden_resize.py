"""Regenerates tests/golden/resize_disp.npz from the reference's own interpolation baseline (needs the reference checkout):

    python tests/golden/make_golden_resize.py

The `multi_evaothers` branch of validate_* (evaluation.py:125-146) pads with pad_for_muti_other (:91-100), runs a fixed-scale model
and resizes its answer: `flow_pr = padder.unpad(flow_pr).cpu()`, then, for scale_test > 1,
`F.interpolate(flow_pr * args.scale_test, (H, W), mode='bicubic', align_corners=False)`.  evaluation.py cannot be imported (see
make_golden.py), so pad_for_muti_other and those two statements are compiled from their AST nodes, with the reference's InputPadder.
pad_for_muti_other always pads to a multiple of 32; for the divis_by = 16 case the name `InputPadder` it looks up is bound to the
reference's class with that divisor, nothing else differs.

Per case k of CASES = (H, W, scale, divis_by) — the shapes of prepare_pair.npz: odd sizes, padding on both sides, ceil making
H != hc * scale:
    c{k}_map    fp32 [2,1,h_pad,w_pad]  the "model output" on the padded low-resolution frame: integers in [-3, 200] from a hash of
                                        the position, the crop's first two rows / columns at -3 and its last two at 200, the padding
                                        next to them at 200 resp. -3 — a step edge ON the crop border, so that a resize whose taps
                                        are clamped to the padded frame instead of the crop differs by tens of pixels
    c{k}_crop   int64 [4]               (top, left, hc, wc) of the un-padded frame inside the map
    c{k}_out    fp32 [2,1,H,W]          the reference's result
    cases       fp64 [5,4]              CASES
The script checks on the way that the wrong-frame restatement misses the tests' limit on every resized case (the fixture can tell the
two apart).  The file is written with fixed zip timestamps: a second run gives the same bytes.
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


def reference_baseline():
    """-> (pad(args, image1, image2, divis_by) -> padder, resize(args, image1, padder, flow_pr) -> flow_pr)."""
    import_reference()
    from models.coreContinuous_IGEV.utils.utils import InputPadder as RefPadder
    tree = ast.parse(open(os.path.join(REF, "evaluation.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "pad_for_muti_other"][0]
    val = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "validate_eth3d"][0]
    stmts = None
    for node in ast.walk(val):  # the first unpad / resize pair of the function: the multi_evaothers branch
        body = getattr(node, "body", None)
        if not isinstance(body, list):
            continue
        for a, b in zip(body, body[1:]):
            if (ast.unparse(a) == "flow_pr = padder.unpad(flow_pr).cpu()" and isinstance(b, ast.If)
                    and ast.unparse(b.test) == "args.scale_test > 1" and "bicubic" in ast.unparse(b)):
                stmts = [a, b]
                break
        if stmts:
            break
    assert stmts is not None, "the multi_evaothers statements were not found in evaluation.py"
    code = compile(ast.Module(body=stmts, type_ignores=[]), "evaluation.py", "exec")

    def pad(args, image1, image2, divis_by):
        ns = {"math": math, "F": F, "torch": torch, "InputPadder": lambda dims, divis_by_=divis_by, **_: RefPadder(dims, divis_by=divis_by_)}
        exec(compile(ast.Module(body=[fn], type_ignores=[]), "evaluation.py", "exec"), ns)
        return ns["pad_for_muti_other"](args, image1, image2)[2]

    def resize(args, image1, padder, flow_pr):
        ns = {"F": F, "torch": torch, "args": args, "image1": image1, "padder": padder, "flow_pr": flow_pr}
        exec(code, ns)
        return ns["flow_pr"]

    return pad, resize


def padded_map(k, h_pad, w_pad, top, left, hc, wc):
    n = torch.arange(BATCH).view(-1, 1, 1)
    y = torch.arange(h_pad).view(1, -1, 1)
    x = torch.arange(w_pad).view(1, 1, -1)
    m = ((y * 37 + x * 101 + n * 53 + k * 17 + (y * x) % 7) % 204 - 3).float()
    yc, xc = y - top, x - left
    inside = (yc >= 0) & (yc < hc) & (xc >= 0) & (xc < wc)
    lo = inside & ((yc < 2) | (xc < 2))
    hi = inside & ~lo & ((yc >= hc - 2) | (xc >= wc - 2))
    m = torch.where(lo.expand_as(m), torch.full_like(m, -3.0), m)
    m = torch.where(hi.expand_as(m), torch.full_like(m, 200.0), m)
    m = torch.where((~inside & ((yc < 0) | (xc < 0))).expand_as(m), torch.full_like(m, 200.0), m)
    m = torch.where((~inside & (yc >= 0) & (xc >= 0)).expand_as(m), torch.full_like(m, -3.0), m)
    return m.unsqueeze(1).contiguous()


def wrong_frame(m, crop, size, mul):
    """The same resize with the taps clamped to the PADDED frame: what the kernel must not compute."""
    top, left, hc, wc = crop
    h, w = size
    x = m[:, 0] * float(mul)

    def axis(n_in, n_out, lo, n_src):
        scale = float(torch.tensor(float(n_in)) / torch.tensor(float(n_out)))
        src = scale * (torch.arange(n_out).float() + 0.5) - 0.5
        fl = src.floor()
        t = src - fl
        a = -0.75
        c1 = lambda v: ((a + 2) * v - (a + 3)) * v * v + 1  # noqa: E731
        c2 = lambda v: ((a * v - 5 * a) * v + 8 * a) * v - 4 * a  # noqa: E731
        idx = torch.stack([(lo + fl.long() - 1 + j).clamp(0, n_src - 1) for j in range(4)])
        return idx, torch.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)])
    iy, wy = axis(hc, h, top, x.shape[1])
    ix, wx = axis(wc, w, left, x.shape[2])
    out = 0
    for a in range(4):
        rows = x[:, iy[a]]
        out = out + sum(rows[:, :, ix[b]] * wx[b].view(1, 1, -1) for b in range(4)) * wy[a].view(1, -1, 1)
    return out.unsqueeze(1)


def main():
    torch.set_num_threads(1)
    pad, resize = reference_baseline()
    arrs = {"cases": np.asarray(CASES, dtype=np.float64)}
    for k, (h, w, s, div) in enumerate(CASES):
        args = argparse.Namespace(scale_test=s)
        image = torch.zeros(1, 3, h, w)
        padder = pad(args, image, image, div)
        p = padder._pad  # [left, right, top, bottom]
        hc, wc = math.ceil(h / s) if s > 1 else h, math.ceil(w / s) if s > 1 else w
        h_pad, w_pad = hc + p[2] + p[3], wc + p[0] + p[1]
        assert h_pad % div == 0 and w_pad % div == 0
        crop = (p[2], p[0], hc, wc)
        m = padded_map(k, h_pad, w_pad, *crop)
        out = resize(args, image, padder, m.clone())
        assert out.dtype == torch.float32 and tuple(out.shape) == (BATCH, 1, h, w), out.shape
        lim = 1e-3 / 255 * float((m * s).abs().max())
        if s > 1:
            d = float((wrong_frame(m, crop, (h, w), s) - out).abs().max())
            assert d > 100 * lim, (k, d, lim)
            print(f"case {k} {(h, w, s, div)}: map {h_pad}x{w_pad}, crop {crop}, limit {lim:.2e}, wrong-frame restatement off by {d:.1f}")
        else:
            assert torch.equal(out, m[:, :, crop[0]:crop[0] + hc, crop[1]:crop[1] + wc])
            print(f"case {k} {(h, w, s, div)}: map {h_pad}x{w_pad}, crop {crop}: the crop itself")
        arrs.update({f"c{k}_map": m, f"c{k}_crop": np.asarray(crop, dtype=np.int64), f"c{k}_out": out})

    path = os.path.join(HERE, "resize_disp.npz")
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
    print(f"wrote resize_disp.npz ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
