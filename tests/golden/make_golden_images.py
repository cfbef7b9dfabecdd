"""Regenerates tests/golden/eval_images.npz from the reference's own picture functions (needs the reference checkout):

    python tests/golden/make_golden_images.py

evaluation.py cannot be imported (missing packages, a dangling model import), so `Disp_to_color` (evaluation.py:35-65) is compiled
from its AST node, as make_golden_prepare.py does for pad_for_multi_train; metrics_utils/visualization.py is loaded by file path
(the package's __init__ imports torchvision) and its `disp_error_image_func.forward` (visualization.py:30-55) is called directly.

Per case k of CASES = (B, H, W, max_disp):
    c{k}_disp    fp32 [B,H,W]    the disparity of the colour picture: seeded uniform values with, at seeded positions, every colour
                                 edge e_j * max_disp and its neighbours within 2 ulp, +-0, max_disp and its two neighbours, negatives,
                                 values above max_disp and +-inf (no NaN: the reference hands NaN on to save_image)
    c{k}_gt      fp32 [B,H,W]    ground truth, ~15 % of it <= 0
    c{k}_est     fp32 [B,H,W]    the estimate of the error picture: gt + noise with, outside the legend, errors exactly on each of the
                                 nine inner band edges and 1 ulp either side in both regimes (gt = 30: the absolute term E / 3 is the
                                 minimum; gt = 100: the relative term (E / gt) / 0.05 is), and NaN, +inf, -inf estimates
    c{k}_color   fp32 [B,H,W,3]  Disp_to_color(disp[b:b+1], max_disp), image by image (the reference's repeat(6,1,1) serves B = 1)
    c{k}_error   fp32 [B,H,W,3]  disp_error_image_func.forward(est, gt)
    cases        fp64 [4,4]      CASES
The shapes: 2 x 13 x 37 = 962 pixels (two left over after the groups of four, the second image starts at an odd pixel, the legend
clipped at x = 37), 1 x 7 x 250 (the legend clipped by the height, ending at x = 200), 2 x 24 x 203 (a multiple of four, the whole
legend) and 1 x 1 x 5 (one group and one pixel).  The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
from __future__ import annotations

import ast
import importlib.util
import io
import os
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

CASES = [(2, 13, 37, 192.0), (1, 7, 250, 192.0), (2, 24, 203, 400.0), (1, 1, 5, 192.0)]
EDGES = (114, 299, 413, 587, 701, 886)
BAND_EDGES = (0.0625, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)


def reference_functions():
    tree = ast.parse(open(os.path.join(REF, "evaluation.py")).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "Disp_to_color"][0]
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "evaluation.py", "exec"), ns)
    spec = importlib.util.spec_from_file_location("ref_visualization", os.path.join(REF, "metrics_utils", "visualization.py"))
    vis = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vis)
    return ns["Disp_to_color"], lambda est, gt: vis.disp_error_image_func.forward(None, est, gt)


def ulps(x: float, k: int) -> float:
    v = np.float32(x)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return float(v)


def color_specials(max_disp: float):
    m = np.float32(max_disp)
    out = []
    for c in EDGES:
        x = np.float32(np.float32(c) / np.float32(1000.0)) * m
        out += [ulps(x, k) for k in (0, 1, -1, 2, -2)]
    out += [0.0, -0.0, float(m), ulps(m, -1), ulps(m, 1), -1.0, -1e-3, float(m) * 1.5, float("inf"), float("-inf")]
    return out


def error_specials():
    """(gt, est) pairs: |gt - est| on every inner band edge and 1 ulp of est either side, in both regimes, then NaN and +-inf."""
    out = []
    for i, edge in enumerate(BAND_EDGES):
        for gt, scale in ((30.0, 3.0), (100.0, 5.0)):  # E / 3 == edge; (E / 100) / 0.05 ~ edge
            sign = 1.0 if i % 2 else -1.0
            est = gt + sign * edge * scale
            out += [(gt, ulps(est, k)) for k in (0, 1, -1)]
    out += [(30.0, float("nan")), (30.0, float("inf")), (100.0, float("-inf"))]
    return out


def make_case(k, b, h, w, max_disp):
    g = torch.Generator().manual_seed(5200 + k)
    n = b * h * w
    disp = (torch.rand(n, generator=g) * (1.35 * max_disp) - 0.15 * max_disp).float()
    gt = (torch.rand(n, generator=g) * 160.0 - 24.0).float()
    est = gt + (torch.rand(n, generator=g) * 2.0 - 1.0) * torch.exp(torch.rand(n, generator=g) * 6.0 - 2.0)
    # colour specials: anywhere
    spec = color_specials(max_disp)
    pos = torch.randperm(n, generator=g)[:len(spec)]
    for p, v in zip(pos.tolist(), spec):  # a case smaller than the list takes its head: an edge first
        disp[p] = v
    # error specials: outside the legend, where the band shows
    q = torch.arange(n) % (h * w)
    free = torch.nonzero(~((q // w < 10) & (q % w < 200))).flatten()
    free = free[torch.randperm(free.numel(), generator=g)]
    for p, (gv, ev) in zip(free.tolist(), error_specials()):
        gt[p], est[p] = gv, ev
    return disp.view(b, h, w), gt.view(b, h, w), est.float().view(b, h, w)


def main():
    torch.set_num_threads(1)
    to_color, error_image = reference_functions()
    arrs = {"cases": np.asarray(CASES, dtype=np.float64)}
    for k, (b, h, w, max_disp) in enumerate(CASES):
        disp, gt, est = make_case(k, b, h, w, max_disp)
        color = torch.stack([to_color(disp[i:i + 1], max_disp).permute(1, 2, 0) for i in range(b)])
        with np.errstate(all="ignore"):
            error = error_image(est, gt).permute(0, 2, 3, 1)
        assert color.dtype == torch.float32 and tuple(color.shape) == (b, h, w, 3) and not torch.isnan(color).any()
        assert error.dtype == torch.float32 and tuple(error.shape) == (b, h, w, 3)
        arrs.update({f"c{k}_disp": disp, f"c{k}_gt": gt, f"c{k}_est": est, f"c{k}_color": color.contiguous(),
                     f"c{k}_error": error.contiguous()})
        bands = sorted({tuple(int(round(float(x) * 255)) for x in px) for px in error.reshape(-1, 3)})
        print(f"case {k} {(b, h, w, max_disp)}: {len(bands)} distinct error colours, gt <= 0 on {(gt <= 0).float().mean().item():.2f}, "
              f"white {(color.min(-1).values >= 1).sum().item()}, black {(color.max(-1).values <= 0).sum().item()}")

    path = os.path.join(HERE, "eval_images.npz")
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
    print(f"wrote eval_images.npz ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
