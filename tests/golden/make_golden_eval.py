"""Regenerates tests/golden/eval_metrics.npz from the reference's metrics_utils (needs the reference checkout):

    python tests/golden/make_golden_eval.py

Per shape s in (2,24,80), (1,37,131), (2,64,200) — a two-plane scene: left disparity 4.25 + 0.03 * row with a foreground
rectangle at 13.5 over rows [H/4, 3H/4) x cols [W/3, 2W/3) (moved right by 7 columns per sample, so the samples of a batch
differ), right disparity = the same planes with the rectangle moved left by int(13.5), U(0, 0.2) noise on both:
    s{k}_dl, s{k}_dr       fp32 [B,H,W]
    s{k}_occ_mask          uint8 — the reference's occ_mask(dl, dr) (1 = consistent = non-occluded)
    s{k}_l2r2l             fp32 — the reference's warped column index (for the margin | |x - l2r2l| - 3 |)
    s{k}_est               fp32 [2,B,H,W] — dl + noise of sigma 2.5 px; estimate 0 holds a handful of +-inf, estimate 1 none; no NaN
    s{k}_valid_gt          fp32 0 / 1 with ~10 % holes
    s{k}_plain, s{k}_filter  fp32 [2 estimates, 3 regions (all, noc, occ), 5 (EPE, D1, Thres1, Thres2, Thres3)] — the reference's
                           *_metric / *_metric_filter over valid = valid_gt > 0.5 & gt < 1000, valid & occ_mask, valid & ~occ_mask
Protocol cases on sample 0 of shape 0 (batch of 1):
    case_filter_valid_gt   valid_gt that leaves 4 non-occluded pixels: the `_filter` rule skips the region (share of gt > 0 below 0.005)
    case_filter_out        [3 regions, 5] — *_metric_filter (the skipped region reads 0, metrics.py:59-61)
    case_filter_skip       uint8 [3] — the reference's own skip expression per region (metrics.py:53)
    case_guard_valid_gt    valid_gt with no non-occluded pixel: the guard of evaluation.py:399 skips the image
The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
from __future__ import annotations

import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = "/root/reference"
sys.path.insert(0, os.path.join(ROOT, "any-stereo_amd"))

from anystereo.harness.synthetic import det_uniform  # noqa: E402

SHAPES = [(2, 24, 80), (1, 37, 131), (2, 64, 200)]
NEAR = 1e-3        # a pixel is "near" when the reference's own margin to the threshold is below this
NEAR_CAP = 0.005   # at most this share of a shape's pixels may be near
Q = 4096.0         # inputs are multiples of 1 / 4096 (compresses better; exact in fp32)


def import_metrics():
    sys.modules.setdefault("metrics_utils", types.ModuleType("metrics_utils")).__path__ = [REF + "/metrics_utils"]
    if "torchvision" not in sys.modules:  # experiment.py imports torchvision.utils for image logging only
        tv = types.ModuleType("torchvision"); tv.utils = types.ModuleType("torchvision.utils")
        sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
    import metrics_utils.experiment as rexp
    import metrics_utils.metrics as rmet
    return rmet, rexp


def quant(t):
    return torch.round(t * Q) / Q


def scene(b, h, w, seed):
    row = torch.arange(h, dtype=torch.float32).view(1, h, 1)
    bg = (4.25 + 0.03 * row).expand(b, h, w)
    dl, dr = bg.clone(), bg.clone()
    for i in range(b):
        c0, c1 = w // 3 + 7 * i, 2 * w // 3 + 7 * i
        dl[i, h // 4:3 * h // 4, c0:c1] = 13.5
        dr[i, h // 4:3 * h // 4, c0 - 13:c1 - 13] = 13.5
    dl = dl + det_uniform((b, h, w), seed, 0.0, 0.2)
    dr = dr + det_uniform((b, h, w), seed + 1, 0.0, 0.2)
    return quant(dl).contiguous(), quant(dr).contiguous()


def noise(shape, seed, sigma):
    """~N(0, sigma^2): the sum of four hashed uniforms (plain arithmetic, so the same bits everywhere)."""
    s = sum(det_uniform(shape, seed + i, 0.0, 1.0) for i in range(4))
    return (s - 2.0) * (3.0 ** 0.5) * sigma


def ref_metrics(rmet, est, gt, masks, filt):
    f = (rmet.EPE_metric_filter, rmet.D1_metric_filter, rmet.Thres_metric_filter) if filt else (rmet.EPE_metric, rmet.D1_metric, rmet.Thres_metric)
    out = np.zeros((len(masks), 5), dtype=np.float32)
    for r, m in enumerate(masks):
        out[r] = [float(f[0](est, gt, m)), float(f[1](est, gt, m)), float(f[2](est, gt, m, 1.0)), float(f[2](est, gt, m, 2.0)),
                  float(f[2](est, gt, m, 3.0))]
    return out


def main():
    rmet, rexp = import_metrics()
    arrs = {}
    for k, (b, h, w) in enumerate(SHAPES):
        dl, dr = scene(b, h, w, 1000 + 10 * k)
        left, right = dl.unsqueeze(1), dr.unsqueeze(1)
        occ = rexp.occ_mask(left, right)[:, 0]
        index = torch.arange(w).float().repeat(b, 1, h, 1)
        l2r2l = rexp.warp(rexp.warp(index, right), -left)[:, 0]
        margin = ((index[:, 0] - l2r2l).abs() - 3.0).abs()
        near = float((margin < NEAR).float().mean())
        assert near <= NEAR_CAP, f"shape {(b, h, w)}: {near:.4f} of the pixels lie within {NEAR} of the threshold"
        assert torch.equal(occ, ((index[:, 0] - l2r2l).abs() < 3.0).float())
        if b > 1:
            assert not torch.equal(occ[0], occ[1]), "the samples of a batch must differ"
        est = torch.stack([quant(dl + noise((b, h, w), 2000 + 10 * k + 4 * i, 2.5)) for i in range(2)])
        flat = est[0].view(-1)
        for j, p in enumerate(range(5, flat.numel(), flat.numel() // 6)):  # a handful of +-inf, at valid and invalid pixels alike
            flat[p] = float("inf") if j % 2 == 0 else float("-inf")
        assert torch.isinf(est[0]).sum() >= 5 and not torch.isinf(est[1]).any() and not torch.isnan(est).any()
        valid_gt = (det_uniform((b, h, w), 3000 + k, 0.0, 1.0) > 0.1).float()
        valid = (valid_gt > 0.5) & (dl < 1000)
        noc = valid & occ.bool()
        masks = [valid, noc, valid & ~noc]
        assert all(int(m.sum()) > 0 for m in masks)
        plain, filt = [], []
        for i in range(2):
            e = torch.where(torch.isinf(est[i]), torch.zeros_like(est[i]), est[i])  # evaluation.py:389
            plain.append(ref_metrics(rmet, e, dl, masks, False))
            filt.append(ref_metrics(rmet, e, dl, masks, True))
        arrs.update({f"s{k}_dl": dl, f"s{k}_dr": dr, f"s{k}_occ_mask": occ.to(torch.uint8), f"s{k}_l2r2l": l2r2l, f"s{k}_est": est,
                     f"s{k}_valid_gt": valid_gt, f"s{k}_plain": np.stack(plain), f"s{k}_filter": np.stack(filt)})
        print(f"shape {(b, h, w)}: noc {int(noc.sum())}, occ {int(masks[2].sum())}, near {near:.2e}, "
              f"within 1e-2 {float((margin < 1e-2).float().mean()):.2e}")

    # ---- protocol cases: sample 0 of shape 0 as a batch of 1 ----
    dl, occ = arrs["s0_dl"][:1], arrs["s0_occ_mask"][:1].bool()
    est = arrs["s0_est"][1, :1]
    n_pos = int((dl > 0).sum())
    noc_idx = occ.view(-1).nonzero().view(-1)
    keep = torch.zeros_like(occ.view(-1))
    keep[noc_idx[::max(1, len(noc_idx) // 4)][:4]] = True           # 4 non-occluded pixels stay valid
    v_filter = ((~occ) | keep.view_as(occ)).float()
    v_guard = (~occ).float()
    valid = v_filter > 0.5
    masks = [valid, valid & occ, valid & ~occ]
    skip = np.zeros(3, dtype=np.uint8)
    for r, m in enumerate(masks):
        ratio = float(m.float().mean() / (dl > 0).float().mean())
        assert ratio < 0.005 or ratio > 0.02, f"filter case: region {r} ratio {ratio} too close to 0.01"
        skip[r] = ratio < 0.01
        assert skip[r] == (m[0].float().mean() / (dl[0] > 0).float().mean() < 0.01)
    assert list(skip) == [0, 1, 0] and int(masks[1].sum()) == 4, (skip, [int(m.sum()) for m in masks], n_pos)
    assert int(((v_guard > 0.5) & occ).sum()) == 0 and int((v_guard > 0.5).sum()) > 0
    arrs.update(case_filter_valid_gt=v_filter, case_guard_valid_gt=v_guard, case_filter_out=ref_metrics(rmet, est, dl, masks, True),
                case_filter_skip=skip)

    path = os.path.join(HERE, "eval_metrics.npz")
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
    print(f"wrote eval_metrics.npz ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
