"""The reference's evaluation protocol (evaluation.py:104-553: validate_things / validate_kitti / validate_middlebury /
validate_eth3d) on the device: EPE, D1 and Thres-1/2/3 per image over the regions all / non-occluded / occluded, averaged over
the dataset.

Per update the prediction is read ONCE (`ops.disparity_metrics`, csrc/eval_metrics.hip): 19 numbers per (estimate, image) stay
on the device until `result()`, which synchronises once.  The reference's form is 45 metric calls per image, each a mask-gather,
a reduction and an `.item()` after `.cpu()`.

    ev = Evaluator("things")
    for image1, image2, gt, gt_right, valid_gt in loader:
        ev.update(model(...).view(B, H, W), gt, valid_gt, gt_right=gt_right)
    print(ev.result()["noc"]["EPE"])

On CPU tensors the Evaluator computes the same 19-number rows with plain torch (`metric_rows_host`, `lr_consistency_host`) — the
ops themselves refuse CPU tensors.  That restatement is what the tests compare the kernels against.
"""
from __future__ import annotations

import time
from typing import Optional, Sequence

import torch

from . import dist
from .query import pad_for_multi_train, prepare_on_device, query_plan, resize_disparity_host

REGIONS = ("all", "noc", "occ")
METRICS = ("EPE", "D1", "Thres1", "Thres2", "Thres3")
ROW = 19  # per region (n, sum E, n_D1, n_T1, n_T2, n_T3), then n_gt_pos

# protocol -> (valid_gt comparison, its threshold, the `_filter` rule)
#   validate_things      evaluation.py:391  valid_gt > 0.5,   *_metric_filter
#   validate_kitti       evaluation.py:275  valid_gt >= 0.5,  *_metric
#   validate_middlebury  evaluation.py:500  valid_gt >= -0.5, *_metric
#   validate_eth3d       evaluation.py:154  valid_gt >= -0.5, *_metric
PROTOCOLS = {"things": ("gt", 0.5, True), "kitti": ("ge", 0.5, False), "middlebury": ("ge", -0.5, False), "eth3d": ("ge", -0.5, False)}
GT_MAX = 1000.0      # `disp_gt < 1000` of every protocol
FILTER_RATIO = 0.01  # metrics.py:53


# ---- plain-torch restatement (any device; used for CPU tensors) -----------------------------------------------------------
@torch.no_grad()
def metric_rows_host(est, gt, valid=None, noc=None, gt_lo=float("-inf"), gt_hi=float("inf"), thres=(1.0, 2.0, 3.0)):
    """What `ops.disparity_metrics` returns, stated with torch ops: est fp32 [N,B,H,W], gt fp32 [B,H,W], valid / noc bool or uint8
    [B,H,W] or None -> fp64 [N,B,19].  E is formed in fp32 and summed in fp64; masking is a select."""
    if est.dim() == 3:
        est = est.unsqueeze(0)
    ones = torch.ones_like(gt, dtype=torch.bool)
    v = (ones if valid is None else valid.bool()) & (gt > gt_lo) & (gt < gt_hi)
    nc = ones if noc is None else noc.bool()
    x = torch.where(torch.isinf(est), torch.zeros_like(est), est)
    err = (gt.unsqueeze(0) - x).abs()
    d1 = (err > 3) & (err / gt.abs().unsqueeze(0) > 0.05)
    e64 = err.double()
    zero = torch.zeros((), dtype=torch.float64, device=est.device)
    cols = []
    for region in (v, v & nc, v & ~nc):
        r = region.unsqueeze(0).expand_as(err)
        cols.append(r.sum((-2, -1)).double())
        cols.append(torch.where(r, e64, zero).sum((-2, -1)))
        cols.append((r & d1).sum((-2, -1)).double())
        for t in thres:
            cols.append((r & (err > float(t))).sum((-2, -1)).double())
    cols.append((gt > 0).sum((-2, -1)).double().unsqueeze(0).expand(est.shape[0], -1))
    return torch.stack(cols, dim=-1)


def _linspace01(n, device):
    """linspace(0, 1, n) in fp32, one rounding per operation: step = 1 / (n - 1), up from 0 in the first half, down from 1 after."""
    i = torch.arange(n, device=device)
    step = torch.ones((), dtype=torch.float32, device=device) / float(n - 1)
    return torch.where(i < n // 2, step * i.float(), 1.0 - step * (n - 1 - i).float())


def _sample_coord(g01, n):
    """[0,1] grid value -> pixel coordinate of grid_sample(align_corners=False, padding_mode='border')."""
    g = 2.0 * g01 - 1.0
    return (((g + 1.0) * float(n) - 1.0) / 2.0).clamp(0.0, float(n - 1))


@torch.no_grad()
def lr_consistency_host(dl, dr, thr=3.0):
    """What `ops.lr_consistency` returns, stated with torch ops (occ_mask, experiment.py:286-296, in closed form): the first warp
    samples the column ramp, so it yields the clamped sampling coordinate itself; the second interpolates that image bilinearly."""
    b, h, w = dl.shape
    assert dr.shape == dl.shape and h >= 2 and w >= 2
    xs = _linspace01(w, dl.device)
    l2r = _sample_coord(xs + dr / float(w), w)                      # [B,H,W]
    x = _sample_coord(xs + (-dl) / float(w), w)                     # [B,H,W]
    y = _sample_coord(_linspace01(h, dl.device), h)                 # [H]
    xf, yf = x.floor(), y.floor()
    xa = xf.long().clamp(0, w - 1)
    ya = yf.long().clamp(0, h - 1)
    xb, yb = (xa + 1).clamp(max=w - 1), (ya + 1).clamp(max=h - 1)
    wx1, wx0 = x - xf, (xf + 1.0) - x
    wy1, wy0 = (y - yf).view(1, h, 1), ((yf + 1.0) - y).view(1, h, 1)
    bi = torch.arange(b, device=dl.device).view(b, 1, 1)
    ya, yb = ya.view(1, h, 1), yb.view(1, h, 1)
    v = l2r[bi, ya, xa] * (wx0 * wy0)
    v = v + l2r[bi, ya, xb] * (wx1 * wy0)
    v = v + l2r[bi, yb, xa] * (wx0 * wy1)
    v = v + l2r[bi, yb, xb] * (wx1 * wy1)
    col = torch.arange(w, device=dl.device).float()
    return ((col - v).abs() < thr).to(torch.uint8)


class Evaluator:
    """Accumulates the per-image metric rows of one dataset pass.

    protocol: "things" (SceneFlow: `valid = valid_gt > 0.5 & gt < 1000`, the non-occluded mask from the left-right consistency of
    `gt` and `gt_right`, and the `_filter` rule: an image is skipped for a region when n_region / n_gt_pos < 0.01, metrics.py:53) or
    "kitti" / "middlebury" / "eth3d" (plain metrics, `noc` supplied by the caller; None = everything non-occluded).
    max_disp: additionally `gt < max_disp` (--max_enable).  thres: the three Thres-k thresholds.

    The reference's guards (evaluation.py:399,412) hold for every protocol: an image with no non-occluded pixel contributes to no
    region, and its occluded numbers count only when that region is non-empty.

    Averaging is over IMAGES, each image weighing the same.  The reference averages per-batch means over batches; the two agree
    whenever the batch size is 1 (the reference's evaluation default) or no image of a batch is filtered.  (With batch size 1 the
    reference books a filtered image as a 0 — metrics.py:59-61 — where this class leaves it out of the mean and reports the count.)
    """

    def __init__(self, protocol: str = "things", max_disp: Optional[float] = None, thres: Sequence[float] = (1, 2, 3)):
        if protocol not in PROTOCOLS:
            raise ValueError(f"Evaluator: unknown protocol {protocol!r} (one of {sorted(PROTOCOLS)})")
        if len(thres) != 3:
            raise ValueError("Evaluator: three thresholds expected")
        self.protocol = protocol
        self.gt_hi = GT_MAX if max_disp is None else min(GT_MAX, float(max_disp))
        self.thres = tuple(float(t) for t in thres)
        self._rows = []

    def _valid_mask(self, valid, gt):
        if valid is None:
            return None
        if valid.dim() == 4 and valid.shape[1] == 1:
            valid = valid[:, 0]
        if valid.dtype in (torch.bool, torch.uint8):
            return valid.contiguous()
        op, t, _ = PROTOCOLS[self.protocol]
        return ((valid > t) if op == "gt" else (valid >= t)).contiguous()

    @torch.no_grad()
    def update(self, est, gt, valid=None, noc=None, gt_right=None) -> None:
        """est fp32 [N,B,H,W] (N estimates of the same images) or [B,H,W]; gt fp32 [B,H,W] (or [B,1,H,W]); valid = the dataset's
        valid_gt (float, thresholded as the protocol does) or a bool / uint8 mask; noc bool / uint8, 1 = non-occluded; gt_right =
        the right view's ground truth ("things": the mask is lr_consistency(gt, gt_right) unless `noc` is given).
        Issues the kernels and returns; nothing is synchronised."""
        if gt.dim() == 4 and gt.shape[1] == 1:
            gt = gt[:, 0]
        if est.dim() == 3:
            est = est.unsqueeze(0)
        if est.dim() != 4 or tuple(est.shape[1:]) != tuple(gt.shape):
            raise ValueError(f"Evaluator.update: est {tuple(est.shape)} does not match gt {tuple(gt.shape)} ([N,B,H,W] against [B,H,W])")
        if self._rows and self._rows[0].shape[0] != est.shape[0]:
            raise ValueError(f"Evaluator.update: {est.shape[0]} estimates after updates with {self._rows[0].shape[0]}")
        est, gt = est.float().contiguous(), gt.float().contiguous()
        v = self._valid_mask(valid, gt)
        on_device = est.is_cuda
        if noc is None and self.protocol == "things":
            if gt_right is None:
                raise ValueError('Evaluator.update: protocol "things" needs gt_right (or a ready noc mask)')
            if gt_right.dim() == 4 and gt_right.shape[1] == 1:
                gt_right = gt_right[:, 0]
            gt_right = gt_right.float().contiguous()
            if on_device:
                from .. import ops
                noc = ops.lr_consistency(gt, gt_right, 3.0)
            else:
                noc = lr_consistency_host(gt, gt_right, 3.0)
        elif noc is not None:
            if noc.dim() == 4 and noc.shape[1] == 1:
                noc = noc[:, 0]
            if noc.dtype not in (torch.bool, torch.uint8):
                noc = noc > 0.5
            noc = noc.contiguous()
        if on_device:
            from .. import ops
            rows = ops.disparity_metrics(est, gt, v, noc, float("-inf"), self.gt_hi, self.thres)
        else:
            rows = metric_rows_host(est, gt, v, noc, float("-inf"), self.gt_hi, self.thres)
        self._rows.append(rows)

    def rows(self) -> torch.Tensor:
        """Every image's row so far, fp64 [N, images, 19] on the host (synchronises)."""
        if not self._rows:
            return torch.zeros((0, 0, ROW), dtype=torch.float64)
        return torch.cat(self._rows, dim=1).cpu()

    def merge(self, device="cpu") -> None:
        """All ranks' rows on every rank, for a dataset sharded by `dist.shard_indices` (rank r holds images r, r + world, ...): each
        rank places its rows at its images' positions in a zero array and the arrays are summed over the ranks
        (`dist.sum_over_ranks`; adding zeros is exact, so the merged rows are the single-process rows bit for bit).
        `device`: where the collective's buffer lives ("cpu" for gloo, the rank's GPU for RCCL)."""
        rank, world, _ = dist.env_rank()
        if world <= 1:
            return
        mine = self.rows()
        counts = [0.0] * world
        counts[rank] = float(mine.shape[1])
        n_est = [0.0] * world
        n_est[rank] = float(mine.shape[0])
        both = dist.sum_over_ranks(counts + n_est, device=device)
        counts, n_est = [int(c) for c in both[:world]], [int(c) for c in both[world:]]
        total, n = sum(counts), max(n_est)
        for r in range(world):
            if counts[r] != len(dist.shard_indices(total, r, world)) or (counts[r] and n_est[r] != n):
                raise RuntimeError(f"Evaluator.merge: rank {r} holds {counts[r]} images x {n_est[r]} estimates; a dataset of {total} "
                                   f"images sharded by dist.shard_indices gives it {len(dist.shard_indices(total, r, world))}")
        full = torch.zeros((n, total, ROW), dtype=torch.float64)
        if mine.shape[1]:
            full[:, dist.shard_indices(total, rank, world)] = mine
        flat = dist.sum_over_ranks(full.reshape(-1).tolist(), device=device)
        self._rows = [torch.tensor(flat, dtype=torch.float64).view(n, total, ROW)]

    def result(self) -> dict:
        """{"all" | "noc" | "occ": {"EPE" | "D1" | "Thres1" | "Thres2" | "Thres3": [N floats]}, "images": {"seen", "all", "noc",
        "occ"}} — the mean over the images that count for the region (0.0 where none does).  One synchronisation."""
        rows = self.rows()
        n_est, n_img = rows.shape[0], rows.shape[1]
        out = {"images": {"seen": n_img}}
        if n_img == 0:
            for r in REGIONS:
                out[r] = {m: [] for m in METRICS}
                out["images"][r] = 0
            return out
        cnt = [rows[0, :, 6 * r] for r in range(3)]   # the masks do not depend on the estimate
        pos = rows[0, :, 18]
        keep = [cnt[1] > 0, cnt[1] > 0, (cnt[1] > 0) & (cnt[2] > 0)]
        if PROTOCOLS[self.protocol][2]:
            keep = [k & ~((c / pos) < FILTER_RATIO) for k, c in zip(keep, cnt)]  # x / 0 = inf or nan: not below the ratio, as in the reference
        for r, name in enumerate(REGIONS):
            k = keep[r]
            n_keep = int(k.sum())
            out["images"][name] = n_keep
            res = {}
            for m, mname in enumerate(METRICS):
                if n_keep == 0:
                    res[mname] = [0.0] * n_est
                    continue
                per_image = rows[:, k, 6 * r + 1 + m] / rows[:, k, 6 * r]
                res[mname] = [float(x) for x in per_image.mean(dim=1)]
            out[name] = res
        return out


def _field_estimates(model, i1, i2, coord, sc, iters, ks, baseline, scale, divis_by, h, w):
    """[N,B,H,W]: the curve's iterations and the baseline of one padded pair, from ONE encoded pass."""
    from .. import ops
    bs = i1.shape[0]
    field = model.encode(i1, i2, iters=iters, at=ks)
    ests = [field.query(coord.clone(), sc, at=k).reshape(bs, h, w) for k in ks]
    if baseline == "bicubic":
        h_pad, w_pad = i1.shape[-2:]
        plan = query_plan(h, w, scale, divis_by)  # the pair's geometry: where the low-resolution frame lies inside the padded one
        if (plan.h_pad, plan.w_pad) != (h_pad, w_pad):
            raise RuntimeError(f"evaluate: the padded pair is {h_pad}x{w_pad}, query_plan gives {plan.h_pad}x{plan.w_pad}")
        one = query_plan(h_pad, w_pad, 1.0, divis_by)  # the padded frame queried at its own pixels: no padding, no resize
        if i1.is_cuda:
            grid = ops.query_grid(one, bs, i1.device)
        else:
            from .query import query_grid_host
            grid = query_grid_host(one, bs, i1.device)
        low = field.query(grid, torch.ones_like(sc)).reshape(bs, h_pad, w_pad)
        crop, size = (plan.pad[0], plan.pad[2], plan.h_lr, plan.w_lr), (h, w)
        ests.append(ops.resize_disparity(low, crop, size, float(scale)) if low.is_cuda
                    else resize_disparity_host(low, crop, size, float(scale)))
    return torch.stack(ests, 0)


@torch.no_grad()
def evaluate(model, pairs, scale: float, iters: int, protocol: str = "kitti", max_disp: Optional[float] = None, thres=(1, 2, 3),
             divis_by: int = 32, evaluator: Optional[Evaluator] = None, prep: str = "host", images=None, curve=None,
             baseline: Optional[str] = None) -> dict:
    """Run `model` over `pairs` as the reference's validate_* loops do (evaluation.py:341-373): down-scale by `scale` and pad
    (`query.pad_for_multi_train`), query the full-resolution grid in test_mode, reshape [B,1,Q] -> [B,H,W] and feed an Evaluator.

    pairs: an iterable of (image1, image2, gt, valid) or (image1, image2, gt, valid, extra) on the model's device — image [B,3,H,W],
    gt [B,H,W]; `extra` is the right view's ground truth for "things" and the non-occluded mask for the other protocols.
    Returns the Evaluator's result plus {"pairs", "seconds", "pairs_per_s"}; the host synchronises once, at the end.  `evaluator`:
    feed this one (a rank of a sharded dataset calls its `merge()` afterwards) instead of a new Evaluator(protocol, ...).
    prep: "host" = `query.pad_for_multi_train` (torch ops, the query grid built on the host and uploaded); "device" =
    `query.prepare_on_device` (two launches, nothing on the host; the images may be uint8).
    images: an `images.ImageSink` (or None): every batch's prediction and gt go to its `add` — one more launch and non-blocking
    copies, still no synchronisation inside the loop — and its `flush()` writes the PNG files after the one synchronisation (outside
    the timed span); the result gains "images_written".  The sink's pinned host buffers are allocated inside the loop, once per
    batch until its first flush (reused afterwards): that allocation is in the timed span.  With None nothing changes.

    With `curve` and `baseline` at None only the last GRU iteration is evaluated, by the model's forward: in test_mode the models
    up-sample the final disparity alone (continuous_IGEVstereo.py:267-268).
    curve: 1-based GRU iterations, each at most `iters`, e.g. (4, 8, 16, 32): the pass is encoded ONCE per batch
    (`model.encode(..., at=curve)`) and every iteration of the curve is one more query of that field — accuracy per iteration for
    one loop instead of one evaluation per candidate `iters`.
    baseline: "bicubic" = the interpolation baseline of the reference's `multi_evaothers` branch (evaluation.py:91-100, :125-146):
    the disparity at scale 1 on the padded low-resolution frame — here a second query of the same field, the model's OWN scale-1
    output; other fixed-scale networks are not built — un-padded, multiplied by `scale` and resized bicubically to the full
    frame (`ops.resize_disparity`).  It is the protocol the continuous output is meant to beat.
    With either option the estimates are, in order, the curve's iterations (`iters` alone when curve is None) and the baseline;
    all go into one `Evaluator.update` as [N,B,H,W], the result gains "estimates": ["iter4", ..., "bicubic"], and `images` takes
    the last continuous estimate.  Still one synchronisation per dataset."""
    if prep not in ("host", "device"):
        raise ValueError(f"evaluate: prep must be 'host' or 'device', got {prep!r}")
    if baseline not in (None, "bicubic"):
        raise ValueError(f"evaluate: baseline must be None or 'bicubic', got {baseline!r}")
    field_mode = curve is not None or baseline is not None
    if field_mode:
        ks = (int(iters),) if curve is None else tuple(int(k) for k in curve)
        if not ks or any(k < 1 or k > int(iters) for k in ks) or list(ks) != sorted(set(ks)):
            raise ValueError(f"evaluate: curve must be ascending distinct iterations in [1, {int(iters)}], got {curve!r}")
        names = [f"iter{k}" for k in ks] + ([baseline] if baseline else [])
    ev = evaluator if evaluator is not None else Evaluator(protocol, max_disp=max_disp, thres=thres)
    model.eval()
    n_pairs = 0
    t0 = time.perf_counter()
    for pair in pairs:
        image1, image2, gt, valid = pair[:4]
        extra = pair[4] if len(pair) > 4 else None
        bs, _, h, w = image1.shape
        if prep == "device":
            i1, i2, coord, _ = prepare_on_device(image1, image2, scale, divis_by=divis_by)
        else:
            i1, i2, coord, _ = pad_for_multi_train(image1, image2, scale, divis_by=divis_by)
            coord = coord.to(image1.device).unsqueeze(0).expand(bs, *coord.shape).contiguous()
            i1, i2 = i1.contiguous(), i2.contiguous()
        sc = torch.full((bs, 1), float(scale), device=image1.device)
        if field_mode:
            est = _field_estimates(model, i1, i2, coord, sc, iters, ks, baseline, scale, divis_by, h, w)
        else:
            pred = model(i1, i2, iters=iters, test_mode=True, hr_coord=coord, scale=sc)
            est = pred.reshape(1, bs, h, w)
        if ev.protocol == "things":
            ev.update(est, gt, valid, gt_right=extra)
        else:
            ev.update(est, gt, valid, noc=extra)
        if images is not None:
            images.add(est[len(ks) - 1] if field_mode else est[0], gt)
        n_pairs += bs
    res = ev.result()  # the one synchronisation
    dt = time.perf_counter() - t0
    res.update(pairs=n_pairs, seconds=dt, pairs_per_s=(n_pairs / dt if dt > 0 else 0.0))
    if field_mode:
        res["estimates"] = names
    if images is not None:
        res["images_written"] = len(images.flush())
    return res
