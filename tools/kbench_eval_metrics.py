"""The evaluation kernels (csrc/eval_metrics.hip) at the cfg-2 (540x960) and Middlebury-F (1988x2964) output sizes against the
paths a user had before them, and against their traffic floors.  One JSON object on stdout (and in --out).

    python tools/kbench_eval_metrics.py [--out profiles/eval_metrics_kbench.json]
    python tools/kbench_eval_metrics.py --only metrics:540x960          # one step, in this process

Steps (each in a child process of its own with a time limit; the parent never opens the GPU and stops at the first failure):
    metrics:HxW   ops.disparity_metrics, N = 1, valid and noc masks (all three regions), device events, median of repeated blocks;
                  beside it the fifteen harness/metrics.py calls (5 metrics x 3 regions) on device tensors with their `.item()`s
    mask:HxW      ops.lr_consistency; beside it the reference's form: two grid_sample warps of the column ramp, stated with torch ops
Floors: 10 B per pixel per estimate (est 4 + gt 4 + 2 masks) and 9 B per pixel (4 reads of dr are cache hits: dl 4 + dr 4 + 1 out) at
6.3 TB/s, plus one ~1.5 us kernel boundary for the two-launch metrics."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

HBM_BPS = 6.3e12          # what the chip reaches on a streaming copy
KERNEL_BOUNDARY_US = 1.5  # a dependent launch on the same stream
SIZES = [(540, 960), (1988, 2964)]


def _median(v):
    return sorted(v)[len(v) // 2]


def _events(fn, reps, blocks):
    """us per call: median over `blocks` of the device-event time of `reps` back-to-back calls."""
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return _median(out), out


def _host(fn, reps, blocks):
    """us per call of a path that synchronises by itself (`.item()`): host clock around synchronised work."""
    import torch
    for _ in range(2):
        fn()
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return _median(out), out


def _scene(h, w, dev):
    """A two-plane scene with noise (the fixture's, at size): left / right disparity, an estimate, valid with ~10 % holes."""
    import torch
    from anystereo.harness.synthetic import det_uniform
    row = torch.arange(h, dtype=torch.float32).view(1, h, 1)
    dl = (4.25 + 0.03 * row * (64.0 / h)).expand(1, h, w).clone()
    dr = dl.clone()
    dl[:, h // 4:3 * h // 4, w // 3:2 * w // 3] = 13.5
    dr[:, h // 4:3 * h // 4, w // 3 - 13:2 * w // 3 - 13] = 13.5
    dl += det_uniform((1, h, w), 1, 0.0, 0.2)
    dr += det_uniform((1, h, w), 2, 0.0, 0.2)
    est = dl + det_uniform((1, h, w), 3, -5.0, 5.0)
    valid = det_uniform((1, h, w), 4, 0.0, 1.0) > 0.1
    return dl.to(dev), dr.to(dev), est.to(dev), valid.to(dev)


def step_metrics(h, w, reps, blocks):
    import torch
    from anystereo import ops
    from anystereo.harness import metrics as M
    dev = "cuda:0"
    dl, dr, est, valid = _scene(h, w, dev)
    noc = ops.lr_consistency(dl, dr)
    est4 = est.unsqueeze(0).contiguous()
    us, all_us = _events(lambda: ops.disparity_metrics(est4, dl, valid, noc, float("-inf"), 1000.0), reps, blocks)

    v = valid & (dl < 1000)
    masks = [v, v & noc.bool(), v & ~noc.bool()]

    def old():
        vals = []
        for m in masks:
            vals += [M.epe_metric(est, dl, m).item(), M.d1_metric(est, dl, m).item(), M.thres_metric(est, dl, m, 1.0).item(),
                     M.thres_metric(est, dl, m, 2.0).item(), M.thres_metric(est, dl, m, 3.0).item()]
        return vals
    old_us, old_all = _host(old, max(1, reps // 20), blocks)
    rows = ops.disparity_metrics(est4, dl, valid, noc, float("-inf"), 1000.0).cpu()[0, 0]
    new_vals = [float(rows[6 * r + 1 + m] / rows[6 * r]) for r in range(3) for m in range(5)]
    dev_max = max(abs(a - b) / max(abs(b), 1e-30) if i % 5 == 0 else abs(a - b) for i, (a, b) in enumerate(zip(new_vals, old())))
    nbytes = 10 * h * w
    floor = nbytes / HBM_BPS * 1e6 + KERNEL_BOUNDARY_US
    return {"step": f"metrics:{h}x{w}", "pixels": h * w, "estimates": 1, "bytes": nbytes, "traffic_floor_us": round(nbytes / HBM_BPS * 1e6, 2),
            "floor_us": round(floor, 2), "disparity_metrics_us": round(us, 2), "blocks_us": [round(x, 2) for x in all_us],
            "x_floor": round(us / floor, 2), "achieved_GBps": round(nbytes / us / 1e3, 1),
            "bound": "launch" if nbytes / HBM_BPS * 1e6 < 2 * KERNEL_BOUNDARY_US else "HBM",
            "fifteen_metric_calls_with_item_us": round(old_us, 1), "old_blocks_us": [round(x, 1) for x in old_all],
            "speedup_vs_fifteen_calls": round(old_us / us, 1), "max_dev_vs_fifteen_calls": dev_max}


def _warp(img, disp):
    """grid_sample(bilinear, border) of img [B,1,H,W] at x + disp on a linspace(0,1,n) base grid (experiment.py:267-284)."""
    import torch
    import torch.nn.functional as F
    b, _, h, w = img.shape
    xb = torch.linspace(0, 1, w, device=img.device).view(1, 1, w).expand(b, h, w)
    yb = torch.linspace(0, 1, h, device=img.device).view(1, h, 1).expand(b, h, w)
    grid = torch.stack((xb + disp[:, 0] / w, yb), dim=3)
    return F.grid_sample(img, 2 * grid - 1, mode="bilinear", padding_mode="border", align_corners=False)


def step_mask(h, w, reps, blocks):
    import torch
    from anystereo import ops
    dev = "cuda:0"
    dl, dr, _, _ = _scene(h, w, dev)
    us, all_us = _events(lambda: ops.lr_consistency(dl, dr), reps, blocks)

    def old():
        index = torch.arange(w, device=dev).float().repeat(1, 1, h, 1)
        back = _warp(_warp(index, dr.unsqueeze(1)), -dl.unsqueeze(1))
        return ((index - back).abs() < 3.0).float()
    old_us, old_all = _events(old, max(1, reps // 10), blocks)
    mism = (ops.lr_consistency(dl, dr).float() != old()[:, 0]).float().mean().item()
    nbytes = 9 * h * w
    floor = nbytes / HBM_BPS * 1e6
    return {"step": f"mask:{h}x{w}", "pixels": h * w, "bytes": nbytes, "floor_us": round(floor, 2), "lr_consistency_us": round(us, 2),
            "blocks_us": [round(x, 2) for x in all_us], "x_floor": round(us / floor, 2), "achieved_GBps": round(nbytes / us / 1e3, 1),
            "bound": "launch" if floor < 2 * KERNEL_BOUNDARY_US else "HBM",
            "two_grid_sample_form_us": round(old_us, 1), "old_blocks_us": [round(x, 1) for x in old_all],
            "speedup_vs_two_grid_sample_form": round(old_us / us, 1), "mask_mismatch_share_vs_two_grid_sample_form": mism}


def run_step(name, reps, blocks):
    import torch
    assert torch.cuda.is_available(), "kbench_eval_metrics needs a GPU"
    kind, size = name.split(":")
    h, w = (int(x) for x in size.split("x"))
    return (step_metrics if kind == "metrics" else step_mask)(h, w, reps, blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--only", default=None, help="run this one step here, e.g. metrics:540x960")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a.reps, a.blocks)))
        return
    steps = [f"{k}:{h}x{w}" for k in ("metrics", "mask") for h, w in SIZES]
    res = {"command": "python tools/kbench_eval_metrics.py", "reps": a.reps, "blocks": a.blocks, "hbm_GBps_assumed": HBM_BPS / 1e9,
           "kernel_boundary_us_assumed": KERNEL_BOUNDARY_US, "steps": []}
    for s in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", s, "--reps", str(a.reps), "--blocks", str(a.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res["error"] = f"{s}: no result after {a.step_timeout} s"
            break
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            res["error"] = f"{s}: exit {r.returncode}: {r.stderr[-800:]}"
            break  # nothing more is started on the GPU after a failure
        res["steps"].append(json.loads(lines[-1]))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if "error" in res:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
