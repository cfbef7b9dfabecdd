"""The init-disparity head's backward (csrc/init_head.hip) at the cfg-4 per-rank shape (B=4, D=48, 40x80 = the 1/4-resolution
volume of a 160x320 crop; train_continuous_IGEV.py:96-122 under --supervise_init) against the path it replaces, and the graphed
cfg-4 training step with supervise_init off and on (alternated blocks in one process).  One JSON object on stdout.

    python tools/kbench_init_head.py                          # everything
    python tools/kbench_init_head.py --skip-step              # kernels only
    rocprofv3 --kernel-trace --stats -d OUT -o kb -- python tools/kbench_init_head.py --skip-step   # per-kernel times
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

import torch  # noqa: E402

HBM_BPS = 6.3e12      # what the chip reaches on a streaming copy
FP32_FLOPS = 157.3e12


def _events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us per call


def kernels(reps):
    from anystereo import grad as G
    from anystereo import ops
    from anystereo.harness.synthetic import det_uniform
    from anystereo.nn import blocks as B
    from anystereo.nn import functional as AF
    dev = "cuda:0"
    b, d, h, w = 4, 48, 40, 80
    geo = det_uniform((b, 8, d, h, w), 1).to(dev)
    conv = torch.nn.Conv3d(8, 1, 3, 1, 1, bias=False).to(dev)
    with torch.no_grad():
        conv.weight.copy_(det_uniform((1, 8, 3, 3, 3), 2) * 0.24)
    g = det_uniform((b, 1, h, w), 3).to(dev)
    x = geo.clone().requires_grad_(True)
    with torch.no_grad():
        cost = B.conv3d_train(conv, geo).squeeze(1).float().contiguous()
    wt = conv.weight.detach().contiguous()
    kernel_us = _events(lambda: ops.init_head_bwd(geo, wt, cost, g), reps)
    new = G.InitDispHead.apply(x, conv.weight)
    new_us = _events(lambda: torch.autograd.grad(new, (x, conv.weight), g, retain_graph=True), reps)
    old = AF.softmax_disparity_regression(B.conv3d_train(conv, x).squeeze(1))
    old_us = _events(lambda: torch.autograd.grad(old, (x, conv.weight), g, retain_graph=True), reps)
    ga = torch.autograd.grad(new, (x, conv.weight), g, retain_graph=True)
    gb = torch.autograd.grad(old, (x, conv.weight), g, retain_graph=True)
    nbytes = 4 * (2 * geo.numel() + cost.numel() + g.numel())
    flops = 2 * 2 * 27 * geo.numel()  # d_geo and dW: 27 FMAs each per geo element
    floor_us = max(nbytes / HBM_BPS, flops / FP32_FLOPS) * 1e6
    return {"shape": [b, 8, d, h, w], "bytes": nbytes, "flop": flops, "floor_us": round(floor_us, 2),
            "floor_bound": "HBM" if nbytes / HBM_BPS > flops / FP32_FLOPS else "fp32 VALU",
            "init_head_bwd_plus_reduce_us": round(kernel_us, 2), "x_floor": round(kernel_us / floor_us, 2),
            "autograd_backward_new_us": round(new_us, 2), "autograd_backward_replaced_us": round(old_us, 2),
            "new_vs_replaced_max_rel_dev": {"d_geo": ((ga[0] - gb[0]).abs().max() / gb[0].abs().max()).item(),
                                            "d_weight": ((ga[1] - gb[1]).abs().max() / gb[1].abs().max()).item()}}


def step(blocks, steps):
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer, synthetic_train_batch
    from anystereo.models import __models__, default_args
    dev = "cuda:0"
    args = default_args("continuous_IGEVStereo")
    batch = synthetic_train_batch(4, 160, 320, seed=0, device=dev, low_disp=True)
    trs = {}
    for on in (False, True):
        m = __models__["continuous_IGEVStereo"](args)
        fill_module_deterministic(m, base_seed=1)
        trs[on] = Trainer(m.to(dev), train_iters=16, max_disp=args.max_disp, supervise_init=on)
    bt = {False: batch[:5], True: batch}
    for on, tr in trs.items():
        for _ in range(6):  # 3 eager warm-up steps, the capture, replays
            tr.step(bt[on])
        assert tr._graph is not None
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(blocks):
        for on in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                trs[on].step(bt[on])
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {"what": "cfg-4 graphed Trainer step, 4 x 160x320, 16 GRU iters, 51200 queries/sample, one rank",
            "supervise_init_off_ms": [round(v, 2) for v in ms[False]], "supervise_init_on_ms": [round(v, 2) for v in ms[True]],
            "median_off_ms": round(med[False], 2), "median_on_ms": round(med[True], 2),
            "on_minus_off_ms": round(med[True] - med[False], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "kbench_init_head needs a GPU"
    out = {"kernels": kernels(a.reps)}
    if not a.skip_step:
        out["step"] = step(a.blocks, a.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
