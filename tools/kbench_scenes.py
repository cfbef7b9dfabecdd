"""The three kernels of csrc/scenes/scenes.hip at the cfg-4 and cfg-2 shapes against their byte floors (the bytes they write: they read
nothing but a [B,Q,2] coordinate list) and against the host path (the plain-torch restatements on CPU tensors plus the upload).

    python tools/kbench_scenes.py [--out profiles/scenes_kbench.txt]

cfg 4 (training): render_pair B = 4 at 160 x 320; ground_truth of the four crops at scales 1.0, 1.65, 2.3, 2.95 (left disparity only,
as scene_train_batch asks for it) and with all three outputs; disparity_at B = 4, Q = 51 200.
cfg 2 (evaluation): render_pair B = 1 at 540 x 960; ground_truth of one 540 x 960 frame (disp + disp_right, and disp + noc);
disparity_at B = 1, Q = 518 400 with the mask.

`us` = device events around repeated warm calls of the Python op (allocations and ctypes call included), median of the blocks.  The
kernels are arithmetic, not traffic: ~100 integer hashes per rendered pixel and a loop over the layers per view, so `of floor` says how
far below the write bandwidth that arithmetic sits, not how well a copy was written.  A floor below 3 us is launch-bound by
construction.  `host us` = the restatement on CPU tensors (torch's default threads) and the copy of its results to the device, host
clock, best of 2 — the data path a loader process would be, not the code under test.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

HBM_BPS = 6.3e12
LAUNCH_US = 3.0
SCALES = [1.0, 1.65, 2.3, 2.95]


def _events(fn, reps, blocks):
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
    return sorted(out)[len(out) // 2]


def _host(fn, dev):
    import torch
    best = None
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        for t in res:
            if t is not None:
                t.to(dev)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e6
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from anystereo import _scenes_lib
    from anystereo.harness import scenes as H
    from anystereo.nn.liif import make_coord
    assert torch.cuda.is_available(), "kbench_scenes needs a GPU"
    dev = torch.device("cuda:0")
    spec = H.SceneSpec()
    flat = lambda lists: [t for lst in lists for t in lst]  # noqa: E731
    crops = [(round(160 * s), round(320 * s)) for s in SCALES]
    n_crops = sum(h * w for h, w in crops)
    coord4 = torch.stack([make_coord([160, 320]) for _ in range(4)]).contiguous()
    coord2 = make_coord([540, 960]).view(1, -1, 2).contiguous()
    c4, c2 = coord4.to(dev), coord2.to(dev)
    rows = [
        ("cfg4 render_pair B=4 160x320", 2 * 4 * 3 * 160 * 320 * 4,
         lambda d: H.render_pair(spec, 1, 0, 4, 160, 320, d)),
        ("cfg4 ground_truth 4 crops (disp)", n_crops * 4,
         lambda d: flat(H.ground_truth(spec, 1, crops, [0, 1, 2, 3], d, want=("disp",)))),
        ("cfg4 ground_truth 4 crops (all three)", n_crops * 9,
         lambda d: flat(H.ground_truth(spec, 1, crops, [0, 1, 2, 3], d))),
        ("cfg4 disparity_at B=4 Q=51200", 4 * 51200 * (8 + 4),
         lambda d: [H.disparity_at(spec, 1, [0, 1, 2, 3], c4 if d.type == "cuda" else coord4, [320.0] * 4)]),
        ("cfg2 render_pair B=1 540x960", 2 * 3 * 540 * 960 * 4,
         lambda d: H.render_pair(spec, 1, 0, 1, 540, 960, d)),
        ("cfg2 ground_truth 540x960 (disp, disp_right)", 540 * 960 * 8,
         lambda d: flat(H.ground_truth(spec, 1, [(540, 960)], [0], d, want=("disp", "disp_right")))),
        ("cfg2 ground_truth 540x960 (disp, noc)", 540 * 960 * 5,
         lambda d: flat(H.ground_truth(spec, 1, [(540, 960)], [0], d, want=("disp", "noc")))),
        ("cfg2 disparity_at B=1 Q=518400 (+noc)", 518400 * (8 + 4 + 1),
         lambda d: list(H.disparity_at(spec, 1, [0], c2 if d.type == "cuda" else coord2, [960.0], noc=True))),
    ]
    lines = ["python tools/kbench_scenes.py --reps %d --blocks %d" % (a.reps, a.blocks),
             "device: %s; library: %s" % (torch.cuda.get_device_name(0), _scenes_lib.library_info()),
             "floor = bytes / %.1f TB/s; below %.0f us a row is launch-bound; host = CPU restatement (%d threads) + upload" % (
                 HBM_BPS / 1e12, LAUNCH_US, torch.get_num_threads()),
             "", "%-48s %10s %10s %10s %9s %12s %8s %6s" % ("row", "bytes", "floor us", "us", "of floor", "host us", "host/dev", "equal")]
    cpu = torch.device("cpu")
    for name, nbytes, fn in rows:
        us = _events(lambda: fn(dev), a.reps, a.blocks)
        floor = nbytes / HBM_BPS * 1e6
        host_us = _host(lambda: fn(cpu), dev)
        same = all((g is None and w is None) or bool(torch.equal(g.cpu(), w)) for g, w in zip(fn(dev), fn(cpu)))
        lines.append("%-48s %10d %10.2f %10.2f %8.1f%% %12.0f %8.0f %6s" % (name, nbytes, floor, us, 100.0 * floor / us, host_us, host_us / us,
                                                                        "yes" if same else "NO"))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
