"""The two kernels of csrc/prepare.hip (as_prepare_pair, as_query_grid) against their traffic floors and against the path they replace,
at the cfg-2 (540x960 x1.0), KITTI (375x1242 x2.0) and Middlebury-F (1988x2964 x1.5) protocols.  One JSON object on stdout (and in
--out).

    python tools/kbench_prepare.py [--out profiles/prepare_kbench.json]
    python tools/kbench_prepare.py --only 375x1242x2.0          # one shape, in this process

Per shape (each in a child process of its own with a time limit; the parent never opens the GPU and stops at the first failure),
B = 1, device events around repeated warm calls, median of the blocks:
    prepare_pair_{f32,u8}_us   ops.prepare_pair on float32 / uint8 images; floor = (2 images x 3 x H x W x {4,1} B read +
                               2 x 3 x h_pad x w_pad x 4 B written) / 6.3 TB/s
    query_grid_us              ops.query_grid; floor = B x Q x 8 B written / 6.3 TB/s
    device_path_*              `query.prepare_on_device` (both launches, the plan, the allocations) timed exactly as the replaced path is:
                               host clock between synchronisations (`_host_us`, the figure the speed-up uses) and device events
    replaced_*_us              the path these replace, `query.pad_for_multi_train` on device images + `.to(device)` of the host-built
                               grid + `.expand(B, ...).contiguous()` (what evaluate(prep="host") does per pair), timed end to end on
                               the host clock between synchronisations; `replaced_images_us` is its image part alone (two bicubic
                               F.interpolate + two replicate F.pad + .contiguous()) in device events
A ratio to the floor above 3 is a finding the DESIGN.md entry has to explain; a floor below 3 us is launch-bound by construction
(one launch costs more than the traffic)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

HBM_BPS = 6.3e12   # what the chip reaches on a streaming copy
LAUNCH_US = 3.0    # below this much traffic time a call is launch-bound
SHAPES = [(540, 960, 1.0), (375, 1242, 2.0), (1988, 2964, 1.5)]
DIVIS_BY = 32


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
    """us per call of a path with host work in it: host clock between synchronisations."""
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


def run_shape(h, w, s, reps, blocks):
    import torch
    import torch.nn.functional as F
    from anystereo import ops
    from anystereo.harness.query import InputPadder, pad_for_multi_train, prepare_on_device, query_plan
    assert torch.cuda.is_available(), "kbench_prepare needs a GPU"
    dev = torch.device("cuda:0")
    pl = query_plan(h, w, s, DIVIS_BY)
    g = torch.Generator().manual_seed(5)
    u1 = torch.randint(0, 256, (1, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    u2 = torch.randint(0, 256, (1, 3, h, w), generator=g, dtype=torch.uint8).to(dev)
    f1, f2 = u1.float(), u2.float()
    q = pl.h_want * pl.w_want

    pp_f32, pp_f32_all = _events(lambda: ops.prepare_pair(f1, f2, pl), reps, blocks)
    pp_u8, pp_u8_all = _events(lambda: ops.prepare_pair(u1, u2, pl), reps, blocks)
    qg, qg_all = _events(lambda: ops.query_grid(pl, 1, dev), reps, blocks)

    def old_images():
        a, b = f1, f2
        if s > 1:
            a = F.interpolate(a, (pl.h_lr, pl.w_lr), mode="bicubic", align_corners=False)
            b = F.interpolate(b, (pl.h_lr, pl.w_lr), mode="bicubic", align_corners=False)
        pa, pb = InputPadder(a.shape, divis_by=DIVIS_BY).pad(a, b)
        return pa.contiguous(), pb.contiguous()

    def old_path():
        i1, i2, coord, _ = pad_for_multi_train(f1, f2, s, divis_by=DIVIS_BY)
        coord = coord.to(dev).unsqueeze(0).expand(1, *coord.shape).contiguous()
        return i1.contiguous(), i2.contiguous(), coord

    old_img, old_img_all = _events(old_images, max(1, reps // 10), blocks)
    old_reps = max(1, min(reps // 10, int(4e6 // q) or 1))
    old, old_all = _host(old_path, old_reps, blocks)
    # the device path end to end, on the same clock and with the same repetitions as the path it replaces, and in device events
    new_host, new_host_all = _host(lambda: prepare_on_device(f1, f2, s, divis_by=DIVIS_BY), old_reps, blocks)
    new_host_u8, _ = _host(lambda: prepare_on_device(u1, u2, s, divis_by=DIVIS_BY), old_reps, blocks)
    new_ev, new_ev_all = _events(lambda: prepare_on_device(f1, f2, s, divis_by=DIVIS_BY), reps, blocks)

    # agreement at this size
    n1, _ = ops.prepare_pair(u1, u2, pl)
    o1, _, ocoord = old_path()
    d_img = (n1 - o1).abs().max().item()
    d_grid = (ops.query_grid(pl, 1, dev) - ocoord).abs().max().item()

    in_px, out_px = 2 * 3 * h * w, 2 * 3 * pl.h_pad * pl.w_pad
    fl_f32 = (in_px * 4 + out_px * 4) / HBM_BPS * 1e6
    fl_u8 = (in_px * 1 + out_px * 4) / HBM_BPS * 1e6
    fl_qg = q * 8 / HBM_BPS * 1e6

    def entry(us, all_us, floor, nbytes):
        return {"us": round(us, 2), "blocks_us": [round(x, 2) for x in all_us], "bytes": nbytes, "floor_us": round(floor, 2),
                "x_floor": round(us / floor, 2), "achieved_GBps": round(nbytes / us / 1e3, 1),
                "bound": "launch" if floor < LAUNCH_US else "HBM"}

    return {"shape": f"{h}x{w}x{s}", "batch": 1, "divis_by": DIVIS_BY, "low_res": [pl.h_lr, pl.w_lr], "padded": [pl.h_pad, pl.w_pad],
            "queries": q, "grid_resized": pl.resized,
            "prepare_pair_f32": entry(pp_f32, pp_f32_all, fl_f32, in_px * 4 + out_px * 4),
            "prepare_pair_u8": entry(pp_u8, pp_u8_all, fl_u8, in_px + out_px * 4),
            "query_grid": entry(qg, qg_all, fl_qg, q * 8),
            "device_path_f32_host_us": round(new_host, 1), "device_path_f32_host_blocks_us": [round(x, 1) for x in new_host_all],
            "device_path_u8_host_us": round(new_host_u8, 1),
            "device_path_f32_events_us": round(new_ev, 2), "device_path_f32_events_blocks_us": [round(x, 2) for x in new_ev_all],
            "replaced_images_us": round(old_img, 1), "replaced_images_blocks_us": [round(x, 1) for x in old_img_all],
            "replaced_path_us": round(old, 1), "replaced_path_blocks_us": [round(x, 1) for x in old_all],
            "replaced_path_reps": old_reps,
            "speedup_vs_replaced_path": round(old / new_host, 1),
            "max_dev_images_vs_replaced_path": d_img, "max_dev_grid_vs_replaced_path": d_grid}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--only", default=None, help="run this one shape here, e.g. 375x1242x2.0")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.only:
        h, w, s = a.only.split("x")
        print(json.dumps(run_shape(int(h), int(w), float(s), a.reps, a.blocks)))
        return
    res = {"command": "python tools/kbench_prepare.py", "reps": a.reps, "blocks": a.blocks, "hbm_GBps_assumed": HBM_BPS / 1e9,
           "launch_bound_below_floor_us": LAUNCH_US, "steps": []}
    for h, w, s in SHAPES:
        name = f"{h}x{w}x{s}"
        cmd = [sys.executable, os.path.abspath(__file__), "--only", name, "--reps", str(a.reps), "--blocks", str(a.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res["error"] = f"{name}: no result after {a.step_timeout} s"
            break
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            res["error"] = f"{name}: exit {r.returncode}: {r.stderr[-800:]}"
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
