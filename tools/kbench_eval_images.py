"""The picture kernel (csrc/eval_images.hip) at the KITTI (375x1242), cfg-2 (540x960) and Middlebury-F (1988x2964) output sizes against
its traffic floor and against the paths it replaces.  One JSON object on stdout (and in --out).

    python tools/kbench_eval_images.py [--out profiles/eval_images_kbench.json]
    python tools/kbench_eval_images.py --only images:540x960          # one step, in this process

Steps (each in a child process of its own with a time limit; the parent never opens the GPU and stops at the first failure):
    images:HxW    ops.disparity_images with the colour picture and the error map (what `evaluate(images=...)` issues) and with the
                  16-bit encoding added; device events, median of repeated blocks.  Beside it
                    - the reference's form: `.cpu()` of the prediction, then the plain-torch restatement of Disp_to_color and
                      disp_error_image_func with their quantisation on the host (harness/images.py; the reference itself runs a
                      ten-pass numpy loop and a seven-way broadcast compare there);
                    - the same restatement with torch ops on the device;
                    - the non-blocking copy of the two 8-bit pictures into pinned host memory, which the sink issues per batch.
Floors: 4 B (disp) + 4 B (gt) read and 3 B per picture (2 B for the encoding) written per pixel at 6.3 TB/s: 14 B for colour + error,
16 B for all three.  HBM_BPS, KERNEL_BOUNDARY_US and the timing are those of tools/kbench_eval_metrics.py.  No time here is a pass /
fail criterion."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd"), os.path.join(ROOT, "tools")]

from kbench_eval_metrics import HBM_BPS, KERNEL_BOUNDARY_US, _events, _host  # noqa: E402

SIZES = [(375, 1242), (540, 960), (1988, 2964)]


def _scene(h, w):
    """Ground truth with ~10 % holes and an estimate whose error spans every band."""
    import torch
    from anystereo.harness.synthetic import det_uniform
    gt = det_uniform((1, h, w), 31, -20.0, 180.0)
    est = gt + det_uniform((1, h, w), 32, -1.0, 1.0) * torch.exp(det_uniform((1, h, w), 33, -3.0, 4.0))
    return est.contiguous(), gt.contiguous()


def step_images(h, w, reps, blocks):
    import torch
    from anystereo import ops
    from anystereo.harness import images as I
    dev = "cuda:0"
    est_h, gt_h = _scene(h, w)
    est, gt = est_h.to(dev), gt_h.to(dev)
    px = h * w
    us2, all2 = _events(lambda: ops.disparity_images(est, gt, 192.0), reps, blocks)
    us3, all3 = _events(lambda: ops.disparity_images(est, gt, 192.0, enc16=True), reps, blocks)
    us1, _ = _events(lambda: ops.disparity_images(est, None, 192.0), reps, blocks)

    def restate(e, g):
        return I.quantize_host(I.disp_to_color_host(e, 192.0)), I.quantize_host(I.error_image_host(e, g))

    def old():
        return restate(est.cpu(), gt_h)
    old_us, old_all = _host(old, 1, min(blocks, 3))
    dev_us, dev_all = _events(lambda: restate(est, gt), max(1, reps // 20), blocks)
    c, e, _ = ops.disparity_images(est, gt, 192.0)
    pinned = [torch.empty(t.shape, dtype=torch.uint8, pin_memory=True) for t in (c, e)]

    def copy():
        for p, t in zip(pinned, (c, e)):
            p.copy_(t, non_blocking=True)
    copy_us, _ = _events(copy, max(1, reps // 10), blocks)
    want = old()
    torch.cuda.synchronize()
    same = bool(torch.equal(c.cpu(), want[0]) and torch.equal(e.cpu(), want[1]))
    b2, b3 = 14 * px, 16 * px
    f2, f3 = b2 / HBM_BPS * 1e6, b3 / HBM_BPS * 1e6
    return {"step": f"images:{h}x{w}", "pixels": px,
            "color_error": {"bytes": b2, "traffic_floor_us": round(f2, 2), "kernel_us": round(us2, 2), "blocks_us": [round(x, 2) for x in all2],
                            "x_floor": round(us2 / f2, 2), "achieved_GBps": round(b2 / us2 / 1e3, 1)},
            "color_error_enc16": {"bytes": b3, "traffic_floor_us": round(f3, 2), "kernel_us": round(us3, 2),
                                  "blocks_us": [round(x, 2) for x in all3], "x_floor": round(us3 / f3, 2),
                                  "achieved_GBps": round(b3 / us3 / 1e3, 1)},
            "color_only_us": round(us1, 2),
            "bound": "launch" if f2 < 2 * KERNEL_BOUNDARY_US else "HBM",
            "cpu_copy_plus_host_restatement_us": round(old_us, 1), "old_blocks_us": [round(x, 1) for x in old_all],
            "restatement_with_torch_ops_on_device_us": round(dev_us, 1), "device_restatement_blocks_us": [round(x, 1) for x in dev_all],
            "pinned_copy_of_two_pictures_us": round(copy_us, 1),
            "speedup_vs_cpu_path": round(old_us / us2, 1), "speedup_vs_torch_ops_on_device": round(dev_us / us2, 1),
            "bytes_equal_host_restatement": same}


def run_step(name, reps, blocks):
    import torch
    assert torch.cuda.is_available(), "kbench_eval_images needs a GPU"
    kind, size = name.split(":")
    assert kind == "images", name
    h, w = (int(x) for x in size.split("x"))
    return step_images(h, w, reps, blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--only", default=None, help="run this one step here, e.g. images:540x960")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.only:
        print(json.dumps(run_step(a.only, a.reps, a.blocks)))
        return
    res = {"command": "python tools/kbench_eval_images.py", "reps": a.reps, "blocks": a.blocks, "hbm_GBps_assumed": HBM_BPS / 1e9,
           "kernel_boundary_us_assumed": KERNEL_BOUNDARY_US, "steps": []}
    for s in [f"images:{h}x{w}" for h, w in SIZES]:
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
