"""N `Trainer` steps on fresh procedural scenes (harness/scenes.py) and the end-point error on held-out scenes before and after: the
first run of this training stack on data whose ground truth has something to do with its images.  One JSON line on stdout.

    python tools/train_scenes.py --steps 200                       # 160 x 320, batch 4, 16 GRU iterations, split precision
    python tools/train_scenes.py --steps 20 --height 64 --width 128 --batch 2 --iters 4
    python tools/train_scenes.py --steps 50 --no-supervise-init --eager
    python tools/train_scenes.py --steps 200 --augment flow        # the reference's photometric augmentation and eraser on every pair
    python tools/train_scenes.py --steps 200 --augment flow --spatial flow --frame 540 960    # ... and its rescale / flip / crop / resize

Every step draws `--batch` new scenes (`scene_train_batch`: the pair at the network's size, one hashed scale per sample in
[--scale-min, --scale-max], the ground truth rendered at that scale's size, the queries drawn on the device).  Held-out: 8 scenes
whose indices no training step reaches, queried on the full grid at scales 1.0 and 2.0 (`disparity_at` gives the exact disparity at the
same coordinates, in pixels of the queried width); EPE is the mean absolute error over all queries, `epe_noc` over the non-occluded.
The weights start from the deterministic fill, so "before" is an untrained network.  Whether the error falls is the finding; the line
reports what was measured either way.
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

HELD_OUT_INDEX0 = 1 << 30   # training step t of rank r uses indices (t * world + r) * batch + b: far below


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="continuous_IGEVStereo", choices=["continuous_IGEVStereo", "continuous_RAFTStereo"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--height", type=int, default=160)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--scale-min", type=float, default=1.0)
    ap.add_argument("--scale-max", type=float, default=2.95)
    ap.add_argument("--scene-layers", type=int, default=None, metavar="K")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", default="split", choices=["split", "fp32"])
    ap.add_argument("--no-supervise-init", action="store_true", help="train without the 1/4-resolution loss on init_disp (low_disp)")
    ap.add_argument("--eager", action="store_true", help="no captured step graph")
    ap.add_argument("--held-out", type=int, default=8)
    ap.add_argument("--augment", default=None, choices=["flow", "sparse"],
                    help="photometric augmentation and eraser of every training pair (harness/augment.py: FlowAugmentor's or "
                         "SparseFlowAugmentor's constants); default: none")
    ap.add_argument("--spatial", default=None, choices=["flow", "sparse"],
                    help="spatial augmentation (harness/spatial.py: FlowAugmentorWoCrop's or SparseFlowAugmentorWoCrop's constants): the scenes "
                         "are rendered as --frame frames, rescaled, cropped and resized to --height x --width; default: none")
    ap.add_argument("--frame", type=int, nargs=2, default=None, metavar=("H", "W"), help="the full frame of --spatial; default 540 960")
    ap.add_argument("--eval-iters", type=int, default=None, help="GRU iterations of the held-out queries; default: --iters")
    a = ap.parse_args(argv)
    if a.steps < 1 or a.batch < 1 or a.held_out < 1:
        ap.error("--steps, --batch and --held-out must be positive")
    if a.frame is not None and a.spatial is None:
        ap.error("--frame needs --spatial")
    return a


@torch.no_grad()
def held_out_epe(model, spec, seed, n, h, w, scales, iters, dev):
    """{scale: {"epe", "epe_noc"}} over scenes HELD_OUT_INDEX0 .. + n - 1, one pair at a time; one synchronisation per scale."""
    from anystereo.harness.scenes import disparity_at, render_pair
    from anystereo.nn.liif import make_coord
    was_training = model.training
    model.eval()
    out = {}
    for s in scales:
        hh, wh = round(h * s), round(w * s)
        coord = make_coord([hh, wh]).view(1, -1, 2).to(dev)
        sc = torch.full((1, 1), float(s), device=dev)
        tot = torch.zeros(4, dtype=torch.float64, device=dev)
        for i in range(HELD_OUT_INDEX0, HELD_OUT_INDEX0 + n):
            i1, i2 = render_pair(spec, seed, i, 1, h, w, dev)
            gt, noc = disparity_at(spec, seed, [i], coord, [float(wh)], noc=True)
            pred = model(i1, i2, iters=iters, test_mode=True, hr_coord=coord.clone(), scale=sc)
            err = (pred.view(-1) - gt.view(-1)).abs().double()
            m = noc.view(-1).double()
            tot += torch.stack((err.sum(), torch.tensor(float(err.numel()), dtype=torch.float64, device=dev), (err * m).sum(), m.sum()))
        t = tot.cpu().tolist()
        out[f"{s:g}"] = {"epe": t[0] / t[1], "epe_noc": t[2] / max(t[3], 1.0)}
    if was_training:
        model.train()
    return out


def main():
    a = parse_args()
    from anystereo import _lib, _scenes_lib, ops
    from anystereo.harness.scenes import SceneSpec, scene_train_batch
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer
    from anystereo.models import __models__, default_args

    if not torch.cuda.is_available():
        raise SystemExit("tools/train_scenes.py needs a GPU: the models' hot path has no CPU fallback")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    _lib.load()
    ops.set_precision(a.precision)
    spec = SceneSpec(aspect=a.height / a.width, **({} if a.scene_layers is None else {"n_layers": a.scene_layers})).validate()
    args = default_args(a.model)
    model = __models__[a.model](args)
    fill_module_deterministic(model, base_seed=1)
    model = model.to(dev)
    supervise = not a.no_supervise_init and "IGEV" in a.model
    photo = None
    if a.augment is not None:
        from anystereo.harness.augment import PhotoSpec
        photo = getattr(PhotoSpec, a.augment)()
    spatial = None
    if a.spatial is not None:
        from anystereo.harness.spatial import SpatialSpec
        spatial = SpatialSpec.flow() if a.spatial == "flow" else SpatialSpec.sparse(wo_crop=True)
    eval_iters = a.eval_iters or a.iters
    before = held_out_epe(model, spec, a.seed, a.held_out, a.height, a.width, (1.0, 2.0), eval_iters, dev)
    tr = Trainer(model, lr=a.lr, num_steps=a.steps, train_iters=a.iters, max_disp=args.max_disp, supervise_init=supervise,
                 graph=False if a.eager else None)
    losses = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(a.steps):
        batch = scene_train_batch(spec, a.seed, step, a.batch, a.height, a.width, a.scale_min, a.scale_max,
                                  mode="sparse" if a.spatial == "sparse" else "dense",   # a sparse ground truth: the sparse query draw
                                  device=dev, low_disp=supervise, augment=photo, spatial=spatial, frame_hw=a.frame)
        loss, _ = tr.step(batch)
        losses.append(loss.detach() if torch.is_tensor(loss) else torch.tensor(float(loss)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    losses = [float(v) for v in torch.stack([v.reshape(()).float().cpu() for v in losses])]
    after = held_out_epe(model, spec, a.seed, a.held_out, a.height, a.width, (1.0, 2.0), eval_iters, dev)
    k = max(1, min(10, a.steps // 4))
    print(json.dumps({"tool": "train_scenes", "model": a.model, "steps": a.steps, "size": [a.height, a.width], "batch": a.batch,
                      "iters": a.iters, "eval_iters": eval_iters, "precision": a.precision, "supervise_init": supervise, "lr": a.lr,
                      "graphed_step": bool(tr.use_graph), "scene_layers": spec.n_layers, "augment": a.augment, "spatial": a.spatial, "frame": a.frame,
                      "scales": [a.scale_min, a.scale_max],
                      "weights": "deterministic fill", "loss_first": losses[0], "loss_last": losses[-1],
                      "loss_mean_first_k": sum(losses[:k]) / k, "loss_mean_last_k": sum(losses[-k:]) / k, "k": k,
                      "loss_every_10th": [round(v, 4) for v in losses[::10]], "finite": all(v == v and abs(v) != float("inf") for v in losses),
                      "held_out_scenes": a.held_out, "epe_before": before, "epe_after": after,
                      "epe_fell": {s: after[s]["epe"] < before[s]["epe"] for s in before},
                      "seconds": round(dt, 2), "steps_per_s": round(a.steps / dt, 3),
                      "library": _lib.library_info(), "scenes_library": _scenes_lib.library_info()}))


if __name__ == "__main__":
    main()
