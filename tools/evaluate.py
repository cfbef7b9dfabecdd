"""The evaluation protocol (anystereo/harness/evaluate.py) over synthetic pairs whose ground truth is known: `synthetic_pair(shift=k)`
has disparity k everywhere, so the right view's ground truth is k as well.  One JSON line on stdout (rank 0).

    python tools/evaluate.py --pairs 8 --height 256 --width 512 --scale 1.5 --iters 8 --protocol things
    python tools/evaluate.py --pairs 4 --prep host                  # down-scale / pad / query grid with torch ops and a host-built grid
    python tools/evaluate.py --pairs 4 --uint8                      # 8-bit images as a loader delivers them (--prep device only)
    python -m torch.distributed.run --nproc-per-node 2 tools/evaluate.py --pairs 8       # pairs sharded over the ranks
    python tools/evaluate.py --pairs 2 --model-max-disp 256         # the model built for disparities up to 256 (volume of D = 64, the
                                                                    # largest as_gwc_volume_fwd serves; above it the library's error)
    python tools/evaluate.py --pairs 2 --lsp-window 5               # the upsampler built with a 5x5 affinity window (3, 5 or 7)
    python tools/evaluate.py --pairs 2 --save-images out/           # disp_{i}.png (colour map) and error_{i}.png per pair; --enc16 adds
                                                                    # the 16-bit disp16_{i}.png, --image-limit N stops after N pairs
    python tools/evaluate.py --pairs 4 --iters 32 --curve 4,8,16,32 # accuracy per GRU iteration from ONE loop per pair (model.encode +
                                                                    # one field query per entry); the metrics become lists in that order
    python tools/evaluate.py --pairs 4 --baseline bicubic           # plus the reference's interpolation baseline (multi_evaothers): this
                                                                    # model's own scale-1 output, un-padded, times scale, bicubic resize
    python tools/evaluate.py --pairs 8 --scenes --scene-layers 6    # procedural scenes (harness/scenes.py) instead of the rolled image: a
                                                                    # non-constant ground truth, a right-view ground truth that differs from
                                                                    # it and a non-empty occluded region, all made on the device

The weights are the deterministic fill, so EPE here says nothing about a trained model: the
line shows that the protocol runs on the device, what it counts and how fast.  No dataset readers.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

import torch  # noqa: E402


def model_args(a):
    """The model's construction arguments for the parsed command line `a`: default_args, with --model-max-disp as max_disp and
    --lsp-window as lsp_width = lsp_height."""
    from anystereo.models import default_args
    over = {} if a.model_max_disp is None else {"max_disp": a.model_max_disp}
    if a.lsp_window is not None:
        over.update(lsp_width=a.lsp_window, lsp_height=a.lsp_window)
    return default_args(a.model, **over)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="continuous_IGEVStereo", choices=["continuous_IGEVStereo", "continuous_RAFTStereo"])
    ap.add_argument("--protocol", default="things", choices=["things", "kitti", "middlebury", "eth3d"])
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--height", type=int, default=128)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--shift", type=int, default=6)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--max-disp", type=float, default=None, help="the evaluator's: additionally count only gt < this value")
    ap.add_argument("--model-max-disp", type=int, default=None, metavar="N",
                    help="the model's disparity range (IGEV: the geometry volume holds N/4 disparities; a multiple of 32, at most 256 today); "
                         "default: default_args' value")
    ap.add_argument("--lsp-window", type=int, default=None, metavar="N", choices=[3, 5, 7],
                    help="the upsampler's affinity window, lsp_width = lsp_height = N (3, 5 or 7; 5 and 7 take the staged upsampler); "
                         "default: default_args' 3")
    ap.add_argument("--prep", default="device", choices=["host", "device"],
                    help="device: as_prepare_pair + as_query_grid (two launches); host: query.pad_for_multi_train + upload of the grid")
    ap.add_argument("--uint8", action="store_true", help="feed the images as uint8 (rounded); needs --prep device")
    ap.add_argument("--save-images", default=None, metavar="DIR",
                    help="write the colourised disparity and the error map of every pair as PNG files (harness/images.py); with several "
                         "ranks each writes into DIR/rank<r>")
    ap.add_argument("--image-limit", type=int, default=None, help="stop writing pictures after this many pairs (per rank)")
    ap.add_argument("--enc16", action="store_true", help="with --save-images: also the 16-bit disparity PNG (disparity * 256)")
    ap.add_argument("--curve", default=None, metavar="K1,K2,...",
                    help="evaluate these GRU iterations (1-based, ascending, each at most --iters) from one encoded pass per pair")
    ap.add_argument("--baseline", default=None, choices=["bicubic"],
                    help="also evaluate the interpolation baseline: the scale-1 query of the same pass resized bicubically")
    ap.add_argument("--scenes", action="store_true",
                    help="evaluate on procedural scenes (harness/scenes.py: pair, ground truth, right-view ground truth / exact occlusion "
                         "mask made on the device) instead of the rolled synthetic pair; --shift is then unused")
    ap.add_argument("--scene-layers", type=int, default=None, metavar="K",
                    help="with --scenes: the layers of a scene, the background included (1..8); default: SceneSpec's 6")
    a = ap.parse_args(argv)
    if a.scene_layers is not None and not a.scenes:
        ap.error("--scene-layers needs --scenes")
    if a.scene_layers is not None and not 1 <= a.scene_layers <= 8:
        ap.error(f"--scene-layers {a.scene_layers}: 1..8 expected")
    if a.scenes and a.uint8:
        ap.error("--scenes renders float images: --uint8 is for the rolled pair")
    if a.curve is not None:
        try:
            a.curve = tuple(int(k) for k in a.curve.split(","))
        except ValueError:
            ap.error(f"--curve takes comma-separated integers, got {a.curve!r}")
        if any(k < 1 or k > a.iters for k in a.curve) or list(a.curve) != sorted(set(a.curve)):
            ap.error(f"--curve {a.curve}: ascending distinct GRU iterations in [1, --iters = {a.iters}] expected")
    return a


def _scene_info(a):
    """What --scenes adds to the result line (without it the line is as it always was)."""
    from anystereo import _scenes_lib
    from anystereo.harness.scenes import SceneSpec
    return {"data": "scenes", "scene_layers": a.scene_layers or SceneSpec().n_layers, "gt_disparity": None,
            "scenes_library": _scenes_lib.library_info()}


def main():
    a = parse_args()

    from anystereo import _lib
    from anystereo.harness import dist
    from anystereo.harness.evaluate import Evaluator, evaluate
    from anystereo.harness.images import ImageSink
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__

    if not torch.cuda.is_available():
        raise SystemExit("tools/evaluate.py needs a GPU: the models' hot path has no CPU fallback")
    if a.uint8 and a.prep != "device":
        raise SystemExit("--uint8 needs --prep device: the host path takes float images")
    rank, world, local = dist.env_rank()
    dev = torch.device("cuda", local % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    dist.init("gloo")  # the only traffic is the merge of the per-image rows: a few KB from host memory
    _lib.load()

    args = model_args(a)
    model = __models__[a.model](args).eval()
    fill_module_deterministic(model, base_seed=1)
    model = model.to(dev)

    def scene_pairs():
        from anystereo.harness.scenes import SceneSpec, scene_pairs as one_scene
        spec = SceneSpec(aspect=a.height / a.width, **({} if a.scene_layers is None else {"n_layers": a.scene_layers})).validate()
        for i in dist.shard_indices(a.pairs, rank, world):
            yield from one_scene(spec, 1000, 1, a.height, a.width, protocol=a.protocol, device=dev, index0=i)

    def pairs():
        if a.scenes:
            yield from scene_pairs()
            return
        for i in dist.shard_indices(a.pairs, rank, world):
            i1, i2 = synthetic_pair(1, a.height, a.width, shift=a.shift, seed=1000 + i)
            if a.uint8:
                i1, i2 = i1.round().to(torch.uint8), i2.round().to(torch.uint8)
            gt = torch.full((1, a.height, a.width), float(a.shift), device=dev)
            valid = torch.ones((1, a.height, a.width), device=dev)
            extra = gt.clone() if a.protocol == "things" else torch.ones((1, a.height, a.width), dtype=torch.uint8, device=dev)
            yield i1.to(dev), i2.to(dev), gt, valid, extra

    divis_by = 32 if "IGEV" in a.model else 16
    evaluate(model, list(pairs())[:1], scale=a.scale, iters=a.iters, protocol=a.protocol, divis_by=divis_by,
             prep=a.prep, curve=a.curve, baseline=a.baseline)  # warm-up, not counted
    ev = Evaluator(a.protocol, max_disp=a.max_disp)
    sink = None
    if a.save_images:
        sink = ImageSink(a.save_images if world == 1 else os.path.join(a.save_images, f"rank{rank}"), enc16=a.enc16, limit=a.image_limit)
    res = evaluate(model, pairs(), scale=a.scale, iters=a.iters, protocol=a.protocol, evaluator=ev, divis_by=divis_by, prep=a.prep,
                   images=sink, curve=a.curve, baseline=a.baseline)
    local_rate, local_pairs = res["pairs_per_s"], res["pairs"]
    written = [0.0] * world
    written[rank] = float(res.get("images_written", 0))
    if world > 1:
        ev.merge()
        merged = ev.result()
        rates = [0.0] * world
        rates[rank] = local_rate
        rates = dist.sum_over_ranks(rates)
        written = dist.sum_over_ranks(written)
    else:
        merged, rates = {k: res[k] for k in ("all", "noc", "occ", "images")}, [local_rate]
    if "estimates" in res:
        merged["estimates"] = res["estimates"]
    dist.finalize()
    if rank == 0:
        print(json.dumps({"tool": "evaluate", "model": a.model, "protocol": a.protocol, "n_gpus": world, "pairs": a.pairs,
                          "size": [a.height, a.width], "scale": a.scale, "prep": a.prep,
                          "image_dtype": "uint8" if a.uint8 else "float32", "iters": a.iters, "gt_disparity": a.shift,
                          "weights": "deterministic fill", "model_max_disp": args.max_disp, "lsp_window": [args.lsp_height, args.lsp_width], "pairs_per_s": round(sum(rates), 3),
                          "per_rank_pairs_per_s": [round(r, 3) for r in rates], "rank0_pairs": local_pairs,
                          "library": _lib.library_info(), **(_scene_info(a) if a.scenes else {}), **({"images_written": int(sum(written))} if sink is not None else {}),
                          **merged}))


if __name__ == "__main__":
    main()
