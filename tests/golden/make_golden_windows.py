"""The implicit upsampler with 5x5 and 7x7 affinity windows (--lsp_width / --lsp_height; liif.py:417-446, :448-572, :575-678),
captured from the IMPORTED reference like make_golden_variants.py (same shims, same generators, read-only).

    python tests/golden/make_golden_windows.py            # needs the reference checkout; writes the three files below
    python tests/golden/make_golden_windows.py --check    # exit 1 unless regenerating reproduces them bit for bit

liif_windows.npz / liif_windows.json
  Upsampler, inputs [176 @ 4x6, 32 @ 8x12], coord = make_coord([24, 36]) with the two boundary queries of the variants fixture,
  scale 1.5, windows 5 and 7 times 'with_v2ISU', 'with_ISU', 'with_1_4ISU', 'only_ISU':
    w<win>_<mode>__aff     AffinityFeature(win, win) on the first input [1, win*win-1, 4, 6]
    w<win>_<mode>__mask    the mask logits [1, 9, Q];  __convex  the convex-upsampled disparity [1, Q]
  and in the json the state-dict shapes and `in_dim` of every case, and for the windows the reference cannot run (3x5, 5x3,
  'with_embed_ISU' at 5) the exception type and the first line of its message.
  Under autograd, window 5, 'with_v2ISU' and 'with_ISU', batch 2, loss = sum(upsampled disparity * det_uniform weight):
    grad_w5_<mode>__p.<parameter>   the gradient of every parameter;  __in0 / __in1  of both inputs.
model_windows.npz
  Whole models, 2 iterations, test mode, scale 1.5: IGEV 64x128 with lsp_width = lsp_height = 5 and 7; RAFT 64x96 with
  lsp_width = 5, lsp_height = 3 (prune_raft_stereo.py:184-185 takes both sides from lsp_width: a 5x5 model).  The json holds their
  options and the shapes of their `liif_up.` state-dict entries.
Beside the reference's OUTPUTS only `coord` and `dlow` are stored; the other inputs are regenerated from their seeds.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, npy  # noqa: E402
from anystereo.harness.synthetic import det_uniform, fill_module_deterministic, synthetic_pair  # noqa: E402
from anystereo.models.base import default_args  # noqa: E402

WINDOWS = (5, 7)
MODES = ("with_v2ISU", "with_ISU", "with_1_4ISU", "only_ISU")
GRAD_MODES = ("with_v2ISU", "with_ISU")
# (win_h, win_w, mode) the reference fails on
DEAD = {"w3x5_with_v2ISU": (3, 5, "with_v2ISU"), "w5x3_with_v2ISU": (5, 3, "with_v2ISU"), "w5_with_embed_ISU": (5, 5, "with_embed_ISU")}
MODELS = {
    "igev_w5": ("continuous_IGEVStereo", (64, 128), dict(lsp_width=5, lsp_height=5)),
    "igev_w7": ("continuous_IGEVStereo", (64, 128), dict(lsp_width=7, lsp_height=7)),
    "raft_w5_h3": ("continuous_RAFTStereo", (64, 96), dict(lsp_width=5, lsp_height=3)),
}


def inputs(batch=1):
    return [det_uniform((batch, 176, 4, 6), 81), det_uniform((batch, 32, 8, 12), 82)], [176, 32]


def build(rliif, win_h, win_w, mode):
    _, chans = inputs()
    aff = {"win_w": win_w, "win_h": win_h, "dilation": [1, 2, 4, 8]}
    up = rliif.liif_out_multi_scale_Training(encoder_dim=sum(chans), mlphidden_list=[128, 64, 64], pos_dim=0, affinity_settings=aff,
                                             number_input=2, chanels=chans, unfold=mode).eval()
    fill_module_deterministic(up, base_seed=7, gain=2.0)
    return up


def _err(e):
    return {"ok": False, "error": type(e).__name__, "message": (str(e).splitlines() or [""])[0][:160]}


def generate():
    torch.manual_seed(0)
    import_reference()
    import models.coreContinuous_IGEV.liif as rliif
    import models.coreContinuous_IGEV.submodule as rsub
    from models.coreContinuous_IGEV.continuous_IGEVstereo import continuous_IGEVStereo as RefIGEV
    from models.corePrune_RAFT.prune_raft_stereo import continuous_RaftStereo as RefRAFT
    arrs, meta, models = {}, {"cases": {}, "dead": {}, "models": {}, "model_state_dict": {}}, {}
    coord = rliif.make_coord([24, 36]).unsqueeze(0)  # scale 1.5 over the 16x24 full-resolution grid
    coord[:, 0] = torch.tensor([-1.0, 1.0])          # on the clamp boundary
    coord[:, 5] = torch.tensor([0.999, -0.999])
    dlow = det_uniform((1, 1, 4, 6), 83, 0, 20)
    arrs["coord"], arrs["dlow"] = npy(coord), npy(dlow)
    scale = torch.tensor([[1.5]])
    with torch.no_grad():
        for win in WINDOWS:
            for mode in MODES:
                name = f"w{win}_{mode}"
                feats, _ = inputs()
                up = build(rliif, win, win, mode)
                mask = up([f.clone() for f in feats], coord.clone(), scale)
                conv = rsub.context_upsample_multiscale_train(dlow * 4.0 * 1.5, torch.softmax(mask, dim=1), coord.clone())
                arrs[f"{name}__aff"] = npy(rliif.AffinityFeature(win, win, 1, 0)(feats[0].clone()))
                arrs[f"{name}__mask"], arrs[f"{name}__convex"] = npy(mask), npy(conv)
                meta["cases"][name] = {"win": win, "mode": mode, "in_dim": int(up.imnet.layers[0].weight.shape[1]),
                                       "state_dict": {k: list(v.shape) for k, v in up.state_dict().items()}}
                print(name, "ok", meta["cases"][name]["in_dim"])
        for name, (wh, ww, mode) in DEAD.items():
            try:
                up = build(rliif, wh, ww, mode)
                ent = {"win_h": wh, "win_w": ww, "mode": mode, "in_dim": int(up.imnet.layers[0].weight.shape[1]),
                       "state_dict": {k: list(v.shape) for k, v in up.state_dict().items()}}
                up([f.clone() for f in inputs()[0]], coord.clone(), scale)
                ent["ok"] = True
            except Exception as e:  # the reference cannot run this window
                ent.update(_err(e))
            meta["dead"][name] = ent
            print(name, ent.get("error"), ent.get("message"))
    # autograd: batch 2
    for mode in GRAD_MODES:
        feats, _ = inputs(2)
        feats = [f.clone().requires_grad_(True) for f in feats]
        up = build(rliif, 5, 5, mode)
        for p_ in up.parameters():
            p_.requires_grad_(True)
        c2 = coord.repeat(2, 1, 1)
        d2 = det_uniform((2, 1, 4, 6), 83, 0, 20)
        mask = up(feats, c2.clone(), torch.tensor([[1.5], [1.5]]))
        conv = rsub.context_upsample_multiscale_train(d2 * 4.0 * 1.5, torch.softmax(mask, dim=1), c2.clone())
        wq = det_uniform(tuple(conv.shape), 91, -1.0, 1.0)
        (conv * wq).sum().backward()
        arrs[f"grad_w5_{mode}__convex"] = npy(conv)
        for k, p_ in up.named_parameters():
            arrs[f"grad_w5_{mode}__p.{k}"] = npy(p_.grad)
        arrs[f"grad_w5_{mode}__in0"], arrs[f"grad_w5_{mode}__in1"] = npy(feats[0].grad), npy(feats[1].grad)
        print("grad", mode, "ok", tuple(conv.shape))
    with torch.no_grad():
        for name, (mname, (H, W), opt) in MODELS.items():
            model = (RefIGEV if "IGEV" in mname else RefRAFT)(default_args(mname, **opt)).eval()
            fill_module_deterministic(model, base_seed=1)
            img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
            hr = rliif.make_coord([round(H * 1.5), round(W * 1.5)]).unsqueeze(0)
            out = model(img1, img2, iters=2, test_mode=True, hr_coord=hr.clone(), scale=torch.tensor([[1.5]]))
            models[name] = npy(out)
            meta["models"][name] = [mname, [H, W], opt]
            meta["model_state_dict"][name] = {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith("liif_up.")}
            print("model", name, "ok", tuple(out.shape), float(out.min()), float(out.max()))
    return arrs, models, json.dumps(meta, indent=1, sort_keys=True) + "\n"


def _same(path, arrs):
    old = np.load(path)
    return [k for k in sorted(set(old.files) | set(arrs)) if k not in old.files or k not in arrs or old[k].dtype != arrs[k].dtype
            or not np.array_equal(old[k], arrs[k])]


def main(argv):
    arrs, models, meta = generate()
    paths = [os.path.join(HERE, n) for n in ("liif_windows.npz", "model_windows.npz", "liif_windows.json")]
    if "--check" in argv:
        bad = _same(paths[0], arrs) + _same(paths[1], models) + ([] if open(paths[2]).read() == meta else ["liif_windows.json"])
        n = len(arrs) + len(models) + 1
        print(f"liif_windows / model_windows: {n - len(bad)} of {n} entries bit-equal" + (f"; differing: {bad}" if bad else ""))
        return 1 if bad else 0
    np.savez_compressed(paths[0], **arrs)
    np.savez_compressed(paths[1], **models)
    with open(paths[2], "w") as f:
        f.write(meta)
    for p_ in paths:
        print("wrote %s (%.1f KiB)" % (os.path.basename(p_), os.path.getsize(p_) / 1024))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
