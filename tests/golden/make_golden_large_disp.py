"""Golden vectors of the whole IGEV model at disparity ranges above 256 (geometry volumes of D = max_disp / 4 > 64), generated
by IMPORTING THE REFERENCE (read-only) exactly as make_golden.py does, whose helpers this script reuses.

    python tests/golden/make_golden_large_disp.py            # needs the reference checkout; writes model_igev_large_disp.npz
    python tests/golden/make_golden_large_disp.py --check    # exit 1 unless regenerating reproduces the stored arrays bit for bit

model_igev_large_disp.npz   the reference continuous_IGEVStereo (deterministic fill, base_seed 1) in test mode, iters = 3:
  shape A  max_disp = 384 (D = 96), image 64 x 512: the quarter-resolution map is 16 x 128, wider than D, so every disparity chunk
           of the volume holds real products; synthetic_pair(shift=300) is a shift of 75 quarter-resolution pixels, beyond d = 64.  Outputs at scales
           1.0 and 1.5 and init_disp.
  shape B  max_disp = 768 (D = 192), image 64 x 128: W/4 = 32 < D, most of the volume is zeros.  Scale 1.0 and init_disp.
Per shape also, as every STRIDE-th element plus fp64 sums (the layout of preloop_igev.npz, tests/_preloop.py::check_preloop):
  <tag>.gev     the geometry encoding volume [1,8,D,h,w] (cost_agg's output),
  <tag>.gwc_hi  the disparities d >= 64 of the reference's own build_gwc_volume on its matching features.
The outputs alone do not pin the volume beyond d = 64: with the deterministic fill the regression's softmax is nearly uniform
(init_disp = (D-1)/2 +- 0.02), and zeroing d >= 64 of the oracle's gwc volume moves shape A's output by a mean of 6.3e-4 px and
its init_disp by 4.5e-4, both under the 1e-3 bar, and shape B's not at all (W/4 = 32: those disparities are zeros anyway).  The
same cut moves A.gev by 4.9e-2 of its maximum, about 100 times the 5e-4 that check_preloop allows the GPU path
(tests/test_large_disp_cpu.py asserts an order of magnitude).
Only the reference's OUTPUTS are stored (the inputs are regenerated from their seeds).  Every value is deterministic.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (its module level only sets paths and imports the package)
from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair  # noqa: E402
from anystereo.models.base import default_args  # noqa: E402

NAME = "model_igev_large_disp"
ITERS = 3
STRIDE = 61  # every 61st element of the flattened volumes (coprime to every map width used)
# tag -> (max_disp, H, W, shift, seed, scales)
SHAPES = {"A": (384, 64, 512, 300, 99, (1.0, 1.5)), "B": (768, 64, 128, 6, 99, (1.0,))}


def key(s):
    return str(s).replace(".", "p")


def generate():
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    MG.import_reference()
    import models.coreContinuous_IGEV.liif as rliif
    import models.coreContinuous_IGEV.submodule as rsub
    from models.coreContinuous_IGEV.continuous_IGEVstereo import continuous_IGEVStereo as RefIGEV
    outs = {}
    for tag, (max_disp, H, W, shift, seed, scales) in SHAPES.items():
        model = RefIGEV(default_args("continuous_IGEVStereo", max_disp=max_disp)).eval()
        fill_module_deterministic(model, base_seed=1)
        img1, img2 = synthetic_pair(1, H, W, shift=shift, seed=seed)
        for s in scales:
            coord = rliif.make_coord([round(H * s), round(W * s)]).unsqueeze(0)
            outs[f"{tag}_test_{key(s)}"] = model(img1, img2, iters=ITERS, test_mode=True, hr_coord=coord.clone(), scale=torch.tensor([[s]]))
        coord = rliif.make_coord([H, W]).unsqueeze(0)
        cap = {"desc": []}
        hooks = [model.desc.register_forward_hook(lambda m, i, o: cap["desc"].append(o.detach().clone())),
                 model.cost_agg.register_forward_hook(lambda m, i, o: cap.__setitem__("gev", o.detach().clone()))]
        init_disp, _ = model(img1, img2, iters=1, test_mode=False, hr_coord=coord.clone(), scale=torch.tensor([[1.0]]))
        for h_ in hooks:
            h_.remove()
        assert len(cap["desc"]) == 2
        gwc = rsub.build_gwc_volume(cap["desc"][0], cap["desc"][1], max_disp // 4, 8)
        for n, t in (("gev", cap["gev"]), ("gwc_hi", gwc[:, :, 64:].contiguous())):
            flat = t.reshape(-1)
            outs[f"{tag}.{n}"] = flat[::STRIDE].clone()
            outs[f"{tag}.{n}.shape"] = np.array(t.shape)
            outs[f"{tag}.{n}.sums"] = np.array([float(flat.double().sum()), float(flat.double().abs().sum())])
        outs[f"{tag}_init_disp"] = init_disp
        outs[f"{tag}_case"] = np.array([max_disp, H, W, shift, seed])
        print(tag, "max_disp", max_disp, "init_disp range", float(init_disp.min()), float(init_disp.max()),
              "share of init_disp beyond 64:", float((init_disp > 64).float().mean()))
    outs["stride"] = STRIDE
    return {k: (MG.npy(v) if torch.is_tensor(v) else np.asarray(v)) for k, v in outs.items()}


def main(argv):
    arrs = generate()
    path = os.path.join(HERE, NAME + ".npz")
    if "--check" in argv:
        old = np.load(path)
        bad = [k for k in sorted(set(old.files) | set(arrs)) if k not in old.files or k not in arrs or old[k].dtype != arrs[k].dtype
               or not np.array_equal(old[k], arrs[k])]
        print(f"{NAME}.npz: {len(arrs) - len(bad)} of {len(arrs)} arrays bit-equal" + (f"; differing: {bad}" if bad else ""))
        return 1 if bad else 0
    MG.save(NAME, **arrs)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
