"""The implicit upsampler with 5x5 and 7x7 affinity windows on the GPU: the window kernels (csrc/affinity_window.hip) against the
float64 restatement of liif.py:432-446 and its autograd, the upsampler and the whole models against the reference's outputs
(tests/golden/liif_windows.npz, model_windows.npz; make_golden_windows.py), graph replay and one training step."""
import numpy as np
import pytest
import torch

from _affinity_window import META, affinity_dots, affinity_ref, build_upsampler, close, fixture_inputs, gold

from anystereo.harness.synthetic import det_uniform, fill_module_deterministic, synthetic_pair, tiny_train_case
from anystereo.models.base import default_args
from anystereo.nn import liif as NL

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, C, H, W), win, seed: a map smaller than the window in both axes with odd C and a batch stride; C = 1; the real channel count
# on a map that crosses one 16-pixel tile boundary in each axis; several tiles and batch
FORWARD = [((2, 13, 2, 3), 7, 500), ((1, 1, 9, 20), 5, 501), ((1, 184, 17, 35), 5, 502), ((1, 184, 17, 35), 7, 502),
           ((2, 40, 33, 70), 7, 503)]
_REF = {}


def _case(shape, win, seed):
    """(input, float64 affinity) of a forward case, computed once."""
    key = (shape, win, seed)
    if key not in _REF:
        x = det_uniform(shape, seed)
        _REF[key] = (x, affinity_ref(x, win))
    return _REF[key]


@pytest.mark.parametrize("shape,win,seed", FORWARD, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_forward_matches_float64(shape, win, seed):
    from anystereo import ops
    x, want = _case(shape, win, seed)
    if shape[1] == 1:  # in-map dots are +-1: both sides of the clamp are covered
        dots, inmap = affinity_dots(x, win)
        vals = want[:, inmap]
        assert (vals == 0).double().mean() >= 0.1 and (vals > 0).double().mean() >= 0.1 and (dots[:, inmap] < 0).any()
    xd = x.to(DEV)
    aff = ops.affinity_window(xd, win, False)
    assert tuple(aff.shape) == (shape[0], win * win - 1, shape[2], shape[3])
    close(aff, want, 1e-5, 2e-6, "affinity alone")
    cat = ops.affinity_window(xd, win, True)
    assert torch.equal(cat[:, :shape[1]], xd), "x is copied through"
    close(cat[:, shape[1]:], want, 1e-5, 2e-6, "affinity in cat(x, aff)")
    assert torch.equal(cat[:, shape[1]:], aff)
    _, inmap = affinity_dots(x, win)
    assert (aff.cpu()[:, ~inmap] == 0).all(), "a neighbour outside the map gives exactly 0"


def test_window_3_matches_the_3x3_kernel():
    from anystereo import ops
    x = det_uniform((1, 184, 17, 35), 502).to(DEV)
    want = ops.structure_feature(x)
    got = ops.affinity_window(x, 3, True)
    assert torch.equal(got[:, :184], want[:, :184])
    close(got[:, 184:], want[:, 184:], 1e-5, 2e-6, "window 3 vs structure_feature")
    close(ops.affinity_window(x, 3, False), affinity_ref(x.cpu(), 3), 1e-5, 2e-6, "window 3 vs float64")


@pytest.mark.parametrize("win", [5, 7])
def test_all_zero_pixel(win):
    from anystereo import ops
    x = det_uniform((1, 24, 17, 35), 504)
    py, px = 9, 16  # on a tile boundary
    x[:, :, py, px] = 0
    aff = ops.affinity_window(x.to(DEV), win, False).cpu()
    assert torch.isfinite(aff).all()
    assert (aff[:, :, py, px] == 0).all(), "the zero pixel's own channels"
    r, j = win // 2, 0
    for ky in range(win):
        for kx in range(win):
            if (ky, kx) == (r, r):
                continue
            y, xx = py - (ky - r), px - (kx - r)  # the pixel whose neighbour j is the zero pixel
            assert aff[0, j, y, xx] == 0, (ky, kx)
            j += 1
    close(aff, affinity_ref(x, win), 1e-5, 2e-6, "with a zero pixel")


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("shape,win,seed", [((2, 13, 2, 3), 7, 510), ((1, 24, 17, 35), 5, 510)], ids=["2x13x2x3-7", "1x24x17x35-5"])
def test_backward_matches_float64_autograd(shape, win, seed, with_x):
    from anystereo import grad as G
    x = det_uniform(shape, seed)
    dots, inmap = affinity_dots(x, win)
    assert dots[:, inmap].abs().min().item() > 1e-5, "a dot product next to the clamp: a flipped mask would be a legitimate difference"
    b, c, h, w = shape
    g = det_uniform((b, (c if with_x else 0) + win * win - 1, h, w), seed + 1)
    xr = x.double().requires_grad_(True)
    (affinity_ref(xr, win, with_x) * g.double()).sum().backward()
    runs = []
    for _ in range(2):
        xd = x.to(DEV).requires_grad_(True)
        out = G.StructureFeatureLive.apply(xd, with_x, win)
        (out * g.to(DEV)).sum().backward()
        runs.append(xd.grad.clone())
    close(out, affinity_ref(x, win, with_x), 1e-5, 2e-6, "forward under autograd")
    ref = xr.grad
    err = (runs[0].double().cpu() - ref).abs().max().item()
    lim = 2e-4 * max(1.0, ref.abs().max().item())
    print(f"dx: max abs err {err:.3e} (limit {lim:.3e}, |ref|max {ref.abs().max().item():.3e})")
    assert err <= lim
    assert torch.equal(runs[0], runs[1])


def test_detached_structure_feature_backward_is_the_slice():
    from anystereo import grad as G
    x = det_uniform((1, 24, 5, 7), 520).to(DEV).requires_grad_(True)
    g = det_uniform((1, 48, 5, 7), 521).to(DEV)
    (G.StructureFeature.apply(x, 5) * g).sum().backward()
    assert torch.equal(x.grad, g[:, :24])


# ---- the upsampler against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_upsampler_matches_reference_fixture(name):
    from anystereo import ops
    g = gold()
    ent = META["cases"][name]
    up = build_upsampler(ent["win"], ent["win"], ent["mode"], DEV)
    feats, _ = fixture_inputs(DEV)
    coord = torch.from_numpy(g["coord"]).to(DEV)
    with torch.no_grad():
        close(NL.AffinityFeature(ent["win"], ent["win"], 1, 0)(feats[0]), torch.from_numpy(g[f"{name}__aff"]), 1e-5, 2e-6, "affinity")
        mask = up(feats, coord.clone(), torch.tensor([[1.5]], device=DEV))
        conv = ops.convex_upsample(torch.from_numpy(g["dlow"]).to(DEV), mask.contiguous(), coord.clone(),
                                   scale=torch.tensor([1.5], device=DEV), mask_is_logits=True)
    ref = g[f"{name}__mask"]
    assert tuple(mask.shape) == ref.shape
    e_mask = np.abs(mask.cpu().numpy() - ref).max()
    e_conv = np.abs(conv[:, 0].cpu().numpy() - g[f"{name}__convex"]).max()
    print(f"{name}: logits err {e_mask:.3e} (limit {5e-5 * max(1.0, np.abs(ref).max()):.3e}), convex err {e_conv:.3e} (limit 3e-3)")
    assert e_mask <= 5e-5 * max(1.0, np.abs(ref).max())
    assert e_conv <= 3e-3


@pytest.mark.parametrize("mode", ["with_v2ISU", "with_ISU"])
def test_upsampler_gradients_match_reference_fixture(mode):
    """Window 5, batch 2, loss = sum(upsampled disparity * w): the gradients of every parameter and of both inputs."""
    from anystereo import grad as G
    g = gold()
    up = build_upsampler(5, 5, mode, DEV)
    for p_ in up.parameters():
        p_.requires_grad_(True)
    feats = [f.requires_grad_(True) for f in fixture_inputs(DEV, batch=2)[0]]
    coord = torch.from_numpy(g["coord"]).to(DEV).repeat(2, 1, 1)
    d = det_uniform((2, 1, 4, 6), 83, 0, 20).to(DEV)
    mask = up(feats, coord.clone(), torch.tensor([[1.5], [1.5]], device=DEV)).contiguous()
    out = G.ConvexUpsample.apply(d, mask, coord.clone().clamp(-1 + 1e-6, 1 - 1e-6), torch.tensor([1.5, 1.5], device=DEV), True)
    wq = det_uniform((2, coord.shape[1]), 91, -1.0, 1.0).to(DEV)
    (out[:, 0] * wq).sum().backward()
    pre = f"grad_w5_{mode}__"
    assert np.abs(out[:, 0].detach().cpu().numpy() - g[pre + "convex"]).max() <= 3e-3
    got = {"p." + k: p_.grad for k, p_ in up.named_parameters()}
    got["in0"], got["in1"] = feats[0].grad, feats[1].grad
    assert sorted(pre + k for k in got) == sorted(k for k in g.files if k.startswith(pre) and not k.endswith("__convex"))
    worst = []
    for k, t in got.items():
        ref = g[pre + k]
        assert t is not None and tuple(t.shape) == ref.shape, k
        err, lim = np.abs(t.cpu().numpy() - ref).max(), 2e-4 * max(1.0, np.abs(ref).max())
        print(f"{mode} {k}: err {err:.3e} limit {lim:.3e}")
        if err > lim:
            worst.append((k, float(err), float(lim)))
    assert not worst, worst


# ---- whole models -------------------------------------------------------------------------------------------------------------
def _model(name):
    from anystereo.models import __models__
    mname, (H, W), opt = META["models"][name]
    model = __models__[mname](default_args(mname, **opt)).eval()
    fill_module_deterministic(model, base_seed=1)
    img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
    coord = NL.make_coord([round(H * 1.5), round(W * 1.5)]).unsqueeze(0).to(DEV)
    return model.to(DEV), img1.to(DEV), img2.to(DEV), coord, torch.tensor([[1.5]], device=DEV)


@pytest.mark.parametrize("precision", ["split", "fp32"])
@pytest.mark.parametrize("name", sorted(META["models"]))
def test_models_match_reference(name, precision):
    from anystereo import ops
    ops.set_precision(precision)
    try:
        model, img1, img2, coord, scale = _model(name)
        with torch.no_grad():
            out = model(img1, img2, iters=2, test_mode=True, hr_coord=coord.clone(), scale=scale)
    finally:
        ops.set_precision("split")
    ref = gold("model_windows")[name]
    assert tuple(out.shape) == ref.shape
    err = np.abs(out.cpu().numpy() - ref)
    print(f"{name} {precision}: mean {err.mean():.3e} max {err.max():.3e}")
    assert err.mean() <= 2e-3 and err.max() <= 5e-2, (float(err.mean()), float(err.max()))


def test_model_graph_replay_equals_eager():
    model, img1, img2, coord, scale = _model("igev_w5")
    with torch.no_grad():
        eager = model(img1, img2, iters=2, test_mode=True, hr_coord=coord.clone(), scale=scale)
        model.enable_graph(True)
        g1 = model(img1, img2, iters=2, test_mode=True, hr_coord=coord.clone(), scale=scale)
        g2 = model(img1, img2, iters=2, test_mode=True, hr_coord=coord.clone(), scale=scale)
    assert torch.equal(g1, g2)
    assert (g1 - eager).abs().max().item() <= 1e-4


def test_training_step_gives_finite_upsampler_gradients():
    from anystereo.harness.train import Trainer
    from anystereo.models import __models__
    model = __models__["continuous_IGEVStereo"](default_args("continuous_IGEVStereo", lsp_width=5, lsp_height=5))
    fill_module_deterministic(model, base_seed=1)
    trainer = Trainer(model.to(DEV))
    _, _, img1, img2, coord, gt, scale = tiny_train_case("igev")
    loss, _ = trainer.step(tuple(t.to(DEV) for t in (img1, img2, coord, gt, scale)))
    assert torch.isfinite(torch.as_tensor(loss)).all()
    params = dict(trainer.model.liif_up.named_parameters())
    assert params and params["imnet.layers.0.weight"].shape[1] == 260
    for k, p_ in params.items():
        assert p_.grad is not None and torch.isfinite(p_.grad).all(), k
