"""GPU (-m gpu): the init-disparity head's fused backward (csrc/init_head.hip, grad.InitDispHead) and the --supervise_init training
branch that needs it (train_continuous_IGEV.py:96-122, :220-221).

  * the kernel against fp64 autograd of conv3d -> softmax -> regression on the CPU, bit-repeatable, argument checks
  * InitDispHead's forward is the composition it replaces, bit for bit
  * the G8 step with the supervise_init loss against the imported reference (tests/golden/train_igev_superinit*.npz)
  * deterministic mode: two steps, bit-equal gradients
  * the Trainer's graphed step with 6-tuple batches against its eager step
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_hip_parity import G8_ZERO_GOT, G8_ZERO_REF, _g8_limits, close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def U(shape, seed, lo=-1.0, hi=1.0):
    from anystereo.harness.synthetic import det_uniform
    return det_uniform(shape, seed, lo, hi)


def _head_case(b, d, h, w, seed=0):
    geo = U((b, 8, d, h, w), 900 + seed)
    wt = U((1, 8, 3, 3, 3), 901 + seed) * (3.0 / 216) ** 0.5 * 2.0
    g = U((b, h, w), 902 + seed)
    g = torch.where(U((b, h, w), 903 + seed, 0.0, 1.0) < 0.2, torch.zeros(()), g)  # masked pixels: no gradient
    return geo, wt, g


def _fp64_reference(geo, wt, g):
    x = geo.double().requires_grad_(True)
    w = wt.double().requires_grad_(True)
    cost = torch.nn.functional.conv3d(x, w, padding=1).squeeze(1)
    d = cost.shape[1]
    init = (torch.softmax(cost, 1) * torch.arange(d, dtype=torch.float64).view(1, d, 1, 1)).sum(1)
    (init * g.double()).sum().backward()
    return cost.detach(), x.grad, w.grad


@pytest.mark.parametrize("b,d,h,w", [(2, 48, 16, 32), (1, 48, 17, 33), (4, 48, 40, 80), (1, 12, 9, 20), (1, 128, 8, 16)])
def test_init_head_bwd_vs_fp64_autograd(b, d, h, w):
    from anystereo import ops
    geo, wt, g = _head_case(b, d, h, w)
    cost64, dx, dw = _fp64_reference(geo, wt, g)
    args = (geo.to(DEV), wt.to(DEV), cost64.float().contiguous().to(DEV), g.to(DEV))
    d_geo, d_w = ops.init_head_bwd(*args)
    d_geo2, d_w2 = ops.init_head_bwd(*args)
    torch.cuda.synchronize()
    for got, want, what in ((d_geo, dx, "d_geo"), (d_w, dw, "d_weight")):
        got = got.double().cpu()
        assert got.shape == want.shape and torch.isfinite(got).all(), what
        err = ((got - want).abs().max() / want.abs().max()).item()
        print(f"[init_head_bwd {b}x{d}x{h}x{w}] {what}: max |d| / max |ref| = {err:.2e}")
        assert err <= 1e-5, (what, err)
    assert torch.equal(d_geo, d_geo2) and torch.equal(d_w, d_w2), "two launches differ"


def test_init_head_bwd_rejects_bad_arguments():
    from anystereo import _lib
    lib = _lib.load()
    t = torch.zeros(8 * 4 * 4 * 16, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    part = torch.zeros(int(lib.as_init_head_partial_elems(1, 4, 16)), device=DEV)
    pp = ctypes.c_void_p(part.data_ptr())
    null = ctypes.c_void_p(0)
    rc = lib.as_init_head_bwd(p, p, p, null, p, pp, 1, 4, 4, 16, null)
    assert rc == -1 and b"init_head_bwd" in lib.as_last_error_string()
    for d in (0, 129):
        rc = lib.as_init_head_bwd(p, p, p, p, p, pp, 1, d, 4, 16, null)
        assert rc == -2 and b"init_head_bwd" in lib.as_last_error_string(), d
    rc = lib.as_init_head_bwd(p, p, p, p, p, pp, 0, 4, 4, 16, null)
    assert rc == -1 and b"init_head_bwd" in lib.as_last_error_string()
    rc = lib.as_init_head_wgrad_reduce(null, 1, p, null)
    assert rc == -1 and b"init_head_wgrad_reduce" in lib.as_last_error_string()
    assert lib.as_init_head_partial_elems(0, 4, 16) < 0
    torch.cuda.synchronize()


def test_init_disp_head_forward_equals_composition():
    """grad.InitDispHead's forward launches the kernels of the composition it replaces (searched convolution, then the fused
    softmax + regression): the same bits.  Its backward agrees with the composition's (MIOpen's convolution backward behind
    DisparityRegression's)."""
    from anystereo import grad as G
    from anystereo.nn import blocks as B
    from anystereo.nn import functional as AF
    conv = torch.nn.Conv3d(8, 1, 3, 1, 1, bias=False).to(DEV)
    geo, wt, _ = _head_case(2, 48, 16, 32, seed=5)
    with torch.no_grad():
        conv.weight.copy_(wt)
    x = geo.to(DEV).requires_grad_(True)
    assert B.init_head_ok(conv, x)
    new = G.InitDispHead.apply(x, conv.weight)
    old = AF.softmax_disparity_regression(B.conv3d_train(conv, x).squeeze(1))
    torch.cuda.synchronize()
    assert new.shape == old.shape == (2, 1, 16, 32)
    assert torch.equal(new, old)
    g = U((2, 1, 16, 32), 77).to(DEV)
    ga = torch.autograd.grad(new, (x, conv.weight), g)
    gb = torch.autograd.grad(old, (x, conv.weight), g)
    for a_, b_, what in zip(ga, gb, ("d_geo", "d_weight")):
        close(a_, b_, rtol=2e-5, atol=0.0, what=what)


def _g8_superinit(mode, deterministic=False):
    from anystereo import ops
    from anystereo.harness.metrics import sequence_loss_multiscale_superinit
    from anystereo.harness.synthetic import fill_module_deterministic, tiny_low_disp_gt, tiny_train_case
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo")
    model = __models__[args.model](args)
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV).train()
    model.freeze_bn()
    h, w, img1, img2, coord, gt, scale = tiny_train_case("igev")
    low = tiny_low_disp_gt().to(DEV)
    prev, prev_mode, prev_det = torch.backends.cudnn.deterministic, ops.get_precision(), ops.get_deterministic()
    torch.backends.cudnn.deterministic = True
    ls = 4096.0 if mode == "split" else 1.0
    try:
        ops.set_precision(mode)
        ops.set_deterministic(deterministic)
        init, preds = model(img1.to(DEV), img2.to(DEV), iters=3, hr_coord=coord.to(DEV), scale=scale.to(DEV))
        gtd = gt.to(DEV)
        loss, _ = sequence_loss_multiscale_superinit(init, low, preds, gtd, ((gtd < 512) & (gtd > 0)).float(), max_disp=args.max_disp,
                                                     sync_free=True)
        (loss * ls).backward()
        torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.deterministic = prev
        ops.set_precision(prev_mode)
        ops.set_deterministic(prev_det)
    grads = {n: p.grad.detach() / ls for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach(), init.detach(), preds[-1].detach(), grads


@pytest.mark.parametrize("mode", ["split", "fp32"])
def test_training_step_supervise_init_vs_reference(mode):
    """The G8 step with the supervise_init loss (init_disp differentiated through grad.InitDispHead) against the imported
    reference: loss, init_disp, last prediction, every gradient norm, the stored full tensors (classifier.weight and the
    hourglass' last upsampling convolution included); limits per tensor from the reference's own perturbation sensitivities."""
    z = np.load(os.path.join(GOLDEN, "train_igev_superinit.npz"))
    loss, init, last, grads = _g8_superinit(mode)
    assert abs(loss.item() - float(z["loss"])) < 1e-5 * abs(float(z["loss"])), (loss.item(), float(z["loss"]))
    e_init = (init.cpu() - torch.from_numpy(z["init_disp"])).abs().mean().item()
    e_last = (last.cpu() - torch.from_numpy(z["last_pred"])).abs().mean().item()
    print(f"[G8 superinit {mode}] loss rel {abs(loss.item() - float(z['loss'])) / abs(float(z['loss'])):.2e}; init_disp mean abs err "
          f"{e_init:.2e} px; last prediction {e_last:.2e} px")
    assert e_init <= 2e-4 and e_last < 2e-4, (e_init, e_last)
    names = [str(n) for n in z["names"]]
    assert sorted(grads) == names and "classifier.weight" in names
    lim_e, lim_n = _g8_limits("igev_superinit")
    norms = np.array([float(grads[n].double().norm()) for n in names])
    zero = z["norms"] < G8_ZERO_REF * z["norms"].max()
    assert (norms[zero] < G8_ZERO_GOT * z["norms"].max()).all()
    rel = np.where(zero, 0.0, np.abs(norms - z["norms"]) / (z["norms"] + 1e-6 * z["norms"].max()))
    ratio = rel / np.array([lim_n[n] for n in names])
    k = int(ratio.argmax())
    print(f"[G8 superinit {mode}] grad-norm rel max {rel.max():.2e}; closest to its limit: {names[k]} {rel[k]:.2e} / {lim_n[names[k]]:.1e}")
    assert ratio.max() < 1.0, f"grad-norm mismatch {rel[k]:.3e} at {names[k]}"
    for i, n in enumerate(str(x) for x in z["full_names"]):
        want = torch.from_numpy(z[f"g{i}"])
        got = grads[n].cpu()
        e = ((got - want).abs().max() / want.abs().max()).item()
        print(f"[G8 superinit {mode}] {n}: max |d| / max |g| = {e:.2e} (limit {lim_e[n]:.1e})")
        close(got, want, rtol=lim_e[n], atol=1e-6 * want.abs().max().item(), what=n)


def test_training_step_supervise_init_deterministic_mode():
    """ops.set_deterministic(True) + cudnn.deterministic: two supervise_init G8 steps give bit-equal gradients for every parameter."""
    l0, i0, _, g0 = _g8_superinit("split", deterministic=True)
    l1, i1, _, g1 = _g8_superinit("split", deterministic=True)
    assert torch.equal(l0, l1) and torch.equal(i0, i1)
    assert sorted(g0) == sorted(g1) and "classifier.weight" in g0
    diff = [n for n in g0 if not torch.equal(g0[n], g1[n])]
    assert not diff, diff[:5]


@pytest.mark.parametrize("scope", ["grads", "step"])
def test_trainer_supervise_init_graphed_matches_eager(scope, monkeypatch):
    """Trainer(supervise_init=True) with 6-tuple batches: 3 eager warm-up steps, capture, replays — against the eager step fed the
    same batches (the tolerances of test_trainer_graphed_step_recaptures_and_matches_eager); the classifier trains.  Scope "grads"
    also runs one mixed-precision eager step: finite gradients, the classifier's included."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer, synthetic_train_batch
    from anystereo.models import __models__, default_args
    monkeypatch.setenv("ANYSTEREO_TRAIN_GRAPH_SCOPE", scope)
    monkeypatch.setenv("ANYSTEREO_FUSED_ADAMW", "0")
    args = default_args("continuous_IGEVStereo")

    def fresh(graph, **kw):
        m = __models__["continuous_IGEVStereo"](args)
        fill_module_deterministic(m, base_seed=1)
        return Trainer(m.to(DEV), lr=2e-4, num_steps=100000, train_iters=3, max_disp=args.max_disp, graph=graph, supervise_init=True, **kw)

    a = synthetic_train_batch(2, 64, 128, n_query=3000, seed=1, device=DEV, low_disp=True)
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        eager, gr = fresh(False), fresh(True)
        assert gr.use_graph and gr.graph_scope == scope
        c0 = eager.model.classifier.weight.detach().clone()
        graphs = []
        for i in range(6):
            le, me = eager.step(tuple(t.clone() for t in a))
            lg, mg = gr.step(tuple(t.clone() for t in a))
            graphs.append(None if gr._graph is None else id(gr._graph["graph"]))
            assert abs(float(le) - float(lg)) <= 1e-3 * abs(float(le)), (scope, i, float(le), float(lg))
            for k in me:
                tol = 2e-2 * max(abs(float(me[k])), 1e-3) if k == "epe" else 2e-2
                assert abs(float(me[k]) - float(mg[k])) <= tol, (scope, i, k, float(me[k]), float(mg[k]))
        assert graphs[2] is None and graphs[3] is not None and graphs[3] == graphs[4] == graphs[5], graphs
        worst = 0.0
        for (n1, p1), (_, p2) in zip(eager.model.named_parameters(), gr.model.named_parameters()):
            worst = max(worst, ((p1 - p2).abs().max() / p1.abs().max().clamp_min(1e-12)).item())
        print(f"[graphed Trainer supervise_init, scope {scope}] worst parameter deviation {worst:.2e}")
        assert worst < 5e-3, worst
        for tr in (eager, gr):
            assert not torch.equal(c0, tr.model.classifier.weight.detach()), "the classifier did not train"
        if scope == "grads":
            mp_ = fresh(False, mixed_precision=True)
            loss, _ = mp_.step(tuple(t.clone() for t in a))
            torch.cuda.synchronize()
            assert torch.isfinite(loss)
            assert mp_.model.classifier.weight.grad is not None
            assert all(torch.isfinite(p.grad).all() for p in mp_.model.parameters() if p.grad is not None)
    finally:
        torch.backends.cudnn.deterministic = prev
