"""CPU: the --supervise_init training branch (train_continuous_IGEV.py:96-122, :220-221) — the loss against the imported
reference's values (tests/golden/loss_superinit.npz), its synchronisation-free form, the low-resolution ground truth of the
synthetic batches, train_step's batch / model checks, and a gloo world-2 Trainer step on the CPU oracle model against the
reference step (tests/golden/train_igev_superinit.npz)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _loss_inputs(golden):
    g = golden("loss_superinit")
    preds = [g[f"pred{i}"] for i in range(4)]
    return g, g["init"], g["low"], preds, g["gt"], g["valid"], int(g["max_disp"])


@pytest.mark.parametrize("sync_free", [False, True])
def test_superinit_loss_matches_reference(golden, sync_free):
    from anystereo.harness import metrics as M
    g, init, low, preds, gt, valid, md = _loss_inputs(golden)
    assert torch.isinf(low).any() and (low <= 0).any() and (low >= md / 4).any()  # the fixture covers what it should
    d = (init - low)[low < md / 4]
    assert (d.abs() < 1).any() and (d.abs() >= 1).any()
    loss, met = M.sequence_loss_multiscale_superinit(init, low, preds, gt, valid, max_disp=md, sync_free=sync_free)
    assert torch.isfinite(loss)
    assert abs(loss.item() - float(g["loss"])) <= 1e-6 * abs(float(g["loss"])), (loss.item(), float(g["loss"]))
    for k, gk in (("epe", "epe"), ("1px", "px1"), ("3px", "px3")):
        assert abs(float(met[k]) - float(g[gk])) <= (0.0 if not sync_free else 2e-6), (k, float(met[k]), float(g[gk]))


def test_superinit_sync_free_gradient_equals_reference_form(golden):
    """autograd of the masked-sum form gives the reference statement's dL/d init_disp (and dL/d predictions); the inf in the
    low-resolution ground truth produces no NaN anywhere."""
    from anystereo.harness import metrics as M
    _, init, low, preds, gt, valid, md = _loss_inputs(golden)
    grads = []
    for sync_free in (False, True):
        i = init.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in preds]
        loss, _ = M.sequence_loss_multiscale_superinit(i, low, ps, gt, valid, max_disp=md, sync_free=sync_free)
        loss.backward()
        assert torch.isfinite(i.grad).all() and all(torch.isfinite(p.grad).all() for p in ps), sync_free
        grads.append((i.grad, [p.grad for p in ps]))
    (a, pa), (b, pb) = grads
    assert (a - b).abs().max().item() <= 1e-7 * a.abs().max().item()
    assert (a[~(low < md / 4)] == 0).all()  # masked pixels (inf included) receive nothing
    for x, y in zip(pa, pb):
        assert (x - y).abs().max().item() <= 1e-7 * x.abs().max().item() + 1e-12


def test_superinit_loss_without_valid_pixel_is_nan():
    """the reference's mean over an empty selection: NaN, in both forms"""
    from anystereo.harness import metrics as M
    low = torch.full((1, 4, 5), 100.0)
    init = torch.zeros(1, 4, 5)
    gt = torch.full((1, 1, 6), 3.0)
    preds = [gt + 1.0, gt + 0.5]
    for sync_free in (False, True):
        loss, _ = M.sequence_loss_multiscale_superinit(init, low, preds, gt, torch.ones_like(gt), max_disp=192, sync_free=sync_free)
        assert torch.isnan(loss), sync_free


def test_synthetic_batch_low_disp():
    from anystereo.harness.train import synthetic_train_batch
    a = synthetic_train_batch(2, 64, 128, n_query=50, seed=3, low_disp=True)
    b = synthetic_train_batch(2, 64, 128, n_query=50, seed=3, low_disp=True)
    plain = synthetic_train_batch(2, 64, 128, n_query=50, seed=3)
    assert len(a) == 6 and len(plain) == 5
    assert tuple(a[5].shape) == (2, 16, 32) and a[5].dtype == torch.float32
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(a[:5], plain))  # the first five tensors are unchanged
    frac = (a[5] < 192 / 4).float().mean().item()
    assert 0.0 < frac < 1.0 and 0.75 <= frac <= 0.92, frac
    assert not torch.equal(a[5], synthetic_train_batch(2, 64, 128, n_query=50, seed=4, low_disp=True)[5])


def test_tiny_low_disp_gt_equal_valid_counts():
    from anystereo.harness.synthetic import tiny_low_disp_gt
    g = tiny_low_disp_gt()
    v = g < 192 / 4
    assert tuple(g.shape) == (2, 16, 32) and torch.isinf(g).any()
    assert v[0].sum() == v[1].sum() and 0 < v.sum() < v.numel()


class _PredsOnly(torch.nn.Module):
    """a model with the RAFT return convention: the predictions only"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))

    def forward(self, image1, image2, iters=1, hr_coord=None, scale=None):
        return [self.w * torch.ones(image1.shape[0], 1, hr_coord.shape[1])]


def test_train_step_supervise_init_checks():
    from anystereo.harness.metrics import train_step
    m = _PredsOnly().train()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    b5 = (torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 4, 2), torch.ones(1, 1, 4), torch.ones(1, 1))
    b6 = b5 + (torch.ones(1, 2, 2),)
    with pytest.raises(ValueError, match="6-tuple"):
        train_step(m, opt, None, None, b5, 1, supervise_init=True)
    with pytest.raises(ValueError, match="5-tuple"):
        train_step(m, opt, None, None, b6, 1)
    with pytest.raises(ValueError, match="init_disp"):
        train_step(m, opt, None, None, b6, 1, supervise_init=True)
    loss, _ = train_step(m, opt, None, None, b5, 1)  # the default path is unchanged
    assert torch.isfinite(loss)


def _superinit_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path[:0] = [root, os.path.join(root, "any-stereo_amd")]
    import numpy as np
    from anystereo.harness import dist
    from anystereo.harness.synthetic import fill_module_deterministic, tiny_low_disp_gt, tiny_train_case
    from anystereo.harness.train import Trainer, shard_batch
    from anystereo.models import default_args
    from oracle.model import OracleIGEV
    torch.set_num_threads(2)
    r, w, _ = dist.init("gloo")
    args = default_args("continuous_IGEVStereo")
    model = OracleIGEV(args)
    fill_module_deterministic(model, base_seed=1)
    tr = Trainer(model, num_steps=50, train_iters=3, max_disp=args.max_disp, supervise_init=True)
    _, _, img1, img2, coord, gt, scale = tiny_train_case("igev")
    batch = shard_batch((img1, img2, coord, gt, scale, tiny_low_disp_gt()), r, w)
    c0 = model.classifier.weight.detach().clone()
    loss, _ = tr.step(batch)
    assert isinstance(tr.module, torch.nn.parallel.DistributedDataParallel)
    z = np.load(os.path.join(root, "tests", "golden", "train_igev_superinit.npz"))
    total = float(np.sqrt((z["norms_w2"] ** 2).sum()))  # clip_grad_norm_(1.0) scaled the averaged gradient by 1/total
    named = dict(model.named_parameters())
    devs = {}
    for i, n in enumerate(str(x) for x in z["full_names"]):
        ref = torch.from_numpy(z[f"g{i}_w2"])
        got = named[n].grad * (total + 1e-6)
        devs[n] = ((got - ref).abs().max() / ref.abs().max()).item()
    moved = not torch.equal(c0, model.classifier.weight.detach())
    try:
        tr.step(batch[:5])
        raised = False
    except ValueError:
        raised = True
    losses = dist.sum_over_ranks([float(loss)])
    dist.finalize()
    q.put((r, devs, losses[0] / w, float(z["loss_w2"]), list(tr.frozen_unused), moved, raised))


def test_trainer_supervise_init_ddp_world2():
    """2 ranks x 1 sample, DDP(gloo), supervise_init: the probe pass runs the supervise_init loss, so the classifier is NOT frozen;
    the rank-averaged loss and the clip-scaled averaged gradients match the reference run the same way (the fixture's *_w2
    entries: each sample alone through the reference, averaged — the hourglass' BatchNorm3d normalises per rank)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_superinit_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = []
    for _ in range(600):
        try:
            res.append(q.get(timeout=0.5))
        except Exception:
            assert all(p.exitcode in (None, 0) for p in ps), "a rank died"
        if len(res) == len(ps):
            break
    assert len(res) == len(ps)
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    import numpy as np
    sens = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_igev_superinit_sens.npz"))
    lim = {str(n): min(5e-2, max(1e-3, 3.0 * float(d))) for n, d in zip(sens["full_names"], sens["full_dev"])}
    assert lim["classifier.weight"] == 1e-3  # stable in the reference: the tight floor applies to the classifier
    for r, devs, mean_loss, ref_loss, frozen, moved, raised in sorted(res):
        assert "classifier.weight" not in frozen and len(frozen) <= 4, frozen
        assert moved, "the classifier did not train"
        assert raised, "a 5-tuple batch with supervise_init did not raise"
        assert abs(mean_loss - ref_loss) < 1e-4 * abs(ref_loss), (mean_loss, ref_loss)
        # per tensor: 3x the deviation the reference's own eps-level input perturbations cause (train_igev_superinit_sens.npz;
        # ReLU patterns that flip move a few tensors by discrete amounts), never tighter than 1e-3
        print(f"[superinit world2 rank {r}] loss {mean_loss:.6f} vs {ref_loss:.6f}; " + ", ".join(f"{n} {d:.1e}" for n, d in devs.items()))
        for n, d in devs.items():
            assert d < lim[n], f"rank {r}: {n} deviates {d:.2e} of its maximum (limit {lim[n]:.1e})"
