"""GPU (-m gpu): the fused evaluation kernels (csrc/eval_metrics.hip) — `ops.disparity_metrics` and `ops.lr_consistency` against the
plain-torch restatement of harness/evaluate.py and against the reference's own numbers (tests/golden/eval_metrics.npz), their
registered operators, the Evaluator on the device and `evaluate()` end to end.

The three fixture shapes take every path of the metrics kernel: 24 x 80 = 1920 pixels lie inside one 2048-pixel chunk; 37 x 131 =
4847 is odd (scalar loads, image planes that start unaligned, a partly filled last chunk); 64 x 200 = 12 800 spans 7 chunks, so the
second launch sums real rows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(2, 24, 80), (1, 37, 131), (2, 64, 200)]
REGIONS = ("all", "noc", "occ")
METRICS = ("EPE", "D1", "Thres1", "Thres2", "Thres3")
COUNT_COLS = [c for c in range(19) if c not in (1, 7, 13)]
SUM_COLS = [1, 7, 13]
INF = float("inf")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("eval_metrics")


def _case(fx, k, n):
    """est [n,B,H,W], gt, valid (bool), noc (uint8) of shape k.  The third estimate is the mirror image of the first two's mean."""
    est = fx[f"s{k}_est"]
    if n == 1:
        est = est[:1]
    elif n == 3:
        est = torch.cat([est, (est[1:] * 0.5 + fx[f"s{k}_dl"].unsqueeze(0) * 0.5)])
    return est.contiguous(), fx[f"s{k}_dl"], fx[f"s{k}_valid_gt"] > 0.5, fx[f"s{k}_occ_mask"]


def _assert_rows(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == torch.float64, what
    assert torch.equal(got[..., COUNT_COLS], want[..., COUNT_COLS]), (what, "counts")
    # both sides add the same fp32 values in fp64: reordering n <= 2^20 terms moves the sum by at most n * 2^-53 ~ 1e-10 relative
    a, b = got[..., SUM_COLS], want[..., SUM_COLS]
    assert ((a - b).abs() <= 1e-9 * b.abs()).all(), (what, "sum E", (a - b).abs().max().item())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_disparity_metrics_vs_host_restatement(fx, k, n):
    from anystereo import ops
    from anystereo.harness.evaluate import metric_rows_host
    est, gt, valid, noc = _case(fx, k, n)
    d = [t.to(DEV) for t in (est, gt, valid, noc)]
    for use_valid, use_noc, lo, hi in [(True, True, -INF, INF), (False, False, -INF, INF), (True, False, -INF, 1000.0),
                                       (False, True, 4.5, 13.0)]:
        v, m = (valid if use_valid else None), (noc if use_noc else None)
        got = ops.disparity_metrics(d[0], d[1], d[2] if use_valid else None, d[3] if use_noc else None, lo, hi)
        want = metric_rows_host(est, gt, v, m, lo, hi)
        assert tuple(got.shape) == (n, SHAPES[k][0], 19) and got.is_cuda
        _assert_rows(got, want, (k, n, use_valid, use_noc, lo, hi))
    # other thresholds, and a [B,H,W] estimate counts as N = 1
    got = ops.disparity_metrics(d[0][0], d[1], d[2], d[3], thres=(0.5, 1.5, 4.0))
    _assert_rows(got, metric_rows_host(est[:1], gt, valid, noc, thres=(0.5, 1.5, 4.0)), (k, "thres"))


def test_disparity_metrics_multi_trip_blocks():
    """Above 2^21 pixels per image a block takes several 2048-pixel trips: 1030 x 2040 = 2 101 200 pixels -> 2 trips, 513 chunks, the
    last one ending inside its first trip.  Same bound as above (n * 2^-53 = 2.3e-10 here)."""
    from anystereo import _lib, ops
    from anystereo.harness.evaluate import metric_rows_host
    from anystereo.harness.synthetic import det_uniform
    h, w = 1030, 2040
    assert _lib.load().as_disp_metrics_partial_elems(1, 1, h, w) == 513 * 19
    gt = det_uniform((1, h, w), 11, -2.0, 60.0)
    est = (gt + det_uniform((1, h, w), 12, -6.0, 6.0)).unsqueeze(0)
    valid = det_uniform((1, h, w), 13, 0.0, 1.0) > 0.1
    noc = (det_uniform((1, h, w), 14, 0.0, 1.0) > 0.2).to(torch.uint8)
    got = ops.disparity_metrics(est.to(DEV), gt.to(DEV), valid.to(DEV), noc.to(DEV), 0.0, 50.0)
    _assert_rows(got, metric_rows_host(est, gt, valid, noc, 0.0, 50.0), "multi-trip")
    assert torch.equal(got, ops.disparity_metrics(est.to(DEV), gt.to(DEV), valid.to(DEV), noc.to(DEV), 0.0, 50.0))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_disparity_metrics_vs_reference_fixture(fx, k):
    """D1 / Thres-k as count / n in fp32 within 1e-6 of the reference's values (both a correctly rounded quotient of the same integers,
    averaged over the batch); EPE within rel 1e-5 (the reference's fp32 pairwise sum over n <= 2^20 terms carries ~1.2e-6)."""
    from anystereo import ops
    est, gt, valid, noc = _case(fx, k, 2)
    rows = ops.disparity_metrics(est.to(DEV), gt.to(DEV), valid.to(DEV), noc.to(DEV), -INF, 1000.0).cpu()
    want = fx[f"s{k}_plain"]  # [2 estimates, 3 regions, 5]
    assert torch.equal(want, fx[f"s{k}_filter"])  # no image of these scenes is filtered
    for i in range(2):
        for r in range(3):
            n = rows[i, :, 6 * r]
            epe = (rows[i, :, 6 * r + 1] / n).float().mean().item()
            w = want[i, r, 0].item()
            print(f"[eval fixture s{k} est{i} {REGIONS[r]}] EPE {epe:.7f} (reference {w:.7f})")
            assert abs(epe - w) <= 1e-5 * abs(w), (k, i, r)
            for m in range(1, 5):
                ratio = (rows[i, :, 6 * r + 1 + m].float() / n.float()).mean().item()
                assert abs(ratio - want[i, r, m].item()) <= 1e-6, (k, i, r, METRICS[m], ratio, want[i, r, m].item())


def test_inf_estimates_count_as_zeros(fx):
    from anystereo import ops
    est, gt, valid, noc = _case(fx, 0, 1)
    assert torch.isinf(est).sum() >= 5
    zeroed = torch.where(torch.isinf(est), torch.zeros_like(est), est)
    a = ops.disparity_metrics(est.to(DEV), gt.to(DEV), valid.to(DEV), noc.to(DEV))
    b = ops.disparity_metrics(zeroed.to(DEV), gt.to(DEV), valid.to(DEV), noc.to(DEV))
    assert torch.equal(a, b) and torch.isfinite(a).all()


@pytest.mark.parametrize("k", [1, 2])
def test_disparity_metrics_repeatable_and_complete(fx, k):
    from anystereo import ops
    est, gt, valid, noc = (t.to(DEV) for t in _case(fx, k, 3))
    a = ops.disparity_metrics(est, gt, valid, noc)
    b = ops.disparity_metrics(est, gt, valid, noc)
    assert torch.equal(a, b)
    # every element of the output is written: a NaN-filled buffer comes back NaN-free, also when no pixel is valid
    out = torch.full((3, gt.shape[0], 19), float("nan"), dtype=torch.float64, device=DEV)
    res = ops.disparity_metrics(est, gt, torch.zeros_like(valid), noc, out=out)
    assert res.data_ptr() == out.data_ptr()
    out = out.cpu()
    assert torch.equal(out[..., :18], torch.zeros(3, gt.shape[0], 18, dtype=torch.float64))
    assert torch.equal(out[..., 18], (gt > 0).sum((-2, -1)).double().cpu().expand(3, -1))
    out2 = torch.full((3, gt.shape[0], 19), float("nan"), dtype=torch.float64, device=DEV)
    ops.disparity_metrics(est, gt, valid, noc, out=out2)
    assert torch.equal(out2, a)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_lr_consistency_vs_reference_mask(fx, k):
    """Pixels whose reference margin | |x - l2r2l| - 3 | is below 1e-3 (at most 0.5 % of the shape) are left out; all others equal.
    Shapes 0 and 2 hold two samples that differ, so a batch-stride slip shows."""
    from anystereo import ops
    b, h, w = SHAPES[k]
    dl, dr, ref = fx[f"s{k}_dl"], fx[f"s{k}_dr"], fx[f"s{k}_occ_mask"]
    got = ops.lr_consistency(dl.to(DEV), dr.to(DEV))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (b, h, w)
    got = got.cpu()
    near = ((torch.arange(w).float() - fx[f"s{k}_l2r2l"]).abs() - 3.0).abs() < 1e-3
    assert near.float().mean().item() <= 0.005
    assert torch.equal(got[~near], ref[~near]), int((got != ref)[~near].sum())
    if b == 2:
        assert not torch.equal(ref[0], ref[1])
        swapped = ops.lr_consistency(dl.flip(0).contiguous().to(DEV), dr.flip(0).contiguous().to(DEV)).cpu()
        assert torch.equal(swapped, got.flip(0))
    # [B,1,H,W] inputs give the same mask; a wider threshold can only add pixels
    assert torch.equal(ops.lr_consistency(dl.unsqueeze(1).to(DEV), dr.unsqueeze(1).to(DEV)).cpu(), got)
    wider = ops.lr_consistency(dl.to(DEV), dr.to(DEV), 5.0).cpu()
    assert bool((wider >= got).all()) and int(wider.sum()) > int(got.sum())


def test_registered_operators_return_what_ops_return(fx):
    import anystereo  # noqa: F401
    from anystereo import ops
    est, gt, valid, noc = (t.to(DEV) for t in _case(fx, 1, 3))
    a = torch.ops.anystereo.disparity_metrics(est, gt, valid, noc, -INF, 1000.0, [1.0, 2.0, 3.0])
    assert torch.equal(a, ops.disparity_metrics(est, gt, valid, noc, -INF, 1000.0))
    a = torch.ops.anystereo.disparity_metrics(est, gt, None, None, -INF, INF, [0.5, 1.0, 2.0])
    assert torch.equal(a, ops.disparity_metrics(est, gt, thres=(0.5, 1.0, 2.0)))
    dl, dr = fx["s1_dl"].to(DEV), fx["s1_dr"].to(DEV)
    assert torch.equal(torch.ops.anystereo.lr_consistency(dl, dr, 3.0), ops.lr_consistency(dl, dr, 3.0))


def _same_result(got, want, what):
    assert got["images"] == want["images"], (what, got["images"], want["images"])
    for region in REGIONS:
        for metric in METRICS:
            for g, w in zip(got[region][metric], want[region][metric]):
                # the counts are exact on both sides, so the ratios are the same fp64 quotients; EPE: sum E reordered
                assert abs(g - w) <= (1e-6 * abs(w) if metric == "EPE" else 0.0), (what, region, metric, g, w)


@pytest.mark.parametrize("protocol", ["things", "kitti", "middlebury", "eth3d"])
def test_evaluator_on_gpu_equals_evaluator_on_cpu(fx, protocol):
    from anystereo.harness.evaluate import Evaluator
    cpu, gpu = Evaluator(protocol), Evaluator(protocol)

    def vmap(v):  # the fixture's valid_gt is 0 / 1; middlebury / eth3d test `valid_gt >= -0.5`, so holes are -1 there
        return v * 2 - 1 if protocol in ("middlebury", "eth3d") else v
    for k in range(3):
        est, dl, dr, occ = fx[f"s{k}_est"], fx[f"s{k}_dl"], fx[f"s{k}_dr"], fx[f"s{k}_occ_mask"]
        valid = vmap(fx[f"s{k}_valid_gt"])
        if protocol == "things":
            cpu.update(est, dl, valid, gt_right=dr)
            gpu.update(est.to(DEV), dl.to(DEV), valid.to(DEV), gt_right=dr.to(DEV))
        else:
            cpu.update(est, dl, valid, noc=occ)
            gpu.update(est.to(DEV), dl.to(DEV), valid.to(DEV), noc=occ.to(DEV))
    # the filter and the guard case ride along
    extra = {"gt_right": fx["s0_dr"][:1]} if protocol == "things" else {"noc": fx["s0_occ_mask"][:1]}
    for name in ("case_filter_valid_gt", "case_guard_valid_gt"):
        cpu.update(fx["s0_est"][:, :1], fx["s0_dl"][:1], vmap(fx[name]), **extra)
        gpu.update(fx["s0_est"][:, :1].to(DEV), fx["s0_dl"][:1].to(DEV), vmap(fx[name]).to(DEV), **{k_: v.to(DEV) for k_, v in extra.items()})
    assert all(r.is_cuda for r in gpu._rows)
    want, got = cpu.result(), gpu.result()
    assert want["images"]["seen"] == 7 and want["images"]["all"] == 6
    assert want["images"]["noc"] == (5 if protocol == "things" else 6)
    rows_c, rows_g = cpu.rows(), gpu.rows()
    assert torch.equal(rows_c[..., COUNT_COLS], rows_g[..., COUNT_COLS])
    _same_result(got, want, protocol)


class _Recorder(torch.nn.Module):
    """Keeps what the wrapped model returned, so the CPU side sees the very same predictions."""

    def __init__(self, model):
        super().__init__()
        self.model, self.preds = model, []

    def forward(self, *args, **kwargs):
        out = self.model(*args, **kwargs)
        self.preds.append(out.detach().clone())
        return out


def test_evaluate_end_to_end():
    """evaluate() on two synthetic pairs of known disparity 6: IGEV, deterministic fill, 2 iterations, scale 1.5, protocol "kitti"
    with an all-ones mask.  The result equals the CPU Evaluator fed the same predictions."""
    from anystereo.harness import evaluate as E
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    h, w, s, iters = 64, 128, 1.5, 2
    model = __models__["continuous_IGEVStereo"](default_args("continuous_IGEVStereo")).eval()
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV)
    pairs = []
    for seed in (7, 8):
        i1, i2 = synthetic_pair(1, h, w, shift=6, seed=seed)
        pairs.append((i1.to(DEV), i2.to(DEV), torch.full((1, h, w), 6.0, device=DEV), torch.ones(1, h, w, device=DEV),
                      torch.ones(1, h, w, dtype=torch.uint8, device=DEV)))
    rec = _Recorder(model)
    res = E.evaluate(rec, pairs, scale=s, iters=iters, protocol="kitti")
    assert res["pairs"] == 2 and res["pairs_per_s"] > 0
    assert res["images"] == {"seen": 2, "all": 2, "noc": 2, "occ": 0}
    for region in ("all", "noc"):
        for metric in METRICS:
            v = res[region][metric]
            assert len(v) == 1 and v[0] == v[0] and abs(v[0]) != INF, (region, metric, v)
    assert res["occ"] == {m: [0.0] for m in METRICS}
    # the same predictions through the CPU Evaluator
    cpu = E.Evaluator("kitti")
    assert len(rec.preds) == 2
    for pred, (i1, i2, gt, valid, noc) in zip(rec.preds, pairs):
        assert tuple(pred.shape) == (1, 1, h * w)
        cpu.update(pred.reshape(1, 1, h, w).cpu(), gt.cpu(), valid.cpu(), noc=noc.cpu())
    want = cpu.result()
    _same_result({k: res[k] for k in want}, want, "end to end")


def test_refusals():
    from anystereo import ops
    g = torch.zeros(2, 8, 16, device=DEV)
    c = torch.zeros(2, 8, 16)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_metrics(c, c)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_metrics(g, g, valid=torch.ones(2, 8, 16, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.lr_consistency(c, c)
    with pytest.raises(RuntimeError, match="float32"):
        ops.disparity_metrics(g.double(), g)
    with pytest.raises(RuntimeError, match="uint8 or bool"):
        ops.disparity_metrics(g, g, valid=torch.ones(2, 8, 16, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        ops.lr_consistency(g.half(), g.half())
    with pytest.raises(RuntimeError, match="does not match"):
        ops.disparity_metrics(torch.zeros(1, 2, 8, 15, device=DEV), g)
    with pytest.raises(RuntimeError, match="does not match"):
        ops.disparity_metrics(g, g, noc=torch.ones(2, 8, 15, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="empty"):
        ops.disparity_metrics(torch.zeros(0, 2, 8, 16, device=DEV), g)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.disparity_metrics(g.transpose(1, 2), g.transpose(1, 2))
    with pytest.raises(RuntimeError, match="share"):
        ops.lr_consistency(g, torch.zeros(2, 8, 15, device=DEV))
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        ops.lr_consistency(torch.zeros(1, 1, 16, device=DEV), torch.zeros(1, 1, 16, device=DEV))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.disparity_metrics(g, g, out=torch.zeros(1, 2, 18, dtype=torch.float64, device=DEV))
