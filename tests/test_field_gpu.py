"""GPU: `model.encode` / `StereoField.query` against `forward` and the generic loop's per-iteration predictions, under graph replay
and after weight / precision changes; `ops.resize_disparity` (csrc/resize_disp.hip) against the reference fixture and its plain-torch
restatement; `evaluate(curve=, baseline=)` end to end.  Models: the default IGEV (64x128) and RAFT (64x96) with the deterministic
fill, 4 GRU iterations, queried on the x1.5 grid.

Limits.  field.query against forward, repeated / partial / permuted queries: equal bits (the same kernels on the same operands; a
query's value does not depend on its neighbours).  Per-iteration states against the generic loop's predictions (code this feature
does not touch): mean |d| < 1e-3 px, the project's parity pin between the pipelined and the generic loop.  Graph replay against
eager: two replays equal, replay within 1e-4 of eager (the whole-forward replay tests' pin).  Resize: IMAGE_TOL / 255 * max|src * mul|
against the fixture (tests/test_field_cpu.py), equal bits against the restatement."""
import pytest
import torch

from test_field_cpu import CASES, IMAGE_TOL

from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
from anystereo.models.base import default_args
from anystereo.nn import liif as NL

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = 4
FAMILIES = {"igev": ("continuous_IGEVStereo", (64, 128)), "raft": ("continuous_RAFTStereo", (64, 96))}
_CACHE = {}


def setup(family):
    """(model, img1, img2, coord [1,Q,2], scale, grid shape, forward's result, forward's clamped coord), built once per family."""
    if family not in _CACHE:
        from anystereo.models import __models__
        mname, (H, W) = FAMILIES[family]
        model = __models__[mname](default_args(mname)).eval()
        fill_module_deterministic(model, base_seed=1)
        model = model.to(DEV)
        img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
        hq, wq = round(H * 1.5), round(W * 1.5)
        coord = NL.make_coord([hq, wq]).unsqueeze(0).to(DEV)
        coord[0, 0] = torch.tensor([-1.0, 1.0])  # outside the clamp range: the in-place side effect must show
        scale = torch.tensor([[1.5]], device=DEV)
        img1, img2 = img1.to(DEV), img2.to(DEV)
        used = coord.clone()
        with torch.no_grad():
            fwd = model(img1, img2, iters=ITERS, test_mode=True, hr_coord=used, scale=scale)
        _CACHE[family] = (model, img1, img2, coord, scale, (hq, wq), fwd, used)
    return _CACHE[family]


def field_of(family, at=None):
    key = (family, "field", at)
    if key not in _CACHE:
        model, img1, img2 = setup(family)[:3]
        with torch.no_grad():
            _CACHE[key] = model.encode(img1, img2, iters=ITERS, at=at)
    return _CACHE[key]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_query_equals_forward(family):
    model, img1, img2, coord, scale, _, fwd, used = setup(family)
    field = field_of(family)
    assert field.at == (ITERS,) and field.iters == ITERS
    mine = coord.clone()
    got = field.query(mine, scale)
    assert got.shape == fwd.shape == (1, 1, coord.shape[1]) and torch.isfinite(got).all()
    assert torch.equal(got, fwd), (got - fwd).abs().max().item()
    assert torch.equal(mine, used) and not torch.equal(mine, coord)  # clamped in place, as forward clamps its caller's tensor
    parts = [[t for t in (field._stem_4x, field._net[ITERS]) if t is not None]] + ([[field._stem_2x]] if field._stem_2x is not None else [])
    with torch.no_grad():
        fused = field._stem_1x is None and model.liif_up.fused_ok(parts, coord)
    assert fused or family != "igev"  # the default IGEV takes the fused tail
    if fused:  # then the rows of its inputs are kept: stem_2x's per field, the hidden state's per kept iteration
        assert sorted(field._rows) == [ITERS] and (field._rows_static is not None) == (len(parts) == 2)
    low = field.low()
    assert tuple(low.shape) == (1, 1, img1.shape[-2] // 4, img1.shape[-1] // 4) and torch.isfinite(low).all()
    low.zero_()
    assert torch.equal(field.query(coord.clone(), scale), fwd)  # low() hands out a clone


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_repeated_partial_and_unordered_queries(family):
    _, _, _, coord, scale, (hq, wq), fwd, _ = setup(family)
    field = field_of(family)
    first = field.query(coord.clone(), scale)
    assert torch.equal(field.query(coord.clone(), scale), first) and torch.equal(first, fwd)
    # a sub-rectangle of the grid (another Q, rows that do not start at a row of the full grid's tiles)
    ys, xs = torch.arange(5, hq - 7, device=DEV), torch.arange(3, wq - 11, device=DEV)
    idx = (ys.view(-1, 1) * wq + xs.view(1, -1)).reshape(-1)
    sub = field.query(coord[:, idx].contiguous(), scale)
    assert sub.shape == (1, 1, idx.numel()) and torch.equal(sub, first[:, :, idx])
    # unordered: a fixed permutation of the queries
    perm = torch.randperm(coord.shape[1], generator=torch.Generator().manual_seed(5)).to(DEV)
    assert torch.equal(field.query(coord[:, perm].contiguous(), scale), first[:, :, perm])
    # another scale on the same field: what a forward at that scale gives
    model, img1, img2 = setup(family)[:3]
    c2 = NL.make_coord([img1.shape[-2] * 2, img1.shape[-1] * 2]).unsqueeze(0).to(DEV)
    s2 = torch.tensor([[2.0]], device=DEV)
    with torch.no_grad():
        want = model(img1, img2, iters=ITERS, test_mode=True, hr_coord=c2.clone(), scale=s2)
    assert torch.equal(field.query(c2.clone(), s2), want)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_kept_iterations_match_the_generic_loop(family):
    """The test that catches a kept tensor a later iteration overwrote: at = (1, 2, 4) against the predictions of the generic loop
    (test_mode=False under no_grad: every iteration up-sampled by the same upsampler)."""
    model, img1, img2, coord, scale, _, fwd, _ = setup(family)
    with torch.no_grad():
        out = model(img1, img2, iters=ITERS, test_mode=False, hr_coord=coord.clone(), scale=scale)
    preds = out[1] if family == "igev" else out
    assert len(preds) == ITERS
    field = field_of(family, at=(1, 2, 4))
    assert field.at == (1, 2, 4)
    every = field.query(coord.clone(), scale, at="all")
    assert every.shape == (3, 1, 1, coord.shape[1])
    for i, k in enumerate(field.at):
        got = field.query(coord.clone(), scale, at=k)
        assert torch.equal(got, every[i])
        d = (got - preds[k - 1]).abs()
        print(f"[{family} iteration {k}] against the generic loop: mean |d| = {d.mean().item():.3e}, max |d| = {d.max().item():.3e}")
        assert d.mean().item() < 1e-3, (family, k)
    assert torch.equal(every[2], fwd) and torch.equal(field.low(), field.low(at=4))
    assert not torch.equal(every[0], every[1]) and not torch.equal(field.low(at=1), field.low(at=2))
    with pytest.raises(ValueError, match="not kept"):
        field.query(coord.clone(), scale, at=3)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_graph_replay_equals_eager(family):
    model, img1, img2, coord, scale, _, fwd, _ = setup(family)
    eager = field_of(family, at=(2, 4))
    try:
        model.enable_graph(True)
        with torch.no_grad():
            g1 = model.encode(img1, img2, iters=ITERS, at=(2, 4))
            g2 = model.encode(img1, img2, iters=ITERS, at=(2, 4))
            assert len(model._graphs) == 1
            other = model.encode(img1, img2, iters=ITERS, at=(1, 4))
        assert len(model._graphs) == 2 and len({k.at for k in model._graphs}) == 2  # two `at` sets, two graphs
        assert other.at == (1, 4)
        for k in (2, 4):
            q1, q2 = g1.query(coord.clone(), scale, at=k), g2.query(coord.clone(), scale, at=k)
            assert torch.equal(q1, q2) and torch.equal(g1.low(at=k), g2.low(at=k))
            d = (q1 - eager.query(coord.clone(), scale, at=k)).abs().max().item()
            dl = (g1.low(at=k) - eager.low(at=k)).abs().max().item()
            print(f"[{family} iteration {k}] replay against eager: query max |d| = {d:.3e}, low max |d| = {dl:.3e}")
            assert d <= 1e-4 and dl <= 1e-4
        assert torch.equal(other.query(coord.clone(), scale), g1.query(coord.clone(), scale))
    finally:
        model.enable_graph(False)
    with torch.no_grad():  # forward is what it was
        assert torch.equal(model(img1, img2, iters=ITERS, test_mode=True, hr_coord=coord.clone(), scale=scale), fwd)


def test_refusals():
    from anystereo import ops
    model, img1, img2, coord, scale = setup("raft")[:5]
    with torch.no_grad():
        for bad in ((0,), (5,)):
            with pytest.raises(ValueError, match="outside"):
                model.encode(img1, img2, iters=ITERS, at=bad)
        try:
            with pytest.raises(RuntimeError, match="training mode"):
                model.train().encode(img1, img2, iters=ITERS)
        finally:
            model.eval()
        with pytest.raises(RuntimeError, match="CUDA"):
            model.encode(img1.cpu(), img2.cpu(), iters=ITERS)
    with pytest.raises(RuntimeError, match="gradients"):
        model.encode(img1, img2, iters=ITERS)
    with torch.no_grad():
        field = model.encode(img1, img2, iters=ITERS)
        want = field.query(coord.clone(), scale)
        try:
            ops.set_precision("fp32")
            with pytest.raises(RuntimeError, match="set_precision"):
                field.query(coord.clone(), scale)
        finally:
            ops.set_precision("split")
        assert torch.equal(field.query(coord.clone(), scale), want)
        try:
            next(model.parameters()).add_(0.0)  # an in-place update: same values, another version
            with pytest.raises(RuntimeError, match="weights changed"):
                field.query(coord.clone(), scale)
            assert torch.equal(model.encode(img1, img2, iters=ITERS).query(coord.clone(), scale), want)
        finally:  # the fields other tests cached for this model belong to the old version
            for key in [k for k in _CACHE if isinstance(k, tuple) and k[0] == "raft"]:
                del _CACHE[key]


# ---- ops.resize_disparity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(5))
def test_resize_disparity_vs_fixture_and_restatement(golden, k):
    from anystereo import ops
    from anystereo.harness.query import resize_disparity_host
    fx = golden("resize_disp")
    h, w, s, _ = CASES[k]
    m, want = fx[f"c{k}_map"], fx[f"c{k}_out"][:, 0]
    crop = tuple(int(v) for v in fx[f"c{k}_crop"])
    lim = IMAGE_TOL / 255 * (m * s).abs().max().item()
    src = m.to(DEV)
    out = torch.full((2, h, w), float("nan"), device=DEV)  # written in full: no NaN may be left
    got = ops.resize_disparity(src, crop, (h, w), s, out=out)
    assert got is out and not torch.isnan(out).any()
    d = (got.cpu() - want).abs().max().item()
    print(f"[resize_disparity {(h, w)} x{s}] max |d| = {d:.3e} (limit {lim:.3e})")
    if s == 1.0:
        assert torch.equal(got.cpu(), want)
    else:
        assert d <= lim, (k, d, lim)
    assert torch.equal(got.cpu(), resize_disparity_host(m, crop, (h, w), s))
    again = ops.resize_disparity(src[:, 0].contiguous(), crop, (h, w), s)
    assert torch.equal(again, got)
    assert torch.equal(torch.ops.anystereo.resize_disparity(src, list(crop), [h, w], s), got)
    # captured: no allocation, the caller's stream
    static = torch.full((2, h, w), float("nan"), device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.resize_disparity(src, crop, (h, w), s, out=static)
    torch.cuda.current_stream().wait_stream(side)
    static.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.resize_disparity(src, crop, (h, w), s, out=static)
    static.fill_(float("nan"))
    g.replay()
    assert torch.equal(static, got)


def test_resize_disparity_many_blocks_and_offsets_past_2_31():
    """Odd sizes over many tiles, against the restatement; then 40000 maps of 232 x 232 = 2.15e9 output elements: the per-map
    offsets pass 2^31, the first and the last maps are compared."""
    from anystereo import ops
    from anystereo.harness.query import resize_disparity_host
    from anystereo.harness.synthetic import det_uniform
    src = det_uniform((3, 1, 150, 271), 31, -3, 200).to(DEV)
    crop, size = (7, 13, 131, 250), (301, 517)
    assert torch.equal(ops.resize_disparity(src, crop, size, 2.3), resize_disparity_host(src, crop, size, 2.3))
    assert torch.equal(ops.resize_disparity(src, crop, (131, 250), 1.0), src[:, 0, 7:138, 13:263])
    n, hw = 40000, 232
    small = det_uniform((n, 10, 12), 32, -3, 200).to(DEV)
    assert n * hw * hw > 2 ** 31
    out = ops.resize_disparity(small, (1, 2, 8, 9), (hw, hw), 1.7)
    for sl in (slice(0, 50), slice(n - 50, n)):
        assert torch.equal(out[sl], resize_disparity_host(small[sl], (1, 2, 8, 9), (hw, hw), 1.7))
    del out
    torch.cuda.empty_cache()


def test_resize_disparity_refusals():
    from anystereo import ops
    z = torch.zeros(1, 8, 8, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.resize_disparity(z.cpu(), (0, 0, 4, 4), (6, 6))
    for crop in ((0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -1, 4)):
        with pytest.raises(RuntimeError, match="empty crop"):
            ops.resize_disparity(z, crop, (6, 6))
    for crop in ((-1, 0, 4, 4), (0, -1, 4, 4), (5, 0, 4, 4), (0, 5, 4, 4), (0, 0, 9, 4), (0, 0, 4, 9)):
        with pytest.raises(RuntimeError, match="leaves"):
            ops.resize_disparity(z, crop, (6, 6))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.resize_disparity(z, (0, 0, 4, 4), (6, 6), out=torch.zeros(1, 6, 7, device=DEV))
    with pytest.raises(RuntimeError, match="float32"):
        ops.resize_disparity(z.double(), (0, 0, 4, 4), (6, 6))


# ---- evaluate(curve=, baseline=) ----------------------------------------------------------------------------------------------
def test_evaluate_with_curve_and_baseline():
    from anystereo.harness.evaluate import Evaluator, evaluate
    from anystereo.harness.query import prepare_on_device, query_grid_host, query_plan, resize_disparity_host

    class Keeping(Evaluator):
        def update(self, est, *a, **k):
            self.kept = est.clone()
            return super().update(est, *a, **k)

    model = setup("igev")[0]
    h, w, s, div = 45, 70, 1.3, 32
    i1, i2 = synthetic_pair(1, h, w, shift=6, seed=123)
    i1, i2 = i1.to(DEV), i2.to(DEV)
    gt = torch.full((1, h, w), 6.0, device=DEV)
    pair = (i1, i2, gt, torch.ones(1, h, w, device=DEV), torch.ones(1, h, w, dtype=torch.uint8, device=DEV))
    base = evaluate(model, [pair], scale=s, iters=ITERS, protocol="kitti", divis_by=div, prep="device")
    ev = Keeping("kitti")
    res = evaluate(model, [pair], scale=s, iters=ITERS, protocol="kitti", divis_by=div, prep="device", evaluator=ev, curve=(2, 4),
                   baseline="bicubic")
    assert res["estimates"] == ["iter2", "iter4", "bicubic"] and "estimates" not in base
    for region in ("all", "noc", "occ"):
        for metric, vals in res[region].items():
            assert len(vals) == 3 and vals[1] == base[region][metric][0], (region, metric)
    assert res["all"]["EPE"][0] != res["all"]["EPE"][1]
    assert tuple(ev.kept.shape) == (3, 1, h, w)
    # the baseline: a separate scale-1 forward of the same padded pair, un-padded, times scale, resized
    plan = query_plan(h, w, s, div)
    p1, p2, _, _ = prepare_on_device(i1, i2, s, divis_by=div)
    grid = query_grid_host(query_plan(plan.h_pad, plan.w_pad, 1.0, div), 1).to(DEV)
    with torch.no_grad():
        low = model(p1, p2, iters=ITERS, test_mode=True, hr_coord=grid, scale=torch.ones(1, 1, device=DEV))
    low = low.reshape(1, plan.h_pad, plan.w_pad).cpu()
    want = resize_disparity_host(low, (plan.pad[0], plan.pad[2], plan.h_lr, plan.w_lr), (h, w), s)
    lim = IMAGE_TOL / 255 * (low * s).abs().max().item()
    d = (ev.kept[2].cpu() - want).abs().max().item()
    print(f"[evaluate baseline] against resize_disparity_host of a scale-1 forward: max |d| = {d:.3e} (limit {lim:.3e})")
    assert d <= lim
