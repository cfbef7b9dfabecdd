"""GPU (-m gpu): the two kernels of csrc/prepare.hip — `ops.prepare_pair` (bicubic down-scale + replicate pad + uint8 -> fp32 of both
images) and `ops.query_grid` (hr_coord written by the device) — against their plain-torch restatements, the project's host path,
the reference's own pad_for_multi_train (tests/golden/prepare_pair.npz), their registered operators, and `evaluate(prep="device")`
against `evaluate(prep="host")`.

Shapes (H, W, scale, divis_by), the smallest at which each failure mode exists: 40x64 x1.0 no resize, rows padded 12/12, crop branch;
64x96 x2.0 exact half-pixel phase, columns padded 8/8, crop branch; 37x53 x1.5 odd sizes (every second query row starts on an odd
query: the shifted 16-byte pairs), uneven padding, `resized` branch; 45x70 x1.3 a non-terminating scale; 33x65 x2.95 the taps reach
past all four borders of a 12x23 frame; 375x1242 x2.0 several blocks per row; 1988x2964 x1.5 (grid only) 5.9 M queries, offsets
above 2^23 elements.  B = 2 with different images throughout.

Limits: see tests/test_prepare_cpu.py (grid: equal in the crop branch, 2.4e-7 in the `resized` branch; images: 1e-3 grey levels).
The kernel and `query_grid_host` perform the same unfused fp32 operations, so those two are compared with torch.equal."""
import pytest
import torch

from test_prepare_cpu import B, IMAGE_TOL, RESIZED, SHAPES, check_grid, host_coord

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INF = float("inf")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("prepare_pair")


def _plan(k):
    from anystereo.harness.query import query_plan
    h, w, s, div = SHAPES[k]
    return query_plan(h, w, s, div)


def _nan_then_free(numel, count=1):
    """Fill `count` blocks of the caching allocator with NaN, all alive together, and free them: the next `count` allocations of
    that size reuse them."""
    t = [torch.full((numel,), float("nan"), device=DEV) for _ in range(count)]
    torch.cuda.synchronize()
    del t


_grids = {}


def device_grid(k):
    """ops.query_grid at SHAPES[k] into a NaN-pre-filled block, on the host (computed once)."""
    if k not in _grids:
        from anystereo import ops
        pl = _plan(k)
        _nan_then_free(B * pl.h_want * pl.w_want * 2)
        g = ops.query_grid(pl, B, DEV)
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (B, pl.h_want * pl.w_want, 2) and g.is_contiguous()
        rows = ops.liif_query_rows(g)
        again = ops.query_grid(pl, B, DEV)
        _grids[k] = (g.cpu(), int(rows.item()), torch.equal(g, again))
    return _grids[k]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_query_grid_equals_host_restatement(k):
    from anystereo.harness.query import query_grid_host
    got, _, same = device_grid(k)
    assert not torch.isnan(got).any(), "an element of hr_coord was not written"
    want = query_grid_host(_plan(k), B)
    n_diff = int((got != want).sum())
    print(f"[query_grid {SHAPES[k]}] elements that differ from query_grid_host: {n_diff}")
    assert torch.equal(got, want), n_diff
    assert same, "two calls gave different bits"


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_query_grid_vs_pad_for_multi_train(k):
    check_grid(device_grid(k)[0], host_coord(k)[0], RESIZED[k], f"device {SHAPES[k]}")


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_query_grid_row_length_is_found_on_the_device(k):
    assert device_grid(k)[1] == SHAPES[k][1]


def test_query_grid_fixed_protocol():
    from anystereo import ops
    from anystereo.harness.query import pad_for_multi_train_fixed, query_plan
    for h, w, scale, div in [(37, 53, 3, 16), (40, 64, 2, 16)]:
        z = torch.zeros(1, 3, h, w)
        _, _, coord, _ = pad_for_multi_train_fixed(z, z, scale, divis_by=div)
        check_grid(ops.query_grid(query_plan(h, w, scale, div, fixed=True), B, DEV).cpu(), coord, False, f"fixed {h}x{w} x{scale}")


def _pair(fx, k):
    return fx[f"c{k}_image1"].to(DEV), fx[f"c{k}_image2"].to(DEV)


@pytest.mark.parametrize("k", range(5))
def test_prepare_pair_vs_reference_fixture(fx, k):
    from anystereo import ops
    pl = _plan(k)
    u1, u2 = _pair(fx, k)
    _nan_then_free(B * 3 * pl.h_pad * pl.w_pad, count=2)
    got = ops.prepare_pair(u1, u2, pl)
    again = ops.prepare_pair(u1, u2, pl)
    as_float = ops.prepare_pair(u1.float(), u2.float(), pl)
    for i, name in enumerate(("1", "2")):
        want = fx[f"c{k}_pad{name}"]
        g = got[i].cpu()
        assert g.dtype == torch.float32 and g.shape == want.shape and got[i].is_contiguous()
        assert not torch.isnan(g).any(), "an element of the padded image was not written"
        d = (g - want).abs().max().item()
        print(f"[prepare_pair {SHAPES[k]} image{name}] max |d| vs the reference = {d:.3e}")
        assert d <= IMAGE_TOL, (k, name, d)
        assert torch.equal(got[i], again[i]), "two calls gave different bits"
        assert torch.equal(got[i], as_float[i]), "uint8 input and the same values as fp32 gave different bits"
        if SHAPES[k][2] == 1.0:
            f = torch.nn.functional.pad(fx[f"c{k}_image{name}"].float(), [pl.pad[2], pl.pad[3], pl.pad[0], pl.pad[1]], mode="replicate")
            assert torch.equal(g, f)
    assert not torch.equal(got[0][0], got[0][1]) and not torch.equal(got[0], got[1])


def test_prepare_pair_kitti_size_vs_host_path():
    """375x1242 x2.0: 10 x 48 blocks per batch element.  The reference here is the project's host path (the reference's function
    stated with the same ATen calls), on the CPU."""
    from anystereo import ops
    from anystereo.harness.query import pad_for_multi_train
    k = 5
    h, w, s, div = SHAPES[k]
    pl = _plan(k)
    g = torch.Generator().manual_seed(77)
    u1 = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    u2 = torch.randint(0, 256, (B, 3, h, w), generator=g, dtype=torch.uint8)
    w1, w2, _, _ = pad_for_multi_train(u1.float(), u2.float(), s, divis_by=div)
    _nan_then_free(B * 3 * pl.h_pad * pl.w_pad, count=2)
    got = ops.prepare_pair(u1.to(DEV), u2.to(DEV), pl)
    as_float = ops.prepare_pair(u1.float().to(DEV), u2.float().to(DEV), pl)
    for i, want in enumerate((w1, w2)):
        gi = got[i].cpu()
        assert gi.shape == want.shape and not torch.isnan(gi).any()
        d = (gi - want).abs().max().item()
        print(f"[prepare_pair {SHAPES[k]} image{i + 1}] max |d| vs the host path = {d:.3e}")
        assert d <= IMAGE_TOL, (i, d)
        assert torch.equal(got[i], as_float[i])


def test_prepare_pair_fixed_protocol_is_a_pad(fx):
    from anystereo import ops
    from anystereo.harness.query import pad_for_multi_train_fixed, query_plan
    img1, img2 = fx["c2_image1"].float(), fx["c2_image2"].float()  # 37x53, divis_by 16 -> 48x64
    w1, w2, _, p = pad_for_multi_train_fixed(img1, img2, 3, divis_by=16)
    pl = query_plan(37, 53, 3, 16, fixed=True)
    g1, g2 = ops.prepare_pair(img1.to(DEV), img2.to(DEV), pl)
    assert torch.equal(g1.cpu(), w1) and torch.equal(g2.cpu(), w2) and list(pl.p) == p


def test_prepare_on_device_and_registered_operators(fx):
    import anystereo  # noqa: F401
    from anystereo import ops
    from anystereo.harness.query import prepare_on_device, query_plan
    for k in (0, 2, 3):
        h, w, s, div = SHAPES[k]
        pl = _plan(k)
        u1, u2 = _pair(fx, k)
        a1, a2 = ops.prepare_pair(u1, u2, pl)
        grid = ops.query_grid(pl, B, DEV)
        t1, t2 = torch.ops.anystereo.prepare_pair(u1, u2, s, div, False)
        assert torch.equal(t1, a1) and torch.equal(t2, a2)
        assert torch.equal(torch.ops.anystereo.query_grid(u1, s, div, False), grid)
        d1, d2, coord, p = prepare_on_device(u1, u2, s, divis_by=div)
        assert torch.equal(d1, a1) and torch.equal(d2, a2) and torch.equal(coord, grid) and p == list(pl.p)
    u1, u2 = _pair(fx, 2)
    pl = query_plan(37, 53, 3, 16, fixed=True)
    t1, _ = torch.ops.anystereo.prepare_pair(u1, u2, 3.0, 16, True)
    assert torch.equal(t1, ops.prepare_pair(u1, u2, pl)[0])
    assert torch.equal(torch.ops.anystereo.query_grid(u1, 3.0, 16, True), ops.query_grid(pl, B, DEV))
    d1, _, coord, p = prepare_on_device(u1, u2, 3, divis_by=16, fixed=True)
    assert torch.equal(d1, t1) and tuple(coord.shape) == (B, 37 * 3 * 53 * 3, 2) and p == list(pl.p)


def test_kernels_can_be_captured_in_a_graph(fx):
    """Both launches run on the caller's stream without synchronising or allocating beyond their outputs: a captured replay gives the
    bits of the eager call."""
    from anystereo import ops
    k = 2
    pl = _plan(k)
    u1, u2 = _pair(fx, k)
    want = ops.prepare_pair(u1, u2, pl) + (ops.query_grid(pl, B, DEV),)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = ops.prepare_pair(u1, u2, pl) + (ops.query_grid(pl, B, DEV),)
    for t in got:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for g, w_ in zip(got, want):
        assert torch.equal(g, w_)


def test_refusals():
    from anystereo import ops
    from anystereo.harness.query import QueryPlan, query_plan
    pl = query_plan(8, 16, 1.5, 32)
    g = torch.zeros(2, 3, 8, 16, device=DEV)
    c = torch.zeros(2, 3, 8, 16)
    with pytest.raises(RuntimeError, match="prepare_pair.*CUDA"):
        ops.prepare_pair(c, c, pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*CUDA"):
        ops.prepare_pair(g, c, pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*uint8 or float32"):
        ops.prepare_pair(g.half(), g.half(), pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*uint8 or float32"):
        ops.prepare_pair(g.double(), g.double(), pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*contiguous"):
        ops.prepare_pair(g.transpose(2, 3), g.transpose(2, 3), pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*must share"):
        ops.prepare_pair(g, torch.zeros(2, 3, 8, 15, device=DEV), pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*must share"):
        ops.prepare_pair(g, g.to(torch.uint8), pl)
    with pytest.raises(RuntimeError, match=r"prepare_pair.*\[B,3,H,W\]"):
        ops.prepare_pair(g[:, :1].contiguous(), g[:, :1].contiguous(), pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*plan"):
        ops.prepare_pair(g, g, query_plan(8, 17, 1.5, 32))
    with pytest.raises(RuntimeError, match="prepare_pair.*empty"):
        ops.prepare_pair(g[:0], g[:0], pl)
    with pytest.raises(RuntimeError, match="query_grid.*CUDA"):
        ops.query_grid(pl, 2, "cpu")
    with pytest.raises(RuntimeError, match="query_grid.*batch"):
        ops.query_grid(pl, 0, DEV)
    with pytest.raises(RuntimeError, match="query_grid.*empty"):
        ops.query_grid(pl._replace(p=(pl.h_hr, 0, 0, 0)), 2, DEV)
    with pytest.raises(RuntimeError, match="query_grid.*2\\^31-1"):
        ops.query_grid(query_plan(32768, 32768, 1.0, 32), 1, DEV)
    with pytest.raises(RuntimeError, match="query_grid.*65535"):  # the C entry's own refusal
        ops.query_grid(query_plan(8, 16, 1.0, 8), 65536, DEV)
    assert isinstance(pl, QueryPlan)
    with pytest.raises(RuntimeError, match="query_plan.*integer"):
        query_plan(8, 16, 2.5, 16, fixed=True)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.anystereo.prepare_pair(c, c, 1.5, 32, False)


# ---- end to end -------------------------------------------------------------------------------------------------------------

class _Recorder(torch.nn.Module):
    """Keeps what the wrapped model received and returned."""

    def __init__(self, model):
        super().__init__()
        self.model, self.preds, self.inputs = model, [], []

    def forward(self, image1, image2, **kwargs):
        self.inputs.append((image1.detach().clone(), image2.detach().clone(), kwargs["hr_coord"].detach().clone()))
        out = self.model(image1, image2, **kwargs)
        self.preds.append(out.detach().clone())
        return out


@pytest.fixture(scope="module")
def igev():
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models import __models__, default_args
    model = __models__["continuous_IGEVStereo"](default_args("continuous_IGEVStereo")).eval()
    fill_module_deterministic(model, base_seed=1)
    return model.to(DEV)


def _pairs(h, w, as_uint8=False, rounded=False):
    """The pairs of test_evaluate_end_to_end (known disparity 6, seeds 7 and 8, all-ones masks)."""
    from anystereo.harness.synthetic import synthetic_pair
    out = []
    for seed in (7, 8):
        i1, i2 = synthetic_pair(1, h, w, shift=6, seed=seed)
        if rounded or as_uint8:
            i1, i2 = i1.round(), i2.round()
        if as_uint8:
            i1, i2 = i1.to(torch.uint8), i2.to(torch.uint8)
        out.append((i1.to(DEV), i2.to(DEV), torch.full((1, h, w), 6.0, device=DEV), torch.ones(1, h, w, device=DEV),
                    torch.ones(1, h, w, dtype=torch.uint8, device=DEV)))
    return out


def _run(model, pairs, scale, prep):
    from anystereo.harness import evaluate as E
    rec = _Recorder(model)
    res = E.evaluate(rec, pairs, scale=scale, iters=2, protocol="kitti", prep=prep)
    assert res["pairs"] == 2 and len(rec.preds) == 2
    return res, rec


def test_evaluate_device_prep_vs_host_prep_scale_1p5(igev):
    """IGEV, deterministic fill, 2 iterations, 64x128 x1.5: the mean absolute difference of the predictions is below 1e-3 px (the
    project's parity bound), every count of the `images` block identical."""
    h, w = 64, 128
    host, rec_h = _run(igev, _pairs(h, w), 1.5, "host")
    dev, rec_d = _run(igev, _pairs(h, w), 1.5, "device")
    assert dev["images"] == host["images"] == {"seen": 2, "all": 2, "noc": 2, "occ": 0}
    for i, (a, b) in enumerate(zip(rec_d.preds, rec_h.preds)):
        assert a.shape == b.shape == (1, 1, h * w) and torch.isfinite(a).all()
        d_img = (rec_d.inputs[i][0] - rec_h.inputs[i][0]).abs().max().item()
        d_grid = (rec_d.inputs[i][2] - rec_h.inputs[i][2]).abs().max().item()
        mad = (a - b).abs().mean().item()
        print(f"[evaluate x1.5 pair {i}] padded image max |d| {d_img:.3e}, grid max |d| {d_grid:.3e}, prediction mean |d| {mad:.3e} px")
        assert mad < 1e-3, (i, mad)


def test_evaluate_device_prep_equals_host_prep_at_scale_1(igev):
    """At scale 1.0 the two paths' padded images and grids are bit-identical, so the predictions are."""
    h, w = 40, 128  # rows padded 12/12 -> 64 x 128
    host, rec_h = _run(igev, _pairs(h, w), 1.0, "host")
    dev, rec_d = _run(igev, _pairs(h, w), 1.0, "device")
    for ins_d, ins_h, a, b in zip(rec_d.inputs, rec_h.inputs, rec_d.preds, rec_h.preds):
        for x, y in zip(ins_d, ins_h):
            assert torch.equal(x, y)
        assert torch.equal(a, b)
    assert dev["images"] == host["images"]
    for region in ("all", "noc", "occ"):
        assert dev[region] == host[region]


def test_evaluate_device_prep_uint8_equals_float(igev):
    h, w = 64, 128
    as_float, rec_f = _run(igev, _pairs(h, w, rounded=True), 1.5, "device")
    as_u8, rec_u = _run(igev, _pairs(h, w, as_uint8=True), 1.5, "device")
    for a, b in zip(rec_u.preds, rec_f.preds):
        assert torch.equal(a, b)
    assert as_u8["images"] == as_float["images"]
    for region in ("all", "noc", "occ"):
        assert as_u8[region] == as_float[region]
