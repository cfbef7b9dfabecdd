"""GPU (-m gpu): the picture kernel (csrc/eval_images.hip) — `ops.disparity_images` against the plain-torch restatement of
harness/images.py and against the reference's own pictures (tests/golden/eval_images.npz), exact in every byte; its registered
operator, and `evaluate()` with an ImageSink end to end.

The four fixture shapes take every path of the kernel: 2 x 13 x 37 = 962 pixels leave two for the byte-store tail, the second image
starts at an odd flat pixel (a thread's four pixels straddle both images) and the legend is clipped at x = 37; 1 x 7 x 250 clips the
legend by the height and ends it at x = 200; 2 x 24 x 203 is a multiple of four with the whole legend; 1 x 1 x 5 is one group of
four and one tail pixel."""
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(2, 13, 37, 192.0), (1, 7, 250, 192.0), (2, 24, 203, 400.0), (1, 1, 5, 192.0)]
FILL = 0xA5
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]  # (color, error, enc16)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("eval_images")


@pytest.fixture(scope="module")
def want(fx):
    """Per case, computed once on the host: the quantised restatement of both inputs and the quantised fixture."""
    from anystereo.harness import images as I
    out = []
    for k, (b, h, w, md) in enumerate(CASES):
        disp, est, gt = fx[f"c{k}_disp"], fx[f"c{k}_est"], fx[f"c{k}_gt"]
        out.append({"color": I.quantize_host(I.disp_to_color_host(disp, md)), "color_est": I.quantize_host(I.disp_to_color_host(est, md)),
                    "error": I.quantize_host(I.error_image_host(est, gt)), "error_disp": I.quantize_host(I.error_image_host(disp, gt)),
                    "enc16": I.encode16_host(disp), "enc16_est": I.encode16_host(est),
                    "fx_color": I.quantize_host(fx[f"c{k}_color"]), "fx_error": I.quantize_host(fx[f"c{k}_error"])})
    return out


def _run(disp, gt, md, subset):
    """The kernel into buffers pre-filled with 0xA5 (an unwritten byte shows) -> (color, error, enc16) on the host, None where not asked."""
    from anystereo import ops
    b, h, w = disp.shape
    bufs = [torch.full((b, h, w, c), FILL, dtype=torch.uint8, device=DEV) if on else None for on, c in zip(subset, (3, 3, 2))]
    ops.disparity_images_out(disp, gt, bufs[0], bufs[1], bufs[2], md)
    return [None if t is None else t.cpu() for t in bufs]


@pytest.mark.parametrize("k", range(4))
def test_every_subset_equals_restatement_and_reference(fx, want, k):
    b, h, w, md = CASES[k]
    disp, est, gt = (fx[f"c{k}_{n}"].to(DEV) for n in ("disp", "est", "gt"))
    wk = want[k]
    assert torch.equal(wk["color"], wk["fx_color"]) and torch.equal(wk["error"], wk["fx_error"])  # the yardsticks agree
    for subset in SUBSETS:
        c, e, n = _run(disp, gt, md, subset)
        assert (c is not None, e is not None, n is not None) == subset
        if c is not None:
            assert torch.equal(c, wk["color"]) and torch.equal(c, wk["fx_color"]), (k, subset, "color", int((c != wk["fx_color"]).sum()))
        if e is not None:
            assert torch.equal(e, wk["error_disp"]), (k, subset, "error", int((e != wk["error_disp"]).sum()))
        if n is not None:
            assert torch.equal(n, wk["enc16"]), (k, subset, "enc16", int((n != wk["enc16"]).sum()))
        # the estimate with NaN and +-inf: the error picture of the fixture; colour and enc16 treat NaN as black / 0
        c, e, n = _run(est, gt, md, subset)
        if c is not None:
            assert torch.equal(c, wk["color_est"]), (k, subset, "color of est")
        if e is not None:
            assert torch.equal(e, wk["error"]) and torch.equal(e, wk["fx_error"]), (k, subset, "error", int((e != wk["fx_error"]).sum()))
        if n is not None:
            assert torch.equal(n, wk["enc16_est"]), (k, subset, "enc16 of est")
    # without gt: colour and enc16 alone
    c, e, n = _run(disp, None, md, (True, False, True))
    assert torch.equal(c, wk["fx_color"]) and torch.equal(n, wk["enc16"])


@pytest.mark.parametrize("k", range(4))
def test_public_op_defaults_and_shapes(fx, want, k):
    from anystereo import ops
    b, h, w, md = CASES[k]
    est, gt = fx[f"c{k}_est"].to(DEV), fx[f"c{k}_gt"].to(DEV)
    c, e, n = ops.disparity_images(est, gt, md)  # error=None: "when gt is given"
    assert n is None and c.dtype == torch.uint8 and tuple(c.shape) == (b, h, w, 3) and tuple(e.shape) == (b, h, w, 3) and c.is_cuda
    assert torch.equal(c.cpu(), want[k]["color_est"]) and torch.equal(e.cpu(), want[k]["fx_error"])
    c, e, n = ops.disparity_images(est, None, md, enc16=True)
    assert e is None and tuple(n.shape) == (b, h, w, 2) and torch.equal(n.cpu(), want[k]["enc16_est"])
    c, e, n = ops.disparity_images(est.unsqueeze(1), gt.unsqueeze(1), md, color=False)  # [B,1,H,W]
    assert c is None and n is None and torch.equal(e.cpu(), want[k]["fx_error"])
    c2, e2, n2 = ops.disparity_images(est, gt, md, color=False, error=False, enc16=True)
    assert c2 is None and e2 is None and torch.equal(n2.cpu(), want[k]["enc16_est"])


@pytest.mark.parametrize("k", range(4))
def test_inputs_off_the_16_byte_boundary_give_the_same_bytes(fx, want, k):
    """A view one element into a buffer is 4-byte but not 16-byte aligned: the scalar-load path."""
    b, h, w, md = CASES[k]
    n = b * h * w

    def shifted(t):
        buf = torch.empty(n + 1, device=DEV)
        buf[1:] = t.reshape(-1).to(DEV)
        v = buf[1:].view(b, h, w)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    c, e, s = _run(shifted(fx[f"c{k}_est"]), shifted(fx[f"c{k}_gt"]), md, (True, True, True))
    assert torch.equal(c, want[k]["color_est"]) and torch.equal(e, want[k]["fx_error"]) and torch.equal(s, want[k]["enc16_est"])
    # only one of the two off the boundary
    c, e, s = _run(fx[f"c{k}_disp"].to(DEV), shifted(fx[f"c{k}_gt"]), md, (True, True, False))
    assert torch.equal(c, want[k]["fx_color"]) and torch.equal(e, want[k]["error_disp"])


def test_output_off_the_4_byte_boundary_is_refused(fx):
    from anystereo import ops
    b, h, w, md = CASES[0]
    disp, gt = fx["c0_disp"].to(DEV), fx["c0_gt"].to(DEV)
    for which, c in ((0, 3), (1, 3), (2, 2)):
        buf = torch.zeros(b * h * w * c + 1, dtype=torch.uint8, device=DEV)
        view = buf[1:].view(b, h, w, c)
        outs = [None, None, None]
        outs[which] = view
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            ops.disparity_images_out(disp, gt, outs[0], outs[1], outs[2], md)
        assert int(buf.sum()) == 0  # refused before the launch


NARROW = [(2, 11, 3), (1, 15, 1), (1, 12, 4), (1, 19, 1), (3, 11, 9), (1, 10, 7), (1, 9, 7), (2, 29, 2), (1, 200, 1)]


@pytest.mark.parametrize("shape", NARROW)
def test_legend_stops_after_ten_rows_of_a_narrow_image(shape):
    """H > 10 with W < 10: 10 * W <= H * W < 10 * W + 10 for several of these, where a floored H * W / 10 would let the legend run
    on into row 10.  The rows below the legend carry their own band (or black for gt <= 0); every byte equals the host restatement."""
    from anystereo import ops
    from anystereo.harness import images as I
    from anystereo.harness.synthetic import det_uniform
    b, h, w = shape
    gt = det_uniform((b, h, w), 61, -10.0, 120.0)
    est = gt + det_uniform((b, h, w), 62, -1.0, 1.0) * torch.exp(det_uniform((b, h, w), 63, -3.0, 4.0))
    want = I.quantize_host(I.error_image_host(est, gt))
    if h > 10:
        assert (want[:, 10:].reshape(-1, 3) != torch.tensor(I.ERROR_BANDS[0], dtype=torch.uint8)).any()  # not legend-coloured
    c, e, n = ops.disparity_images(est.to(DEV), gt.to(DEV), enc16=True)
    assert torch.equal(e.cpu(), want), (shape, int((e.cpu() != want).sum()))
    assert torch.equal(c.cpu(), I.quantize_host(I.disp_to_color_host(est, 192.0))) and torch.equal(n.cpu(), I.encode16_host(est))


def test_540x960_exact_and_repeatable():
    """cfg-2's output size: 2025 blocks.  Seeded inputs with holes in gt, values beyond both ends of the colour map, and a sprinkle of
    NaN / inf estimates; every byte equals the host restatement, and a second call gives the same bytes."""
    from anystereo import ops
    from anystereo.harness import images as I
    from anystereo.harness.synthetic import det_uniform
    h, w, md = 540, 960, 192.0
    gt = det_uniform((1, h, w), 21, -20.0, 200.0)
    est = gt + det_uniform((1, h, w), 22, -1.0, 1.0) * torch.exp(det_uniform((1, h, w), 23, -3.0, 4.0))
    flat = est.view(-1)
    flat[1000::7919] = float("nan")
    flat[2000::7919] = float("inf")
    flat[3000::7919] = float("-inf")
    a = ops.disparity_images(est.to(DEV), gt.to(DEV), md, enc16=True)
    b = ops.disparity_images(est.to(DEV), gt.to(DEV), md, enc16=True)
    wants = (I.quantize_host(I.disp_to_color_host(est, md)), I.quantize_host(I.error_image_host(est, gt)), I.encode16_host(est))
    for name, x, y, wnt in zip(("color", "error", "enc16"), a, b, wants):
        assert torch.equal(x, y), name
        assert torch.equal(x.cpu(), wnt), (name, int((x.cpu() != wnt).sum()))


def test_registered_operator_returns_what_ops_returns(fx):
    import anystereo  # noqa: F401
    from anystereo import ops
    md = CASES[0][3]
    est, gt = fx["c0_est"].to(DEV), fx["c0_gt"].to(DEV)
    got = torch.ops.anystereo.disparity_images(est, gt, md, True, None, True, 3.0, 0.05)
    for g, w in zip(got, ops.disparity_images(est, gt, md, True, None, True)):
        assert torch.equal(g, w)
    got = torch.ops.anystereo.disparity_images(est, None, 400.0, True, None, False, 3.0, 0.05)
    w = ops.disparity_images(est, None, 400.0)
    assert got[1] is None and got[2] is None and w[1] is None and torch.equal(got[0], w[0])
    got = torch.ops.anystereo.disparity_images(est, gt, md, False, True, False, 2.0, 0.1)
    assert got[0] is None and torch.equal(got[1], ops.disparity_images(est, gt, md, color=False, abs_thres=2.0, rel_thres=0.1)[1])


def test_other_thresholds_equal_restatement(fx):
    from anystereo import ops
    from anystereo.harness import images as I
    est, gt = fx["c2_est"], fx["c2_gt"]
    _, e, _ = ops.disparity_images(est.to(DEV), gt.to(DEV), color=False, abs_thres=1.0, rel_thres=0.125)
    assert torch.equal(e.cpu(), I.quantize_host(I.error_image_host(est, gt, 1.0, 0.125)))


class _Recorder(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model, self.preds = model, []

    def forward(self, *args, **kwargs):
        out = self.model(*args, **kwargs)
        self.preds.append(out.detach().clone())
        return out


def test_evaluate_with_image_sink_end_to_end(tmp_path):
    """The configuration of test_eval_metrics_gpu.py's end-to-end test (IGEV, deterministic fill, 64 x 128, scale 1.5, 2 iterations):
    the files decode to the bytes of ops.disparity_images on the same predictions, and the metrics are those of a run without a sink."""
    from anystereo import ops
    from anystereo.harness import evaluate as E
    from anystereo.harness import images as I
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
    plain = E.evaluate(model, pairs, scale=s, iters=iters, protocol="kitti")
    assert "images_written" not in plain
    rec = _Recorder(model)
    sink = I.ImageSink(str(tmp_path), enc16=True)
    res = E.evaluate(rec, pairs, scale=s, iters=iters, protocol="kitti", images=sink)
    assert res["images_written"] == 6 and res["pairs"] == 2
    for key in ("all", "noc", "occ", "images"):
        assert res[key] == plain[key], key  # bit-identical metrics
    assert sorted(os.listdir(str(tmp_path))) == sorted(f"{kind}_{i:06d}.png" for kind in ("disp", "error", "disp16") for i in range(2))
    for i, (pred, pair) in enumerate(zip(rec.preds, pairs)):
        c, e, n = ops.disparity_images(pred.reshape(1, h, w), pair[2], 192.0, enc16=True)
        for kind, t in (("disp", c), ("error", e), ("disp16", n)):
            assert np.array_equal(I.read_png(str(tmp_path / f"{kind}_{i:06d}.png")), t[0].cpu().numpy()), (kind, i)


def test_refusals():
    from anystereo import ops
    g = torch.zeros(2, 8, 16, device=DEV)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_images(torch.zeros(2, 8, 16))
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_images(g, torch.zeros(2, 8, 16))
    with pytest.raises(RuntimeError, match="needs gt"):
        ops.disparity_images(g, error=True)
    with pytest.raises(RuntimeError, match="does not match"):
        ops.disparity_images(g, torch.zeros(2, 8, 15, device=DEV))
    for bad in (0.0, -192.0, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="max_disp"):
            ops.disparity_images(g, max_disp=bad)
    with pytest.raises(RuntimeError, match="rel_thres"):
        ops.disparity_images(g, g, rel_thres=0.0)
    with pytest.raises(RuntimeError, match="no output"):
        ops.disparity_images(g, color=False)
    with pytest.raises(RuntimeError, match="float32"):
        ops.disparity_images(g.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.disparity_images(g.transpose(1, 2))
    with pytest.raises(RuntimeError, match=r"\[B,H,W\]"):
        ops.disparity_images(torch.zeros(8, 16, device=DEV))
    with pytest.raises(RuntimeError, match="empty"):
        ops.disparity_images(torch.zeros(0, 8, 16, device=DEV))
    with pytest.raises(RuntimeError, match="color must be"):
        ops.disparity_images_out(g, None, torch.zeros(2, 8, 16, 2, dtype=torch.uint8, device=DEV), None, None)
