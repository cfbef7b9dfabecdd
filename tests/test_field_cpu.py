"""CPU: the host side of StereoField / the interpolation baseline — the plain-torch restatement of csrc/resize_disp.hip
(`query.resize_disparity_host`) against the reference's own `multi_evaothers` statements (tests/golden/resize_disp.npz, written by
tests/golden/make_golden_resize.py), the argument checks of as_resize_disp (no launch happens), the command line of tools/evaluate.py
and the labels of evaluate(curve=, baseline=) with a stub model.

Limit of the resize: IMAGE_TOL / 255 * max|src * mul| with IMAGE_TOL = 1e-3 — tests/test_prepare_cpu.py's limit for the same bicubic
restatement, as a fraction of the value range (a direct fp32 restatement differs from ATen's CPU kernel by about a quarter of it).
Scale 1.0: equal to the crop.  A restatement that clamps its taps to the padded frame instead of the crop misses the limit by four
orders of magnitude on this fixture (its step edge lies on the crop border)."""
import ctypes
import importlib.util
import os

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CASES = [(40, 64, 1.0, 32), (64, 96, 2.0, 32), (37, 53, 1.5, 32), (45, 70, 1.3, 16), (33, 65, 2.95, 32)]
IMAGE_TOL = 1e-3


@pytest.fixture(scope="module")
def fx(golden):
    f = golden("resize_disp")
    assert [tuple(c) for c in f["cases"].tolist()] == [tuple(float(v) for v in s) for s in CASES]
    return f


def case(fx, k):
    """(map [2,1,h_pad,w_pad], crop, size, mul, want [2,H,W], limit) of fixture case k."""
    h, w, s, _ = CASES[k]
    m, want = fx[f"c{k}_map"], fx[f"c{k}_out"][:, 0]
    assert m.dtype == torch.float32 and tuple(want.shape) == (2, h, w) and not torch.equal(m[0], m[1])
    return m, tuple(int(v) for v in fx[f"c{k}_crop"]), (h, w), s, want, IMAGE_TOL / 255 * (m * s).abs().max().item()


def wrong_frame(m, crop, size, mul):
    """resize_disparity_host with the taps clamped to the PADDED frame: what as_resize_disp must not compute."""
    from anystereo.harness import query as Q
    top, left, hc, wc = crop
    x = m[:, 0] * float(mul)

    def axis(n_in, n_out, lo, n_src):
        _, wgt = Q._cubic_axis(n_in, n_out, n_out, 0, "cpu")
        scale = float(torch.tensor(float(n_in)) / torch.tensor(float(n_out)))
        i = (scale * (torch.arange(n_out).float() + 0.5) - 0.5).floor().long()
        return torch.stack([(lo + i - 1 + j).clamp(0, n_src - 1) for j in range(4)]), wgt
    iy, wy = axis(hc, size[0], top, x.shape[1])
    ix, wx = axis(wc, size[1], left, x.shape[2])
    out = 0
    for a in range(4):
        rows = x[:, iy[a]]
        out = out + sum(rows[:, :, ix[b]] * wx[b].view(1, 1, -1) for b in range(4)) * wy[a].view(1, -1, 1)
    return out


@pytest.mark.parametrize("k", range(5))
def test_query_plan_locates_the_fixture_crop(fx, k):
    from anystereo.harness.query import query_plan
    h, w, s, div = CASES[k]
    pl = query_plan(h, w, s, div)
    assert tuple(int(v) for v in fx[f"c{k}_crop"]) == (pl.pad[0], pl.pad[2], pl.h_lr, pl.w_lr)
    assert tuple(fx[f"c{k}_map"].shape) == (2, 1, pl.h_pad, pl.w_pad)


@pytest.mark.parametrize("k", range(5))
def test_resize_disparity_host_vs_reference_fixture(fx, k):
    from anystereo.harness.query import resize_disparity_host
    m, crop, size, s, want, lim = case(fx, k)
    got = resize_disparity_host(m, crop, size, s)
    assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
    d = (got - want).abs().max().item()
    print(f"[resize_disparity_host {size} x{s}] max |d| = {d:.3e} (limit {lim:.3e}), values {want.min().item():.1f} .. {want.max().item():.1f}")
    if s == 1.0:
        top, left, hc, wc = crop
        assert torch.equal(got, m[:, 0, top:top + hc, left:left + wc]) and torch.equal(got, want)
    else:
        assert d <= lim, (k, d, lim)
        assert want.min().item() < -3 * s and want.max().item() > 200 * s  # the overshoot of the bicubic kernel is kept
    assert torch.equal(resize_disparity_host(m[:, 0], crop, size, s), got)  # [N,Hs,Ws] and [N,1,Hs,Ws]: the same


@pytest.mark.parametrize("k", range(1, 5))
def test_fixture_tells_the_crop_from_the_padded_frame(fx, k):
    m, crop, size, s, want, lim = case(fx, k)
    d = (wrong_frame(m, crop, size, s) - want).abs().max().item()
    print(f"[taps clamped to the padded frame {size} x{s}] max |d| = {d:.3e} (limit {lim:.3e})")
    assert d > lim
    # the same code with the crop as its own frame is the restatement: the difference above is the clamping alone
    top, left, hc, wc = crop
    inner = m[:, :, top:top + hc, left:left + wc].contiguous()
    assert (wrong_frame(inner, (0, 0, hc, wc), size, s) - want).abs().max().item() <= lim


def test_identity_copies_the_crop_times_mul():
    from anystereo.harness.query import resize_disparity_host
    x = torch.arange(2 * 7 * 9, dtype=torch.float32).view(2, 7, 9) / 7
    assert torch.equal(resize_disparity_host(x, (1, 2, 5, 6), (5, 6), 1.0), x[:, 1:6, 2:8])
    assert torch.equal(resize_disparity_host(x, (1, 2, 5, 6), (5, 6), 1.3), x[:, 1:6, 2:8] * 1.3)


def test_abi_argument_validation_without_gpu():
    """NULL pointers, non-positive sizes -> AS_ERR_BAD_ARG (-1); an empty crop, a crop outside the source, N above 65535 ->
    AS_ERR_BAD_SHAPE (-2); all before any launch.  The new entry extends the ABI: its number stays."""
    from anystereo import _lib
    lib = _lib.load()
    assert lib.as_abi_version() == 38
    buf = (ctypes.c_float * 64)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)

    def call(src=p, out=p, n=1, hs=8, ws=8, top=1, left=1, hc=4, wc=4, h=6, w=6, mul=1.5):
        return lib.as_resize_disp(src, out, n, hs, ws, top, left, hc, wc, h, w, mul, null)

    def msg():
        return lib.as_last_error_string().decode()

    for name in ("src", "out"):
        assert call(**{name: null}) == -1 and "resize_disp: null pointer" in msg()
    for name in ("n", "hs", "ws", "h", "w"):
        for v in (0, -2):
            assert call(**{name: v}) == -1 and "non-positive" in msg(), (name, v)
    for name in ("hc", "wc"):
        for v in (0, -1):
            assert call(**{name: v}) == -2 and "empty crop" in msg(), (name, v)
    for bad in (dict(top=-1), dict(left=-1), dict(top=5), dict(left=5), dict(hc=8), dict(wc=9), dict(top=2 ** 31 - 1)):
        assert call(**bad) == -2 and "leaves" in msg(), bad
    assert call(n=65536) == -2 and "65535" in msg()
    assert call(h=262141) == -2


def test_ops_refuse_cpu_tensors():
    import anystereo  # noqa: F401
    from anystereo import ops
    z = torch.zeros(1, 8, 8)
    with pytest.raises(RuntimeError, match="resize_disparity.*CUDA"):
        ops.resize_disparity(z, (0, 0, 4, 4), (6, 6), 1.5)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.anystereo.resize_disparity(z, [0, 0, 4, 4], [6, 6], 1.5)


def test_encode_refusals_that_need_no_gpu():
    from anystereo.models import __models__, default_args
    from anystereo.models.field import normalize_at
    assert normalize_at(None, 4) == (4,) and normalize_at((2, 1, 2), 4) == (1, 2, 4) and normalize_at([4], 4) == (4,)
    for bad in ((0,), (5,), (1, 9), (-1,), (1.5,)):
        with pytest.raises(ValueError, match="outside"):
            normalize_at(bad, 4)
    with pytest.raises(ValueError, match="iterable"):
        normalize_at(3, 4)
    model = __models__["continuous_RAFTStereo"](default_args("continuous_RAFTStereo"))
    z = torch.zeros(1, 3, 32, 32)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="training mode"):
            model.train().encode(z, z, iters=2)
        with pytest.raises(RuntimeError, match="CUDA"):
            model.eval().encode(z, z, iters=2)
    with pytest.raises(RuntimeError, match="gradients are enabled"):
        model.eval().encode(z, z, iters=2)


def _tool():
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(ROOT, "tools", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    return ev


def test_evaluate_tool_parses_curve_and_baseline():
    ev = _tool()
    a = ev.parse_args(["--pairs", "1", "--iters", "32", "--curve", "4,8,16,32", "--baseline", "bicubic"])
    assert a.curve == (4, 8, 16, 32) and a.baseline == "bicubic"
    a = ev.parse_args(["--pairs", "1"])
    assert a.curve is None and a.baseline is None
    for bad in (["--iters", "8", "--curve", "4,16"], ["--curve", "0,4"], ["--curve", "8,4"], ["--curve", "4,x"], ["--baseline", "bilinear"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)


class _StubField:
    """query(at=k) answers the constant k; the scale-1 query of the baseline answers the last iteration's constant."""

    def __init__(self, at, log):
        self.at, self.log = tuple(at), log

    def query(self, hr_coord, scale, at=None):
        k = self.at[-1] if at is None else at
        assert k in self.at
        self.log.append((k, hr_coord.shape[1], float(scale.reshape(-1)[0])))
        return torch.full((hr_coord.shape[0], 1, hr_coord.shape[1]), float(k))


class _StubModel:
    def __init__(self):
        self.encodes, self.queries = [], []

    def eval(self):
        return self

    def encode(self, image1, image2, iters=32, at=None):
        self.encodes.append((tuple(image1.shape), iters, tuple(at)))
        return _StubField(at, self.queries)


def test_evaluate_labels_curve_and_baseline_with_a_stub_model():
    from anystereo.harness.evaluate import evaluate
    from anystereo.harness.query import query_plan
    h, w, s = 45, 70, 1.3
    img = torch.zeros(1, 3, h, w)
    gt = torch.full((1, h, w), 6.0)
    pairs = [(img, img, gt, torch.ones(1, h, w), torch.ones(1, h, w, dtype=torch.uint8))] * 2
    model = _StubModel()
    res = evaluate(model, pairs, scale=s, iters=4, protocol="kitti", divis_by=16, curve=(2, 4), baseline="bicubic")
    pl = query_plan(h, w, s, 16)
    assert res["estimates"] == ["iter2", "iter4", "bicubic"] and res["pairs"] == 2 and res["images"]["seen"] == 2
    assert model.encodes == [((1, 3, pl.h_pad, pl.w_pad), 4, (2, 4))] * 2          # one encoded pass per batch
    assert model.queries[:3] == [(2, h * w, pytest.approx(s)), (4, h * w, pytest.approx(s)), (4, pl.h_pad * pl.w_pad, 1.0)]
    epe = res["all"]["EPE"]
    assert len(epe) == 3 and epe[0] == pytest.approx(4.0) and epe[1] == pytest.approx(2.0)
    assert epe[2] == pytest.approx(6.0 - 4 * s, abs=1e-4)                        # bicubic of the constant 4 * scale
    only = evaluate(_StubModel(), pairs[:1], scale=s, iters=4, protocol="kitti", divis_by=16, baseline="bicubic")
    assert only["estimates"] == ["iter4", "bicubic"]
    curve = evaluate(_StubModel(), pairs[:1], scale=s, iters=4, protocol="kitti", divis_by=16, curve=(1, 3))
    assert curve["estimates"] == ["iter1", "iter3"] and len(curve["all"]["EPE"]) == 2
    for bad in ((0, 4), (5,), (4, 2), ()):
        with pytest.raises(ValueError, match="curve"):
            evaluate(_StubModel(), pairs[:1], scale=s, iters=4, protocol="kitti", divis_by=16, curve=bad)
    with pytest.raises(ValueError, match="baseline"):
        evaluate(_StubModel(), pairs[:1], scale=s, iters=4, protocol="kitti", divis_by=16, baseline="bilinear")
