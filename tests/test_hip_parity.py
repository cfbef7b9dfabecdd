"""GPU (-m gpu): every HIP entry point, called through the C ABI via anystereo.ops, against the CPU
oracle on the same seeded inputs and against the committed golden vectors of the reference.

Tolerances (fp32 path; north_star's end-to-end bar is EPE delta < 1e-3):
  * gathers / lerps / stencils: 2e-5 relative to the tensor's max magnitude (rounding order only)
  * fp32-MFMA convolutions / GEMMs: 1e-5 * sqrt(K)-free bound, written per test (fma-chain order differs
    from the oracle's blocked CPU GEMM)
"""
import os

import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def U(shape, seed, lo=-1.0, hi=1.0):
    from anystereo.harness.synthetic import det_uniform
    return det_uniform(shape, seed, lo, hi)


def close(a, b, rtol=2e-5, atol=1e-6, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values in the HIP result"
    err = (a - b).abs().max().item()
    lim = atol + rtol * b.abs().max().item()
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


@pytest.fixture(params=["fp32", "split"])
def precision(request):
    """Run a test under both matrix-core modes: exact fp32 MFMA and 3 x fp16 split precision."""
    from anystereo import ops
    prev = ops.get_precision()
    ops.set_precision(request.param)
    yield request.param
    ops.set_precision(prev)


def test_native_library_is_loaded():
    from anystereo import _lib
    lib = _lib.load()
    assert lib.as_device_count() >= 1
    with open("/proc/self/maps") as f:
        assert "libanystereo_hip.so" in f.read()


# ---------------------------------------------------------------------------------------------
# a1/a2/a3  volumes + lookup
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,c,h,w1,w2,L", [(2, 96, 3, 20, 20, 2), (1, 96, 2, 21, 21, 2), (1, 256, 2, 37, 37, 4),
                                           (1, 96, 5, 240, 240, 2), (2, 33, 3, 70, 45, 3)])
def test_corr_build_pyramid(b, c, h, w1, w2, L):
    from anystereo import ops
    f1, f2 = U((b, c, h, w1), 1), U((b, c, h, w2), 2)
    lv = ops.corr_build_pyramid(f1.to(DEV), f2.to(DEV), L)
    ref = O.corr_pyramid(O.all_pairs_corr(f1.double(), f2.double()), L)
    for i in range(L):
        close(lv[i], ref[i], rtol=1e-6, atol=2e-6 * c ** 0.5, what=f"corr level {i}")


@pytest.mark.parametrize("mode", ["fp32", "split"])
def test_corr_build_precision_modes(mode):
    """Both matrix-core modes (exact fp32 MFMA / 3 x fp16 split) against the fp64 oracle, with operands
    spanning 6 orders of magnitude (the split keeps 22 significand bits at every scale)."""
    from anystereo import ops
    prev = ops.get_precision()
    try:
        ops.set_precision(mode)
        for (b, c, h, w1, w2, L) in [(1, 96, 3, 70, 70, 2), (1, 256, 2, 40, 33, 4), (1, 40, 2, 33, 20, 1)]:
            f1 = U((b, c, h, w1), 5) * torch.pow(10.0, U((b, c, h, w1), 6, -3, 3))
            f2 = U((b, c, h, w2), 7) * torch.pow(10.0, U((b, c, h, w2), 8, -3, 3))
            lv = ops.corr_build_pyramid(f1.to(DEV), f2.to(DEV), L)
            ref = O.corr_pyramid(O.all_pairs_corr(f1.double(), f2.double()), L)
            # error bound relative to sum |a||b| (the scale of the rounding errors), not to the cancelled sum
            scale = O.all_pairs_corr(f1.abs().double(), f2.abs().double()).max().item()
            for i in range(L):
                err = (lv[i].double().cpu() - ref[i]).abs().max().item()
                assert err <= 2e-6 * scale, f"{mode} level {i}: {err:.3e} vs bound {2e-6 * scale:.3e}"
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("b,g,d,h,w,L", [(2, 8, 48, 3, 20, 2), (1, 8, 48, 4, 70, 2), (1, 4, 17, 2, 33, 3)])
def test_geo_pyramid(b, g, d, h, w, L):
    from anystereo import ops
    gev = U((b, g, d, h, w), 3)
    lv = ops.geo_pyramid(gev.to(DEV), L)
    ref = O.geo_pyramid(gev, L)
    for i in range(L):
        close(lv[i].permute(0, 1, 2, 4, 3), ref[i], 0, 1e-7, what=f"geo level {i}")


def _lookup_case(b, h, w, g, d, L, r, seed, lo, hi):
    from anystereo import ops
    corr = [U((b, h, w, w >> i), seed + i, -3, 3) for i in range(L)]
    geo = [U((b, h, w, g, d >> i), seed + 10 + i, -3, 3) for i in range(L)] if g else None
    disp = U((b, 1, h, w), seed + 20, lo, hi)
    disp.view(-1)[:6] = torch.tensor([0.0, 3.0, 7.5, -0.5, float(w - 1), 1e-7])
    out = ops.geo_corr_lookup([t.permute(0, 1, 2, 4, 3).contiguous().to(DEV) for t in geo] if g else None,
                              [t.to(DEV) for t in corr], disp.to(DEV), r)
    ref = O.geo_corr_lookup([t.double() for t in geo] if g else None, [t.double() for t in corr], disp.double(), r)
    return out, ref


@pytest.mark.parametrize("b,h,w,g,d,L,r", [(2, 3, 20, 8, 48, 2, 4), (1, 5, 37, 0, 0, 4, 4), (1, 7, 70, 8, 48, 2, 4),
                                           (1, 2, 33, 4, 16, 3, 2), (1, 3, 300, 0, 0, 1, 3)])
def test_lookup_vs_oracle(b, h, w, g, d, L, r):
    out, ref = _lookup_case(b, h, w, g, d, L, r, 30, -6.0, w + 6.0)
    close(out, ref, rtol=2e-5, atol=2e-5, what="lookup")


def test_lookup_golden(golden):
    from anystereo import ops
    for tag in ("even", "odd"):
        g = golden(f"lookup_igev_{tag}")
        corr = ops.corr_build_pyramid(g["f1"].to(DEV), g["f2"].to(DEV), 2)
        geo = ops.geo_pyramid(g["gev"].to(DEV), 2)
        close(corr[0], g["corr0"], 1e-5, 1e-5, "corr0")
        close(corr[1], g["corr1"], 1e-5, 1e-5, "corr1")
        close(geo[1].permute(0, 1, 2, 4, 3), g["geo1"], 0, 1e-7, "geo1")
        out = ops.geo_corr_lookup(geo, corr, g["disp"].to(DEV), 4)
        close(out, g["out"], 3e-5, 2e-5, "lookup vs reference")
    g = golden("lookup_raft")
    corr = ops.corr_build_pyramid(g["f1"].to(DEV), g["f2"].to(DEV), 4)
    out = ops.geo_corr_lookup(None, corr, g["disp"].to(DEV), 4)
    close(out, g["out"], 3e-5, 3e-5, "raft lookup vs reference")


def test_lookup_class_api(golden):
    """The reference's corr_block contract: obj(disp [B,1,h,w], coords [B,h,w,1]) -> [B,162,h,w]."""
    from anystereo.models.coreContinuous_IGEV.geometry import Combined_Geo_Encoding_Volume
    g = golden("lookup_igev_even")
    fn = Combined_Geo_Encoding_Volume(g["f1"].to(DEV), g["f2"].to(DEV), g["gev"].to(DEV), num_levels=2, radius=4)
    b, _, h, w = g["disp"].shape
    coords = torch.arange(w, device=DEV).float().reshape(1, 1, w, 1).repeat(b, h, 1, 1)
    out = fn(g["disp"].to(DEV), coords)
    assert out.shape == (b, 162, h, w) and out.is_contiguous() and out.dtype == torch.float32
    close(out, g["out"], 3e-5, 2e-5, "class api")


def test_lookup_backward_is_transpose():
    from anystereo import ops
    b, h, w, g, d, L, r = 1, 3, 24, 8, 48, 2, 4
    corr = [U((b, h, w, w >> i), 40 + i) for i in range(L)]
    geo = [U((b, h, w, d >> i, g), 50 + i) for i in range(L)]
    disp = U((b, 1, h, w), 60, -4.0, w + 4.0)
    gout = U((b, L * 9 * (g + 1), h, w), 61)
    dg, dc = ops.geo_corr_lookup_backward(disp.to(DEV), gout.to(DEV), [tuple(t.shape) for t in geo],
                                          [tuple(t.shape) for t in corr], r)
    cr = [t.clone().double().requires_grad_(True) for t in corr]
    gr = [t.permute(0, 1, 2, 4, 3).clone().double().requires_grad_(True) for t in geo]
    O.geo_corr_lookup(gr, cr, disp.double(), r).backward(gout.double())
    for i in range(L):
        close(dc[i], cr[i].grad, 2e-5, 1e-6, f"d_corr{i}")
        close(dg[i].permute(0, 1, 2, 4, 3), gr[i].grad, 2e-5, 1e-6, f"d_geo{i}")


@pytest.mark.parametrize("tag", ["igev", "raft"])
def test_lookup_backward_accumulates_over_iterations(tag):
    """Several lookups on one pyramid (one per GRU iteration) under autograd: their backward passes add into ONE gradient per
    level (as_geo_corr_lookup_bwd_accum behind grad.LookupAnchor); gradients w.r.t. the feature maps / the geometry volume
    against fp64 autograd of the oracle lookups, including a lookup whose output never reaches the loss and overlapping windows."""
    from anystereo.nn.geometry import Combined_Geo_Encoding_Volume, CorrBlock1D
    b, c, h, w, r = 2, 16, 3, 24, 4
    f1, f2, gev = U((b, c, h, w), 80), U((b, c, h, w), 81), U((b, 8, 48, h, w), 82)
    disps = [U((b, 1, h, w), 83 + i, -3.0, w + 3.0) for i in range(4)]
    disps[2] = disps[0] + 0.25  # windows overlapping those of the first lookup
    L = 2 if tag == "igev" else 4
    a1, a2, ag = _leaf(f1, DEV), _leaf(f2, DEV), _leaf(gev, DEV)
    fn = Combined_Geo_Encoding_Volume(a1, a2, ag, num_levels=L, radius=r) if tag == "igev" else CorrBlock1D(a1, a2, num_levels=L, radius=r)
    outs = [fn(d.to(DEV)) for d in disps]
    gs = [U(tuple(outs[0].shape), 90 + i) for i in range(3)]
    sum((o * g.to(DEV)).sum() for o, g in zip(outs[:3], gs)).backward()
    r1, r2, rg = _leaf(f1, dt=torch.float64), _leaf(f2, dt=torch.float64), _leaf(gev, dt=torch.float64)
    corr = O.corr_pyramid(O.all_pairs_corr(r1, r2), L)
    geo = O.geo_pyramid(rg, L) if tag == "igev" else []
    sum((O.geo_corr_lookup(geo, corr, d.double(), r) * g.double()).sum() for d, g in zip(disps[:3], gs)).backward()
    close(a1.grad, r1.grad, 5e-5, 1e-5, "d f1")
    close(a2.grad, r2.grad, 5e-5, 1e-5, "d f2")
    if tag == "igev":
        close(ag.grad, rg.grad, 2e-5, 1e-6, "d gev")
    assert fn._holder.get("acc") is None, "the shared gradient is released by the anchor's backward"


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 2e-5), (torch.float64, 1e-12), (torch.float16, 8e-3)])
def test_corr_sampler_module(dtype, tol):
    """`corr_sampler.forward/backward` (sampler/sampler.cpp:48-51) incl. zero-pad edges, ragged W2, r != 4."""
    import corr_sampler as top_level  # the reference's extension module name (sampler/sampler.cpp:48-51), any-stereo_amd on sys.path
    from anystereo import corr_sampler
    assert top_level.forward is corr_sampler.forward and top_level.backward is corr_sampler.backward
    for (n, h1, w1, w2, r) in [(2, 3, 20, 20, 4), (1, 2, 33, 17, 3), (1, 1, 5, 1, 4)]:
        vol = U((n, h1, w1, w2), 70, -2, 2).to(dtype)
        coords = torch.stack([U((n, h1, w1), 71, -6.0, w2 + 6.0), torch.zeros(n, h1, w1)], dim=1)
        coords[0, 0, 0, :3] = torch.tensor([0.0, 2.5, float(w2 - 1)])
        (out,) = corr_sampler.forward(vol.to(DEV), coords.to(DEV), r)
        ref = O.corr_sampler_forward(vol.double(), coords, r)
        assert out.dtype == dtype and out.shape == (n, 2 * r + 1, h1, w1)
        close(out, ref, tol, tol, "sampler fwd")
        gr = U(tuple(out.shape), 72).to(dtype)
        (vg,) = corr_sampler.backward(vol.to(DEV), coords.to(DEV), gr.to(DEV), r)
        close(vg, O.corr_sampler_backward(vol.double(), coords, gr.double(), r), tol, tol, "sampler bwd")
    with pytest.raises(RuntimeError):  # CHECK_INPUT semantics (sampler.cpp:20-22)
        corr_sampler.forward(vol, coords.to(DEV), 4)
    with pytest.raises(RuntimeError):
        corr_sampler.forward(vol.to(DEV).transpose(1, 2), coords.to(DEV), 4)


# ---------------------------------------------------------------------------------------------
# a4/a5
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b,c,h,w,d,g", [(1, 96, 3, 60, 48, 8), (2, 96, 2, 130, 48, 8), (1, 32, 2, 20, 50, 4)])
def test_gwc_volume(b, c, h, w, d, g):
    from anystereo import ops
    fl, fr = U((b, c, h, w), 80), U((b, c, h, w), 81)
    out = ops.gwc_volume(fl.to(DEV), fr.to(DEV), d, g)
    close(out, O.gwc_volume(fl.double(), fr.double(), d, g), 1e-6, 1e-6, "gwc")


def test_gwc_dispreg_golden(golden):
    from anystereo import ops
    g = golden("gwc_dispreg")
    close(ops.gwc_volume(g["fl"].to(DEV), g["fr"].to(DEV), 48, 8), g["vol"], 1e-5, 1e-6, "gwc vs reference")
    close(ops.disparity_regression(g["cost"].to(DEV), True), g["init_disp"], 1e-5, 1e-5, "dispreg vs reference")
    close(ops.disparity_regression(torch.softmax(g["cost"], 1).to(DEV), False), g["init_disp"], 1e-5, 1e-5, "dispreg(prob)")


# ---------------------------------------------------------------------------------------------
# a6-a10 convolutions / update block
# ---------------------------------------------------------------------------------------------

def _ref_conv(x, w, bias, pad):
    return torch.nn.functional.conv2d(x.double(), w.double(), None if bias is None else bias.double(), padding=pad)


@pytest.mark.parametrize("b,cins,cout,ks,h,w,act", [
    (1, [128, 128, 128], 128, 3, 8, 12, 1), (2, [64], 64, 3, 9, 33, 1), (1, [128], 127, 3, 7, 20, 1),
    (1, [128], 256, 3, 5, 40, 1), (1, [162], 64, 1, 6, 21, 1), (1, [36], 64, 1, 3, 50, 0),
    (1, [228], 128, 1, 1, 300, 1), (1, [64], 9, 1, 1, 77, 0), (1, [20, 12], 40, 3, 17, 9, 2), (1, [16], 32, 3, 34, 60, 3)])
def test_conv2d_linear(b, cins, cout, ks, h, w, act, precision):
    from anystereo import ops, _lib as L
    cin = sum(cins)
    srcs = [U((b, c, h, w), 90 + i) for i, c in enumerate(cins)]
    wt = U((cout, cin, ks, ks), 95) * (3.0 / (cin * ks * ks)) ** 0.5
    bias = U((cout,), 96) * 0.1
    add = U((b, cout + 5, h, w), 97)
    pk = ops.PackedConv().get([wt.to(DEV)], [bias.to(DEV)])
    out = ops.conv2d([s.to(DEV) for s in srcs], pk, act=act, add=add.to(DEV), add_coff=3)
    ref = _ref_conv(torch.cat(srcs, 1), wt, bias, ks // 2) + add[:, 3:3 + cout].double()
    ref = [ref, torch.relu(ref), torch.sigmoid(ref), torch.tanh(ref)][act]
    close(out, ref, 1e-5, 1e-5, "conv2d")
    # cat-free producer: write into a channel window of a larger tensor
    big = torch.full((b, cout + 7, h, w), 7.0, device=DEV)
    ops.conv2d([s.to(DEV) for s in srcs], pk, act=act, add=add.to(DEV), add_coff=3, out=big, out_coff=4)
    close(big[:, 4:4 + cout], ref, 1e-5, 1e-5, "conv2d window")
    assert (big[:, :4] == 7.0).all() and (big[:, 4 + cout:] == 7.0).all()


@pytest.mark.parametrize("b,cin,cout,h,w", [(1, 64, 96, 18, 36), (2, 96, 128, 17, 35), (1, 16, 32, 5, 7), (1, 64, 64, 64, 130)])
def test_conv2d_stride2(b, cin, cout, h, w):
    """3x3 / stride 2 / padding 1 (split precision): odd and even sizes, bias + ReLU + residual, vs the fp64 conv."""
    from anystereo import ops, _lib as L
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        x = U((b, cin, h, w), 400, -2, 2)
        wt = U((cout, cin, 3, 3), 401) * (3.0 / (cin * 9)) ** 0.5
        bias = U((cout,), 402) * 0.1
        ref = torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), stride=2, padding=1).relu()
        res = U(tuple(ref.shape), 403)
        pk = ops.PackedConv().get([wt.to(DEV)], [bias.to(DEV)])
        out = ops.conv2d([x.to(DEV)], pk, act=L.ACT_RELU, stride=2)
        close(out, ref, 1e-5, 1e-5, "conv2d stride 2")
        out = ops.conv2d([x.to(DEV)], pk, act=L.ACT_RELU, stride=2, h=res.to(DEV))
        close(out, (ref + res.double()).relu(), 1e-5, 1e-5, "conv2d stride 2 + residual")
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("h,w", [(8, 12), (5, 33), (17, 9)])
def test_conv_gru_fused(h, w, precision):
    from anystereo.nn.update import ConvGRU
    from anystereo.harness.synthetic import fill_module_deterministic
    gru = ConvGRU(128, 256).to(DEV).eval()
    fill_module_deterministic(gru, 3)
    hh = torch.tanh(U((1, 128, h, w), 100, -2, 2))
    ctx = U((1, 384, h, w), 101)
    x1, x2 = U((1, 128, h, w), 102), U((1, 128, h, w), 103)
    with torch.no_grad():
        cz, cr, cq = ctx.to(DEV).split(128, dim=1)
        out = gru(hh.to(DEV), cz, cr, cq, x1.to(DEV), x2.to(DEV))
        # non-view context tensors take the concat fallback and must agree
        out2 = gru(hh.to(DEV), cz.clone(), cr.clone(), cq.clone(), x1.to(DEV), x2.to(DEV))
        # the h-part of the gate conv issued ahead (inference schedule of models/base.py)
        out3 = gru(hh.to(DEV), cz, cr, cq, x1.to(DEV), x2.to(DEV), pre_zr=gru.pre_zr(hh.to(DEV), cz, cr, cq))
        ref = O.conv_gru(gru.cpu().double(), hh.double(), *ctx.double().split(128, dim=1), x1.double(), x2.double())
    close(out, ref, 1e-5, 1e-5, "convgru")
    close(out2, ref, 1e-5, 1e-5, "convgru (cat fallback)")
    close(out3, ref, 1e-5, 1e-5, "convgru (h-part of the gates ahead)")


@pytest.mark.parametrize("cin,cout,stride,h,w", [(64, 64, 1, 18, 37), (64, 96, 2, 18, 36), (128, 128, 1, 7, 129)])
def test_residual_block_fused_inference(cin, cout, stride, h, w, precision):
    """§8 f4: the inference fast path of the BatchNorm ResidualBlock (folded BN, ReLU + residual tail in the conv
    epilogue) against the fp64 evaluation of the plain module (extractor.py:10-62)."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.encoders import ResidualBlock
    blk = ResidualBlock(cin, cout, "batch", stride).eval()
    fill_module_deterministic(blk, 5)
    with torch.no_grad():
        for i, m in enumerate(mm for mm in blk.modules() if isinstance(mm, torch.nn.BatchNorm2d)):
            m.running_mean.copy_(U((m.num_features,), 120 + i) * 0.3)
            m.running_var.copy_(U((m.num_features,), 130 + i, 0.5, 2.0))
            m.weight.copy_(U((m.num_features,), 140 + i, 0.5, 1.5))
            m.bias.copy_(U((m.num_features,), 150 + i) * 0.2)
    x = U((2, cin, h, w), 160, -2, 2)
    with torch.enable_grad():  # grad mode keeps the plain PyTorch path
        ref = blk.double()(x.double()).detach()
    blk = blk.float().to(DEV)
    with torch.no_grad():
        out = blk(x.to(DEV))
    close(out, ref, 2e-5, 2e-5, "residual block (fused)")


@pytest.mark.parametrize("b,c,h,w,stride,act", [(2, 32, 17, 70, 1, 4), (1, 96, 18, 67, 2, 4), (1, 5, 3, 3, 2, 0), (1, 8, 65, 130, 1, 5),
                                                # the trunk's half-resolution layers at 960x540 (8-row strips per wave), odd sizes at both strides
                                                # (4-row strips, ragged last strip)
                                                (2, 32, 270, 480, 1, 4), (2, 96, 269, 479, 2, 4), (1, 48, 131, 250, 1, 0), (1, 40, 133, 251, 2, 5)])
def test_dwconv3x3(b, c, h, w, stride, act):
    from anystereo import ops
    x, wt, bias = U((b, c, h, w), 170, -3, 3), U((c, 1, 3, 3), 171), U((c,), 172)
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=1, groups=c)
    ref = {0: ref, 4: ref.clamp(0, 6), 5: torch.nn.functional.leaky_relu(ref, 0.01)}[act]
    res = U(tuple(ref.shape), 173)
    out = ops.dwconv3x3(x.to(DEV), wt.to(DEV), bias.to(DEV), stride, act, residual=res.to(DEV))
    close(out, ref + res.double(), 1e-6, 1e-6, "dwconv3x3")
    close(ops.dwconv3x3(x.to(DEV), wt.to(DEV), None, stride, act), {0: lambda t: t, 4: lambda t: t.clamp(0, 6), 5: lambda t: torch.nn.functional.leaky_relu(t, 0.01)}[act](
        torch.nn.functional.conv2d(x.double(), wt.double(), None, stride=stride, padding=1, groups=c)), 1e-6, 1e-6, "dwconv3x3 (no bias)")


@pytest.mark.parametrize("b,cin,cout,d,h,w,stride,act", [(1, 8, 8, 6, 9, 70, 1, 5), (2, 8, 1, 5, 6, 33, 1, 0), (1, 8, 16, 7, 9, 66, 2, 5),
                                                         (1, 16, 16, 4, 5, 20, 1, 5), (1, 3, 5, 3, 4, 7, 2, 1),
                                                         # stride 1 covers 62 columns per wave (neighbours by wave shifts): the seams
                                                         (1, 8, 8, 3, 5, 62, 1, 0), (1, 8, 8, 3, 5, 63, 1, 5), (1, 8, 8, 2, 6, 125, 1, 0)])
def test_conv3d_k3(b, cin, cout, d, h, w, stride, act):
    from anystereo import ops
    x = U((b, cin, d, h, w), 180, -2, 2)
    wt = U((cout, cin, 3, 3, 3), 181) * (3.0 / (cin * 27)) ** 0.5
    bias = U((cout,), 182) * 0.1
    ref = torch.nn.functional.conv3d(x.double(), wt.double(), bias.double(), stride=stride, padding=1)
    ref = {0: ref, 1: ref.relu(), 5: torch.nn.functional.leaky_relu(ref, 0.01)}[act]
    wp = wt.permute(1, 2, 3, 4, 0).reshape(cin, 27, cout).contiguous()
    out = ops.conv3d_k3(x.to(DEV), wp.to(DEV), bias.to(DEV), stride, act)
    close(out, ref, 2e-6, 2e-6, "conv3d_k3")


@pytest.mark.parametrize("cin,cout,d,h,w,stride", [(8, 8, 6, 9, 33, 1), (8, 16, 6, 10, 34, 2), (32, 32, 4, 6, 21, 1), (16, 16, 24, 68, 120, 1)])
def test_conv3d_with_feature_att_gate(cin, cout, d, h, w, stride, monkeypatch):
    """FeatureAtt (submodule.py:328-341) folded into the launch that produces the volume it gates (as_conv3d_k3_gated; the MFMA
    path's layout copy): FeatureAtt.after(block, x, feat) must equal FeatureAtt(block(x), feat) BIT for bit (one fp32 multiply
    either way), on the direct kernel (stride 1 and 2, large volumes) and on the MFMA path, single blocks and Sequentials."""
    from anystereo import ops
    from anystereo.nn import blocks as B
    from anystereo.harness.synthetic import fill_module_deterministic
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        seq = torch.nn.Sequential(B.BasicConv(cin, cin, is_3d=True, bn=True, relu=True, kernel_size=3, stride=1, padding=1),
                                  B.BasicConv(cin, cout, is_3d=True, bn=True, relu=True, kernel_size=3, stride=stride, padding=1)).eval()
        att = B.FeatureAtt(cout, 64).eval()
        for i, m in enumerate((seq, att)):
            fill_module_deterministic(m, base_seed=41 + i)
            _randomize_bn(m, 960 + 10 * i)
        seq, att = seq.to(DEV), att.to(DEV)
        x = U((1, cin, d, h, w), 970, -2, 2).to(DEV)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        feat = U((1, 64, ho, wo), 971, -2, 2).to(DEV)
        with torch.no_grad():
            monkeypatch.setattr(B.FeatureAtt, "fused_gate", False)
            want = att.after(seq, x, feat)
            want1 = att.after(seq[1], seq[0](x), feat)
            monkeypatch.setattr(B.FeatureAtt, "fused_gate", True)
            got = att.after(seq, x, feat)
            got1 = att.after(seq[1], seq[0](x), feat)
        assert got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got, want) and torch.equal(got1, want1)
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("cin,cout,d,h,w,relu", [(32, 32, 12, 34, 60, True), (48, 48, 6, 17, 30, True), (16, 16, 5, 9, 14, False),
                                                  (32, 48, 1, 7, 33, True), (64, 32, 3, 8, 16, True)])
def test_conv3d_on_the_mfma_kernel(cin, cout, d, h, w, relu, monkeypatch):
    """§8 f4: the small stride-1 3x3x3 layers of the hourglass (continuous_IGEVstereo.py:22-89) as ONE 2-D convolution with
    batch = depth over three depth-shifted views of a zero-padded depth-major copy (nn/blocks.py::conv3d_mfma) — against the
    fp64 module (BatchNorm3d eval + LeakyReLU) and against the direct VALU kernel it replaces; D = 1 (both neighbours are the
    zero slices), ragged planes, Cin != Cout."""
    from anystereo import ops
    from anystereo.nn import blocks as B
    from anystereo.harness.synthetic import fill_module_deterministic
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        m = B.BasicConv(cin, cout, is_3d=True, bn=True, relu=relu, kernel_size=3, stride=1, padding=1).eval()
        fill_module_deterministic(m, base_seed=31)
        with torch.no_grad():
            m.bn.running_mean.copy_(U((cout,), 191) * 0.3), m.bn.running_var.copy_(U((cout,), 192, 0.5, 2.0))
        x = U((1, cin, d, h, w), 190, -2, 2)
        want = m.double()(x.double())
        m = m.float().to(DEV)
        with torch.no_grad():
            assert B.conv3d_mfma_ok(m.conv, x.to(DEV))
            got = m(x.to(DEV))
            monkeypatch.setattr(B, "_CONV3D_MFMA", False)
            direct = m(x.to(DEV))
        assert got.shape == want.shape and got.is_contiguous()
        close(got, want, 1e-5, 1e-5, "conv3d on the MFMA kernel vs fp64")
        close(got, direct, 1e-5, 1e-5, "conv3d on the MFMA kernel vs the direct kernel")
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("b,cin,cout,d,h,w,act", [(1, 16, 8, 4, 6, 70, 0), (2, 8, 16, 3, 5, 33, 5), (1, 5, 3, 2, 3, 9, 1),
                                                  (1, 8, 8, 2, 3, 62, 0), (1, 8, 8, 2, 3, 63, 5), (1, 8, 8, 2, 2, 125, 0)])
def test_deconv3d_k4s2(b, cin, cout, d, h, w, act):
    from anystereo import ops
    x = U((b, cin, d, h, w), 185, -2, 2)
    wt = U((cin, cout, 4, 4, 4), 186) * (3.0 / (cin * 8)) ** 0.5
    bias = U((cout,), 187) * 0.1
    ref = torch.nn.functional.conv_transpose3d(x.double(), wt.double(), bias.double(), stride=2, padding=1)
    ref = {0: ref, 1: ref.relu(), 5: torch.nn.functional.leaky_relu(ref, 0.01)}[act]
    out = ops.deconv3d_k4s2(x.to(DEV), wt.permute(0, 2, 3, 4, 1).contiguous().to(DEV), bias.to(DEV), act)
    close(out, ref, 2e-6, 2e-6, "deconv3d_k4s2")


@pytest.mark.parametrize("b,h,w,act,with_bias", [(1, 24, 40, 1, True), (2, 17, 33, 0, True), (1, 8, 16, 5, False), (1, 70, 130, 1, True)])
def test_conv7x7_c3_stem(b, h, w, act, with_bias):
    """7x7, 3 -> 64 stem on the split-precision MFMA kernel vs fp64 F.conv2d (edges, ragged tiles, several tiles per block)."""
    from anystereo import ops
    ops.set_precision("split")
    x = U((b, 3, h, w), 310, -1.0, 1.0)
    wt = U((64, 3, 7, 7), 311) * (3.0 / 147) ** 0.5
    bias = U((64,), 312) * 0.2 if with_bias else None
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), None if bias is None else bias.double(), padding=3)
    ref = {0: ref, 1: ref.relu(), 5: torch.nn.functional.leaky_relu(ref, 0.01)}[act]
    pk = ops.Stem7x7Pack()
    wd = wt.to(DEV)
    out = ops.conv7x7_c3(x.to(DEV), pk, wd, None if bias is None else bias.to(DEV), act=act)
    close(out, ref, 3e-6, 3e-6, "conv7x7_c3")
    wd.mul_(0.5)  # in-place weight update: the pack follows the version counter
    out2 = ops.conv7x7_c3(x.to(DEV), pk, wd, None, act=0)
    close(out2, torch.nn.functional.conv2d(x.double(), 0.5 * wt.double(), None, padding=3), 3e-6, 3e-6, "conv7x7_c3 repack")


@pytest.mark.parametrize("b,cin,cout,h,w,stride,act", [(2, 3, 32, 21, 70, 2, 4), (1, 3, 8, 9, 130, 1, 1), (1, 1, 16, 6, 5, 2, 0)])
def test_conv3x3_few(b, cin, cout, h, w, stride, act):
    from anystereo import ops
    x = U((b, cin, h, w), 320, -1, 1)
    wt = U((cout, cin, 3, 3), 321) * 0.5
    bias = U((cout,), 322)
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=1)
    ref = {0: ref, 1: ref.relu(), 4: ref.clamp(0, 6)}[act]
    wp = wt.permute(1, 2, 3, 0).reshape(cin, 9, cout).contiguous()
    out = ops.conv3x3_few(x.to(DEV), wp.to(DEV), bias.to(DEV), stride=stride, act=act)
    close(out, ref, 2e-6, 2e-6, "conv3x3_few")


def _randomize_bn(mod, seed):
    with torch.no_grad():
        for i, m in enumerate(mm for mm in mod.modules() if isinstance(mm, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d))):
            m.running_mean.copy_(U((m.num_features,), seed + 4 * i) * 0.3)
            m.running_var.copy_(U((m.num_features,), seed + 4 * i + 1, 0.5, 2.0))
            m.weight.copy_(U((m.num_features,), seed + 4 * i + 2, 0.5, 1.5))
            m.bias.copy_(U((m.num_features,), seed + 4 * i + 3) * 0.2)


def _fused_vs_plain(mod, x, rtol, what):
    with torch.enable_grad():  # grad mode keeps the plain PyTorch path
        ref = mod.double()(x.double()).detach()
    mod = mod.float().to(DEV)
    with torch.no_grad():
        out = mod(x.to(DEV))
    close(out, ref, rtol, rtol, what)


def test_backbone_blocks_fused_inference(precision):
    """§8 f4: MobileNetV2 blocks (pw/dw/pwl with folded BN, ReLU6, skip) and the BatchNorm Conv3d block."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.blocks import BasicConv, BasicConv_IN, HighRes_Aggregation, HighRes_Aggregation_LN_GeLU
    from anystereo.nn.encoders import ResidualBlock, _DSConv, _InvRes
    for k, (mod, shape) in enumerate([(_InvRes(24, 24, 1), (2, 24, 17, 37)), (_InvRes(16, 24, 2), (1, 16, 18, 40)),
                                      (_DSConv(32, 16, 1), (1, 32, 9, 70)), (_InvRes(64, 64, 1), (1, 64, 5, 9)),
                                      (BasicConv(8, 16, is_3d=True, kernel_size=3, padding=1, stride=2), (1, 8, 6, 9, 33)),
                                      (BasicConv(16, 16, is_3d=True, kernel_size=3, padding=1, stride=1), (1, 16, 4, 6, 21)),
                                      (BasicConv(16, 8, deconv=True, is_3d=True, kernel_size=(4, 4, 4), padding=(1, 1, 1),
                                                 stride=(2, 2, 2)), (1, 16, 3, 5, 21)),
                                      (BasicConv_IN(12, 32, kernel_size=3, stride=1, padding=1), (2, 12, 11, 37)),
                                      (BasicConv_IN(16, 8, deconv=True, kernel_size=4, stride=2, padding=1), (1, 16, 7, 9)),
                                      (HighRes_Aggregation_LN_GeLU(3, 32), (1, 3, 16, 36)),
                                      (HighRes_Aggregation(3, 48), (2, 3, 12, 20)),
                                      (ResidualBlock(64, 64, "instance", 1), (2, 64, 13, 37)),
                                      (ResidualBlock(64, 96, "instance", 2), (1, 64, 14, 36))]):
        mod = mod.eval()
        fill_module_deterministic(mod, 7 + k)
        _randomize_bn(mod, 200 + 40 * k)
        _fused_vs_plain(mod, U(shape, 190 + k, -2, 2), 3e-5, f"fused block {k}")


@pytest.mark.parametrize("cin,cout,stride,b,h,w", [(16, 24, 2, 2, 34, 60), (24, 24, 1, 2, 17, 37), (24, 32, 2, 1, 19, 33), (32, 32, 1, 1, 9, 21),
                                                    (32, 64, 2, 2, 10, 18), (64, 64, 1, 2, 5, 9), (64, 96, 1, 1, 8, 8), (96, 96, 1, 1, 7, 10),
                                                    (96, 160, 2, 2, 9, 15), (160, 160, 1, 1, 5, 8), (160, 160, 1, 2, 17, 30)])
def test_ir_block_one_launch(cin, cout, stride, b, h, w, monkeypatch):
    """§8 f4: every (Cin, Cout, stride) of the MobileNetV2 trunk's inverted-residual blocks (extractor.py:327-342) as ONE launch
    (csrc/irblock.hip: expand -> ReLU6 -> depthwise -> ReLU6 -> project [+ x], BatchNorm folded, the expanded tensor in LDS) against
    the fp64 module and against the three-launch path it replaces; odd planes (ragged tiles, the zero padding of the EXPANDED
    tensor at every border), batch 2, the 144-channel expansion (4.5 chunks), activations that saturate ReLU6."""
    from anystereo import ops
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.encoders import _InvRes
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        mod = _InvRes(cin, cout, stride).eval()
        fill_module_deterministic(mod, 50 + cin + cout)
        _randomize_bn(mod, 900 + cin)
        x = U((b, cin, h, w), 950 + cout, -3, 3)
        with torch.enable_grad():  # grad mode keeps the plain PyTorch path
            want = mod.double()(x.double()).detach()
        mod = mod.float().to(DEV)
        with torch.no_grad():
            monkeypatch.setattr(_InvRes, "fused_ir", True)
            got = mod(x.to(DEV))
            monkeypatch.setattr(_InvRes, "fused_ir", False)
            three = mod(x.to(DEV))
        assert got.shape == want.shape
        close(got, want, 2e-5, 2e-5, "ir_block vs fp64")
        close(got, three, 2e-5, 2e-5, "ir_block vs the three-launch path")
    finally:
        ops.set_precision(prev)


def test_norm_kernels():
    from anystereo import _lib as L
    from anystereo import ops
    x = U((2, 5, 37, 50), 300, -3, 5)
    ref = torch.nn.functional.instance_norm(x.double(), eps=1e-5)
    close(ops.instance_norm_act(x.to(DEV), 1e-5, L.ACT_NONE), ref, 2e-6, 2e-6, "instance norm")
    close(ops.instance_norm_act(x.to(DEV), 1e-5, L.ACT_LEAKY), torch.nn.functional.leaky_relu(ref, 0.01), 2e-6, 2e-6, "IN + leaky")
    x3 = U((1, 3, 4, 9, 11), 301) + 100.0  # large mean: the fp64 partial sums must not cancel
    close(ops.instance_norm_act(x3.to(DEV), 1e-5, L.ACT_RELU), torch.nn.functional.instance_norm(x3.double(), eps=1e-5).relu(), 2e-4, 2e-4, "IN 3-D, offset data")
    for c in (32, 48):
        y = U((2, c, 9, 21), 302 + c, -2, 4)
        w, b = U((c,), 303, 0.5, 1.5), U((c,), 304) * 0.3
        mu = y.double().mean(1, keepdim=True)
        var = (y.double() - mu).pow(2).mean(1, keepdim=True)
        ln = w.double().view(1, -1, 1, 1) * ((y.double() - mu) / (var + 1e-6).sqrt()) + b.double().view(1, -1, 1, 1)
        close(ops.layernorm2d_act(y.to(DEV), w.to(DEV), b.to(DEV), 1e-6, L.ACT_GELU), torch.nn.functional.gelu(ln), 3e-6, 3e-6, "LN + GELU")
        close(ops.layernorm2d_act(y.to(DEV), w.to(DEV), b.to(DEV), 1e-6, L.ACT_RELU), ln.relu(), 3e-6, 3e-6, "LN + ReLU")


def test_direct_convs_and_resamplers(precision):
    from anystereo import ops
    x = U((2, 1, 19, 37), 110, 0, 30)
    w7, b7 = U((64, 1, 7, 7), 111) * 0.2, U((64,), 112) * 0.1
    close(ops.conv7x7_c1_relu(x.to(DEV), w7.to(DEV), b7.to(DEV)), torch.relu(_ref_conv(x, w7, b7, 3)), 1e-5, 1e-5, "conv7x7")
    y = U((2, 256, 9, 70), 113)
    w3, b3 = U((1, 256, 3, 3), 114) * 0.05, U((1,), 115)
    close(ops.conv3x3_to1(y.to(DEV), w3.to(DEV), b3.to(DEV)), _ref_conv(y, w3, b3, 1), 1e-5, 1e-5, "conv3x3_to1")
    z = U((2, 5, 9, 14), 116)
    close(ops.pool2x(z.to(DEV)), O.pool2x(z.double()), 1e-6, 1e-6, "pool2x")
    close(ops.pool2x(z[..., :13].contiguous().to(DEV)), O.pool2x(z[..., :13].double()), 1e-6, 1e-6, "pool2x odd")
    close(ops.interp(z.to(DEV), 18, 27), O.interp_to(z.double(), 18, 27), 1e-5, 1e-6, "interp")
    close(ops.interp(z.to(DEV), 17, 28), torch.nn.functional.interpolate(z, (17, 28), mode="bilinear", align_corners=True),
          1e-5, 1e-6, "interp vs torch")


def test_update_block_golden(golden, precision):
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models.base import default_args
    from anystereo.nn.update import BasicMultiUpdateBlock
    for tag in ("igev", "raft"):
        g = golden(f"update_{tag}")
        args = default_args("continuous_IGEVStereo" if tag == "igev" else "continuous_RAFTStereo")
        ub = BasicMultiUpdateBlock(args, hidden_dims=args.hidden_dims, geo_channels=8 if tag == "igev" else 0).eval()
        fill_module_deterministic(ub, base_seed=5)
        ub = ub.to(DEV)
        net = [g["net0"].to(DEV), g["net1"].to(DEV), g["net2"].to(DEV)]
        inp = [list(g[f"ctx{i}"].to(DEV).split(128, dim=1)) for i in range(3)]
        with torch.no_grad():
            mf = ub.encoder(g["disp"].to(DEV), g["corr"].to(DEV))
            close(mf if torch.is_tensor(mf) else mf.float(), g["motion"], 2e-5, 2e-5, "motion encoder")  # blocked link tensor in split mode
            close(ub.disp_head(net[0]), g["head"], 2e-5, 2e-5, "disp head")
            out, delta = ub([n.clone() for n in net], inp, g["corr"].to(DEV), g["disp"].to(DEV))
            for i in range(3):
                close(out[i], g[f"out{i}"], 2e-5, 3e-5, f"net{i}")
            close(delta, g["delta"], 2e-5, 3e-5, "delta")
            lo = ub([n.clone() for n in net], inp, iter16=True, iter08=True, iter04=False, update=False)
            close(lo[1], g["lo1"], 2e-5, 3e-5, "slow-fast net1")


def test_update_block_flag_combinations_golden(golden, precision):
    """G5: every (iter16, iter08, iter04, update) pattern of BasicMultiUpdateBlock.forward against the reference's outputs
    (update.py:116-136; slow-fast pre-updates continuous_IGEVstereo.py:288-291)."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models.base import default_args
    from anystereo.nn.update import BasicMultiUpdateBlock
    from test_oracle_golden import FLAG_COMBOS
    for tag in ("igev", "raft"):
        g, gf = golden(f"update_{tag}"), golden(f"update_flags_{tag}")
        args = default_args("continuous_IGEVStereo" if tag == "igev" else "continuous_RAFTStereo")
        ub = BasicMultiUpdateBlock(args, hidden_dims=args.hidden_dims, geo_channels=8 if tag == "igev" else 0).eval()
        fill_module_deterministic(ub, base_seed=5)
        ub = ub.to(DEV)
        inp = [list(g[f"ctx{i}"].to(DEV).split(128, dim=1)) for i in range(3)]
        for name, kw in FLAG_COMBOS:
            net = [g["net0"].to(DEV).clone(), g["net1"].to(DEV).clone(), g["net2"].to(DEV).clone()]
            with torch.no_grad():
                res = ub(net, inp, g["corr"].to(DEV) if kw["iter04"] else None, g["disp"].to(DEV) if kw["iter04"] else None, **kw)
            nets = res[0] if kw["update"] else res
            for i in range(3):
                close(nets[i], gf[f"{name}_net{i}"], 2e-5, 3e-5, f"{tag} {name} net{i}")
            if kw["update"]:
                close(res[1], gf[f"{name}_delta"], 2e-5, 3e-5, f"{tag} {name} delta")


# ---------------------------------------------------------------------------------------------
# a12-a17 LIIF
# ---------------------------------------------------------------------------------------------

def test_liif_golden(golden, precision):
    from anystereo import ops
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.liif import liif_out_multi_scale_Training, liif_feat_multiscale_train, AffinityFeature
    from anystereo.nn.functional import context_upsample_multiscale_train
    g = golden("liif")
    close(AffinityFeature(3, 3, 1, 0)(g["feat"].to(DEV)), g["aff"], 1e-5, 2e-6, "affinity")
    sf = ops.structure_feature(g["feat"].to(DEV))
    close(sf[:, :20], g["feat"], 0, 0, "structure feature copy")
    for key in ("1p0", "1p5", "2p0", "2p95"):
        rel, qf, _ = liif_feat_multiscale_train(g["feat"].to(DEV), g[f"coord_{key}"].to(DEV))
        close(qf, g[f"qfeat_{key}"], 0, 0, f"q_feat {key}")
        close(rel, g[f"rel_{key}"], 0, 2e-6, f"rel {key}")
    up = liif_out_multi_scale_Training(encoder_dim=208, mlphidden_list=[128, 64, 64], pos_dim=0, unfold="with_v2ISU",
                                       affinity_settings={"win_w": 3, "win_h": 3, "dilation": [1, 2, 4, 8]},
                                       number_input=2, chanels=[176, 32]).eval()
    fill_module_deterministic(up, base_seed=7, gain=2.0)
    up = up.to(DEV)
    with torch.no_grad():
        mask = up([g["x4"].to(DEV), g["x2"].to(DEV)], g["coord"].to(DEV), torch.tensor([[1.5]], device=DEV))
    assert mask.shape == g["mask"].shape
    close(mask, g["mask"], 2e-5, 2e-5, "liif mask logits")
    up.query_chunk = 256  # force the query-slab path used for > 2^20 queries (Middlebury-F: 5.7 M)
    with torch.no_grad():
        mask_c = up([g["x4"].to(DEV), g["x2"].to(DEV)], g["coord"].to(DEV), torch.tensor([[1.5]], device=DEV))
    close(mask_c, mask, 2e-6, 2e-6, "query-slab processing")
    up.query_chunk = 1 << 20
    up.fused_first_layer = False  # literal order: gather the 228-channel latent, then all four Linear layers per query
    with torch.no_grad():
        mask_l = up([g["x4"].to(DEV), g["x2"].to(DEV)], g["coord"].to(DEV), torch.tensor([[1.5]], device=DEV))
    close(mask_l, g["mask"], 2e-5, 2e-5, "liif mask logits (unfused first layer)")
    close(mask_l, mask, 1e-5, 1e-5, "first layer at low resolution == per-query")
    up.fused_first_layer = True
    with torch.no_grad():  # single-source form (stem_2x absent)
        u1 = liif_out_multi_scale_Training(encoder_dim=176, mlphidden_list=[128, 64, 64], pos_dim=0, unfold="with_v2ISU",
                                           affinity_settings={"win_w": 3, "win_h": 3, "dilation": [1, 2, 4, 8]},
                                           number_input=1, chanels=[176]).eval()
        fill_module_deterministic(u1, base_seed=9, gain=2.0)
        u1 = u1.to(DEV)
        ma = u1([g["x4"].to(DEV)], g["coord"].to(DEV), torch.tensor([[1.5]], device=DEV))
        u1.fused_first_layer = False
        mb = u1([g["x4"].to(DEV)], g["coord"].to(DEV), torch.tensor([[1.5]], device=DEV))
    close(ma, mb, 1e-5, 1e-5, "single-source fused first layer")
    coord = g["coord"].clone().to(DEV)
    cu = context_upsample_multiscale_train((g["dlow"] * 4.0 * 1.5).to(DEV), torch.softmax(g["mask"], 1).to(DEV), coord)
    close(cu, g["convex"], 1e-5, 1e-5, "convex upsample (reference contract)")
    fused = ops.convex_upsample(g["dlow"].to(DEV), g["mask"].to(DEV), g["coord"].to(DEV),
                                scale=torch.tensor([1.5], device=DEV), mask_is_logits=True)
    close(fused[:, 0], g["convex"], 1e-5, 1e-5, "convex upsample (fused softmax+scale)")
    # MLP reference contract [..., in] -> [..., out]
    lat = U((3, 50, 228), 120)
    with torch.no_grad():
        close(up.imnet(lat.to(DEV)), O.mlp(up.imnet.cpu().double(), lat.double()), 2e-5, 2e-5, "MLP")


# ---------------------------------------------------------------------------------------------
# whole models (G7) — HIP vs the imported reference and vs the CPU oracle
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["igev", "raft"])
def test_whole_model(name, golden, precision):
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    g = golden(f"model_{name}")
    H, W = int(g["H"]), int(g["W"])
    key = "continuous_IGEVStereo" if name == "igev" else "continuous_RAFTStereo"
    model = __models__[key](default_args(key)).eval()
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV)
    img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
    with torch.no_grad():
        for s, k in ((1.0, "1p0"), (1.5, "1p5")):
            coord = O.make_coord([round(H * s), round(W * s)]).view(1, -1, 2).to(DEV)
            up = model(img1.to(DEV), img2.to(DEV), iters=3, test_mode=True, hr_coord=coord, scale=torch.tensor([[s]], device=DEV))
            assert up.shape == g[f"test_{k}"].shape
            epe = (up.cpu() - g[f"test_{k}"]).abs().mean().item()
            assert epe < 1e-3, f"{name} scale {s}: EPE vs reference {epe:.3e} (bar 1e-3)"
        coord = O.make_coord([H, W]).view(1, -1, 2).to(DEV)
        res = model(img1.to(DEV), img2.to(DEV), iters=3, test_mode=False, hr_coord=coord, scale=torch.tensor([[1.0]], device=DEV))
        preds = res[1] if name == "igev" else res
        assert len(preds) == 3
        for i, p in enumerate(preds):
            assert (p.cpu() - g[f"pred_{i}"]).abs().mean().item() < 1e-3


# ---- allocation hygiene of the whole model (tests/_guarded.py; the entry points one by one: tests/test_memory_hygiene_gpu.py) ----

def _hygiene_forward(name, put, graph=False, iters=2, calls=1):
    """A fresh model (fresh weight packs) and `calls` forward passes in test_mode at 64x128, scale 1.5."""
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    key = "continuous_IGEVStereo" if name == "igev" else "continuous_RAFTStereo"
    model = __models__[key](default_args(key)).eval()
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV)
    img1, img2 = synthetic_pair(1, 64, 128, shift=6, seed=99)
    img1, img2, scale = put(img1), put(img2), put(torch.tensor([[1.5]]))
    coord = O.make_coord([96, 192]).view(1, -1, 2)
    with torch.no_grad():
        if graph:
            model.enable_graph(True)
        return [model(img1, img2, iters=iters, test_mode=True, hr_coord=put(coord), scale=scale) for _ in range(calls)]


@pytest.mark.parametrize("name", ["igev", "raft"])
def test_whole_model_allocation_hygiene(name, precision):
    """The eager forward with every torch.empty buffer of ops.py and nn/*.py poisoned and guarded (NaN, then finite garbage) and the
    inputs placed between poisoned neighbours: the guards stay intact and the output is the plain run's, bit for bit."""
    from _guarded import PATTERNS, guarded, place
    (plain,) = _hygiene_forward(name, lambda t: place(t, DEV))
    assert torch.isfinite(plain).all()
    for pattern in PATTERNS:
        with guarded(pattern) as g:
            (out,) = _hygiene_forward(name, lambda t: place(t, DEV))
            g.check()
            n, out = len(g.buffers), out.clone()
        assert torch.isfinite(out).all(), f"fill 0x{pattern:02X}: non-finite output"
        assert torch.equal(out, plain), f"fill 0x{pattern:02X}: {int((out != plain).sum())} of {out.numel()} output elements differ from the plain run"
        print(f"[hygiene {name} {precision} 0x{pattern:02X}] {n} guarded buffers, guards intact, output bit-equal")


@pytest.mark.parametrize("name", ["igev", "raft"])
def test_whole_model_training_step_allocation_hygiene(name):
    """The G8 step (tiny_train_case, split mode) plain and under both fills.  Finite loss and gradients, guards intact.  Held to what
    test_training_step_is_bit_repeatable holds between two plain runs of the default mode, and to nothing wider: loss and every
    prediction bit-equal; the backward starts with the upsampler's float-atomic scatter-adds, so no parameter gradient is held
    bit-equal there — EVERY parameter gradient within that test's 1e-5 of its maximum."""
    from _guarded import PATTERNS, guarded, place
    l0, p0, g0 = _g8_run(name, "split", put=lambda t: place(t, DEV))
    for pattern in PATTERNS:
        with guarded(pattern) as g:
            l1, p1, g1 = _g8_run(name, "split", put=lambda t: place(t, DEV))
            g.check()
            n, l1, p1, g1 = len(g.buffers), l1.clone(), [t.clone() for t in p1], {k: v.clone() for k, v in g1.items()}
        assert torch.isfinite(l1) and sorted(g1) == sorted(g0)
        bad = [k for k, v in g1.items() if not torch.isfinite(v).all()]
        assert not bad, f"fill 0x{pattern:02X}: non-finite gradients {bad[:8]}"
        assert torch.equal(l0, l1), f"fill 0x{pattern:02X}: loss {l1.item()!r} vs the plain run's {l0.item()!r}"
        for a, b in zip(p0, p1):
            assert torch.equal(a, b), f"fill 0x{pattern:02X}: a prediction differs from the plain run"
        # every parameter gradient, not only the stored ones: within 1e-5 of its maximum, or — the form that test's deterministic
        # branch uses for gradients that are zero in exact arithmetic — its maximum below 1e-6 of the largest gradient's
        top = max(v.abs().max().item() for v in g0.values())
        worst = 0.0
        for k in sorted(g0):
            d = ((g0[k] - g1[k]).abs().max() / g0[k].abs().max().clamp_min(1e-30)).item()
            tiny = max(g0[k].abs().max().item(), g1[k].abs().max().item()) < 1e-6 * top
            worst = worst if tiny else max(worst, d)
            assert d < 1e-5 or tiny, f"fill 0x{pattern:02X}: {k} differs from the plain run by {d:.2e} of its maximum"
        print(f"[hygiene train {name} 0x{pattern:02X}] {n} guarded buffers, guards intact, forward bit-equal, all {len(g0)} gradients within {worst:.1e}")


@pytest.mark.parametrize("precision", ["fp32", "split"])
def test_whole_model_graph_replay_allocation_hygiene(precision):
    """The default IGEV model as in test_default_model_graph_capture_in_both_precisions (64x128, 3 iterations), captured under
    guarded(0xFF): the poison fills are nodes of the graph and run at every replay.  Two replays bit-equal, each within that
    test's 1e-4 of the plain eager result and finite, guards intact after the second."""
    from anystereo import ops
    from _guarded import NAN_FILL, guarded, place
    prev = ops.get_precision()
    ops.set_precision(precision)
    try:
        (eager,) = _hygiene_forward("igev", lambda t: place(t, DEV), iters=3)
        with guarded(NAN_FILL) as g:
            g1, g2 = (t.clone() for t in _hygiene_forward("igev", lambda t: place(t, DEV), graph=True, iters=3, calls=2))
            g.check()
        assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
        assert torch.equal(g1, g2), f"{int((g1 != g2).sum())} of {g1.numel()} elements differ between two replays"
        assert (g1 - eager).abs().max().item() <= 1e-4
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("name", ["igev", "raft"])
def test_model_options_vs_reference(name, golden, precision):
    """forward() branches beyond the main G7 fixture, HIP path vs the imported reference (tests/golden/model_opts.npz):
    `slow_fast_gru = True` (continuous_IGEVstereo.py:288-291, prune_raft_stereo.py:280-283 — the un-pipelined loop with the two
    pre-updates of the low-resolution GRUs), `flow_init` (read by neither reference forward), `output_raw=True` (RAFT: the
    (low-resolution disparity, upsampled) tuple, prune_raft_stereo.py:293-296; IGEV: ignored, continuous_IGEVstereo.py:303-305)."""
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    g = golden("model_opts")
    H, W = (int(v) for v in g[f"{name}_HW"])
    key = "continuous_IGEVStereo" if name == "igev" else "continuous_RAFTStereo"
    model = __models__[key](default_args(key)).eval()
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV)
    img1, img2 = (t.to(DEV) for t in synthetic_pair(1, H, W, shift=6, seed=99))
    coord = O.make_coord([round(H * 1.5), round(W * 1.5)]).view(1, -1, 2).to(DEV)
    sc = torch.tensor([[1.5]], device=DEV)
    with torch.no_grad():
        base = model(img1, img2, iters=3, test_mode=True, hr_coord=coord, scale=sc)
        assert (base.cpu() - g[f"{name}_base"]).abs().mean().item() < 1e-3
        with_fi = model(img1, img2, iters=3, flow_init=g[f"{name}_flow_init"].to(DEV), test_mode=True, hr_coord=coord, scale=sc)
        # the reference never reads flow_init: the result must not move.  Checked to 1e-4 px (an argument that WAS read would move
        # it by pixels: the fixture's flow_init is U(0, 20)); run-to-run bit equality of two eager forwards is a separate property
        # (test_training_step_is_bit_repeatable) — on one MI355X lease of round 6 two identical RAFT forwards differed by one ulp
        # of the output (7.6e-6 px) in every precision mode while IGEV's were bit-equal, on six other leases both were bit-equal
        # (DESIGN.md §2 "run-to-run")
        d_fi = (with_fi - base).abs().max().item()
        if d_fi != 0.0:
            print(f"[model_opts {name} {precision}] two forwards differ by {d_fi:.1e} px (not bit-equal on this box)")
        assert d_fi < 1e-4, f"flow_init must not change the result (the reference never reads it): {d_fi:.2e} px"
        raw = model(img1, img2, iters=3, test_mode=True, hr_coord=coord, scale=sc, output_raw=True)
        if name == "raft":
            assert isinstance(raw, tuple) and len(raw) == 2
            assert raw[0].shape == g["raft_raw_disp"].shape and (raw[0].cpu() - g["raft_raw_disp"]).abs().mean().item() < 1e-3
            assert (raw[1].cpu() - g["raft_raw_up"]).abs().mean().item() < 1e-3
        else:
            assert torch.is_tensor(raw) and (raw.cpu() - g["igev_output_raw"]).abs().mean().item() < 1e-3
        model.args.slow_fast_gru = True
        sf = model(img1, img2, iters=3, test_mode=True, hr_coord=coord, scale=sc)
        epe = (sf.cpu() - g[f"{name}_slowfast"]).abs().mean().item()
        assert epe < 1e-3, f"{name} slow_fast_gru: EPE vs reference {epe:.3e} (bar 1e-3)"
        assert (sf - base).abs().mean().item() > 1e-3, "the slow-fast branch was not taken"


def test_ops_reject_cpu_tensors():
    """No silent CPU fallback in the product path."""
    from anystereo import ops
    with pytest.raises(RuntimeError):
        ops.corr_build_pyramid(torch.zeros(1, 4, 2, 8), torch.zeros(1, 4, 2, 8), 2)
    with pytest.raises(RuntimeError):
        ops.pool2x(torch.zeros(1, 1, 4, 4))


# ---------------------------------------------------------------------------------------------
# training (cfg 4): backward kernels vs autograd of the oracle; one training step vs the reference's gradients (G8)
# ---------------------------------------------------------------------------------------------

def _leaf(t, dev=None, dt=None):
    t = t.clone()
    if dt is not None:
        t = t.to(dt)
    if dev is not None:
        t = t.to(dev)
    return t.requires_grad_(True)


@pytest.mark.parametrize("b,c,h,w1,w2,L", [(2, 96, 3, 20, 20, 2), (1, 64, 2, 21, 21, 2), (1, 32, 2, 37, 37, 4), (2, 33, 3, 70, 45, 3)])
def test_corr_build_backward(b, c, h, w1, w2, L):
    from anystereo import grad as G
    f1, f2 = U((b, c, h, w1), 401), U((b, c, h, w2), 402)
    gs = [U((b, h, w1, w2 >> i), 410 + i) for i in range(L)]
    a1, a2 = _leaf(f1, DEV), _leaf(f2, DEV)
    lv = G.CorrBuildPyramid.apply(a1, a2, L)
    torch.autograd.backward(lv, [g.to(DEV) for g in gs])
    r1, r2 = _leaf(f1, dt=torch.float64), _leaf(f2, dt=torch.float64)
    ref = O.corr_pyramid(O.all_pairs_corr(r1, r2), L)
    torch.autograd.backward(ref, [g.double().view_as(r) for g, r in zip(gs, ref)])
    close(a1.grad, r1.grad, 2e-5, 1e-6, "d f1")
    close(a2.grad, r2.grad, 2e-5, 1e-6, "d f2")
    # only the coarsest level receives a gradient (the others arrive as None)
    a1.grad = None
    lv = G.CorrBuildPyramid.apply(a1, a2.detach(), L)
    lv[-1].backward(gs[-1].to(DEV))
    r1.grad = None
    ref = O.corr_pyramid(O.all_pairs_corr(r1, r2.detach()), L)
    ref[-1].backward(gs[-1].double().view_as(ref[-1]))
    close(a1.grad, r1.grad, 2e-5, 1e-6, "d f1 (last level only)")


@pytest.mark.parametrize("b,g,d,h,w,L", [(2, 8, 48, 3, 20, 2), (1, 4, 17, 2, 9, 3), (1, 8, 48, 5, 33, 2)])
def test_geo_pyramid_backward(b, g, d, h, w, L):
    from anystereo import grad as G
    gev = U((b, g, d, h, w), 420)
    gs = [U((b, h, w, d >> i, g), 421 + i) for i in range(L)]
    a = _leaf(gev, DEV)
    torch.autograd.backward(G.GeoPyramid.apply(a, L), [t.to(DEV) for t in gs])
    r = _leaf(gev, dt=torch.float64)
    torch.autograd.backward(O.geo_pyramid(r, L), [t.double().permute(0, 1, 2, 4, 3) for t in gs])
    close(a.grad, r.grad, 1e-6, 1e-7, "d gev")


@pytest.mark.parametrize("b,c,h,w,D,G_", [(2, 96, 3, 60, 48, 8), (1, 32, 2, 20, 48, 4), (1, 96, 5, 37, 12, 8)])
def test_gwc_backward(b, c, h, w, D, G_):
    from anystereo import grad as G
    fl, fr = U((b, c, h, w), 430), U((b, c, h, w), 431)
    gv = U((b, G_, D, h, w), 432)
    a1, a2 = _leaf(fl, DEV), _leaf(fr, DEV)
    G.GwcVolume.apply(a1, a2, D, G_).backward(gv.to(DEV))
    r1, r2 = _leaf(fl, dt=torch.float64), _leaf(fr, dt=torch.float64)
    O.gwc_volume(r1, r2, D, G_).backward(gv.double())
    close(a1.grad, r1.grad, 2e-5, 1e-6, "d fl")
    close(a2.grad, r2.grad, 2e-5, 1e-6, "d fr")


def test_disparity_regression_backward():
    from anystereo import grad as G
    cost = U((2, 48, 5, 33), 440, -4, 4)
    g = U((2, 1, 5, 33), 441)
    for softmax in (True, False):
        a = _leaf(cost, DEV)
        G.DisparityRegression.apply(a, softmax).backward(g.to(DEV))
        r = _leaf(cost, dt=torch.float64)
        O.disparity_regression(torch.softmax(r, 1) if softmax else r, 48).backward(g.double())
        close(a.grad, r.grad, 2e-5, 1e-6, f"d cost (softmax={softmax})")


@pytest.mark.parametrize("b,c,h,w", [(2, 5, 7, 10), (1, 3, 8, 9), (2, 4, 1, 6), (1, 2, 40, 80)])
def test_pool2x_interp_backward(b, c, h, w):
    """a8^T: the update block's resamplers under autograd (as_pool2x_bwd, as_interp_bilinear_ac_bwd) against autograd of the
    fp64 oracle (avg_pool2d / bilinear align_corners, update.py:94-102), odd sizes, a one-row map, and the same-size / 2x / odd
    destination sizes the update block meets."""
    from anystereo import grad as G
    x = U((b, c, h, w), 460)
    a = _leaf(x, DEV)
    y = G.Pool2x.apply(a)
    g = U(tuple(y.shape), 461)
    y.backward(g.to(DEV))
    r = _leaf(x, dt=torch.float64)
    yr = O.pool2x(r)
    yr.backward(g.double())
    close(y.detach(), yr.detach(), 1e-6, 1e-7, "pool2x forward")
    close(a.grad, r.grad, 1e-6, 1e-7, "pool2x backward")
    for ho, wo in ((2 * h, 2 * w), (2 * h - 1, 2 * w - 1), (h, w), (2 * h + 1, 2 * w - 3 if w > 2 else 3), (1, 1), (max(1, h // 2), max(1, w // 2))):
        a = _leaf(x, DEV)
        y = G.InterpBilinear.apply(a, ho, wo)
        g = U((b, c, ho, wo), 462 + ho)
        y.backward(g.to(DEV))
        r = _leaf(x, dt=torch.float64)
        yr = O.interp_to(r, ho, wo)
        yr.backward(g.double())
        close(y.detach(), yr.detach(), 1e-5, 2e-6, f"interp forward -> {ho}x{wo}")  # fp32 source positions
        close(a.grad, r.grad, 2e-5, 2e-6, f"interp backward -> {ho}x{wo}")


@pytest.mark.parametrize("scale", [1.0, 1.5, 2.95])
def test_liif_gather_and_convex_backward(scale):
    """Scatter-add transposes (float atomics: summation order varies, tolerance covers it)."""
    from anystereo import grad as G
    from anystereo.nn.liif import make_coord
    b, c, h, w = 2, 40, 6, 10
    feat = U((b, c, h, w), 450)
    grid = make_coord([round(4 * h * scale), round(4 * w * scale)])
    coord = grid[None].repeat(b, 1, 1).contiguous()
    coord[0, :3] = torch.tensor([[-1.0, -1.0], [1.0, 1.0], [0.0, 0.0]])
    q = coord.shape[1]
    # a13 + a14
    a = _leaf(feat, DEV)
    lat = G.LiifGather.apply(G.StructureFeature.apply(a), coord.to(DEV))
    gl = U((b, c + 8 + 2, q), 451)
    lat.backward(gl.to(DEV))
    r = _leaf(feat, dt=torch.float64)
    rel, qf = O.liif_query(O.structure_feature_v2isu(r), coord.double())
    torch.cat([qf, rel], -1).permute(0, 2, 1).backward(gl.double())
    close(lat, torch.cat([qf, rel], -1).permute(0, 2, 1), 2e-5, 2e-5, "latent")
    close(a.grad, r.grad, 1e-4, 1e-5, "d feat")
    # a16/a17, logits + scale (the model's call) and the reference function's own contract
    disp, logits, gout = U((b, 1, h, w), 452, 0, 30), U((b, 9, q), 453, -3, 3), U((b, 1, q), 454)
    sc = torch.tensor([scale, 1.0 + 0.5 * scale])
    ad, am = _leaf(disp, DEV), _leaf(logits, DEV)
    out = G.ConvexUpsample.apply(ad, am, coord.to(DEV), sc.to(DEV), True)
    out.backward(gout.to(DEV))
    rd, rm = _leaf(disp, dt=torch.float64), _leaf(logits, dt=torch.float64)
    ref = O.convex_upsample(rd * 4.0 * sc.double().view(-1, 1, 1, 1), torch.softmax(rm, 1), coord.double()).unsqueeze(1)
    ref.backward(gout.double())
    close(out, ref, 2e-5, 2e-5, "convex fwd")
    close(am.grad, rm.grad, 5e-5, 1e-5, "d logits")
    close(ad.grad, rd.grad, 1e-4, 1e-5, "d disp")
    ad, am = _leaf(disp, DEV), _leaf(torch.softmax(logits, 1), DEV)
    G.ConvexUpsample.apply(ad, am, coord.to(DEV), None, False).backward(gout.to(DEV))
    rd, rm = _leaf(disp, dt=torch.float64), _leaf(torch.softmax(logits, 1), dt=torch.float64)
    O.convex_upsample(rd, rm, coord.double()).unsqueeze(1).backward(gout.double())
    close(am.grad, rm.grad, 5e-5, 1e-5, "d mask")
    close(ad.grad, rd.grad, 1e-4, 1e-5, "d disp (plain)")


# G8 limits.  The gradient of a ReLU network is piecewise constant in its activation pattern, and the tiny fixture has ~10^6
# pre-activations of which a handful lie within 1e-6 (relative) of zero: whichever side an implementation's rounding puts them on
# moves individual gradient tensors by a DISCRETE amount — RAFT `convd1.weight` by 5.2e-4, 7.5e-4, 2.5e-3 or 1.47e-2 of its maximum
# (one element each; the fp64 CPU oracle shows exactly these steps when its input images are perturbed by 1e-6 relative, and the
# round-3 driver run landed on the 1.47e-2 one because MIOpen picks its forward algorithms by measured time, per box:
# DESIGN.md §2 "G8", profiles/r04_g8_stress_*.txt).  One fixed element tolerance therefore either hides regressions of the smooth
# tensors or fails on an unlucky box.  The limits are per tensor: tests/golden/train_*_sens.npz holds, from the IMPORTED REFERENCE
# itself, the largest deviation of every gradient norm and of every stored gradient under 128 such perturbations (64 at 1e-6 and 64
# at 2e-6 relative: make_golden.py --only train_sens [--sens-merge]); a tensor's limit is 3x that deviation, floored by 3x the worst value the product showed over the round-4
# stress leases for tensors the perturbations do not move (G8_FLOOR_*).
G8_FLOOR_ELEM = 3e-5   # stored gradients: max |d| / max |g| (worst observed on a tensor the perturbations leave alone: 4.8e-6)
G8_FLOOR_NORM = 2e-3   # gradient norms, relative (worst observed / limit over the stress leases: 0.3)
# parameters whose gradient is identically zero in exact arithmetic (the biases in front of the RAFT feature net's InstanceNorm):
# the reference's value is rounding noise (1e-9 of the largest norm); required of the product: noise of that size, not its digits
G8_ZERO_REF, G8_ZERO_GOT = 1e-7, 1e-6
G8_CAP_ELEM, G8_CAP_NORM = 5e-2, 5e-2  # no fixture deviation buys more than this
# Tensors the reference's own 128 perturbations move by LESS than G8_STABLE are stable in the reference: there the limit is the
# reference's observed maximum itself (not 3x), floored by G8_STABLE_FLOOR_* — 10x below the general norm floor (the product's own
# rounding differs from the reference's — split operands, summation order, MIOpen's per-box solver choice — so a limit below its
# noise would test the box, not the code).  Measured margin (tools/g8_margins.py, profiles/r06_g8_margins.txt): over the 165
# (IGEV) + 49 (RAFT) such tensors the product's worst relative norm deviation is 4.1e-5 (RAFT split), 2.1e-5 (IGEV fp32).
G8_STABLE = 1e-4
G8_STABLE_FLOOR_NORM = 2e-4
G8_STABLE_FLOOR_ELEM = 3e-5


def _g8_limits(name):
    import numpy as np
    s = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"train_{name}_sens.npz"))
    def lim(d, floor, stable_floor, cap):
        d = float(d)
        if d < G8_STABLE:  # stable in the reference: its own observed maximum, not a multiple of it
            return max(stable_floor, d)
        return min(cap, max(floor, 3.0 * d))
    elem = {str(n): lim(d, G8_FLOOR_ELEM, G8_STABLE_FLOOR_ELEM, G8_CAP_ELEM) for n, d in zip(s["full_names"], s["full_dev"])}
    norm = {str(n): lim(d, G8_FLOOR_NORM, G8_STABLE_FLOOR_NORM, G8_CAP_NORM) for n, d in zip(s["names"], s["norm_dev"])}
    return elem, norm


def _g8_run(name, mode, fast16=False, put=None):
    """The G8 step of the product model: (loss, predictions, {parameter: gradient / loss scale}).
    fast16: the one-MFMA mode of the forward / dgrad convolutions (fp16 operands: the reference's autocast arithmetic).
    put: how a host input reaches the device (default .to(DEV); tests/_guarded.place gives it poisoned neighbours)."""
    put = put or (lambda t: t.to(DEV))
    from anystereo import ops
    from anystereo.harness.metrics import sequence_loss_multiscale
    from anystereo.harness.synthetic import fill_module_deterministic, tiny_train_case
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo" if name == "igev" else "continuous_RAFTStereo")
    model = __models__[args.model](args)
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV).train()
    model.freeze_bn()
    h, w, img1, img2, coord, gt, scale = tiny_train_case(name)
    prev = torch.backends.cudnn.deterministic
    prev_mode = ops.get_precision()
    torch.backends.cudnn.deterministic = True
    ls = 4096.0 if mode == "split" else 1.0
    try:
        ops.set_precision(mode)
        with ops.fast_fp16(bool(fast16)):
            res = model(put(img1), put(img2), iters=3, hr_coord=put(coord), scale=put(scale))
            preds = res[1] if name == "igev" else res
            gtd = put(gt)
            loss, _ = sequence_loss_multiscale(preds, gtd, ((gtd < 512) & (gtd > 0)).float(), max_disp=args.max_disp)
            (loss * ls).backward()
            torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.deterministic = prev
        ops.set_precision(prev_mode)
    grads = {n: p.grad.detach() / ls for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach(), [p.detach() for p in preds], grads


@pytest.mark.parametrize("mode", ["split", "fp32"])
@pytest.mark.parametrize("name", ["igev", "raft"])
def test_training_step_vs_reference(name, mode):
    """One training forward/backward of the product model (train mode, frozen BatchNorm2d, 3 GRU iterations with the
    LIIF upsampler every iteration, sequence_loss_multiscale) on the GPU vs the loss and parameter gradients captured
    from the imported reference (tests/golden/train_*.npz, G8), in both matrix-core modes, the split mode with the trainer's
    loss scale (harness/train.py) as a training step runs it.  Limits per tensor: see _g8_limits."""
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"train_{name}.npz"))
    loss, preds, grads = _g8_run(name, mode)
    assert abs(loss.item() - float(z["loss"])) < 1e-5 * abs(float(z["loss"])), (loss.item(), float(z["loss"]))
    assert (preds[-1].cpu() - torch.from_numpy(z["last_pred"])).abs().mean().item() < 2e-4
    names = [str(n) for n in z["names"]]
    assert sorted(grads) == names
    lim_e, lim_n = _g8_limits(name)
    norms = np.array([float(grads[n].double().norm()) for n in names])
    zero = z["norms"] < G8_ZERO_REF * z["norms"].max()
    assert (norms[zero] < G8_ZERO_GOT * z["norms"].max()).all(), [n for n, zz, v in zip(names, zero, norms) if zz and v >= G8_ZERO_GOT * z["norms"].max()]
    rel = np.where(zero, 0.0, np.abs(norms - z["norms"]) / (z["norms"] + 1e-6 * z["norms"].max()))
    ratio = rel / np.array([lim_n[n] for n in names])
    order = np.argsort(-ratio)[:3]
    print(f"[G8 {name} {mode}] loss rel {abs(loss.item() - float(z['loss'])) / abs(float(z['loss'])):.2e}; grad-norm rel max "
          f"{rel.max():.3e}, median {np.median(rel):.3e}; closest to their limits: "
          + ", ".join(f"{names[i]} {rel[i]:.2e} / {lim_n[names[i]]:.1e}" for i in order))
    # the margin actually used, per class of tensor (stable in the reference / moved by its perturbations)
    stable = np.array([lim_n[n] <= G8_STABLE_FLOOR_NORM for n in names]) & ~zero
    for tag, sel in (("stable tensors (limit = the reference's own maximum, floor 2e-4)", stable), ("perturbation-sensitive tensors (limit 3x)", ~stable & ~zero)):
        if sel.any():
            k = int(np.argmax(np.where(sel, ratio, -1.0)))
            print(f"[G8 {name} {mode}] {int(sel.sum())} {tag}: worst deviation / limit = {ratio[k]:.2f} at {names[k]} ({rel[k]:.2e} / {lim_n[names[k]]:.1e})")
    assert ratio.max() < 1.0, f"{name}: grad-norm mismatch {rel[int(ratio.argmax())]:.3e} at {names[int(ratio.argmax())]}"
    # element-wise, on one tensor per operator family, relative to the tensor's max
    for i, n in enumerate(str(x) for x in z["full_names"]):
        want = torch.from_numpy(z[f"g{i}"])
        got = grads[n].cpu()
        e = ((got - want).abs().max() / want.abs().max()).item()
        print(f"[G8 {name} {mode}] {n}: max |d| / max |g| = {e:.2e} (limit {lim_e[n]:.1e}, margin used {e / lim_e[n]:.2f})")
        close(got, want, rtol=lim_e[n], atol=1e-6 * want.abs().max().item(), what=n)


@pytest.mark.parametrize("name", ["igev", "raft"])
def test_training_step_reduced_precision_vs_reference(name):
    """The G8 step in the REFERENCE's own training arithmetic (autocast: fp16 operands, fp32 accumulation;
    train_continuous_IGEV.py:206,288) = the one-MFMA mode of the forward and data-gradient convolutions (ops.fast_fp16), against
    the fp32 fixture of the imported reference.  A second arithmetic mode with its own, stated tolerance — what bench.py's
    `train_mode.reduced_precision` leg runs; never the parity mode.  Tolerances: loss 5e-3 relative, last prediction 5e-2 px (the
    inference mode's bar), gradient norms: median 2e-2 relative, and no tensor off by more than 0.1 of its norm unless the fp32
    reference itself moves it under its own eps-level perturbations (G8 sensitivity > 1e-3)."""
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"train_{name}.npz"))
    s = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"train_{name}_sens.npz"))
    loss, preds, grads = _g8_run(name, "split", fast16=True)
    lrel = abs(loss.item() - float(z["loss"])) / abs(float(z["loss"]))
    epe = (preds[-1].cpu() - torch.from_numpy(z["last_pred"])).abs().mean().item()
    names = [str(n) for n in z["names"]]
    assert sorted(grads) == names
    norms = np.array([float(grads[n].double().norm()) for n in names])
    live = z["norms"] >= 1e-6 * z["norms"].max()
    rel = np.abs(norms - z["norms"])[live] / z["norms"][live]
    stable = np.array([float(d) < 1e-3 for d in s["norm_dev"]])[live]
    print(f"[G8 {name} reduced precision] loss rel {lrel:.2e}; last prediction EPE {epe:.2e} px; grad-norm rel: median {np.median(rel):.2e}, "
          f"max over reference-stable tensors {rel[stable].max():.2e}, max {rel.max():.2e}")
    assert all(torch.isfinite(g).all() for g in grads.values())
    assert lrel < 5e-3 and epe < 5e-2, (lrel, epe)
    assert np.median(rel) < 2e-2 and rel[stable].max() < 0.1, (np.median(rel), rel[stable].max())


@pytest.mark.parametrize("name", ["igev", "raft"])
def test_training_step_is_bit_repeatable(name):
    """The G8 step twice in one process, fresh model each time (a race or an uninitialised read shows up here,
    on any box, as a difference between two runs of the same program).
    Default mode: the forward must be BIT-equal (loss, every prediction).  Its backward starts with the upsampler's scatter-adds
    (float atomics, as in ATen: the order in which a pixel's queries are summed varies between launches), so every gradient
    downstream may differ in its last bits: every stored full gradient within 1e-5 of its maximum (observed over the round-4
    stress leases: <= 1.9e-6).
    Deterministic mode (ops.set_deterministic: gather-form scatters with a fixed summation order, library layers under
    torch.backends.cudnn.deterministic): EVERY parameter gradient must be bit-equal between the two runs."""
    import numpy as np
    from anystereo import ops
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"train_{name}.npz"))
    l0, p0, g0 = _g8_run(name, "split")
    l1, p1, g1 = _g8_run(name, "split")
    assert torch.equal(l0, l1), "loss differs between two runs of the same step"
    for a, b in zip(p0, p1):
        assert torch.equal(a, b), "a prediction differs between two runs of the same step"
    worst = 0.0
    for n in (str(x) for x in z["full_names"]):
        d = ((g0[n] - g1[n]).abs().max() / g0[n].abs().max()).item()
        worst = max(worst, d)
        assert d < 1e-5, f"{n}: run-to-run gradient difference {d:.2e} of its maximum"
    ops.set_deterministic(True)
    try:
        ld0, pd0, gd0 = _g8_run(name, "split")
        ld1, pd1, gd1 = _g8_run(name, "split")
    finally:
        ops.set_deterministic(False)
    assert torch.equal(ld0, l0) and all(torch.equal(a, b) for a, b in zip(pd0, p0)), "the deterministic mode changed the forward"
    differing = [n for n in gd0 if not torch.equal(gd0[n], gd1[n])]
    # ... and it is the same gradient as the default mode's up to summation order
    for n in (str(x) for x in z["full_names"]):
        d = ((gd0[n] - g0[n]).abs().max() / g0[n].abs().max()).item()
        assert d < 1e-5, f"{n}: deterministic vs default gradient {d:.2e} of its maximum"
    print(f"[G8 repeat {name}] forward bit-equal; default mode: stored gradients differ by at most {worst:.1e} of their maxima between two "
          f"runs; deterministic mode: {len(gd0) - len(differing)} of {len(gd0)} parameter gradients bit-equal" +
          (f"; differing: {differing[:8]}" if differing else ""))
    # Every gradient whose backward path runs on this library's kernels alone (loss -> upsampler -> update block) must be bit-equal.
    # The backbone's gradients also pass through MIOpen's backward kernels: bit-equal on every lease so far (432/432, 234/234), but
    # which solver MIOpen picks is a per-box matter — there, last-bit noise is tolerated, anything larger is not.
    own = [n for n in differing if n.startswith(("update_block.", "liif_up."))]
    assert not own, f"deterministic mode: gradients of the library's own path differ between two runs: {own[:8]}"
    for n in differing:
        d = ((gd0[n] - gd1[n]).abs().max() / gd0[n].abs().max().clamp_min(1e-30)).item()
        assert d < 1e-5 or gd0[n].abs().max().item() < 1e-6 * max(g.abs().max().item() for g in gd0.values()), \
            f"deterministic mode: {n} differs by {d:.2e} of its maximum between two runs"


@pytest.mark.parametrize("name", ["igev", "raft"])
def test_training_batched_upsampler_equals_per_iteration(name):
    """Training forward / backward with the upsampler of all iterations issued after the loop as batched calls over (iteration,
    sample) (models/base.py::_upsample_batched) against the reference's order (one call per iteration): same predictions, same
    loss, same gradients up to fp32 summation order; the caller's hr_coord is clamped in place either way."""
    from anystereo.harness.metrics import sequence_loss_multiscale
    from anystereo.harness.synthetic import fill_module_deterministic, tiny_train_case
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo" if name == "igev" else "continuous_RAFTStereo")
    h, w, img1, img2, coord, gt, scale = tiny_train_case(name)
    coord = coord.clone()
    coord[0, 0] = torch.tensor([-1.0, 1.0])  # outside the clamp range: the in-place side effect must show
    res = {}
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for batched in (False, True):
            model = __models__[args.model](args)
            fill_module_deterministic(model, base_seed=1)
            model = model.to(DEV).train()
            model.freeze_bn()
            model.batched_train_upsample = batched
            c = coord.clone().to(DEV)
            out = model(img1.to(DEV), img2.to(DEV), iters=4, hr_coord=c, scale=scale.to(DEV))
            preds = out[1] if name == "igev" else out
            gtd = gt.to(DEV)
            loss, _ = sequence_loss_multiscale(preds, gtd, ((gtd < 512) & (gtd > 0)).float(), max_disp=args.max_disp)
            loss.backward()
            res[batched] = ([p.detach().clone() for p in preds], loss.item(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, c)
    finally:
        torch.backends.cudnn.deterministic = prev
    a, b_ = res[False], res[True]
    assert len(a[0]) == len(b_[0]) == 4
    for i, (x, y) in enumerate(zip(a[0], b_[0])):
        assert x.shape == y.shape
        close(y, x, 2e-5, 2e-5, f"prediction of iteration {i}")
    assert abs(a[1] - b_[1]) <= 1e-5 * abs(a[1])
    assert sorted(a[2]) == sorted(b_[2])
    gmax = max(g.abs().max().item() for g in a[2].values())
    for n in a[2]:  # atol: biases in front of an InstanceNorm have a true gradient of zero — what is compared there is rounding noise
        close(b_[2][n], a[2][n], 2e-3, 1e-6 * gmax, f"gradient of {n}")
    assert torch.equal(a[3], b_[3]) and a[3].abs().max().item() <= 1 - 1e-6 + 1e-9, "hr_coord clamped in place"


def test_conv7x7_c1_relu_backward_and_head_conv2():
    """The two per-iteration layers that used to stay on the library in training: convd1 (7x7, 1 -> 64, ReLU; weight / bias
    gradient of several iterations in one launch) and the head's conv2 (3x3, 256 -> 1: forward, dgrad with ONE input channel,
    wgrad with one output channel) against fp64 autograd."""
    import torch.nn.functional as F
    from anystereo import grad as G, ops
    b, h, w = 3, 21, 37
    wt, bs = U((64, 1, 7, 7), 900, -0.2, 0.2), U((64,), 901)
    xs = [U((b, 1, h, w), 902 + i, 0.0, 30.0) for i in range(3)]
    gs = [U((b, 64, h, w), 910 + i) * 1e-3 for i in range(3)]
    wl, bl = _leaf(wt, DEV), _leaf(bs, DEV)
    ys = [G.Conv7x7C1Relu.apply(x.to(DEV), wl, bl, None) for x in xs]
    torch.autograd.backward(ys, [g.to(DEV) for g in gs])
    wr, br = wt.double().requires_grad_(True), bs.double().requires_grad_(True)
    yr = [F.relu(F.conv2d(x.double(), wr, br, padding=3)) for x in xs]
    torch.autograd.backward(yr, [g.double() for g in gs])
    for y, r in zip(ys, yr):
        close(y.detach().cpu(), r.detach().float(), 2e-5, 2e-5, "convd1 forward")
    # the batched form (all iterations in one launch) equals the sum of the per-call gradients
    masked = [torch.ops.aten.threshold_backward(g.to(DEV), y.detach(), 0.0) for g, y in zip(gs, ys)]
    dw, db = ops.conv7x7_c1_wgrad([x.to(DEV) for x in xs], masked)
    for nm, got, want in (("dW", wl.grad, wr.grad), ("db", bl.grad, br.grad), ("dW batched", dw, wr.grad), ("db batched", db, br.grad)):
        e = ((got.cpu().double() - want).abs().max() / want.abs().max()).item()
        print(f"[convd1 {nm}] max |d| / max |g| = {e:.2e}")
        assert e < 1e-5, (nm, e)
    # head conv2
    hw2, hb2 = U((1, 256, 3, 3), 920, -0.05, 0.05), U((1,), 921)
    hx, hg = U((b, 256, h, w), 922, 0.0, 1.0), U((b, 1, h, w), 923) * 1e-2
    a = [_leaf(t, DEV) for t in (hx, hw2, hb2)]
    out = G.Conv2dSame.apply(a[0], a[1], a[2], False, ops.PackedConv(), ops.PackedConv(), None)
    out.backward(hg.to(DEV))
    r = [t.double().requires_grad_(True) for t in (hx, hw2, hb2)]
    ref = F.conv2d(r[0], r[1], r[2], padding=1)
    ref.backward(hg.double())
    close(out.detach().cpu(), ref.detach().float(), 2e-5, 2e-5, "head conv2 forward")
    for nm, got, want in zip(("d_x", "d_w", "d_b"), a, r):
        e = ((got.grad.cpu().double() - want.grad).abs().max() / want.grad.abs().max()).item()
        print(f"[head conv2 {nm}] max |d| / max |g| = {e:.2e}")
        assert e < 5e-5, (nm, e)


def test_preloop_tensors_vs_reference(golden, precision):
    """The pre-loop of the HIP path — fused backbone kernels, gwc volume, cost aggregation, context network: what the GRU loop
    starts from — against the imported reference's own tensors (tests/golden/preloop_igev.npz) at 64x128 and at the non-square
    96x160, eager and as the captured forward runs it (same code path), both matrix-core modes (round-5 review item 7: the
    full-size oracle shares the product's module wiring; this pins that wiring against the reference at two shapes)."""
    from _preloop import capture_preloop, check_preloop
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    g = golden("preloop_igev")
    args = default_args("continuous_IGEVStereo")
    model = __models__["continuous_IGEVStereo"](args).eval()
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV)
    for H, W in ((int(a), int(b)) for a, b in g["sizes"]):
        img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
        coord = O.make_coord([H, W]).view(1, -1, 2)
        cap = capture_preloop(model, img1.to(DEV), img2.to(DEV), coord.to(DEV), torch.tensor([[1.0]], device=DEV))
        worst = check_preloop(cap, g, f"{H}x{W}", 5e-4, f"hip {precision}")
        print(f"[preloop hip {precision} {H}x{W}] " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


def test_autocast_training_step_keeps_resamplers_on_hip():
    """The reference trains under autocast + GradScaler (train_continuous_IGEV.py:206,288).  One such step (args.mixed_precision,
    Trainer(mixed_precision=True), eager) on a small problem: the loss is finite, and row a8 (pool2x / interp, update.py:94-102)
    went through the HIP forward kernels — counted by the launch-stream timing hooks — whatever dtype autocast handed them;
    there is no ATen branch left for them to take (nn/update.py::_hip_train_input raises for anything it does not serve)."""
    import math
    from anystereo.harness import timing
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer, synthetic_train_batch
    from anystereo.models import __models__, default_args
    from anystereo.nn import update as U
    args = default_args("continuous_IGEVStereo", mixed_precision=True)
    m = __models__["continuous_IGEVStereo"](args)
    fill_module_deterministic(m, base_seed=1)
    tr = Trainer(m.to(DEV), lr=2e-4, num_steps=1000, train_iters=3, max_disp=args.max_disp, mixed_precision=True, graph=False)
    batch = synthetic_train_batch(2, 64, 128, n_query=3000, seed=1, device=DEV)
    tr.step(batch)  # solver searches, packs
    timing.enable(True)
    loss, met = tr.step(batch)
    ks = timing.collect()
    timing.enable(False)
    assert math.isfinite(float(loss)) and all(math.isfinite(float(v)) for v in met.values())
    # per iteration: pool2x(net[1]), pool2x(net[0]), interp(net[2]), interp(net[1])  (update.py:118-128)
    assert ks.get("pool2x", {}).get("count", 0) == 2 * 3 and ks.get("interp", {}).get("count", 0) == 2 * 3, {k: v["count"] for k, v in ks.items()}
    # fp16 inputs are served by the kernels (cast in, cast back), not by a library fallback
    x = torch.randn(1, 16, 12, 20, device=DEV, dtype=torch.float16, requires_grad=True)
    y = U.pool2x(x)
    assert y.dtype == torch.float16 and y.shape == (1, 16, 6, 10)
    want = torch.nn.functional.avg_pool2d(x.float(), 3, stride=2, padding=1)
    assert (y.float() - want).abs().max() < 2e-3
    z = U.interp(x, torch.empty(1, 1, 24, 40))
    want = torch.nn.functional.interpolate(x.float(), (24, 40), mode="bilinear", align_corners=True)
    assert z.dtype == torch.float16 and (z.float() - want).abs().max() < 2e-3
    (y.float().sum() + z.float().sum()).backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()


@pytest.mark.parametrize("scope", ["grads", "step"])
def test_trainer_graphed_step_recaptures_and_matches_eager(scope, monkeypatch):
    """The Trainer's graphed step on a small problem, against the eager step fed the same sequence of batches: warm-up, capture,
    replays; a batch of ANOTHER shape (new query count and image size) runs one eager step, then captures its own graph; back to the
    first shape replays the cached graph (the parameters' .grad follow the replayed graph).
    Both scopes: the gradient half as the graph with clip + AdamW eager ("grads", the default), the whole step incl. a capturable
    AdamW as the graph ("step")."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer, synthetic_train_batch
    from anystereo.models import __models__, default_args
    monkeypatch.setenv("ANYSTEREO_TRAIN_GRAPH_SCOPE", scope)
    monkeypatch.setenv("ANYSTEREO_FUSED_ADAMW", "0")  # the two scopes then run the same foreach / capturable update arithmetic
    args = default_args("continuous_IGEVStereo")

    def fresh(graph):
        m = __models__["continuous_IGEVStereo"](args)
        fill_module_deterministic(m, base_seed=1)
        # the reference's schedule length: the first steps sit at the bottom of the one-cycle ramp (lr / 25), so two runs stay within
        # rounding of each other and a wrong gradient set or a stale graph cannot hide in training's own divergence
        return Trainer(m.to(DEV), lr=2e-4, num_steps=100000, train_iters=3, max_disp=args.max_disp, graph=graph)

    a = synthetic_train_batch(2, 64, 128, n_query=3000, seed=1, device=DEV)
    b = synthetic_train_batch(1, 96, 160, n_query=2048, seed=2, device=DEV)
    seq = [a, a, a, a, a, b, b, b, a, a]
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        eager, gr = fresh(False), fresh(True)
        assert gr.use_graph and gr.graph_scope == scope
        graphs, rels = [], []
        for i, bt in enumerate(seq):
            le, me = eager.step(tuple(t.clone() for t in bt))
            lg, mg = gr.step(tuple(t.clone() for t in bt))
            graphs.append(None if gr._graph is None else id(gr._graph["graph"]))
            rels.append(abs(float(le) - float(lg)) / abs(float(le)))
            assert rels[-1] <= 1e-3, (scope, i, float(le), float(lg), rels)
            for k in me:  # threshold fractions over 2-3 thousand queries: a handful of queries near 1 / 3 px flip between two runs
                tol = 2e-2 * max(abs(float(me[k])), 1e-3) if k == "epe" else 2e-2
                assert abs(float(me[k]) - float(mg[k])) <= tol, (scope, i, k, float(me[k]), float(mg[k]))
        assert graphs[2] is None and graphs[3] is not None and graphs[4] == graphs[3], graphs          # 3 warm-up steps, capture, replay
        # a new shape: one eager step (solver search), capture, replay; the first shape's graph is still cached
        assert graphs[5] is None and graphs[6] not in (None, graphs[4]) and graphs[7] == graphs[6] and graphs[8] == graphs[4] == graphs[9], graphs
        worst = 0.0
        for (n1, p1), (_, p2) in zip(eager.model.named_parameters(), gr.model.named_parameters()):
            worst = max(worst, ((p1 - p2).abs().max() / p1.abs().max().clamp_min(1e-12)).item())
        print(f"[graphed Trainer, scope {scope}] relative loss differences per step {[f'{r:.1e}' for r in rels]}; worst parameter deviation {worst:.2e}")
        assert worst < 5e-3, worst
    finally:
        torch.backends.cudnn.deterministic = prev


@pytest.mark.parametrize("batched", [False, True])
def test_training_fused_liif_mlp_equals_layered(batched):
    """Training forward / backward with the upsampler's per-query MLP as one forward kernel + one recomputing data-gradient kernel
    (grad.LiifMlpTail) against the layer-by-layer form (LiifGatherMlp1 + PointwiseLinear): same predictions, loss and gradients
    to the split arithmetic's rounding (the first layer's finish runs on the matrix cores in the fused form)."""
    from anystereo.harness.metrics import sequence_loss_multiscale
    from anystereo.harness.synthetic import fill_module_deterministic, tiny_train_case
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo")
    h, w, img1, img2, coord, gt, scale = tiny_train_case("igev")
    res = {}
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for fused in (False, True):
            model = __models__[args.model](args)
            fill_module_deterministic(model, base_seed=1)
            model = model.to(DEV).train()
            model.freeze_bn()
            model.batched_train_upsample = batched
            model.liif_up.fused_train_mlp = fused
            out = model(img1.to(DEV), img2.to(DEV), iters=3, hr_coord=coord.clone().to(DEV), scale=scale.to(DEV))
            gtd = gt.to(DEV)
            loss, _ = sequence_loss_multiscale(out[1], gtd, ((gtd < 512) & (gtd > 0)).float(), max_disp=args.max_disp)
            loss.backward()
            res[fused] = ([p.detach().clone() for p in out[1]], loss.item(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    finally:
        torch.backends.cudnn.deterministic = prev
    a, b_ = res[False], res[True]
    for i, (x, y) in enumerate(zip(a[0], b_[0])):
        close(y, x, 2e-5, 2e-5, f"prediction of iteration {i}")
    assert abs(a[1] - b_[1]) <= 1e-5 * abs(a[1])
    assert sorted(a[2]) == sorted(b_[2])
    gmax = max(g.abs().max().item() for g in a[2].values())
    worst = ("", 0.0)
    for n in a[2]:
        e = ((b_[2][n] - a[2][n]).abs().max() / max(a[2][n].abs().max().item(), 1e-30)).item()
        worst = max(worst, (n, e), key=lambda t: t[1])
        close(b_[2][n], a[2][n], 2e-3, 1e-6 * gmax, f"gradient of {n}")
    print(f"[fused LIIF MLP, batched={batched}] loss {a[1]:.6f} vs {b_[1]:.6f}; worst gradient deviation {worst[1]:.2e} of the tensor's max ({worst[0]})")


@pytest.mark.parametrize("fuse_first,sort", [(True, True), (True, False), (False, True)])
def test_liif_mlp_tail_function_vs_fp64(fuse_first, sort, monkeypatch):
    """grad.LiifMlpTail alone, with a shared second input (B1 < B) and queries outside the clamp range, against an fp64 torch
    statement of the same function: logits and every gradient (u0, u1, wrel, biases, the three later layers' weights).
    fuse_first: the first layer's scatter-adds and the wrel reduction inside the backward kernel (on queries sorted by source pixel
    as in training — long runs per pixel — and in random order — every lane its own run) or as separate kernels over d1."""
    from anystereo import grad as G, ops
    monkeypatch.setattr(G, "_LIIF_FUSE_FIRST", fuse_first)
    from anystereo.nn.liif import make_coord
    n, b1, h0, w0 = 3, 2, 6, 10
    nb = n * b1
    grid = make_coord([8 * h0, 8 * w0])
    idx = (U((nb, 900), 880, 0.0, 1.0) * grid.shape[0]).long().clamp(max=grid.shape[0] - 1)
    coord = torch.stack([grid[i] for i in idx]).contiguous()
    coord[0, 0] = torch.tensor([-1.0, 1.0])
    coord[1, 5] = torch.tensor([1.0, -1.0])
    if sort:
        _, key = ops.liif_rel_key(coord.to(DEV), [(h0, w0), (2 * h0, 2 * w0)], want_rel=False, want_key=True)
        perm = torch.argsort(key, dim=1).cpu()
        coord = torch.gather(coord, 1, perm.unsqueeze(-1).expand(-1, -1, 2)).contiguous()
    u0, u1 = U((nb, 128, h0, w0), 881), U((b1, 128, 2 * h0, 2 * w0), 882)
    wrel, bias1 = U((128, 4), 883), U((128,), 884)
    w2, bb2, w3, bb3, w4, bb4 = U((64, 128), 885, -0.15, 0.15), U((64,), 886), U((64, 64), 887, -0.2, 0.2), U((64,), 888), U((9, 64), 889, -0.2, 0.2), U((9,), 890)
    gout = U((nb, 9, coord.shape[1]), 891) * 1e-3
    sizes = [(h0, w0), (2 * h0, 2 * w0)]

    class Lin:  # what LiifTailPack.get reads of an nn.Linear
        def __init__(self, w_, b_):
            self.weight, self.bias = w_, b_
    leaves = [_leaf(t, DEV) for t in (u0, u1, wrel, bias1, w2, bb2, w3, bb3, w4, bb4)]
    w1full = torch.zeros((128, 4), device=DEV)  # LiifTailPack slices the relative-coordinate columns out of the first layer's weight
    with torch.no_grad():
        w1full.copy_(leaves[2])
    lin = [Lin(w1full, leaves[3]), Lin(leaves[4], leaves[5]), Lin(leaves[6], leaves[7]), Lin(leaves[8], leaves[9])]
    pack = ops.LiifTailPack().get(lin, [0, 2])
    c = coord.to(DEV)
    out = G.LiifMlpTail.apply(leaves[0], leaves[1], c, leaves[2], leaves[3], *leaves[4:], pack, ops.LiifMlpBwdPack(), None)
    out.backward(gout.to(DEV))
    # fp64 statement
    ref = [t.double().requires_grad_(True) for t in (u0, u1, wrel, bias1, w2, bb2, w3, bb3, w4, bb4)]
    rel, _ = ops.liif_rel_key(c, sizes)
    rel = rel.cpu().double()
    cc = coord.clamp(-1 + 1e-6, 1 - 1e-6)

    def nearest(n_, cv):
        return torch.round(((cv.float() + 1.0) * n_ - 1.0) / 2.0).long().clamp(0, n_ - 1)
    rows = []
    for e in range(nb):
        iy0, ix0 = nearest(h0, cc[e, :, 0]), nearest(w0, cc[e, :, 1])
        iy1, ix1 = nearest(2 * h0, cc[e, :, 0]), nearest(2 * w0, cc[e, :, 1])
        rows.append(ref[0][e][:, iy0, ix0] + ref[1][e % b1][:, iy1, ix1])
    x = torch.relu(torch.stack(rows) + torch.einsum("ck,bkq->bcq", ref[2], rel) + ref[3][None, :, None])
    x = torch.relu(torch.einsum("oc,bcq->boq", ref[4], x) + ref[5][None, :, None])
    x = torch.relu(torch.einsum("oc,bcq->boq", ref[6], x) + ref[7][None, :, None])
    want = torch.einsum("oc,bcq->boq", ref[8], x) + ref[9][None, :, None]
    want.backward(gout.double())
    close(out.detach().cpu(), want.detach().float(), 2e-5, 2e-5, "logits")
    for nm, got, r in zip(("u0", "u1", "wrel", "b1", "w2", "b2", "w3", "b3", "w4", "b4"), leaves, ref):
        e = ((got.grad.cpu().double() - r.grad).abs().max() / r.grad.abs().max()).item()
        print(f"[LiifMlpTail] d_{nm}: max |d| / max |g| = {e:.2e}")
        assert e < 2e-4, (nm, e)


@pytest.mark.parametrize("sort", [False, True])
def test_liif_gather_mlp1_backward(sort):
    """Fused gather + first Linear/ReLU and its backward (scatter-adds with in-wave run pre-summation), on random queries
    as drawn in training and on the same queries sorted by source pixel."""
    from anystereo import grad as G, ops
    from anystereo.nn.liif import make_coord
    b, c, h0, w0 = 2, 24, 5, 9
    grid = make_coord([4 * h0 * 2, 4 * w0 * 2])
    idx = (U((b, 700), 470, 0.0, 1.0) * grid.shape[0]).long().clamp(max=grid.shape[0] - 1)
    coord = torch.stack([grid[i] for i in idx]).contiguous()
    if sort:
        _, key = ops.liif_rel_key(coord.to(DEV), [(h0, w0), (2 * h0, 2 * w0)], want_rel=False, want_key=True)
        perm = torch.argsort(key, dim=1).cpu()
        coord = torch.gather(coord, 1, perm.unsqueeze(-1).expand(-1, -1, 2)).contiguous()
    u0, u1 = U((b, c, h0, w0), 471), U((b, c, 2 * h0, 2 * w0), 472)
    wrel, bias, gout = U((c, 4), 473), U((c,), 474), U((b, c, coord.shape[1]), 475)
    a = [_leaf(t, DEV) for t in (u0, u1, wrel, bias)]
    out = G.LiifGatherMlp1.apply(a[0], a[1], coord.to(DEV), a[2], a[3])
    out.backward(gout.to(DEV))
    r = [_leaf(t, dt=torch.float64) for t in (u0, u1, wrel, bias)]
    rel0, q0 = O.liif_query(r[0], coord.double())
    rel1, q1 = O.liif_query(r[1], coord.double())
    ref = torch.relu(q0 + q1 + torch.cat([rel0, rel1], -1) @ r[2].t() + r[3]).permute(0, 2, 1)
    ref.backward(gout.double())
    close(out, ref, 2e-5, 2e-5, "h1")
    for x, y, n in zip(a, r, ("d u0", "d u1", "d wrel", "d bias")):
        close(x.grad, y.grad, 1e-4, 1e-5, n)


def test_pointwise_linear_backward(precision):
    """MLP layer on the conv kernel: forward + dgrad (W^T as a 1x1 conv) + library wgrad vs autograd of F.linear in fp64."""
    from anystereo import grad as G, ops
    b, q = 2, 1500
    for cin, cout, relu in ((128, 64, True), (64, 64, True), (64, 9, False)):
        x, w, bias, g = U((b, cin, q), 480), U((cout, cin), 481, -0.2, 0.2), U((cout,), 482), U((b, cout, q), 483)
        a = [_leaf(t, DEV) for t in (x, w, bias)]
        y = G.PointwiseLinear.apply(a[0], a[1], a[2], relu, ops.PackedConv(), ops.PackedConv())
        y.backward(g.to(DEV))
        r = [_leaf(t, dt=torch.float64) for t in (x, w, bias)]
        ref = torch.matmul(r[1], r[0]) + r[2][None, :, None]
        ref = torch.relu(ref) if relu else ref
        ref.backward(g.double())
        tol = 2e-5 if precision == "fp32" else 5e-5
        close(y, ref, tol, 1e-5, "y")
        close(a[0].grad, r[0].grad, tol, 1e-5, "d x")
        close(a[1].grad, r[1].grad, 1e-4, 1e-5, "d w")
        close(a[2].grad, r[2].grad, 1e-4, 1e-5, "d b")


@pytest.mark.parametrize("cin,cout,k,relu", [(384, 256, 3, False), (128, 127, 3, True), (162, 64, 1, True), (64, 64, 3, True)])
def test_conv2d_same_backward(cin, cout, k, relu, precision):
    """Update-block conv in training: forward + dgrad on the implicit-GEMM kernel (transposed, flipped weights), library
    wgrad, vs autograd of F.conv2d in fp64."""
    import torch.nn.functional as F
    from anystereo import grad as G, ops
    b, h, w = 2, 9, 21
    x, wt = U((b, cin, h, w), 490), U((cout, cin, k, k), 491, -0.05, 0.05)
    bias, g = U((cout,), 492), U((b, cout, h, w), 493)
    a = [_leaf(t, DEV) for t in (x, wt, bias)]
    y = G.Conv2dSame.apply(a[0], a[1], a[2], relu, ops.PackedConv(), ops.PackedConv())
    y.backward(g.to(DEV))
    r = [_leaf(t, dt=torch.float64) for t in (x, wt, bias)]
    ref = F.conv2d(r[0], r[1], r[2], padding=k // 2)
    ref = torch.relu(ref) if relu else ref
    ref.backward(g.double())
    tol = 2e-5 if precision == "fp32" else 5e-5
    close(y, ref, tol, 1e-5, "y")
    close(a[0].grad, r[0].grad, tol, 1e-5, "d x")
    close(a[1].grad, r[1].grad, 2e-4, 1e-5, "d w")
    close(a[2].grad, r[2].grad, 2e-4, 1e-5, "d b")


@pytest.mark.parametrize("b,cin,cout,h,w,k", [(3, 40, 70, 6, 16, 3), (2, 162, 64, 5, 24, 1), (4, 33, 130, 7, 21, 3), (2, 7, 5, 3, 5, 1),
                                              (2, 64, 128, 4, 104, 3), (16, 128, 127, 10, 20, 3), (3, 64, 9, 1, 1000, 1), (2, 128, 64, 1, 333, 1)])
def test_conv2d_wgrad(b, cin, cout, h, w, k):
    """as_conv2d_wgrad (bf16 hi/lo split MFMA, split-K, bias gradient as a tile of ones) against fp64 autograd of F.conv2d:
    channel counts that do not fill the 128 x 32 tiles, widths with and without the 16-byte fetch path, rows longer than one
    96-pixel segment, tiny gradients (1e-7 scale: fp32 exponent range, no scaling pass), repeatable bit for bit."""
    import torch.nn.functional as F
    from anystereo import ops
    x, dy = U((b, cin, h, w), 530), U((b, cout, h, w), 531)
    for scale in (1.0, 1e-7):
        g = (dy * scale).contiguous()
        dw, db = ops.conv2d_wgrad(x.to(DEV), g.to(DEV), k)
        wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
        bias = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double(), wt, bias, padding=k // 2).backward(g.double())
        # error model: 3 bf16 products = 2^-16 relative per term, random over K = b*h*w terms of size <= |x||dy|
        lim = 4e-5 * scale * (b * h * w) ** 0.5
        assert (dw.double().cpu() - wt.grad).abs().max().item() <= lim, ((dw.double().cpu() - wt.grad).abs().max().item(), lim)
        assert (db.double().cpu() - bias.grad).abs().max().item() <= lim
        rel = (dw.double().cpu() - wt.grad).norm() / wt.grad.norm()
        assert rel < 2e-5, rel
        dw2, db2 = ops.conv2d_wgrad(x.to(DEV), g.to(DEV), k)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), "deterministic"
    dw3, none = ops.conv2d_wgrad(x.to(DEV), dy.to(DEV), k, want_bias=False)
    assert none is None and torch.isfinite(dw3).all()
    # the same reduction over a LIST of (x, dy) pairs (one per GRU iteration, no stacking copy): bit-identical to the stacked call
    xs = [t.contiguous().to(DEV) for t in x.split(1)]
    gs = [t.contiguous().to(DEV) for t in dy.split(1)]
    dw4, db4 = ops.conv2d_wgrad(xs, gs, k)
    dw5, db5 = ops.conv2d_wgrad(x.to(DEV), dy.to(DEV), k)
    assert torch.equal(dw4, dw5) and torch.equal(db4, db5)


def _log_uniform_grad(shape, seed, lo=1e-9, hi=1e-6):
    """Upstream gradients as cfg 4 produces them: magnitudes log-uniform in [lo, hi] (the masked-mean loss over 204 800 queries
    divides every path by the query count), random signs."""
    import math
    u = U(shape, seed, 0.0, 1.0)
    sgn = torch.where(U(shape, seed + 1, -1.0, 1.0) >= 0, 1.0, -1.0)
    return (sgn * torch.exp(u * (math.log(hi) - math.log(lo)) + math.log(lo))).float().contiguous()


@pytest.mark.parametrize("cin,cout,k", [(384, 256, 3), (128, 127, 3), (128, 64, 1)])
def test_dgrad_wgrad_production_magnitude_gradients(cin, cout, k):
    """dgrad (split-fp16 forward kernel on the transposed weights) and wgrad (bf16 split) of the update-block / MLP layer shapes
    with upstream gradients of 1e-9 .. 1e-6 — the magnitude cfg 4 really has — at the cfg-4 map size, against fp64 autograd.
    x = hi + lo/2048 keeps 22 bits only for |x| above ~6e-5, so the split dgrad is exercised the way harness/train.py runs it:
    on (gradient x Trainer.loss_scale = 4096), divided afterwards (exact, powers of two).  The same call WITHOUT the scale is
    evaluated next to it: it must be measurably worse, or the scale would be dead weight."""
    import torch.nn.functional as F
    from anystereo import grad as G, ops
    from anystereo.harness.train import Trainer  # noqa: F401  (the scale under test is the trainer's default)
    scale = 4096.0
    b, h, w = 4, 40, 80
    x, wt = U((b, cin, h, w), 610, -1.5, 1.5), (U((cout, cin, k, k), 611) * (3.0 / (cin * k * k)) ** 0.5).contiguous()
    bias = U((cout,), 612, -0.1, 0.1)
    g = _log_uniform_grad((b, cout, h, w), 613)
    r = [_leaf(t, dt=torch.float64) for t in (x, wt, bias)]
    F.conv2d(r[0], r[1], r[2], padding=k // 2).backward(g.double())
    prev = ops.get_precision()
    errs = {}
    try:
        for mode in ("split", "fp32"):
            ops.set_precision(mode)
            for s in ((scale, 1.0) if mode == "split" else (1.0,)):
                a = [_leaf(t, DEV) for t in (x, wt, bias)]
                y = G.Conv2dSame.apply(a[0], a[1], a[2], False, ops.PackedConv(), ops.PackedConv())
                y.backward((g * s).to(DEV))
                dx = a[0].grad.double().cpu() / s
                dw = a[1].grad.double().cpu() / s
                db = a[2].grad.double().cpu() / s
                errs[(mode, s)] = ((dx - r[0].grad).norm() / r[0].grad.norm(), (dw - r[1].grad).norm() / r[1].grad.norm(),
                                   (db - r[2].grad).norm() / r[2].grad.norm(), (dx - r[0].grad).abs().max() / r[0].grad.abs().max())
    finally:
        ops.set_precision(prev)
    for key, e in errs.items():
        print(f"[{cin}->{cout} k{k} {key}] dgrad rel {e[0]:.2e} (max-norm {e[3]:.2e}), wgrad rel {e[1]:.2e}, bias rel {e[2]:.2e}")
    sp, raw, f32 = errs[("split", scale)], errs[("split", 1.0)], errs[("fp32", 1.0)]
    # with the trainer's scale the split dgrad is as good as the exact-fp32 MFMA path (both limited by fp32 accumulation);
    # the weight gradient carries the bf16 split's ~2^-16 per product, averaged over K = b*h*w terms
    assert sp[0] < 2e-6 and sp[3] < 2e-6, sp
    assert f32[0] < 2e-6, f32
    assert sp[1] < 3e-5 and sp[2] < 3e-5 and f32[1] < 3e-5, (sp, f32)
    assert raw[0] > 4 * sp[0], f"unscaled split dgrad is not worse ({raw[0]:.2e} vs {sp[0]:.2e}): the loss scale would be dead weight"


@pytest.mark.parametrize("cin,cout,k,iters", [(384, 256, 3, 16), (128, 127, 3, 16), (64, 64, 3, 16), (128, 64, 1, 4)])
def test_wgrad_hip_vs_library_cfg4_shapes(cin, cout, k, iters):
    """ANYSTEREO_WGRAD=hip (default) routes every 1x1 / 3x3 weight gradient through as_conv2d_wgrad: bf16 hi + lo per operand,
    hi*hi + hi*lo + lo*hi, the lo*lo term dropped.  At the cfg-4 shapes (4 x 40 x 80 pixels x 16 iterations reduced in one
    launch, production-magnitude upstream gradients) it must be as close to the fp64 gradient as the library's fp32 wgrad
    (MIOpen via aten.convolution_backward) up to a stated factor: both are dominated by fp32 accumulation over K = 204 800
    terms, the split adds 2^-16 x sqrt-of-K averaging."""
    import torch.nn.functional as F
    from anystereo import ops
    b, h, w = 4, 40, 80
    xs = [U((b, cin, h, w), 700 + i, -1.5, 1.5) for i in range(iters)]
    gs = [_log_uniform_grad((b, cout, h, w), 800 + 2 * i) for i in range(iters)]
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    for x, g in zip(xs, gs):
        F.conv2d(x.double(), wt, None, padding=k // 2).backward(g.double())
    want = wt.grad
    dw, _ = ops.conv2d_wgrad([t.to(DEV) for t in xs], [t.to(DEV) for t in gs], k, want_bias=False)
    xcat, gcat = torch.cat(xs).to(DEV), torch.cat(gs).to(DEV)
    _, lib, _ = torch.ops.aten.convolution_backward(gcat, xcat, torch.zeros(cout, cin, k, k, device=DEV), None, [1, 1], [k // 2] * 2,
                                                   [1, 1], False, [0, 0], 1, [False, True, False])
    e_hip = ((dw.double().cpu() - want).norm() / want.norm()).item()
    e_lib = ((lib.double().cpu() - want).norm() / want.norm()).item()
    m_hip = ((dw.double().cpu() - want).abs().max() / want.abs().max()).item()
    print(f"[wgrad {cin}->{cout} k{k} x{iters}] hip rel {e_hip:.2e} (max-norm {m_hip:.2e}), library fp32 rel {e_lib:.2e}")
    assert e_hip < 2e-5 and m_hip < 5e-5, (e_hip, m_hip)          # the stated wgrad tolerance
    assert e_hip < max(20 * e_lib, 5e-6), (e_hip, e_lib)


@pytest.mark.parametrize("kind", ["conv3", "conv1_cat", "linear"])
def test_deferred_weight_gradients(kind):
    """A layer applied once per GRU iteration: its weight / bias gradients as ONE batched reduction per step (grad.WeightAnchor)
    against fp64 autograd of the same recurrence — three chained uses, one use whose output never reaches the loss, two
    steps in a row with a weight update in between (the anchor is renewed), and convz|convr as one concatenated weight."""
    import torch.nn as nn
    import torch.nn.functional as F
    from anystereo import grad as G
    torch.manual_seed(0)
    b, c, h, w = 2, 32, 7, 11
    mod = nn.Module()
    if kind == "linear":
        lin = nn.Linear(c, c)
        ref = nn.Linear(c, c).double()
        ref.load_state_dict(lin.state_dict())
        lin = lin.to(DEV)
        params, rparams = [lin.weight, lin.bias], [ref.weight, ref.bias]
    else:
        k = 3 if kind == "conv3" else 1
        convs = [nn.Conv2d(c, c // 2 if kind == "conv1_cat" else c, k, padding=k // 2) for _ in range(2 if kind == "conv1_cat" else 1)]
        refs = [nn.Conv2d(c, m.out_channels, k, padding=k // 2).double() for m in convs]
        for m, r in zip(convs, refs):
            r.load_state_dict(m.state_dict())
            m.to(DEV)
        params = [p for m in convs for p in (m.weight, m.bias)]
        rparams = [p for m in refs for p in (m.weight, m.bias)]
    for step in range(2):
        x0 = U((b, c, h * w) if kind == "linear" else (b, c, h, w), 520 + step)

        def run(x, dev_side):
            outs = []
            for i in range(4):
                if kind == "linear":
                    y = G.pointwise_linear(mod, "l", x, lin, True) if dev_side else torch.relu(torch.einsum("oc,bcq->boq", ref.weight, x) + ref.bias[None, :, None])
                elif dev_side:
                    y = G.conv2d_same(mod, "c", x, tuple(m.weight for m in convs) if len(convs) > 1 else convs[0].weight,
                                      tuple(m.bias for m in convs) if len(convs) > 1 else convs[0].bias, relu=True)
                else:
                    y = torch.relu(F.conv2d(x, torch.cat([m.weight for m in refs]), torch.cat([m.bias for m in refs]), padding=k // 2))
                outs.append(y)
                x = 0.5 * x + 0.25 * y
            return sum((i + 1) * o.sum() for i, o in enumerate(outs[:3]))  # the fourth use gets no gradient

        a = x0.to(DEV).requires_grad_(True)
        for p in params:
            p.grad = None
        run(a, True).backward()
        r = x0.double().requires_grad_(True)
        for p in rparams:
            p.grad = None
        run(r, False).backward()
        close(a.grad, r.grad, 1e-4, 1e-4, f"step {step}: d x")
        for i, (p, q) in enumerate(zip(params, rparams)):
            close(p.grad, q.grad, 2e-4, 1e-4, f"step {step}: d param {i}")
        with torch.no_grad():  # "optimizer step": the next forward must see the new weights and build a new anchor
            for p, q in zip(params, rparams):
                p.mul_(0.9)
                q.mul_(0.9)
    st = mod.__dict__["_wgrad_anchors"]["l" if kind == "linear" else "c"]
    assert st.done and not st.xs and not st.ds, "the stash is emptied by the anchor's backward"


def test_conv_gru_training_fused_gates():
    """ConvGRU under autograd: conv kernel + the two fused gate stages (forward and backward) vs autograd of the fp64 oracle,
    with the context passed as views of one tensor (the model's layout) — gradients to h, x, the context and all weights."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.update import ConvGRU
    b, h, w = 2, 9, 14
    gru = ConvGRU(128, 256)
    fill_module_deterministic(gru, 3)
    hh, ctx = torch.tanh(U((b, 128, h, w), 500, -2, 2)), U((b, 384, h, w), 501)
    x1, x2, g = U((b, 128, h, w), 502), U((b, 128, h, w), 503), U((b, 128, h, w), 504)
    ref_m = ConvGRU(128, 256).double()
    ref_m.load_state_dict(gru.state_dict())
    r = [_leaf(t, dt=torch.float64) for t in (hh, ctx, x1, x2)]
    O.conv_gru(ref_m, r[0], *r[1].split(128, dim=1), r[2], r[3]).backward(g.double())
    gru = gru.to(DEV).train()
    for fused in (True, False):
        gru.fused_gates = fused
        gru.zero_grad()
        a = [_leaf(t, DEV) for t in (hh, ctx, x1, x2)]
        out = gru(a[0], *a[1].split(128, dim=1), a[2], a[3])
        out.backward(g.to(DEV))
        for x, y, n in zip(a, r, ("d h", "d ctx", "d x1", "d x2")):
            close(x.grad, y.grad, 5e-5, 1e-6, f"{n} (fused_gates={fused})")
        for (n, p), (_, q) in zip(gru.named_parameters(), ref_m.named_parameters()):
            close(p.grad, q.grad, 2e-4, 1e-6, f"d {n} (fused_gates={fused})")


# ---------------------------------------------------------------------------------------------
# blocked split-fp16 link tensors between convolutions (as_conv_desc.src_bs / out_bs)
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(9, 14), (136, 240)])  # split-K + finish kernel / the MFMA epilogue
def test_conv_blocked_split_link_is_bit_identical(h, w):
    """A conv -> conv link through a BS8 tensor gives exactly the result of the fp32 link (the record pairs are what the
    consumer's loaders would compute), incl. a channel count that is no multiple of 8, a channel window written by two
    producers, a 1x1 consumer and mixed fp32 / BS8 sources."""
    from anystereo import _lib as Lb, ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        x = U((1, 48, h, w), 301).to(DEV)
        p1 = ops.PackedConv().get([(U((40, 48, 3, 3), 302) * 0.1).to(DEV)], [U((40,), 303).to(DEV)])
        p2 = ops.PackedConv().get([(U((64, 40, 3, 3), 304) * 0.1).to(DEV)], [U((64,), 305).to(DEV)])
        p2k1 = ops.PackedConv().get([(U((24, 40, 1, 1), 306) * 0.1).to(DEV)], [None])
        y = ops.conv2d([x], p1, act=Lb.ACT_RELU)
        ybs = ops.BS8.empty(1, 40, h, w, DEV)
        y_again = ops.conv2d([x], p1, act=Lb.ACT_RELU, out_bs=ybs)
        assert torch.equal(y, y_again)
        close(ybs.float(), y, 0, 2.0 ** -21 * y.abs().max().item(), "BS8 record pairs")
        assert ops.conv2d([x], p1, act=Lb.ACT_RELU, out_bs=ybs, bs_only=True) is None
        assert torch.equal(ops.conv2d([ybs], p2, act=Lb.ACT_TANH), ops.conv2d([y], p2, act=Lb.ACT_TANH))
        assert torch.equal(ops.conv2d([ybs], p2k1), ops.conv2d([y], p2k1))
        # two producers into one blocked tensor (channel windows 0 and 64), one mixed-source consumer
        pa = ops.PackedConv().get([(U((64, 48, 3, 3), 310) * 0.1).to(DEV)], [U((64,), 311).to(DEV)])
        pb = ops.PackedConv().get([(U((64, 48, 1, 1), 312) * 0.1).to(DEV)], [U((64,), 313).to(DEV)])
        pc = ops.PackedConv().get([(U((127, 176, 3, 3), 314) * 0.05).to(DEV)], [U((127,), 315).to(DEV)])
        cat = torch.empty((1, 128, h, w), device=DEV)
        cbs = ops.BS8.empty(1, 128, h, w, DEV)
        ops.conv2d([x], pa, act=Lb.ACT_RELU, out=cat, out_coff=0)
        ops.conv2d([x], pb, act=Lb.ACT_RELU, out=cat, out_coff=64)
        ops.conv2d([x], pa, act=Lb.ACT_RELU, out_bs=cbs, out_bs_coff=0, bs_only=True)
        ops.conv2d([x], pb, act=Lb.ACT_RELU, out_bs=cbs, out_bs_coff=64, bs_only=True)
        assert torch.equal(ops.conv2d([cbs, x], pc, act=Lb.ACT_RELU), ops.conv2d([cat, x], pc, act=Lb.ACT_RELU))
        assert torch.equal(ops.conv2d([x, cbs], pc_swap(ops, DEV), act=Lb.ACT_RELU), ops.conv2d([x, cat], pc_swap(ops, DEV), act=Lb.ACT_RELU))
        # GRU: r*h handed to the q conv as a blocked tensor only; the new hidden state with a blocked twin
        hs, xs = U((1, 128, h, w), 320).to(DEV), U((1, 128, h, w), 321).to(DEV)
        ctx = U((1, 384, h, w), 322).to(DEV)
        pzr = ops.PackedConv().get([(U((256, 256, 3, 3), 323) * 0.03).to(DEV)], [U((256,), 324).to(DEV)])
        pq = ops.PackedConv().get([(U((128, 256, 3, 3), 325) * 0.03).to(DEV)], [U((128,), 326).to(DEV)])
        z, rh = ops.conv2d([hs, xs], pzr, add=ctx, add_coff=0, epilogue=Lb.EPI_GRU_ZR, h=hs)
        hn = ops.conv2d([rh, xs], pq, add=ctx, add_coff=256, epilogue=Lb.EPI_GRU_Q, h=hs, z=z)
        rbs, hbs = ops.BS8.empty(1, 128, h, w, DEV), ops.BS8.empty(1, 128, h, w, DEV)
        z2, none = ops.conv2d([hs, xs], pzr, add=ctx, add_coff=0, epilogue=Lb.EPI_GRU_ZR, h=hs, out_bs=rbs, bs_only=True)
        assert none is None and torch.equal(z, z2)
        hn2 = ops.conv2d([rbs, xs], pq, add=ctx, add_coff=256, epilogue=Lb.EPI_GRU_Q, h=hs, z=z2, out_bs=hbs)
        assert torch.equal(hn, hn2)
        z3, rh3 = ops.conv2d([hbs, xs], pzr, add=ctx, add_coff=0, epilogue=Lb.EPI_GRU_ZR, h=hn2)
        z4, rh4 = ops.conv2d([hn, xs], pzr, add=ctx, add_coff=0, epilogue=Lb.EPI_GRU_ZR, h=hn)
        assert torch.equal(z3, z4) and torch.equal(rh3, rh4)
    finally:
        ops.set_precision(prev)


def pc_swap(ops, dev):
    return ops.PackedConv().get([(U((127, 176, 3, 3), 316) * 0.05).to(dev)], [U((127,), 317).to(dev)])


@pytest.mark.parametrize("hw", [(9, 14), (9, 15), (10, 128), (7, 2), (34, 60), (68, 120)])
def test_resamplers_blocked_split_output(hw):
    """pool2x / interp with a BS8 result hold exactly the split of the fp32 kernels' values (C not a multiple of 8 too).  Even
    widths take `pool2x_bs_even_kernel` (8-byte row loads), odd ones `pool2x_bs_kernel`: both are held to the same fp32 kernel,
    on one-block and multi-block shapes, on output widths that are and are not multiples of 64, and on the loop's own 1/8- and
    1/16-resolution maps."""
    from anystereo import ops
    hh, ww = hw
    for c in (16, 13):
        x = U((2, c, hh, ww), 330 + c).to(DEV)
        for bs, ref in ((ops.pool2x_bs(x), ops.pool2x(x)), (ops.interp_bs(x, 2 * hh, 2 * ww - 1), ops.interp(x, 2 * hh, 2 * ww - 1))):
            assert tuple(bs.shape) == tuple(ref.shape)
            hi = ref.half()
            lo = ((ref - hi.float()) * 2048.0).half()
            b, _, c8, h, w, _ = bs.t.shape
            got_hi = bs.t[:, 0].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w)
            got_lo = bs.t[:, 1].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w)
            assert torch.equal(got_hi[:, :c], hi) and torch.equal(got_lo[:, :c], lo)
            assert (got_hi[:, c:] == 0).all() and (got_lo[:, c:] == 0).all()


def test_update_block_links_on_off_equal(monkeypatch):
    """The whole update block with blocked split-fp16 links == with fp32 links.  A link tensor holds exactly the operand split
    the consumer would compute, so every convolution sees identical operands; the only difference is that an all-blocked
    convolution on a small map runs 64-channel tiles with another split-K factor (fp32 partial sums grouped differently):
    equal to fp32 rounding of that regrouping, bit for bit where no K split is involved
    (test_conv_blocked_split_link_is_bit_identical)."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models.base import default_args
    from anystereo.nn import update as UP
    from anystereo import ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        args = default_args("continuous_IGEVStereo")
        ub = UP.BasicMultiUpdateBlock(args, hidden_dims=args.hidden_dims, geo_channels=8).eval()
        fill_module_deterministic(ub, base_seed=7)
        ub = ub.to(DEV)
        h, w = 24, 40
        net0 = [U((1, 128, h >> i, w >> i), 340 + i).to(DEV) for i in range(3)]
        inp = [list(U((1, 384, h >> i, w >> i), 350 + i).to(DEV).split(128, dim=1)) for i in range(3)]
        corr, disp = U((1, 162, h, w), 360).to(DEV), U((1, 1, h, w), 361, 0.0, 30.0).to(DEV)
        outs = []
        for on in (True, False):
            monkeypatch.setattr(UP, "_LINKS_ENV", on)
            with torch.no_grad():
                net = [n.clone() for n in net0]
                for _ in range(2):  # second pass consumes the hidden states' blocked twins
                    net, delta = ub(net, inp, corr, disp)
                outs.append([t.clone() for t in net] + [delta.clone()])
        for a, b in zip(*outs):
            close(a, b, 2e-6, 2e-6, "links on vs off")
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("h,w", [(9, 14), (136, 240)])
def test_blocked_split_partial_block_and_passthrough(h, w):
    """A 127-channel result + the 7x7 kernel's input pass-through in slot 127 of the same blocked tensor (the motion
    features, update.py:91), and a 43-channel result whose pad slots must read as zeros."""
    from anystereo import _lib as Lb, ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        x = U((1, 128, h, w), 401).to(DEV)
        disp = U((1, 1, h, w), 402, -3.0, 40.0).to(DEV)
        w7, b7 = (U((64, 1, 7, 7), 403) * 0.2).to(DEV), (U((64,), 404) * 0.1).to(DEV)
        pe = ops.PackedConv().get([(U((127, 128, 3, 3), 405) * 0.05).to(DEV)], [U((127,), 406).to(DEV)])
        pz = ops.PackedConv().get([(U((64, 128, 3, 3), 407) * 0.05).to(DEV)], [U((64,), 408).to(DEV)])
        ref = torch.empty((1, 128, h, w), device=DEV)
        d1 = ops.conv7x7_c1_relu(disp, w7, b7, copy_out=ref, copy_coff=127)
        ops.conv2d([x], pe, act=Lb.ACT_RELU, out=ref, out_coff=0)
        for order in (0, 1):  # the two producers in either order
            bs = ops.BS8.empty(1, 128, h, w, DEV)
            bs.t.fill_(float("nan"))
            if order == 0:
                d2 = ops.conv7x7_c1_relu(disp, w7, b7, copy_out=bs, copy_coff=127)
            ops.conv2d([x], pe, act=Lb.ACT_RELU, out_bs=bs, out_bs_coff=0, bs_only=True)
            if order == 1:
                d2 = ops.conv7x7_c1_relu(disp, w7, b7, copy_out=bs, copy_coff=127)
            assert torch.equal(d1, d2)
            assert torch.isfinite(bs.t.float()).all()
            assert torch.equal(ops.conv2d([bs], pz, act=Lb.ACT_TANH), ops.conv2d([ref], pz, act=Lb.ACT_TANH))
        p43 = ops.PackedConv().get([(U((43, 128, 1, 1), 409) * 0.05).to(DEV)], [U((43,), 410).to(DEV)])
        b43 = ops.BS8.empty(1, 43, h, w, DEV)
        b43.t.fill_(float("nan"))
        y43 = ops.conv2d([x], p43, act=Lb.ACT_SIGMOID, out_bs=b43)
        full = b43.t[:, 0].permute(0, 1, 4, 2, 3).reshape(1, 48, h, w)
        assert torch.isfinite(b43.t.float()).all() and (full[:, 43:] == 0).all()
        close(b43.float(), y43, 0, 2.0 ** -21, "43-channel blocked copy")
    finally:
        ops.set_precision(prev)


@pytest.mark.parametrize("h,w", [(9, 14), (136, 240)])  # sequential fallback (split-K) / the fused grid
def test_conv_dual_launch_equals_two_launches(h, w, precision):
    """as_conv_desc.dual: two same-shape convolutions in one launch == the two launches, bit for bit (fp32 and blocked outputs,
    fp32 and blocked second source)."""
    from anystereo import _lib as Lb, ops
    xa, xb = U((1, 64, h, w), 501).to(DEV), U((1, 64, h, w), 502).to(DEV)
    pa = ops.PackedConv().get([(U((64, 64, 3, 3), 503) * 0.1).to(DEV)], [U((64,), 504).to(DEV)])
    pb = ops.PackedConv().get([(U((64, 64, 3, 3), 505) * 0.1).to(DEV)], [U((64,), 506).to(DEV)])
    ref = torch.empty((1, 128, h, w), device=DEV)
    ops.conv2d([xa], pa, act=Lb.ACT_RELU, out=ref, out_coff=0)
    ops.conv2d([xb], pb, act=Lb.ACT_RELU, out=ref, out_coff=64)
    got = torch.empty((1, 128, h, w), device=DEV)
    ops.conv2d([xa], pa, act=Lb.ACT_RELU, out=got, out_coff=0, dual={"src": xb, "pack": pb, "out_coff": 64})
    assert torch.equal(got, ref)
    if precision == "split":
        bs_ref, bs_got = ops.BS8.empty(1, 128, h, w, DEV), ops.BS8.empty(1, 128, h, w, DEV)
        xbb = ops.BS8.empty(1, 64, h, w, DEV)
        pid = ops.PackedConv().get([torch.eye(64, device=DEV).view(64, 64, 1, 1).contiguous()], [None])
        ops.conv2d([xb], pid, out_bs=xbb, bs_only=True)  # xb as a blocked tensor
        ops.conv2d([xa], pa, act=Lb.ACT_RELU, out_bs=bs_ref, out_bs_coff=0, bs_only=True)
        ops.conv2d([xb], pb, act=Lb.ACT_RELU, out_bs=bs_ref, out_bs_coff=64, bs_only=True)
        ops.conv2d([xa], pa, act=Lb.ACT_RELU, out_bs=bs_got, out_bs_coff=0, bs_only=True,
                   dual={"src": xbb, "pack": pb, "out_bs_coff": 64})
        assert torch.equal(bs_got.t, bs_ref.t)


@pytest.mark.parametrize("b,h,w", [(1, 9, 14), (2, 17, 30), (1, 136, 240)])  # sequential fallback (split-K) / batch 2 / the fused grid
def test_conv_dual_launch_residual_act_separate_outputs(b, h, w, precision):
    """as_conv_desc.dual, round-6 form: the second convolution with its own residual (h2), its own activation (act2) and DENSE
    outputs of its own (out_b / out_bs_b) == the two single launches, bit for bit — fp32 outputs, blocked outputs, same and
    different sources: the paired heads of a context-network scale (nn/encoders.py::MultiBasicEncoder._heads)."""
    from anystereo import _lib as Lb, ops
    c = 128
    x, xb = U((b, c, h, w), 511).to(DEV), U((b, c, h, w), 512).to(DEV)
    pa = ops.PackedConv().get([(U((c, c, 3, 3), 513) * 0.05).to(DEV)], [U((c,), 514).to(DEV)])
    pb = ops.PackedConv().get([(U((c, c, 3, 3), 515) * 0.05).to(DEV)], [U((c,), 516).to(DEV)])
    ha, hb = U((b, c, h, w), 517).to(DEV), U((b, c, h, w), 518).to(DEV)
    # (1) same source, residual on both, fp32 outputs, different activations
    ra = ops.conv2d([x], pa, act=Lb.ACT_RELU, h=ha)
    rb = ops.conv2d([x], pb, act=Lb.ACT_NONE, h=hb)
    ga, gb = ops.conv2d([x], pa, act=Lb.ACT_RELU, h=ha, dual={"src": x, "pack": pb, "h": hb, "act": Lb.ACT_NONE, "out": True})
    assert torch.equal(ga, ra) and torch.equal(gb, rb)
    # (2) tanh | relu without residual, two sources (the heads' last convolutions)
    ra, rb = ops.conv2d([x], pa, act=Lb.ACT_TANH), ops.conv2d([xb], pb, act=Lb.ACT_RELU)
    ga, gb = ops.conv2d([x], pa, act=Lb.ACT_TANH, dual={"src": xb, "pack": pb, "act": Lb.ACT_RELU, "out": True})
    assert torch.equal(ga, ra) and torch.equal(gb, rb)
    close(ga, torch.tanh(ops.conv2d([x], pa)), 0, 5e-7, "tanh epilogue vs ATen tanh")
    if precision == "split":
        # (3) blocked outputs only, blocked second source, residual
        xbb = ops.BS8.empty(b, c, h, w, DEV)
        pid = ops.PackedConv().get([torch.eye(c, device=DEV).view(c, c, 1, 1).contiguous()], [None])
        ops.conv2d([xb], pid, out_bs=xbb, bs_only=True)
        ra_bs, rb_bs, ga_bs, gb_bs = (ops.BS8.empty(b, c, h, w, DEV) for _ in range(4))
        ops.conv2d([x], pa, act=Lb.ACT_RELU, h=ha, out_bs=ra_bs, bs_only=True)
        ops.conv2d([xbb], pb, act=Lb.ACT_RELU, h=hb, out_bs=rb_bs, bs_only=True)
        ops.conv2d([x], pa, act=Lb.ACT_RELU, h=ha, out_bs=ga_bs, bs_only=True, dual={"src": xbb, "pack": pb, "h": hb, "out_bs": gb_bs})
        assert torch.equal(ga_bs.t, ra_bs.t) and torch.equal(gb_bs.t, rb_bs.t)
    with pytest.raises(RuntimeError, match="residual"):
        ops.conv2d([x], pa, h=ha, dual={"src": x, "pack": pb, "out": True})


def test_context_heads_paired_equals_separate():
    """MultiBasicEncoder's heads per scale as dual launches (with tanh | relu in the last epilogue) == head by head with ATen's
    tanh / relu behind them: the convolutions bit-identical, tanh within 1 ulp-scale of ATen's."""
    from anystereo import _lib as Lb
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.encoders import MultiBasicEncoder
    net = MultiBasicEncoder(output_dim=[[128, 128, 128], [128, 128, 128]], norm_fn="batch", downsample=2).eval()
    fill_module_deterministic(net, base_seed=3)
    net = net.to(DEV)
    x = (U((1, 3, 64, 96), 521) * 2).to(DEV)
    with torch.no_grad():
        net.paired_heads = False
        want = net(x, num_layers=3)
        net.paired_heads = True
        got = net(x, num_layers=3)
        net.head_acts = (Lb.ACT_TANH, Lb.ACT_RELU)
        got_act = net(x, num_layers=3)
        net.head_acts = None
    for lv, (w_, g_, ga_) in enumerate(zip(want, got, got_act)):
        for k in range(2):
            assert torch.equal(g_[k], w_[k]), (lv, k)
        close(ga_[0], torch.tanh(w_[0]), 0, 5e-7, f"hidden head, level {lv}")
        assert torch.equal(ga_[1], torch.relu(w_[1]))


@pytest.mark.parametrize("b,cin,cout,h,w", [(1, 128, 256, 136, 240), (2, 32, 100, 9, 14), (1, 16, 64, 24, 40)])
def test_conv_relu_taps_epilogue(b, cin, cout, h, w):
    """AS_EPI_RELU_TAPS + as_tap_shift_sum(groups) == conv3x3(relu(conv3x3(x))) with a 1-channel second conv (DispHead)."""
    from anystereo import _lib as Lb, ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        x = U((b, cin, h, w), 601)
        w1, b1 = U((cout, cin, 3, 3), 602) * 0.05, U((cout,), 603) * 0.1
        w2, b2 = U((1, cout, 3, 3), 604) * 0.05, U((1,), 605)
        add = U((b, 1, h, w), 606)
        p1 = ops.PackedConv().get([w1.to(DEV)], [b1.to(DEV)])
        taps = ops.conv2d([x.to(DEV)], p1, act=Lb.ACT_RELU, epilogue=Lb.EPI_RELU_TAPS, tap_w=w2[0].reshape(cout, 9).contiguous().to(DEV))
        assert tuple(taps.shape) == (b, (cout + 63) // 64 * 9, h, w)
        got = ops.tap_shift_sum(taps, b2.to(DEV), add.to(DEV))
        ref = add.double() + _ref_conv(torch.relu(_ref_conv(x, w1, b1, 1)), w2, b2, 1)
        close(got, ref, 2e-5, 2e-5, "fused head")
        again = ops.tap_shift_sum(ops.conv2d([x.to(DEV)], p1, act=Lb.ACT_RELU, epilogue=Lb.EPI_RELU_TAPS,
                                             tap_w=w2[0].reshape(cout, 9).contiguous().to(DEV)), b2.to(DEV), add.to(DEV))
        assert torch.equal(got, again)  # fixed summation order
    finally:
        ops.set_precision(prev)


def test_conv7x7_blocked_split_output():
    """The 7x7 one-channel conv with a BS8 result holds exactly the split of its fp32 result (+ the disparity pass-through)."""
    from anystereo import ops
    for cout, h, w in ((64, 20, 37), (13, 9, 14)):
        disp = U((2, 1, h, w), 701, -2.0, 30.0).to(DEV)
        w7, b7 = (U((cout, 1, 7, 7), 702) * 0.2).to(DEV), (U((cout,), 703) * 0.1).to(DEV)
        ref = ops.conv7x7_c1_relu(disp, w7, b7)
        bs = ops.BS8.empty(2, cout, h, w, DEV)
        bs.t.fill_(float("nan"))
        assert ops.conv7x7_c1_relu(disp, w7, b7, out=bs) is bs
        hi = ref.half()
        lo = ((ref - hi.float()) * 2048.0).half()
        b, _, c8, hh, ww, _ = bs.t.shape
        got_hi = bs.t[:, 0].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, hh, ww)
        got_lo = bs.t[:, 1].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, hh, ww)
        assert torch.equal(got_hi[:, :cout], hi) and torch.equal(got_lo[:, :cout], lo)
        assert (got_hi[:, cout:] == 0).all() and (got_lo[:, cout:] == 0).all()


def test_hidden_state_twin_is_dropped_after_inplace_update():
    """A hidden state modified in place by the caller must not be read through its (now stale) blocked twin."""
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn import update as UP
    from anystereo import ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        gru = UP.ConvGRU(128, 128).eval()
        fill_module_deterministic(gru, base_seed=9)
        gru = gru.to(DEV)
        h0, x = U((1, 128, 12, 20), 801).to(DEV), U((1, 128, 12, 20), 802).to(DEV)
        ctx = list(U((1, 384, 12, 20), 803).to(DEV).split(128, dim=1))
        with torch.no_grad():
            h1 = gru(h0, *ctx, x)
            assert UP._twin(h1) is not h1                      # twin attached and valid
            ref = gru(h1.clone().mul_(0.5), *ctx, x)           # fresh tensor: no twin
            h1.mul_(0.5)                                       # caller edits the hidden state in place
            assert UP._twin(h1) is h1                          # stale twin ignored
            assert torch.equal(gru(h1, *ctx, x), ref)
    finally:
        ops.set_precision(prev)


# ---------------------------------------------------------------------------------------------
# fused LIIF inference pipeline (csrc/liif_fused.hip): affinity without the copy, first layer at low resolution with a
# channels-last result, ONE per-query kernel (gather + MLP + softmax + convex combination)
# ---------------------------------------------------------------------------------------------

def _liif_module(seed=7, two=True):
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.liif import liif_out_multi_scale_Training
    up = liif_out_multi_scale_Training(encoder_dim=208 if two else 176, mlphidden_list=[128, 64, 64], pos_dim=0, unfold="with_v2ISU",
                                       affinity_settings={"win_w": 3, "win_h": 3, "dilation": [1, 2, 4, 8]},
                                       number_input=2 if two else 1, chanels=[176, 32] if two else [176]).eval()
    fill_module_deterministic(up, base_seed=seed, gain=2.0)
    return up.to(DEV)


def test_liif_fused_pipeline_golden(golden):
    """Against the reference's own outputs (G6: liif.npz): affinity, mask logits (`liif_up`'s return value) and the convex
    upsampling result of the fused pipeline; the caller's coordinates come back clamped (submodule.py:366)."""
    from anystereo import ops
    g = golden("liif")
    x4, x2 = g["x4"].to(DEV), g["x2"].to(DEV)
    close(ops.liif_affinity([g["feat"].to(DEV)]), g["aff"], 1e-5, 2e-6, "affinity (tile kernel)")
    f = g["feat"].to(DEV)
    close(ops.liif_affinity([f[:, :8].contiguous(), f[:, 8:].contiguous()]), g["aff"], 1e-5, 2e-6, "affinity, two sources")
    up = _liif_module()
    coord = g["coord"].clone().to(DEV)
    sv = torch.tensor([1.5], device=DEV)
    with torch.no_grad():
        assert up.fused_ok([[x4[:, :48], x4[:, 48:]], [x2]], coord) or ops.get_precision() != "split"
        prev = ops.get_precision()
        ops.set_precision("split")
        try:
            out, logits = up.upsample_fused([[x4[:, :48].contiguous(), x4[:, 48:].contiguous()], [x2]], coord, g["dlow"].to(DEV), sv,
                                            want_logits=True)
        finally:
            ops.set_precision(prev)
    close(logits, g["mask"], 2e-5, 2e-5, "fused tail: mask logits")
    close(out[:, 0], g["convex"], 2e-5, 2e-5, "fused tail: upsampled disparity")
    assert torch.equal(coord.cpu(), g["coord"].clamp(-1 + 1e-6, 1 - 1e-6)), "coordinates are clamped in place"


@pytest.mark.parametrize("two,b,h,w,s,nq", [(True, 2, 9, 14, 1.5, None), (False, 1, 7, 11, 2.95, None), (True, 1, 12, 20, 1.0, 1000),
                                             (True, 3, 5, 9, 2.0, 33)])
def test_liif_fused_tail_vs_staged(two, b, h, w, s, nq):
    """The fused pipeline against the fp64 oracle and against the staged HIP path on the same module: batch > 1 (tiles that
    straddle batch elements), a ragged query count (last tile partly empty), one and two inputs, scales 1 .. 2.95, queries
    exactly on +-1 (clamp) and on cell borders."""
    from anystereo import ops
    up = _liif_module(seed=11, two=two)
    x4 = U((b, 176, h, w), 201, -1.5, 1.5).to(DEV)
    x2 = U((b, 32, 2 * h, 2 * w), 202, -1.5, 1.5).to(DEV)
    grid = O.make_coord([round(4 * h * s), round(4 * w * s)])
    if nq is not None:
        idx = (U((nq,), 203, 0.0, 1.0) * grid.shape[0]).long().clamp(max=grid.shape[0] - 1)
        grid = grid[idx]
        grid[0] = torch.tensor([-1.0, 1.0])
        grid[1] = torch.tensor([1.0, -1.0])
    coord = grid.view(1, -1, 2).repeat(b, 1, 1).contiguous()
    disp = U((b, 1, h, w), 204, 0.0, 40.0).to(DEV)
    sv = torch.full((b,), float(s), device=DEV)
    feats = [x4, x2] if two else [x4]
    parts = [[x4[:, :48].contiguous(), x4[:, 48:].contiguous()]] + ([[x2]] if two else [])
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        with torch.no_grad():
            c1 = coord.clone().to(DEV)
            out, logits = up.upsample_fused(parts, c1, disp, sv, want_logits=True)
            c2 = coord.clone().to(DEV)
            staged_logits = up(feats, c2, sv.view(-1, 1))
            staged = ops.convex_upsample(disp, staged_logits, c2.clamp(-1 + 1e-6, 1 - 1e-6), scale=sv, mask_is_logits=True)
    finally:
        ops.set_precision(prev)
    assert out.shape == (b, 1, coord.shape[1]) and torch.isfinite(out).all()
    close(logits, staged_logits, 3e-5, 3e-5, "fused vs staged logits")
    close(out, staged, 3e-5, 3e-5, "fused vs staged disparity")
    up64 = up.cpu().double()
    want_mask = O.liif_up_mask(up64, [t.cpu().double() for t in feats], coord.double())
    d = disp.cpu().double() * 4.0 * s
    want = O.convex_upsample(d, torch.softmax(want_mask, 1), coord.double().clamp(-1 + 1e-6, 1 - 1e-6)).unsqueeze(1)
    close(logits, want_mask, 3e-5, 3e-5, "fused logits vs fp64 oracle")
    close(out, want, 3e-5, 3e-5, "fused disparity vs fp64 oracle")
    up.float().to(DEV)


@pytest.mark.parametrize("b,h,w,s", [(1, 17, 29, 1.0), (2, 9, 13, 2.95), (1, 24, 40, 1.5), (3, 8, 10, 1.0), (1, 34, 60, 2.0)])
def test_liif_tail_patch_order_is_bit_identical(b, h, w, s, monkeypatch):
    """The tail's raster-patch query order (as_liif_query_rows: row length found on the device; waves of a block share a 32-column
    tile of consecutive query rows) against the round-5 order (32-query runs): every query is processed once either way and a
    query's result depends on its own operand column only, so disparities and logits must be BIT-identical — ragged row lengths
    (R % 32 != 0), row counts that do not fill the last patch, batch > 1 (patches straddling batch elements), both tail forms.
    Random / permuted queries: the detector answers 0 and the old order runs."""
    from anystereo import ops
    up = _liif_module(seed=17, two=True)
    x4 = U((b, 176, h, w), 221, -1.5, 1.5).to(DEV)
    x2 = U((b, 32, 2 * h, 2 * w), 222, -1.5, 1.5).to(DEV)
    hq, wq = round(4 * h * s), round(4 * w * s)
    grid = O.make_coord([hq, wq])
    disp = U((b, 1, h, w), 224, 0.0, 40.0).to(DEV)
    sv = torch.full((b,), float(s), device=DEV)
    parts = [[x4[:, :48].contiguous(), x4[:, 48:].contiguous()], [x2]]
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        with torch.no_grad():
            coord = grid.view(1, -1, 2).repeat(b, 1, 1).contiguous().to(DEV)
            assert int(ops.liif_query_rows(coord).item()) == wq
            cropped = grid.view(hq, wq, 2)[2:-1, 3:-2].reshape(1, -1, 2).repeat(b, 1, 1).contiguous().to(DEV)  # pad_for_multi_train's crop
            assert int(ops.liif_query_rows(cropped).item()) == wq - 5
            perm = torch.argsort(U((hq * wq,), 225, 0.0, 1.0))
            shuffled = grid.reshape(-1, 2)[perm].view(1, -1, 2).repeat(b, 1, 1).contiguous().to(DEV)
            assert int(ops.liif_query_rows(shuffled).item()) in (0, 1)  # no raster structure (1: a single-query "row", never used)
            for direct in (False, True):
                up.direct_second_input = direct
                for cd in (coord, cropped, shuffled):
                    monkeypatch.setattr(ops, "PATCH_ORDER", True)
                    o1, l1 = up.upsample_fused(parts, cd.clone(), disp, sv, want_logits=True)
                    monkeypatch.setattr(ops, "PATCH_ORDER", False)
                    o0, l0 = up.upsample_fused(parts, cd.clone(), disp, sv, want_logits=True)
                    assert torch.equal(o1, o0) and torch.equal(l1, l0), (direct, tuple(cd.shape))
    finally:
        up.direct_second_input = False
        ops.set_precision(prev)


@pytest.mark.parametrize("b,h,w,s,nq", [(1, 17, 29, 1.0, None), (2, 9, 13, 2.95, 777), (1, 24, 40, 1.5, None)])
def test_liif_tail_direct_second_input(b, h, w, s, nq):
    """The tail with the second input handed over as raw channels-last rows (its first-layer product taken per query,
    as_liif_tail_direct) against the form that gathers that input's low-resolution first-layer rows, and against the fp64
    oracle: same logits and disparity up to the fp32 order of a K = 40 sum; rows are a zero-padded channels-last copy."""
    from anystereo import ops
    up = _liif_module(seed=13, two=True)
    x4 = U((b, 176, h, w), 211, -1.5, 1.5).to(DEV)
    x2 = U((b, 32, 2 * h, 2 * w), 212, -1.5, 1.5).to(DEV)
    grid = O.make_coord([round(4 * h * s), round(4 * w * s)])
    if nq is not None:
        idx = (U((nq,), 213, 0.0, 1.0) * grid.shape[0]).long().clamp(max=grid.shape[0] - 1)
        grid = grid[idx]
        grid[0] = torch.tensor([-1.0, 1.0])
    coord = grid.view(1, -1, 2).repeat(b, 1, 1).contiguous()
    disp = U((b, 1, h, w), 214, 0.0, 40.0).to(DEV)
    sv = torch.full((b,), float(s), device=DEV)
    parts = [[x4[:, :48].contiguous(), x4[:, 48:].contiguous()], [x2]]
    prev = ops.get_precision()
    ops.set_precision("split")
    outs = {}
    try:
        with torch.no_grad():
            aff = ops.liif_affinity([x2])
            rows = ops.liif_rows_cl([x2, aff])
            want_rows = torch.cat([x2, aff, torch.zeros(b, 8, 2 * h, 2 * w, device=DEV)], 1).permute(0, 2, 3, 1).reshape(b, -1, 48)
            assert torch.equal(rows, want_rows), "rows = channels-last copy"
            for direct in (True, False):
                up.direct_second_input = direct
                outs[direct] = up.upsample_fused(parts, coord.clone().to(DEV), disp, sv, want_logits=True)
    finally:
        up.__dict__.pop("direct_second_input", None)
        ops.set_precision(prev)
    close(outs[True][1], outs[False][1], 3e-5, 3e-5, "direct vs low-resolution-rows logits")
    close(outs[True][0], outs[False][0], 3e-5, 3e-5, "direct vs low-resolution-rows disparity")
    up64 = up.cpu().double()
    want_mask = O.liif_up_mask(up64, [x4.cpu().double(), x2.cpu().double()], coord.double())
    close(outs[True][1], want_mask, 3e-5, 3e-5, "direct logits vs fp64 oracle")
    up.float().to(DEV)


def test_liif_lowres_channels_last():
    """First MLP layer at low resolution, channels-last: against the fp64 product; three sources, a column window of the
    weight, pixel counts that are not multiples of 32."""
    from anystereo import ops
    b, h, w = 2, 7, 13
    srcs = [U((b, c, h, w), 210 + i).to(DEV) for i, c in enumerate((48, 128, 8))]
    wt = (U((128, 228), 215) * 0.2).to(DEV)
    got = ops.liif_lowres_cl(srcs, ops.LiifLowresPack().get(wt, 0, 184))
    x = torch.cat(srcs, 1).double().permute(0, 2, 3, 1).reshape(b, h * w, 184)
    want = x @ wt[:, :184].double().t()
    close(got, want, 2e-5, 2e-5, "lowres first layer (K = 184)")
    srcs = [U((1, c, 2 * h, 2 * w), 220 + i).to(DEV) for i, c in enumerate((32, 8))]
    got = ops.liif_lowres_cl(srcs, ops.LiifLowresPack().get(wt, 186, 40))
    x = torch.cat(srcs, 1).double().permute(0, 2, 3, 1).reshape(1, 4 * h * w, 40)
    close(got, x @ wt[:, 186:226].double().t(), 2e-5, 2e-5, "lowres first layer (K = 40, column offset)")


@pytest.mark.parametrize("b,h,w,g,d,L", [(2, 3, 20, 8, 48, 2), (1, 5, 37, 0, 0, 4), (1, 7, 70, 8, 48, 2), (1, 136, 240, 8, 48, 2)])
def test_lookup_convc1_fused(b, h, w, g, d, L):
    """lookup -> convc1 -> ReLU as one kernel (geometry.py:34-60 + update.py:84-85) against the fp64 oracle: both model
    geometries, zero-pad edges, pixel counts that do not fill the last 64-pixel block, batch 2; the blocked split-fp16
    result carries the same values as the fp32 one."""
    from anystereo import ops
    f1, f2 = U((b, 32, h, w), 301).to(DEV), U((b, 32, h, w), 302).to(DEV)
    corr = ops.corr_build_pyramid(f1, f2, L)
    geo = ops.geo_pyramid(U((b, g, d, h, w), 303).to(DEV), L) if g else None
    disp = U((b, 1, h, w), 304, -6.0, w + 6.0).to(DEV)
    disp[:, :, 0, :4] = torch.tensor([0.0, 1.5, 3.0, float(w - 1)], device=DEV)
    cin = L * 9 * (g + 1)
    wt = (U((64, cin, 1, 1), 305) * (3.0 / cin) ** 0.5).to(DEV)
    bias = (U((64,), 306) * 0.1).to(DEV)
    pack = ops.LookupConvPack().get(wt, bias)
    bs = ops.BS8.empty(b, 64, h, w, DEV)
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        out = ops.lookup_convc1(geo, corr, disp, 4, pack, out_bs=bs, want_f32=True)
        lk = ops.geo_corr_lookup(geo, corr, disp, 4)
    finally:
        ops.set_precision(prev)
    want = torch.relu(torch.einsum("oc,bchw->bohw", wt[:, :, 0, 0].double(), lk.double()) + bias.double().view(1, -1, 1, 1))
    close(out, want, 2e-5, 2e-5, "fused lookup + convc1")
    assert (bs.float() - out).abs().max().item() <= 2e-6 * max(1.0, out.abs().max().item()), "blocked split-fp16 copy"
    geo64 = [t.permute(0, 1, 2, 4, 3).double().cpu() for t in geo] if g else None
    ref = O.geo_corr_lookup(geo64, [t.double().cpu() for t in corr], disp.double().cpu(), 4)
    want2 = torch.relu(torch.einsum("oc,bchw->bohw", wt[:, :, 0, 0].double().cpu(), ref) + bias.double().cpu().view(1, -1, 1, 1))
    close(out, want2, 3e-5, 3e-5, "fused lookup + convc1 vs the oracle's lookup")


def test_split_mode_range_guard():
    """Split precision represents an operand as fp16 hi + lo: |x| >= 65504 has no such form.  The kernels SATURATE such
    operands (MODE.FP16_OVFL / round-toward-zero conversions: finite results, never inf / NaN) and count the waves that met
    one (ops.split_overflow_count); exact-fp32 mode computes them correctly.  Activations of scale 1e5 through a conv, the
    blocked split-fp16 link tensor, the all-pairs correlation and the fused lookup conv, in both modes."""
    import torch.nn.functional as F
    from anystereo import ops
    prev = ops.get_precision()
    x = (U((1, 32, 12, 20), 401) * 2e5).to(DEV)           # |x| up to 2e5 > 65504
    xs = (U((1, 32, 12, 20), 401) * 2.0).to(DEV)            # the same pattern in range
    w = (U((64, 32, 3, 3), 402) * 0.05).to(DEV)
    ref = F.conv2d(x.double(), w.double(), padding=1)
    try:
        ops.set_precision("fp32")
        pk = ops.PackedConv().get([w], [None])
        close(ops.conv2d([x], pk), ref, 2e-5, 1e-3, "fp32 mode, 1e5-scale activations")
        ops.set_precision("split")
        ops.split_overflow_count()                            # reset
        pk = ops.PackedConv().get([w], [None])
        y = ops.conv2d([xs], pk)
        close(y, F.conv2d(xs.double(), w.double(), padding=1), 2e-5, 2e-5, "split mode, in range")
        assert ops.split_overflow_count() == 0, "in-range operands must not be counted"
        bs = ops.BS8.empty(1, 64, 12, 20, DEV)
        y = ops.conv2d([x], pk, out_bs=bs)                   # fp32 source (loader split) + blocked result (epilogue split)
        assert torch.isfinite(y).all() and torch.isfinite(bs.t.float()).all(), "saturation must keep everything finite"
        assert ops.split_overflow_count() > 0, "out-of-range operands must be counted"
        big = ops.BS8.empty(1, 32, 12, 20, DEV)
        ops.conv2d([x], ops.PackedConv().get([torch.eye(32, device=DEV).view(32, 32, 1, 1).contiguous()], [None]), out_bs=big)
        assert big.float().abs().max().item() <= 65504.0 * (1 + 2.0 ** -10) and torch.isfinite(big.t.float()).all()
        ops.split_overflow_count()
        f1 = (U((1, 96, 4, 40), 403) * 1e5).to(DEV)
        lv = ops.corr_build_pyramid(f1, f1, 2)
        assert all(torch.isfinite(t).all() for t in lv) and ops.split_overflow_count() > 0
        # fused lookup + convc1: a 1e6-scale correlation volume saturates in the tile split, finite output
        corr = [t * 0 + 3e6 for t in ops.corr_build_pyramid(xs[:, :, :4].contiguous(), xs[:, :, :4].contiguous(), 4)]
        wt = (U((64, 36, 1, 1), 404) * 0.1).to(DEV)
        out = ops.lookup_convc1(None, corr, torch.zeros(1, 1, 4, 20, device=DEV), 4, ops.LookupConvPack().get(wt, None), want_f32=True)
        assert torch.isfinite(out).all() and ops.split_overflow_count() > 0
        ops.set_precision("fp32")
        lv32 = ops.corr_build_pyramid(f1, f1, 1)
        close(lv32[0], O.all_pairs_corr(f1.double().cpu(), f1.double().cpu()), 2e-5, 1.0, "fp32 mode all-pairs at 1e5 scale")
    finally:
        ops.set_precision(prev)
        ops.split_overflow_count()


def test_lookup_rejects_foreign_coords():
    """`coords` is part of the reference signature (geometry.py:34) but the kernels regenerate the pixel-column grid: the
    model's own grid and an equal caller-made grid are accepted, anything else raises instead of being ignored."""
    from anystereo.nn.geometry import Combined_Geo_Encoding_Volume
    b, h, w = 1, 4, 24
    f1, f2 = U((b, 32, h, w), 501).to(DEV), U((b, 32, h, w), 502).to(DEV)
    gev = U((b, 8, 48, h, w), 503).to(DEV)
    fn = Combined_Geo_Encoding_Volume(f1, f2, gev, num_levels=2, radius=4)
    disp = U((b, 1, h, w), 504, 0.0, 10.0).to(DEV)
    good = torch.arange(w, device=DEV).float().view(1, 1, w, 1).repeat(b, h, 1, 1)
    ref = fn(disp, good)
    assert torch.equal(fn(disp, None), ref)
    bad = good + 0.5
    with pytest.raises(RuntimeError, match="arange"):
        fn(disp, bad)
    with pytest.raises(RuntimeError, match="coords must be"):
        fn(disp, good[:, :, :-1])


def test_reduced_precision_mode(golden):
    """`args.mixed_precision` in inference = the one-MFMA mode of the convolution kernels (fp16 operands, fp32 accumulate;
    the counterpart of the reference's autocast path, continuous_IGEVstereo.py:287, evaluation.py:558).  It is a SECOND mode
    with its own tolerance — against the reference's fp32 output: a single conv within 2e-3 relative (fp16 operand rounding
    2^-11 over a K = 1152 dot product), the whole model within 5e-2 px EPE — and it must really differ from the
    parity mode (whose bar stays 1e-3)."""
    import torch.nn.functional as F
    from anystereo import ops
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        x = U((1, 128, 20, 36), 601, -2, 2).to(DEV)
        w = (U((64, 128, 3, 3), 602) * (3.0 / 1152) ** 0.5).to(DEV)
        ref = F.conv2d(x.double(), w.double(), padding=1)
        pk = ops.PackedConv().get([w], [None])
        exact = ops.conv2d([x], pk)
        with ops.fast_fp16(True):
            fast = ops.conv2d([x], pk)
        assert not ops.get_fast_fp16()
        e_exact = (exact.double() - ref).abs().max().item() / ref.abs().max().item()
        e_fast = (fast.double() - ref).abs().max().item() / ref.abs().max().item()
        assert e_exact < 2e-6 and 1e-5 < e_fast < 2e-3, (e_exact, e_fast)
        g = golden("model_igev")
        H, W = int(g["H"]), int(g["W"])
        img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
        outs = {}
        for mp in (False, True):
            model = __models__["continuous_IGEVStereo"](default_args("continuous_IGEVStereo", mixed_precision=mp)).eval()
            fill_module_deterministic(model, base_seed=1)
            model = model.to(DEV)
            coord = O.make_coord([round(H * 1.5), round(W * 1.5)]).view(1, -1, 2).to(DEV)
            with torch.no_grad():
                outs[mp] = model(img1.to(DEV), img2.to(DEV), iters=3, test_mode=True, hr_coord=coord, scale=torch.tensor([[1.5]], device=DEV))
            assert not ops.get_fast_fp16(), "the mode must not leak out of forward()"
        key = [k for k in g if "test" in k and "1p5" in k]
        d = (outs[True] - outs[False]).abs().mean().item()
        print(f"reduced precision vs parity mode: mean |d| = {d:.3e} px; conv rel err {e_fast:.2e}")
        assert torch.isfinite(outs[True]).all() and 1e-7 < d < 5e-2, d
    finally:
        ops.set_fast_fp16(False)
        ops.set_precision(prev)


@pytest.mark.parametrize("tag,h,w", [("igev", 8, 12), ("igev", 23, 37), ("raft", 9, 21)])
def test_loop_front_fused_equals_staged(golden, tag, h, w):
    """The front of a GRU iteration as ONE launch (disp += delta from the head's tap planes, lookup + convc1, 7x7 conv of the
    disparity branch; as_loop_front_fwd) against the staged launches it replaces (as_tap_shift_sum -> as_lookup_convc1_fwd ->
    as_conv7x7_c1_relu): the new disparity is bit-identical and the motion features agree — bit for bit for the RAFT geometry;
    for IGEV the staged path's lookup + convc1 is the register-direct kernel, whose K order differs from the fused front's
    LDS-tile form (fp32 rounding of a permuted sum) — for both model geometries and map sizes that do not fill the blocks."""
    from anystereo import ops
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models.base import default_args
    from anystereo.nn.geometry import Combined_Geo_Encoding_Volume, CorrBlock1D
    from anystereo.nn.update import BasicMultiUpdateBlock
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        args = default_args("continuous_IGEVStereo" if tag == "igev" else "continuous_RAFTStereo")
        ub = BasicMultiUpdateBlock(args, hidden_dims=args.hidden_dims, geo_channels=8 if tag == "igev" else 0).eval()
        fill_module_deterministic(ub, base_seed=5)
        ub = ub.to(DEV)
        b = 2
        f1, f2 = U((b, 32, h, w), 701).to(DEV), U((b, 32, h, w), 702).to(DEV)
        if tag == "igev":
            fn = Combined_Geo_Encoding_Volume(f1, f2, U((b, 8, 48, h, w), 703).to(DEV), num_levels=2, radius=4)
        else:
            fn = CorrBlock1D(f1, f2, num_levels=4, radius=4)
        net0 = torch.tanh(U((b, 128, h, w), 704, -2, 2)).to(DEV)
        disp = U((b, 1, h, w), 705, 0.0, float(w)).to(DEV)
        with torch.no_grad():
            assert ub.encoder.fused_lookup_ok(fn) and ub.disp_head.taps_ok(net0)
            taps = ub.disp_head.taps(net0)
            d_ref = ub.disp_head.finish(taps, addend=disp)
            mf_ref = ub.encoder.forward_fused_lookup(d_ref, fn)
            d_full = ub.disp_head(net0, addend=disp)
            for mode in ("lite", "full"):  # lite: finish + lookup + convc1 in one launch, 7x7 staged; full: all three in one grid
                ub.encoder.fused_front = mode
                mf, d_new = ub.encoder.forward_front(taps, ub.disp_head, disp, fn)
                assert torch.equal(d_new, d_ref) and torch.equal(d_full, d_ref), f"new disparity ({mode})"
                if tag == "raft":
                    assert torch.equal(mf.t, mf_ref.t), f"motion features (blocked split-fp16, {mode})"
                else:
                    close(mf.float(), mf_ref.float(), 2e-5, 2e-6, f"motion features ({mode})")
                assert (mf.float()[:, 127:128] - d_ref).abs().max().item() <= 2e-6 * max(1.0, d_ref.abs().max().item()), "disparity pass-through"
    finally:
        ops.set_precision(prev)

@pytest.mark.parametrize("b,c,h,w,stride", [(2, 32, 20, 40, 1), (1, 144, 13, 37, 2), (3, 16, 9, 14, 2), (2, 96, 10, 20, 1), (1, 8, 3, 5, 1),
                                            (4, 32, 80, 160, 1)])
def test_dwconv3x3_backward(b, c, h, w, stride):
    """Depthwise 3x3 under autograd (grad.DwConv3x3: MobileNetV2's conv_dw layers in training, extractor.py:331-342): forward, data
    gradient (stride 1: the forward kernel on flipped taps; stride 2: the gather kernel) and weight gradient (two-stage fixed-order
    reduction) against the fp64 grouped convolution; odd sizes, both strides, a multi-slice reduction.  The weight gradient is
    the same bits on every run."""
    import torch.nn.functional as F
    from anystereo import grad as G
    x = U((b, c, h, w), 700 + c).to(DEV).requires_grad_(True)
    wt = (U((c, 1, 3, 3), 701 + c) * 0.3).to(DEV).requires_grad_(True)
    gout = U((b, c, (h - 1) // stride + 1, (w - 1) // stride + 1), 702 + c).to(DEV)
    y = G.DwConv3x3.apply(x, wt, stride)
    y.backward(gout)
    xd, wd = x.detach().double().requires_grad_(True), wt.detach().double().requires_grad_(True)
    yd = F.conv2d(xd, wd, None, stride, 1, 1, c)
    yd.backward(gout.double())
    for got, want, what in ((y, yd, "forward"), (x.grad, xd.grad, "d_x"), (wt.grad, wd.grad, "d_weight")):
        err = (got.double() - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
        assert err < 2e-6, f"dwconv3x3 {what}: max err / max |ref| = {err:.2e}"
    g1 = wt.grad.clone()
    wt.grad = None
    x.grad = None
    G.DwConv3x3.apply(x, wt, stride).backward(gout)
    assert torch.equal(wt.grad, g1), "dwconv3x3 weight gradient is not bit-repeatable"

@pytest.mark.parametrize("cin,cout,ks,bias", [(64, 64, 3, True), (32, 96, 1, False)])
@pytest.mark.parametrize("mean_scale", [1.0, 30.0])
def test_conv_frozen_bn_backward(cin, cout, ks, bias, mean_scale):
    """relu(bn(conv(x))) with a FROZEN BatchNorm2d under autograd (grad.conv_frozen_bn: the context network's residual blocks in the
    training step, extractor.py:10-62 with train_continuous_IGEV.py:189): the affine map folded into the convolution's weights by
    differentiable weight-sized operations — output and the gradients of x, W, bias, gamma, beta against the fp64 modules."""
    import torch.nn as nn
    from anystereo import grad as G
    from anystereo import ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        b, h, w = 2, 128, 128   # 2 * cout * 128 * 128 >= 2^21 output elements: the folded branch
        conv = nn.Conv2d(cin, cout, ks, padding=ks // 2, bias=bias).to(DEV)
        bn = nn.BatchNorm2d(cout).to(DEV).eval()
        with torch.no_grad():
            conv.weight.copy_((U(tuple(conv.weight.shape), 810 + ks) * 0.1).to(DEV))
            if bias:
                conv.bias.copy_(U((cout,), 811).to(DEV))
            bn.weight.copy_(U((cout,), 812, 0.5, 1.5).to(DEV)), bn.bias.copy_(U((cout,), 813).to(DEV))
            # mean_scale 30: |running_mean| / std up to ~40 — the regime in which the fold's gamma gradient,
            # rs * (sum(dW' * W) - mean * sum(dy)), is a difference of two activation-sized sums |mean| / std times larger than
            # itself (advisor, round 5): its error grows by that ratio over the ~5e-6 of the weight-gradient kernel
            bn.running_mean.copy_((U((cout,), 814) * mean_scale).to(DEV)), bn.running_var.copy_(U((cout,), 815, 0.5, 2.0).to(DEV))
        holder = nn.Module()
        x = U((b, cin, h, w), 816).to(DEV).requires_grad_(True)
        gout = U((b, cout, h, w), 817).to(DEV)
        G.begin_forward()
        y = G.conv_frozen_bn(holder, "t", conv, bn, x, relu=True)
        assert "_frozen_bn_consts" in holder.__dict__, "the folded branch was not taken"
        y.backward(gout)
        got = {"y": y, "d_x": x.grad, "d_w": conv.weight.grad, "d_gamma": bn.weight.grad, "d_beta": bn.bias.grad}
        if bias:
            got["d_bias"] = conv.bias.grad
        import copy
        convd, bnd = copy.deepcopy(conv).double(), copy.deepcopy(bn).double().eval()
        for p_ in list(convd.parameters()) + list(bnd.parameters()):
            p_.grad = None
        xd = x.detach().double().requires_grad_(True)
        yd = torch.relu(bnd(convd(xd)))
        yd.backward(gout.double())
        want = {"y": yd, "d_x": xd.grad, "d_w": convd.weight.grad, "d_gamma": bnd.weight.grad, "d_beta": bnd.bias.grad}
        if bias:
            want["d_bias"] = convd.bias.grad
        for k_, tol in (("y", 5e-6), ("d_x", 1e-5), ("d_w", 1e-4), ("d_gamma", 1e-4 * max(1.0, mean_scale / 3.0)), ("d_beta", 1e-4), ("d_bias", 1e-4)):
            if k_ not in got:
                continue
            err = (got[k_].double() - want[k_]).abs().max().item() / max(want[k_].abs().max().item(), 1e-30)
            print(f"[conv_frozen_bn {cin}->{cout} k{ks} mean x{mean_scale:g}] {k_}: {err:.2e} (limit {tol:g})")
            assert err < tol, f"conv_frozen_bn {k_}: max err / max |ref| = {err:.2e} (limit {tol:g})"
    finally:
        ops.set_precision(prev)

@pytest.mark.parametrize("cout,cin,ks", [(64, 48, 3), (100, 37, 3), (9, 64, 1), (256, 384, 3)])
def test_dgrad_pack_equals_transposed_flipped_copy(cout, cin, ks):
    """PackedConv.get_dgrad (as_conv_pack_weights_split_t: the data-gradient convolution's pack read straight from the forward weight)
    is bit for bit the pack of `weight.transpose(0, 1).flip(2, 3)`; ragged channel counts, 1x1 and 3x3, a Linear's 2-D weight."""
    from anystereo import ops
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        w = (U((cout, cin, ks, ks), 900 + cout) * 0.2).to(DEV)
        a = ops.PackedConv().get_dgrad(w)
        b = ops.PackedConv().get([w], [None], transform=lambda t: t.transpose(0, 1).flip(2, 3).contiguous())
        assert (a.cin, a.cout, a.ks) == (b.cin, b.cout, b.ks) == (cout, cin, ks) and a.bias is None
        assert torch.equal(a.wpack, b.wpack)
        if ks == 1:
            a2 = ops.PackedConv().get_dgrad(w.view(cout, cin))
            assert torch.equal(a2.wpack, b.wpack)
    finally:
        ops.set_precision(prev)


# name, precision, (B, H, W, Cin, Cout), conv2d form, the instantiation the default knobs select: family (1 = conv_split_kernel),
# KS, TW, BN, kernel epilogue (3 = K-split partial sums), NSUB, S, FAST, LEAN.  Each shape is the smallest that selects its
# instantiation: Cin 16 is a single K chunk, which keeps a small map from splitting K.
_DISPATCH_CASES = [
    ("tw16_bn64", "split", (1, 9, 14, 16, 64), {}, (1, 3, 16, 64, 0, 1, 1, 0, 0)),
    ("tw32_bn64", "split", (1, 4, 60, 16, 64), {}, (1, 3, 32, 64, 0, 1, 1, 0, 0)),
    # 255 blocks of 128 channels: no room for a K split, and two rounds of wide blocks
    ("tw16_bn128", "split", (17, 8, 80, 32, 384), {}, (1, 3, 16, 128, 0, 1, 1, 0, 0)),
    ("tw32_bn128", "split", (17, 4, 160, 32, 384), {}, (1, 3, 32, 128, 0, 1, 1, 0, 0)),
    ("wide", "split", (1, 16, 17, 16, 128), {}, (1, 3, 16, 64, 0, 2, 1, 0, 0)),
    ("lean", "split", (1, 136, 240, 16, 256), {"blocked": True}, (1, 3, 16, 64, 0, 2, 1, 0, 1)),
    ("ksplit", "split", (1, 17, 30, 128, 128), {}, (1, 3, 32, 128, 3, 1, 1, 0, 0)),
    ("stride2", "split", (1, 9, 35, 16, 32), {"stride": 2}, (1, 3, 16, 64, 0, 1, 2, 0, 0)),
    ("1x1_bn64", "split", (1, 3, 50, 36, 64), {"ks": 1}, (1, 1, 128, 64, 0, 1, 1, 0, 0)),
    ("1x1_bn128", "split", (1, 1, 300, 32, 128), {"ks": 1}, (1, 1, 128, 128, 0, 1, 1, 0, 0)),
    ("relu_taps", "split", (1, 24, 40, 16, 64), {"taps": True}, (1, 3, 16, 64, 4, 1, 1, 0, 0)),
    ("dual_fused", "split", (1, 9, 14, 16, 64), {"dual": 1}, (1, 3, 16, 64, 0, 1, 1, 0, 0)),
    ("dual_sequential", "split", (1, 9, 14, 64, 64), {"dual": 2}, (1, 3, 16, 64, 3, 1, 1, 0, 0)),
    ("fp32_tw8", "fp32", (1, 9, 8, 20, 40), {}, (0, 3, 8, 64, 0, 1, 1, 0, 0)),
    ("fp32_tw16", "fp32", (1, 5, 16, 20, 40), {}, (0, 3, 16, 64, 0, 1, 1, 0, 0)),
    ("fp32_tw32", "fp32", (1, 2, 33, 20, 40), {}, (0, 3, 32, 64, 0, 1, 1, 0, 0)),
]


from _conv_cases import planned_kernels as _planned_kernels  # noqa: E402  (shared with test_conv_instantiations_gpu.py)


def test_conv_dispatch_runs_the_planned_kernel():
    """as_conv2d launches what its planner (csrc/conv_plan.h) says, under the default knobs, for a shape per
    instantiation family: ops.conv_plan names the expected instantiation; the kernels as_conv2d really launches — their names and
    order, read from the profiler's kernel trace — are the plan's, K-split finish launches and the two calls of an unfused dual
    launch included; and the result of ops.conv2d is the fp64 convolution's (+ the epilogue in torch) within the conv parity tests'
    1e-5 (RELU_TAPS: 2e-5, through tap_shift_sum, as test_conv_relu_taps_epilogue)."""
    import re

    from torch.profiler import ProfilerActivity, profile

    from anystereo import _lib as Lb, ops
    prev = ops.get_precision()
    tuple_of = ("family", "KS", "TW", "BN", "epilogue", "NSUB", "S", "FAST", "LEAN")
    expected = []
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for name, prec, (b, h, w, cin, cout), form, want in _DISPATCH_CASES:
                ops.set_precision(prec)
                ks, stride, dual = form.get("ks", 3), form.get("stride", 1), form.get("dual", 0)
                plan = ops.conv_plan(dict(B=b, H=h, W=w, Cin=cin, Cout=cout, KS=ks, precision=int(prec == "split"), stride=stride, dual=dual,
                                          blocked=form.get("blocked"), epilogue=Lb.EPI_RELU_TAPS if form.get("taps") else Lb.EPI_LINEAR,
                                          act=Lb.ACT_RELU))
                assert tuple(plan[f] for f in tuple_of) == want and plan["dual"] == dual, (name, plan)
                assert (plan["ksplit"] > 1) == (want[4] == 3) == bool(plan["finish"]), (name, plan)
                expected += [(name, k) for k in _planned_kernels(plan)]
                x = U((b, cin, h, w), 700, -2, 2)
                wt, bias = U((cout, cin, ks, ks), 701) * (3.0 / (cin * ks * ks)) ** 0.5, U((cout,), 702) * 0.1
                pk = ops.PackedConv().get([wt.to(DEV)], [bias.to(DEV)])
                ref = torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=ks // 2).relu()
                src = x.to(DEV)
                if form.get("blocked"):
                    hi = src.half()
                    lo = ((src - hi.float()) * 2048.0).half()
                    src = ops.BS8(torch.stack([hi, lo], 1).view(b, 2, cin // 8, 8, h, w).permute(0, 1, 2, 4, 5, 3).contiguous(), cin)
                if form.get("taps"):
                    w2, b2 = U((1, cout, 3, 3), 703) * 0.05, U((1,), 704)
                    taps = ops.conv2d([src], pk, act=Lb.ACT_RELU, epilogue=Lb.EPI_RELU_TAPS, tap_w=w2[0].reshape(cout, 9).contiguous().to(DEV))
                    close(ops.tap_shift_sum(taps, b2.to(DEV)), _ref_conv(ref, w2, b2, 1), 2e-5, 2e-5, name)
                elif dual:
                    x2, wt2 = U((b, cin, h, w), 705, -2, 2), U((cout, cin, ks, ks), 706) * (3.0 / (cin * ks * ks)) ** 0.5
                    pk2 = ops.PackedConv().get([wt2.to(DEV)], [None])
                    out = torch.empty((b, 2 * cout, h, w), device=DEV)
                    ops.conv2d([src], pk, act=Lb.ACT_RELU, out=out, dual={"src": x2.to(DEV), "pack": pk2, "out_coff": cout})
                    close(out[:, :cout], ref, 1e-5, 1e-5, name)
                    close(out[:, cout:], _ref_conv(x2, wt2, None, ks // 2).relu(), 1e-5, 1e-5, name + " (second)")
                else:
                    close(ops.conv2d([src], pk, act=Lb.ACT_RELU, stride=stride), ref, 1e-5, 1e-5, name)
            torch.cuda.synchronize()
    finally:
        ops.set_precision(prev)
    launched = sorted((e.time_range.start, m.group(0)) for e in prof.events()
                      for m in [re.search(r"conv_(split|igemm|finish)_kernel<[^>]*>", e.name)] if m)
    assert [k for _, k in launched] == [k for _, k in expected], list(zip(expected, [k for _, k in launched]))


def test_conv_dual_as_two_calls_runs_each_half_s_plan():
    """A dual launch that cannot be fused — fp32 precision, or split precision on a map small enough that K splits — runs as two
    calls, each validated and planned for itself inside as_conv2d.  B 1, 3x3, 20 x 24 (4x32 tiles, partial along both axes): both
    results are the fp64 convolutions' within the neighbouring tests' 1e-5, and the launched kernels are those of the two halves'
    own plans, finish launches included.  In the 128 -> 128 case the halves plan differently: the first source is blocked
    (64-channel tiles, all-DMA staging), the second is fp32 (128-channel tiles)."""
    from torch.profiler import ProfilerActivity, profile

    from _conv_cases import launched_kernels, to_bs

    from anystereo import _lib as Lb, ops
    prev = ops.get_precision()
    b, h, w, expected = 1, 20, 24, []
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for name, prec, c, blocked in (("fp32", "fp32", 64, False), ("split", "split", 64, True), ("split_128", "split", 128, True)):
                ops.set_precision(prec)
                halves = [ops.conv_plan(dict(B=b, H=h, W=w, Cin=c, Cout=c, precision=int(prec == "split"), blocked=bl, act=Lb.ACT_RELU))
                          for bl in (blocked, False)]
                assert all((p["ksplit"] > 1) == (prec == "split") and p["dual"] == 0 for p in halves), (name, halves)
                assert (name == "split_128") == (_planned_kernels(halves[0]) != _planned_kernels(halves[1])), (name, halves)
                expected += [(name, k) for p in halves for k in _planned_kernels(p)]
                x, x2 = U((b, c, h, w), 710, -2, 2), U((b, c, h, w), 711, -2, 2)
                wt, wt2 = (U((c, c, 3, 3), 712 + i) * (3.0 / (c * 9)) ** 0.5 for i in range(2))
                bias, bias2 = U((c,), 714) * 0.1, U((c,), 715) * 0.1
                pk, pk2 = (ops.PackedConv().get([t.to(DEV)], [bb.to(DEV)]) for t, bb in ((wt, bias), (wt2, bias2)))
                out = torch.full((b, 2 * c, h, w), float("nan"), device=DEV)
                src = to_bs(x.to(DEV)) if blocked else x.to(DEV)
                ops.conv2d([src], pk, act=Lb.ACT_RELU, out=out, dual={"src": x2.to(DEV), "pack": pk2, "out_coff": c})
                close(out[:, :c], _ref_conv(x, wt, bias, 1).relu(), 1e-5, 1e-5, name)
                close(out[:, c:], _ref_conv(x2, wt2, bias2, 1).relu(), 1e-5, 1e-5, name + " (second)")
            torch.cuda.synchronize()
    finally:
        ops.set_precision(prev)
    launched = launched_kernels(prof)
    assert launched == [k for _, k in expected] and len(launched) == 2 + 4 + 4, list(zip(expected, launched))


KNOB_SETS = [
    {"AS_CONV_LEAN": "0", "AS_CONV_XCD": "0", "AS_CONV_DMA": "0", "AS_POOL2X_EVEN": "0", "AS_LOOKUP_DIRECT": "0"},
    {"AS_CONV_XCD": "1", "AS_CONV_LEAN": "3", "AS_CONV_KSPLIT_MAX": "1", "AS_CONV_WIDE": "0", "AS_CONV_WIDE64": "0", "AS_CONV_SMALL_DMA": "0", "AS_LOOKUP_DIRECT": "2"},
    {"AS_CONV_LEAN": "2", "AS_CONV_PREFER64": "1", "AS_CONV_XCD_STAGGER": "4", "AS_CONV_LEAN_OFFSET": "8", "AS_CONV_KSPLIT_MAX": "2"},
]


def test_schedule_knobs_keep_results(tmp_path):
    """The AS_* environment knobs of csrc/conv.hip / lookup.hip (README: A/B switches of the kernel schedule — block shape, lean
    blocks, XCD order and stagger, K split, staging path, resampler form) select HOW a launch is tiled, never WHAT it computes.  They
    are read once per process, so each set runs tests/_knob_probe.py (the loop's launches at the cfg-2 sizes + two training-shaped
    layers) in a child process; every result must agree with the default schedule's: bit for bit where the summation order is the
    same, within 2e-6 of the tensor's range where a K split changes the order of the partial sums."""
    import subprocess
    import sys

    import numpy as np
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_knob_probe.py")
    base_env = {k: v for k, v in os.environ.items() if not k.startswith(("AS_CONV_", "AS_POOL2X", "AS_LOOKUP_"))}
    outs = []
    for i, knobs in enumerate([{}] + KNOB_SETS):
        path = str(tmp_path / f"knobs{i}.npz")
        r = subprocess.run([sys.executable, probe, path], env=dict(base_env, **knobs), capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, f"knob set {knobs}: child failed\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
        outs.append(dict(np.load(path)))
    ref = outs[0]
    assert len(ref) >= 20
    for knobs, got in zip(KNOB_SETS, outs[1:]):
        assert got.keys() == ref.keys()
        exact = 0
        for k, a in ref.items():
            assert np.isfinite(got[k]).all(), (knobs, k)
            d = float(np.abs(got[k] - a).max())
            exact += d == 0.0
            assert d <= 2e-6 * float(np.abs(a).max()) + 1e-9, f"{knobs}: {k} differs from the default schedule by {d:.3e} (range {np.abs(a).max():.3e})"
        print(f"[knobs] {knobs}: {exact}/{len(ref)} results bit-identical to the default schedule")
