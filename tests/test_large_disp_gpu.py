"""GPU (-m gpu): the kernels behind the geometry volume above D = 48, as far as they run today.

The lookups, the fused lookup + convc1, the loop front and the backward kernels of the geometry pyramid, the lookup and the
disparity regression are generic in D by reading (`Dl = D >> level`) and had never been run above D = 48.  Here they run at
D = 96, 128 and 192 (max_disp 384 / 768) against the fp64 oracle (oracle/ops.py is generic in D and W), with the tolerances the
tests of the same kernels use at D = 48 (tests/test_hip_parity.py).  Disparities are drawn from [-6, D + 6] with planted values
around the old range's end and the new one's.  Where a case needs a pyramid of D = 192 it is built by the oracle, and the backward
of the gwc volume and of the pyramid are launched through their Functions' own backward without the forward: as_geo_pyramid
holds its whole [G*D][33] tile in LDS (G*D <= 1240) and as_gwc_volume_fwd serves D <= 64, so the whole model above
max_disp = 256 is not covered here.
"""
import pytest
import torch

from oracle import ops as O
from test_hip_parity import U, _leaf, close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _planted_disp(b, h, w, d, seed):
    disp = U((b, 1, h, w), seed, -6.0, d + 6.0)
    disp.view(-1)[:5] = torch.tensor([63.5, 64.0, float(d - 1), d - 0.5, float(d + 3)])
    return disp


def _oracle_geo_levels(gev, L):
    """The geometry pyramid of gev [B,G,D,H,W] in the device layout [B,H,W,D>>i,G], built by the oracle (any D)."""
    return [t.permute(0, 1, 2, 4, 3).contiguous().float().to(DEV) for t in O.geo_pyramid(gev, L)]


@pytest.mark.parametrize("d", [96, 192])
def test_lookup_large_d(d):
    from anystereo import ops
    b, h, w, g, L, r = 1, 3, 37, 8, 2, 4
    corr = [U((b, h, w, w >> i), 30 + i, -3, 3) for i in range(L)]
    geo = [U((b, h, w, g, d >> i), 40 + i, -3, 3) for i in range(L)]
    disp = _planted_disp(b, h, w, d, 50)
    out = ops.geo_corr_lookup([t.permute(0, 1, 2, 4, 3).contiguous().to(DEV) for t in geo], [t.to(DEV) for t in corr], disp.to(DEV), r)
    ref = O.geo_corr_lookup([t.double() for t in geo], [t.double() for t in corr], disp.double(), r)
    close(out, ref, rtol=2e-5, atol=2e-5, what="lookup")


@pytest.mark.parametrize("d", [96, 192])
def test_lookup_convc1_fused_large_d(d):
    """lookup -> convc1 -> ReLU as one kernel on a pyramid of D = 96 / 192, as test_lookup_convc1_fused does it at D = 48:
    against the staged lookup + fp64 1x1 convolution and against the oracle's lookup."""
    from anystereo import ops
    b, h, w, g, L = 1, 5, 70, 8, 2
    f1, f2 = U((b, 32, h, w), 301).to(DEV), U((b, 32, h, w), 302).to(DEV)
    corr = ops.corr_build_pyramid(f1, f2, L)
    geo = _oracle_geo_levels(U((b, g, d, h, w), 303), L)
    disp = _planted_disp(b, h, w, d, 304).to(DEV)
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
    geo64 = [t.permute(0, 1, 2, 4, 3).double().cpu() for t in geo]
    ref = O.geo_corr_lookup(geo64, [t.double().cpu() for t in corr], disp.double().cpu(), 4)
    want2 = torch.relu(torch.einsum("oc,bchw->bohw", wt[:, :, 0, 0].double().cpu(), ref) + bias.double().cpu().view(1, -1, 1, 1))
    close(out, want2, 3e-5, 3e-5, "fused lookup + convc1 vs the oracle's lookup")


def test_loop_front_large_d():
    """The front of a GRU iteration as one launch against its staged form on a geometry volume of D = 128 (max_disp 512: the
    largest of the ranges the reference runs whose pyramid as_geo_pyramid builds, G*D = 1024 <= 1240), as
    test_loop_front_fused_equals_staged holds it at D = 48: the new disparity bit-identical, the motion features to 2e-5."""
    from anystereo import ops
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models.base import default_args
    from anystereo.nn.geometry import Combined_Geo_Encoding_Volume
    from anystereo.nn.update import BasicMultiUpdateBlock
    d = 128
    prev = ops.get_precision()
    ops.set_precision("split")
    try:
        args = default_args("continuous_IGEVStereo", max_disp=4 * d)
        ub = BasicMultiUpdateBlock(args, hidden_dims=args.hidden_dims, geo_channels=8).eval()
        fill_module_deterministic(ub, base_seed=5)
        ub = ub.to(DEV)
        b, h, w = 2, 23, 37
        f1, f2 = U((b, 32, h, w), 701).to(DEV), U((b, 32, h, w), 702).to(DEV)
        fn = Combined_Geo_Encoding_Volume(f1, f2, U((b, 8, d, h, w), 703).to(DEV), num_levels=2, radius=4)
        net0 = torch.tanh(U((b, 128, h, w), 704, -2, 2)).to(DEV)
        disp = _planted_disp(b, h, w, d, 705).to(DEV)
        with torch.no_grad():
            assert ub.encoder.fused_lookup_ok(fn) and ub.disp_head.taps_ok(net0)
            taps = ub.disp_head.taps(net0)
            d_ref = ub.disp_head.finish(taps, addend=disp)
            mf_ref = ub.encoder.forward_fused_lookup(d_ref, fn)
            for mode in ("lite", "full"):
                ub.encoder.fused_front = mode
                mf, d_new = ub.encoder.forward_front(taps, ub.disp_head, disp, fn)
                assert torch.equal(d_new, d_ref), f"new disparity ({mode})"
                close(mf.float(), mf_ref.float(), 2e-5, 2e-6, f"motion features ({mode})")
    finally:
        ops.set_precision(prev)


# ---------------------------------------------------------------------------------------------
# backward kernels against fp64 autograd of the oracle
# ---------------------------------------------------------------------------------------------

class _Ctx:
    """Stands in for the autograd context of a grad.py Function whose forward kernel does not serve the shape yet: the Function's
    own backward (its launch of the backward kernel) runs on what the forward would have saved."""

    def __init__(self, saved=(), **attrs):
        self.saved_tensors = tuple(saved)
        self.__dict__.update(attrs)


def test_gwc_backward_large_d():
    """G.GwcVolume's backward (as_gwc_volume_bwd) at D = 96 against fp64 autograd of the oracle's volume.  The forward kernel
    stops at D = 64, and the backward needs only fl, fr and d_vol."""
    from anystereo import grad as G
    b, c, h, w, D, G_ = 1, 96, 2, 70, 96, 8
    fl, fr = U((b, c, h, w), 430), U((b, c, h, w), 431)
    gv = U((b, G_, D, h, w), 432)
    dfl, dfr, _, _ = G.GwcVolume.backward(_Ctx((fl.to(DEV), fr.to(DEV)), maxdisp=D, groups=G_), gv.to(DEV))
    r1, r2 = _leaf(fl, dt=torch.float64), _leaf(fr, dt=torch.float64)
    O.gwc_volume(r1, r2, D, G_).backward(gv.double())
    close(dfl, r1.grad, 2e-5, 1e-6, "d fl")
    close(dfr, r2.grad, 2e-5, 1e-6, "d fr")


def test_geo_pyramid_backward_large_d():
    """G.GeoPyramid's backward (as_geo_pyramid_bwd) at the max_disp = 768 form, D = 192: it needs only the level gradients, not
    the forward, whose tile stops at G*D = 1240."""
    from anystereo import grad as G
    b, g, d, h, w, L = 1, 8, 192, 2, 37, 2
    gev = U((b, g, d, h, w), 420)
    gs = [U((b, h, w, d >> i, g), 421 + i) for i in range(L)]
    d_gev, _ = G.GeoPyramid.backward(_Ctx(shape=(b, g, d, h, w)), *[t.to(DEV) for t in gs])
    r = _leaf(gev, dt=torch.float64)
    torch.autograd.backward(O.geo_pyramid(r, L), [t.double().permute(0, 1, 2, 4, 3) for t in gs])
    close(d_gev, r.grad, 1e-6, 1e-7, "d gev")


def test_geo_pyramid_function_at_d128():
    """G.GeoPyramid forward and backward under autograd at D = 128 (max_disp 512), the largest range whose forward tile fits."""
    from anystereo import grad as G
    b, g, d, h, w, L = 1, 8, 128, 2, 37, 2
    gev = U((b, g, d, h, w), 420)
    gs = [U((b, h, w, d >> i, g), 421 + i) for i in range(L)]
    a = _leaf(gev, DEV)
    lv = G.GeoPyramid.apply(a, L)
    torch.autograd.backward(lv, [t.to(DEV) for t in gs])
    r = _leaf(gev, dt=torch.float64)
    ref = O.geo_pyramid(r, L)
    for i in range(L):
        close(lv[i].permute(0, 1, 2, 4, 3), ref[i], 0, 1e-7, what=f"geo level {i}")
    torch.autograd.backward(ref, [t.double().permute(0, 1, 2, 4, 3) for t in gs])
    close(a.grad, r.grad, 1e-6, 1e-7, "d gev")


def test_disparity_regression_backward_large_d():
    from anystereo import grad as G
    D = 192
    cost = U((2, D, 5, 33), 440, -4, 4)
    g = U((2, 1, 5, 33), 441)
    a = _leaf(cost, DEV)
    out = G.DisparityRegression.apply(a, True)
    out.backward(g.to(DEV))
    r = _leaf(cost, dt=torch.float64)
    ref = O.disparity_regression(torch.softmax(r, 1), D)
    ref.backward(g.double())
    close(out, ref, 2e-5, 1e-6, "init disparity")
    close(a.grad, r.grad, 2e-5, 1e-6, "d cost")


@pytest.mark.parametrize("d", [96, 192])
def test_lookup_backward_large_d(d):
    """The transpose of the lookup on pyramids of D = 96 / 192 (what G.Lookup's backward launches), as
    test_lookup_backward_is_transpose holds it at D = 48."""
    from anystereo import ops
    b, h, w, g, L, r = 1, 3, 24, 8, 2, 4
    corr = [U((b, h, w, w >> i), 40 + i) for i in range(L)]
    geo = [U((b, h, w, d >> i, g), 50 + i) for i in range(L)]
    disp = _planted_disp(b, h, w, d, 60)
    gout = U((b, L * 9 * (g + 1), h, w), 61)
    dg, dc = ops.geo_corr_lookup_backward(disp.to(DEV), gout.to(DEV), [tuple(t.shape) for t in geo], [tuple(t.shape) for t in corr], r)
    cr = [t.clone().double().requires_grad_(True) for t in corr]
    gr = [t.permute(0, 1, 2, 4, 3).clone().double().requires_grad_(True) for t in geo]
    O.geo_corr_lookup(gr, cr, disp.double(), r).backward(gout.double())
    for i in range(L):
        close(dc[i], cr[i].grad, 2e-5, 1e-6, f"d_corr{i}")
        close(dg[i].permute(0, 1, 2, 4, 3), gr[i].grad, 2e-5, 1e-6, f"d_geo{i}")
