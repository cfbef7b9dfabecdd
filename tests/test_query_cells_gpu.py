"""The query-cell arithmetic of the upsampler kernels (csrc/query.h) at the one place where its rounding rule matters: queries
exactly ON a cell boundary, where ((c + 1) * n - 1) / 2 is k + 0.5 and grid_sample(nearest) takes the EVEN index.  The golden
fixtures never get there (their queries are make_coord centres of a 4 x s grid), so every kernel that locates a query is
run here on a query set that does, against the CPU oracle (oracle/ops.py), never against another kernel's cell.

Query set of a case with sources H0 x W0 and H1 x W1: the cartesian product of
  rows    (2k + 2) / n - 1 for n in (H0, H1), k = -1 .. n - 1;  +-1, +-1.5, -1 + 1e-6, 1 - 1e-6
  columns the same for (W0, W1)
followed by make_coord([13, 29]) as ordinary filler; batch element 1 holds the same queries in a fixed shuffled order.
Case "pow2" (4 x 8 and 8 x 16): every boundary is exact in fp32 and an exact tie.  Case "mixed" (6 x 12 and 12 x 24): the
boundaries are rounded, only some are exact ties.

Tolerances are the ones the existing tests hold the same quantities to: rel 2e-6 and convex 1e-5 (test_liif_golden), the
quarter-nearest sum 1e-4 and its rel 1e-5 (test_liif_variants.py), fused tail / direct second input against the staged path
3e-5 (test_liif_fused_tail_vs_staged, test_liif_tail_direct_second_input).  Gathered values and integer-valued scatter sums are
compared exactly.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ops as O

DEV = "cuda:0"
CASES = {"pow2": ((4, 8), (8, 16)), "mixed": ((6, 12), (12, 24))}
B = 2


def U(shape, seed, lo=-1.0, hi=1.0):
    from anystereo.harness.synthetic import det_uniform
    return det_uniform(shape, seed, lo, hi)


def close(a, b, rtol, atol, what):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values in the HIP result"
    err = (a - b).abs().max().item()
    lim = atol + rtol * b.abs().max().item()
    print(f"{what}: max abs err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


def _axis(ns):
    vals = []
    for n in ns:
        k = torch.arange(-1, n, dtype=torch.float32)
        vals.append((2 * k + 2) / n - 1)
    vals.append(torch.tensor([1.0, -1.0, 1.5, -1.5, -1 + 1e-6, 1 - 1e-6], dtype=torch.float32))
    return torch.cat(vals)


@functools.lru_cache(maxsize=None)
def queries(case):
    """coord [B,Q,2] fp32 on the CPU (read-only: every user clones)."""
    (h0, w0), (h1, w1) = CASES[case]
    rows, cols = _axis((h0, h1)), _axis((w0, w1))
    q = torch.cat([torch.stack(torch.meshgrid(rows, cols, indexing="ij"), -1).view(-1, 2), O.make_coord([13, 29]).view(-1, 2)])
    perm = torch.argsort(U((q.shape[0],), 31, 0.0, 1.0))
    return torch.stack([q, q[perm]]).contiguous()


def cells(coord, h, w):
    """The oracle's nearest cell (iy, ix) of every query, int64 [B,Q]."""
    cc = coord.clamp(-1 + 1e-6, 1 - 1e-6)
    return O.nearest_index(cc[..., 0], h), O.nearest_index(cc[..., 1], w)


def oracle_key(coord, sizes):
    (h0, w0), (h1, w1) = sizes
    iy0, ix0 = cells(coord, h0, w0)
    iy1, ix1 = cells(coord, h1, w1)
    return ((iy0 * w0 + ix0) * 4 + ((iy1 & 1) << 1) + (ix1 & 1)).to(torch.int32)


def index_map(c, h, w):
    """[B,c,h,w] whose every element is its own flat index: a gathered value names the element it came from."""
    return torch.arange(B * c * h * w, dtype=torch.float32).view(B, c, h, w)


def int_valued(shape, seed, lo=-4, hi=4):
    return torch.round(U(shape, seed, float(lo), float(hi)))


def test_query_set_and_oracle_at_ties():
    """CPU: what the other tests rest on.  pow2: every interior boundary is an exact tie and the oracle's index there is
    F.grid_sample(nearest)'s, the even one; both cases: the clamped index is always inside the map."""
    for case, sizes in CASES.items():
        coord = queries(case)
        for h, w in sizes:
            iy, ix = cells(coord, h, w)
            assert iy.min() >= 0 and iy.max() < h and ix.min() >= 0 and ix.max() < w
    for n in (4, 8, 16):
        k = torch.arange(0, n - 1, dtype=torch.float32)
        c = (2 * k + 2) / n - 1
        assert torch.equal(((c + 1) * n - 1) / 2, k + 0.5), "exact ties"
        idx = O.nearest_index(c, n)
        assert torch.equal(idx, (2 * torch.round((k + 0.5) / 2)).long()), "ties to even"
        src = torch.arange(n, dtype=torch.float32).view(1, 1, 1, n)
        grid = torch.stack([c, torch.zeros_like(c)], -1).view(1, 1, -1, 2)  # grid_sample's (x, y)
        got = F.grid_sample(src, grid, mode="nearest", align_corners=False).view(-1)
        assert torch.equal(got.long(), idx), "oracle == grid_sample(nearest) on ties"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_rel_key(case):
    from anystereo import ops
    sizes = CASES[case]
    coord = queries(case)
    rel, key = ops.liif_rel_key(coord.to(DEV), list(sizes), want_rel=True, want_key=True)
    want_key = oracle_key(coord, sizes)
    bad = (key.cpu() != want_key).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} sort keys differ from the oracle's cells, first at (b, q) = {bad[0].tolist()}: " \
                             f"coord {coord[bad[0, 0], bad[0, 1]].tolist()}"
    for s, (h, w) in enumerate(sizes):
        want, _ = O.liif_query(index_map(1, h, w), coord)
        close(rel[:, 2 * s:2 * s + 2], want.permute(0, 2, 1), 0, 2e-6, f"rel, source {s}")
    one, _ = ops.liif_rel_key(coord.to(DEV), [sizes[0]], want_rel=True, want_key=False)
    assert torch.equal(one, rel[:, :2]), "one source == first of two"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gather_and_latent(case):
    from anystereo import ops
    coord = queries(case)
    cd = coord.to(DEV)
    q = coord.shape[1]
    for (h, w), c in zip(CASES[case], (8, 4)):
        feat = index_map(c, h, w)
        rel, qf = O.liif_query(feat, coord)
        lat = torch.empty(B, c + 2, q, device=DEV)
        ops.liif_gather(feat.to(DEV), cd, lat, 0)
        assert torch.equal(lat[:, :c].cpu(), qf.permute(0, 2, 1)), f"liif_gather {h}x{w}: gathered values"
        close(lat[:, c:], rel.permute(0, 2, 1), 0, 2e-6, f"liif_gather {h}x{w}: rel")
        for unfold9 in (False, True):
            src = O.unfold3x3(feat) if unfold9 else feat
            for n_samp in (1, 4):
                rel, qf = O.liif_query(src, coord) if n_samp == 1 else O.liif_query_quater(src, coord)
                width = ops.liif_latent_width(c, unfold9=unfold9, n_samp=n_samp)
                lat = torch.empty(B, width, q, device=DEV)
                ops.liif_latent(feat.to(DEV), cd, lat, 0, unfold9=unfold9, n_samp=n_samp)
                what = f"liif_latent {h}x{w} unfold9={unfold9} n_samp={n_samp}"
                assert torch.equal(lat[:, :width - 2].cpu(), qf.permute(0, 2, 1)), f"{what}: gathered values"
                close(lat[:, width - 2:], rel.permute(0, 2, 1), 0, 2e-6 if n_samp == 1 else 1e-5, f"{what}: rel")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_convex_upsample(case):
    from anystereo import ops
    coord = queries(case)
    cd = coord.to(DEV)
    q = coord.shape[1]
    h, w = CASES[case][0]
    s = 1.5
    disp = U((B, 1, h, w), 41, 0.0, 30.0)
    sv = torch.full((B,), s, device=DEV)
    m9 = U((B, 9, q), 42, -2.0, 2.0)
    got = ops.convex_upsample(disp.to(DEV), m9.to(DEV), cd, scale=sv, mask_is_logits=True)
    close(got[:, 0], O.convex_upsample(disp * 4.0 * s, torch.softmax(m9, 1), coord.clone()), 1e-5, 1e-5, "convex_upsample")
    m4 = U((B, 4, q), 43, -2.0, 2.0)
    got = ops.convex_upsample_quater(disp.to(DEV), m4.to(DEV), cd, scale=sv, mask_is_logits=True)
    close(got[:, 0], O.convex_upsample_quater(disp * 4.0 * s, torch.softmax(m4, 1), coord.clone()), 0, 1e-4, "convex_upsample_quater")
    assert torch.equal(cd.cpu(), coord), "the operator layer leaves the coordinates alone"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gather_mlp1_vs_staged(case):
    """relu(u0[n0(q)] + u1[n1(q)] + wrel . rel(q) + bias) against the same sum over liif_gather's rows and rel."""
    from anystereo import ops
    (h0, w0), (h1, w1) = CASES[case]
    coord = queries(case).to(DEV)
    q, c = coord.shape[1], 12
    u0, u1 = U((B, c, h0, w0), 51).to(DEV), U((B, c, h1, w1), 52).to(DEV)
    wrel, bias = U((c, 4), 53).to(DEV), U((c,), 54).to(DEV)
    lat = torch.empty(B, 2 * (c + 2), q, device=DEV)
    ops.liif_gather(u0, coord, lat, 0)
    ops.liif_gather(u1, coord, lat, c + 2)
    lat = lat.double()
    rel = torch.cat([lat[:, c:c + 2], lat[:, 2 * c + 2:]], 1)
    want = torch.relu(lat[:, :c] + lat[:, c + 2:2 * c + 2] + torch.einsum("ck,bkq->bcq", wrel.double(), rel) + bias.double().view(1, -1, 1))
    close(ops.liif_gather_mlp1(u0, u1, coord, wrel, bias), want, 3e-5, 3e-5, "gather_mlp1, two sources")
    want1 = torch.relu(lat[:, :c] + torch.einsum("ck,bkq->bcq", wrel[:, :2].double(), rel[:, :2]))
    close(ops.liif_gather_mlp1(u0, None, coord, wrel[:, :2].contiguous(), None), want1, 3e-5, 3e-5, "gather_mlp1, one source")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_tail_vs_staged(case):
    """liif_tail, and liif_tail_direct for the second input, against the staged path on the same module: a wrong cell is a
    gross error at these sizes."""
    from anystereo import ops
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.liif import liif_out_multi_scale_Training
    (h, w), (h1, w1) = CASES[case]
    up = liif_out_multi_scale_Training(encoder_dim=208, mlphidden_list=[128, 64, 64], pos_dim=0, unfold="with_v2ISU",
                                       affinity_settings={"win_w": 3, "win_h": 3, "dilation": [1, 2, 4, 8]},
                                       number_input=2, chanels=[176, 32]).eval()
    fill_module_deterministic(up, base_seed=11, gain=2.0)
    up = up.to(DEV)
    coord = queries(case)
    x4, x2 = U((B, 176, h, w), 61, -1.5, 1.5).to(DEV), U((B, 32, h1, w1), 62, -1.5, 1.5).to(DEV)
    disp = U((B, 1, h, w), 63, 0.0, 40.0).to(DEV)
    sv = torch.full((B,), 1.5, device=DEV)
    parts = [[x4[:, :48].contiguous(), x4[:, 48:].contiguous()], [x2]]
    prev = ops.get_precision()
    ops.set_precision("split")
    outs = {}
    try:
        with torch.no_grad():
            c2 = coord.clone().to(DEV)
            staged_logits = up([x4, x2], c2, sv.view(-1, 1))
            staged = ops.convex_upsample(disp, staged_logits, c2.clamp(-1 + 1e-6, 1 - 1e-6), scale=sv, mask_is_logits=True)
            for direct in (False, True):
                up.direct_second_input = direct
                c1 = coord.clone().to(DEV)
                outs[direct] = up.upsample_fused(parts, c1, disp, sv, want_logits=True)
                assert torch.equal(c1.cpu(), coord.clamp(-1 + 1e-6, 1 - 1e-6)), "coordinates are clamped in place"
    finally:
        up.__dict__.pop("direct_second_input", None)
        ops.set_precision(prev)
    for direct, name in ((False, "liif_tail"), (True, "liif_tail_direct")):
        close(outs[direct][1], staged_logits, 3e-5, 3e-5, f"{name} vs staged logits")
        close(outs[direct][0], staged, 3e-5, 3e-5, f"{name} vs staged disparity")


def _orders(case):
    """(name, coord [B,Q,2], perm [B,Q]) with the queries as they are and sorted by the oracle's key: only the sorted order
    puts equal cells into consecutive lanes, which is the run-head path of the scatter kernels."""
    coord = queries(case)
    ident = torch.arange(coord.shape[1]).expand(B, -1)
    perm = torch.argsort(oracle_key(coord, CASES[case]).long(), dim=1, stable=True)
    return (("unsorted", coord, ident), ("sorted", torch.gather(coord, 1, perm.unsqueeze(-1).expand(-1, -1, 2)).contiguous(), perm))


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_scatter_add_backward(case):
    """Integer-valued incoming gradients: every sum is exact whatever order the atomics land in, so the scatter kernels must
    EQUAL the oracle's index_add, with the queries unsorted and sorted by key."""
    from anystereo import ops
    h, w = CASES[case][0]
    c, ctot, coff = 5, 9, 3
    for name, coord, perm in _orders(case):
        q = coord.shape[1]
        d_rows = int_valued((B, ctot, q), 71)
        d_rows = torch.gather(d_rows, 2, perm.unsqueeze(1).expand(-1, ctot, -1)).contiguous()
        iy, ix = cells(coord, h, w)
        want = torch.zeros(B, c, h * w)
        for b in range(B):
            want[b].index_add_(1, iy[b] * w + ix[b], d_rows[b, coff:coff + c])
        got = ops.liif_scatter_add(d_rows.to(DEV), coord.to(DEV), c, h, w, coff=coff)
        assert torch.equal(got.cpu(), want.view(B, c, h, w)), f"liif_scatter_add, {name} queries"
        for unfold9 in (False, True):
            for n_samp in (1, 4):
                feat = index_map(c, h, w).double().requires_grad_(True)
                src = O.unfold3x3(feat) if unfold9 else feat
                _, qf = O.liif_query(src, coord) if n_samp == 1 else O.liif_query_quater(src, coord)  # cells from the fp32 coordinates
                nf = qf.shape[2]
                d_lat = int_valued((B, nf + 2, q), 72)
                qf.backward(d_lat[:, :nf].permute(0, 2, 1).double())
                got = ops.liif_latent_backward(d_lat.to(DEV), coord.to(DEV), 0, c, h, w, unfold9=unfold9, n_samp=n_samp)
                assert torch.equal(got.cpu().double(), feat.grad), f"liif_latent_backward unfold9={unfold9} n_samp={n_samp}, {name} queries"


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_convex_upsample_backward(case):
    """G.ConvexUpsample with integer-valued disparity, weights (used as they are: mask_is_logits=False, no scale) and incoming
    gradient: output, d_mask and the scattered d_disp are exact and must equal autograd through the oracle."""
    from anystereo import grad as G
    h, w = CASES[case][0]
    for name, coord, perm in _orders(case):
        q = coord.shape[1]
        disp = int_valued((B, 1, h, w), 81, 0, 9)
        mask = torch.gather(int_valued((B, 9, q), 82, -3, 3), 2, perm.unsqueeze(1).expand(-1, 9, -1)).contiguous()
        g = torch.gather(int_valued((B, 1, q), 83, -3, 3), 2, perm.unsqueeze(1)).contiguous()
        d0, m0 = disp.clone().double().requires_grad_(True), mask.clone().double().requires_grad_(True)
        want = O.convex_upsample(d0, m0, coord.clone())  # cells from the fp32 coordinates
        want.backward(g[:, 0].double())
        d1, m1 = disp.clone().to(DEV).requires_grad_(True), mask.clone().to(DEV).requires_grad_(True)
        got = G.ConvexUpsample.apply(d1, m1, coord.to(DEV), None, False)
        got.backward(g.to(DEV))
        assert torch.equal(got[:, 0].detach().cpu().double(), want.detach()), f"ConvexUpsample forward, {name} queries"
        assert torch.equal(m1.grad.cpu().double(), m0.grad), f"ConvexUpsample d_mask, {name} queries"
        assert torch.equal(d1.grad.cpu().double(), d0.grad), f"ConvexUpsample d_disp, {name} queries"
