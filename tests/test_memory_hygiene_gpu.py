"""GPU (-m gpu): no kernel reads memory nobody wrote, none writes outside its output (tests/_guarded.py).

One row per launching symbol of anystereo._lib.SIGNATURES, reached through its `ops` wrapper (its autograd Function in
anystereo.grad for the backward symbols; the library call itself for the three symbols without a wrapper of their own).  A row
builds its inputs on the CPU from det_uniform and runs three times — plain (inputs placed with zero-filled neighbours, no
patching), under guarded(0xFF) (NaN) and under guarded(0x47) (finite garbage) — and must leave every guard intact (those around
the inputs too), return finite tensors, and return the SAME BITS in all three runs.  Rows whose kernel accumulates with float
atomics (the atomicAdd uses of csrc/backward.hip, csrc/liif_variants.hip, csrc/liif_fused.hip; csrc/lookup.hip names atomicAdd
in a comment only: its kernels are gather-form and their rows are held bit-equal) are compared within the tolerance of the
existing parity test of that entry, which the row cites.  No tolerance is set here.

Weight packs are cached objects (PackedConv, the lookup / IR-block / stem / tail / lowres / MLP-backward images): every run builds
a fresh one, so that the pack kernel's own output and its padding are poisoned, and the pack rows return the image itself.

Blocked split-fp16 (BS8) buffers: a row hands a producer a blocked tensor of exactly the channels it fills, so the whole record
array, channel padding included (the contract of DESIGN.md: the producer zeroes it), must come back the same bits.

uint8 buffers are poisoned like floating-point ones.  The uint8 scratch the kernels receive are the packed weight images (lookup +
convc1, IR block, 7x7 stem, LIIF lowres / tail / MLP-backward): their pack kernels write split-fp16 fragment values and fp32 biases
only (csrc/lookup.hip frag_pack*, irblock.hip, stem7x7.hip, liif_fused.hip *_pack_kernel) — no index or counter that a consumer reads
before writing; the image outputs of eval_images / lr_consistency are written in full.  The one uint8 buffer that holds indices and
counts, the sparse-mode scratch of ops.train_queries, gets guards only (tests/_guarded.py).

Pointer-alignment branches (the second half of the module): an entry that chooses its kernel by a pointer's alignment gets a case
with the pointer off the boundary, held to its parity test's reference and to the aligned run's bits; an entry that demands an
alignment must refuse with the library's message before anything is launched.

The coverage check: the loaded library's functions are wrapped with a call counter for the duration of the module; after the
table has run every name of SIGNATURES has been called under a guard or stands in EXEMPT with its reason
(tests/test_guarded_cpu.py holds EXEMPT ∪ rows == SIGNATURES without a GPU).  The module writes profiles/memory_hygiene.txt at
teardown: each symbol, its rows' shapes and compare modes, the cited parity tests, the EXEMPT reasons.
"""
import ctypes as C
import os

import pytest
import torch

import _conv_cases as cc
import _guarded as GD
from _guarded import hygiene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# Symbols that launch nothing on a tensor: one line each.
EXEMPT = {
    "as_set_precision": "setter of the process-wide matrix-core mode",
    "as_get_precision": "getter",
    "as_set_fast16": "setter of the reduced-precision flag",
    "as_get_fast16": "getter",
    "as_last_error_string": "host string of the last error",
    "as_abi_version": "host constant",
    "as_source_hash": "host constant",
    "as_device_count": "host query",
    "as_graph_replace_memsets": "edits a captured graph's nodes on the host; takes no tensor and no stream",
    "as_ir_block_pack_bytes": "size query",
    "as_lookup_convc1_pack_bytes": "size query",
    "as_lookup_split_overflow": "reads (and resets) a device counter with a synchronous copy; no tensor argument",
    "as_conv_split_overflow": "overflow counter, as above",
    "as_volumes_split_overflow": "overflow counter, as above",
    "as_pointwise_split_overflow": "overflow counter, as above",
    "as_liif_split_overflow": "overflow counter, as above",
    "as_conv2d_plan": "the planner: host arithmetic on a descriptor, never dereferences a data pointer",
    "as_conv1x1_stream_ok": "host predicate on a descriptor",
    "as_conv_ws_elems": "size query",
    "as_conv_pack_size": "size query",
    "as_conv_pack_size_split": "size query",
    "as_instance_norm_ws_bytes": "size query",
    "as_conv7x7_c3_pack_bytes": "size query",
    "as_affinity_window_ws_bytes": "size query",
    "as_liif_affinity_ws_bytes": "size query",
    "as_liif_lowres_pack_bytes": "size query",
    "as_liif_tail_image_bytes": "size query",
    "as_liif_rows_pitch": "host constant",
    "as_liif_mlp_bwd_image_bytes": "size query",
    "as_conv2d_wgrad_ws_bytes": "size query",
    "as_conv7x7_c1_wgrad_ws_bytes": "size query",
    "as_dwconv3x3_wgrad_slices": "size query",
    "as_init_head_partial_elems": "size query",
    "as_disp_metrics_partial_elems": "size query",
    "as_train_queries_ws_bytes": "size query (reads two host arrays)",
}

# the existing parity tests whose bound the float-atomics rows take: (limit as a function of max |b|, that limit in words, the test)
T_GATHER_BWD = (lambda m: 1e-5 + 1e-4 * m, "|a - b| <= 1e-5 + 1e-4 * max |b|",
                "test_hip_parity.py::test_liif_gather_and_convex_backward ('d feat': close(1e-4, 1e-5))")
T_CONVEX_BWD = (lambda m: 1e-5 + 1e-4 * m, "|a - b| <= 1e-5 + 1e-4 * max |b|",
                "test_hip_parity.py::test_liif_gather_and_convex_backward ('d disp': close(1e-4, 1e-5))")
T_VARIANTS = (lambda m: 2e-4 * max(1.0, m), "|a - b| <= 2e-4 * max(1, max |b|)", "test_liif_variants.py::test_hip_gradients_match_oracle")
T_MLP_BWD = (lambda m: 2e-4 * m, "max |a - b| / max |b| < 2e-4", "test_hip_parity.py::test_liif_mlp_tail_function_vs_fp64")


class Row:
    def __init__(self, name, symbols, shape, fn, tol, precision, note):
        self.name, self.symbols, self.shape, self.fn, self.tol, self.precision, self.note = name, tuple(symbols), shape, fn, tol, precision, note


ROWS = []


def row(name, symbols, shape, tol=None, precision="split", note=""):
    """Register fn(put) -> result as a row.  tol: None = bit-equal; one of the T_* triples for a float-atomics entry; a dict
    {result index: such a triple} where only some results come from atomics."""
    def deco(fn):
        ROWS.append(Row(name, symbols, shape, fn, tol, precision, note))
        return fn
    return deco


def U(shape, seed, lo=-1.0, hi=1.0):
    from anystereo.harness.synthetic import det_uniform
    return det_uniform(shape, seed, lo, hi)


def _lib():
    from anystereo import _lib as L
    return L


def _stream():
    from anystereo import ops
    return ops._stream()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _leaf(put, t):
    return put(t).requires_grad_(True)


def _coords(b, h, w, scale, seed, nq=None):
    """Query coordinates [b, Q, 2] of an (h x w) * 4 * scale grid: the whole raster, or nq of its points with the corners +-1."""
    from anystereo.nn.liif import make_coord
    grid = make_coord([round(4 * h * scale), round(4 * w * scale)])
    if nq is not None:
        idx = (U((nq,), seed, 0.0, 1.0) * grid.shape[0]).long().clamp(max=grid.shape[0] - 1)
        grid = grid[idx].clone()
        grid[0] = torch.tensor([-1.0, 1.0])
        grid[1] = torch.tensor([1.0, -1.0])
    return grid.view(1, -1, 2).repeat(b, 1, 1).contiguous()


# ---- the detector detects on the device (the CPU statement of this is tests/test_guarded_cpu.py) -------------------------------

def test_detector_on_the_device():
    """A write one element past a torch.empty output (it lands inside the big buffer: nothing faults) trips the guard check and
    names the allocation site; `out + scratch` with the scratch unwritten trips finiteness under 0xFF and equality under 0x47; the
    clean form passes."""
    x = U((3, 4), 9)

    def writes_one_past(put):
        out = torch.empty((3, 4), device=DEV)
        out.copy_(put(x) * 2)
        if out._base is not None:
            torch.as_strided(out, (1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
        return out

    def reads_unwritten_scratch(put):
        a = put(x)
        out, scratch = torch.empty_like(a), torch.empty_like(a)
        if scratch._base is None:
            scratch.zero_()  # the plain run stands for the test process whose allocator happens to hand back zeros
        out.copy_(a * 2)
        return out + scratch

    def clean(put):
        a = put(x)
        out = torch.empty_like(a)
        out.copy_(a * 2)
        return out

    with pytest.raises(AssertionError, match=r"back guard of the empty allocated at .*test_memory_hygiene_gpu.py:\d+"):
        hygiene(writes_one_past, DEV)
    with pytest.raises(AssertionError, match="fill 0xFF: result 0 .* is not finite"):
        hygiene(reads_unwritten_scratch, DEV)
    with pytest.raises(AssertionError, match="fill 0x47: result 0 .* differs from the plain run"):
        hygiene(reads_unwritten_scratch, DEV, patterns=(GD.FINITE_FILL,))
    assert torch.equal(hygiene(clean, DEV).cpu(), x * 2)
    with GD.guarded(GD.NAN_FILL) as g:
        t = torch.empty((5, 7), device=DEV)
        assert t.data_ptr() % GD.ALIGN == 0 and g.is_poisoned(t) and len(g.buffers) == 1 and g.buffers[0].lo == GD.GUARD
        assert torch.empty(3).device.type == "cpu" and len(g.buffers) == 1


# ---- volumes, pyramids, lookup ----------------------------------------------------------------------------------------------

def _corr_build(put):
    from anystereo import ops
    return ops.corr_build_pyramid(put(U((2, 33, 3, 21), 1)), put(U((2, 33, 3, 13), 2)), 3)


row("corr_build_pyramid[fp32]", ["as_corr_build_pyramid"], "f1 (2,33,3,21) f2 (2,33,3,13) L=3", precision="fp32")(_corr_build)
row("corr_build_pyramid[split]", ["as_corr_build_pyramid"], "f1 (2,33,3,21) f2 (2,33,3,13) L=3")(_corr_build)


@row("geo_pyramid", ["as_geo_pyramid"], "gev (2,4,17,2,33) L=3")
def _(put):
    from anystereo import ops
    return ops.geo_pyramid(put(U((2, 4, 17, 2, 33), 3)), 3)


def _lookup_operands(put, b, h, w, g, d, nl, seed=30):
    corr = [put(U((b, h, w, w >> i), seed + i, -3, 3)) for i in range(nl)]
    geo = [put(U((b, h, w, d >> i, g), seed + 10 + i, -3, 3)) for i in range(nl)] if g else None
    disp = U((b, 1, h, w), seed + 20, -6.0, w + 6.0)
    disp.view(-1)[:6] = torch.tensor([0.0, 3.0, 7.5, -0.5, float(w - 1), 1e-7])
    return geo, corr, put(disp)


@row("geo_corr_lookup[geo]", ["as_geo_corr_lookup_fwd"], "b 2, 2x33, G 4, D 16, L 3, r 2 (test_lookup_vs_oracle's smallest row, batch 2)")
def _(put):
    from anystereo import ops
    geo, corr, disp = _lookup_operands(put, 2, 2, 33, 4, 16, 3)
    return ops.geo_corr_lookup(geo, corr, disp, 2)


@row("geo_corr_lookup[corr only]", ["as_geo_corr_lookup_fwd"], "b 2, 5x37, G 0, L 4, r 4")
def _(put):
    from anystereo import ops
    geo, corr, disp = _lookup_operands(put, 2, 5, 37, 0, 0, 4)
    return ops.geo_corr_lookup(None, corr, disp, 4)


@row("geo_corr_lookup_backward", ["as_geo_corr_lookup_bwd", "as_geo_corr_lookup_bwd_accum"], "b 2, 3x24, G 8, D 48, L 2, r 4; then a second lookup added into the first's gradients",
     note="gather-form kernels into zero-filled gradients (torch.zeros): no atomics")
def _(put):
    from anystereo import ops
    b, h, w, g, d, nl, r = 2, 3, 24, 8, 48, 2, 4
    gs = [(b, h, w, d >> i, g) for i in range(nl)]
    cs = [(b, h, w, w >> i) for i in range(nl)]
    disp, gout = put(U((b, 1, h, w), 60, -4.0, w + 4.0)), put(U((b, nl * 9 * (g + 1), h, w), 61))
    acc = ops.geo_corr_lookup_backward(disp, gout, gs, cs, r)
    first = [t.clone() for t in acc[0] + acc[1]]
    disp2, gout2 = put(U((b, 1, h, w), 62, -4.0, w + 4.0)), put(U((b, nl * 9 * (g + 1), h, w), 63))
    acc = ops.geo_corr_lookup_backward(disp2, gout2, gs, cs, r, into=acc)
    return first, acc


def _convc1_operands(put, g, nl, seed):
    cin = nl * 9 * (g + 1)
    return put(U((64, cin, 1, 1), seed) * (3.0 / cin) ** 0.5), put(U((64,), seed + 1) * 0.1)


for _tag, _g, _d, _nl in (("igev", 8, 48, 2), ("raft", 0, 0, 4)):
    @row(f"lookup_convc1[{_tag}]", ["as_lookup_convc1_pack", "as_lookup_convc1_fwd"], f"b 2, 3x20, G {_g}, L {_nl}, r 4; fp32 and blocked result",
         note="the blocked result holds exactly the 64 channels the kernel fills; the pack image is returned too")
    def _(put, g=_g, d=_d, nl=_nl):
        from anystereo import ops
        geo, corr, disp = _lookup_operands(put, 2, 3, 20, g, d, nl, seed=300)
        wt, bias = _convc1_operands(put, g, nl, 305)
        pack = ops.LookupConvPack().get(wt, bias)
        bs = ops.BS8.empty(2, 64, 3, 20, DEV)
        out = ops.lookup_convc1(geo, corr, disp, 4, pack, out_bs=bs, want_f32=True)
        return out, bs, pack.image

    for _mode in ("full", "lite"):
        @row(f"loop_front[{_tag}, {_mode}]", ["as_loop_front_fwd"], f"b 2, 9x21, G {_g}, L {_nl}, r 4, 2 tap groups; {_mode}: " +
             ("lookup + convc1 + 7x7 in one grid" if _mode == "full" else "finish + lookup + convc1, no 7x7"))
        def _(put, g=_g, d=_d, nl=_nl, mode=_mode):
            from anystereo import ops
            b, h, w = 2, 9, 21
            geo, corr, disp = _lookup_operands(put, b, h, w, g, d, nl, seed=700)
            wt, bias = _convc1_operands(put, g, nl, 705)
            pack = ops.LookupConvPack().get(wt, bias)
            taps, hb = put(U((b, 18, h, w), 707) * 0.2), put(U((1,), 708))
            w7, b7 = (put(U((64, 1, 7, 7), 709) * 0.2), put(U((64,), 710) * 0.1)) if mode == "full" else (None, None)
            return ops.loop_front(geo, corr, taps, hb, disp, 4, pack, w7, b7)


for _dt in (torch.float32, torch.float16):
    @row(f"corr_sampler[{str(_dt)[6:]}]", ["as_corr_sampler_fwd", "as_corr_sampler_bwd"], "volume (2,3,20,17) r 3, coords with 2 channels")
    def _(put, dt=_dt):
        from anystereo import ops
        n, h1, w1, w2, r = 2, 3, 20, 17, 3
        vol = put(U((n, h1, w1, w2), 70, -2, 2).to(dt))
        coords = torch.stack([U((n, h1, w1), 71, -6.0, w2 + 6.0), torch.zeros(n, h1, w1)], dim=1)
        coords[0, 0, 0, :3] = torch.tensor([0.0, 2.5, float(w2 - 1)])
        coords = put(coords)
        out = ops.corr_sampler_forward(vol, coords, r)
        return out, ops.corr_sampler_backward(vol, coords, put(U(tuple(out.shape), 72).to(dt)), r)


@row("gwc_volume", ["as_gwc_volume_fwd", "as_gwc_volume_bwd"], "fl, fr (2,32,2,21), D 10, 4 groups; forward and backward")
def _(put):
    from anystereo import grad as G
    fl, fr = _leaf(put, U((2, 32, 2, 21), 80)), _leaf(put, U((2, 32, 2, 21), 81))
    vol = G.GwcVolume.apply(fl, fr, 10, 4)
    vol.backward(put(U(tuple(vol.shape), 82)))
    return vol.detach(), fl.grad, fr.grad


for _sm in (True, False):
    @row(f"disparity_regression[softmax={_sm}]", ["as_disparity_regression", "as_disparity_regression_bwd"], "cost (2,17,3,21); forward and backward")
    def _(put, sm=_sm):
        from anystereo import grad as G
        cost = U((2, 17, 3, 21), 83, -3, 3)
        cost = _leaf(put, cost if sm else torch.softmax(cost, 1))
        out = G.DisparityRegression.apply(cost, sm)
        out.backward(put(U(tuple(out.shape), 84)))
        return out.detach(), cost.grad


@row("corr_pyramid_backward", ["as_corr_pyramid_bwd"], "f1 (2,16,3,21) f2 (2,16,3,13) L=3 through grad.CorrBuildPyramid")
def _(put):
    from anystereo import grad as G
    f1, f2 = _leaf(put, U((2, 16, 3, 21), 85)), _leaf(put, U((2, 16, 3, 13), 86))
    lv = G.CorrBuildPyramid.apply(f1, f2, 3)
    torch.autograd.backward(list(lv), [put(U(tuple(t.shape), 87 + i)) for i, t in enumerate(lv)])
    return [t.detach() for t in lv], f1.grad, f2.grad


@row("geo_pyramid_backward", ["as_geo_pyramid_bwd"], "gev (2,4,17,2,33) L=3 through grad.GeoPyramid")
def _(put):
    from anystereo import grad as G
    gev = _leaf(put, U((2, 4, 17, 2, 33), 90))
    lv = G.GeoPyramid.apply(gev, 3)
    torch.autograd.backward(list(lv), [put(U(tuple(t.shape), 91 + i)) for i, t in enumerate(lv)])
    return gev.grad


@row("init_head_bwd", ["as_init_head_bwd", "as_init_head_wgrad_reduce"], "geo (2,8,12,9,20) (test_init_head_bwd_vs_fp64_autograd's smallest row, batch 2)")
def _(put):
    from anystereo import ops
    b, d, h, w = 2, 12, 9, 20
    return ops.init_head_bwd(put(U((b, 8, d, h, w), 95)), put(U((1, 8, 3, 3, 3), 96) * 0.3), put(U((b, d, h, w), 97, -3, 3)), put(U((b, 1, h, w), 98)))


# ---- convolutions other than conv2d's table -----------------------------------------------------------------------------------

for _split in (False, True):
    @row(f"conv_pack_weights[{'split' if _split else 'fp32'}]", ["as_conv_pack_weights_split" if _split else "as_conv_pack_weights"],
         "weights (40,37,3,3) and (100,37,1,1): the pack images themselves", precision="split" if _split else "fp32",
         note="the packed image is returned, so its padding must be written by the pack kernel")
    def _(put):
        from anystereo import ops
        return [ops.PackedConv().get([put(U((co, 37, k, k), 100 + k))], [None]).wpack for co, k in ((40, 3), (100, 1))]


@row("conv_pack_weights_split_t", ["as_conv_pack_weights_split_t"], "data-gradient packs of weights (40,37,3,3) and (100,37,1,1)")
def _(put):
    from anystereo import ops
    return [ops.PackedConv().get_dgrad(put(U((co, 37, k, k), 104 + k))).wpack for co, k in ((40, 3), (100, 1))]


for _name, _srcs, _cout, _b, _h, _w, _act, _bias, _add, _res in (("16to96_odd_plane", [16], 96, 2, 9, 37, 0, False, False, False),
                                                                    ("32p16to48_two_sources_residual", [32, 16], 48, 1, 7, 26, 1, True, False, True),
                                                                    ("20to8_bias_relu6_add", [20], 8, 1, 5, 33, 4, True, True, False)):
    @row(f"conv1x1_stream[{_name}]", ["as_conv1x1_stream"], f"sources {_srcs} -> {_cout}, b {_b}, {_h}x{_w} (test_pointwise_stream_gpu.py's case)")
    def _(put, srcs=_srcs, cout=_cout, b=_b, h=_h, w=_w, act=_act, bias=_bias, add=_add, res=_res):
        from anystereo import ops
        cin = sum(srcs)
        x = [put(U((b, c, h, w), 9000 + j, -2, 2)) for j, c in enumerate(srcs)]
        pack = ops.PackedConv().get([put(U((cout, cin, 1, 1), 9008) * (3.0 / cin) ** 0.5)], [put(U((cout,), 9009) * 0.1) if bias else None])
        return ops.conv1x1(x, pack, act=act, add=put(U((b, cout + 3, h, w), 9010)) if add else None, add_coff=2 if add else 0,
                           h=put(torch.tanh(U((b, cout, h, w), 9011, -2, 2))) if res else None, force=True)


@row("conv7x7_c1_relu", ["as_conv7x7_c1_relu"], "x (2,1,9,14) -> 64 channels: fp32 result, and blocked result")
def _(put):
    from anystereo import ops
    x, w7, b7 = put(U((2, 1, 9, 14), 110, -3.0, 40.0)), put(U((64, 1, 7, 7), 111) * 0.2), put(U((64,), 112) * 0.1)
    return ops.conv7x7_c1_relu(x, w7, b7), ops.conv7x7_c1_relu(x, w7, b7, out=ops.BS8.empty(2, 64, 9, 14, DEV))


@row("conv7x7_c1_relu[pass-through slot]", ["as_conv7x7_c1_relu", "as_conv2d"], "x (1,1,9,14), copy into slot 127 of a 128-channel blocked tensor",
     note="BS8 contract (DESIGN.md, test_blocked_split_partial_block_and_passthrough): slots 0..126 are another producer's — the row "
          "runs that producer (a 127-channel convolution with a blocked result) on the same tensor, in both orders, and fills nothing else")
def _(put):
    from anystereo import _lib as Lb, ops
    h, w = 9, 14
    x, disp = put(U((1, 128, h, w), 401)), put(U((1, 1, h, w), 402, -3.0, 40.0))
    w7, b7 = put(U((64, 1, 7, 7), 403) * 0.2), put(U((64,), 404) * 0.1)
    outs = []
    for order in (0, 1):
        pe = ops.PackedConv().get([put(U((127, 128, 3, 3), 405) * 0.05)], [put(U((127,), 406))])
        bs = ops.BS8.empty(1, 128, h, w, DEV)
        if order == 0:
            outs.append(ops.conv7x7_c1_relu(disp, w7, b7, copy_out=bs, copy_coff=127))
        ops.conv2d([x], pe, act=Lb.ACT_RELU, out_bs=bs, out_bs_coff=0, bs_only=True)
        if order == 1:
            outs.append(ops.conv7x7_c1_relu(disp, w7, b7, copy_out=bs, copy_coff=127))
        outs.append(bs)
    return outs


@row("conv3x3_few", ["as_conv3x3_few"], "x (2,3,6,5) -> 16, stride 2 and stride 1", precision="fp32")
def _(put):
    from anystereo import _lib as Lb, ops
    x, wp, bias = put(U((2, 3, 6, 5), 120)), put(U((3, 9, 16), 121) * 0.3), put(U((16,), 122))
    return ops.conv3x3_few(x, wp, bias, stride=2, act=Lb.ACT_RELU), ops.conv3x3_few(x, wp, None, stride=1)


def _ir_modules(put, cin, mid, cout, seed):
    import torch.nn as nn
    mods = [nn.Conv2d(cin, mid, 1, bias=False), nn.BatchNorm2d(mid), nn.Conv2d(mid, mid, 3, padding=1, groups=mid, bias=False), nn.BatchNorm2d(mid),
            nn.Conv2d(mid, cout, 1, bias=False), nn.BatchNorm2d(cout)]
    k = 0
    for m in mods:
        m.eval()
        for name, t in list(m.named_parameters()) + [(n, bf) for n, bf in m.named_buffers() if bf.dtype.is_floating_point]:
            lo, hi = (0.5, 1.5) if name in ("weight", "running_var") and isinstance(m, nn.BatchNorm2d) else (-0.5, 0.5)
            t.data = put(U(tuple(t.shape), seed + k, lo, hi))
            k += 1
        for n, bf in m.named_buffers():
            if not bf.dtype.is_floating_point:
                m._buffers[n] = bf.to(DEV)
    return mods


for _cin, _cout, _stride in ((16, 24, 2), (24, 24, 1)):
    @row(f"ir_block[stride {_stride}]", ["as_ir_block_pack", "as_ir_block"], f"x (2,{_cin},9,14) -> {_cout}, expansion 6" + (", residual" if _stride == 1 else ""),
         note="the pack image is returned too")
    def _(put, cin=_cin, cout=_cout, stride=_stride):
        from anystereo import ops
        with torch.no_grad():
            pk = ops.IrBlockPack().get(*_ir_modules(put, cin, 6 * cin, cout, 130))
            return ops.ir_block(put(U((2, cin, 9, 14), 129)), pk, stride, stride == 1 and cin == cout), pk.pack


@row("conv7x7_c3", ["as_conv7x7_c3_pack", "as_conv7x7_c3"], "x (2,3,9,17), the encoders' stem; the pack image is returned too")
def _(put):
    from anystereo import _lib as Lb, ops
    pk = ops.Stem7x7Pack()
    out = ops.conv7x7_c3(put(U((2, 3, 9, 17), 140)), pk, put(U((64, 3, 7, 7), 141) * 0.1), put(U((64,), 142) * 0.1), act=Lb.ACT_RELU)
    return out, pk.wpack


@row("conv3x3_to1", ["as_conv3x3_to1"], "x (2,37,5,9)", precision="fp32")
def _(put):
    from anystereo import ops
    return ops.conv3x3_to1(put(U((2, 37, 5, 9), 143)), put(U((1, 37, 3, 3), 144) * 0.2), put(U((1,), 145)))


@row("tap_shift_sum", ["as_tap_shift_sum"], "s (2,18,5,9) with an addend")
def _(put):
    from anystereo import ops
    return ops.tap_shift_sum(put(U((2, 18, 5, 9), 146)), put(U((1,), 147)), put(U((2, 1, 5, 9), 148)))


@row("pool2x / interp", ["as_pool2x", "as_pool2x_bwd", "as_interp_bilinear_ac", "as_interp_bilinear_ac_bwd"], "x (2,5,7,10) and (2,5,7,9); interp to 14x19; forward and backward")
def _(put):
    from anystereo import grad as G
    outs = []
    for w in (10, 9):
        a = _leaf(put, U((2, 5, 7, w), 150))
        y = G.Pool2x.apply(a)
        y.backward(put(U(tuple(y.shape), 151)))
        a2 = _leaf(put, U((2, 5, 7, w), 152))
        z = G.InterpBilinear.apply(a2, 14, 19)
        z.backward(put(U(tuple(z.shape), 153)))
        outs += [y.detach(), a.grad, z.detach(), a2.grad]
    return outs


for _w, _kernel in ((14, "pool2x_bs_even_kernel (8-byte row loads)"), (15, "pool2x_bs_kernel")):
    @row(f"pool2x_bs / interp_bs[W {_w}]", ["as_pool2x_bs", "as_interp_bilinear_ac_bs"], f"x (2,13,9,{_w}): {_kernel}; 13 channels leave 3 padding slots")
    def _(put, w=_w):
        from anystereo import ops
        x = put(U((2, 13, 9, w), 343))
        return ops.pool2x_bs(x), ops.interp_bs(x, 18, 2 * w - 1)


@row("dwconv3x3", ["as_dwconv3x3", "as_dwconv3x3_s2_bwd_data", "as_dwconv3x3_wgrad"], "x (2,5,7,9): stride 2 with bias and residual; backward at stride 2 and 1", precision="fp32")
def _(put):
    from anystereo import _lib as Lb, grad as G, ops
    x, wt = put(U((2, 5, 7, 9), 160)), put(U((5, 1, 3, 3), 161))
    outs = [ops.dwconv3x3(x, wt, put(U((5,), 162)), stride=2, act=Lb.ACT_RELU6, residual=put(U((2, 5, 4, 5), 163)))]
    for stride in (2, 1):
        a, wl = _leaf(put, U((2, 5, 7, 9), 164)), _leaf(put, U((5, 1, 3, 3), 165))
        y = G.DwConv3x3.apply(a, wl, stride)
        y.backward(put(U(tuple(y.shape), 166)))
        outs += [y.detach(), a.grad, wl.grad]
    return outs


@row("dwconv3x3_wgrad[several slices]", ["as_dwconv3x3_wgrad"], "x (3,16,40,80) stride 1: the position range is cut into slices", precision="fp32")
def _(put):
    from anystereo import _lib as Lb, ops
    assert Lb.load().as_dwconv3x3_wgrad_slices(3, 16, 40, 80, 1) > 1, "this shape is meant to take the multi-slice path"
    return ops.dwconv3x3_wgrad(put(U((3, 16, 40, 80), 167)), put(U((3, 16, 40, 80), 168)), 1)


@row("conv3d_k3", ["as_conv3d_k3_gated", "as_conv3d_k3"], "x (2,5,2,3,9) -> 3: stride 1 gated, stride 2 plain, and the ungated symbol itself", precision="fp32",
     note="as_conv3d_k3 has no wrapper of its own (ops.conv3d_k3 calls the gated entry with a null gate): the row calls the symbol")
def _(put):
    from anystereo import _lib as Lb, ops
    b, cin, cout, d, h, w = 2, 5, 3, 2, 3, 9
    x, wp, bias = put(U((b, cin, d, h, w), 170)), put(U((cin, 27, cout), 171) * 0.2), put(U((cout,), 172))
    gated = ops.conv3d_k3(x, wp, bias, stride=1, act=Lb.ACT_LEAKY, gate=put(U((b, cout, h, w), 173, 0.0, 1.0)))
    s2 = ops.conv3d_k3(x, wp, None, stride=2)
    out = torch.empty((b, cout, d, h, w), device=DEV, dtype=torch.float32)
    Lb.check(Lb.load().as_conv3d_k3(_p(x), _p(wp), _p(bias), _p(out), b, cin, cout, d, h, w, 1, Lb.ACT_RELU, _stream()), "conv3d_k3")
    return gated, s2, out


@row("deconv3d_k4s2", ["as_deconv3d_k4s2"], "x (2,5,2,3,9) -> 3", precision="fp32")
def _(put):
    from anystereo import _lib as Lb, ops
    return ops.deconv3d_k4s2(put(U((2, 5, 2, 3, 9), 174)), put(U((5, 4, 4, 4, 3), 175) * 0.2), put(U((3,), 176)), act=Lb.ACT_RELU)


@row("instance_norm_act", ["as_instance_norm_act"], "x (2,5,37,50) with and without a residual; a 5-D volume (2,3,4,5,7)")
def _(put):
    from anystereo import _lib as Lb, ops
    x = put(U((2, 5, 37, 50), 180))
    return (ops.instance_norm_act(x, act=Lb.ACT_RELU), ops.instance_norm_act(x, act=Lb.ACT_NONE, residual=put(U((2, 5, 37, 50), 181))),
            ops.instance_norm_act(put(U((2, 3, 4, 5, 7), 182)), act=Lb.ACT_LEAKY))


@row("layernorm2d_act", ["as_layernorm2d_act"], "x (2,13,5,9)")
def _(put):
    from anystereo import _lib as Lb, ops
    return ops.layernorm2d_act(put(U((2, 13, 5, 9), 183)), put(U((13,), 184, 0.5, 1.5)), put(U((13,), 185)), act=Lb.ACT_GELU)


for _name, _b, _cin, _cout, _h, _w, _k, _what in (("one range", 2, 7, 5, 3, 5, 1, "nsplit 1, scalar fetch (W % 4 != 0)"),
                                                   ("split-K", 2, 7, 5, 9, 20, 3, "nsplit 4, 16-byte fetch"),
                                                   ("split-K, tiles", 3, 40, 130, 6, 16, 3, "nsplit 4, two Cout tiles and two Cin tiles")):
    @row(f"conv2d_wgrad[{_name}]", ["as_conv2d_wgrad_multi", "as_conv2d_wgrad"], f"x ({_b},{_cin},{_h},{_w}) dy {_cout} channels, k {_k}: {_what}; "
         "stacked, as a list of per-image pairs, and through the single-tensor symbol",
         note="as_conv2d_wgrad has no wrapper of its own (ops.conv2d_wgrad calls the multi entry): the row calls the symbol")
    def _(put, b=_b, cin=_cin, cout=_cout, h=_h, w=_w, k=_k):
        from anystereo import _lib as Lb, ops
        x, dy = U((b, cin, h, w), 530), U((b, cout, h, w), 531)
        xd, dyd = put(x), put(dy)
        outs = [ops.conv2d_wgrad(xd, dyd, k), ops.conv2d_wgrad(xd, dyd, k, want_bias=False)[0],
                ops.conv2d_wgrad([put(t.contiguous()) for t in x.split(1)], [put(t.contiguous()) for t in dy.split(1)], k)]
        lib = Lb.load()
        nbytes = int(lib.as_conv2d_wgrad_ws_bytes(b, cin, cout, h, w, k))
        ws = torch.empty((nbytes + 3) // 4, device=DEV, dtype=torch.float32)
        dw, db = torch.empty((cout, cin, k, k), device=DEV), torch.empty((cout,), device=DEV)
        Lb.check(lib.as_conv2d_wgrad(_p(xd), _p(dyd), _p(dw), _p(db), b, cin, cout, h, w, k, _p(ws), nbytes, _stream()), "conv2d_wgrad")
        return outs, dw, db


@row("conv7x7_c1_wgrad", ["as_conv7x7_c1_wgrad_multi"], "three pairs x (2,1,9,14), dy 64 channels; one pair with 40 channels and no bias")
def _(put):
    from anystereo import ops
    xs, dys = [put(U((2, 1, 9, 14), 190 + i)) for i in range(3)], [put(U((2, 64, 9, 14), 194 + i)) for i in range(3)]
    return ops.conv7x7_c1_wgrad(xs, dys), ops.conv7x7_c1_wgrad(put(U((1, 1, 5, 33), 198)), put(U((1, 40, 5, 33), 199)), want_bias=False)[0]


def _gates(put, with_holder):
    from anystereo import grad as G
    b, c, h, w = 2, 13, 5, 9
    base = put(U((b, 3 * c + 2, h, w), 200))
    hid = _leaf(put, torch.tanh(U((b, c, h, w), 201, -2, 2)))
    lin = _leaf(put, U((b, 2 * c, h, w), 202))
    holder = {} if with_holder else None
    z, rh = G.GruGatesZR.apply(lin, base[:, 1:1 + c], base[:, 1 + c:1 + 2 * c], hid, base, 1, holder)
    linq = _leaf(put, U((b, c, h, w), 203))
    out = G.GruGatesQ.apply(linq, base[:, 1 + 2 * c:1 + 3 * c], z, hid, base, 1 + 2 * c, holder)
    torch.autograd.backward([out, rh], [put(U((b, c, h, w), 204)), put(U((b, c, h, w), 205))])
    return z.detach(), rh.detach(), out.detach(), lin.grad, linq.grad, hid.grad, None if holder is None else holder["acc"]


row("gru_gates", ["as_gru_gates_zr", "as_gru_gates_q", "as_gru_gates_zr_bwd", "as_gru_gates_q_bwd"],
    "h (2,13,5,9), context of 41 channels at offset 1; forward and backward")(lambda put: _gates(put, False))
row("gru_gates[context accumulator]", ["as_gru_gates_zr", "as_gru_gates_q", "as_gru_gates_zr_bwd_ctx", "as_gru_gates_q_bwd_ctx"],
    "as above, the context gradient added into one zero-filled accumulator (grad.ContextAnchor's holder)")(lambda put: _gates(put, True))


# ---- LIIF upsampler -----------------------------------------------------------------------------------------------------------

@row("structure_feature", ["as_structure_feature", "as_affinity_bwd"], "x (2,5,9,14): cat(x, affinity) forward; the live-map backward with and without x", precision="fp32")
def _(put):
    from anystereo import grad as G, ops
    outs = [ops.structure_feature(put(U((2, 5, 9, 14), 210)))]
    for with_x in (True, False):
        a = _leaf(put, U((2, 5, 9, 14), 211))
        y = G.StructureFeatureLive.apply(a, with_x, 3)
        y.backward(put(U(tuple(y.shape), 212)))
        outs += [y.detach(), a.grad]
    return outs


for _win in (3, 5, 7):
    @row(f"affinity_window[{_win}]", ["as_affinity_window", "as_affinity_window_bwd"], f"x (1,8,9,14), window {_win}: with and without x, forward and backward", precision="fp32")
    def _(put, win=_win):
        from anystereo import ops
        outs = []
        for with_x in (True, False):
            x = put(U((1, 8, 9, 14), 213))
            out = ops.affinity_window(x, win, with_x)
            outs += [out, ops.affinity_window_backward(x, out, put(U(tuple(out.shape), 214)), win, with_x)]
        return outs


@row("liif_gather", ["as_liif_gather"], "feat (2,13,6,10), scale 2.95 grid, into channels [3, 18) of a 20-channel latent",
     note="ops.liif_gather fills a channel window of the caller's tensor: the row zero-fills the latent first and returns all of it")
def _(put):
    from anystereo import ops
    coord = put(_coords(2, 6, 10, 2.95, 220))
    lat = torch.zeros((2, 20, coord.shape[1]), device=DEV)
    ops.liif_gather(put(U((2, 13, 6, 10), 221)), coord, lat, 3)
    return lat


@row("liif_gather_mlp1 / rel_key", ["as_liif_gather_mlp1", "as_liif_rel_key"], "u0 (2,24,5,9), u1 (2,24,10,18), 700 random queries; one source; rel and sort key")
def _(put):
    from anystereo import ops
    coord = put(_coords(2, 5, 9, 2.0, 470, nq=700))
    u0, u1 = put(U((2, 24, 5, 9), 471)), put(U((2, 24, 10, 18), 472))
    two = ops.liif_gather_mlp1(u0, u1, coord, put(U((24, 4), 473)), put(U((24,), 474)))
    one = ops.liif_gather_mlp1(u0, None, coord, put(U((24, 2), 475)), None)
    return two, one, ops.liif_rel_key(coord, [(5, 9), (10, 18)], want_rel=True, want_key=True), ops.liif_rel_key(coord, [(5, 9)])[0]


@row("liif_scatter_add[atomics]", ["as_liif_gather_bwd"], "d_rows (2,26,Q) channels [1,25) onto (6,10), scale 1.5 grid", tol=T_GATHER_BWD, precision="fp32")
def _(put):
    from anystereo import ops
    assert not ops.get_deterministic()
    coord = put(_coords(2, 6, 10, 1.5, 0))
    return ops.liif_scatter_add(put(U((2, 26, coord.shape[1]), 451)), coord, 24, 6, 10, coff=1)


@row("liif_scatter_add[deterministic]", ["as_liif_gather_bwd_det", "as_liif_rel_key"], "as above in the gather form over sorted queries", precision="fp32")
def _(put):
    from anystereo import ops
    coord = put(_coords(2, 6, 10, 1.5, 0))
    ops.set_deterministic(True)
    try:
        return ops.liif_scatter_add(put(U((2, 26, coord.shape[1]), 451)), coord, 24, 6, 10, coff=1)
    finally:
        ops.set_deterministic(False)


@row("convex_upsample", ["as_convex_upsample", "as_convex_upsample_bwd"], "disp (2,1,6,10), scale 2.95 grid, logits + per-sample scale; forward and backward",
     tol={2: T_CONVEX_BWD}, precision="fp32", note="d_mask is written per query (bit-equal); d_disp is scattered with float atomics")
def _(put):
    from anystereo import grad as G
    coord = put(_coords(2, 6, 10, 2.95, 0))
    q = coord.shape[1]
    disp, logits = _leaf(put, U((2, 1, 6, 10), 452, 0, 30)), _leaf(put, U((2, 9, q), 453, -3, 3))
    out = G.ConvexUpsample.apply(disp, logits, coord, put(torch.tensor([2.95, 2.475])), True)
    out.backward(put(U((2, 1, q), 454)))
    return out.detach(), logits.grad, disp.grad


@row("convex_upsample_quater", ["as_convex_upsample_quater", "as_convex_upsample_quater_bwd"], "disp (2,1,5,7), scale 1.5 grid; forward and backward",
     tol={2: T_VARIANTS}, precision="fp32", note="d_mask is written per query (bit-equal); d_disp is scattered with float atomics")
def _(put):
    from anystereo import grad as G
    coord = put(_coords(2, 5, 7, 1.5, 0))
    q = coord.shape[1]
    disp, mask = _leaf(put, U((2, 1, 5, 7), 78, 0, 30)), _leaf(put, U((2, 4, q), 79, -2, 2))
    out = G.ConvexUpsampleQuater.apply(disp, mask, coord, put(torch.tensor([1.5, 1.25])), True)
    out.backward(put(U((2, 1, q), 77)))
    return out.detach(), mask.grad, disp.grad


for _unfold9, _nsamp in ((False, 1), (True, 1), (False, 4)):
    @row(f"liif_latent[unfold9={_unfold9}, n_samp={_nsamp}]", ["as_liif_latent", "as_liif_latent_bwd"], "feat (2,12,5,7), scale 1.5 grid, 3 learned frequencies and cells; forward and backward",
         tol={1: T_VARIANTS}, precision="fp32", note="the latent is written per query (bit-equal); d_feat is scattered with float atomics")
    def _(put, unfold9=_unfold9, nsamp=_nsamp):
        from anystereo import grad as G
        coord = put(_coords(2, 5, 7, 1.5, 0))
        feat = _leaf(put, U((2, 12, 5, 7), 77))
        lat = G.LiifLatent.apply(feat, coord, put(U((3, 2), 76, 0.0, 6.0)), put(torch.full((2, coord.shape[1], 2), 2 / 1.5)), unfold9, nsamp)
        lat.backward(put(U(tuple(lat.shape), 75)))
        return lat.detach(), feat.grad


def _liif_module(put, two, seed):
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn.liif import liif_out_multi_scale_Training
    up = liif_out_multi_scale_Training(encoder_dim=208 if two else 176, mlphidden_list=[128, 64, 64], pos_dim=0, unfold="with_v2ISU",
                                       affinity_settings={"win_w": 3, "win_h": 3, "dilation": [1, 2, 4, 8]},
                                       number_input=2 if two else 1, chanels=[176, 32] if two else [176]).eval()
    fill_module_deterministic(up, base_seed=seed, gain=2.0)
    for p_ in up.parameters():
        p_.data = put(p_.data)
    for n, bf in list(up.named_buffers()):
        bf.data = put(bf.data) if bf.dtype.is_floating_point else bf.data.to(DEV)
    return up


for _two, _b, _h, _w, _s, _nq, _direct in ((True, 2, 9, 14, 1.5, None, False), (False, 1, 7, 11, 2.95, None, False), (True, 3, 5, 9, 2.0, 33, False),
                                           (True, 2, 9, 13, 2.95, 777, True)):
    _syms = ["as_liif_affinity", "as_liif_lowres_pack", "as_liif_lowres_cl", "as_liif_tail_pack", "as_liif_query_rows"]
    _syms += ["as_liif_rows_cl", "as_liif_tail_direct"] if _direct else ["as_liif_tail"]
    @row(f"liif fused pipeline[{'two' if _two else 'one'} inputs, b {_b}, {_h}x{_w}, x{_s}{', direct second input' if _direct else ''}]", _syms,
         f"x4 ({_b},176,{_h},{_w})" + (f", x2 ({_b},32,{2 * _h},{2 * _w})" if _two else "") + f", {'the raster' if _nq is None else str(_nq) + ' random queries'} at scale {_s}",
         note="a fresh module (fresh lowres / tail packs) per run; disparity, mask logits, the clamped coordinates and the pack images are compared")
    def _(put, two=_two, b=_b, h=_h, w=_w, s=_s, nq=_nq, direct=_direct):
        up = _liif_module(put, two, 11)
        if direct:
            up.direct_second_input = True
        x4a, x4b = put(U((b, 176, h, w), 201, -1.5, 1.5)[:, :48].contiguous()), put(U((b, 176, h, w), 201, -1.5, 1.5)[:, 48:].contiguous())
        parts = [[x4a, x4b]] + ([[put(U((b, 32, 2 * h, 2 * w), 202, -1.5, 1.5))]] if two else [])
        coord = put(_coords(b, h, w, s, 203, nq))
        with torch.no_grad():
            out, logits = up.upsample_fused(parts, coord, put(U((b, 1, h, w), 204, 0.0, 40.0)), put(torch.full((b,), float(s))), want_logits=True)
        images = [pk.image for pk in up._lowres_packs if pk.image is not None] + [up._tail_pack.image]
        return out, logits, coord, images


@row("liif_lowres_cl", ["as_liif_lowres_pack", "as_liif_lowres_cl", "as_liif_rows_cl", "as_liif_affinity"], "three sources (48,128,8) at (2,7,13), K 184; two sources (32,8) at (1,14,26) with a column offset; rows of (32,8)")
def _(put):
    from anystereo import ops
    wt = put(U((128, 228), 215) * 0.2)
    srcs = [put(U((2, c, 7, 13), 210 + i)) for i, c in enumerate((48, 128, 8))]
    pk = ops.LiifLowresPack().get(wt, 0, 184)
    a = ops.liif_lowres_cl(srcs, pk)
    srcs2 = [put(U((1, c, 14, 26), 220 + i)) for i, c in enumerate((32, 8))]
    pk2 = ops.LiifLowresPack().get(wt, 186, 40)
    return a, pk.image, ops.liif_lowres_cl(srcs2, pk2), pk2.image, ops.liif_rows_cl(srcs2), ops.liif_affinity(srcs), ops.liif_affinity(srcs2[:1])


class _Lin:  # what LiifTailPack.get reads of an nn.Linear
    def __init__(self, w_, b_):
        self.weight, self.bias = w_, b_


def _mlp_tail(put, fuse_first):
    from anystereo import grad as G, ops
    n, b1, h0, w0 = 3, 2, 6, 10
    nb = n * b1
    from anystereo.nn.liif import make_coord
    grid = make_coord([8 * h0, 8 * w0])
    idx = (U((nb, 900), 880, 0.0, 1.0) * grid.shape[0]).long().clamp(max=grid.shape[0] - 1)
    coord = torch.stack([grid[i] for i in idx]).contiguous()
    coord[0, 0] = torch.tensor([-1.0, 1.0])
    coord[1, 5] = torch.tensor([1.0, -1.0])
    shapes = ((nb, 128, h0, w0), (b1, 128, 2 * h0, 2 * w0), (128, 4), (128,), (64, 128), (64,), (64, 64), (64,), (9, 64), (9,))
    lims = (1, 1, 1, 1, 0.15, 1, 0.2, 1, 0.2, 1)
    leaves = [_leaf(put, U(s, 881 + i, -m, m)) for i, (s, m) in enumerate(zip(shapes, lims))]
    w1full = put(leaves[2].detach().cpu())
    lin = [_Lin(w1full, leaves[3]), _Lin(leaves[4], leaves[5]), _Lin(leaves[6], leaves[7]), _Lin(leaves[8], leaves[9])]
    pack, pack_t = ops.LiifTailPack().get(lin, [0, 2]), ops.LiifMlpBwdPack()
    prev, G._LIIF_FUSE_FIRST = G._LIIF_FUSE_FIRST, fuse_first
    try:
        out = G.LiifMlpTail.apply(leaves[0], leaves[1], put(coord), leaves[2], leaves[3], *leaves[4:], pack, pack_t, None)
        out.backward(put(U((nb, 9, 900), 891) * 1e-3))
    finally:
        G._LIIF_FUSE_FIRST = prev
    return [out.detach(), pack.image, pack_t.image] + [t.grad for t in leaves]


row("liif_mlp_tail[layered first layer]", ["as_liif_mlp_fwd", "as_liif_mlp_bwd", "as_liif_mlp_bwd_pack", "as_liif_tail_pack", "as_liif_gather_bwd"],
    "u0 (6,128,6,10), u1 (2,128,12,20) shared by 3 evaluations, 900 random queries (test_liif_mlp_tail_function_vs_fp64's case)",
    tol={3: T_GATHER_BWD, 4: T_GATHER_BWD, 6: T_GATHER_BWD},
    note="logits, the pack images, d_wrel and the later layers' gradients bit-equal; d_u0, d_u1 come from as_liif_gather_bwd's atomics, d_b1 "
         "is a reduction of d_u0")(lambda put: _mlp_tail(put, False))
row("liif_mlp_tail[fused first layer]", ["as_liif_mlp_fwd", "as_liif_mlp_bwd", "as_liif_mlp_bwd_pack", "as_liif_tail_pack"],
    "as above, the first layer's scatter-adds and the wrel reduction inside the backward kernel",
    tol={3: T_MLP_BWD, 4: T_MLP_BWD, 5: T_MLP_BWD, 6: T_MLP_BWD},
    note="d_u0, d_u1, d_wrel are accumulated with float atomics inside as_liif_mlp_bwd, d_b1 is a reduction of d_u0; everything else bit-equal")(
        lambda put: _mlp_tail(put, True))


# ---- evaluation and training batches ---------------------------------------------------------------------------------------------

@row("disparity_metrics / lr_consistency", ["as_disp_metrics", "as_lr_consistency"], "3 estimates of (2,37,53) with both masks; one estimate without masks")
def _(put):
    from anystereo import ops
    gt = put(U((2, 37, 53), 230, -5.0, 60.0))
    est = put(U((3, 2, 37, 53), 231, 0.0, 60.0))
    valid, noc = put((U((2, 37, 53), 232) > -0.6).to(torch.uint8)), put(U((2, 37, 53), 233) > 0.0)
    return (ops.disparity_metrics(est, gt, valid, noc, gt_lo=0.0, gt_hi=50.0), ops.disparity_metrics(est[0], gt),
            ops.lr_consistency(put(U((2, 37, 53), 234, 0.0, 20.0)), put(U((2, 37, 53), 235, 0.0, 20.0))))


@row("disparity_images", ["as_disp_images"], "disp, gt (2,37,53): all three pictures; (1,5,7) colour only (B*H*W % 4 != 0)")
def _(put):
    from anystereo import ops
    d, g = put(U((2, 37, 53), 236, 0.0, 200.0)), put(U((2, 37, 53), 237, -5.0, 200.0))
    return ops.disparity_images(d, g, enc16=True), ops.disparity_images(put(U((1, 5, 7), 238, 0.0, 200.0)))


@row("prepare_pair / query_grid / resize_disparity", ["as_prepare_pair", "as_query_grid", "as_resize_disp"], "uint8 pair (2,3,37,53) x1.5 /32 and fixed x3 /16; its grids; a (2,19,27) crop resized to 37x53")
def _(put):
    from anystereo import ops
    from anystereo.harness.query import query_plan
    u1, u2 = put((U((2, 3, 37, 53), 240, 0.0, 255.99)).to(torch.uint8)), put((U((2, 3, 37, 53), 241, 0.0, 255.99)).to(torch.uint8))
    outs = []
    for pl in (query_plan(37, 53, 1.5, 32), query_plan(37, 53, 3, 16, fixed=True)):
        outs += [ops.prepare_pair(u1, u2, pl), ops.query_grid(pl, 2, DEV)]
    outs.append(ops.prepare_pair(put(U((1, 3, 37, 53), 242, 0.0, 255.0)), put(U((1, 3, 37, 53), 243, 0.0, 255.0)), query_plan(37, 53, 2.95, 32)))
    outs.append(ops.resize_disparity(put(U((2, 24, 32), 244, 0.0, 60.0)), (3, 2, 19, 27), (37, 53), mul=1.5))
    return outs


_TQ_MODES = ("dense", "dense_all", "sparse", "sparse_ordered")


@row("train_queries / low_disp", ["as_train_queries", "as_low_disp"], "crops (33,47), (40,29), (17,64), Q 66, every mode with scales (dense_all on two 6x11 crops); low_disp to (17,70) and (2,3)",
     note="index and n_valid are int32 (guards only), the sparse modes' cached uint8 scratch gets guards only and is dropped before every "
          "run so that the run allocates it; hr_coord / hr_disp / scale are poisoned; the second crop has fewer valid pixels than Q")
def _(put):
    from anystereo import ops
    ops._train_ws.clear()
    try:
        crops = []
        for i, (h, w) in enumerate(((33, 47), (40, 29), (17, 64))):
            d = U((h, w), 250 + i, 0.0, 60.0)
            d[U((h, w), 260 + i) > (-0.95 if i == 1 else 0.3)] = 0.0  # invalid pixels (the sparse modes list the valid ones); crop 1: V < Q
            crops.append(put(d))
        outs = [ops.train_queries(crops, 66, m, 1234, scales=[1.0, 1.5, 2.95]) for m in _TQ_MODES if m != "dense_all"]
        outs.append(ops.train_queries([put(U((6, 11), 270 + i, 0.5, 60.0)) for i in range(2)], 66, "dense_all", 1234))  # needs Q == N
        outs.append(ops.train_queries(crops, 96, "dense", 7))
        return outs, ops.low_disp(crops, [1.0, 1.5, 2.95], (17, 70)), ops.low_disp(crops, [1.0, 1.5, 2.95], (2, 3))
    finally:
        ops._train_ws.clear()


@row("stamp", ["as_stamp"], "two markers into an 8-slot int64 buffer",
     note="the slots receive the device clock: compared are which slots are non-zero, and the slots no marker names")
def _(put):
    from anystereo import ops
    st = ops.Stamps(DEV, slots=8)
    st.buf = put(torch.zeros(8, dtype=torch.int64))
    st.mark("a"), st.mark("b")
    return (st.buf != 0).to(torch.uint8), st.buf[2:]


CONV_TABLE_SYMBOLS = {"as_conv2d", "as_conv_pack_weights", "as_conv_pack_weights_split", "as_tap_shift_sum"}  # what test_conv2d_table calls
ROW_SYMBOLS = {s for r in ROWS for s in r.symbols} | CONV_TABLE_SYMBOLS


# ---- the harness of the table ----------------------------------------------------------------------------------------------------

CALLS = {}      # symbol -> calls made while a guarded context was active
_RESULTS = {}   # row name -> "passed" | "FAILED"
_CONV_RESULTS = {}  # fill pattern -> "passed" | "FAILED" of the conv2d table


@pytest.fixture(scope="module", autouse=True)
def _counted_library():
    """Wrap every function of the loaded library with a counter for the duration of the module; write the profile at teardown."""
    try:
        with GD.counted(_lib(), CALLS):
            yield
    finally:
        _write_profile()


def _mode(r):
    if r.tol is None:
        return "bit-equal", []
    tols = [r.tol] if isinstance(r.tol, tuple) else list(r.tol.values())
    what = "tolerance" if isinstance(r.tol, tuple) else "bit-equal but results %s: tolerance" % sorted(r.tol)
    return what, sorted({"%s of %s" % (t[1], t[2]) for t in tols})


def _write_profile():
    L = _lib()
    if len([r for r in ROWS if r.name in _RESULTS]) < len(ROWS) or "conv2d table" not in _RESULTS:
        return  # a selection of the table (-k): the file describes whole runs only
    lines = ["memory hygiene: every launching symbol under guarded(0xFF) and guarded(0x47) with placed inputs (tests/test_memory_hygiene_gpu.py)",
             "", "ROWS  (name | precision | compare mode | result; shape; note; for a tolerance row the parity test it takes the tolerance from)"]
    for r in ROWS:
        mode, cites = _mode(r)
        lines.append("%s | %s | %s | %s" % (r.name, r.precision, mode, _RESULTS.get(r.name, "not run")))
        lines.append("    " + r.shape)
        lines += ["    note: " + r.note] if r.note else []
        lines += ["    " + c for c in cites]
    lines.append("conv2d table | per case | check_case's bounds (test_conv_instantiations_gpu.py: 1e-5, RELU_TAPS 2e-5) + guards | %s (%s)" % (
        _RESULTS.get("conv2d table", "not run"), ", ".join("0x%02X %s" % (p_, _CONV_RESULTS.get(p_, "not run")) for p_ in GD.PATTERNS)))
    lines.append("    %d cases of tests/_conv_cases.py under both fills: every one whose plan splits K or has a finish kernel, one per remaining (family, epilogue)" % len(CONV_CASES))
    lines += ["    " + c["name"] + "  B %d %dx%d srcs %s Cout %d" % (c["B"], c["H"], c["W"], c["srcs"], c["Cout"]) for c in CONV_CASES]
    lines += ["", "SYMBOLS  (calls made under a guard in this run: rows)"]
    for name in L.SIGNATURES:
        if name not in EXEMPT:
            rows = [r.name for r in ROWS if name in r.symbols] + (["conv2d table"] if name in CONV_TABLE_SYMBOLS else [])
            lines.append("%-32s %4d: %s" % (name, CALLS.get(name, 0), "; ".join(rows)))
    lines += ["", "EXEMPT"] + ["%-34s %s" % kv for kv in sorted(EXEMPT.items())]
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "memory_hygiene.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass  # a read-only checkout: the table has still run


def _close(limit):
    def compare(a, b, what):
        a, b = a.double(), b.double()
        err, lim = (a - b).abs().max().item(), limit(b.abs().max().item())
        assert err <= lim, f"{what}: max abs difference from the plain run {err:.3e} > {lim:.3e}"
    return compare


def _compare_of(r):
    if r.tol is None:
        return None
    if isinstance(r.tol, tuple):
        return _close(r.tol[0])
    by_index = {i: _close(t[0]) for i, t in r.tol.items()}

    def compare(a, b, what):
        i = int(what.split("result ")[1].split(" ")[0])
        if i in by_index:
            return by_index[i](a, b, what)
        assert torch.equal(a, b), f"{what} differs from the plain run in {int((a != b).sum())} of {a.numel()} elements: the op read memory nobody wrote"
    return compare


def _stop_after_a_fault(e, where):
    """A device fault poisons the process: end the run there instead of starting the remaining rows on a faulted device."""
    if any(k in str(e) for k in ("illegal memory access", "HIP error", "hipError", "unspecified launch failure")):
        pytest.exit(f"device fault in {where}: {e}", returncode=3)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_row(name):
    from anystereo import ops
    r = next(r for r in ROWS if r.name == name)
    prev = ops.get_precision()
    ops.set_precision(r.precision)
    _RESULTS[name] = "FAILED"
    try:
        hygiene(r.fn, DEV, compare=_compare_of(r))
    except RuntimeError as e:
        _stop_after_a_fault(e, name)
        raise
    finally:
        ops.set_precision(prev)
    _RESULTS[name] = "passed"


# ---- conv2d: the table of tests/_conv_cases.py ------------------------------------------------------------------------------------

def _conv_selection():
    """Every case whose plan (under the knobs of this process: the defaults) splits K or has a finish kernel, plus the cheapest case
    of every remaining (family, epilogue) pair."""
    picked, rest = [], {}
    for c in cc.CASES:
        p = cc.plan(dict(c, knobs={}))
        if p["ksplit"] > 1 or p["finish"]:
            picked.append(c)
        else:
            key, cost = (p["family"], c["epi"]), c["B"] * c["H"] * c["W"] * c["Cout"]
            if key not in rest or cost < rest[key][0]:
                rest[key] = (cost, c)
    return picked + [c for _, c in rest.values()]


try:
    CONV_CASES = _conv_selection()
except Exception:  # no built library (collection on a box without one): the GPU tests cannot run there anyway
    CONV_CASES = []


@pytest.mark.parametrize("pattern", GD.PATTERNS, ids=["nan", "finite"])
def test_conv2d_table(pattern):
    """The selected cases of the conv2d table with placed operands under one fill: check_case unchanged (its bounds and the fills
    around the windows) plus the guards — the split-K workspace and the packed weight images are poisoned."""
    assert CONV_CASES
    _CONV_RESULTS[pattern] = "FAILED"
    _RESULTS["conv2d table"] = "FAILED"
    failed = []
    for c in CONV_CASES:
        o, want = cc.operands(c), None
        try:
            with GD.guarded(pattern) as g:
                got = cc.run_case(c, o, DEV, put=lambda t: GD.place(t, DEV))
                g.check()
        except RuntimeError as e:
            _stop_after_a_fault(e, c["name"])
            raise
        want = cc.expected(c, o)
        try:
            cc.check_case(c, got, want, 2e-5 if c["epi"] == cc.TAPS else 1e-5)  # test_conv_instantiations_gpu.py's RTOL_TAPS / RTOL
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "\n".join(failed)
    _CONV_RESULTS[pattern] = "passed"
    if all(_CONV_RESULTS.get(p_) == "passed" for p_ in GD.PATTERNS):
        _RESULTS["conv2d table"] = "passed"


# ---- pointer-alignment branches ------------------------------------------------------------------------------------------------------
# torch allocations are 512-B aligned, so the branch an entry takes for a pointer off its boundary (a contiguous batch slice of an
# odd-sized tensor in real use) never runs elsewhere in the suite but for eval_metrics / eval_images, which have tests of their own
# (test_eval_images_gpu.py::test_inputs_off_the_16_byte_boundary_give_the_same_bytes, test_eval_metrics_gpu.py).  Inputs are placed
# 4 bytes past a 16-B boundary; a buffer the wrapper allocates itself is moved by the allocator (guarded(skew_sites=...)).

def _skewed_equals_aligned(fn, reference, skew_sites=None):
    """fn(put) aligned and plain, then under both fills with every input 4 bytes off: guards intact, finite, the same bits as the
    aligned run (the kernels differ in how they fetch, not in what they add up in which order), and reference(result) holds."""
    aligned = [t.clone() for t in GD.flatten(fn(lambda t: GD.place(t, DEV)))]
    reference(aligned)
    for pattern in GD.PATTERNS:
        with GD.guarded(pattern, skew_sites=skew_sites) as g:
            got = [t.clone() for t in GD.flatten(fn(lambda t: GD.place(t, DEV, skew=4)))]
            g.check()
        for i, (a, b) in enumerate(zip(got, aligned)):
            assert not a.is_floating_point() or torch.isfinite(a).all(), (pattern, i)
            assert torch.equal(a, b), f"fill 0x{pattern:02X}: result {i} off the boundary differs from the aligned run in {int((a != b).sum())} elements"
        reference(got)


def test_pool2x_bs_off_the_8_byte_boundary():
    """W even and x off its 8-byte boundary: pool2x_bs_kernel instead of pool2x_bs_even_kernel.  Reference and bound of
    test_resamplers_blocked_split_output: exactly the split of the fp32 kernel's values, padding slots zero."""
    from anystereo import ops
    x = U((2, 13, 9, 14), 343)
    ref = ops.pool2x(x.to(DEV))
    hi = ref.half()
    lo = ((ref - hi.float()) * 2048.0).half()

    def reference(res):
        t = res[0]
        b, _, c8, h, w, _ = t.shape
        got_hi = t[:, 0].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w)
        got_lo = t[:, 1].permute(0, 1, 4, 2, 3).reshape(b, c8 * 8, h, w)
        assert torch.equal(got_hi[:, :13], hi) and torch.equal(got_lo[:, :13], lo)
        assert (got_hi[:, 13:] == 0).all() and (got_lo[:, 13:] == 0).all()
    _skewed_equals_aligned(lambda put: ops.pool2x_bs(put(x)), reference)


@pytest.mark.parametrize("form", ["stacked", "list", "symbol"])
def test_conv2d_wgrad_off_the_16_byte_boundary(form):
    """W % 4 == 0 and x / dy off their 16-byte boundary: the scalar fetch instead of the 16-byte one (wgrad_run), through
    as_conv2d_wgrad_multi with one tensor pair and with a list of pairs, and through as_conv2d_wgrad itself (no wrapper of its
    own).  Reference and bounds of test_conv2d_wgrad."""
    import torch.nn.functional as F
    from anystereo import ops
    b, cin, cout, h, w, k = 2, 7, 5, 9, 20, 3
    x, dy = U((b, cin, h, w), 530), U((b, cout, h, w), 531)
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), wt, bias, padding=k // 2).backward(dy.double())
    lim = 4e-5 * (b * h * w) ** 0.5

    def reference(res):
        dw, db = res[0].double().cpu(), res[1].double().cpu()
        assert (dw - wt.grad).abs().max().item() <= lim and (db - bias.grad).abs().max().item() <= lim
        assert (dw - wt.grad).norm() / wt.grad.norm() < 2e-5

    def fn(put):
        if form == "stacked":
            return ops.conv2d_wgrad(put(x), put(dy), k)
        if form == "list":
            return ops.conv2d_wgrad([put(t.contiguous()) for t in x.split(1)], [put(t.contiguous()) for t in dy.split(1)], k)
        Lb = _lib()
        lib, xd, dyd = Lb.load(), put(x), put(dy)
        nbytes = int(lib.as_conv2d_wgrad_ws_bytes(b, cin, cout, h, w, k))
        ws = torch.empty((nbytes + 3) // 4, device=DEV, dtype=torch.float32)
        dw, db = torch.empty((cout, cin, k, k), device=DEV), torch.empty((cout,), device=DEV)
        Lb.check(lib.as_conv2d_wgrad(_p(xd), _p(dyd), _p(dw), _p(db), b, cin, cout, h, w, k, _p(ws), nbytes, _stream()), "conv2d_wgrad")
        return dw, db
    _skewed_equals_aligned(fn, reference)


def test_query_grid_off_the_16_byte_boundary():
    """hr_coord 8 bytes past a 16-B boundary (the entry refuses 4): 8-byte stores instead of the shifted 16-byte pairs.  Reference of
    test_prepare_gpu.py::test_query_grid_equals_host_restatement: torch.equal to query_grid_host, crop branch and `resized` branch."""
    from anystereo import ops
    from anystereo.harness.query import query_grid_host, query_plan
    plans = [query_plan(37, 53, 1.5, 32), query_plan(40, 64, 1.0, 32)]
    want = [query_grid_host(pl, 2) for pl in plans]

    def reference(res):
        for got, w_ in zip(res, want):
            assert torch.equal(got.cpu(), w_)
    with GD.guarded(GD.NAN_FILL, skew_sites={("ops.py", "query_grid", torch.float32): 8}):
        assert ops.query_grid(plans[0], 2, DEV).data_ptr() % 16 == 8
    _skewed_equals_aligned(lambda put: [ops.query_grid(pl, 2, DEV) for pl in plans], reference,
                           skew_sites={("ops.py", "query_grid", torch.float32): 8})


def _refuse_lookup(which):
    def fn(put, skew):
        from anystereo import ops
        geo, corr, disp = _lookup_operands(put, 2, 3, 20, 8, 48, 2, seed=300)
        geo = [skew(t.cpu()) for t in geo]
        if which == "lookup_fwd":
            return lambda: ops.geo_corr_lookup(geo, corr, disp, 4)
        pack = ops.LookupConvPack().get(*_convc1_operands(put, 8, 2, 305))
        if which == "lookup_convc1":
            return lambda: ops.lookup_convc1(geo, corr, disp, 4, pack, want_f32=True)
        taps, hb = put(U((2, 18, 3, 20), 707) * 0.2), put(U((1,), 708))
        return lambda: ops.loop_front(geo, corr, taps, hb, disp, 4, pack, None, None)
    return fn


def _refuse_ir_block(put, skew):
    from anystereo import ops
    with torch.no_grad():
        pk = ops.IrBlockPack().get(*_ir_modules(put, 16, 96, 24, 130))
    pk.pack = skew(pk.pack.cpu())
    x = put(U((2, 16, 9, 14), 129))
    return lambda: ops.ir_block(x, pk, 2, False)


def _refuse_conv2d(what):
    def fn(put, skew):
        from anystereo import ops
        pk = ops.PackedConv().get([put(U((40, 32, 3, 3), 100) * 0.1)], [None])
        x = U((2, 32, 9, 14), 101)
        if what == "wpack":
            pk.wpack = skew(pk.wpack.cpu())
            src = put(x)
        else:
            src = ops.BS8(skew(cc.to_bs(x).t), 32)
        return lambda: ops.conv2d([src], pk)
    return fn


def _refuse_deconv3d(put, skew):
    from anystereo import ops
    x, wp = put(U((2, 5, 2, 3, 9), 174)), put(U((5, 4, 4, 4, 3), 175) * 0.2)
    return lambda: ops.deconv3d_k4s2(x, wp)


def _refuse_resampler(which):
    def fn(put, skew):
        from anystereo import ops
        x = put(U((2, 13, 9, 14), 343))
        return (lambda: ops.pool2x_bs(x)) if which == "pool2x_bs" else (lambda: ops.interp_bs(x, 18, 27))
    return fn


def _refuse_query_grid(put, skew):
    from anystereo import ops
    from anystereo.harness.query import query_plan
    return lambda: ops.query_grid(query_plan(37, 53, 1.5, 32), 2, DEV)


def _refuse_train_queries(put, skew):
    from anystereo import ops
    crops = [put(U((33, 47), 250, 0.5, 60.0))]
    return lambda: ops.train_queries(crops, 66, "dense", 7)


# name -> (build(put, skew) -> the refused call, the library's message, precision, allocation sites the allocator moves by 4 bytes)
REFUSALS = {
    "geo_corr_lookup: geo": (_refuse_lookup("lookup_fwd"), r"lookup_fwd: geo\[0\] not 16-B aligned", "split", None),
    "lookup_convc1: geo": (_refuse_lookup("lookup_convc1"), r"lookup_convc1: geo\[0\] not 16-B aligned", "split", None),
    "loop_front: geo": (_refuse_lookup("loop_front"), r"loop_front: geo\[0\] not 16-B aligned", "split", None),
    "ir_block: pack": (_refuse_ir_block, "ir_block: pack not 16-B aligned", "split", None),
    "conv2d: wpack": (_refuse_conv2d("wpack"), "conv2d: wpack not 16-B aligned", "split", None),
    "conv2d: blocked source": (_refuse_conv2d("source"), "conv2d: blocked source 0 not 16-B aligned", "split", None),
    "deconv3d_k4s2: out": (_refuse_deconv3d, "deconv3d_k4s2: out not 8-B aligned", "fp32", {("ops.py", "deconv3d_k4s2", torch.float32): 4}),
    "pool2x_bs: out_bs": (_refuse_resampler("pool2x_bs"), "pool2x_bs: out_bs not 16-B aligned", "split", {("ops.py", "empty", torch.float16): 4}),
    "interp_bs: out_bs": (_refuse_resampler("interp_bs"), "interp_bs: out_bs not 16-B aligned", "split", {("ops.py", "empty", torch.float16): 4}),
    "query_grid: hr_coord": (_refuse_query_grid, "query_grid: hr_coord is not 8-byte aligned", "split", {("ops.py", "query_grid", torch.float32): 4}),
    "train_queries: hr_coord": (_refuse_train_queries, "train_queries: hr_coord is not 8-byte aligned", "split",
                                {("ops.py", "train_queries", torch.float32): 4}),
}
# Not reachable through the operator layer, so without a case: instance norm's `ws` and disparity_metrics' partials are float64
# tensors (torch keeps a tensor aligned to its element size, the entries ask for 8 bytes); the lookup backward's d_geo comes from
# torch.zeros inside the wrapper.


@pytest.mark.parametrize("name", list(REFUSALS))
def test_misaligned_pointer_is_refused_and_nothing_is_launched(name):
    """A pointer off the alignment an entry demands: RuntimeError with the library's message, the guards intact, and every buffer
    the wrapper allocated for the call still poisoned in every byte — nothing was launched."""
    from anystereo import ops
    build, message, precision, sites = REFUSALS[name]
    prev = ops.get_precision()
    ops.set_precision(precision)
    try:
        for pattern in GD.PATTERNS:
            with GD.guarded(pattern, skew_sites=sites) as g:
                call = build(lambda t: GD.place(t, DEV), lambda t: GD.place(t, DEV, skew=4))
                since = len(g.buffers)
                with pytest.raises(RuntimeError, match=message):
                    call()
                g.check()
                assert g.nothing_written(since), f"{name}: an output or scratch buffer was written although the call was refused"
    finally:
        ops.set_precision(prev)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------

def test_every_launching_symbol_ran_under_a_guard():
    L = _lib()
    missing = [n for n in L.SIGNATURES if n not in EXEMPT and not CALLS.get(n)]
    assert not missing, f"never called under a guard: {missing}"
