"""GPU (-m gpu): the streaming 1x1 convolution (csrc/pointwise.hip, ops.conv1x1) computes BIT FOR BIT what ops.conv2d computes.

Each case runs ops.conv2d and the streaming entry on the same det_uniform operands, the output a channel window [4, 4 + Cout) of
a tensor pre-filled with 7.0, and requires torch.equal of the two tensors — results and fill alike — so no tolerance is chosen.
The shapes are the smallest at which the kernel can still go wrong:
  16->96, B 2, 9x37      plane of 333 floats: odd channels' planes are not 8-B aligned (dword accesses instead of 8-B ones), a pixel
                         tail inside a 32-pixel MFMA tile, the batch stride, three output tiles
  144->24, 1x8x40        nine chunks (off the four-chunk unit of conv_split_kernel and of the K sweep's groups), Cout off the
                         32-row tile, the accumulator-resident K sweep
  20->8, 1x5x33          bias, ReLU6 and `add`; the last chunk partly padding, Cout below one tile
  32+16->48              two sources, a residual `h`, an `out_coff` window
  96->96, 2x12x44        sigmoid (the FeatureAtt gate's form), several output tiles, six resident chunks
  128->72, 64->72, 48->136, 192->64   the remaining instantiations (eight, four and three resident chunks; two accumulator
                         tiles over three groups of the K sweep), tanh and LeakyReLU
  overflow               values >= 65504: equal results, and ops.split_overflow_count rises by the same amount on both paths
  rejected               a descriptor as_conv1x1_stream_ok rejects: an error, no launch, the fill intact."""
import ctypes as C

import pytest
import torch

from anystereo import _lib as L
from anystereo import ops
from anystereo.harness.synthetic import det_uniform as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FILL, COFF, CPAD = 7.0, 4, 8

# name -> (source channels, Cout, B, H, W, act, bias, add, residual)
CASES = {
    "16to96_odd_plane": ([16], 96, 2, 9, 37, L.ACT_NONE, False, False, False),
    "144to24_ksweep": ([144], 24, 1, 8, 40, L.ACT_RELU, True, False, False),
    "20to8_bias_relu6_add": ([20], 8, 1, 5, 33, L.ACT_RELU6, True, True, False),
    "32p16to48_two_sources_residual": ([32, 16], 48, 1, 7, 26, L.ACT_RELU, True, False, True),
    "96to96_sigmoid_gate": ([96], 96, 2, 12, 44, L.ACT_SIGMOID, True, False, False),
    "128to72_tanh_resident8": ([128], 72, 1, 6, 50, L.ACT_TANH, False, True, True),
    "64to72_resident4": ([64], 72, 1, 4, 35, L.ACT_NONE, True, False, False),
    "48to136_leaky": ([48], 136, 1, 3, 70, L.ACT_LEAKY, True, False, False),
    "192to64_ksweep_two_tiles": ([192], 64, 1, 10, 30, L.ACT_NONE, False, True, False),
}


@pytest.fixture(scope="module", autouse=True)
def _split_precision():
    prev = ops.get_precision()
    ops.set_precision("split")
    yield
    ops.set_precision(prev)


def _operands(name):
    srcs, cout, b, h, w, act, bias, add, res = CASES[name]
    seed = 9000 + 32 * list(CASES).index(name)
    cin = sum(srcs)
    o = {"x": [U((b, c, h, w), seed + j, -2, 2).to(DEV) for j, c in enumerate(srcs)],
         "w": (U((cout, cin, 1, 1), seed + 8) * (3.0 / cin) ** 0.5).to(DEV),
         "bias": (U((cout,), seed + 9) * 0.1).to(DEV) if bias else None,
         "add": U((b, cout + 3, h, w), seed + 10).to(DEV) if add else None,
         "h": torch.tanh(U((b, cout, h, w), seed + 11, -2, 2)).to(DEV) if res else None}
    return o


def _both(o, cout, act):
    """(conv2d's output tensor, the streaming kernel's) for the same operands, each a window of a 7.0-filled tensor."""
    b, _, h, w = o["x"][0].shape
    pack = ops.PackedConv().get([o["w"]], [o["bias"]])
    outs = []
    for fn in (ops.conv2d, lambda *a, **k: ops.conv1x1(*a, force=True, **k)):
        out = torch.full((b, cout + CPAD, h, w), FILL, device=DEV)
        fn(o["x"], pack, act=act, add=o["add"], add_coff=2 if o["add"] is not None else 0, out=out, out_coff=COFF, h=o["h"])
        outs.append(out)
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("name", list(CASES))
def test_stream_equals_conv2d_bit_for_bit(name):
    cout, act = CASES[name][1], CASES[name][5]
    want, got = _both(_operands(name), cout, act)
    assert bool((want[:, :COFF] == FILL).all()) and bool((want[:, COFF + cout:] == FILL).all())  # the yardstick itself
    assert torch.isfinite(want).all() and float(want[:, COFF:COFF + cout].abs().max()) > 0.05
    diff = (want != got)
    print("[pointwise] %-34s differing elements %d of %d" % (name, int(diff.sum()), diff.numel()))
    assert torch.equal(want, got), f"{name}: {int(diff.sum())} elements differ, first at {diff.nonzero()[:4].tolist()}"


def test_overflow_is_saturated_and_counted_alike():
    """One operand >= 65504 per batch element (one block of either kernel each, Cout <= 64: conv_split_kernel splits every source
    value once per launch, as the streaming kernel does): the saturated results are equal and both paths count two waves."""
    b, cin, cout, h, w = 2, 16, 32, 6, 40
    x = U((b, cin, h, w), 77, -2, 2)
    x[0, 3, 2, 5], x[1, 11, 4, 30] = 1.0e5, -7.0e4
    o = {"x": [x.to(DEV)], "w": (U((cout, cin, 1, 1), 78) * 0.4).to(DEV), "bias": None, "add": None, "h": None}
    pack = ops.PackedConv().get([o["w"]], [None])
    ops.split_overflow_count()  # reset
    want = ops.conv2d(o["x"], pack)
    n_conv = ops.split_overflow_count()
    got = ops.conv1x1(o["x"], pack, force=True)
    n_stream = ops.split_overflow_count()
    print(f"[pointwise] overflow waves counted: conv2d {n_conv}, streaming {n_stream}")
    assert torch.isfinite(want).all() and torch.equal(want, got)
    assert n_conv == 2 and n_stream == n_conv
    ops.conv1x1([U((b, cin, h, w), 79, -2, 2).to(DEV)], pack, force=True)
    assert ops.split_overflow_count() == 0, "in-range operands must not be counted"


def test_rejected_descriptor_is_an_error_and_launches_nothing():
    b, cin, cout, h, w = 1, 16, 32, 6, 40
    x = U((b, cin, h, w), 90).to(DEV)
    pack = ops.PackedConv().get([(U((cout, cin, 3, 3), 91) * 0.1).to(DEV)], [None])  # a 3x3 convolution
    out = torch.full((b, cout, h, w), FILL, device=DEV)
    d = L.ConvDesc()
    d.src[0], d.src_c[0], d.n_src = x.data_ptr(), cin, 1
    d.wpack, d.out, d.out_ctot = pack.wpack.data_ptr(), out.data_ptr(), cout
    d.B, d.H, d.W, d.Cin, d.Cout, d.KS = b, h, w, cin, cout, 3
    d.stride, d.act, d.epilogue, d.precision = 1, L.ACT_NONE, L.EPI_LINEAR, 1
    lib = L.load()
    assert lib.as_conv1x1_stream_ok(C.byref(d)) == 0
    rc = lib.as_conv1x1_stream(C.byref(d), ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"conv1x1_stream" in lib.as_last_error_string()
    assert bool((out == FILL).all())
    with pytest.raises(RuntimeError):
        ops.conv1x1([x], pack, force=True)
    assert torch.equal(ops.conv1x1([x], pack), ops.conv2d([x], pack))  # unforced: the planned kernel
