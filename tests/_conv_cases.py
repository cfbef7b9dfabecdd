"""One small convolution per instantiation of csrc/conv.hip (the 91 of tests/golden/conv_kernels.txt), and the runner that turns
such a case into an ops.conv2d call and its fp64 expectation (tests/test_conv_cases_cpu.py, tests/test_conv_instantiations_gpu.py,
tests/_conv_case_probe.py).

A case is named for the kernel the planner (as_conv2d_plan) selects for it and is written in the case(...) form of
tests/golden/make_golden_conv_plans.py plus a knob dict, so that file's descriptor() plans it.  The shapes were found by a search
over the planner's arithmetic alone (no device), and test_conv_cases_cpu.py holds every row to its name.  The rules of the search:
  * knobs: the default knobs wherever they reach the instantiation; {lean: 2} only for the rest (the LEAN kernels with NSUB = 1).
  * plane: the first of 9x17, 11x60, 13x21, ... that selects the instantiation with at least two pixel tiles along each axis, the
    last tile partial in both (1x1 kernels see the flattened plane: two tiles, the last partial).  What the planner makes of these
    planes: 13x21 tiles 8x16 in split precision (9x17 does not: 4x32 pads it less) and 8x8 in fp32, 11x60 tiles 4x32 (split) and
    4x16 (fp32), 5x60 tiles 2x32 (fp32), 9x17 serves the 1x1 kernels, 17x33 is the input of the stride-2 kernel's 9x17 plane.
  * where a selection rule admits no small launch, the cheapest launch that it admits:
      - 128-channel tiles without a K split stay only while ceil(wide blocks / 256) > ceil(blocks / 256): an odd pixel-tile count
        (3x3 tiles: 17x33, 11x65) and 52..56 (batch x 64-channel tiles), hence B 13 x Cout 256;
      - RELU_TAPS with two sub-tiles and the LEAN kernels with two sub-tiles need >= 512 wide blocks: B 52..172 of a 9x33 (2x3
        tiles), 9x49 (3x2 tiles) or 3x3-tile plane with Cin 16 — up to 0.7 GMAC, the largest cases of the table.
  * an odd pixel-tile count (the last wide block's second sub-tile is empty) for some of the NSUB = 2 cases, a LEAN one included.
  * channels: fp32 sources that end off the K chunk (16 split, 8 / 32 fp32: 37 = 16 + 21, 71 = 48 + 23, 69 = 32 + 16 + 21, 37 =
    32 + 5), blocked sources in multiples of 16, one to three sources, Cout 40 / 100 / 127 beside the multiples of 64 (RELU_TAPS
    included), and at least two K chunks per slice wherever K is split (the planner's own rule).
  * the K-split kernels store raw partial sums, so their cases rotate over LINEAR, GRU_ZR and GRU_Q behind the finish launch.
  * seven cases carry a dual launch: fused (narrow, wide, lean, 1x1, outputs of its own) and as two calls (fp32, K split).
"""
import importlib.util
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def _load_gen():
    spec = importlib.util.spec_from_file_location("make_golden_conv_plans", os.path.join(GOLDEN, "make_golden_conv_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_gen()
LIN, ZR, Q, TAPS = gen.LIN, gen.ZR, gen.Q, gen.TAPS
LEAN2 = {"lean": 2}
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, ACT_RELU6, ACT_LEAKY = range(6)
OUT_COFF, OUT_PAD = 4, 7       # LINEAR: out is channels [4, 4 + Cout) of a tensor of Cout + 7 channels filled with OUT_FILL
OUT_FILL = 7.0
ADD_COFF, ADD_PAD = 3, 5       # add: channels [3, 3 + Cout) of a tensor of Cout + 5 channels
BS_COFF, BS_PAD = 8, 16        # blocked copy: channels [8, 8 + C) of a BS8 of C + 16 channels filled with NaN


def r8(n):
    return (n + 7) // 8 * 8


def K(kernel, B, H, W, srcs, Cout, KS=3, prec=1, epi=LIN, stride=1, dual=None, fast16=0, knobs=None):
    """A case named for its instantiation.  A blocked copy of the result is requested wherever the form allows one (split precision,
    stride 1, not RELU_TAPS): out_bs = the channels of the blocked tensor it is a window of."""
    out_bs = 0
    if prec == 1 and stride == 1 and epi != TAPS:
        out_bs = 2 * r8(Cout) + BS_PAD if dual in ("bs", "f32") else (Cout // 2 if epi == ZR else Cout) + BS_PAD
    c = gen.case(kernel, B, H, W, srcs, Cout, KS=KS, prec=prec, epi=epi, stride=stride, ws=True, out_bs=out_bs, dual=dual, fast16=fast16)
    c["knobs"] = dict(knobs or {})
    return c


CASES = [
    K("conv_igemm_kernel<1, 64, 0>", 2, 9, 17, [32, 5], 100, KS=1, prec=0),  # tiles 1x3, grid 12
    K("conv_igemm_kernel<1, 64, 1>", 2, 9, 17, [256, 48], 128, KS=1, prec=0, epi=ZR),  # tiles 1x3, grid 12
    K("conv_igemm_kernel<1, 64, 2>", 2, 9, 17, [256, 5], 127, KS=1, prec=0, epi=Q),  # tiles 1x3, grid 12
    K("conv_igemm_kernel<3, 16, 0>", 1, 11, 60, [37], 64, prec=0, dual="f32"),  # tiles 3x4, grid 12, dual mode 2
    K("conv_igemm_kernel<3, 16, 1>", 1, 11, 60, [37], 128, prec=0, epi=ZR),  # tiles 3x4, grid 24
    K("conv_igemm_kernel<3, 16, 2>", 2, 11, 60, [16, 21], 40, prec=0, epi=Q),  # tiles 3x4, grid 24
    K("conv_igemm_kernel<3, 32, 0>", 2, 5, 60, [64, 16], 100, prec=0),  # tiles 3x2, grid 24
    K("conv_igemm_kernel<3, 32, 1>", 2, 5, 60, [32, 16, 21], 128, prec=0, epi=ZR),  # tiles 3x2, grid 24
    K("conv_igemm_kernel<3, 32, 2>", 2, 5, 60, [37], 127, prec=0, epi=Q),  # tiles 3x2, grid 24
    K("conv_igemm_kernel<3, 8, 0>", 2, 13, 21, [48, 23], 127, prec=0),  # tiles 2x3, grid 24
    K("conv_igemm_kernel<3, 8, 1>", 2, 13, 21, [16, 21], 256, prec=0, epi=ZR),  # tiles 2x3, grid 48
    K("conv_igemm_kernel<3, 8, 2>", 2, 13, 21, [64, 16], 40, prec=0, epi=Q),  # tiles 2x3, grid 12
    K("conv_split_kernel<1, 128, 128, 0, 1, 1, false, false>", 2, 9, 17, [32, 5], 100, KS=1),  # tiles 1x2, grid 4
    K("conv_split_kernel<1, 128, 128, 1, 1, 1, false, false>", 2, 9, 17, [37], 256, KS=1, epi=ZR),  # tiles 1x2, grid 8
    K("conv_split_kernel<1, 128, 128, 2, 1, 1, false, false>", 2, 9, 17, [64, 32, 5], 127, KS=1, epi=Q),  # tiles 1x2, grid 4
    K("conv_split_kernel<1, 128, 128, 3, 1, 1, false, false>", 2, 9, 17, [256, 5], 127, KS=1),  # tiles 1x2, ksplit 2 over 5 chunks, grid 8
    K("conv_split_kernel<1, 128, 64, 0, 1, 1, false, false>", 2, 9, 17, [128], 40, KS=1, dual="f32"),  # tiles 1x2, grid 8, dual mode 1
    K("conv_split_kernel<1, 128, 64, 1, 1, 1, false, false>", 2, 9, 17, [32, 5], 384, KS=1, epi=ZR),  # tiles 1x2, grid 24
    K("conv_split_kernel<1, 128, 64, 2, 1, 1, false, false>", 2, 9, 17, [37], 40, KS=1, epi=Q),  # tiles 1x2, grid 4
    K("conv_split_kernel<1, 128, 64, 3, 1, 1, false, false>", 2, 9, 17, [256, 5], 40, KS=1, epi=Q),  # tiles 1x2, ksplit 2 over 5 chunks, grid 8
    K("conv_split_kernel<3, 16, 128, 0, 1, 1, false, false>", 13, 17, 33, [16], 256),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 16, 128, 0, 1, 1, true, false>", 13, 17, 33, [16], 256, fast16=1),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 16, 128, 1, 1, 1, false, false>", 13, 17, 33, [16], 256, epi=ZR),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 16, 128, 1, 1, 1, true, false>", 13, 17, 33, [16], 256, epi=ZR, fast16=1),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 16, 128, 2, 1, 1, false, false>", 13, 17, 33, [16], 256, epi=Q),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 16, 128, 2, 1, 1, true, false>", 13, 17, 33, [16], 256, epi=Q, fast16=1),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 16, 128, 3, 1, 1, false, false>", 1, 13, 21, [48, 23], 256, epi=ZR),  # tiles 2x2, ksplit 2 over 5 chunks, grid 16
    K("conv_split_kernel<3, 16, 128, 3, 1, 1, true, false>", 2, 13, 21, [32, 16, 21], 127, fast16=1),  # tiles 2x2, ksplit 2 over 5 chunks, grid 16
    K("conv_split_kernel<3, 16, 64, 0, 1, 1, false, false>", 2, 13, 21, [37], 40, dual="f32"),  # tiles 2x2, grid 16, dual mode 1
    K("conv_split_kernel<3, 16, 64, 0, 1, 1, false, true>", 2, 13, 21, [-16], 40, knobs=LEAN2),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 0, 1, 1, true, false>", 2, 13, 21, [16, 21], 40, fast16=1),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 0, 1, 2, false, false>", 2, 17, 33, [64, 16], 100, stride=2),  # tiles 2x2, grid 16
    K("conv_split_kernel<3, 16, 64, 0, 2, 1, false, false>", 2, 17, 33, [16, 21], 127),  # tiles 3x3, grid 20
    K("conv_split_kernel<3, 16, 64, 0, 2, 1, false, true>", 172, 9, 33, [-16], 40),  # tiles 2x3, grid 516
    K("conv_split_kernel<3, 16, 64, 0, 2, 1, true, false>", 2, 13, 21, [-16], 128, dual="bs", fast16=1),  # tiles 2x2, grid 16, dual mode 1
    K("conv_split_kernel<3, 16, 64, 1, 1, 1, false, false>", 1, 13, 21, [16, 21], 384, epi=ZR),  # tiles 2x2, grid 24
    K("conv_split_kernel<3, 16, 64, 1, 1, 1, false, true>", 2, 13, 21, [-16, -16], 128, epi=ZR, knobs=LEAN2),  # tiles 2x2, grid 16
    K("conv_split_kernel<3, 16, 64, 1, 1, 1, true, false>", 2, 13, 21, [16, 21], 128, epi=ZR, fast16=1),  # tiles 2x2, grid 16
    K("conv_split_kernel<3, 16, 64, 1, 2, 1, false, false>", 2, 13, 21, [37], 256, epi=ZR),  # tiles 2x2, grid 16
    K("conv_split_kernel<3, 16, 64, 1, 2, 1, false, true>", 86, 9, 33, [-16], 128, epi=ZR),  # tiles 2x3, grid 516
    K("conv_split_kernel<3, 16, 64, 1, 2, 1, true, false>", 2, 13, 21, [16, 21], 256, epi=ZR, fast16=1),  # tiles 2x2, grid 16
    K("conv_split_kernel<3, 16, 64, 2, 1, 1, false, false>", 2, 13, 21, [16, 21], 40, epi=Q),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 2, 1, 1, false, true>", 2, 13, 21, [-16, -16], 40, epi=Q, knobs=LEAN2),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 2, 1, 1, true, false>", 2, 13, 21, [37], 40, epi=Q, fast16=1),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 2, 2, 1, false, false>", 2, 13, 21, [37], 127, epi=Q),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 2, 2, 1, false, true>", 172, 9, 33, [-16], 40, epi=Q),  # tiles 2x3, grid 516
    K("conv_split_kernel<3, 16, 64, 2, 2, 1, true, false>", 2, 13, 21, [16, 21], 127, epi=Q, fast16=1),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 3, 1, 1, false, false>", 1, 13, 21, [128], 40, dual="f32"),  # tiles 2x2, ksplit 4 over 8 chunks, grid 16, dual mode 2
    K("conv_split_kernel<3, 16, 64, 3, 1, 1, false, true>", 2, 13, 21, [-32, -16, -16], 100, knobs=LEAN2),  # tiles 2x2, ksplit 2 over 4 chunks, grid 32
    K("conv_split_kernel<3, 16, 64, 3, 1, 1, true, false>", 2, 13, 21, [48, 23], 40, epi=Q, fast16=1),  # tiles 2x2, ksplit 2 over 5 chunks, grid 16
    K("conv_split_kernel<3, 16, 64, 4, 1, 1, false, false>", 2, 13, 21, [16, 21], 127, epi=TAPS),  # tiles 2x2, grid 16
    K("conv_split_kernel<3, 16, 64, 4, 1, 1, false, true>", 1, 13, 21, [-64, -64], 127, epi=TAPS, knobs=LEAN2),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 4, 1, 1, true, false>", 2, 13, 21, [32, 16, 21], 40, epi=TAPS, fast16=1),  # tiles 2x2, grid 8
    K("conv_split_kernel<3, 16, 64, 4, 2, 1, false, false>", 172, 9, 33, [16], 40, epi=TAPS),  # tiles 2x3, grid 516
    K("conv_split_kernel<3, 16, 64, 4, 2, 1, false, true>", 128, 17, 33, [-16], 40, epi=TAPS),  # tiles 3x3, grid 640
    K("conv_split_kernel<3, 16, 64, 4, 2, 1, true, false>", 172, 9, 33, [16], 40, epi=TAPS, fast16=1),  # tiles 2x3, grid 516
    K("conv_split_kernel<3, 32, 128, 0, 1, 1, false, false>", 13, 11, 65, [16], 256),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 32, 128, 0, 1, 1, true, false>", 13, 11, 65, [16], 256, fast16=1),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 32, 128, 1, 1, 1, false, false>", 13, 11, 65, [16], 256, epi=ZR),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 32, 128, 1, 1, 1, true, false>", 13, 11, 65, [16], 256, epi=ZR, fast16=1),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 32, 128, 2, 1, 1, false, false>", 13, 11, 65, [16], 256, epi=Q),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 32, 128, 2, 1, 1, true, false>", 13, 11, 65, [16], 256, epi=Q, fast16=1),  # tiles 3x3, grid 234
    K("conv_split_kernel<3, 32, 128, 3, 1, 1, false, false>", 1, 11, 60, [32, 16, 21], 100, epi=Q),  # tiles 3x2, ksplit 2 over 5 chunks, grid 12
    K("conv_split_kernel<3, 32, 128, 3, 1, 1, true, false>", 1, 11, 60, [32, 16, 21], 100, fast16=1),  # tiles 3x2, ksplit 2 over 5 chunks, grid 12
    K("conv_split_kernel<3, 32, 64, 0, 1, 1, false, false>", 2, 11, 60, [37], 40),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 0, 1, 1, false, true>", 2, 11, 60, [-48], 40, dual="bs", knobs=LEAN2),  # tiles 3x2, grid 24, dual mode 1
    K("conv_split_kernel<3, 32, 64, 0, 1, 1, true, false>", 2, 11, 60, [16, 21], 40, fast16=1),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 0, 2, 1, false, false>", 2, 11, 60, [16], 128, dual="sep"),  # tiles 3x2, grid 24, dual mode 1
    K("conv_split_kernel<3, 32, 64, 0, 2, 1, false, true>", 172, 9, 49, [-16], 40),  # tiles 3x2, grid 516
    K("conv_split_kernel<3, 32, 64, 0, 2, 1, true, false>", 1, 11, 60, [37], 127, fast16=1),  # tiles 3x2, grid 6
    K("conv_split_kernel<3, 32, 64, 1, 1, 1, false, false>", 1, 11, 60, [16, 21], 128, epi=ZR),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 1, 1, 1, false, true>", 2, 11, 60, [-16, -16], 128, epi=ZR, knobs=LEAN2),  # tiles 3x2, grid 24
    K("conv_split_kernel<3, 32, 64, 1, 1, 1, true, false>", 1, 11, 60, [16, 21], 128, epi=ZR, fast16=1),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 1, 2, 1, false, false>", 2, 11, 60, [16], 256, epi=ZR),  # tiles 3x2, grid 24
    K("conv_split_kernel<3, 32, 64, 1, 2, 1, false, true>", 52, 11, 65, [-16], 128, epi=ZR),  # tiles 3x3, grid 520
    K("conv_split_kernel<3, 32, 64, 1, 2, 1, true, false>", 2, 11, 60, [16], 256, epi=ZR, fast16=1),  # tiles 3x2, grid 24
    K("conv_split_kernel<3, 32, 64, 2, 1, 1, false, false>", 2, 11, 60, [16, 21], 40, epi=Q),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 2, 1, 1, false, true>", 2, 11, 60, [-16, -16], 40, epi=Q, knobs=LEAN2),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 2, 1, 1, true, false>", 2, 11, 60, [37], 40, epi=Q, fast16=1),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 2, 2, 1, false, false>", 2, 11, 60, [37], 100, epi=Q),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 2, 2, 1, false, true>", 172, 9, 49, [-16], 40, epi=Q),  # tiles 3x2, grid 516
    K("conv_split_kernel<3, 32, 64, 2, 2, 1, true, false>", 1, 11, 65, [16, 21], 127, epi=Q, fast16=1),  # tiles 3x3, grid 10
    K("conv_split_kernel<3, 32, 64, 3, 1, 1, false, false>", 2, 11, 60, [32, 16, 21], 40, epi=Q),  # tiles 3x2, ksplit 2 over 5 chunks, grid 24
    K("conv_split_kernel<3, 32, 64, 3, 1, 1, false, true>", 1, 11, 60, [-32, -16, -16], 128, epi=ZR, knobs=LEAN2),  # tiles 3x2, ksplit 2 over 4 chunks, grid 24
    K("conv_split_kernel<3, 32, 64, 3, 1, 1, true, false>", 2, 11, 60, [48, 23], 40, fast16=1),  # tiles 3x2, ksplit 2 over 5 chunks, grid 24
    K("conv_split_kernel<3, 32, 64, 4, 1, 1, false, false>", 2, 11, 60, [16, 21], 100, epi=TAPS),  # tiles 3x2, grid 24
    K("conv_split_kernel<3, 32, 64, 4, 1, 1, false, true>", 1, 11, 60, [-64, -64], 40, epi=TAPS, knobs=LEAN2),  # tiles 3x2, grid 6
    K("conv_split_kernel<3, 32, 64, 4, 1, 1, true, false>", 1, 11, 60, [32, 16, 21], 100, epi=TAPS, fast16=1),  # tiles 3x2, grid 12
    K("conv_split_kernel<3, 32, 64, 4, 2, 1, false, false>", 172, 9, 49, [16], 40, epi=TAPS),  # tiles 3x2, grid 516
    K("conv_split_kernel<3, 32, 64, 4, 2, 1, false, true>", 172, 9, 49, [-16], 40, epi=TAPS),  # tiles 3x2, grid 516
    K("conv_split_kernel<3, 32, 64, 4, 2, 1, true, false>", 172, 9, 49, [16], 40, epi=TAPS, fast16=1),  # tiles 3x2, grid 516
]
assert len({c["name"] for c in CASES}) == len(CASES)


def _forms():
    """The LINEAR cases alternate between a plain activation and the residual form relu(h + act(.)); RELU_TAPS is act = RELU."""
    plain = (ACT_RELU, ACT_LEAKY, ACT_NONE, ACT_TANH, ACT_SIGMOID, ACT_RELU6)
    n = 0
    for c in CASES:
        c["act"], c["residual"] = (ACT_RELU if c["epi"] == TAPS else ACT_NONE), False
        if c["epi"] == LIN:
            c["residual"] = n % 2 == 1
            c["act"] = (ACT_NONE, ACT_RELU)[(n // 2) % 2] if c["residual"] else plain[(n // 2) % len(plain)]
            n += 1


_forms()


# ---- the plan of a case -------------------------------------------------------------------------------------------------------

def plan(c):
    """as_conv2d_plan of a case under its explicit knobs and its fast16 flag, as a dict.  Host arithmetic only."""
    import ctypes as C

    from anystereo import _lib as L
    lib = L.load()
    knobs = L.ConvKnobs(**dict(gen.KNOB_DEFAULTS, **c["knobs"]))
    n_ws = lib.as_conv_ws_elems(c["B"], c["Cout"], *gen.out_plane(c))
    was = lib.as_get_fast16()
    try:
        lib.as_set_fast16(c["fast16"])
        d, p = gen.descriptor(L, c, n_ws), L.ConvPlan()
        rc = lib.as_conv2d_plan(C.byref(d), C.byref(knobs), C.byref(p))
        assert rc == 0, (c["name"], rc, lib.as_last_error_string())
    finally:
        lib.as_set_fast16(was)
    return {n: int(getattr(p, n)) for n, _ in L.ConvPlan._fields_}


def kernel_name(plan):
    """The instantiation a plan names, as the code object spells it (tests/golden/conv_kernels.txt)."""
    if plan["family"]:
        return "conv_split_kernel<%d, %d, %d, %d, %d, %d, %s, %s>" % (
            plan["KS"], plan["TW"], plan["BN"], plan["epilogue"], plan["NSUB"], plan["S"], str(bool(plan["FAST"])).lower(), str(bool(plan["LEAN"])).lower())
    return "conv_igemm_kernel<%d, %d, %d>" % (plan["KS"], plan["TW"], plan["epilogue"])


def planned_kernels(plan):
    """The names of the kernels a plan (ops.conv_plan) says as_conv2d launches, in launch order."""
    one = [kernel_name(plan)] + (["conv_finish_kernel<%d>" % plan["finish_epilogue"]] if plan["finish"] else [])
    return one * (2 if plan["dual"] == 2 else 1)  # a dual launch as two calls: the second has the first's shape


def launched_kernels(prof):
    """The conv kernels of a torch.profiler kernel trace, in launch order."""
    found = sorted((e.time_range.start, m.group(0)) for e in prof.events()
                   for m in [re.search(r"conv_(split|igemm|finish)_kernel<[^>]*>", e.name)] if m)
    return [k for _, k in found]


def family(c, plan):
    """The family a FAST error is reported under: epilogue x NSUB x K split."""
    return "%s nsub%d %s" % ({LIN: "LINEAR", ZR: "GRU_ZR", Q: "GRU_Q", TAPS: "RELU_TAPS"}[c["epi"]], plan["NSUB"], "ksplit" if plan["ksplit"] > 1 else "whole-K")


# ---- operands and the fp64 expectation (CPU) ------------------------------------------------------------------------------------

def operands(c):
    """The fp32 operands of a case on the CPU, from det_uniform with seeds of the case's own."""
    import torch

    from anystereo.harness.synthetic import det_uniform as U
    seed = 5000 + 64 * CASES.index(c)
    B, H, W, Cout, KS, epi = c["B"], c["H"], c["W"], c["Cout"], c["KS"], c["epi"]
    ho, wo = gen.out_plane(c)
    cin = sum(abs(ch) for ch in c["srcs"])
    scale = (3.0 / (cin * KS * KS)) ** 0.5
    o = {"x": [U((B, abs(ch), H, W), seed + j, -2, 2) for j, ch in enumerate(c["srcs"])],
         "w": U((Cout, cin, KS, KS), seed + 8) * scale, "bias": U((Cout,), seed + 9) * 0.1}
    if epi != TAPS and not c["dual"]:
        o["add"] = U((B, Cout + ADD_PAD, ho, wo), seed + 10)
    ch = Cout // 2 if epi == ZR else Cout
    if epi in (ZR, Q) or c["residual"]:
        o["h"] = torch.tanh(U((B, ch, ho, wo), seed + 11, -2, 2))
    if epi == Q:
        o["z"] = U((B, Cout, ho, wo), seed + 12, 0.02, 0.98)
    if epi == TAPS:
        o["tap_w"], o["head_bias"] = U((Cout, 9), seed + 13) * 0.05, U((1,), seed + 14)
    if c["dual"]:
        o["x2"], o["w2"], o["bias2"] = U((B, cin, H, W), seed + 20, -2, 2), U((Cout, cin, KS, KS), seed + 21) * scale, U((Cout,), seed + 22) * 0.1
        if c["residual"]:
            o["h2"] = torch.tanh(U((B, Cout, ho, wo), seed + 23, -2, 2))
    return o


def act2_of(c):
    """The second convolution of a dual launch has an activation of its own."""
    return ACT_RELU if c["act"] == ACT_LEAKY else ACT_LEAKY


def _act64(v, act):
    import torch
    if act == ACT_RELU:
        return v.relu()
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_RELU6:
        return v.clamp(0.0, 6.0)
    if act == ACT_LEAKY:
        return torch.where(v >= 0, v, 0.01 * v)
    assert act == ACT_NONE
    return v


def _conv64(c, x, w, bias):
    """The convolution in float64 on the fp32 operands; FAST: on the operands rounded to fp16, which is all the one-MFMA kernel
    reads of them (hi = fp16(x), no scaling; blocked sources hold the same hi parts) — what remains is its fp32 accumulation."""
    import torch
    if c["fast16"]:
        x, w = x.half().float(), w.half().float()
    return torch.nn.functional.conv2d(x.double(), w.double(), bias.double(), stride=c["stride"], padding=c["KS"] // 2)


def expected(c, o):
    """name -> [(first channel, fp64 reference)]: the windows of each output tensor that the launch must fill (include/anystereo_hip.h,
    AS_EPI_*).  'bs' / 'bs_b' are the blocked copies (of out; GRU_ZR: of r*h), 'tss' is tap_shift_sum of the RELU_TAPS planes."""
    import torch
    Cout, epi = c["Cout"], c["epi"]
    x = torch.cat(o["x"], 1)
    acc = _conv64(c, x, o["w"], o["bias"])
    if "add" in o:
        acc = acc + o["add"][:, ADD_COFF:ADD_COFF + Cout].double()
    want = {}
    if epi == LIN:
        y = _act64(acc, c["act"])
        if c["residual"]:
            y = (o["h"].double() + y).relu()
        want["out"], bs = [(OUT_COFF, y)], [(BS_COFF, y)]
        if c["dual"]:
            y2 = _act64(_conv64(c, o["x2"], o["w2"], o["bias2"]), act2_of(c))
            if c["residual"]:
                y2 = (o["h2"].double() + y2).relu()
            if c["dual"] == "sep":
                want["out_b"] = [(0, y2)]
                if c["out_bs"]:
                    want["bs_b"] = [(0, y2)]
            else:
                want["out"].append((OUT_COFF + Cout, y2))
                bs.append((BS_COFF + r8(Cout), y2))
        if c["out_bs"]:
            want["bs"] = bs
    elif epi == ZR:
        g = torch.sigmoid(acc)
        rh = g[:, Cout // 2:] * o["h"].double()
        want["out"], want["out2"] = [(0, g[:, :Cout // 2])], [(0, rh)]
        if c["out_bs"]:
            want["bs"] = [(BS_COFF, rh)]
    elif epi == Q:
        z, h = o["z"].double(), o["h"].double()
        y = (1.0 - z) * h + z * torch.tanh(acc)
        want["out"] = [(0, y)]
        if c["out_bs"]:
            want["bs"] = [(BS_COFF, y)]
    else:
        # per 64-channel tile g and tap t: sum over the tile's channels of tap_w[c][t] * relu(conv)[c]; then the 3x3, Cout -> 1
        # convolution those planes are the channel reductions of
        y, tw = acc.relu(), o["tap_w"].double()
        planes = [torch.einsum("bchw,ct->bthw", y[:, g0:g0 + 64], tw[g0:g0 + 64]) for g0 in range(0, Cout, 64)]
        want["out"] = [(0, torch.cat(planes, 1))]
        want["tss"] = [(0, torch.nn.functional.conv2d(y, tw.reshape(1, Cout, 3, 3), o["head_bias"].double(), padding=1))]
    return want


# ---- the launch (GPU) -----------------------------------------------------------------------------------------------------------

def to_bs(x):
    """An fp32 tensor as the blocked split-fp16 link tensor a convolution would have written (tests/_knob_probe.py)."""
    import torch

    from anystereo import ops
    bb, cc, hh, ww = x.shape
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    return ops.BS8(torch.stack([hi, lo], 1).view(bb, 2, cc // 8, 8, hh, ww).permute(0, 1, 2, 4, 5, 3).contiguous(), cc)


def run_case(c, o, dev, put=None):
    """ops.conv2d of a case; put(t) moves a host operand to the device (default t.to(dev); tests/_guarded.place gives it poisoned
    neighbours).  Every output is passed in pre-filled (the caching allocator can hand back an earlier, correct result):
    out with OUT_FILL, out2 / dual outputs / blocked copies with NaN.  Returns name -> the WHOLE output tensor on the CPU (fp32;
    blocked tensors as their fp16 records), surroundings included."""
    import torch

    from anystereo import ops
    B, Cout, epi = c["B"], c["Cout"], c["epi"]
    ho, wo = gen.out_plane(c)
    nan = float("nan")
    if put is None:
        put = lambda t: t.to(dev)  # noqa: E731
    prev = ops.get_precision()
    ops.set_precision("split" if c["prec"] else "fp32")
    try:
        with ops.fast_fp16(bool(c["fast16"])):
            srcs = [to_bs(put(x)) if ch < 0 else put(x) for x, ch in zip(o["x"], c["srcs"])]
            pk = ops.PackedConv().get([put(o["w"])], [put(o["bias"])])
            kw, res = dict(epilogue=epi, stride=c["stride"], act=c["act"]), {}
            if "add" in o:
                kw.update(add=put(o["add"]), add_coff=ADD_COFF)
            if "h" in o:
                kw["h"] = put(o["h"])
            if c["out_bs"]:
                res["bs"] = ops.BS8.empty(B, c["out_bs"], ho, wo, dev)
                res["bs"].t.fill_(nan)
                kw.update(out_bs=res["bs"], out_bs_coff=BS_COFF)
            if epi == LIN:
                windows = 2 if c["dual"] in ("bs", "f32") else 1
                res["out"] = torch.full((B, windows * Cout + OUT_PAD, ho, wo), OUT_FILL, device=dev)
                kw.update(out=res["out"], out_coff=OUT_COFF)
                if c["dual"]:
                    s2 = put(o["x2"])
                    pk2 = ops.PackedConv().get([put(o["w2"])], [put(o["bias2"])])
                    dual = {"src": to_bs(s2) if c["dual"] == "bs" else s2, "pack": pk2, "act": act2_of(c)}
                    if "h2" in o:
                        dual["h"] = put(o["h2"])
                    if c["dual"] == "sep":
                        res["out_b"] = dual["out"] = torch.full((B, Cout, ho, wo), nan, device=dev)
                        if c["out_bs"]:
                            res["bs_b"] = dual["out_bs"] = ops.BS8.empty(B, Cout, ho, wo, dev)
                            res["bs_b"].t.fill_(nan)
                    else:
                        dual.update(out_coff=OUT_COFF + Cout, out_bs_coff=BS_COFF + r8(Cout) if c["out_bs"] else 0)
                    kw["dual"] = dual
            elif epi == ZR:
                res["out"] = torch.full((B, Cout // 2, ho, wo), OUT_FILL, device=dev)
                res["out2"] = torch.full((B, Cout // 2, ho, wo), nan, device=dev)
                kw.update(out=res["out"], out2=res["out2"])
            elif epi == Q:
                res["out"] = torch.full((B, Cout, ho, wo), OUT_FILL, device=dev)
                kw.update(out=res["out"], z=put(o["z"]))
            else:
                res["out"] = torch.full((B, (Cout + 63) // 64 * 9, ho, wo), OUT_FILL, device=dev)
                kw.update(out=res["out"], tap_w=put(o["tap_w"]))
            ops.conv2d(srcs, pk, **kw)
            if epi == TAPS:
                res["tss"] = ops.tap_shift_sum(res["out"], put(o["head_bias"]))
    finally:
        ops.set_precision(prev)
    return {k: (v.t if isinstance(v, ops.BS8) else v).cpu() for k, v in res.items()}


def run_cases(cases, dev):
    """Every case under one torch.profiler session -> ([outputs per case], [launched conv kernel names, in order])."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    outs = []
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for c in cases:
            outs.append(run_case(c, operands(c), dev))
        torch.cuda.synchronize()
    return outs, launched_kernels(prof)


# ---- the comparison (CPU) -------------------------------------------------------------------------------------------------------

def _unblock(t):
    """BS8 records [B, 2, C8, H, W, 8] fp16 -> (hi, lo) planes [B, C8 * 8, H, W] in float64."""
    b, _, c8, h, w, _ = t.shape
    planes = t.double().permute(0, 1, 2, 5, 3, 4).reshape(b, 2, c8 * 8, h, w)
    return planes[:, 0], planes[:, 1]


def check_case(c, got, want, rtol):
    """Every window of every output within rtol x the reference's maximum (blocked copies: + 2^-21 x the maximum for the record
    pairs), finite, and everything around the windows still what it was filled with.  Returns name -> the largest error / maximum."""
    import torch
    assert set(got) == set(want), (c["name"], sorted(got), sorted(want))
    worst = {}
    for name, windows in want.items():
        t = torch.as_tensor(got[name])
        blocked = name in ("bs", "bs_b")
        if blocked:
            hi, lo = _unblock(t)
            val, rest_of = hi + lo / 2048.0, (hi, lo)
        else:
            val = t.double()
            rest_of = (val,)
        inside = torch.zeros(val.shape[1], dtype=torch.bool)
        for coff, ref in windows:
            g = val[:, coff:coff + ref.shape[1]]
            what = "%s: %s[%d:%d]" % (c["name"], name, coff, coff + ref.shape[1])
            assert g.shape == ref.shape, (what, g.shape, ref.shape)
            assert torch.isfinite(g).all(), what + ": non-finite values"
            top = ref.abs().max().item()
            err = (g - ref).abs().max().item()
            lim = (rtol + (2.0 ** -21 if blocked else 0.0)) * top
            worst[name] = max(worst.get(name, 0.0), err / top)
            assert err <= lim, "%s: max abs err %.3e > %.3e (%.2e of the reference's maximum %.3e)" % (what, err, lim, err / top, top)
            inside[coff:coff + ref.shape[1]] = True
        # A blocked window ends at 8 + C with the tensor holding C + 16 channels, so the slots up to the next multiple of 8 are
        # inside the tensor's channel count: another producer's, not padding (which conv.hip zeroes only past that count) -> untouched
        for r in rest_of:
            around = r[:, ~inside]
            if blocked or name in ("out2", "out_b"):
                assert torch.isnan(around).all(), "%s: %s written outside its window" % (c["name"], name)
            else:
                assert (around == OUT_FILL).all(), "%s: %s written outside its window" % (c["name"], name)
    return worst
