"""The case list of tests/test_conv_plan_cpu.py and the generator of tests/golden/conv_plans.json.

    python tests/golden/make_golden_conv_plans.py            # rewrite conv_plans.json from the tree's as_conv2d_plan
    python tests/golden/make_golden_conv_plans.py --check    # exit 1 if the file differs from what the tree plans

conv_plans.json was first recorded from the launches of as_conv2d itself (a throwaway build in which each kernel launch
printed its template arguments, grid, block, LDS and schedule parameters); the generator reproduces that file from
as_conv2d_plan, and the test holds the planner to it row for row.  A change of the table is a change of the schedule: regenerate
on purpose, never to make a test pass.

A row is one (knob set, case); the file keeps the distinct rows once (`plans`) and an index per knob set and case (`rows`).
Needs no GPU: data pointers are fake, non-null and 16-byte aligned, and the planner never dereferences them.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "conv_plans.json")

LIN, ZR, Q, TAPS = 0, 1, 2, 4
KNOB_FIELDS = ("lean", "xcd", "xcd_stagger", "lean_offset", "ksplit_max", "dma", "wide", "wide64", "small_dma", "prefer64")
KNOB_DEFAULTS = dict(lean=1, xcd=2, xcd_stagger=0, lean_offset=0, ksplit_max=8, dma=1, wide=1, wide64=1, small_dma=1, prefer64=0)
# the default, the three KNOB_SETS of test_hip_parity.py (their conv knobs), every knob alone at each documented non-default value
KNOB_SETS = {
    "default": {},
    "set1": dict(lean=0, xcd=0, dma=0),
    "set2": dict(xcd=1, lean=3, ksplit_max=1, wide=0, wide64=0, small_dma=0),
    "set3": dict(lean=2, prefer64=1, xcd_stagger=4, lean_offset=8, ksplit_max=2),
    "lean0": dict(lean=0), "lean2": dict(lean=2), "lean3": dict(lean=3),
    "xcd0": dict(xcd=0), "xcd1": dict(xcd=1),
    "ksplit_max1": dict(ksplit_max=1), "prefer64": dict(prefer64=1),
    "dma0": dict(dma=0), "wide0": dict(wide=0), "wide64_0": dict(wide64=0), "small_dma0": dict(small_dma=0),
    "xcd_stagger4": dict(xcd_stagger=4), "lean_offset8": dict(lean_offset=8),
}
PLAN_FIELDS = ("family", "KS", "TW", "BN", "NSUB", "S", "FAST", "LEAN", "epilogue", "finish", "finish_epilogue", "ksplit", "tiles_x",
               "tiles_y", "n_tiles", "chunks", "H", "W", "Hi", "Wi", "all_bs", "xcd_map", "stagger", "lean_offset", "dual", "block", "lds",
               "grid", "finish_grid")


def case(name, B, H, W, srcs, Cout, KS=3, prec=1, epi=LIN, stride=1, ws=True, out_bs=0, dual=None, fast16=0):
    """srcs: channels per source, negative = a blocked (BS8) source.  out_bs: channels of the blocked result tensor (0: none).
    dual: None | "bs" | "f32" (the second source's form) | "sep" (fp32 second source, outputs of its own).  ws: split-K scratch
    as ops.conv2d passes it (as_conv_ws_elems)."""
    return dict(name=name, B=B, H=H, W=W, srcs=list(srcs), Cout=Cout, KS=KS, prec=prec, epi=epi, stride=stride, ws=ws, out_bs=out_bs,
                dual=dual, fast16=fast16)


def _cases():
    cs = []
    # the GRU loop at the cfg-2 sizes (tests/_knob_probe.py): z|r, q; then the motion encoder and the head, blocked links
    for tag, h, w in (("04", 136, 240), ("08", 68, 120), ("16", 34, 60)):
        cs.append(case("zr" + tag, 1, h, w, [-128] * 3, 256, epi=ZR, out_bs=128))
        cs.append(case("q" + tag, 1, h, w, [-128] * 3, 128, epi=Q, out_bs=128))
        cs.append(case("zr%s_f16" % tag, 1, h, w, [-128] * 3, 256, epi=ZR, out_bs=128, fast16=1))
        cs.append(case("q%s_f32src" % tag, 1, h, w, [128] * 3, 128, epi=Q))
        cs.append(case("zr%s_nows" % tag, 1, h, w, [-128] * 3, 256, epi=ZR, ws=False))
    cs += [
        case("enc_c2d2", 1, 136, 240, [-64], 64, out_bs=128, dual="bs"),
        case("enc_c2d2_f16", 1, 136, 240, [-64], 64, out_bs=128, dual="bs", fast16=1),
        case("enc_conv", 1, 136, 240, [-128], 127, out_bs=128),
        case("head_taps", 1, 136, 240, [-128], 256, epi=TAPS),
        case("head_taps_f16", 1, 136, 240, [-128], 256, epi=TAPS, fast16=1),
        case("head_taps_f32src", 1, 136, 240, [128], 256, epi=TAPS),
        case("cnet_64", 1, 272, 480, [64], 64),
        case("cnet_64_f16", 1, 272, 480, [64], 64, fast16=1),
        case("cnet_64_bs", 1, 272, 480, [-64], 64),
        case("train_128_256", 4, 40, 80, [128], 256),
        case("train_128_128_1x1", 4, 40, 80, [128], 128, KS=1),
        # the smallest shapes that select an instantiation under the default knobs (test_conv_dispatch_runs_the_planned_kernel)
        case("lean_16_256", 1, 136, 240, [-16], 256),
        case("ksplit_128_128", 1, 17, 30, [128], 128),
        case("ksplit_128_128_nows", 1, 17, 30, [128], 128, ws=False),
        # a big plane that tiles 4x32: wide lean blocks and the tap epilogue at TW 32
        case("big32_lean_16_256", 1, 196, 224, [-16], 256),
        case("big32_taps", 1, 196, 224, [-128], 256, epi=TAPS),
        case("big32_taps_f16", 1, 196, 224, [-128], 256, epi=TAPS, fast16=1),
        case("big32_taps_f32src", 1, 196, 224, [128], 256, epi=TAPS),
    ]
    # tile shape: 4x32 beats 8x16 and the reverse (split kernel); TW 8 / 16 / 32 of the fp32 kernel; every epilogue on each
    for tag, h, w in (("4x32", 4, 32), ("8x16", 8, 16), ("12x33", 12, 33), ("9x47", 9, 47)):
        for cout in (64, 128):
            cs.append(case("tile_%s_c%d" % (tag, cout), 2, h, w, [48], cout))
            cs.append(case("tile_%s_c%d_nows" % (tag, cout), 2, h, w, [48], cout, ws=False))
            cs.append(case("tile_%s_c%d_q_bs" % (tag, cout), 2, h, w, [-48], cout, epi=Q, ws=False))
            cs.append(case("tile_%s_c%d_q_f16" % (tag, cout), 2, h, w, [48], cout, epi=Q, fast16=1))
        cs.append(case("tile_%s_zr" % tag, 2, h, w, [48], 128, epi=ZR))
        cs.append(case("tile_%s_taps" % tag, 2, h, w, [-48], 100, epi=TAPS))
        cs.append(case("tile_%s_taps_f16" % tag, 2, h, w, [48], 100, epi=TAPS, fast16=1))
        cs.append(case("tile_%s_taps_f32src" % tag, 2, h, w, [48], 100, epi=TAPS))
    for tag, h, w in (("8x8", 8, 8), ("4x16", 4, 16), ("2x32", 2, 32), ("13x21", 13, 21)):
        for epi, cout in ((LIN, 100), (ZR, 128), (Q, 64)):
            cs.append(case("fp32_%s_e%d" % (tag, epi), 3, h, w, [16, 21], cout, prec=0, epi=epi))
            cs.append(case("fp32_1x1_%s_e%d" % (tag, epi), 3, h, w, [32, 5], cout, KS=1, prec=0, epi=epi))
    # channel counts
    for cout in (9, 64, 100, 127, 128, 256):
        for cin in (16, 37, 48, 64, 128, 384):
            cs.append(case("ch_%d_%d" % (cin, cout), 1, 40, 56, [cin], cout))
            cs.append(case("ch_%d_%d_1x1" % (cin, cout), 1, 40, 56, [cin], cout, KS=1))
        cs.append(case("ch_bs_64_%d" % cout, 1, 40, 56, [-64], cout))
        cs.append(case("ch_fp32_64_%d" % cout, 1, 40, 56, [64], cout, prec=0))
    # 128-channel tiles that stay (255 blocks: no room for a K split, two rounds of wide blocks), with and without blocked sources
    for epi, cout in ((LIN, 384), (ZR, 384), (Q, 384)):
        for tag, src, f16 in (("", 32, 0), ("_bs", -32, 0), ("_f16", 32, 1), ("_bs_f16", -32, 1)):
            cs.append(case("bn128_e%d%s" % (epi, tag), 17, 8, 80, [src], cout, epi=epi, fast16=f16))
            cs.append(case("bn128_tw32_e%d%s" % (epi, tag), 17, 4, 160, [src], cout, epi=epi, fast16=f16))
    # small maps: K split at every tile shape, every epilogue behind the finish launch, with and without a blocked result
    for tag, h, w in (("8x16", 8, 16), ("4x32", 4, 32)):
        for epi, cout in ((LIN, 64), (ZR, 128), (Q, 64), (LIN, 128), (Q, 128)):
            for sfx, src, f16, obs in (("", 64, 0, 0), ("_bs", -64, 0, 72), ("_f16", 64, 1, 0)):
                cs.append(case("small_%s_e%d_c%d%s" % (tag, epi, cout, sfx), 1, h, w, [src] * 2, cout, epi=epi, fast16=f16,
                               out_bs=obs and (cout // 2 if epi == ZR else cout) + 8))
    for epi, cout in ((LIN, 64), (LIN, 128), (ZR, 128), (ZR, 256), (Q, 64), (Q, 128)):
        cs.append(case("1x1_small_e%d_c%d" % (epi, cout), 1, 17, 30, [256], cout, KS=1, epi=epi))
        cs.append(case("1x1_big_e%d_c%d" % (epi, cout), 2, 68, 120, [37], cout, KS=1, epi=epi))
        cs.append(case("1x1_big_e%d_c%d_f16" % (epi, cout), 2, 68, 120, [37], cout, KS=1, epi=epi, fast16=1))
    # stride 2
    cs += [case("s2_64", 1, 136, 240, [64], 64, stride=2), case("s2_100_odd", 2, 37, 53, [37], 100, stride=2),
           case("s2_128_f16", 1, 68, 120, [64], 128, stride=2, fast16=1)]
    # dual launches: fused (wide and narrow blocks, blocked and fp32 sources, outputs of its own), two calls by precision, by K split
    cs += [
        case("dual_wide_f32", 1, 136, 240, [64], 64, dual="f32"),
        case("dual_narrow_bs", 1, 40, 56, [-64], 64, out_bs=128, dual="bs"),
        case("dual_narrow_mixed", 1, 40, 56, [-64], 64, dual="f32"),
        case("dual_sep", 1, 68, 120, [128], 128, dual="sep"),
        case("dual_sep_f16", 1, 68, 120, [128], 128, dual="sep", fast16=1),
        case("dual_1x1", 1, 68, 120, [128], 128, KS=1, dual="f32"),
        case("dual_fp32", 1, 40, 56, [64], 64, prec=0, dual="f32"),
        case("dual_fp32_1x1", 1, 40, 56, [64], 64, KS=1, prec=0, dual="f32"),
        case("dual_ksplit", 1, 17, 30, [128], 128, dual="f32"),
        case("dual_ksplit_bs", 1, 17, 30, [-128], 128, dual="bs"),
        case("dual_ksplit_1x1", 1, 17, 30, [128], 128, KS=1, dual="f32"),
        case("dual_small_nows", 1, 17, 30, [128], 128, ws=False, dual="f32"),
    ]
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


CASES = _cases()
FAKE = 0x10000  # data "pointers": non-null, 16-byte aligned, never dereferenced by the host


def descriptor(lib_mod, c, ws_elems):
    """The as_conv_desc of a case, filled as ops.conv2d fills it.  ws_elems: as_conv_ws_elems of the problem."""
    d = lib_mod.ConvDesc()
    for i, ch in enumerate(c["srcs"]):
        d.src[i], d.src_c[i], d.src_bs[i] = FAKE * (i + 1), abs(ch), 1 if ch < 0 else 0
    d.n_src, d.Cin = len(c["srcs"]), sum(abs(ch) for ch in c["srcs"])
    d.B, d.H, d.W, d.Cout, d.KS = c["B"], c["H"], c["W"], c["Cout"], c["KS"]
    d.precision, d.epilogue, d.stride = c["prec"], c["epi"], c["stride"]
    d.wpack, d.bias, d.out = FAKE * 8, FAKE * 9, FAKE * 10
    epi = c["epi"]
    if epi == ZR:
        d.h, d.out2 = FAKE * 11, FAKE * 12
    elif epi == Q:
        d.h, d.z = FAKE * 11, FAKE * 13
    elif epi == TAPS:
        d.tap_w, d.act = FAKE * 14, 1
    else:
        d.out_ctot = 2 * c["Cout"] if c["dual"] in ("bs", "f32") else c["Cout"]
    if c["out_bs"]:
        d.out_bs, d.out_bs_ctot = FAKE * 15, c["out_bs"]
    if c["dual"]:
        d.dual, d.src2, d.src2_bs, d.wpack2 = 1, FAKE * 16, 1 if c["dual"] == "bs" else 0, FAKE * 17
        if c["dual"] == "sep":
            d.out_b = FAKE * 18
            if c["out_bs"]:
                d.out_bs_b = FAKE * 20
        else:
            d.out_coff2, d.out_bs_coff2 = c["Cout"], c["Cout"] if c["out_bs"] else 0
    if c["ws"] and c["prec"] == 1 and c["stride"] == 1 and ws_elems > 0:
        d.ws, d.ws_elems = FAKE * 19, ws_elems
    return d


def out_plane(c):
    return (c["H"], c["W"]) if c["stride"] == 1 else ((c["H"] - 1) // 2 + 1, (c["W"] - 1) // 2 + 1)


def pack_table(knob_rows, ws_elems):
    """knob_rows: {knob set: [row per case]}, a row = the PLAN_FIELDS values -> the file's form (distinct rows kept once)."""
    plans, index = [], {}
    rows = {}
    for name in KNOB_SETS:
        rows[name] = []
        for row in knob_rows[name]:
            row = tuple(int(v) for v in row)
            if row not in index:
                index[row] = len(plans)
                plans.append(list(row))
            rows[name].append(index[row])
    return {"fields": list(PLAN_FIELDS), "cases": [c["name"] for c in CASES], "ws_elems": [int(v) for v in ws_elems],
            "plans": plans, "rows": rows}


def dump(table):
    body = ",\n".join('  %s: %s' % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in table.items() if k != "plans")
    plans = ",\n".join("    " + json.dumps(p, separators=(",", ":")) for p in table["plans"])
    return "{\n%s,\n  \"plans\": [\n%s\n  ]\n}\n" % (body, plans)


def plan_table():
    """The table as the tree's library plans it (as_conv2d_plan, every knob set passed explicitly, one process)."""
    sys.path.insert(0, os.path.join(HERE, "..", "..", "any-stereo_amd"))
    from anystereo import _lib as L
    lib = L.load()
    ws_elems = [lib.as_conv_ws_elems(c["B"], c["Cout"], *out_plane(c)) for c in CASES]
    knob_rows = {}
    was = lib.as_get_fast16()
    try:
        for name, over in KNOB_SETS.items():
            knobs = L.ConvKnobs(**dict(KNOB_DEFAULTS, **over))
            knob_rows[name] = []
            for c, n_ws in zip(CASES, ws_elems):
                lib.as_set_fast16(c["fast16"])
                d, plan = descriptor(L, c, n_ws), L.ConvPlan()
                rc = lib.as_conv2d_plan(C.byref(d), C.byref(knobs), C.byref(plan))
                assert rc == 0, (c["name"], name, rc, lib.as_last_error_string())
                knob_rows[name].append([getattr(plan, f) for f in PLAN_FIELDS])
    finally:
        lib.as_set_fast16(was)
    return pack_table(knob_rows, ws_elems)


if __name__ == "__main__":
    text = dump(plan_table())
    if "--check" in sys.argv:
        same = os.path.exists(PATH) and open(PATH).read() == text
        print("conv_plans.json", "matches" if same else "DIFFERS from", "the tree's as_conv2d_plan")
        sys.exit(0 if same else 1)
    open(PATH, "w").write(text)
    print("wrote", PATH, len(text), "bytes")
