"""CPU (-m "not gpu"): the case table of tests/_conv_cases.py names exactly the instantiations of csrc/conv.hip.  Each
case is planned (as_conv2d_plan) under its own explicit knobs and its fast16 flag, so a schedule change that moves a case to
another kernel — and with it drops that kernel from tests/test_conv_instantiations_gpu.py — fails here, without a GPU."""
import os

import pytest

import _conv_cases as cc


@pytest.fixture(scope="module")
def plans():
    return {c["name"]: cc.plan(c) for c in cc.CASES}


@pytest.mark.parametrize("name", [c["name"] for c in cc.CASES])
def test_case_selects_the_instantiation_it_is_named_for(name, plans):
    c = next(c for c in cc.CASES if c["name"] == name)
    p = plans[name]
    assert cc.kernel_name(p) == name, (c, p)
    # the knob set is needed: default knobs wherever they reach the instantiation
    if c["knobs"]:
        assert c["knobs"] == cc.LEAN2 and cc.kernel_name(cc.plan(dict(c, knobs={}))) != name
    # GRU_ZR: a channel tile lies inside the z or the r half
    assert c["epi"] != cc.ZR or (c["Cout"] // 2) % p["BN"] == 0 or not p["family"], p
    # at least two K chunks per slice wherever K is split
    assert p["ksplit"] == 1 or p["chunks"] // p["ksplit"] >= 2, p
    # at least two pixel tiles along each axis, the last partial in both (a 1x1 kernel sees one flattened row)
    th = (128 if p["family"] else 64) // p["TW"]
    assert p["tiles_x"] >= 2 and p["W"] % p["TW"], p
    assert c["KS"] == 1 or (p["tiles_y"] >= 2 and p["H"] % th), p
    # ops.conv2d passes the sources as they are only while no K chunk straddles two of them; blocked sources in multiples of 8
    kc = 16 if c["prec"] else (8 if c["KS"] == 3 else 32)
    assert all(abs(ch) % kc == 0 for ch in c["srcs"][:-1]) and all(ch % 8 == 0 for ch in c["srcs"] if ch < 0), c["srcs"]


def test_cases_cover_every_instantiation(plans):
    built = set(open(os.path.join(cc.GOLDEN, "conv_kernels.txt")).read().split("\n")) - {""}
    assert len(built) == 91 and {c["name"] for c in cc.CASES} == built and len(cc.CASES) == 91
    knobbed = [c["name"] for c in cc.CASES if c["knobs"]]
    assert len(knobbed) == 10 and all(n.endswith(", 1, 1, false, true>") for n in knobbed), knobbed  # the LEAN kernels with NSUB = 1


def test_cases_cover_the_edges(plans):
    """What the table must hold across its rows (the shapes at which a kernel can go wrong)."""
    rows = [(c, plans[c["name"]]) for c in cc.CASES]
    # an odd pixel-tile count under two sub-tiles per block: the last wide block's second sub-tile is empty
    assert any(p["NSUB"] == 2 and (p["tiles_x"] * p["tiles_y"]) % 2 for _, p in rows)
    assert any(p["NSUB"] == 2 and p["LEAN"] and (p["tiles_x"] * p["tiles_y"]) % 2 for _, p in rows)
    # Cin off the K chunk in every family; only fp32 sources end off it
    for fam, ks, kc in ((0, 3, 8), (0, 1, 32), (1, 3, 16), (1, 1, 16)):
        assert any(p["family"] == fam and c["KS"] == ks and sum(map(abs, c["srcs"])) % kc for c, p in rows), (fam, ks)
    # Cout off the 64-channel tile, under the tap epilogue too; concatenations of two and of three sources, fp32 and blocked
    assert {40, 100, 127} <= {c["Cout"] for c, _ in rows} and any(c["epi"] == cc.TAPS and c["Cout"] % 64 for c, _ in rows)
    for n in (2, 3):
        assert any(len(c["srcs"]) == n and c["srcs"][0] > 0 for c, _ in rows) and any(len(c["srcs"]) == n and c["srcs"][0] < 0 for c, _ in rows)
    # the K-split kernels store raw partial sums, so any epilogue can sit behind them: every conv_finish_kernel<epilogue> is launched
    assert {p["finish_epilogue"] for _, p in rows if p["finish"]} == {cc.LIN, cc.ZR, cc.Q}
    assert {c["residual"] for c, p in rows if c["epi"] == cc.LIN and p["finish"]} == {False, True}
    assert {c["residual"] for c, p in rows if c["epi"] == cc.LIN and not p["finish"]} == {False, True}
    # dual launches: fused and as two calls, with a window and with outputs of their own
    assert {p["dual"] for _, p in rows} == {0, 1, 2} and {c["dual"] for c, _ in rows} == {None, "bs", "f32", "sep"}
    # every case is small: the fp64 reference of the whole table takes seconds
    macs = [c["B"] * p["H"] * p["W"] * sum(map(abs, c["srcs"])) * c["KS"] ** 2 * c["Cout"] for c, p in rows]
    assert max(macs) < 0.8e9 and sum(macs) < 14e9, (max(macs), sum(macs))
