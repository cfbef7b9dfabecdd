"""CPU (-m "not gpu"): the schedule of as_conv2d as a value.  as_conv2d_plan maps (descriptor, knobs) to the kernel instantiation,
grid, LDS and schedule parameters without touching a device, so the whole dispatch — every knob set, in one process — is held
row for row to tests/golden/conv_plans.json, first recorded from the launches of as_conv2d itself.  as_conv2d runs that plan:
validate, plan, then the launch table keyed by the plan's tuple."""
import ctypes
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_golden_conv_plans", os.path.join(GOLDEN, "make_golden_conv_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "conv_plans.json")))


@pytest.fixture(scope="module")
def planned(gen):
    return gen.plan_table()


def _rows(table):
    for knobs, idx in table["rows"].items():
        for name, i in zip(table["cases"], idx):
            yield knobs, name, dict(zip(table["fields"], table["plans"][i]))


def test_conv_plan_matches_recorded_schedule(gen, recorded, planned):
    assert recorded["fields"] == list(gen.PLAN_FIELDS) and recorded["cases"] == [c["name"] for c in gen.CASES]
    assert list(recorded["rows"]) == list(gen.KNOB_SETS)
    got = {(k, n): r for k, n, r in _rows(planned)}
    n = 0
    for knobs, name, want in _rows(recorded):
        assert got[(knobs, name)] == want, f"{name} under {knobs or 'default'}: " + ", ".join(
            f"{f} {got[(knobs, name)][f]} (recorded {v})" for f, v in want.items() if got[(knobs, name)][f] != v)
        n += 1
    assert n == len(gen.KNOB_SETS) * len(gen.CASES) == len(got)
    # every conv_igemm_kernel / conv_split_kernel instantiation of the library's code object (golden/conv_kernels.txt: the global
    # function symbols of csrc/conv.hip compiled for gfx950, demangled) is some row's, and no row names another one.  (GRU_ZR with
    # Cout % 256 == 128 takes 64-channel tiles, a tile lying inside the z or the r half: the 1x1 kernel of that form is reached too.)
    def kernel(r):
        if not r["family"]:
            return "conv_igemm_kernel<%d, %d, %d>" % (r["KS"], r["TW"], r["epilogue"])
        return "conv_split_kernel<%d, %d, %d, %d, %d, %d, %s, %s>" % (
            r["KS"], r["TW"], r["BN"], r["epilogue"], r["NSUB"], r["S"], str(bool(r["FAST"])).lower(), str(bool(r["LEAN"])).lower())
    built = set(open(os.path.join(GOLDEN, "conv_kernels.txt")).read().split("\n")) - {""}
    reached = {kernel(r) for _, _, r in _rows(recorded)}
    assert len(built) == 91 and reached <= built, reached - built
    assert built == reached
    assert {r["dual"] for _, _, r in _rows(recorded)} == {0, 1, 2}


def test_conv_workspace_covers_every_plan(gen, recorded, planned):
    """Python sizes the split-K scratch by as_conv_ws_elems and the K split depends on it: the recorded values, and room for
    every plan's slabs."""
    assert planned["ws_elems"] == recorded["ws_elems"]
    ws = dict(zip(recorded["cases"], recorded["ws_elems"]))
    cases = {c["name"]: c for c in gen.CASES}
    split = 0
    for knobs, name, r in _rows(planned):
        c = cases[name]
        slab = c["B"] * ((c["Cout"] + 63) // 64 * 64) * r["H"] * r["W"]
        assert (r["ksplit"] if r["ksplit"] > 1 else 0) * slab <= ws[name], (knobs, name, r)
        assert r["finish"] == (r["ksplit"] > 1) and (r["ksplit"] == 1 or (c["ws"] and r["epilogue"] == 3))
        split += r["ksplit"] > 1
        assert r["lds"] <= 160 * 1024 and (not r["LEAN"] or r["lds"] <= 80 * 1024), (knobs, name, r)
        assert 0 < r["grid"] < 2 ** 31 and r["finish_grid"] < 2 ** 31 and r["block"] == (256 if r["LEAN"] or not r["family"] else 512)
    assert split > 100


def test_conv_plan_validates_like_conv2d(gen):
    """A bad descriptor: as_conv2d_plan returns what as_conv2d returns, with the same message, before anything is planned."""
    from anystereo import _lib
    lib = _lib.load()
    good = next(c for c in gen.CASES if c["name"] == "enc_c2d2")

    def bad(**kw):
        d = gen.descriptor(_lib, good, 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    zero, misaligned = _lib.ConvDesc(), bad()
    misaligned.src[0] = gen.FAKE + 4
    descs = [(zero, -1), (bad(KS=5), -1), (bad(Cin=65), -2), (bad(precision=2), -1), (bad(epilogue=1), -1), (bad(stride=2), -1),
             (bad(out_bs_coff=4), -2), (bad(out_coff2=100), -2), (bad(dual=0, epilogue=1, h=gen.FAKE, out2=gen.FAKE), -1),
             (bad(dual=0, stride=2, out_bs=0, KS=1), -1), (bad(wpack2=0), -1), (bad(H=1 << 16, W=1 << 16), -2), (misaligned, -1)]
    plan = _lib.ConvPlan()
    for d, code in descs:
        assert lib.as_conv2d_plan(ctypes.byref(d), None, ctypes.byref(plan)) == code
        msg = lib.as_last_error_string()
        assert lib.as_conv2d(ctypes.byref(d), None) == code and lib.as_last_error_string() == msg and msg
    assert lib.as_conv2d_plan(None, None, ctypes.byref(plan)) == lib.as_conv2d(None, None) == -1
    assert lib.as_conv2d_plan(ctypes.byref(bad()), None, None) == -1
    # NULL knobs = the process's (the defaults here, unless the environment says otherwise); explicit defaults plan the same
    assert lib.as_conv2d_plan(ctypes.byref(bad()), None, ctypes.byref(plan)) == 0
    if not any(k.startswith("AS_CONV_") for k in os.environ):
        explicit = _lib.ConvPlan()
        knobs = _lib.ConvKnobs(**gen.KNOB_DEFAULTS)
        assert lib.as_conv2d_plan(ctypes.byref(bad()), ctypes.byref(knobs), ctypes.byref(explicit)) == 0
        assert bytes(explicit) == bytes(plan)


def test_conv_launch_table_covers_every_plan(gen, recorded, planned):
    """as_conv2d_plan also fails when the launch table (csrc/conv.hip) has no entry for the planned tuple.  plan_table() asserts
    that it returns 0 for each (knob set, case) it plans, and those are the rows of the golden table: every plan there has a
    launcher."""
    assert planned["cases"] == recorded["cases"] and list(planned["rows"]) == list(recorded["rows"])
    assert sum(len(idx) for idx in planned["rows"].values()) == 17 * 276


def test_conv2d_bad_descriptor_launches_nothing(gen):
    """as_conv2d validates and plans before it launches, both halves of a dual call that runs as two calls included: a bad
    descriptor returns its validation code and message — never AS_ERR_LAUNCH, which is what a launch gives without a device, and
    never a launch with these fake pointers where there is one.  (The descriptors of test_conv_plan_validates_like_conv2d, and
    two-call dual launches whose FIRST half is good and whose second is not.)"""
    from anystereo import _lib
    lib = _lib.load()

    def bad(name, **kw):
        d = gen.descriptor(_lib, next(c for c in gen.CASES if c["name"] == name), 0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    misaligned = bad("enc_c2d2")
    misaligned.src[0] = gen.FAKE + 4
    g = "enc_c2d2"
    descs = [(_lib.ConvDesc(), -1), (bad(g, KS=5), -1), (bad(g, Cin=65), -2), (bad(g, precision=2), -1), (bad(g, epilogue=1), -1),
             (bad(g, stride=2), -1), (bad(g, out_bs_coff=4), -2), (bad(g, out_coff2=100), -2),
             (bad(g, dual=0, epilogue=1, h=gen.FAKE, out2=gen.FAKE), -1), (bad(g, dual=0, stride=2, out_bs=0, KS=1), -1),
             (bad(g, wpack2=0), -1), (bad(g, H=1 << 16, W=1 << 16), -2), (misaligned, -1),
             # fp32 precision: two calls.  The second source blocked, the second output window outside the tensor
             (bad("dual_fp32", src2_bs=1), -1), (bad("dual_fp32", out_coff2=100), -2), (bad("dual_fp32_1x1", out_coff2=65), -2)]
    plan = _lib.ConvPlan()
    for d, code in descs:
        assert lib.as_conv2d(ctypes.byref(d), None) == code
        msg = lib.as_last_error_string()
        assert msg and lib.as_conv2d_plan(ctypes.byref(d), None, ctypes.byref(plan)) == code
        assert lib.as_last_error_string() == msg
    first = bad("dual_fp32", dual=0)  # the first half of those two-call launches alone is a good descriptor
    assert lib.as_conv2d_plan(ctypes.byref(first), None, ctypes.byref(plan)) == 0


def test_conv_plan_structs_match_header():
    """ctypes mirrors of as_conv_knobs / as_conv_plan: field order and types as in the header."""
    import re

    from anystereo import _lib
    hdr = open(os.path.join(GOLDEN, "..", "..", "include", "anystereo_hip.h")).read()
    for name, mirror in (("as_conv_knobs", _lib.ConvKnobs), ("as_conv_plan", _lib.ConvPlan)):
        end = hdr.index("} %s;" % name)
        body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S).split("{", 1)[1]
        fields = []
        for decl in filter(None, (s.strip() for s in body.split(";"))):
            ctype, first = decl.split(None, 1)
            fields += [(n.strip(), {"int": ctypes.c_int, "int64_t": ctypes.c_int64}[ctype]) for n in first.split(",")]
        assert fields == list(mirror._fields_), name


def test_conv_plan_constants_are_the_dispatch_s():
    """The dispatch's constants, helpers and knob reader exist once under csrc/, in conv_plan.h; conv.hip, which includes it, holds
    no second definition and reads no AS_CONV_* variable itself."""
    import re
    csrc = os.path.join(GOLDEN, "..", "..", "any-stereo_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))}
    hip, hdr = texts["conv.hip"], texts["conv_plan.h"]
    assert 'getenv("AS_CONV_' not in hip and '#include "conv_plan.h"' in hip
    assert [f for f, t in texts.items() if re.search(r'"AS_CONV_[A-Z0-9_]+"', t)] == ["conv_plan.h"]  # the names conv_knobs() reads
    defs = [r"constexpr int %s\b" % n for n in ("kNumCU", "kEpiPartial", "kBM", "kBN", "kSplitKC")]
    defs += [r"^[\w:&* ]*\b%s\(" % n for n in ("conv_cout_pad", "conv_pick_ksplit", "conv_ksplit_cap", "conv_split_lds", "conv_knobs")]
    for pat in defs:
        found = {f: len(re.findall(pat + r"[^;\n]*(?:=|\{)", t, flags=re.M)) for f, t in texts.items()}
        assert {f: n for f, n in found.items() if n} == {"conv_plan.h": 1}, (pat, found)
    kc = dict(re.findall(r"template <> struct ConvCfg<(\d)> \{ static constexpr int KC = (\d+); \};", hip))
    assert kc == {"3": "8", "1": "32"} and "return KS == 3 ? 8 : 32;" in hdr
    assert "static_assert(ConvCfg<3>::KC == conv_kc(3) && ConvCfg<1>::KC == conv_kc(1)" in hip
