"""GPU (-m gpu): every instantiation of csrc/conv.hip (the 91 of tests/golden/conv_kernels.txt) computes its convolution.  tests/_conv_cases.py holds one small case per instantiation — partial tiles along both axes, channel
counts off the K chunk and off the 64-channel tile, concatenated and blocked sources, K splits, dual launches; its shapes rest on
the planner's arithmetic alone and test_conv_cases_cpu.py holds each to its name.  For every case here:
  * the launch is an ops.conv2d call on det_uniform operands, every output passed in pre-filled (out: a channel window [4, 4 + Cout)
    of a tensor filled with 7.0; out2, dual outputs and the blocked copy — requested wherever the form allows one, as channels
    [8, 8 + C) of a BS8 of C + 16 channels — filled with NaN), and whatever surrounds a window must still hold its fill;
  * the reference is torch.nn.functional.conv2d in float64 on the same fp32 values with the epilogue written out in torch from the
    header's AS_EPI_* definitions; RELU_TAPS: the nine planes per 64-channel tile, and their value through ops.tap_shift_sum;
  * FAST (the one-MFMA fp16 mode) is held to the same reference on the operands rounded to fp16 (x.half(), w.half(): all that
    kernel reads of them), which leaves its fp32 accumulation — a sharp expectation instead of test_reduced_precision_mode's band;
  * the kernels really launched (names and order from the profiler's kernel trace, finish launches and the two calls of an unfused
    dual launch included) are the plan's.
Bounds, relative to the reference tensor's maximum with no absolute term: 1e-5 (the conv parity tests' bound), RELU_TAPS 2e-5 (as
test_conv_relu_taps_epilogue; planes and tap_shift_sum alike), blocked copies + 2^-21 for the record pairs
(test_conv_blocked_split_link_is_bit_identical).  FAST against the rounded-operand reference is held to the exact modes' 1e-5 in
every family (epilogue x NSUB x K split); largest error / maximum measured on the MI355X per family:
  LINEAR nsub1 whole-K 2.7e-07     LINEAR nsub2 whole-K 3.0e-07     LINEAR nsub1 ksplit 2.5e-07
  GRU_ZR nsub1 whole-K 2.3e-07     GRU_ZR nsub2 whole-K 3.3e-07
  GRU_Q nsub1 whole-K 6.0e-07      GRU_Q nsub2 whole-K 4.9e-07      GRU_Q nsub1 ksplit 5.4e-07
  RELU_TAPS nsub1 whole-K 2.7e-07  RELU_TAPS nsub2 whole-K 2.5e-07
(the exact modes' largest: 1.1e-06, GRU_Q; no FAST K-split case falls to GRU_ZR).  The default-knob cases run once, in this process; the LEAN kernels with one sub-tile need
AS_CONV_LEAN=2, which a process reads once, so they run in one child process (tests/_conv_case_probe.py)."""
import functools
import json
import os
import subprocess
import sys

import pytest

import _conv_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DEFAULT = [c for c in cc.CASES if not c["knobs"]]
KNOBBED = [c for c in cc.CASES if c["knobs"]]
RTOL, RTOL_TAPS = 1e-5, 2e-5  # FAST vs the rounded-operand reference keeps RTOL in every family (docstring)


@pytest.fixture(scope="module")
def launched():
    """Every default-knob case, run once under one profiler session: name -> (outputs, the conv kernels launched for the case)."""
    outs, kernels = cc.run_cases(DEFAULT, DEV)
    per, at = {}, 0
    for c, out in zip(DEFAULT, outs):
        n = len(cc.planned_kernels(cc.plan(c)))
        per[c["name"]] = (out, kernels[at:at + n])
        at += n
    per[None] = kernels
    return per


_WORST = {}  # case name -> (family, FAST, largest error / maximum over the case's outputs)


def _hold(c, out, kernels):
    plan = cc.plan(c)
    assert kernels == cc.planned_kernels(plan), (c["name"], kernels, cc.planned_kernels(plan))
    want = cc.expected(c, cc.operands(c))
    worst = cc.check_case(c, out, want, float("inf"))  # finite, fills intact; the figures are printed before the bound is held
    print("[conv] %-56s %-26s %s" % (c["name"], cc.family(c, plan), " ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    _WORST[c["name"]] = (cc.family(c, plan), c["fast16"], max(worst.values()))
    cc.check_case(c, out, want, RTOL_TAPS if c["epi"] == cc.TAPS else RTOL)


@pytest.mark.parametrize("name", [c["name"] for c in DEFAULT])
def test_instantiation_vs_fp64(name, launched):
    c = next(c for c in DEFAULT if c["name"] == name)
    _hold(c, *launched[name])


def test_every_launch_is_the_planned_one(launched):
    """The whole trace: no conv kernel beside the planned ones, in the planned order."""
    assert launched[None] == [k for c in DEFAULT for k in cc.planned_kernels(cc.plan(c))]


def test_lean_knob_instantiations_vs_fp64(tmp_path):
    """The cases that need {lean: 2}, in ONE child process with AS_CONV_LEAN=2 and every other AS_CONV_* variable stripped: the
    child writes its outputs and launched kernel names, this process holds them to fp64 and to the plan under those knobs."""
    import numpy as np
    assert all(c["knobs"] == cc.LEAN2 for c in KNOBBED)
    probe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_conv_case_probe.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AS_CONV_")}
    path = str(tmp_path / "lean2.npz")
    r = subprocess.run([sys.executable, probe, path], env=dict(env, AS_CONV_LEAN="2"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child failed ({r.returncode})\n{r.stdout[-1000:]}\n{r.stderr[-3000:]}"
    data, kernels = np.load(path), json.load(open(path + ".json"))
    assert kernels == [k for c in KNOBBED for k in cc.planned_kernels(cc.plan(c))]
    at, failed = 0, []
    for c in KNOBBED:
        pre = "%d|" % cc.CASES.index(c)
        out = {k[len(pre):]: data[k] for k in data.files if k.startswith(pre)}
        n = len(cc.planned_kernels(cc.plan(c)))
        try:
            _hold(c, out, kernels[at:at + n])
        except AssertionError as e:  # every case is held, so that one failure does not hide the next kernel's
            failed.append(str(e))
        at += n
    assert not failed, "\n".join(failed)


def test_fast_error_per_family():
    """The largest FAST error per family (epilogue x NSUB x K split) against the rounded-operand fp64 reference, as measured by the
    tests above in this run: printed for the module docstring, and within that family's bound."""
    fams = {}
    for fam, fast, err in _WORST.values():
        key = (fam, bool(fast))
        fams[key] = max(fams.get(key, 0.0), err)
    for (fam, fast), err in sorted(fams.items()):
        print("[conv family] %-5s %-28s %.2e" % ("FAST" if fast else "exact", fam, err))
    for (fam, fast), err in fams.items():
        assert not fast or err <= (RTOL_TAPS if fam.startswith("RELU_TAPS") else RTOL), (fam, err)
