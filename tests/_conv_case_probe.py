"""Child process of test_conv_instantiations_gpu.py::test_lean_knob_instantiations_vs_fp64: the cases of tests/_conv_cases.py that
need a knob set, run under the environment the parent gave this process (csrc/conv.hip reads its AS_CONV_* knobs once, at the first
launch).  Every output tensor, whole, goes to argv[1] (.npz, keys "<case index>|<output>"), the launched conv kernels' names, in
order, to argv[1] + ".json".  Nothing is compared here: the parent holds the outputs to fp64 and the names to the plan."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "any-stereo_amd")):
    sys.path.insert(0, p)
import _conv_cases as cc  # noqa: E402

cases = [c for c in cc.CASES if c["knobs"]]
outs, kernels = cc.run_cases(cases, "cuda:0")
np.savez(sys.argv[1], **{"%d|%s" % (cc.CASES.index(c), k): v.numpy() for c, out in zip(cases, outs) for k, v in out.items()})
json.dump(kernels, open(sys.argv[1] + ".json", "w"))
print("saved", len(cases), "cases,", len(kernels), "launches")
