"""The two entry points of csrc/train_batch.hip (as_train_queries, as_low_disp) at the cfg-4 shapes against their byte floors and
against the host path they replace.  One JSON object on stdout (and in --out).

    python tools/kbench_train_batch.py [--out profiles/train_batch_kbench.json]
    python tools/kbench_train_batch.py --only sparse            # one mode, in this process

B = 4 samples of a 160 x 320 input (Q = 51 200 queries each), scales 1.0, 1.65, 2.3, 2.95, so the crops are 160 x 320, 264 x 528,
368 x 736 and 472 x 944 (dense_all needs N == Q: four 160 x 320 crops at scale 1).  Sparse modes: 40 % of a crop is <= 0, so V < Q
in the first sample and V > Q in the others.  Each mode runs in a child process of its own with a time limit; the parent never opens
the GPU and stops at the first failure.  Per mode:
    train_queries        device events around repeated warm calls, median of the blocks: `entry_us` = the C entry alone (outputs,
                         scratch and argument tables made once: the ctypes call and its launches), `op_us` = ops.train_queries
                         (with its four allocations and tables).  Back-to-back calls of launch-bound kernels measure the rate at
                         which the host issues them as much as the kernels, so no bandwidth is derived from them.  floor =
                         bytes / 6.3 TB/s with bytes = B x Q x (4 read + 8 + 4 + 4 written) in the dense modes, plus in the sparse
                         modes sum_b N_b x (4 read + 4 written) for the ordered pixel list (the crop read once, the list
                         written once) and B x Q x 4 for the list entries the queries read.  The kernels read the crop twice
                         (count, scatter) and gather 4-byte values from whole cache lines, so they cannot reach this floor.
    low_disp             as_low_disp / ops.low_disp to [B, 40, 80], the same two figures; floor = B x 40 x 80 x (16 read + 4 written) bytes: launch-bound
    device_path_host_us  harness.batches.build_train_batch on device crops, host clock between synchronisations
    replaced_*           the host path: train_queries_host / low_disp_host on CPU tensors (one thread, as a DataLoader worker
                         has) and the upload of their results (hr_coord, hr_disp, low_disp), host clock between
                         synchronisations.  This is the reference's work restated in torch, not the code under test.
A floor below 3 us is launch-bound by construction (one launch costs more than the traffic)."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

HBM_BPS = 6.3e12   # what the chip reaches on a streaming copy
LAUNCH_US = 3.0
MODES = ["dense", "dense_all", "sparse", "sparse_ordered"]
H_LR, W_LR = 160, 320
SCALES = [1.0, 1.65, 2.3, 2.95]


def _median(v):
    return sorted(v)[len(v) // 2]


def _events(fn, reps, blocks):
    """us per call: median over `blocks` of the device-event time of `reps` back-to-back calls."""
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps * 1e3)
    return _median(out), out


def _host(fn, reps, blocks):
    """us per call of a path with host work in it: host clock between synchronisations."""
    import torch
    fn()
    out = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return _median(out), out


def run_mode(mode, reps, blocks):
    import torch
    from anystereo import ops
    from anystereo.harness.batches import build_train_batch, low_disp_host, train_queries_host
    from anystereo.harness.synthetic import det_uniform, synthetic_pair
    assert torch.cuda.is_available(), "kbench_train_batch needs a GPU"
    dev = torch.device("cuda:0")
    scales = [1.0] * len(SCALES) if mode == "dense_all" else SCALES
    sizes = [(round(H_LR * s), round(W_LR * s)) for s in scales]
    lo = 0.5 if mode.startswith("dense") else -40.0
    b, q, hw = len(sizes), H_LR * W_LR, (H_LR // 4, W_LR // 4)
    host_crops = [det_uniform(s, 60 + i, lo, 60.0) for i, s in enumerate(sizes)]
    crops = [c.to(dev) for c in host_crops]
    i1, i2 = (t.to(dev) for t in synthetic_pair(len(sizes), H_LR, W_LR))
    seed = [0]

    def queries():
        seed[0] += 1
        return ops.train_queries(crops, q, mode, seed[0])

    # the C entries alone: outputs, scratch and argument tables made once, so a call is the ctypes call and its launches
    import ctypes as C
    from anystereo import _lib
    lib = _lib.load()
    ptrs, keep = _lib.ptr_array([c.data_ptr() for c in crops])
    hs, ws_ = (C.c_int * b)(*[s[0] for s in sizes]), (C.c_int * b)(*[s[1] for s in sizes])
    sc = (C.c_float * b)(*scales)
    m = ops.TRAIN_QUERY_MODES[mode]
    need = int(lib.as_train_queries_ws_bytes(hs, ws_, b, m))
    scratch = torch.empty(max(need, 4), device=dev, dtype=torch.uint8)
    o_coord, o_disp = torch.empty((b, q, 2), device=dev), torch.empty((b, 1, q), device=dev)
    o_index, o_nv = torch.empty((b, q), device=dev, dtype=torch.int32), torch.empty((b,), device=dev, dtype=torch.int32)
    o_scale, o_low = torch.empty((b, 1), device=dev), torch.empty((b,) + hw, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry_queries():
        seed[0] += 1
        rc = lib.as_train_queries(ptrs, hs, ws_, b, q, m, seed[0], vp(o_coord), vp(o_disp), vp(o_index), vp(o_nv), sc, vp(o_scale),
                                  vp(scratch), need, stream)
        assert rc == 0, lib.as_last_error_string()

    def entry_low():
        rc = lib.as_low_disp(ptrs, hs, ws_, sc, vp(o_low), b, hw[0], hw[1], stream)
        assert rc == 0, lib.as_last_error_string()

    tq_e, tq_e_all = _events(entry_queries, reps, blocks)
    ld_e, ld_e_all = _events(entry_low, reps, blocks)
    tq, tq_all = _events(queries, reps, blocks)
    ld, ld_all = _events(lambda: ops.low_disp(crops, scales, hw), reps, blocks)
    dev_path, dev_path_all = _host(lambda: build_train_batch(i1, i2, crops, scales, seed[0], mode=mode), max(1, reps // 4), blocks)

    torch.set_num_threads(1)

    def old_queries():
        seed[0] += 1
        coord, disp, _, _ = train_queries_host(host_crops, q, mode, seed[0])
        return coord.to(dev), disp.to(dev)

    def old_low():
        return low_disp_host(host_crops, scales, hw).to(dev)

    old_q, old_q_all = _host(old_queries, 2, 3)
    old_l, old_l_all = _host(old_low, 2, 3)

    # agreement at this size, on the draws of one seed
    got = ops.train_queries(crops, q, mode, 99)
    want = train_queries_host(host_crops, q, mode, 99)
    same = all(bool(torch.equal(g.cpu().view(torch.int32), w.contiguous().view(torch.int32))) for g, w in zip(got, want))
    same_low = bool(torch.equal(ops.low_disp(crops, scales, hw).cpu(), low_disp_host(host_crops, scales, hw)))

    n_sum = sum(h * w for h, w in sizes)
    tq_bytes = b * q * 20 + (n_sum * 8 + b * q * 4 if mode.startswith("sparse") else 0)
    ld_bytes = b * hw[0] * hw[1] * 20

    def entry(entry_us, entry_all, op_us, op_all, nbytes):
        floor = nbytes / HBM_BPS * 1e6
        return {"entry_us": round(entry_us, 2), "entry_blocks_us": [round(x, 2) for x in entry_all], "op_us": round(op_us, 2),
                "op_blocks_us": [round(x, 2) for x in op_all], "bytes": nbytes, "floor_us": round(floor, 3),
                "bound": "launch" if floor < LAUNCH_US else "HBM"}

    return {"mode": mode, "batch": b, "queries": q, "crops": [list(s) for s in sizes], "scales": scales,
            "valid_pixels": [int((c > 0).sum()) for c in host_crops],
            "launches_per_call": 4 if mode.startswith("sparse") else 1,
            "train_queries": entry(tq_e, tq_e_all, tq, tq_all, tq_bytes), "low_disp": entry(ld_e, ld_e_all, ld, ld_all, ld_bytes),
            "device_path_host_us": round(dev_path, 1), "device_path_host_blocks_us": [round(x, 1) for x in dev_path_all],
            "replaced_queries_us": round(old_q, 1), "replaced_queries_blocks_us": [round(x, 1) for x in old_q_all],
            "replaced_low_disp_us": round(old_l, 1), "replaced_low_disp_blocks_us": [round(x, 1) for x in old_l_all],
            "replaced_per_sample_ms": round((old_q + old_l) / b / 1e3, 2),
            "speedup_vs_replaced_path": round((old_q + old_l) / dev_path, 1),
            "bit_equal_to_host_restatement": same, "low_disp_bit_equal_to_host_restatement": same_low}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--only", default=None, choices=MODES, help="run this one mode here")
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.only:
        print(json.dumps(run_mode(a.only, a.reps, a.blocks)))
        return
    res = {"command": "python tools/kbench_train_batch.py", "reps": a.reps, "blocks": a.blocks, "hbm_GBps_assumed": HBM_BPS / 1e9,
           "launch_bound_below_floor_us": LAUNCH_US, "steps": []}
    for mode in MODES:
        cmd = [sys.executable, os.path.abspath(__file__), "--only", mode, "--reps", str(a.reps), "--blocks", str(a.blocks)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            res["error"] = f"{mode}: no result after {a.step_timeout} s"
            break
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            res["error"] = f"{mode}: exit {r.returncode}: {r.stderr[-800:]}"
            break  # nothing more is started on the GPU after a failure
        res["steps"].append(json.loads(lines[-1]))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if "error" in res:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
