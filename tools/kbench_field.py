"""What a StereoField saves, and the interpolation baseline's resize kernel (models/field.py, csrc/resize_disp.hip).

At cfg 2 (IGEV, 960x540, 32 GRU iterations, whole-pass hipGraph as bench.py runs it), host wall time around a synchronised call:
    forward        model(...): the graph replay and the clone of its result
    encode         model.encode(...): the replay of the loop alone and the clones of the kept state
    first query    field.query on a fresh field: the rows of both upsampler inputs, then the tail (eager launches)
    later query    the same field again: the tail alone
    32-point curve encode(at=1..32) + 32 queries, in units of `forward` (without a field: one forward per point)
as_resize_disp at the cfg-3 (384x1248 -> 750x2484, x2) and cfg-5 (1344x1920 -> 1988x2880, x1.5) sizes: N launches in one hipGraph, per
launch, against the byte floor 4 * N * (hc * wc + H * W) at the HBM rate tools/kbench_pointwise.py uses, and the `.cpu()` +
F.interpolate(mode='bicubic') path it replaces (host wall time, the copy included).
    python tools/kbench_field.py [--out profiles/field_kbench.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "any-stereo_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from anystereo import ops  # noqa: E402
from anystereo.harness.query import query_plan  # noqa: E402
from anystereo.harness.synthetic import det_uniform as U  # noqa: E402
from anystereo.harness.workloads import WORKLOADS, build_inputs, build_model  # noqa: E402

REPS, N, HBM = 9, 20, 6.29e12
DEV = "cuda:0"


def wall(fn, reps=REPS, before=None):
    """Median [min .. max] host milliseconds of fn() between two synchronisations; before() runs untimed in front of each."""
    ts = []
    for _ in range(reps):
        arg = before() if before is not None else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg) if before is not None else fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], f"{ts[len(ts) // 2]:8.3f} [{ts[0]:8.3f} .. {ts[-1]:8.3f}]"


def field_table(lines):
    wl = WORKLOADS["cfg2"]
    model, _ = build_model(wl, device=DEV)
    i1, i2, coord, scale = build_inputs(wl, device=DEV)
    model.enable_graph(True)
    model.graph_cache_size = 3
    every = tuple(range(1, wl.iters + 1))
    with torch.no_grad():
        for _ in range(2):  # captures
            model(i1, i2, iters=wl.iters, test_mode=True, hr_coord=coord.clone(), scale=scale)
            model.encode(i1, i2, iters=wl.iters).query(coord.clone(), scale)
            model.encode(i1, i2, iters=wl.iters, at=every)
        fwd, txt = wall(lambda: model(i1, i2, iters=wl.iters, test_mode=True, hr_coord=coord.clone(), scale=scale))
        lines.append(f"  cfg2 forward (graph)          ms {txt}")
        enc, txt = wall(lambda: model.encode(i1, i2, iters=wl.iters))
        lines.append(f"  cfg2 encode (graph)           ms {txt}")
        _, txt = wall(lambda f: f.query(coord.clone(), scale), before=lambda: model.encode(i1, i2, iters=wl.iters))
        lines.append(f"  cfg2 first query              ms {txt}")
        field = model.encode(i1, i2, iters=wl.iters)
        field.query(coord.clone(), scale)
        later, txt = wall(lambda: field.query(coord.clone(), scale))
        lines.append(f"  cfg2 later query              ms {txt}")
        curve, txt = wall(lambda: model.encode(i1, i2, iters=wl.iters, at=every).query(coord.clone(), scale, at="all"), reps=5)
        lines.append(f"  cfg2 32-point curve           ms {txt}   (encode at=1..32 + 32 queries) = {curve / fwd:.2f} forwards")
        lines.append(f"  a second query set costs {later / fwd * 100:.1f} % of a forward; encode + query = {(enc + later) / fwd * 100:.1f} % of forward")
    model.enable_graph(False)


def resize_table(lines):
    for name, (h, w, s, fixed) in (("cfg3", (375, 1242, 2, True)), ("cfg5", (1988, 2880, 1.5, False))):
        pl = query_plan(h, w, s, 32, fixed=fixed)
        crop, size = (pl.pad[0], pl.pad[2], pl.h_lr, pl.w_lr), (pl.h_want, pl.w_want)
        src = U((1, pl.h_pad, pl.w_pad), 5, -3, 200).to(DEV)
        out = torch.empty((1,) + size, device=DEV)
        ops.resize_disparity(src, crop, size, float(s), out=out)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(N):
                ops.resize_disparity(src, crop, size, float(s), out=out)
        ts = []
        for _ in range(REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / N)
        ts.sort()
        floor = 4 * (crop[2] * crop[3] + size[0] * size[1]) / HBM * 1e6
        top, left, hc, wc = crop

        def host():
            x = src[:, None, top:top + hc, left:left + wc].cpu()
            return F.interpolate(x * float(s), size, mode="bicubic", align_corners=False)
        _, txt = wall(host, reps=5)
        lines.append(f"  {name} as_resize_disp {pl.h_pad}x{pl.w_pad} crop {hc}x{wc} -> {size[0]}x{size[1]} x{s}: us {ts[len(ts) // 2]:7.1f} "
                     f"[{ts[0]:7.1f} .. {ts[-1]:7.1f}]  floor {floor:5.1f}  kernel/floor {ts[len(ts) // 2] / floor:4.1f}   "
                     f".cpu() + F.interpolate ms {txt} ({torch.get_num_threads()} threads)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [f"# host wall time between two synchronisations, median [min .. max] of {REPS} (curve: 5); resize: {N} launches per hipGraph "
             f"replay, {REPS} replays"]
    for table in (field_table, resize_table):
        n = len(lines)
        table(lines)
        print("\n".join(lines[n:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
