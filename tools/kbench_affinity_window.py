"""Stand-alone time of the window affinity kernels (as_affinity_window, as_affinity_window_bwd; csrc/affinity_window.hip): forward at
the two cfg-2 upsampler inputs, backward at the cfg-4 per-rank ones, windows 3, 5 and 7.  N launches captured in one hipGraph per path
(no host time between kernels), REPS replays each, the paths alternating; median and range per launch.  Beside each time: the byte
floor (input + norms + result planes once, at the HBM rate tools/kbench_pointwise.py uses), the ATen statement of the same function
(normalize, unfold, dot, clamp — for the backward its eager forward + backward under autograd) and, for window 3, the 3x3 kernels
the default model runs.
    python tools/kbench_affinity_window.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "any-stereo_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from anystereo import ops  # noqa: E402
from anystereo.harness.synthetic import det_uniform as U  # noqa: E402

FORWARD = [(1, 176, 136, 240), (1, 32, 272, 480)]  # cfg 2: cat(stem_4x, hidden) and stem_2x
BACKWARD = [(4, 176, 40, 80), (4, 32, 80, 160)]    # cfg 4, one rank
N, REPS, HBM = 20, 7, 6.29e12


def graph_of(fn, n=N):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g, n


def timed(gn):
    g, n = gn
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / n


def aten_affinity(x, win):
    b, c, h, w = x.shape
    xh = F.normalize(x, dim=1, p=2)
    u = F.unfold(xh, win, padding=win // 2).reshape(b, c, win * win, h, w)
    mid = win * win // 2
    nb = torch.cat((u[:, :, :mid], u[:, :, mid + 1:]), dim=2)
    return torch.cat((x, (nb * xh.unsqueeze(2)).sum(dim=1).clamp_min(0)), dim=1)


def aten_step_eager(x, g, win):
    """The ATen statement's forward + backward as eager launches between two events.  Not captured: an autograd graph recorded on
    the default stream must not be run while another stream captures."""
    xa = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    torch.autograd.grad(aten_affinity(xa, win), xa, g)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3


def fmt(ts):
    ts = sorted(ts)
    return f"{ts[len(ts) // 2]:9.1f} [{ts[0]:8.1f} .. {ts[-1]:8.1f}]"


def run(paths):
    """{name: graph} -> {name: formatted time}, the paths alternating."""
    ts = {k: [] for k in paths}
    for _ in range(REPS):
        for k, g in paths.items():
            ts[k].append(timed(g))
    return {k: fmt(v) for k, v in ts.items()}, {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"# us per launch pair (norm pass + tile kernel), {N} per hipGraph replay (ATen: 3), {REPS} replays per path alternating: "
             "median [min .. max]", "# forward = cat(x, affinity) [B,C+n,H,W]; backward = its gradient w.r.t. x on the live map"]
    for kind, shapes in (("forward", FORWARD), ("backward", BACKWARD)):
        for shape in shapes:
            b, c, h, w = shape
            x = U(shape, 1, -2, 2).to(dev)
            for win in (3, 5, 7):
                n = win * win - 1
                plane = b * h * w * 4
                if kind == "forward":
                    floor = plane * (c + 1 + c + n) / HBM * 1e6
                    paths = {"window": graph_of(lambda: ops.affinity_window(x, win, True)),
                             "aten": graph_of(lambda: aten_affinity(x, win), 3)}
                    if win == 3:
                        paths["3x3 kernel"] = graph_of(lambda: ops.structure_feature(x))
                else:
                    floor = plane * (c + 1 + n + 2 * (c + n)) / HBM * 1e6
                    out = ops.affinity_window(x, win, True)
                    g = U(tuple(out.shape), 2).to(dev)
                    paths = {"window": graph_of(lambda: ops.affinity_window_backward(x, out, g, win, True))}
                    if win == 3:
                        paths["3x3 kernel"] = graph_of(lambda: ops.affinity_backward(x, out, g, True))
                txt, med = run(paths)
                if kind == "backward":
                    txt["aten fwd+bwd (eager)"] = fmt([aten_step_eager(x, g, win) for _ in range(REPS)])
                lines.append(f"  {kind:8s} {b}x{c}x{h}x{w} win {win}  floor {floor:7.1f}  " + "  ".join(f"{k} {v}" for k, v in txt.items())
                             + f"  window/floor {med['window'] / floor:5.1f}")
                print(lines[-1], flush=True)
                del paths
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
