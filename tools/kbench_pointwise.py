"""Stand-alone time of every 1x1 convolution shape of the cfg-2 pre-loop (tools/preloop_convs.py) on as_conv2d and on the
streaming kernel (as_conv1x1_stream): N launches captured in one hipGraph per path (no host time between kernels), REPS
replays each, the two paths alternating; median and range per launch.  The table ops.pw_stream_route rests on.
    python tools/kbench_pointwise.py [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "any-stereo_amd"))
import torch  # noqa: E402

from anystereo import _lib as L  # noqa: E402
from anystereo import ops  # noqa: E402
from anystereo.harness.synthetic import det_uniform as U  # noqa: E402

# (Cin, Cout, B, H, W): the inventory's 1x1 launches, largest maps first
SHAPES = [(16, 96, 2, 272, 480), (32, 16, 2, 272, 480), (64, 96, 1, 272, 480), (24, 144, 2, 136, 240), (96, 96, 2, 136, 240),
          (144, 24, 2, 136, 240), (96, 24, 2, 136, 240), (96, 128, 1, 136, 240), (96, 48, 1, 136, 240), (48, 8, 1, 136, 240),
          (32, 16, 1, 1, 195840), (32, 192, 2, 68, 120), (192, 32, 2, 68, 120), (144, 32, 2, 68, 120), (128, 128, 1, 68, 120),
          (64, 32, 1, 68, 120), (32, 16, 1, 68, 120), (64, 32, 1, 1, 24480), (64, 384, 2, 34, 60), (384, 64, 2, 34, 60),
          (96, 576, 2, 34, 60), (576, 96, 2, 34, 60), (192, 96, 1, 34, 60), (384, 96, 2, 34, 60), (128, 128, 1, 34, 60),
          (192, 64, 2, 34, 60), (96, 32, 1, 34, 60)]
N, REPS = 20, 7


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(N):
            fn()
    return g


def timed(g):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e3 / N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    ops.set_precision("split")
    lines = [f"# us per launch, {N} launches per hipGraph replay, {REPS} replays per path alternating: median [min .. max]",
             f"# {'shape':28s} {'as_conv2d':>24s} {'streaming':>24s}  ratio  floor_us  route"]
    for cin, cout, b, h, w in SHAPES:
        x = U((b, cin, h, w), 1, -2, 2).to(dev)
        wt = (U((cout, cin, 1, 1), 2) * (3.0 / cin) ** 0.5).to(dev)
        pack = ops.PackedConv().get([wt], [None])
        out_a, out_b = torch.empty((b, cout, h, w), device=dev), torch.empty((b, cout, h, w), device=dev)
        name = f"{cin}->{cout} {b}x{h}x{w}"
        plan = ops.conv_plan({"B": b, "H": h, "W": w, "Cin": cin, "Cout": cout, "KS": 1})
        ga = graph_of(lambda: ops.conv2d([x], pack, act=L.ACT_RELU6, out=out_a))
        try:
            gb = graph_of(lambda: ops.conv1x1([x], pack, act=L.ACT_RELU6, out=out_b, force=True))
        except RuntimeError:
            ta = sorted(timed(ga) for _ in range(REPS))
            lines.append(f"  {name:28s} {ta[REPS // 2]:8.1f} [{ta[0]:6.1f} .. {ta[-1]:6.1f}] {'not streamable (ksplit %d)' % plan['ksplit']:>24s}")
            print(lines[-1], flush=True)
            continue
        assert torch.equal(out_a, out_b), name
        ta, tb = [], []
        for _ in range(REPS):
            ta.append(timed(ga))
            tb.append(timed(gb))
        ta.sort(), tb.sort()
        floor = (b * (cin + cout) * h * w * 4) / 6.29e12 * 1e6
        route = ops.pw_stream_route(cin, cout, b * h * w)
        lines.append(f"  {name:28s} {ta[REPS // 2]:8.1f} [{ta[0]:6.1f} .. {ta[-1]:6.1f}] {tb[REPS // 2]:8.1f} [{tb[0]:6.1f} .. {tb[-1]:6.1f}]"
                     f"  {ta[REPS // 2] / tb[REPS // 2]:5.2f}  {floor:7.1f}  {'stream' if route else 'conv2d'}")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
