"""`photometric_pair` (csrc/augment/augment.hip) at the cfg-4 training shape and at 540 x 960 against its byte floor, the numpy
restatement and, where PIL can be imported, the PIL calls it replaces.

    python tools/kbench_augment.py [--out profiles/augment_kbench.txt]

Rows: B = 4 at 160 x 320 and B = 1 at 540 x 960, uint8 -> uint8 and fp32 -> fp32, with the parameters `draw_params(PhotoSpec.flow())`
gives (a mix of shared and asymmetric samples, with and without rectangles), and one row per shape with identity parameters and no
rectangle (one launch: the write-out alone).

`us` = device events around repeated warm calls of the Python op (allocations, parameter table and ctypes call included), median of
the blocks.  `launches` = kernels of one call.  `floor` = (bytes of both inputs read once + bytes of both outputs written) at the
bandwidth the other kbench files use; the grey pass reads the inputs a second time and the rectangles write a little twice, which the
floor does not count.  `host us` = `photometric_pair_host` on CPU tensors plus the upload of its result; `PIL us` = the literal
PIL / numpy calls per sample (uint8 rows only), host clock, best of 2 — the data path of a loader process, not the code under test.
Nothing is asserted on these numbers.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "any-stereo_amd")]

HBM_BPS = 6.3e12
LAUNCH_US = 3.0


def _events(fn, reps, blocks):
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
    return sorted(out)[len(out) // 2]


def _best(fn, n=2):
    best = None
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e6
        best = dt if best is None else min(best, dt)
    return best


def _launches(params):
    """Kernels of one call, as aug_photometric_pair decides them per chunk of 8 samples."""
    n = 0
    for c0 in range(0, len(params), 8):
        chunk = params[c0:c0 + 8]
        n += 1 + any(sp.of(i).contrast != 1.0 for sp in chunk for i in (0, 1)) + any(sp.rects for sp in chunk)
    return n


def _pil_pair(i1, i2, params):
    """color_transform + eraser_transform by the PIL / numpy calls themselves; None when PIL is not there."""
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return None
    import numpy as np

    def jitter(arr, p):
        im = Image.fromarray(arr)
        for op in p.order:
            if op == 0:
                im = ImageEnhance.Brightness(im).enhance(p.brightness)
            elif op == 1:
                im = ImageEnhance.Contrast(im).enhance(p.contrast)
            elif op == 2:
                im = ImageEnhance.Color(im).enhance(p.saturation)
            else:
                h, s, v = im.convert("HSV").split()
                np_h = np.array(h, dtype=np.uint8)
                np_h += np.uint8(p.hue_shift)
                im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
        gamma_map = [int((255 + 1 - 1e-3) * p.gain * pow(e / 255.0, p.gamma)) for e in range(256)] * 3
        return np.array(im.point(gamma_map))

    outs = []
    for b, sp in enumerate(params):
        a1, a2 = (np.ascontiguousarray(t[b].permute(1, 2, 0).numpy()) for t in (i1, i2))
        if sp.shared:
            a1, a2 = np.split(jitter(np.concatenate([a1, a2], axis=0), sp.image1), 2, axis=0)
        else:
            a1, a2 = jitter(a1, sp.image1), jitter(a2, sp.image2)
        a2 = np.array(a2)
        if sp.rects:
            mean = np.mean(a2.reshape(-1, 3), axis=0)
            for x0, y0, dx, dy in sp.rects:
                a2[y0:y0 + dy, x0:x0 + dx, :] = mean
        outs.append((a1, a2))
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from anystereo import _augment_lib
    from anystereo.harness import augment as A
    assert torch.cuda.is_available(), "kbench_augment needs a GPU"
    dev = torch.device("cuda:0")
    lines = ["python tools/kbench_augment.py --reps %d --blocks %d" % (a.reps, a.blocks),
             "device: %s; library: %s" % (torch.cuda.get_device_name(0), _augment_lib.library_info()),
             "floor = (inputs read once + outputs written) / %.1f TB/s; below %.0f us a row is launch-bound; host = numpy restatement "
             "+ upload; PIL = the PIL / numpy calls per sample (no upload)" % (HBM_BPS / 1e12, LAUNCH_US),
             "", "%-44s %9s %8s %9s %9s %9s %11s %11s %6s" % ("row", "bytes", "launches", "floor us", "us", "of floor", "host us", "PIL us", "equal")]
    for label, bsz, h, w in (("cfg4 B=4 160x320", 4, 160, 320), ("cfg2 B=1 540x960", 1, 540, 960)):
        g = torch.Generator().manual_seed(1)
        u1 = torch.randint(0, 256, (bsz, 3, h, w), generator=g, dtype=torch.uint8)
        u2 = torch.randint(0, 256, (bsz, 3, h, w), generator=g, dtype=torch.uint8)
        drawn = A.draw_params(A.PhotoSpec.flow(), 1, 0, bsz, h, w)
        if not any(sp.rects for sp in drawn):   # the row is to hold all three launches
            drawn[0] = A.SampleParams(drawn[0].image1, drawn[0].image2, drawn[0].shared, ((w // 3, h // 3, 75, 75),))
        plain = [A.SampleParams(A.ImageParams(order=(3, 0, 1, 2)), A.ImageParams(order=(3, 0, 1, 2)))] * bsz
        for kind, params, dt in (("flow u8->u8", drawn, torch.uint8), ("flow f32->f32", drawn, torch.float32), ("identity u8->u8", plain, torch.uint8)):
            i1, i2 = (u1, u2) if dt == torch.uint8 else (u1.float(), u2.float())
            d1, d2 = i1.to(dev), i2.to(dev)
            es = 1 if dt == torch.uint8 else 4
            nbytes = 2 * bsz * 3 * h * w * es * 2
            us = _events(lambda: A.photometric_pair(d1, d2, params, out_dtype=dt), a.reps, a.blocks)
            got = A.photometric_pair(d1, d2, params, out_dtype=dt)
            want = A.photometric_pair_host(i1, i2, params, out_dtype=dt)
            same = all(bool(torch.equal(x.cpu(), y)) for x, y in zip(got, want))

            def host():
                for t in A.photometric_pair_host(i1, i2, params, out_dtype=dt):
                    t.to(dev)
                torch.cuda.synchronize()
            host_us = _best(host)
            pil_us = None
            if dt == torch.uint8 and _pil_pair(u1[:1, :, :8, :8], u2[:1, :, :8, :8], plain[:1]) is not None:
                pil_us = _best(lambda: _pil_pair(u1, u2, params))
                pil = _pil_pair(u1, u2, params)
                same = same and all(np.array_equal(want[j][b].permute(1, 2, 0).numpy(), pil[b][j]) for b in range(bsz) for j in (0, 1))
            floor = nbytes / HBM_BPS * 1e6
            lines.append("%-44s %9d %8d %9.2f %9.2f %8.1f%% %11.0f %11s %6s" % (
                f"{label} {kind}", nbytes, _launches(params), floor, us, 100.0 * floor / us, host_us,
                "-" if pil_us is None else "%.0f" % pil_us, "yes" if same else "NO"))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
