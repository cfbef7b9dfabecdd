"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py: the committed PIL fixture as parameter objects, and the
constructed batches both suites run.  A helper module (like tests/_conv_cases.py); it imports neither PIL nor the reference."""
import os

import numpy as np
import torch

from anystereo.harness import augment as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment_photometric.npz")


def fixture_sets():
    """[(name, image1 [1,3,H,W] uint8, image2, [SampleParams], gamma_lut or None, out1, out2)] of tests/golden/augment_photometric.npz."""
    z = np.load(GOLDEN)
    out = []
    for i in range(len(z["pair"])):
        k = int(z["pair"][i])
        ims = [A.ImageParams(tuple(z["order"][i, j]), *[float(v) for v in z["factor"][i, j]], int(z["hue_shift"][i, j]),
                             float(z["gamma"][i, j, 0]), float(z["gamma"][i, j, 1])) for j in range(2)]
        rects = tuple(tuple(int(v) for v in z["rects"][i, r]) for r in range(int(z["n_rects"][i])))
        sp = A.SampleParams(ims[0], ims[1], bool(z["shared"][i]), rects)
        lut = None if bool((z["gamma"][i] == 1.0).all()) else torch.from_numpy(A.gamma_table([sp]))
        t = lambda name: torch.from_numpy(z[name]).unsqueeze(0).contiguous()  # noqa: E731
        out.append((f"set{i}", t(f"in1_{k}"), t(f"in2_{k}"), [sp], lut, t(f"out1_{i}"), t(f"out2_{i}")))
    return out


def random_pair(batch: int, h: int, w: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (batch, 3, h, w), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (batch, 3, h, w), generator=g, dtype=torch.uint8))


def mixed_params(batch: int, h: int, w: int):
    """`batch` samples that differ in everything: shared and asymmetric, another order per sample and per image, contrast first
    (sample 0) and last (sample 1), a contrast factor of exactly 1 (sample 2: no grey sums), samples without, with one and with two
    rectangles, rectangles across both borders."""
    out = []
    for b in range(batch):
        o1, o2 = A.ORDERS[(6 + 7 * b) % 24], A.ORDERS[(23 - 5 * b) % 24]   # b = 0: (1, 0, 2, 3); b = 1: (2, 0, 3, 1) ...
        if b == 1:
            o1 = (0, 2, 3, 1)
        f1 = (0.6 + 0.2 * (b % 5), 1.0 if b == 2 else 1.4 - 0.15 * (b % 7), 0.8 + 0.1 * (b % 7))
        f2 = (1.3 - 0.1 * (b % 8), 0.7 + 0.1 * (b % 8), 1.4 - 0.2 * (b % 6))
        rects = [(), ((w - 3, h - 2, 50, 50),), ((0, 0, max(1, w // 2), max(1, h // 2)), (w // 3, h // 3, w, 2))][b % 3]
        out.append(A.SampleParams(A.ImageParams(o1, *f1, (37 * b + 1) % 256, 0.8 + 0.1 * b, 1.0 + 0.05 * b),
                                  A.ImageParams(o2, *f2, (255 - 50 * b) % 256, 1.2 - 0.1 * b, 1.0), shared=(b % 2 == 0), rects=rects))
    assert out[0].image1.order[0] == A.CONTRAST and (batch < 2 or out[1].image1.order[3] == A.CONTRAST)
    return out


def hue_only(shift1: int, shift2: int):
    return [A.SampleParams(A.ImageParams(hue_shift=shift1), A.ImageParams(hue_shift=shift2), shared=False)]


def all_colours():
    """uint8 [1,3,4096,4096]: every RGB colour once."""
    v = torch.arange(1 << 24, dtype=torch.int32).view(4096, 4096)
    return torch.stack([(v >> 16), (v >> 8) & 255, v & 255]).to(torch.uint8).unsqueeze(0).contiguous()
