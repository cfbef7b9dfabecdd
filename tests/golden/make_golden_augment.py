"""Makes tests/golden/augment_photometric.npz: the reference's photometric augmentation and eraser (augmentor.py:82-111) computed by
the literal PIL and numpy calls, for explicit parameters.

    python tests/golden/make_golden_augment.py

Imports PIL (12.2.0 when the committed file was made) and numpy, nothing of this project and nothing of the reference.  What
torchvision's ColorJitter / adjust_gamma do to a PIL image is written out call by call in `jitter` below; the hue shift is given as
the byte that is added to H.

Arrays: in1_<k>, in2_<k> uint8 [3,H,W] for the pairs k = 0 (24x40 random), 1 (37x53 random), 2 (24x40, image1 bright and image2 dark);
per set i: pair[i], shared[i], order[i,2,4], factor[i,2,3] (fp32), hue_shift[i,2], gamma[i,2,2] = (gamma, gain) per image, n_rects[i],
rects[i,2,4] = (x0, y0, dx, dy), and out1_<i>, out2_<i> uint8 [3,H,W].
"""
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
B, C, S, H = 0, 1, 2, 3


def jitter(arr, order, factor, shift, gamma, gain):
    """ColorJitter with the given order and factors, then AdjustGamma, on an [h, w, 3] uint8 array."""
    im = Image.fromarray(arr)
    for op in order:
        if op == B:
            im = ImageEnhance.Brightness(im).enhance(float(factor[0]))
        elif op == C:
            im = ImageEnhance.Contrast(im).enhance(float(factor[1]))
        elif op == S:
            im = ImageEnhance.Color(im).enhance(float(factor[2]))
        else:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.uint8(shift)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    gamma_map = [int((255 + 1 - 1e-3) * gain * pow(ele / 255.0, gamma)) for ele in range(256)] * 3
    return np.array(im.point(gamma_map), dtype=np.uint8)


def run(img1, img2, shared, order, factor, shift, gamma, rects):
    """img1, img2 [h, w, 3] -> the augmented pair, as color_transform and eraser_transform write it."""
    if shared:
        stack = jitter(np.concatenate([img1, img2], axis=0), order[0], factor[0], shift[0], *gamma[0])
        img1, img2 = np.split(stack, 2, axis=0)
    else:
        img1 = jitter(img1, order[0], factor[0], shift[0], *gamma[0])
        img2 = jitter(img2, order[1], factor[1], shift[1], *gamma[1])
    img2 = np.array(img2)
    if rects:
        mean_color = np.mean(img2.reshape(-1, 3), axis=0)
        for x0, y0, dx, dy in rects:
            img2[y0:y0 + dy, x0:x0 + dx, :] = mean_color
    return img1, img2


def sets():
    """(pair, shared, (order1, order2), (factor1, factor2), (shift1, shift2), ((gamma, gain), (gamma, gain)), rects)"""
    f32 = lambda *v: tuple(float(np.float32(x)) for x in v)  # noqa: E731
    one = (1.0, 1.0)
    orders = list(itertools.permutations(range(4)))
    out = []
    shifts = (0, 1, 128, 255, 37, 200)
    for i, o in enumerate(orders):   # all 24 orders on the small pair, every second one asymmetric with another order for image2
        fa = f32(0.6 + 0.035 * i, 1.4 - 0.03 * i, 0.7 + 0.03 * i)
        fb = f32(1.4 - 0.02 * i, 0.65 + 0.03 * i, 1.35 - 0.025 * i)
        rects = [(), ((5, 3, 10, 8),), ((30, 20, 50, 50), (2, 2, 6, 30))][i % 3]
        out.append((0, i % 2 == 0, (o, orders[23 - i]), (fa, fb), (shifts[i % 6], shifts[(i + 3) % 6]), (one, one), rects))
    id4 = (0, 1, 2, 3)
    out += [
        (1, True, (id4, id4), (f32(0, 0, 0),) * 2, (0, 0), (one, one), ()),                      # f = 0: black, the level, grey
        (1, True, ((1, 0, 2, 3),) * 2, (f32(1, 0, 1),) * 2, (0, 0), (one, one), ()),             # contrast 0 alone: the level everywhere
        (1, True, (id4, id4), (f32(1, 1, 1),) * 2, (0, 0), (one, one), ()),                      # the identity
        (1, False, (id4, (3, 2, 1, 0)), (f32(1.4, 1.4, 1.4), f32(2, 2, 2)), (0, 0), (one, one), ()),   # f > 1 on saturating pixels
        (1, True, ((2, 3, 0, 1),) * 2, (f32(1.17, 1.4, 1.3),) * 2, (1, 1), (one, one), ()),
        (1, False, ((3, 0, 1, 2), (3, 1, 0, 2)), (f32(1, 1, 1), f32(1, 1, 1)), (128, 255), (one, one), ()),   # hue alone
        (1, False, ((3, 0, 1, 2), (0, 3, 1, 2)), (f32(0.9, 1.1, 0.8), f32(1.2, 0.7, 1.1)), (0, 1), (one, one), ()),
        (1, True, (id4, id4), (f32(0.83, 1.17, 1.0),) * 2, (37, 37), ((0.8, 1.0),) * 2, ()),    # gamma
        (1, True, (id4, id4), (f32(1, 1, 1),) * 2, (0, 0), ((1.2, 1.3),) * 2, ()),              # gain > 1: entries above 255
        (1, False, ((1, 2, 3, 0), (2, 1, 0, 3)), (f32(1.1, 0.9, 1.2), f32(0.7, 1.3, 0.9)), (250, 5), ((2.0, 0.9), (0.5, 1.1)), ((40, 30, 20, 20),)),
        # rectangles: across the right and the bottom border, from the last column, overlapping, larger than the image
        (1, True, (id4, id4), (f32(1.2, 0.8, 1.1),) * 2, (10, 10), (one, one), ((45, 10, 50, 5), (10, 30, 5, 50))),
        (1, True, ((1, 3, 2, 0),) * 2, (f32(0.8, 1.3, 0.9),) * 2, (128, 128), (one, one), ((52, 0, 60, 37), (52, 36, 1, 1))),
        (1, False, (id4, (2, 0, 3, 1)), (f32(1, 1, 1), f32(1.3, 1.2, 0.6)), (0, 77), (one, one), ((10, 10, 20, 15), (20, 18, 20, 15))),
        (1, True, (id4, id4), (f32(0.7, 0.7, 0.7),) * 2, (3, 3), (one, one), ((0, 0, 99, 99),)),
        # a bright image1 and a dark image2 as one stacked image: contrast first, last, and in an asymmetric sample for comparison
        (2, True, ((1, 0, 2, 3),) * 2, (f32(1.1, 0.5, 0.9),) * 2, (0, 0), (one, one), ()),
        (2, True, ((0, 2, 3, 1),) * 2, (f32(1.3, 1.4, 1.2),) * 2, (20, 20), (one, one), ((0, 0, 12, 12),)),
        (2, False, ((1, 0, 2, 3),) * 2, (f32(1.1, 0.5, 0.9),) * 2, (0, 0), (one, one), ()),
    ]
    return out


def main():
    rng = np.random.default_rng(20250)
    pairs = [
        (rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)),
        (rng.integers(0, 256, (37, 53, 3), dtype=np.uint8), rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)),
        (rng.integers(180, 256, (24, 40, 3), dtype=np.uint8), rng.integers(0, 70, (24, 40, 3), dtype=np.uint8)),
    ]
    for a, _ in pairs[:2]:   # saturating pixels on purpose
        a[0, :8] = 255
        a[1, :8] = 0
        a[2, :8] = (255, 0, 128)
    ss = sets()
    n = len(ss)
    arrays = {f"in{j + 1}_{k}": np.ascontiguousarray(p[j].transpose(2, 0, 1)) for k, p in enumerate(pairs) for j in range(2)}
    arrays.update(pair=np.zeros(n, np.int32), shared=np.zeros(n, np.int32), order=np.zeros((n, 2, 4), np.int32), factor=np.zeros((n, 2, 3), np.float32),
                  hue_shift=np.zeros((n, 2), np.int32), gamma=np.zeros((n, 2, 2), np.float64), n_rects=np.zeros(n, np.int32),
                  rects=np.zeros((n, 2, 4), np.int32))
    for i, (k, shared, order, factor, shift, gamma, rects) in enumerate(ss):
        o1, o2 = run(pairs[k][0], pairs[k][1], shared, order, factor, shift, gamma, rects)
        arrays[f"out1_{i}"] = np.ascontiguousarray(o1.transpose(2, 0, 1))
        arrays[f"out2_{i}"] = np.ascontiguousarray(o2.transpose(2, 0, 1))
        arrays["pair"][i], arrays["shared"][i], arrays["n_rects"][i] = k, int(shared), len(rects)
        arrays["order"][i], arrays["factor"][i], arrays["hue_shift"][i], arrays["gamma"][i] = order, factor, shift, gamma
        for r, rect in enumerate(rects):
            arrays["rects"][i, r] = rect
    path = os.path.join(HERE, "augment_photometric.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {n} sets, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
