"""Regenerates tests/golden/spatial.npz from the reference's own augmentor classes (needs the reference checkout):

    python tests/golden/make_golden_spatial.py

models/coreContinuous_IGEV/utils/augmentor.py is imported as it is; what it imports and this machine lacks (cv2, skimage, torchvision)
is replaced by stand-in modules.  Only `cv2.resize` of them is used by what runs here, and its stand-in is written below: an
independent numpy statement of the two resizes (INTER_LINEAR with fx / fy, INTER_CUBIC with dsize), two separable passes over whole
arrays — it imports nothing of the package under test.  It is NOT cv2: what the fixture pins is the reference's composition (order
of the steps, frame sizes, flips, y-jitter, crop origins, `resize_sparse_flow_map`) around a stated resize arithmetic.

`np.random.rand / uniform / randint` are replaced by a script per case, and every call is recorded.  color_transform and
eraser_transform are switched off on the instance (they are the photometric library's business and have a fixture of their own), so
`__call__` is spatial_transform plus the tail: the INTER_CUBIC resize of the `*WoCrop` classes and ascontiguousarray.

One input set for all cases: `img1`, `img2` uint8 [40,64,3], `flow` fp32 [40,64,2] (channel 0 the disparity, channel 1 zero, as
stereo_datasets.py:112 builds it), `valid` uint8 [40,64] with valid pixels in row 0 and column 0.
Per case k (CASES below):
    c{k}_par      fp64 [12]   class id (0 FlowAugmentor, 1 FlowAugmentorWoCrop, 2 SparseFlowAugmentor, 3 SparseFlowAugmentorWoCrop),
                              rescale, scale_x, scale_y (as cv2.resize / resize_sparse_flow_map received them), flip (0 none, 1 hf, 2 h,
                              3 v), y0, x0 (after the reference's clip), ch, cw, dy2, out_h, out_w (0 without final resize)
    c{k}_st1/2    uint8       spatial_transform's images [ch,cw,3]
    c{k}_stflow   as written  spatial_transform's flow [ch,cw,2] (fp32 or fp64, whatever the reference's arithmetic left)
    c{k}_stvalid  as written  spatial_transform's valid [ch,cw] (sparse classes)
    c{k}_out1/2   uint8       __call__'s images [out_h,out_w,3], *WoCrop classes only: everything else __call__ returns is asserted
                              here to equal spatial_transform's output and is not stored twice
The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
from __future__ import annotations

import io
import math
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402
from make_golden_train_batch import _Stub  # noqa: E402

F = np.float32
H, W = 40, 64
CLASSES = ("FlowAugmentor", "FlowAugmentorWoCrop", "SparseFlowAugmentor", "SparseFlowAugmentorWoCrop")
FLIP_ID = {None: 0, "hf": 1, "h": 2, "v": 3}

# cls, crop, out (None | (h, w)), do_flip, flip taken, yjitter, scale (the value 2 ** uniform must give), stretch (None | (sx, sy) factors),
# rescale taken, origin ("lo" | "hi" | (fraction_y, fraction_x) of randint's range), dy2
CASES = [
    dict(cls=0, crop=(24, 40), scale=1.3, stretch=(1.1, 0.95), origin=(0.5, 0.3), yjitter=True, dy=-2),
    dict(cls=0, crop=(24, 40), scale=2 ** 0.3, do_flip="hf", flip=True, origin=(0.2, 0.9), yjitter=True, dy=2),
    dict(cls=0, crop=(24, 40), scale=0.87, stretch=(0.875, 0.9), do_flip="h", flip=True, origin="hi"),          # both axes clipped at 0.8
    dict(cls=0, crop=(24, 40), scale=0.8828125, do_flip="v", flip=True, origin=(0.4, 0.6)),                      # 64 * fx = 56.5 -> 56
    dict(cls=0, crop=(24, 40), scale=1.17, stretch=(1.0, 1.1), do_flip="hf", flip=False, origin="lo", yjitter=True, dy=0),
    dict(cls=1, crop=(24, 40), out=(16, 28), scale=1.4, stretch=(0.9, 1.05), origin=(0.7, 0.1), yjitter=True, dy=1),
    dict(cls=1, crop=(27, 43), out=(16, 28), scale=1.25, do_flip="hf", flip=True, origin=(0.3, 0.5)),
    dict(cls=1, crop=(16, 28), out=(16, 28), scale=1.0, do_flip="v", flip=True, origin=(0.6, 0.6)),              # the cubic resize is the identity
    dict(cls=1, crop=(22, 37), out=(16, 28), scale=2.0, do_flip="h", flip=True, origin=(0.5, 0.5), yjitter=True, dy=-1),
    dict(cls=2, crop=(24, 40), scale=0.75, origin="lo"),                                                        # collisions and ties; clipped at 0
    dict(cls=2, crop=(24, 40), scale=1.25, origin="hi"),                                                        # clipped at the far border
    dict(cls=2, crop=(24, 40), scale=1.1, rescale=False, do_flip="hf", flip=True, origin=(0.3, 0.45)),
    dict(cls=2, crop=(24, 40), scale=0.5, do_flip="v", flip=True, origin=(0.5, 0.5)),                            # clipped at min_scale = 41 / 64
    dict(cls=2, crop=(24, 40), scale=1.5, do_flip="h", flip=True, origin=(0.35, 0.5)),                           # ties x * 1.5 = k + 0.5
    dict(cls=2, crop=(24, 40), scale=0.87, do_flip="hf", flip=True, origin=(0.3, 0.5)),
    dict(cls=3, crop=(24, 40), out=(16, 28), scale=1.25, origin=(0.0, 0.99)),
    dict(cls=3, crop=(21, 37), out=(16, 28), scale=1.3, rescale=False, do_flip="hf", flip=True, origin=(0.5, 0.5)),
    dict(cls=3, crop=(24, 40), out=(16, 28), scale=0.75, do_flip="v", flip=True, origin=(0.9, 0.2)),
]


# ---- the cv2.resize stand-in ----------------------------------------------------------------------------------------------------

def _linear_taps(n_src: int, n_dst: int, f: float):
    """Per destination index: (i, t) of the source-coordinate rule with the given factor."""
    inv = 1.0 / f
    taps = []
    for d in range(n_dst):
        s = F((d + 0.5) * inv - 0.5)
        i = int(math.floor(s))
        t = F(s - F(i))
        if i < 0:
            i, t = 0, F(0)
        if i >= n_src - 1:
            i, t = n_src - 1, F(0)
        taps.append((i, min(i + 1, n_src - 1), t))
    return taps


def _resize_linear(img: np.ndarray, fx: float, fy: float) -> np.ndarray:
    h, w = img.shape[:2]
    h1, w1 = int(round(h * fy)), int(round(w * fx))
    src = img.astype(F)
    tmp = np.empty((h, w1) + src.shape[2:], dtype=F)
    for x, (i0, i1, t) in enumerate(_linear_taps(w, w1, fx)):                # horizontal pass
        tmp[:, x] = src[:, i0] * F(F(1) - t) + src[:, i1] * t
    out = np.empty((h1, w1) + src.shape[2:], dtype=F)
    for y, (i0, i1, t) in enumerate(_linear_taps(h, h1, fy)):                # vertical pass
        out[y] = tmp[i0] * F(F(1) - t) + tmp[i1] * t
    if img.dtype == np.uint8:
        return np.clip(np.floor(out + F(0.5)), 0, 255).astype(np.uint8)
    return out


def _cubic_weights(t):
    a = F(-0.75)
    c1 = lambda x: F(F(F(F(F(a + F(2)) * x) - F(a + F(3))) * x) * x) + F(1)                      # noqa: E731
    c2 = lambda x: F(F(F(F(F(F(a * x) - F(F(5) * a)) * x) + F(F(8) * a)) * x) - F(F(4) * a))     # noqa: E731
    return [c2(F(t + F(1))), F(c1(t)), F(c1(F(F(1) - t))), c2(F(F(2) - t))]


def _cubic_taps(n_src: int, n_dst: int):
    scale = F(F(n_src) / F(n_dst))
    taps = []
    for d in range(n_dst):
        s = F(F(scale * F(F(d) + F(0.5))) - F(0.5))
        i = int(math.floor(s))
        taps.append(([min(max(i - 1 + k, 0), n_src - 1) for k in range(4)], _cubic_weights(F(s - F(i)))))
    return taps


def _resize_cubic(img: np.ndarray, w1: int, h1: int) -> np.ndarray:
    assert img.dtype == np.uint8
    h, w = img.shape[:2]
    src = img.astype(F)
    tmp = np.empty((h, w1, 3), dtype=F)
    for x, (idx, wgt) in enumerate(_cubic_taps(w, w1)):
        tmp[:, x] = ((src[:, idx[0]] * wgt[0] + src[:, idx[1]] * wgt[1]) + src[:, idx[2]] * wgt[2]) + src[:, idx[3]] * wgt[3]
    out = np.empty((h1, w1, 3), dtype=F)
    for y, (idx, wgt) in enumerate(_cubic_taps(h, h1)):
        out[y] = ((tmp[idx[0]] * wgt[0] + tmp[idx[1]] * wgt[1]) + tmp[idx[2]] * wgt[2]) + tmp[idx[3]] * wgt[3]
    return np.clip(np.floor(out + F(0.5)), 0, 255).astype(np.uint8)


RESIZES = []  # (fx, fy) of every INTER_LINEAR call of the current case


def cv2_resize(img, dsize=None, fx=None, fy=None, interpolation=None):
    if dsize is None:
        assert interpolation == "linear"
        RESIZES.append((float(fx), float(fy)))
        return _resize_linear(img, float(fx), float(fy))
    assert interpolation == "cubic"
    return _resize_cubic(img, int(dsize[0]), int(dsize[1]))


def import_augmentor():
    import importlib
    for name in ("cv2", "skimage", "torchvision", "torchvision.transforms"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    cv2 = sys.modules["cv2"]
    cv2.resize, cv2.INTER_LINEAR, cv2.INTER_CUBIC = cv2_resize, "linear", "cubic"
    sys.path.insert(0, REF)
    pkg = types.ModuleType("models")
    pkg.__path__ = [REF + "/models"]
    sys.modules["models"] = pkg
    import models.coreContinuous_IGEV.utils.augmentor as aug
    return aug


# ---- scripted np.random ---------------------------------------------------------------------------------------------------------

def exponent_of(scale: float) -> float:
    """e with 2 ** e == scale exactly (the value np.random.uniform is made to return)."""
    e = math.log2(scale)
    if 2 ** e == scale:
        return e
    lo = hi = e
    for _ in range(64):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        for cand in (lo, hi):
            if 2 ** float(cand) == scale:
                return float(cand)
    raise AssertionError(f"no exponent gives {scale!r}")


class Script:
    """np.random's three functions for one case; `log` records (name, arguments, returned value)."""

    def __init__(self, case):
        self.case, self.log = case, []
        sparse = case["cls"] >= 2
        self.uniforms = [exponent_of(case["scale"])]
        self.rands = []
        if not sparse:
            st = case.get("stretch")
            self.rands.append(0.1 if st else 0.9)                            # stretch_prob 0.8
            if st:
                self.uniforms += [exponent_of(st[0]), exponent_of(st[1])]
        self.rands.append(0.5 if case.get("rescale", True) else 0.95)       # spatial_aug_prob 1.0 / 0.8
        if case.get("do_flip"):
            take = case.get("flip", False)
            p = 0.05 if take else 0.7                                        # under 0.1 and 0.5, or over both
            self.rands += [p, p, p]
        self.n_randint = 0

    def rand(self):
        v = self.rands.pop(0)
        self.log.append(("rand", (), v))
        return v

    def uniform(self, lo, hi):
        v = self.uniforms.pop(0)
        self.log.append(("uniform", (lo, hi), v))
        return v

    def randint(self, lo, hi=None):
        k, self.n_randint = self.n_randint, self.n_randint + 1
        assert hi is not None and lo < hi, ("the reference's randint would raise", lo, hi)
        if k == 2:
            v = int(self.case["dy"])
            assert lo <= v < hi
        else:
            o = self.case["origin"]
            v = lo if o == "lo" else hi - 1 if o == "hi" else lo + int(o[k] * (hi - lo))
        self.log.append(("randint", (lo, hi), v))
        return v


def run_case(aug, case, img1, img2, flow, valid):
    cls, sparse, wo = CLASSES[case["cls"]], case["cls"] >= 2, case["cls"] in (1, 3)
    kw = dict(crop_size=list(case["crop"]), do_flip=case.get("do_flip", False))
    if not sparse:
        kw["yjitter"] = case.get("yjitter", False)
    a = getattr(aug, cls)(**kw)
    a.color_transform = lambda x, y: (x, y)
    a.eraser_transform = lambda x, y: (x, y)
    st = {}
    inner = a.spatial_transform

    def recording(*args):
        st["out"] = inner(*args)
        return st["out"]
    a.spatial_transform = recording
    script = Script(case)
    saved = np.random.rand, np.random.uniform, np.random.randint
    np.random.rand, np.random.uniform, np.random.randint = script.rand, script.uniform, script.randint
    del RESIZES[:]
    try:
        args = [img1.copy(), img2.copy(), flow.copy()] + ([valid.copy()] if sparse else [])
        out = a(*args, **(dict(crop_size=list(case["crop"]), scale_size=list(case["out"])) if wo else {}))
    finally:
        np.random.rand, np.random.uniform, np.random.randint = saved
    assert not script.rands and not script.uniforms, "the script was not consumed"
    return st["out"], out, script.log, list(RESIZES)


def main():
    aug = import_augmentor()
    g = np.random.RandomState(20260)
    img1 = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    img2 = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    disp = (g.randint(4, 400, (H, W)) / 4.0).astype(F)
    flow = np.stack([disp, np.zeros_like(disp)], axis=-1)
    valid = (g.rand(H, W) < 0.55).astype(np.uint8)
    valid[0, ::2], valid[::3, 0] = 1, 1
    arrs = {"img1": img1, "img2": img2, "flow": flow, "valid": valid}
    for k, case in enumerate(CASES):
        sparse = case["cls"] >= 2
        st, out, log, resizes = run_case(aug, case, img1, img2, flow, valid)
        ints = [v for name, _, v in log if name == "randint"]
        rescale = bool(resizes) or (sparse and case.get("rescale", True))
        if sparse and rescale:       # resize_sparse_flow_map's factors are cv2.resize's: the same scale_x, scale_y
            assert len(resizes) == 2 and resizes[0] == resizes[1]
        elif rescale:
            assert len(resizes) == 3 and resizes[0] == resizes[1] == resizes[2]
        assert rescale == case.get("rescale", True)
        fx, fy = resizes[0] if rescale else (1.0, 1.0)
        fh, fw = (int(round(H * fy)), int(round(W * fx))) if rescale else (H, W)
        ch, cw = case["crop"]
        y0, x0 = ints[0], ints[1]
        if sparse:                   # the reference's own clip of the origin
            y0, x0 = int(np.clip(y0, 0, fh - ch)), int(np.clip(x0, 0, fw - cw))
        dy2 = ints[2] if len(ints) > 2 else 0
        flip = FLIP_ID[case.get("do_flip")] if case.get("flip") else 0
        oh, ow = case.get("out", (0, 0))
        arrs[f"c{k}_par"] = np.asarray([case["cls"], float(rescale), fx, fy, flip, y0, x0, ch, cw, dy2, oh, ow], dtype=np.float64)
        names = ("1", "2", "flow", "valid")
        for n, a in zip(names, st):
            arrs[f"c{k}_st{n}"] = np.ascontiguousarray(a)
        for n, a, b in zip(names, st, out):   # the tail changes nothing but the *WoCrop images: only those are stored twice
            if case["cls"] in (1, 3) and n in ("1", "2"):
                arrs[f"c{k}_out{n}"] = np.ascontiguousarray(b)
            else:
                assert a.dtype == b.dtype and np.array_equal(a, b), (k, n)
        print(f"case {k} {CLASSES[case['cls']]}: frame {fh}x{fw} fx={fx!r} fy={fy!r} flip={flip} origin=({y0},{x0}) dy2={dy2} "
              f"-> {tuple(out[0].shape)}, flow {out[2].dtype}" + (f", valid {out[3].dtype} {int((np.asarray(out[3]) >= 1).sum())} set" if sparse else ""))

    path = os.path.join(HERE, "spatial.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrs[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))  # fixed: the file regenerates bit for bit
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"wrote spatial.npz ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
