"""Photometric augmentation and eraser of a stereo pair, the first two stages of the reference's augmentor (`color_transform`,
`eraser_transform`; augmentor.py:82-111), on the device and byte for byte (csrc/augment/augment.hip, include/anystereo_augment.h;
DESIGN.md "Photometric augmentation").

`color_transform` is torchvision's `ColorJitter` + `AdjustGamma` on a PIL image: brightness, contrast and saturation are
`Image.blend` with black, the rounded mean grey and the pixel's own grey, hue is a shift of H in PIL's HSV mode, gamma is a
256-entry table.  `photometric_pair_host` states that arithmetic with numpy — integers, fp32 operations rounded one by one, and
double where PIL's C code computes in double — and equals PIL on every input (tests/test_augment_cpu.py, exhaustively); the
kernels equal `photometric_pair_host` (tests/test_augment_gpu.py).  An edit of one side is an edit of the other.

The reference draws its parameters from `torch` / `random` / `np.random` streams that cannot be replayed, so parameters are
explicit inputs everywhere: `draw_params` derives them from keyed hashes with the reference's distributions.

    spec = PhotoSpec.flow()
    params = draw_params(spec, seed, index0, batch, h, w)
    out1, out2 = photometric_pair(image1, image2, params)            # uint8 or fp32 [B,3,H,W] holding integers 0..255

No PIL import here.
"""
from __future__ import annotations

import ctypes as C
import itertools
import math
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .scenes import _slot_hash, scene_key

_F = np.float32
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3   # the entries of `order` (ColorJitter's fn_idx)
ORDERS = tuple(itertools.permutations(range(4)))
MAX_RECTS = 2
MAX_PARTS = 1024     # AUG_MAX_PARTS: partial sums per (sample, image)
TILE = 2048          # AUG_TILE: pixels of one block iteration (256 threads x 8 pixels)
_IDENTITY_ORDER = (0, 1, 2, 3)


def _f32(x) -> float:
    return float(_F(x))


# ------------------------------------------------------------------------------------------------
# parameters
# ------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ImageParams:
    """The jitter of one image: `order` is a permutation of (BRIGHTNESS, CONTRAST, SATURATION, HUE); the factors are held as the
    fp32 numbers `Image.blend` receives; `hue_shift` is what is added to PIL's H byte; (gamma, gain) are `adjust_gamma`'s and only
    `gamma_table` reads them."""
    order: Tuple[int, int, int, int] = _IDENTITY_ORDER
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue_shift: int = 0
    gamma: float = 1.0
    gain: float = 1.0

    def __post_init__(self):
        object.__setattr__(self, "order", tuple(int(o) for o in self.order))
        for n in ("brightness", "contrast", "saturation"):
            object.__setattr__(self, n, _f32(getattr(self, n)))
        object.__setattr__(self, "hue_shift", int(self.hue_shift))

    def validate(self) -> "ImageParams":
        if sorted(self.order) != [0, 1, 2, 3]:
            raise ValueError(f"ImageParams: order={self.order} is no permutation of 0..3")
        for n in ("brightness", "contrast", "saturation"):
            v = getattr(self, n)
            if not (math.isfinite(v) and v >= 0):
                raise ValueError(f"ImageParams: {n}={v} must be finite and non-negative")
        if not 0 <= self.hue_shift <= 255:
            raise ValueError(f"ImageParams: hue_shift={self.hue_shift} outside 0..255")
        return self


@dataclass(frozen=True)
class SampleParams:
    """One sample of the batch.  `shared`: the reference's symmetric branch — the two images are stacked and jittered as ONE image, so
    image2 takes image1's parameters and gamma table and the contrast level is the mean grey of both images together.  `rects`:
    up to two (x0, y0, dx, dy) filled in image2 with the mean colour of the jittered image2."""
    image1: ImageParams = field(default_factory=ImageParams)
    image2: ImageParams = field(default_factory=ImageParams)
    shared: bool = True
    rects: Tuple[Tuple[int, int, int, int], ...] = ()

    def __post_init__(self):
        object.__setattr__(self, "rects", tuple(tuple(int(v) for v in r) for r in self.rects))
        object.__setattr__(self, "shared", bool(self.shared))

    def of(self, img: int) -> ImageParams:
        return self.image1 if (img == 0 or self.shared) else self.image2

    def validate(self, h: int, w: int) -> "SampleParams":
        self.image1.validate()
        self.image2.validate()
        if len(self.rects) > MAX_RECTS:
            raise ValueError(f"SampleParams: {len(self.rects)} rectangles, at most {MAX_RECTS}")
        for x0, y0, dx, dy in self.rects:
            if dx <= 0 or dy <= 0 or not (0 <= x0 < w and 0 <= y0 < h):
                raise ValueError(f"SampleParams: rectangle {(x0, y0, dx, dy)}: positive extents and an origin inside {h}x{w} expected")
        return self


@dataclass(frozen=True)
class PhotoSpec:
    """What the parameters are drawn from: (lo, hi) ranges of the three factors and of the hue factor, `gamma` =
    (gamma_min, gamma_max, gain_min, gain_max) as `AdjustGamma` takes them, the probabilities of the asymmetric branch and of the eraser,
    and the eraser's extents, lo <= dx, dy < hi."""
    brightness: Tuple[float, float] = (0.6, 1.4)
    contrast: Tuple[float, float] = (0.6, 1.4)
    saturation: Tuple[float, float] = (0.6, 1.4)
    hue: Tuple[float, float] = (-0.5 / 3.14, 0.5 / 3.14)
    gamma: Tuple[float, float, float, float] = (1.0, 1.0, 1.0, 1.0)
    asymmetric_prob: float = 0.2
    eraser_prob: float = 0.5
    eraser_bounds: Tuple[int, int] = (50, 100)

    @classmethod
    def flow(cls, saturation=(0.6, 1.4), gamma=(1, 1, 1, 1)) -> "PhotoSpec":
        """`FlowAugmentor`: ColorJitter(0.4, 0.4, saturation_range, 0.5 / 3.14), asymmetric 0.2, eraser 0.5 with [50, 100)."""
        return cls((0.6, 1.4), (0.6, 1.4), tuple(saturation), (-0.5 / 3.14, 0.5 / 3.14), tuple(float(g) for g in gamma), 0.2, 0.5, (50, 100))

    @classmethod
    def sparse(cls, saturation=(0.7, 1.3), gamma=(1, 1, 1, 1)) -> "PhotoSpec":
        """`SparseFlowAugmentor`: ColorJitter(0.3, 0.3, saturation_range, 0.3 / 3.14), always the stacked pair, the same eraser."""
        return cls((0.7, 1.3), (0.7, 1.3), tuple(saturation), (-0.3 / 3.14, 0.3 / 3.14), tuple(float(g) for g in gamma), 0.0, 0.5, (50, 100))

    def validate(self) -> "PhotoSpec":
        for n in ("brightness", "contrast", "saturation"):
            lo, hi = getattr(self, n)
            if not 0 <= lo <= hi:
                raise ValueError(f"PhotoSpec: {n}={getattr(self, n)}: 0 <= lo <= hi expected")
        if not -0.5 <= self.hue[0] <= self.hue[1] <= 0.5:
            raise ValueError(f"PhotoSpec: hue={self.hue}: -0.5 <= lo <= hi <= 0.5 expected")
        if len(self.gamma) != 4 or not (0 < self.gamma[0] <= self.gamma[1] and 0 < self.gamma[2] <= self.gamma[3]):
            raise ValueError(f"PhotoSpec: gamma={self.gamma}: (gamma_min, gamma_max, gain_min, gain_max), positive and ordered, expected")
        if not (0 <= self.asymmetric_prob <= 1 and 0 <= self.eraser_prob <= 1):
            raise ValueError("PhotoSpec: probabilities in [0, 1] expected")
        if not 0 < self.eraser_bounds[0] < self.eraser_bounds[1]:
            raise ValueError(f"PhotoSpec: eraser_bounds={self.eraser_bounds}: 0 < lo < hi expected")
        return self

    @property
    def has_gamma(self) -> bool:
        return tuple(self.gamma) != (1.0, 1.0, 1.0, 1.0)


def hue_shift_of(hue_factor: float) -> int:
    """torchvision's `np_h += np.uint8(hue_factor * 255)`: truncation toward zero, then modulo 256 (the one mapping of
    this stage that is not pinned by a fixture)."""
    return int(math.trunc(_f32(hue_factor) * 255.0)) % 256


# hash slots of a sample: image i uses slots 16 i + j
_S_ASYM, _S_ERASE, _S_COUNT, _S_RECT = 0, 1, 2, 4          # rectangle r: _S_RECT + 4 r + (x0, y0, dx, dy)
_S_IMAGE, _S_ORDER, _S_B, _S_C, _S_S, _S_H, _S_GAMMA, _S_GAIN = 16, 0, 1, 2, 3, 4, 5, 6
_KEY = 0xA06E57


def _u(base: int, slot: int) -> float:
    """[0, 1) with 24 bits, as the scenes' `uniform`."""
    return (_slot_hash(base, slot) >> 8) * 2.0 ** -24


def _draw_image(spec: PhotoSpec, base: int, img: int) -> ImageParams:
    s0 = _S_IMAGE * (1 + img)
    rng = lambda lo_hi, j: lo_hi[0] + (lo_hi[1] - lo_hi[0]) * _u(base, s0 + j)  # noqa: E731
    order = ORDERS[((_slot_hash(base, s0 + _S_ORDER) >> 8) * 24) >> 24]
    return ImageParams(order, rng(spec.brightness, _S_B), rng(spec.contrast, _S_C), rng(spec.saturation, _S_S),
                       hue_shift_of(rng(spec.hue, _S_H)), rng(spec.gamma[0:2], _S_GAMMA), rng(spec.gamma[2:4], _S_GAIN))


def draw_params(spec: PhotoSpec, seed: int, index0: int, batch: int, h: int, w: int) -> List[SampleParams]:
    """The parameters of samples index0 .. index0 + batch - 1 of an h x w pair: host integers and fp32-rounded floats hashed from
    (seed, index), as `scene_scales` derives its scales.  The order is a uniform permutation, each factor uniform in its range, the
    asymmetric branch and the eraser taken with the spec's probabilities; 1 or 2 rectangles with the origin anywhere in the frame
    and the extents in `eraser_bounds`."""
    spec.validate()
    out = []
    for b in range(int(batch)):
        base = scene_key(int(seed) ^ _KEY, int(index0) + b)
        shared = not (_u(base, _S_ASYM) < spec.asymmetric_prob)
        im1 = _draw_image(spec, base, 0)
        im2 = im1 if shared else _draw_image(spec, base, 1)
        rects = []
        if _u(base, _S_ERASE) < spec.eraser_prob:
            lo, hi = spec.eraser_bounds
            for r in range(1 + (_slot_hash(base, _S_COUNT) & 1)):
                u = [_u(base, _S_RECT + 4 * r + j) for j in range(4)]
                rects.append((int(u[0] * w), int(u[1] * h), lo + int(u[2] * (hi - lo)), lo + int(u[3] * (hi - lo))))
        out.append(SampleParams(im1, im2, shared, tuple(rects)).validate(h, w))
    return out


def gamma_table(params: Sequence[SampleParams]) -> np.ndarray:
    """uint8 [B,2,256]: `adjust_gamma`'s table int((255 + 1 - 1e-3) * gain * (e / 255) ** gamma) per image, in Python's double
    arithmetic as torchvision computes it.  `Image.point` stores its table through a clip to 0..255 (an entry above 255, gain > 1,
    becomes 255: tests/test_augment_cpu.py checks it against PIL), and so does this builder."""
    lut = np.empty((len(params), 2, 256), dtype=np.uint8)
    for b, sp in enumerate(params):
        for img in range(2):
            p = sp.of(img)
            lut[b, img] = [min(255, max(0, int((255 + 1 - 1e-3) * p.gain * pow(e / 255.0, p.gamma)))) for e in range(256)]
    return lut


# ------------------------------------------------------------------------------------------------
# the arithmetic, on numpy arrays (every function takes and returns int32 arrays holding 0..255)
# ------------------------------------------------------------------------------------------------

def grey(r, g, b):
    """PIL's convert("L"): (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def blend(x, d, f: float):
    """`Image.blend(degenerate, image, f)`: d + f (x - d) in fp32, the product rounded, then the sum; truncated for 0 <= f <= 1,
    clipped to [0, 255] and truncated otherwise."""
    t = np.asarray(d, dtype=np.int32).astype(_F) + _F(f) * (np.asarray(x, dtype=np.int32) - d).astype(_F)
    if not 0.0 <= f <= 1.0:
        t = np.clip(t, _F(0), _F(255))
    return t.astype(np.int32)


def contrast_level(grey_sum: int, n: int) -> int:
    """int(mean + 0.5) of `ImageEnhance.Contrast`, in integers."""
    return (2 * int(grey_sum) + int(n)) // (2 * int(n))


def rgb_to_hsv(r, g, b):
    """PIL's rgb2hsv_row: fp32 where its C code holds floats, double where a double constant promotes the expression."""
    r, g, b = (np.asarray(a, dtype=np.int32) for a in (r, g, b))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    flat = maxc == minc
    cr = np.where(flat, 1, maxc - minc).astype(_F)
    s = cr / np.where(flat, 1, maxc).astype(_F)
    rc, gc, bc = ((maxc - c).astype(_F) / cr for c in (r, g, b))
    d = np.float64
    h = np.where(r == maxc, bc - gc,
                 np.where(g == maxc, ((2.0 + rc.astype(d)) - bc.astype(d)).astype(_F), ((4.0 + gc.astype(d)) - rc.astype(d)).astype(_F)))
    x = h.astype(d) / 6.0 + 1.0                       # in [5/6, 11/6]
    h = (x - np.floor(x)).astype(_F)                  # fmod(x, 1.0), exact
    uh = np.clip((h.astype(d) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(d) * 255.0).astype(np.int32), 0, 255)
    return np.where(flat, 0, uh), np.where(flat, 0, us), maxc


def hsv_to_rgb(h, s, v):
    """PIL's hsv2rgb."""
    h, s, v = (np.asarray(a, dtype=np.int32) for a in (h, s, v))
    d = np.float64
    hd = h.astype(d) * 6.0 / 255.0
    i = np.floor(hd)
    f = (hd - i).astype(_F)
    fs = (s.astype(d) / 255.0).astype(_F)
    vd = v.astype(d)
    rnd = lambda x: np.clip(np.floor(x + 0.5).astype(np.int32), 0, 255)  # noqa: E731  (round() of a non-negative double)
    p = rnd(vd * (1.0 - fs.astype(d)))
    q = rnd(vd * (1.0 - (fs * f).astype(d)))
    t = rnd(vd * (1.0 - fs.astype(d) * (1.0 - f.astype(d))))
    k = i.astype(np.int32) % 6
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    grey_px = s == 0
    return np.where(grey_px, v, r), np.where(grey_px, v, g), np.where(grey_px, v, b)


def hue(r, g, b, shift: int):
    hh, ss, vv = rgb_to_hsv(r, g, b)
    return hsv_to_rgb((hh + int(shift)) & 255, ss, vv)


def quantise(x: np.ndarray) -> np.ndarray:
    """An input image as int32 0..255: uint8 as it is, floating point as clamp(floor(x + 0.5), 0, 255) in fp32."""
    if x.dtype == np.uint8:
        return x.astype(np.int32)
    return np.clip(np.floor(x.astype(_F) + _F(0.5)), _F(0), _F(255)).astype(np.int32)


def _apply(op: int, rgb, p: ImageParams, level):
    r, g, b = rgb
    if op == BRIGHTNESS:
        return tuple(blend(c, 0, p.brightness) for c in rgb)
    if op == CONTRAST:
        return tuple(blend(c, level, p.contrast) for c in rgb)
    if op == SATURATION:
        l = grey(r, g, b)
        return tuple(blend(c, l, p.saturation) for c in rgb)
    return hue(r, g, b, p.hue_shift)


def _jitter(images, p: ImageParams):
    """ColorJitter on a list of [3, ...] int32 images jittered as one image (one entry: an image of its own)."""
    state = [tuple(im) for im in images]
    for op in p.order:
        level = None
        if op == CONTRAST:
            level = contrast_level(sum(int(grey(*s).sum()) for s in state), sum(s[0].size for s in state))
        state = [_apply(op, s, p, level) for s in state]
    return [np.stack(s) for s in state]


def photometric_pair_host(image1, image2, params: Sequence[SampleParams], out_dtype=torch.uint8, gamma_lut=None):
    """(out1, out2) as `aug_photometric_pair` writes them: CPU tensors [B,3,H,W], uint8 or fp32 holding integers 0..255."""
    a, b = _host_array(image1), _host_array(image2)
    bsz, _, h, w = _check_pair(a.shape, b.shape, params)
    lut = None if gamma_lut is None else np.asarray(torch.as_tensor(gamma_lut).cpu().numpy(), dtype=np.uint8).reshape(bsz, 2, 256)
    out = np.empty((2,) + a.shape, dtype=np.uint8)
    for i, sp in enumerate(params):
        sp.validate(h, w)
        x1, x2 = quantise(a[i]), quantise(b[i])
        if sp.shared:
            y1, y2 = _jitter([x1, x2], sp.image1)
        else:
            (y1,), (y2,) = _jitter([x1], sp.image1), _jitter([x2], sp.image2)
        if lut is not None:
            y1, y2 = lut[i, 0][y1], lut[i, 0 if sp.shared else 1][y2]
        y2 = np.array(y2, dtype=np.int32)
        if sp.rects:
            mean = [int(y2[c].sum()) // (h * w) for c in range(3)]   # floor of numpy's float64 mean stored into uint8
            for x0, y0, dx, dy in sp.rects:
                for c in range(3):
                    y2[c, y0:y0 + dy, x0:x0 + dx] = mean[c]
        out[0, i], out[1, i] = y1, y2
    o1, o2 = torch.from_numpy(out[0]), torch.from_numpy(out[1])
    return (o1, o2) if out_dtype == torch.uint8 else (o1.to(out_dtype), o2.to(out_dtype))


def _host_array(t) -> np.ndarray:
    t = torch.as_tensor(t)
    if t.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"photometric_pair: images must be uint8 or float32, got {t.dtype}")
    return t.detach().cpu().contiguous().numpy()


def _check_pair(s1, s2, params):
    if len(s1) != 4 or s1[1] != 3 or tuple(s1) != tuple(s2) or 0 in tuple(s1):
        raise ValueError(f"photometric_pair: two non-empty [B,3,H,W] images of one shape expected, got {tuple(s1)} and {tuple(s2)}")
    if len(params) != s1[0]:
        raise ValueError(f"photometric_pair: {len(params)} parameter sets for {s1[0]} samples")
    return tuple(int(v) for v in s1)


# ------------------------------------------------------------------------------------------------
# the public call: HIP on CUDA tensors, the restatement on CPU tensors
# ------------------------------------------------------------------------------------------------

def workspace_bytes(batch: int, h: int, w: int) -> int:
    """`aug_workspace_bytes`: 5 uint64 partial sums (two grey, three channel) per sample and block."""
    parts = min((int(h) * int(w) + TILE - 1) // TILE, MAX_PARTS)
    return int(batch) * 5 * parts * 8


def c_samples(params: Sequence[SampleParams]):
    """The host table `aug_photometric_pair` takes."""
    from .. import _augment_lib as A
    rows = []
    for sp in params:
        s = A.Sample()
        for img, p in enumerate((sp.image1, sp.image2)):
            s.img[img].order[:] = p.order
            s.img[img].factor[:] = (p.brightness, p.contrast, p.saturation)
            s.img[img].hue_shift = p.hue_shift
        s.shared, s.n_rects = int(sp.shared), len(sp.rects)
        for r, rect in enumerate(sp.rects[:MAX_RECTS]):
            s.rect[r][:] = rect
        rows.append(s)
    return (A.Sample * len(rows))(*rows)


_DTYPES = {torch.uint8: 0, torch.float32: 1}


def photometric_pair(image1: torch.Tensor, image2: torch.Tensor, params: Sequence[SampleParams], out_dtype=torch.uint8, gamma_lut=None):
    """Jitter, gamma table and eraser of a pair [B,3,H,W] (uint8, or fp32 quantised once as clamp(floor(x + 0.5), 0, 255)) with explicit
    per-sample parameters -> (out1, out2) of `out_dtype` (uint8, or fp32 holding the same integers).  `gamma_lut`: uint8 [B,2,256]
    (`gamma_table(params)`) or None for the identity.  CUDA tensors run the kernels: at most three launches per 8 samples, no
    memset, no host read-back; CPU tensors run `photometric_pair_host`."""
    if out_dtype not in _DTYPES:
        raise TypeError(f"photometric_pair: out_dtype must be torch.uint8 or torch.float32, got {out_dtype}")
    if image1.is_cuda != image2.is_cuda:
        raise ValueError("photometric_pair: both images on one device expected")
    if not image1.is_cuda:
        return photometric_pair_host(image1, image2, params, out_dtype, gamma_lut)
    from .. import _augment_lib as A, ops
    if image1.dtype not in _DTYPES or image2.dtype != image1.dtype:
        raise TypeError(f"photometric_pair: images must both be uint8 or both float32, got {image1.dtype} and {image2.dtype}")
    bsz, _, h, w = _check_pair(image1.shape, image2.shape, params)
    for sp in params:
        sp.validate(h, w)
    image1, image2 = ops._req(image1, "photometric_pair: image1", image1.dtype), ops._req(image2, "photometric_pair: image2", image1.dtype)
    with ops._guard(image1.device):
        lut = None
        if gamma_lut is not None:
            lut = torch.as_tensor(gamma_lut)
            if lut.dtype != torch.uint8 or tuple(lut.shape) != (bsz, 2, 256):
                raise ValueError(f"photometric_pair: gamma_lut must be uint8 [{bsz},2,256], got {lut.dtype} {tuple(lut.shape)}")
            lut = lut.to(image1.device).contiguous()
        out1 = torch.empty(image1.shape, device=image1.device, dtype=out_dtype)
        out2 = torch.empty(image1.shape, device=image1.device, dtype=out_dtype)
        nws = workspace_bytes(bsz, h, w)
        ws = torch.empty((nws // 8,), device=image1.device, dtype=torch.int64)
        A.check(A.load().aug_photometric_pair(ops._p(image1), ops._p(image2), _DTYPES[image1.dtype], ops._p(out1), ops._p(out2),
                                              _DTYPES[out_dtype], bsz, h, w, c_samples(params), ops._p(lut), ops._p(ws), nws, ops._stream()),
                "photometric_pair")
    return out1, out2


def augment_pair(image1: torch.Tensor, image2: torch.Tensor, spec: PhotoSpec, seed: int, index0: int, out_dtype=torch.float32):
    """`photometric_pair` with the parameters `draw_params` gives samples index0 .. index0 + B - 1; the gamma table is built and
    uploaded only when the spec has a gamma range (the reference's default has none)."""
    bsz, _, h, w = image1.shape
    params = draw_params(spec, seed, index0, bsz, h, w)
    lut = torch.from_numpy(gamma_table(params)) if spec.has_gamma else None
    return photometric_pair(image1, image2, params, out_dtype=out_dtype, gamma_lut=lut)
