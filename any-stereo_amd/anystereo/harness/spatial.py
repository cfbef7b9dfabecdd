"""Spatial augmentation of a stereo pair, the third stage of the reference's augmentor (`spatial_transform`: random rescale, flips,
y-jitter, crop; augmentor.py:113-171, :397-445) and the final `INTER_CUBIC` resize to (h_lr, w_lr) of its `*WoCrop` classes
(:306-318, :583-595), on the device (csrc/spatial/spatial.hip, include/anystereo_spatial.h; DESIGN.md "Spatial augmentation").

The composition — the order of the steps, the frame-size rule, the three flip modes with their quirks, the y-jitter, the crop and the
whole of `resize_sparse_flow_map` — is pinned to the reference's own code by tests/golden/spatial.npz.  The two resizes are a stated
arithmetic (the header gives it) whose equality with `cv2.resize` is NOT verified: cv2 is not installed here.  `spatial_pair_host`
states everything with numpy, fp32 operations rounded one by one, and equals the fixture (tests/test_spatial_cpu.py); the kernels
equal `spatial_pair_host` (tests/test_spatial_gpu.py).  An edit of one side is an edit of the other.

Quirks of the reference that are kept:
  - flip "h" (the stereo flip) writes mirror(image2) to image1 and mirror(image1) to image2 and leaves the ground truth untouched,
    NOT mirrored;
  - flip "hf" negates the disparity (a 0 becomes -0.0);
  - the sparse form never flips `valid`: only the images and the disparity are flipped;
  - `resize_sparse_flow_map` keeps a landing position only if it is > 0 on both axes: row 0 and column 0 of a rescaled sparse
    ground truth are empty.

As in `harness.augment`, parameters are explicit inputs and `draw_spatial` derives them from keyed hashes:

    spec = SpatialSpec.flow((320, 720))
    params = draw_spatial(spec, seed, index0, batch, H, W, crop_sizes)
    out1, out2, disps, valids = spatial_pair(image1, image2, disp, params, out_size=(h_lr, w_lr))
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .scenes import _slot_hash, scene_key

_F = np.float32
FLIPS = ("none", "hf", "h", "v")           # SPT_FLIP_*
MIN_SCALE, MAX_SCALE = 0.125, 8.0           # SPT_MIN_SCALE, SPT_MAX_SCALE
_KEY = 0x59A71A


def _rint(x: float) -> int:
    """rint of a double, half to even: what `int(round(x))` and cv2's saturate_cast<int> both give."""
    return int(round(float(x)))


# ------------------------------------------------------------------------------------------------
# parameters
# ------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class SpatialParams:
    """One sample.  `rescale`: the frame is resized by (scale_x, scale_y) — host doubles, already clipped — to
    (rint(H scale_y), rint(W scale_x)); `flip` one of FLIPS, applied to the whole rescaled frame; the crop (ch, cw) starts at (y0, x0)
    of the flipped frame for image1 and the ground truth and at (y0 + dy2, x0) for image2."""
    rescale: bool = False
    scale_x: float = 1.0
    scale_y: float = 1.0
    flip: str = "none"
    y0: int = 0
    x0: int = 0
    ch: int = 0
    cw: int = 0
    dy2: int = 0

    def __post_init__(self):
        object.__setattr__(self, "rescale", bool(self.rescale))
        object.__setattr__(self, "scale_x", float(self.scale_x))
        object.__setattr__(self, "scale_y", float(self.scale_y))
        for n in ("y0", "x0", "ch", "cw", "dy2"):
            object.__setattr__(self, n, int(getattr(self, n)))

    def frame(self, h: int, w: int) -> Tuple[int, int]:
        """The rescaled frame of an h x w input."""
        if not self.rescale:
            return int(h), int(w)
        return _rint(h * self.scale_y), _rint(w * self.scale_x)

    def validate(self, h: int, w: int) -> "SpatialParams":
        if self.flip not in FLIPS:
            raise ValueError(f"SpatialParams: flip={self.flip!r}: one of {FLIPS}")
        if self.rescale:
            for n in ("scale_x", "scale_y"):
                v = getattr(self, n)
                if not (math.isfinite(v) and MIN_SCALE <= v <= MAX_SCALE):
                    raise ValueError(f"SpatialParams: {n}={v} outside [{MIN_SCALE}, {MAX_SCALE}]")
        fh, fw = self.frame(h, w)
        if self.ch < 1 or self.cw < 1:
            raise ValueError(f"SpatialParams: crop {self.ch}x{self.cw} must be positive")
        if self.y0 < 0 or self.x0 < 0 or self.y0 + self.ch > fh or self.x0 + self.cw > fw:
            raise ValueError(f"SpatialParams: the crop {self.ch}x{self.cw} at ({self.y0}, {self.x0}) leaves the {fh}x{fw} frame")
        if self.y0 + self.dy2 < 0 or self.y0 + self.dy2 + self.ch > fh:
            raise ValueError(f"SpatialParams: image2's crop at y0 + dy2 = {self.y0} + {self.dy2} leaves the {fh}x{fw} frame")
        return self


@dataclass(frozen=True)
class SpatialSpec:
    """What the parameters are drawn from: the constants of `FlowAugmentor[WoCrop]` (`flow`) and `SparseFlowAugmentor[WoCrop]` (`sparse`).
    `crop`: the crop size when `draw_spatial` is given none per sample.  `min_pad`: the +8 / +1 of the reference's scale floor
    max((ch + pad) / H, (cw + pad) / W).  `margins` (y, x): the sparse class draws its origin from [0, fh - ch + my) x [-mx, fw - cw + mx)
    and clips it into the frame; (0, 0) for `SparseFlowAugmentorWoCrop`, which has none."""
    kind: str = "flow"
    crop: Optional[Tuple[int, int]] = None
    min_scale: float = -0.2
    max_scale: float = 0.4
    do_flip: object = False            # False | "hf" | "h" | "v"
    yjitter: bool = True
    spatial_aug_prob: float = 1.0
    stretch_prob: float = 0.8
    max_stretch: float = 0.2
    h_flip_prob: float = 0.5
    v_flip_prob: float = 0.1
    min_pad: int = 8
    margins: Tuple[int, int] = (0, 0)

    @classmethod
    def flow(cls, crop=None, min_scale=-0.2, max_scale=0.4, do_flip=False, yjitter=True) -> "SpatialSpec":
        """`FlowAugmentor` / `FlowAugmentorWoCrop`: always rescaled, stretched with probability 0.8 by 2^+-0.2 per axis, scale floor with +8."""
        return cls("flow", None if crop is None else (int(crop[0]), int(crop[1])), float(min_scale), float(max_scale), do_flip, bool(yjitter),
                   1.0, 0.8, 0.2, 0.5, 0.1, 8, (0, 0))

    @classmethod
    def sparse(cls, crop=None, min_scale=-0.2, max_scale=0.4, do_flip=False, wo_crop=False) -> "SpatialSpec":
        """`SparseFlowAugmentor` (margins 20 and 50, the origin clipped) / `SparseFlowAugmentorWoCrop` (wo_crop=True: no margins): rescaled
        with probability 0.8, one scale for both axes, scale floor with +1, no y-jitter."""
        return cls("sparse", None if crop is None else (int(crop[0]), int(crop[1])), float(min_scale), float(max_scale), do_flip, False,
                   0.8, 0.0, 0.2, 0.5, 0.1, 1, (0, 0) if wo_crop else (20, 50))

    def validate(self) -> "SpatialSpec":
        if self.kind not in ("flow", "sparse"):
            raise ValueError(f"SpatialSpec: kind={self.kind!r} (flow | sparse)")
        if self.do_flip not in (False, None, "hf", "h", "v"):
            raise ValueError(f"SpatialSpec: do_flip={self.do_flip!r} (False | 'hf' | 'h' | 'v')")
        if not self.min_scale <= self.max_scale:
            raise ValueError(f"SpatialSpec: min_scale={self.min_scale} > max_scale={self.max_scale}")
        for n in ("spatial_aug_prob", "stretch_prob", "h_flip_prob", "v_flip_prob"):
            if not 0 <= getattr(self, n) <= 1:
                raise ValueError(f"SpatialSpec: {n}={getattr(self, n)} outside [0, 1]")
        if self.kind == "sparse" and self.yjitter:
            raise ValueError("SpatialSpec: the sparse classes have no y-jitter")
        return self


# hash slots of a sample
_S_SCALE, _S_STRETCH, _S_SX, _S_SY, _S_AUG, _S_FLIP, _S_Y0, _S_X0, _S_DY = range(9)


def _u(base: int, slot: int) -> float:
    """[0, 1) with 24 bits, as the scenes' `uniform`."""
    return (_slot_hash(base, slot) >> 8) * 2.0 ** -24


def _randint(base: int, slot: int, lo: int, hi: int, what: str) -> int:
    """`np.random.randint(lo, hi)`: uniform on lo .. hi - 1; ValueError for an empty range, as numpy's."""
    if lo >= hi:
        raise ValueError(f"draw_spatial: {what}: the crop cannot fit (empty range [{lo}, {hi}))")
    return lo + int(_u(base, slot) * (hi - lo))


def draw_spatial(spec: SpatialSpec, seed: int, index0: int, batch: int, h: int, w: int, crop_sizes=None) -> List[SpatialParams]:
    """The parameters of samples index0 .. index0 + batch - 1 of an h x w frame, hashed from (seed, index) with the reference's
    distributions.  `crop_sizes`: B (ch, cw) pairs (the `*WoCrop` call's crop_size), or None for `spec.crop` everywhere.  The scale is
    2^U(min_scale, max_scale), stretched and clipped from below as the spec says; the flip of `spec.do_flip` is taken with its
    probability; the origin is uniform where the reference's `randint` draws it.  A crop that cannot fit raises ValueError, where
    the reference's `randint` would."""
    spec.validate()
    if crop_sizes is None:
        if spec.crop is None:
            raise ValueError("draw_spatial: no crop_sizes and the spec has no crop")
        crop_sizes = [spec.crop] * int(batch)
    crop_sizes = [(int(a), int(b)) for a, b in crop_sizes]
    if len(crop_sizes) != int(batch):
        raise ValueError(f"draw_spatial: {len(crop_sizes)} crop sizes for {batch} samples")
    out = []
    for b, (ch, cw) in enumerate(crop_sizes):
        base = scene_key(int(seed) ^ _KEY, int(index0) + b)
        floor = max((ch + spec.min_pad) / float(h), (cw + spec.min_pad) / float(w))
        scale = 2.0 ** (spec.min_scale + (spec.max_scale - spec.min_scale) * _u(base, _S_SCALE))
        sx = sy = scale
        if _u(base, _S_STRETCH) < spec.stretch_prob:
            sx *= 2.0 ** (spec.max_stretch * (2.0 * _u(base, _S_SX) - 1.0))
            sy *= 2.0 ** (spec.max_stretch * (2.0 * _u(base, _S_SY) - 1.0))
        sx, sy = max(sx, floor), max(sy, floor)
        rescale = _u(base, _S_AUG) < spec.spatial_aug_prob
        flip = "none"
        if spec.do_flip and _u(base, _S_FLIP) < (spec.v_flip_prob if spec.do_flip == "v" else spec.h_flip_prob):
            flip = spec.do_flip
        p = SpatialParams(rescale, sx if rescale else 1.0, sy if rescale else 1.0, flip, 0, 0, ch, cw, 0)
        if rescale:
            for n, v in (("scale_x", sx), ("scale_y", sy)):
                if not MIN_SCALE <= v <= MAX_SCALE:
                    raise ValueError(f"draw_spatial: sample {b}: {n}={v} outside [{MIN_SCALE}, {MAX_SCALE}] (a {ch}x{cw} crop of a {h}x{w} frame)")
        fh, fw = p.frame(h, w)
        dy2 = 0
        if spec.kind == "flow" and spec.yjitter:
            y0 = _randint(base, _S_Y0, 2, fh - ch - 2, f"sample {b}, rows of a {fh}x{fw} frame")
            x0 = _randint(base, _S_X0, 2, fw - cw - 2, f"sample {b}, columns of a {fh}x{fw} frame")
            dy2 = _randint(base, _S_DY, -2, 3, "dy2")
        elif spec.kind == "flow":
            y0 = _randint(base, _S_Y0, 0, fh - ch, f"sample {b}, rows of a {fh}x{fw} frame")
            x0 = _randint(base, _S_X0, 0, fw - cw, f"sample {b}, columns of a {fh}x{fw} frame")
        else:
            my, mx = spec.margins
            if fh < ch or fw < cw:
                raise ValueError(f"draw_spatial: sample {b}: the crop {ch}x{cw} cannot fit the {fh}x{fw} frame")
            y0 = _randint(base, _S_Y0, 0, fh - ch + my, f"sample {b}, rows of a {fh}x{fw} frame")
            x0 = _randint(base, _S_X0, -mx, fw - cw + mx, f"sample {b}, columns of a {fh}x{fw} frame")
            y0, x0 = min(max(y0, 0), fh - ch), min(max(x0, 0), fw - cw)
        out.append(SpatialParams(rescale, p.scale_x, p.scale_y, flip, y0, x0, ch, cw, dy2).validate(h, w))
    return out


# ------------------------------------------------------------------------------------------------
# the arithmetic, on numpy arrays
# ------------------------------------------------------------------------------------------------

def quantise(x: np.ndarray) -> np.ndarray:
    """clamp(floor(x + 0.5), 0, 255) in fp32 -> fp32 holding integers."""
    return np.clip(np.floor(x.astype(_F) + _F(0.5)), _F(0), _F(255))


def lin_axis(d: np.ndarray, f: float, n: int):
    """(i0, i1, t) of the rescaled indices `d` on a source axis of n: inv = 1.0 / f in double, s = (float)((d + 0.5) inv - 0.5),
    i = floor(s), t = s - i in fp32; i < 0 -> (0, 0); i >= n - 1 -> (n - 1, 0)."""
    inv = 1.0 / float(f)
    s = ((d.astype(np.float64) + 0.5) * inv - 0.5).astype(_F)
    fl = np.floor(s)
    i, t = fl.astype(np.int64), (s - fl).astype(_F)
    lo, hi = i < 0, i >= n - 1
    i = np.where(lo, 0, np.where(hi, n - 1, i))
    t = np.where(lo | hi, _F(0), t).astype(_F)
    return i, np.minimum(i + 1, n - 1), t


def linear_at(src: np.ndarray, ys: np.ndarray, xs: np.ndarray, fy: float, fx: float) -> np.ndarray:
    """The rescaled frame of the fp32 planes src [..., H, W] at rows `ys` and columns `xs` -> fp32 [..., len(ys), len(xs)]: horizontal
    S[i] (1 - t) + S[i + 1] t, then vertical likewise, every operation rounded on its own."""
    src = src.astype(_F, copy=False)
    h, w = src.shape[-2:]
    y0, y1, ty = lin_axis(np.asarray(ys), fy, h)
    x0, x1, tx = lin_axis(np.asarray(xs), fx, w)
    one = _F(1)
    with np.errstate(invalid="ignore", over="ignore"):
        top, bot = src[..., y0, :], src[..., y1, :]
        r0 = top[..., x0] * (one - tx) + top[..., x1] * tx
        r1 = bot[..., x0] * (one - tx) + bot[..., x1] * tx
        return (r0 * (one - ty)[:, None] + r1 * ty[:, None]).astype(_F)


def resize_linear_host(src: np.ndarray, fx: float, fy: float) -> np.ndarray:
    """The whole rescaled frame of src [..., H, W] (fp32, not quantised): what the tests hold against fp64."""
    h, w = src.shape[-2:]
    return linear_at(src, np.arange(_rint(h * fy)), np.arange(_rint(w * fx)), fy, fx)


_A = -0.75


def _cubic1(x):
    return ((_F(_A + 2) * x - _F(_A + 3)) * x * x + _F(1)).astype(_F)


def _cubic2(x):
    return (((_F(_A) * x - _F(5 * _A)) * x + _F(8 * _A)) * x - _F(4 * _A)).astype(_F)


def _cubic_axis(n_in: int, n_out: int):
    """csrc/cubic.h's `cubic_axis` for every output index: taps [4, n_out] clamped into [0, n_in), weights fp32 [4, n_out]."""
    scale = _F(n_in) / _F(n_out)
    src = (scale * (np.arange(n_out).astype(_F) + _F(0.5)) - _F(0.5)).astype(_F)
    fl = np.floor(src)
    t = (src - fl).astype(_F)
    i = fl.astype(np.int64)
    idx = np.stack([np.clip(i - 1 + k, 0, n_in - 1) for k in range(4)])
    one = _F(1)
    return idx, np.stack([_cubic2(t + one), _cubic1(t), _cubic1(one - t), _cubic2(_F(2) - t)])


def resize_cubic_host(crop: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """fp32 [..., ch, cw] holding integers -> fp32 [..., out_h, out_w], quantised: the four horizontal products summed left to right,
    then the four vertical ones (csrc/cubic.h, as prepare.hip)."""
    crop = crop.astype(_F, copy=False)
    iy, wy = _cubic_axis(crop.shape[-2], out_h)
    ix, wx = _cubic_axis(crop.shape[-1], out_w)
    out = None
    for a in range(4):
        rows = crop[..., iy[a], :]
        acc = None
        for k in range(4):
            term = rows[..., ix[k]] * wx[k]
            acc = term if acc is None else acc + term
        term = acc * wy[a][:, None]
        out = term if out is None else out + term
    return quantise(out)


def sparse_frame_host(disp: np.ndarray, valid: np.ndarray, fx: float, fy: float):
    """`resize_sparse_flow_map` of one sample: (disp fp32 [fh, fw], valid uint8 [fh, fw]).  A source pixel (x, y) with valid >= 1 lands
    at (rint(x fx), rint(y fy)) and is kept if both are > 0 and inside; its value is (float)((double)d fx); the last in raster order
    wins."""
    h, w = disp.shape
    fh, fw = _rint(h * fy), _rint(w * fx)
    ys, xs = np.nonzero(valid >= 1)                                   # raster order
    tx = np.rint(xs.astype(np.float64) * float(fx)).astype(np.int64)
    ty = np.rint(ys.astype(np.float64) * float(fy)).astype(np.int64)
    keep = (tx > 0) & (tx < fw) & (ty > 0) & (ty < fh)
    winner = np.full(fh * fw, -1, dtype=np.int64)
    np.maximum.at(winner, (ty * fw + tx)[keep], (ys * w + xs)[keep])
    hit = winner >= 0
    out = np.zeros(fh * fw, dtype=_F)
    out[hit] = (disp.reshape(-1)[winner[hit]].astype(np.float64) * float(fx)).astype(_F)
    return out.reshape(fh, fw), hit.astype(np.uint8).reshape(fh, fw)


def _input_planes(a: np.ndarray) -> np.ndarray:
    """An input image as fp32 holding integers 0..255: uint8 as it is, fp32 quantised once."""
    return a.astype(_F) if a.dtype == np.uint8 else quantise(a)


def _host_array(t, dtypes, what) -> np.ndarray:
    t = torch.as_tensor(t)
    if t.dtype not in dtypes:
        raise TypeError(f"spatial_pair: {what} must be one of {dtypes}, got {t.dtype}")
    return t.detach().cpu().contiguous().numpy()


def _check(s1, s2, sd, sv, params, out_size):
    if len(s1) != 4 or s1[1] != 3 or tuple(s1) != tuple(s2) or 0 in tuple(s1):
        raise ValueError(f"spatial_pair: two non-empty [B,3,H,W] images of one shape expected, got {tuple(s1)} and {tuple(s2)}")
    bsz, _, h, w = (int(v) for v in s1)
    if tuple(sd) != (bsz, h, w) or (sv is not None and tuple(sv) != (bsz, h, w)):
        raise ValueError(f"spatial_pair: disp (and valid) must be [{bsz},{h},{w}], got {tuple(sd)}" + ("" if sv is None else f" and {tuple(sv)}"))
    if len(params) != bsz:
        raise ValueError(f"spatial_pair: {len(params)} parameter sets for {bsz} samples")
    for p in params:
        p.validate(h, w)
    if out_size is None:
        if any((p.ch, p.cw) != (params[0].ch, params[0].cw) for p in params):
            raise ValueError("spatial_pair: without out_size all crops must have one size")
        h_out, w_out = params[0].ch, params[0].cw
    else:
        h_out, w_out = int(out_size[0]), int(out_size[1])
        if h_out < 1 or w_out < 1:
            raise ValueError(f"spatial_pair: out_size={tuple(out_size)} must be positive")
    return bsz, h, w, h_out, w_out


def spatial_pair_host(image1, image2, disp, params: Sequence[SpatialParams], valid=None, out_size=None, out_dtype=torch.uint8):
    """(out1, out2, disps, valids) as `spt_spatial_pair` writes them, on the CPU: images [B,3,h_out,w_out] of `out_dtype`, B fp32 crops
    [ch_b, cw_b], and B uint8 validity crops (None without `valid`)."""
    a1, a2 = _host_array(image1, (torch.uint8, torch.float32), "image1"), _host_array(image2, (torch.uint8, torch.float32), "image2")
    d = _host_array(disp, (torch.float32,), "disp")
    v = None if valid is None else _host_array(valid, (torch.uint8,), "valid")
    bsz, h, w, h_out, w_out = _check(a1.shape, a2.shape, d.shape, None if v is None else v.shape, params, out_size)
    outs = np.empty((2, bsz, 3, h_out, w_out), dtype=_F)
    disps, valids = [], []
    for b, p in enumerate(params):
        fh, fw = p.frame(h, w)
        src = (_input_planes(a1[b]), _input_planes(a2[b]))
        if p.flip == "h":
            src = (src[1], src[0])
        for im in range(2):
            ys = p.y0 + (p.dy2 if im == 1 else 0) + np.arange(p.ch)
            xs = p.x0 + np.arange(p.cw)
            if p.flip in ("hf", "h"):
                xs = fw - 1 - xs
            if p.flip == "v":
                ys = fh - 1 - ys
            crop = quantise(linear_at(src[im], ys, xs, p.scale_y, p.scale_x)) if p.rescale else src[im][:, ys][:, :, xs]
            outs[im, b] = crop if out_size is None else resize_cubic_host(crop, h_out, w_out)
        vy, vx = p.y0 + np.arange(p.ch), p.x0 + np.arange(p.cw)           # validity: never flipped
        ys, xs = (fh - 1 - vy if p.flip == "v" else vy), (fw - 1 - vx if p.flip == "hf" else vx)
        if v is not None and p.rescale:
            fd, fv = sparse_frame_host(d[b], v[b], p.scale_x, p.scale_y)
            dc, vc = fd[ys][:, xs], fv[vy][:, vx]
        elif p.rescale:
            with np.errstate(invalid="ignore", over="ignore"):
                dc = (linear_at(d[b], ys, xs, p.scale_y, p.scale_x).astype(np.float64) * p.scale_x).astype(_F)
            vc = None
        else:
            dc, vc = d[b][ys][:, xs], (None if v is None else v[b][vy][:, vx])
        disps.append(torch.from_numpy(np.ascontiguousarray(-dc if p.flip == "hf" else dc)))
        valids.append(None if vc is None else torch.from_numpy(np.ascontiguousarray(vc)))
    o1, o2 = torch.from_numpy(outs[0]).to(out_dtype), torch.from_numpy(outs[1]).to(out_dtype)
    return o1, o2, disps, (None if v is None else valids)


# ------------------------------------------------------------------------------------------------
# the public call: HIP on CUDA tensors, the restatement on CPU tensors
# ------------------------------------------------------------------------------------------------

def c_samples(params: Sequence[SpatialParams]):
    """The host table `spt_spatial_pair` takes."""
    from .. import _spatial_lib as S
    rows = [S.Sample(p.scale_x, p.scale_y, int(p.rescale), FLIPS.index(p.flip), p.y0, p.x0, p.ch, p.cw, p.dy2, 0) for p in params]
    return (S.Sample * len(rows))(*rows)


_DTYPES = {torch.uint8: 0, torch.float32: 1}


def spatial_pair(image1: torch.Tensor, image2: torch.Tensor, disp: torch.Tensor, params: Sequence[SpatialParams], valid=None, out_size=None,
                 out_dtype=torch.uint8):
    """Rescale, flip, crop and (with `out_size` = (h_lr, w_lr)) the final bicubic resize of a pair [B,3,H,W] (uint8, or fp32 quantised once)
    with full-frame ground truth disp fp32 [B,H,W] and, for the sparse form, valid uint8 [B,H,W] -> (out1, out2, disps, valids):
    the images [B,3,h_out,w_out] of `out_dtype` (uint8, or fp32 holding the same integers), B fp32 crops [ch_b, cw_b] in the crop's own
    pixels and B uint8 validity crops (None without `valid`).  Without `out_size` all crops share one size and the images are the
    crops; with it the crops may differ per sample.  The quirks of the reference's flips are kept (module docstring): "h" swaps and
    mirrors the images and leaves the ground truth unmirrored, the sparse form never flips `valid`.  CUDA tensors run the kernels, two
    launches per 8 samples, no workspace, no host read-back; CPU tensors run `spatial_pair_host`."""
    if out_dtype not in _DTYPES:
        raise TypeError(f"spatial_pair: out_dtype must be torch.uint8 or torch.float32, got {out_dtype}")
    cuda = [t.is_cuda for t in (image1, image2, disp) + (() if valid is None else (valid,))]
    if any(cuda) != all(cuda):
        raise ValueError("spatial_pair: all tensors on one device expected")
    if not cuda[0]:
        return spatial_pair_host(image1, image2, disp, params, valid, out_size, out_dtype)
    from .. import _spatial_lib as S, ops
    if image1.dtype not in _DTYPES or image2.dtype != image1.dtype:
        raise TypeError(f"spatial_pair: images must both be uint8 or both float32, got {image1.dtype} and {image2.dtype}")
    bsz, h, w, h_out, w_out = _check(image1.shape, image2.shape, disp.shape, None if valid is None else valid.shape, params, out_size)
    image1, image2 = ops._req(image1, "spatial_pair: image1", image1.dtype), ops._req(image2, "spatial_pair: image2", image1.dtype)
    disp = ops._req(disp, "spatial_pair: disp")
    if valid is not None:
        valid = ops._req(valid, "spatial_pair: valid", torch.uint8)
    dev = image1.device
    with ops._guard(dev):
        out1 = torch.empty((bsz, 3, h_out, w_out), device=dev, dtype=out_dtype)
        out2 = torch.empty((bsz, 3, h_out, w_out), device=dev, dtype=out_dtype)
        disps = [torch.empty((p.ch, p.cw), device=dev, dtype=torch.float32) for p in params]
        valids = None if valid is None else [torch.empty((p.ch, p.cw), device=dev, dtype=torch.uint8) for p in params]
        dptr = (C.c_void_p * bsz)(*[t.data_ptr() for t in disps])
        vptr = None if valids is None else (C.c_void_p * bsz)(*[t.data_ptr() for t in valids])
        oh, ow = (0, 0) if out_size is None else (h_out, w_out)
        S.check(S.load().spt_spatial_pair(ops._p(image1), ops._p(image2), _DTYPES[image1.dtype], ops._p(disp), ops._p(valid), bsz, h, w,
                                          c_samples(params), ops._p(out1), ops._p(out2), _DTYPES[out_dtype], oh, ow, dptr, vptr, ops._stream()),
                "spatial_pair")
    return out1, out2, disps, valids


def augment_frames(image1: torch.Tensor, image2: torch.Tensor, disp: torch.Tensor, photo_spec, spatial_spec: SpatialSpec, seed: int, index0: int,
                   scales, lr_size, valid=None):
    """The reference's `*WoCrop.__call__` on full frames: photometric jitter, eraser (`harness.augment`, `photo_spec`; None skips them),
    then rescale / flip / crop of sample b to (round(h_lr s_b), round(w_lr s_b)) and the final resize of the images to lr_size =
    (h_lr, w_lr).  -> (image1, image2 fp32 [B,3,h_lr,w_lr], disps, valids): what `batches.build_train_batch(image1, image2, disps, scales,
    ...)` takes.  All parameters are hashed from (seed, index0 + b)."""
    bsz, _, h, w = image1.shape
    h_lr, w_lr = int(lr_size[0]), int(lr_size[1])
    scales = [float(s) for s in scales]
    if len(scales) != bsz:
        raise ValueError(f"augment_frames: {len(scales)} scales for {bsz} samples")
    if photo_spec is not None:
        from .augment import augment_pair
        image1, image2 = augment_pair(image1, image2, photo_spec, seed, index0, out_dtype=torch.uint8)
    sizes = [(round(h_lr * s), round(w_lr * s)) for s in scales]
    params = draw_spatial(spatial_spec, seed, index0, bsz, h, w, sizes)
    return spatial_pair(image1, image2, disp, params, valid=valid, out_size=(h_lr, w_lr), out_dtype=torch.float32)
