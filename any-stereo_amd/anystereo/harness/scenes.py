"""Procedural stereo scenes: a data source of the model's own kind — a pair renderable at any resolution whose exact disparity,
right-view disparity and occlusion mask can be evaluated at any query coordinate and any scale, made on the device with no file
read, no upload and no host synchronisation (csrc/scenes/scenes.hip, include/anystereo_scenes.h; DESIGN.md "Procedural scenes").

A scene is a function of (spec, seed, index) and nothing else.

    spec = SceneSpec()                      # six layers, aspect 0.5
    img1, img2 = render_pair(spec, seed, index0, batch, h, w, device)
    disp, disp_right, noc = ground_truth(spec, seed, [(h, w), ...], [index, ...], device)      # ragged lists
    d = disparity_at(spec, seed, [index, ...], hr_coord, mul=[w_hr, ...])                      # [B,1,Q], any coordinates

On CUDA tensors / devices the three calls run the HIP kernels; otherwise `render_pair_host`, `ground_truth_host` and
`disparity_at_host`, which state the kernels' arithmetic operation by operation with torch ops: fp32 add, multiply, divide, floor
and compare in the kernels' order, integer hashes in int64 — bit-identical results (tests/test_scenes_gpu.py).  An edit of one
side is an edit of the other.

`scene_pairs` feeds `harness.evaluate.evaluate`, `scene_train_batch` feeds `Trainer.step`.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields
from typing import List

import numpy as np
import torch

from . import batches
from .batches import _mix32

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
_F = np.float32
MAX_LAYERS, MAX_OCTAVES = 8, 6
# hash slots of a layer (csrc/scenes/scenes.hip): slot = layer * 64 + j
_KIND, _CU, _CV, _A, _B, _K, _ALPHA, _BETA, _GAMMA, _COLOUR, _OCTAVE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 32
_NOISE = MAX_LAYERS * 64
# validate() proves the background plane positive over this box of (u, v): the frame, the right view's reach beyond it (u + d) and
# every query up to coordinate +-2 in hr_coord's convention
BG_BOX = (-0.5, 1.5)
GREY_MAX = 254.999


def _f32(x) -> float:
    return float(_F(x))


@dataclass(frozen=True)
class SceneSpec:
    """What the layers of a scene are drawn from (scn_spec).  Lengths are fractions of the image WIDTH; every value is held as the
    fp32 number the kernels receive."""
    n_layers: int = 6        # the background included, at most 8
    octaves: int = 3         # of value noise
    aspect: float = 0.5      # height / width of the scene, a constant of the spec: every render size shows the same shapes
    bg_min: float = 0.02     # background plane: alpha in [bg_min, bg_max] ...
    bg_max: float = 0.04
    bg_slope: float = 0.005  # ... |beta|, |gamma| <= bg_slope
    d_min: float = 0.05      # layers 1..: alpha in [d_min, d_max] ...
    d_max: float = 0.12
    slope_max: float = 0.05  # ... |beta|, |gamma| <= slope_max (at most 0.05)
    size_min: float = 0.08   # half extents of a support
    size_max: float = 0.25
    shear_max: float = 0.5
    lattice: float = 12.0    # cells of the first noise octave per unit of u
    contrast: float = 60.0   # grey levels of the first octave
    noise: float = 2.0       # image2: +-noise per value

    def __post_init__(self):
        for f in fields(self):
            v = getattr(self, f.name)
            object.__setattr__(self, f.name, int(v) if f.name in ("n_layers", "octaves") else _f32(v))

    def validate(self) -> "SceneSpec":
        """Raises ValueError unless the spec is renderable and every plane it can draw is positive over its support box:
        a layer's support lies within |du| <= a + |k| b and |dv| <= b / aspect of its centre, so its smallest disparity is at least
        d_min - slope_max (size_max (1 + shear_max)) - slope_max size_max / aspect; the background is proved over BG_BOX."""
        if not 1 <= self.n_layers <= MAX_LAYERS:
            raise ValueError(f"SceneSpec: n_layers={self.n_layers} outside [1, {MAX_LAYERS}]")
        if not 1 <= self.octaves <= MAX_OCTAVES:
            raise ValueError(f"SceneSpec: octaves={self.octaves} outside [1, {MAX_OCTAVES}]")
        if not (self.aspect > 0 and self.lattice > 0 and 0 < self.size_min <= self.size_max):
            raise ValueError(f"SceneSpec: aspect={self.aspect}, lattice={self.lattice}, size_min={self.size_min}, size_max={self.size_max}: "
                             "positive values and size_min <= size_max expected")
        if not (0 <= self.slope_max <= _f32(0.05) and 0 <= self.bg_slope <= _f32(0.05)):
            raise ValueError(f"SceneSpec: slope_max={self.slope_max}, bg_slope={self.bg_slope}: slopes in [0, 0.05] expected")
        if not (self.bg_min <= self.bg_max and self.d_min <= self.d_max < 0.5 and self.shear_max >= 0 and self.contrast >= 0 and self.noise >= 0):
            raise ValueError("SceneSpec: need bg_min <= bg_max, d_min <= d_max < 0.5, and non-negative shear_max, contrast, noise")
        reach = max(abs(BG_BOX[0] - 0.5), abs(BG_BOX[1] - 0.5))
        bg_low = self.bg_min - 2 * self.bg_slope * reach
        if not bg_low > 0:
            raise ValueError(f"SceneSpec: the background plane can reach {bg_low:.4g} <= 0 inside u, v in {BG_BOX} "
                             f"(bg_min={self.bg_min}, bg_slope={self.bg_slope})")
        if self.n_layers > 1:
            low = self.d_min - self.slope_max * self.size_max * (1 + self.shear_max) - self.slope_max * self.size_max / self.aspect
            if not low > 0:
                raise ValueError(f"SceneSpec: a layer's plane can reach {low:.4g} <= 0 on its support (d_min={self.d_min}, "
                                 f"slope_max={self.slope_max}, size_max={self.size_max}, shear_max={self.shear_max}, aspect={self.aspect})")
        return self

    def c_struct(self):
        from .. import _scenes_lib as S
        return S.Spec(**{f.name: getattr(self, f.name) for f in fields(self)})


# ------------------------------------------------------------------------------------------------
# hashes and the derived layers (scene_key, slot_hash, uniform, derive_layer)
# ------------------------------------------------------------------------------------------------

def scene_key(seed: int, index: int) -> int:
    seed = int(seed) & _M64
    t = _mix32(((seed & _M32) + 0x9E3779B9) & _M32)
    t = _mix32(t ^ (seed >> 32))
    return _mix32(t ^ (((int(index) & _M32) * 0x85EBCA6B) & _M32))


def _slot_hash(base: int, slot: int) -> int:
    return _mix32(base ^ _mix32((slot + 0x9E3779B9) & _M32))


def _uniform(h: int):
    return _F(h >> 8) * _F(2.0 ** -24)


@dataclass(frozen=True)
class Layer:
    """The host's copy of one derived layer: Python floats holding the kernels' fp32 values."""
    kind: int
    cu: float
    cv: float
    inv_a: float
    k: float
    inv_b: float
    alpha: float
    beta: float
    gamma: float
    col: tuple
    a: float
    b: float
    omb: float
    okey: tuple   # lattice key per octave

    def row(self):
        """The layer as scn_layers writes it (SCN_LAYER_FLOATS values)."""
        return [float(self.kind), self.cu, self.cv, self.inv_a, self.k, self.inv_b, self.alpha, self.beta, self.gamma, *self.col, self.a, self.b,
                self.omb, 0.0]


def layers(spec: SceneSpec, seed: int, index: int) -> List[Layer]:
    """The derived parameters of scene (spec, seed, index), every operation in fp32 in derive_layer's order."""
    base = scene_key(seed, index)
    sp = {f.name: _F(getattr(spec, f.name)) for f in fields(spec) if f.name not in ("n_layers", "octaves")}
    one, two = _F(1), _F(2)
    out = []
    for l in range(spec.n_layers):
        s0 = l * 64
        U = lambda j: _uniform(_slot_hash(base, s0 + j))  # noqa: E731
        if l == 0:
            kind, cu, cv, a, b, k = 0, _F(0.5), _F(0.5), one, one, _F(0)
            lo, hi, slope = sp["bg_min"], sp["bg_max"], sp["bg_slope"]
        else:
            kind = 1 + (_slot_hash(base, s0 + _KIND) & 1)
            cu = _F(0.1) + _F(0.8) * U(_CU)
            cv = _F(0.1) + _F(0.8) * U(_CV)
            a = sp["size_min"] + (sp["size_max"] - sp["size_min"]) * U(_A)
            b = sp["size_min"] + (sp["size_max"] - sp["size_min"]) * U(_B)
            k = (U(_K) * two - one) * sp["shear_max"]
            lo, hi, slope = sp["d_min"], sp["d_max"], sp["slope_max"]
        alpha = lo + (hi - lo) * U(_ALPHA)
        beta = (U(_BETA) * two - one) * slope
        gamma = (U(_GAMMA) * two - one) * slope
        col = tuple(float(_F(40) + _F(170) * U(_COLOUR + c)) for c in range(3))
        vals = [cu, cv, one / a, k, one / b, alpha, beta, gamma]
        assert all(isinstance(v, np.float32) for v in vals + [a, b]), "layers: an operation left fp32"
        out.append(Layer(kind, *(float(v) for v in vals), col, float(a), float(b), float(one - beta),
                         tuple(_slot_hash(base, s0 + _OCTAVE + o) for o in range(spec.octaves))))
    return out


# ------------------------------------------------------------------------------------------------
# the per-point functions, on fp32 tensors of one shape (plane, inside, seen_left, left_column, seen_right, noc_of, texture)
# ------------------------------------------------------------------------------------------------

def _plane(L: Layer, u, v):
    return (L.alpha + L.beta * (u - L.cu)) + L.gamma * (v - L.cv)


def _inside(L: Layer, aspect: float, u, v):
    if L.kind == 0:
        return torch.ones_like(u, dtype=torch.bool)
    du, dv = u - L.cu, (v - L.cv) * aspect
    p, q = (du + L.k * dv) * L.inv_a, dv * L.inv_b
    if L.kind == 1:
        return p * p + q * q <= 1.0
    return (p.abs() <= 1.0) & (q.abs() <= 1.0)


def _seen_left(Ls, spec, u, v):
    best = torch.zeros_like(u, dtype=torch.int64)
    bd = _plane(Ls[0], u, v)
    for l in range(1, len(Ls)):
        d = _plane(Ls[l], u, v)
        m = _inside(Ls[l], spec.aspect, u, v) & (d > bd)
        bd = torch.where(m, d, bd)
        best = torch.where(m, torch.full_like(best, l), best)
    return best, bd


def _left_column(L: Layer, ur, v):
    bc = float(_F(L.beta) * _F(L.cu))
    # a tensor divisor: a true division, whatever a backend does with a scalar one
    return (((ur + L.alpha) - bc) + L.gamma * (v - L.cv)) / torch.full_like(ur, L.omb)


def _seen_right(Ls, spec, ur, v):
    best = torch.zeros_like(ur, dtype=torch.int64)
    bu = _left_column(Ls[0], ur, v)
    bd = _plane(Ls[0], bu, v)
    for l in range(1, len(Ls)):
        ul = _left_column(Ls[l], ur, v)
        d = _plane(Ls[l], ul, v)
        m = _inside(Ls[l], spec.aspect, ul, v) & (d > bd)
        bd = torch.where(m, d, bd)
        bu = torch.where(m, ul, bu)
        best = torch.where(m, torch.full_like(best, l), best)
    return best, bd, bu


def _noc_of(Ls, spec, u, v, best, d):
    ur = u - d
    lr, _, _ = _seen_right(Ls, spec, ur, v)
    return ((lr == best) & (ur >= 0.0)).to(torch.uint8)


def _uniform_t(h):
    return (h >> 8).float() * (2.0 ** -24)


def _lattice(key: int, ix, iy):
    h = _mix32(key ^ (((ix & _M32) * 0x27D4EB2F) & _M32))
    h = _mix32(h ^ (((iy & _M32) * 0x165667B1) & _M32))
    return _uniform_t(h)


def _texture_one(L: Layer, spec, u, v):
    s, t = u - L.cu, (v - L.cv) * spec.aspect
    acc = torch.zeros_like(u)
    f, amp = _F(spec.lattice), _F(spec.contrast)
    for o in range(spec.octaves):
        key = L.okey[o]
        xs, ys = s * float(f), t * float(f)
        x0, y0 = xs.floor(), ys.floor()
        fx, fy = xs - x0, ys - y0
        ix, iy = x0.long(), y0.long()
        a, b = _lattice(key, ix, iy), _lattice(key, ix + 1, iy)
        c, d = _lattice(key, ix, iy + 1), _lattice(key, ix + 1, iy + 1)
        top, bot = a + fx * (b - a), c + fx * (d - c)
        n = top + fy * (bot - top)
        acc = acc + float(amp) * (n - 0.5)
        f, amp = f * _F(2), amp * _F(0.5)
    return acc


def _texture(Ls, spec, best, u, v):
    """(texture [n], base colour [3, n]) of layer best[i] at its surface point (u[i], v[i]) of the left view."""
    tex = torch.zeros_like(u)
    col = torch.zeros((3,) + tuple(u.shape), dtype=torch.float32, device=u.device)
    for l, L in enumerate(Ls):
        m = best == l
        if bool(m.any()):
            tex[m] = _texture_one(L, spec, u[m], v[m])
            for c in range(3):
                col[c][m] = L.col[c]
    return tex, col


def _axis(n: int, device):
    """make_coord of one axis: fl(-1 + 1/n) + fl(2/n) * j."""
    return float(_F(-1.0 + 1.0 / n)) + float(_F(2.0 / n)) * torch.arange(n, device=device).float()


def _grid_uv(h: int, w: int, device):
    y, x = torch.meshgrid(_axis(h, device), _axis(w, device), indexing="ij")
    return ((x.reshape(-1) + 1.0) * 0.5), ((y.reshape(-1) + 1.0) * 0.5)


# ------------------------------------------------------------------------------------------------
# the three host restatements
# ------------------------------------------------------------------------------------------------

def _checked(spec: SceneSpec) -> SceneSpec:
    if not isinstance(spec, SceneSpec):
        raise TypeError(f"expected a SceneSpec, got {type(spec).__name__}")
    return spec.validate()


@torch.no_grad()
def colour_at_host(spec: SceneSpec, seed: int, index: int, u, v, view: str = "left"):
    """The colour function of one view, [3, n] before the clamp and without image2's noise, at points (u, v) in [0, 1] (fp32 tensors of one
    shape) — what render_pair evaluates at the pixel centres."""
    Ls = layers(_checked(spec), seed, index)
    if view == "left":
        best, _ = _seen_left(Ls, spec, u, v)
        tex, col = _texture(Ls, spec, best, u, v)
    else:
        best, _, ul = _seen_right(Ls, spec, u, v)
        tex, col = _texture(Ls, spec, best, ul, v)
    return col + tex


@torch.no_grad()
def render_pair_host(spec: SceneSpec, seed: int, index0: int, batch: int, h: int, w: int, device="cpu"):
    """(image1, image2) fp32 [B,3,h,w] as scn_render_pair writes them."""
    _checked(spec)
    if batch < 1 or h < 1 or w < 1:
        raise ValueError(f"render_pair_host: B={batch} h={h} w={w} must be positive")
    u, v = _grid_uv(h, w, device)
    pix = torch.arange(h * w, device=device)
    im1, im2 = [], []
    for b in range(batch):
        nkey = _slot_hash(scene_key(seed, index0 + b), _NOISE)
        left = colour_at_host(spec, seed, index0 + b, u, v, "left")
        right = colour_at_host(spec, seed, index0 + b, u, v, "right")
        noise = torch.stack([(_uniform_t(_mix32(nkey ^ (pix * 3 + c))) * 2.0 - 1.0) * spec.noise for c in range(3)])
        im1.append(left.clamp(0.0, GREY_MAX).view(3, h, w))
        im2.append((right + noise).clamp(0.0, GREY_MAX).view(3, h, w))
    return torch.stack(im1).contiguous(), torch.stack(im2).contiguous()


@torch.no_grad()
def ground_truth_host(spec: SceneSpec, seed: int, sizes, indices, device="cpu", want=("disp", "disp_right", "noc")):
    """(disp, disp_right, noc): three lists of [h_b, w_b] tensors (None where not wanted) as scn_ground_truth writes them."""
    _checked(spec)
    out = ([], [], [])
    for (h, w), index in zip(sizes, indices):
        Ls = layers(spec, seed, index)
        u, v = _grid_uv(h, w, device)
        wf = float(w)
        disp = right = noc = None
        if "disp" in want or "noc" in want:
            best, d = _seen_left(Ls, spec, u, v)
            if "disp" in want:
                disp = (d * wf).view(h, w)
            if "noc" in want:
                noc = _noc_of(Ls, spec, u, v, best, d).view(h, w)
        if "disp_right" in want:
            right = (_seen_right(Ls, spec, u, v)[1] * wf).view(h, w)
        for lst, t in zip(out, (disp, right, noc)):
            lst.append(t)
    return out


@torch.no_grad()
def disparity_at_host(spec: SceneSpec, seed: int, indices, coord, mul, noc: bool = False, view: str = "left"):
    """out [B,1,Q] (and noc uint8 [B,Q]) as scn_disparity_at writes them: coord [B,Q,2] = (row, col) in hr_coord's convention."""
    _checked(spec)
    bsz, q = coord.shape[:2]
    outs, nocs = [], []
    for b in range(bsz):
        Ls = layers(spec, seed, indices[b])
        u, v = (coord[b, :, 1] + 1.0) * 0.5, (coord[b, :, 0] + 1.0) * 0.5
        if view == "right":
            d = _seen_right(Ls, spec, u, v)[1]
        else:
            best, d = _seen_left(Ls, spec, u, v)
            if noc:
                nocs.append(_noc_of(Ls, spec, u, v, best, d))
        outs.append((d * _f32(mul[b])).view(1, q))
    out = torch.stack(outs).contiguous()
    return (out, torch.stack(nocs).contiguous()) if noc else out


# ------------------------------------------------------------------------------------------------
# the public calls: HIP on CUDA, the restatements otherwise
# ------------------------------------------------------------------------------------------------

def _seed64(seed: int) -> int:
    return int(seed) & _M64


def _want(want):
    want = tuple(want)
    if not want or any(k not in ("disp", "disp_right", "noc") for k in want):
        raise ValueError(f"ground_truth: want={want!r}: a non-empty subset of ('disp', 'disp_right', 'noc')")
    return want


def _per_sample(values, n: int, what: str):
    values = list(values)
    if len(values) != n:
        raise ValueError(f"{what}: {len(values)} values for {n} samples")
    return values


def render_pair(spec: SceneSpec, seed: int, index0: int, batch: int, h: int, w: int, device="cpu"):
    """(image1, image2) fp32 [B,3,h,w] in [0, 254.999]: both views of scenes index0 .. index0 + B - 1 at (h, w).  One launch."""
    device = torch.device(device)
    if device.type != "cuda":
        return render_pair_host(spec, seed, index0, batch, h, w, device)
    from .. import _scenes_lib as S, ops
    _checked(spec)
    batch, h, w = int(batch), int(h), int(w)
    if batch < 1 or h < 1 or w < 1:  # refused here as well: an empty allocation has no pointer to refuse
        raise RuntimeError(f"render_pair: B={batch} h={h} w={w} must be positive")
    with torch.cuda.device(device):
        im1 = torch.empty((batch, 3, h, w), device=device, dtype=torch.float32)
        im2 = torch.empty((batch, 3, h, w), device=device, dtype=torch.float32)
        S.check(S.load().scn_render_pair(ops._p(im1), ops._p(im2), batch, h, w, C.byref(spec.c_struct()), _seed64(seed), int(index0),
                                         ops._stream()), "render_pair")
    return im1, im2


def ground_truth(spec: SceneSpec, seed: int, sizes, indices, device="cpu", want=("disp", "disp_right", "noc")):
    """Ragged ground truth of scenes `indices` at `sizes` [(h_b, w_b)]: (disp, disp_right, noc), three lists of [h_b, w_b] tensors (fp32,
    fp32, uint8; a list of None for what `want` leaves out) in pixels of the sample's own width.  One launch per 8 samples."""
    device, want = torch.device(device), _want(want)
    sizes = [(int(h), int(w)) for h, w in sizes]
    indices = _per_sample(indices, len(sizes), "ground_truth")
    if not sizes:
        raise ValueError("ground_truth: no samples")
    if device.type != "cuda":
        return ground_truth_host(spec, seed, sizes, indices, device, want)
    from .. import _scenes_lib as S, ops
    _checked(spec)
    if any(h < 1 or w < 1 for h, w in sizes):
        raise RuntimeError(f"ground_truth: sizes {sizes} must be positive")
    with torch.cuda.device(device):
        new = lambda key, hw, dt: torch.empty(hw, device=device, dtype=dt) if key in want else None  # noqa: E731
        disp = [new("disp", hw, torch.float32) for hw in sizes]
        right = [new("disp_right", hw, torch.float32) for hw in sizes]
        noc = [new("noc", hw, torch.uint8) for hw in sizes]
        table = (S.GtSample * len(sizes))(*[S.GtSample(ops._p(d), ops._p(r), ops._p(n), h, w, int(i))
                                            for d, r, n, (h, w), i in zip(disp, right, noc, sizes, indices)])
        S.check(S.load().scn_ground_truth(table, len(sizes), C.byref(spec.c_struct()), _seed64(seed), ops._stream()), "ground_truth")
    return disp, right, noc


def disparity_at(spec: SceneSpec, seed: int, indices, coord: torch.Tensor, mul, noc: bool = False, view: str = "left"):
    """The exact disparity of scenes `indices` at arbitrary queries: coord fp32 [B,Q,2] = (row, col) in [-1, 1] (hr_coord's convention;
    values outside are evaluated, not clamped) -> fp32 [B,1,Q] = mul[b] * d, `mul` the width in whose pixels sample b is wanted.
    noc=True: also the exact mask uint8 [B,Q].  view="right": the right view's disparity at right-view coordinates (no mask)."""
    if view not in ("left", "right"):
        raise ValueError(f"disparity_at: view={view!r} (left | right)")
    if noc and view == "right":
        raise ValueError("disparity_at: the mask is defined for the left view only")
    if coord.dim() != 3 or coord.shape[-1] != 2 or coord.dtype != torch.float32 or coord.numel() == 0:
        raise ValueError(f"disparity_at: coord must be a non-empty float32 [B,Q,2] tensor, got {tuple(coord.shape)} {coord.dtype}")
    bsz, q = coord.shape[:2]
    indices = _per_sample(indices, bsz, "disparity_at")
    mul = _per_sample(mul, bsz, "disparity_at")
    if not coord.is_cuda:
        return disparity_at_host(spec, seed, indices, coord, mul, noc, view)
    from .. import _scenes_lib as S, ops
    _checked(spec)
    coord = ops._req(coord, "disparity_at: coord")
    with ops._guard(coord.device):
        out = torch.empty((bsz, 1, q), device=coord.device, dtype=torch.float32)
        mask = torch.empty((bsz, q), device=coord.device, dtype=torch.uint8) if noc else None
        S.check(S.load().scn_disparity_at(ops._p(coord), ops._p(out), ops._p(mask), bsz, q, (C.c_float * bsz)(*[float(m) for m in mul]),
                                          (C.c_int * bsz)(*[int(i) for i in indices]), 1 if view == "right" else 0,
                                          C.byref(spec.c_struct()), _seed64(seed), ops._stream()), "disparity_at")
    return (out, mask) if noc else out


# ------------------------------------------------------------------------------------------------
# what the harness consumes
# ------------------------------------------------------------------------------------------------

def scene_pairs(spec: SceneSpec, seed: int, n: int, h: int, w: int, protocol: str = "things", device="cpu", index0: int = 0):
    """`harness.evaluate.evaluate`'s tuples (image1, image2, gt, valid, extra) of scenes index0 .. index0 + n - 1, one pair each:
    `extra` is the right view's ground truth for "things" (the Evaluator forms the left-right mask from it) and the exact noc mask
    for the other protocols.  Nothing is read from a file or copied from the host."""
    from .evaluate import PROTOCOLS
    if protocol not in PROTOCOLS:
        raise ValueError(f"scene_pairs: unknown protocol {protocol!r} (one of {sorted(PROTOCOLS)})")
    device = torch.device(device)
    for i in range(int(index0), int(index0) + int(n)):
        im1, im2 = render_pair(spec, seed, i, 1, h, w, device)
        things = protocol == "things"
        disp, right, noc = ground_truth(spec, seed, [(h, w)], [i], device, want=("disp", "disp_right") if things else ("disp", "noc"))
        gt = disp[0].view(1, h, w)
        extra = (right[0] if things else noc[0]).view(1, h, w)
        yield im1, im2, gt, torch.ones_like(gt), extra


def scene_scales(seed: int, step: int, batch: int, scale_min: float, scale_max: float, rank: int = 0, world: int = 1) -> List[float]:
    """The scales of a training batch: hashed per sample from (seed, step, rank, b), rounded to fp32 as `ops.host_scales` does."""
    from ..ops import host_scales
    base = scene_key(int(seed) ^ 0x5CA1E5, int(step) * int(world) + int(rank))
    us = [(_slot_hash(base, b) >> 8) * 2.0 ** -24 for b in range(batch)]
    return host_scales([scale_min + (scale_max - scale_min) * u for u in us], batch, "scene_scales")


def scene_train_batch(spec: SceneSpec, seed: int, step: int, batch: int, h_lr: int = 160, w_lr: int = 320, scale_min: float = 1.0,
                      scale_max: float = 2.95, mode: str = "dense", rank: int = 0, world: int = 1, device="cpu", low_disp: bool = True,
                      augment=None, spatial=None, frame_hw=None):
    """`build_train_batch(...)`'s tuple (image1, image2, hr_coord, hr_disp, scale, low_disp) for step `step` of rank `rank`: fresh scenes
    (index = (step * world + rank) * batch + b) rendered at (h_lr, w_lr), one hashed scale per sample, ragged ground-truth crops
    rendered at (round(h_lr s), round(w_lr s)) in their own pixels, the queries drawn by `build_train_batch` with a seed of this
    (step, rank).  On a CUDA device: four launches and no host synchronisation.  `augment`: a `harness.augment.PhotoSpec` — the rendered
    pair goes through the reference's photometric augmentation and eraser (parameters hashed per scene index) before the batch is
    built: up to three more launches, ground truth and queries unchanged.  None (the default): nothing of that runs.
    `spatial`: a `harness.spatial.SpatialSpec` — the scenes are rendered as full frames of `frame_hw` (default 540 x 960) with full-frame
    ground truth and go through `harness.spatial.augment_frames`, the reference's whole `*WoCrop.__call__`: `augment` (if given), then
    rescale / flip / crop to (round(h_lr s), round(w_lr s)) and the final resize of the images to (h_lr, w_lr); a sparse spec takes the
    scenes' exact non-occlusion mask as `valid`, and the returned disparity crops are set to 0 wherever the returned validity is 0,
    so that `build_train_batch(mode="sparse")`, which reads validity as disp > 0, sees the same pixels valid in rescaled and in
    passed-through samples (a passed-through occluded pixel keeps a positive disparity otherwise).  A sparse spec with
    do_flip="hf" yields negative disparities, as the reference's: no pixel of a flipped sample is valid to that mode.  None (the default): nothing of that runs and the outputs are what they were."""
    batch = int(batch)
    scales = scene_scales(seed, step, batch, scale_min, scale_max, rank, world)
    first = (int(step) * int(world) + int(rank)) * batch
    indices = [first + b for b in range(batch)]
    if spatial is not None:
        from .spatial import augment_frames
        fh, fw = (540, 960) if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1]))
        im1, im2 = render_pair(spec, seed, first, batch, fh, fw, device)
        sparse = spatial.kind == "sparse"
        full, _, noc = ground_truth(spec, seed, [(fh, fw)] * batch, indices, device, want=("disp", "noc") if sparse else ("disp",))
        im1, im2, disps, valids = augment_frames(im1, im2, torch.stack(full), augment, spatial, seed, first, scales, (h_lr, w_lr),
                                                 valid=torch.stack(noc) if sparse else None)
        if sparse:
            disps = [torch.where(v != 0, d, torch.zeros_like(d)) for d, v in zip(disps, valids)]
        return batches.build_train_batch(im1, im2, disps, scales, (int(seed) + int(step) * int(world) + int(rank)) & _M64, mode=mode,
                                         low_disp=low_disp)
    if frame_hw is not None:
        raise ValueError("scene_train_batch: frame_hw is the frame of the spatial augmentation; it needs `spatial`")
    im1, im2 = render_pair(spec, seed, first, batch, h_lr, w_lr, device)
    if augment is not None:
        from .augment import augment_pair
        im1, im2 = augment_pair(im1, im2, augment, seed, first)
    sizes = [(round(h_lr * s), round(w_lr * s)) for s in scales]
    disps, _, _ = ground_truth(spec, seed, sizes, indices, device, want=("disp",))
    return batches.build_train_batch(im1, im2, disps, scales, (int(seed) + int(step) * int(world) + int(rank)) & _M64, mode=mode,
                                     low_disp=low_disp)


def train_batch_indices(step: int, batch: int, rank: int = 0, world: int = 1) -> List[int]:
    """The scene indices of `scene_train_batch(step=..., batch=..., rank=..., world=...)`."""
    first = (int(step) * int(world) + int(rank)) * int(batch)
    return [first + b for b in range(int(batch))]
