"""Multi-scale training batches: what of a sample is a function of (ground-truth crop, scale, seed) — the tail of
StereoDataset.__getitem__ (models/*/stereo_datasets.py:148-212) after the augmentor: the queries, the ground truth gathered at
them and the 1/4-resolution target of --supervise_init.

`build_train_batch` makes them on the device (`ops.train_queries`, `ops.low_disp`: csrc/train_batch.hip) for CUDA inputs and with the
plain-torch restatements below otherwise; `train_queries_host` / `low_disp_host` state the kernels' arithmetic operation by operation
(bit-identical results, the drawn pixels included) and, given `indices`, replay somebody else's draws — the reference's
np.random.choice lists of tests/golden/train_batch.npz.

Modes (include/anystereo_hip.h, as_train_queries): "dense" (SceneFlow, multi-scale: Q distinct pixels at random), "dense_all"
(without_mutli_scale: every pixel in raster order), "sparse" (KITTI / Middlebury, multi-scale: the valid pixels first, filled up with
invalid ones at random; Q of the valid ones at random when there are more than Q), "sparse_ordered" (without_mutli_scale: valid pixels,
then invalid pixels, both in raster order).

Seeds.  The draws of sample b are a function of (seed, b, mode) and nothing else: the same seed gives the same batch.  Under DDP every
rank must therefore pass a seed of its own and a new one every step, e.g. `seed = base + step * world_size + rank`; ranks that share
a seed draw the same pixels in every sample of the same size."""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from ..ops import TRAIN_QUERY_MODES as MODES, host_scales   # the mode table (AS_TQ_*) and the fp32 rounding of the scales: kept once

ROUNDS = 6
_M32 = 0xFFFFFFFF


def _mode_id(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r}: one of {sorted(MODES)}")
    return MODES[mode]


# ------------------------------------------------------------------------------------------------
# the keyed bijection (csrc/train_batch.hip: mix32, derive_keys, feistel, permute)
# ------------------------------------------------------------------------------------------------

def _mix32(x):
    """The 32-bit multiply-xorshift mix, on a Python int or an int64 tensor holding values below 2^32 (both multipliers are below
    2^31, so no product reaches 2^63)."""
    x = x ^ (x >> 16)
    x = (x * 0x21F0AAAD) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x735A2D97) & _M32
    return x ^ (x >> 15)


def round_keys(seed: int, b: int, mode: str) -> List[int]:
    """The ROUNDS 32-bit round keys of sample `b`: a function of (seed mod 2^64, b, mode)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    m = _mode_id(mode)
    keys = []
    for r in range(ROUNDS):
        t = _mix32(((seed & _M32) + 0x9E3779B9 * (r + 1)) & _M32)
        t = _mix32(t ^ (seed >> 32))
        t = _mix32(t ^ ((int(b) * 0x85EBCA6B) & _M32))
        keys.append(_mix32(t ^ m))
    return keys


def _feistel(x: torch.Tensor, bits: int, keys: Sequence[int]) -> torch.Tensor:
    lb = bits >> 1
    rb = bits - lb
    for k in keys:
        left, right = x >> rb, x & ((1 << rb) - 1)
        nr = left ^ (_mix32(right ^ k) & ((1 << lb) - 1))
        x = (right << lb) | nr
        lb, rb = rb, lb
    return x


def permute(j: torch.Tensor, n: int, keys: Sequence[int]) -> torch.Tensor:
    """pi(j) for the keyed bijection pi of [0, n): a Feistel network over the next power-of-two domain, walked until the value is
    below n.  `j` int64, 0 <= j < n."""
    n = int(n)
    bits = 0 if n <= 1 else (n - 1).bit_length()
    x = _feistel(j, bits, keys)
    while True:
        out = x >= n
        if not bool(out.any()):
            return x
        x = torch.where(out, _feistel(x, bits, keys), x)


# ------------------------------------------------------------------------------------------------
# plain-torch restatements of the two kernels
# ------------------------------------------------------------------------------------------------

def _check_disps(disps, what):
    if not isinstance(disps, (list, tuple)) or len(disps) == 0:
        raise ValueError(f"{what}: disps must be a non-empty list of [h, w] tensors")
    for b, d in enumerate(disps):
        if not isinstance(d, torch.Tensor) or d.dim() != 2 or d.dtype != torch.float32 or d.numel() == 0:
            raise ValueError(f"{what}: disps[{b}] must be a non-empty float32 [h, w] tensor")


def train_queries_host(disps, q: int, mode: str, seed: int, indices=None):
    """(hr_coord [B,Q,2], hr_disp [B,1,Q], index int32 [B,Q], n_valid int32 [B]) as `as_train_queries` forms them, in plain torch on
    the device of the crops.  `indices` (a list of B integer sequences, None entries allowed): the random draw of sample b is
    replaced by indices[b] — positions in the list the mode draws from (all pixels; the valid pixels when Q < V; else the invalid
    ones)."""
    _check_disps(disps, "train_queries_host")
    _mode_id(mode)
    q = int(q)
    coords, values, index, n_valid = [], [], [], []
    for b, d in enumerate(disps):
        h, w = d.shape
        n, dev = h * w, d.device
        if (n != q) if mode == "dense_all" else (n < q):
            raise ValueError(f"train_queries_host: sample {b}: Q={q} queries from N={n} pixels in mode {mode}")
        flat = d.reshape(-1)
        keys = round_keys(seed, b, mode)
        given = None if indices is None or indices[b] is None else torch.as_tensor(indices[b], dtype=torch.int64, device=dev)

        def draw(k, dom):
            if given is not None:
                assert given.numel() == k and (k == 0 or (int(given.min()) >= 0 and int(given.max()) < dom)), (b, k, dom)
                return given
            return permute(torch.arange(k, device=dev), dom, keys)

        if mode == "dense":
            idx, v = draw(q, n), n
        elif mode == "dense_all":
            idx, v = torch.arange(n, device=dev), n
        else:
            valid = flat > 0
            vi, ii = valid.nonzero().view(-1), (~valid).nonzero().view(-1)
            v = int(vi.numel())
            if mode == "sparse_ordered":
                idx = torch.cat((vi, ii))[:q]
            elif q < v:
                idx = vi[draw(q, v)]
            else:
                idx = torch.cat((vi, ii[draw(q - v, n - v)]))
        y, x = idx // w, idx % w
        rh, rw = 2 / (2 * h), 2 / (2 * w)   # make_coord: r = (v1 - v0) / (2 n), seq = v0 + r + (2 r) * arange(n); one fp32 op each
        coords.append(torch.stack(((-1 + rh) + (2 * rh) * y.float(), (-1 + rw) + (2 * rw) * x.float()), dim=-1))
        values.append(flat[idx].view(1, q))
        index.append(idx.to(torch.int32))
        n_valid.append(v)
    return (torch.stack(coords).contiguous(), torch.stack(values).contiguous(), torch.stack(index).contiguous(),
            torch.tensor(n_valid, dtype=torch.int32, device=disps[0].device))


def _bilinear_axis(n_in: int, n_out: int, device):
    """Taps and weights of one axis of ATen's upsample_bilinear2d(align_corners=False), every operation in fp32."""
    ratio = float(torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32))
    src = (ratio * (torch.arange(n_out, device=device).float() + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.float()
    return i0, i1, 1 - l1, l1


def low_disp_host(disps, scales, out_hw):
    """low_disp [B, h_out, w_out] as `as_low_disp` forms it: the bilinear resize of every crop (no antialiasing), then one division
    by (float32)(4 * scale)."""
    _check_disps(disps, "low_disp_host")
    scales = host_scales(scales, len(disps), "low_disp_host")
    h_out, w_out = int(out_hw[0]), int(out_hw[1])
    out = []
    for d, s in zip(disps, scales):
        h, w = d.shape
        y0, y1, ly0, ly1 = _bilinear_axis(h, h_out, d.device)
        x0, x1, lx0, lx1 = _bilinear_axis(w, w_out, d.device)
        r0, r1 = d[y0], d[y1]
        v = ly0.view(-1, 1) * (lx0 * r0[:, x0] + lx1 * r0[:, x1]) + ly1.view(-1, 1) * (lx0 * r1[:, x0] + lx1 * r1[:, x1])
        # a tensor divisor: ATen's CUDA division by a host scalar multiplies by the reciprocal instead
        out.append(v / torch.tensor(4 * s, dtype=torch.float32, device=d.device))
    return torch.stack(out).contiguous()


# ------------------------------------------------------------------------------------------------
# the batch
# ------------------------------------------------------------------------------------------------

def validate(n_valid: torch.Tensor, q: int, mode: str) -> None:
    """The reference's check of the `sparse_ordered` branch (stereo_datasets.py:199-201): more valid pixels than queries is an
    error there; the kernel writes the first Q valid pixels and reports V.  Reads `n_valid` back, so it synchronises — the only
    call of this module that does."""
    _mode_id(mode)
    if mode != "sparse_ordered":
        return
    v = int(n_valid.max())
    if v > int(q):
        raise ValueError(f"sample_q is {int(q)} valid is {v}: Note sample_q is too small, cannot include all valid pixels")


def build_train_batch(image1, image2, disps, scales, seed: int, mode: str = "dense", low_disp: bool = True, q: Optional[int] = None,
                      check: bool = False):
    """(image1, image2, hr_coord [B,Q,2], hr_disp [B,1,Q], scale [B,1][, low_disp [B,h_lr//4,w_lr//4]]) — the tuple
    `train.synthetic_train_batch` returns and `Trainer.step` / `metrics.train_step` take — from the augmented pair
    image1 / image2 [B,3,h_lr,w_lr], the ground-truth crops `disps` (a list of B float32 [h_hr_b, w_hr_b] tensors in high-resolution
    pixels, h_hr = round(h_lr * scale)) and their `scales` (host numbers).  Q = h_lr * w_lr as in the reference (`sample_q`,
    stereo_datasets.py:71) unless `q` is given.  CUDA crops: two calls into csrc/train_batch.hip; nothing is copied from the host
    (`scale` is written by the queries' launch from its argument table) and nothing waits for the device, so the host runs ahead of
    the stream; otherwise the plain-torch restatements.  `check=True` also runs `validate` on the batch, which waits for the device."""
    _check_disps(disps, "build_train_batch")
    b = len(disps)
    if image1.dim() != 4 or image1.shape != image2.shape or image1.shape[0] != b:
        raise ValueError(f"build_train_batch: images {tuple(image1.shape)} / {tuple(image2.shape)} for {b} crops")
    h_lr, w_lr = image1.shape[-2:]
    q = h_lr * w_lr if q is None else int(q)
    sc = host_scales(scales, b, "build_train_batch")
    dev = disps[0].device
    if any(d.device != dev for d in disps) or image1.device != dev or image2.device != dev:
        raise ValueError("build_train_batch: images and crops must share one device")
    if dev.type == "cuda":
        from .. import ops
        # `scale` comes out of the same launch: a copy of a host tensor from pageable memory would wait for the stream
        hr_coord, hr_disp, _, n_valid, scale = ops.train_queries(list(disps), q, mode, seed, scales=sc)
    else:
        hr_coord, hr_disp, _, n_valid = train_queries_host(list(disps), q, mode, seed)
        scale = torch.tensor(sc, dtype=torch.float32).view(b, 1)
    if check:
        validate(n_valid, q, mode)
    out = (image1, image2, hr_coord, hr_disp, scale)
    if low_disp:
        hw = (h_lr // 4, w_lr // 4)
        if dev.type == "cuda":
            from .. import ops
            out = out + (ops.low_disp(list(disps), sc, hw),)
        else:
            out = out + (low_disp_host(list(disps), sc, hw),)
    return out
