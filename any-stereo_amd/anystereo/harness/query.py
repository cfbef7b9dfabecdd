"""§8(f1) query-grid + padding harness: what defines `hr_coord` / `scale` for arbitrary-scale
evaluation (evaluation.py:67-89 pad_for_multi_train, evaluation_validate.py:92-106
pad_for_multi_train_Fixed, models/*/utils/utils.py:7-26 InputPadder, liif.py:32-45 make_coord).

`InputPadder.get_pad_num()` is called but never defined in the reference; from its
use (`coord[p[0]:H-p[1], p[2]:W-p[3]]`) it returns [top, bottom, left, right]."""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from ..nn.liif import make_coord


class InputPadder:
    """Replicate-pad to a multiple of `divis_by` ('sintel' mode splits the padding on both sides)."""

    def __init__(self, dims, mode="sintel", divis_by=8):
        self.ht, self.wd = dims[-2:]
        pad_ht = (((self.ht // divis_by) + 1) * divis_by - self.ht) % divis_by
        pad_wd = (((self.wd // divis_by) + 1) * divis_by - self.wd) % divis_by
        if mode == "sintel":
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, pad_ht // 2, pad_ht - pad_ht // 2]
        else:
            self._pad = [pad_wd // 2, pad_wd - pad_wd // 2, 0, pad_ht]

    def pad(self, *inputs):
        assert all(x.ndim == 4 for x in inputs)
        return [F.pad(x, self._pad, mode="replicate") for x in inputs]

    def unpad(self, x):
        ht, wd = x.shape[-2:]
        return x[..., self._pad[2]:ht - self._pad[3], self._pad[0]:wd - self._pad[1]]

    def get_pad_num(self):
        return [self._pad[2], self._pad[3], self._pad[0], self._pad[1]]


def pad_for_multi_train(image1, image2, scale_test: float, divis_by: int = 32):
    """Down-scale by `scale_test` (bicubic), pad, and build the query coordinates of the WANTED
    full-resolution output inside the padded low-res frame.  Returns
    (image1_pad, image2_pad, hr_coord [H*W,2], scaled pad_num)  — evaluation.py:67-89."""
    assert scale_test > 0.99
    h_want, w_want = image1.shape[-2:]
    h_lr = int(math.ceil(h_want / float(scale_test)))
    w_lr = int(math.ceil(w_want / float(scale_test)))
    if scale_test > 1:
        image1 = F.interpolate(image1, (h_lr, w_lr), mode="bicubic", align_corners=False)
        image2 = F.interpolate(image2, (h_lr, w_lr), mode="bicubic", align_corners=False)
    padder = InputPadder(image1.shape, divis_by=divis_by)
    image1_pad, image2_pad = padder.pad(image1, image2)
    h_hr = int(image1_pad.shape[2] * scale_test)
    w_hr = int(image1_pad.shape[3] * scale_test)
    coord = make_coord([h_hr, w_hr], flatten=False)
    p = [int(i * scale_test) for i in padder.get_pad_num()]
    coord = coord[p[0]:h_hr - p[1], p[2]:w_hr - p[3], :]
    if coord.shape[0] != h_want or coord.shape[1] != w_want:
        coord = F.interpolate(coord.permute(2, 0, 1).unsqueeze(0), (h_want, w_want), mode="bilinear").squeeze(0).permute(1, 2, 0)
    return image1_pad, image2_pad, coord.contiguous().view(h_want * w_want, -1), p


def pad_for_multi_train_fixed(image1, image2, scale: int, divis_by: int = 16):
    """Fixed integer up-scaling of the given low-res pair (evaluation_validate.py:92-106)."""
    h_want, w_want = image1.shape[-2] * scale, image1.shape[-1] * scale
    padder = InputPadder(image1.shape, divis_by=divis_by)
    image1_pad, image2_pad = padder.pad(image1, image2)
    h_hr, w_hr = image1_pad.shape[2] * scale, image1_pad.shape[3] * scale
    coord = make_coord([h_hr, w_hr], flatten=False)
    p = [round(i * scale) for i in padder.get_pad_num()]
    coord = coord[p[0]:h_hr - p[1], p[2]:w_hr - p[3], :]
    assert coord.shape[0] == h_want and coord.shape[1] == w_want
    return image1_pad, image2_pad, coord.contiguous().view(h_want * w_want, -1), p


# ------------------------------------------------------------------------------------------------
# the same protocol on the device: geometry stated once, the two kernels of csrc/prepare.hip and their plain-torch restatements
# ------------------------------------------------------------------------------------------------

class QueryPlan(NamedTuple):
    """Every size of pad_for_multi_train / pad_for_multi_train_fixed for an h x w input; pads are (top, bottom, left, right)."""
    h: int
    w: int
    scale: float
    h_lr: int
    w_lr: int
    pad: Tuple[int, int, int, int]   # of the low-res frame
    h_pad: int
    w_pad: int
    h_hr: int
    w_hr: int
    p: Tuple[int, int, int, int]     # the padding scaled to the high-res grid
    h_crop: int
    w_crop: int
    h_want: int
    w_want: int
    resized: bool                    # crop shape != wanted shape: the coordinates are resized (bilinear)


def query_plan(h: int, w: int, scale_test, divis_by: int, fixed: bool = False) -> QueryPlan:
    """The integer / float arithmetic of pad_for_multi_train (ceil(h / scale), int(h_pad * scale), int(pad * scale)) or, with
    `fixed`, of pad_for_multi_train_fixed (no down-scaling, h_pad * scale, round(pad * scale)) — no tensor is touched."""
    h, w = int(h), int(w)
    if fixed:
        if float(scale_test) != int(scale_test) or int(scale_test) < 1:
            raise RuntimeError(f"query_plan: the fixed protocol up-scales by a positive integer, got scale {scale_test}")
        scale_test = int(scale_test)
        h_lr, w_lr = h, w
        h_want, w_want = h * scale_test, w * scale_test
    else:
        assert scale_test > 0.99
        h_want, w_want = h, w
        if scale_test > 1:
            h_lr, w_lr = int(math.ceil(h / float(scale_test))), int(math.ceil(w / float(scale_test)))
        else:
            h_lr, w_lr = h, w
    padder = InputPadder((h_lr, w_lr), divis_by=divis_by)
    pad = tuple(padder.get_pad_num())
    h_pad, w_pad = h_lr + pad[0] + pad[1], w_lr + pad[2] + pad[3]
    if fixed:
        h_hr, w_hr = h_pad * scale_test, w_pad * scale_test
        p = tuple(round(i * scale_test) for i in pad)
    else:
        h_hr, w_hr = int(h_pad * scale_test), int(w_pad * scale_test)
        p = tuple(int(i * scale_test) for i in pad)
    h_crop, w_crop = h_hr - p[0] - p[1], w_hr - p[2] - p[3]
    if fixed:
        assert h_crop == h_want and w_crop == w_want
    return QueryPlan(h, w, scale_test, h_lr, w_lr, pad, h_pad, w_pad, h_hr, w_hr, p, h_crop, w_crop, h_want, w_want,
                     (h_crop, w_crop) != (h_want, w_want))


def _coord_table(n_hr: int, lo: int, n_crop: int, n_want: int, resized: bool, device) -> torch.Tensor:
    """One axis of the query grid: make_coord's sequence of the high-res frame, cropped and — when the grid is resized — resized
    1-D as ATen's bilinear (align_corners=False) does.  Every operation is an fp32 torch op of its own (no FMA)."""
    r = 2 / (2 * n_hr)
    v = ((-1 + r) + (2 * r) * torch.arange(n_hr, device=device).float())[lo:lo + n_crop]
    if not resized:
        assert n_crop == n_want
        return v
    scale = float((torch.tensor(float(n_crop), dtype=torch.float32) / torch.tensor(float(n_want), dtype=torch.float32)))
    src = (scale * (torch.arange(n_want, device=device).float() + 0.5) - 0.5).clamp(min=0)
    i0 = src.floor().long().clamp(max=n_crop - 1)
    i1 = (i0 + 1).clamp(max=n_crop - 1)
    l1 = src - i0.float()
    l0 = 1 - l1
    return l0 * v[i0] + l1 * v[i1]


def query_grid_host(plan: QueryPlan, batch: int, device=None) -> torch.Tensor:
    """hr_coord [batch, h_want * w_want, 2] as `as_query_grid` forms it, in plain torch on any device (the kernel's arithmetic)."""
    rows = _coord_table(plan.h_hr, plan.p[0], plan.h_crop, plan.h_want, plan.resized, device)
    cols = _coord_table(plan.w_hr, plan.p[2], plan.w_crop, plan.w_want, plan.resized, device)
    grid = torch.stack((rows.view(-1, 1).expand(plan.h_want, plan.w_want), cols.view(1, -1).expand(plan.h_want, plan.w_want)), dim=-1)
    return grid.reshape(1, plan.h_want * plan.w_want, 2).expand(batch, -1, -1).contiguous()


_CUBIC_A = -0.75


def _cubic1(x):
    return ((_CUBIC_A + 2) * x - (_CUBIC_A + 3)) * x * x + 1


def _cubic2(x):
    return ((_CUBIC_A * x - 5 * _CUBIC_A) * x + 8 * _CUBIC_A) * x - 4 * _CUBIC_A


def _cubic_axis(n_in: int, n_lr: int, n_pad: int, pad_lo: int, device):
    """Tap indices [4, n_pad] and weights [4, n_pad] of one axis of the padded frame (upsample_bicubic2d, align_corners=False)."""
    dst = (torch.arange(n_pad, device=device) - pad_lo).clamp(0, n_lr - 1).float()
    scale = float(torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_lr), dtype=torch.float32))
    src = scale * (dst + 0.5) - 0.5
    fl = src.floor()
    t = src - fl
    i = fl.long()
    idx = torch.stack([(i - 1 + k).clamp(0, n_in - 1) for k in range(4)])
    wgt = torch.stack([_cubic2(t + 1), _cubic1(t), _cubic1(1 - t), _cubic2(2 - t)])
    return idx, wgt


def bicubic_pad_host(image: torch.Tensor, plan: QueryPlan) -> torch.Tensor:
    """One image [B,3,H,W] (uint8 or float) -> fp32 [B,3,h_pad,w_pad] as `as_prepare_pair` forms it, in plain torch on any device:
    four horizontal 4-tap sums, then the vertical one, the padded pixel being the resized pixel at the clamped index."""
    x = image.float()
    assert x.dim() == 4 and tuple(x.shape[-2:]) == (plan.h, plan.w)
    dev = x.device
    if (plan.h_lr, plan.w_lr) == (plan.h, plan.w):
        iy = (torch.arange(plan.h_pad, device=dev) - plan.pad[0]).clamp(0, plan.h - 1)
        ix = (torch.arange(plan.w_pad, device=dev) - plan.pad[2]).clamp(0, plan.w - 1)
        return x[:, :, iy][:, :, :, ix].contiguous()
    iy, wy = _cubic_axis(plan.h, plan.h_lr, plan.h_pad, plan.pad[0], dev)
    ix, wx = _cubic_axis(plan.w, plan.w_lr, plan.w_pad, plan.pad[2], dev)
    out = None
    for a in range(4):
        rows = x[:, :, iy[a]]                                    # [B,3,h_pad,W]
        acc = None
        for b in range(4):
            term = rows[:, :, :, ix[b]] * wx[b].view(1, 1, 1, -1)
            acc = term if acc is None else acc + term
        term = acc * wy[a].view(1, 1, -1, 1)
        out = term if out is None else out + term
    return out.contiguous()


def resize_disparity_host(src: torch.Tensor, crop, size, mul: float = 1.0) -> torch.Tensor:
    """fp32 [N,Hs,Ws] (or [N,1,Hs,Ws]) -> fp32 [N,H,W] as `as_resize_disp` forms it, in plain torch on any device: the resize of the
    interpolation baseline (evaluation.py:125-146, `multi_evaothers`), F.interpolate(unpad(x) * scale, (H, W), mode='bicubic').
    crop = (top, left, hc, wc), size = (H, W).  Each tap is multiplied by `mul` first; the taps are clamped to the crop, never to
    the padded frame around it; a crop of the output's shape is copied (times mul)."""
    x = src.float()
    if x.dim() == 4 and x.shape[1] == 1:
        x = x[:, 0]
    top, left, hc, wc = (int(v) for v in crop)
    h, w = (int(v) for v in size)
    assert x.dim() == 3 and hc > 0 and wc > 0 and top >= 0 and left >= 0 and top + hc <= x.shape[1] and left + wc <= x.shape[2]
    x = x[:, top:top + hc, left:left + wc] * float(mul)
    if (hc, wc) == (h, w):
        return x.contiguous()
    iy, wy = _cubic_axis(hc, h, h, 0, x.device)
    ix, wx = _cubic_axis(wc, w, w, 0, x.device)
    out = None
    for a in range(4):
        rows = x[:, iy[a]]                                       # [N,H,wc]
        acc = None
        for b in range(4):
            term = rows[:, :, ix[b]] * wx[b].view(1, 1, -1)
            acc = term if acc is None else acc + term
        term = acc * wy[a].view(1, -1, 1)
        out = term if out is None else out + term
    return out.contiguous()


def prepare_on_device(image1, image2, scale_test, divis_by: int = 32, fixed: bool = False):
    """The device counterpart of pad_for_multi_train (fixed=False) / pad_for_multi_train_fixed (fixed=True): image1 / image2 [B,3,H,W]
    on the GPU, uint8 or float32 -> (image1_pad, image2_pad fp32 [B,3,h_pad,w_pad], hr_coord [B, Q, 2], p).  Two launches
    (`ops.prepare_pair`, `ops.query_grid`), no host tensor, no synchronisation."""
    from .. import ops
    if image1.dim() != 4:
        raise RuntimeError(f"prepare_on_device: image1 must be [B,3,H,W], got {tuple(image1.shape)}")
    plan = query_plan(image1.shape[-2], image1.shape[-1], scale_test, divis_by, fixed=fixed)
    i1, i2 = ops.prepare_pair(image1, image2, plan)
    coord = ops.query_grid(plan, image1.shape[0], image1.device)
    return i1, i2, coord, list(plan.p)
