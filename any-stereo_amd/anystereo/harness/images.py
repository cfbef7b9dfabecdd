"""The pictures the reference's validate_* loops produce (evaluation.py:187,196 and their repeats at :309,318 / :425,434 / :533,543):
the colourised disparity `Disp_to_color` written with torchvision's `save_image` as disp_{name}.png, and the KITTI error map of
`disp_error_image_func` (metrics_utils/visualization.py:30-55) — plus the KITTI 16-bit disparity PNG, the inverse of
`readDispKITTI` (frame_utils.py:124-127).

On the device the three pictures come out of ONE pass over the prediction (`ops.disparity_images`, csrc/eval_images.hip) as 8-bit
pixels; the copy to the host is asynchronous and the files are written after the caller's one synchronisation:

    sink = ImageSink("out/", max_disp=192.0, limit=20)
    res = evaluate(model, pairs, scale, iters, images=sink)      # res["images_written"]

The `*_host` functions state the same arithmetic with plain torch ops, one fp32 rounding per step in the reference's order: they
give the reference's fp32 bits (tests/golden/eval_images.npz), are what `ImageSink` runs on CPU tensors, and are what the tests
compare the kernel against.  `write_png` / `read_png` need `zlib` and `struct` only.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

COLOR_WEIGHTS = (114, 185, 114, 174, 114, 185, 114)                      # evaluation.py:41-48, the map's last column
COLOR_ROWS = ((0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 0, 1), (0, 1, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1))
ERROR_BANDS = ((49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144), (253, 174, 97),
               (244, 109, 67), (215, 48, 39), (165, 0, 38))             # visualization.py:12-22
ERROR_EDGES = (0.0, 0.0625, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, float("inf"))  # 0.1875 / 3 ... 48 / 3, exact in fp32
LEGEND_ROWS, LEGEND_STEP = 10, 20


def _f32(v, device):
    """A 0-dim fp32 tensor: dividing by it is a division on every backend (a Python scalar may become a product with 1 / v)."""
    return torch.tensor(v, dtype=torch.float32, device=device)


def _strip(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"{what} must be [B,H,W] or [B,1,H,W], got {tuple(t.shape)}")
    return t.float()


# ---- plain-torch restatements (any device; the CPU path) -------------------------------------------------------------------
@torch.no_grad()
def disp_to_color_host(disp: torch.Tensor, max_disp: float = 192.0) -> torch.Tensor:
    """Disp_to_color (evaluation.py:35-65) in closed form: disp [B,H,W] -> fp32 [B,H,W,3] in 0..1, the reference's bits.
    t = clamp(disp / max_disp, 0, 1); k = #{j : t > e_j}; u = (t - lo_k) * inv_k; v = A[k] * (1 - u) + A[k+1] * u."""
    disp = _strip(disp, "disp")
    dev = disp.device
    thousand = _f32(1000.0, dev)
    cum, acc = [], 0
    for w in COLOR_WEIGHTS:
        acc += w
        cum.append(acc)
    edges = torch.tensor(cum[:-1], dtype=torch.float32, device=dev) / thousand          # e_j
    lo = torch.cat([torch.zeros(1, device=dev), edges])
    inv = _f32(1.0, dev) / (torch.tensor(COLOR_WEIGHTS, dtype=torch.float32, device=dev) / thousand)
    rows = torch.tensor(COLOR_ROWS, dtype=torch.float32, device=dev)
    t = (disp / _f32(max_disp, dev)).clamp(0.0, 1.0)
    k = (t.unsqueeze(-1) > edges).sum(-1)
    u = (t - lo[k]) * inv[k]
    return rows[k] * (1.0 - u).unsqueeze(-1) + rows[k + 1] * u.unsqueeze(-1)


@torch.no_grad()
def error_image_host(est: torch.Tensor, gt: torch.Tensor, abs_thres: float = 3.0, rel_thres: float = 0.05) -> torch.Tensor:
    """disp_error_image_func.forward (visualization.py:30-55): est, gt [B,H,W] -> fp32 [B,H,W,3], the band colours as c / 255.
    r = min(E / abs_thres, (E / gt) / rel_thres) (a NaN on either side stays one); band i holds edge_i <= r < edge_{i+1}; gt <= 0
    and r in no band (NaN, +inf) are black; the legend overrides the top-left 10 x 200 pixels."""
    est, gt = _strip(est, "est"), _strip(gt, "gt")
    if est.shape != gt.shape:
        raise ValueError(f"error_image_host: est {tuple(est.shape)} does not match gt {tuple(gt.shape)}")
    dev = est.device
    cols = torch.tensor(ERROR_BANDS, dtype=torch.float32, device=dev) / _f32(255.0, dev)
    mask = gt > 0
    e = (gt - est).abs()
    r = torch.minimum(e / _f32(abs_thres, dev), (e / gt) / _f32(rel_thres, dev))
    img = torch.zeros(tuple(est.shape) + (3,), dtype=torch.float32, device=dev)
    for i in range(len(ERROR_BANDS)):
        img = torch.where((mask & (r >= ERROR_EDGES[i]) & (r < ERROR_EDGES[i + 1])).unsqueeze(-1), cols[i], img)
    for i in range(len(ERROR_BANDS)):
        img[:, :LEGEND_ROWS, i * LEGEND_STEP:(i + 1) * LEGEND_STEP] = cols[i]
    return img


@torch.no_grad()
def quantize_host(v: torch.Tensor) -> torch.Tensor:
    """torchvision.utils.save_image's cast: (uint8) clamp(v * 255 + 0.5, 0, 255), truncating; NaN -> 0 (undefined there)."""
    x = (v.float() * 255.0 + 0.5).clamp(0.0, 255.0)
    return torch.where(torch.isnan(x), torch.zeros_like(x), x).to(torch.uint8)


@torch.no_grad()
def encode16_host(disp: torch.Tensor) -> torch.Tensor:
    """disp [...] -> uint8 [...,2]: n = clamp(rint(disp * 256), 0, 65535) (ties to even, NaN -> 0), high byte first."""
    x = torch.round(disp.float() * 256.0)
    n = torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(0.0, 65535.0).to(torch.int32)
    return torch.stack([n >> 8, n & 255], dim=-1).to(torch.uint8)


def decode16(png: np.ndarray) -> np.ndarray:
    """readDispKITTI's arithmetic on a decoded [H,W,2] file: fp32 png / 256 (0 = invalid there)."""
    png = np.asarray(png)
    return ((png[..., 0].astype(np.uint16) << 8) | png[..., 1]).astype(np.float32) / np.float32(256.0)


# ---- PNG (zlib + struct) ----------------------------------------------------------------------------------------------------
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_FORMATS = {3: (2, 8), 2: (0, 16)}  # last dimension -> (colour type, bit depth): RGB8, 16-bit grey as (high, low) bytes


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path: str, array, level: int = 6) -> str:
    """uint8 [H,W,3] -> an 8-bit RGB PNG; uint8 [H,W,2] -> a 16-bit grey PNG whose samples are the byte pairs (high byte first, PNG's
    order, so the bytes pass through).  Filter 0 on every row, one IDAT chunk."""
    a = array.detach().cpu().numpy() if torch.is_tensor(array) else np.asarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in _FORMATS or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: uint8 [H,W,3] or [H,W,2] expected, got {a.dtype} {tuple(a.shape)}")
    h, w, c = a.shape
    ctype, depth = _FORMATS[c]
    rows = np.empty((h, 1 + w * c), dtype=np.uint8)
    rows[:, 0] = 0
    rows[:, 1:] = a.reshape(h, w * c)
    data = _SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) \
        + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(data)
    return path


def read_png(path: str) -> np.ndarray:
    """What `write_png` emits -> uint8 [H,W,3] or [H,W,2].  Every chunk's CRC is checked; anything write_png does not produce (other
    colour types, interlacing, row filters) raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _SIGNATURE:
        raise ValueError(f"read_png: {path} is not a PNG")
    pos, hdr, idat, ended = 8, None, [], False
    while pos < len(data) and not ended:
        if pos + 12 > len(data):
            raise ValueError(f"read_png: {path}: truncated chunk")
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if pos + 12 + n > len(data):
            raise ValueError(f"read_png: {path}: truncated chunk {kind!r}")
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + body) & 0xFFFFFFFF != crc:
            raise ValueError(f"read_png: {path}: CRC mismatch in chunk {kind!r}")
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if hdr is None or not ended:
        raise ValueError(f"read_png: {path}: missing IHDR or IEND")
    w, h, depth, ctype, comp, flt, interlace = hdr
    c = {(2, 8): 3, (0, 16): 2}.get((ctype, depth))
    if c is None or comp or flt or interlace:
        raise ValueError(f"read_png: {path}: colour type {ctype} depth {depth} interlace {interlace} is not what write_png emits")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if raw.size != h * (1 + w * c):
        raise ValueError(f"read_png: {path}: {raw.size} bytes of image data, {h * (1 + w * c)} expected")
    rows = raw.reshape(h, 1 + w * c)
    if rows[:, 0].any():
        raise ValueError(f"read_png: {path}: a filtered row (write_png emits filter 0 only)")
    return np.ascontiguousarray(rows[:, 1:]).reshape(h, w, c)


# ---- the sink ---------------------------------------------------------------------------------------------------------------
class ImageSink:
    """Collects the pictures of a dataset pass and writes them as PNG files into `directory`:
        disp_{name}.png    the colourised disparity (the reference's file name), `color`
        error_{name}.png   the error map against gt, `error` (only for images added with a gt)
        disp16_{name}.png  16-bit grey, disparity * 256, `enc16`
    `add` issues the kernel (device tensors) or the host restatement (CPU tensors), starts non-blocking copies into pinned host
    memory and returns without synchronising; `flush` — called after the caller's synchronisation — writes the files.  After
    `limit` images `add` takes no more.  The pinned copies of every image added since the last flush are held until then:
    17.7 MB per colour picture at Middlebury-F, so give a `limit` or flush in between on large datasets.  The pinned buffers are
    kept after a flush and reused by later batches of the same picture size, so a pass whose images share one size pays the
    pinned allocations of its first batches only (between flushes every batch needs buffers of its own)."""

    def __init__(self, directory: str, max_disp: float = 192.0, color: bool = True, error: bool = True, enc16: bool = False,
                 limit: Optional[int] = None):
        if not (color or error or enc16):
            raise ValueError("ImageSink: no picture requested")
        if limit is not None and limit < 0:
            raise ValueError(f"ImageSink: limit must be non-negative, got {limit}")
        self.directory, self.max_disp = directory, float(max_disp)
        self.color, self.error, self.enc16, self.limit = bool(color), bool(error), bool(enc16), limit
        self.taken = 0        # images accepted so far (the default names count these)
        self._pending = []    # (names, {"disp" | "error" | "disp16": host uint8 [b,H,W,c]}, event | None)
        self._free = {}       # shape -> pinned uint8 tensors whose files are written: reused instead of a new pinned allocation

    @torch.no_grad()
    def add(self, est: torch.Tensor, gt: Optional[torch.Tensor] = None, names: Optional[Sequence[str]] = None) -> int:
        """est [B,H,W] (or [B,1,H,W]), gt likewise or None, names: one per image (default: the running image index as %06d).
        Returns how many of the B images were taken."""
        est = _strip(est, "est").contiguous()
        gt = None if gt is None else _strip(gt, "gt").contiguous()
        if gt is not None and gt.shape != est.shape:
            raise ValueError(f"ImageSink.add: est {tuple(est.shape)} does not match gt {tuple(gt.shape)}")
        b = est.shape[0]
        if names is not None and len(names) != b:
            raise ValueError(f"ImageSink.add: {len(names)} names for {b} images")
        want_error = self.error and gt is not None
        if not (self.color or want_error or self.enc16):
            return 0  # an error-only sink and no gt: no file, so nothing counts against `limit` and no default name is used up
        take = b if self.limit is None else max(0, min(b, self.limit - self.taken))
        if take == 0:
            return 0
        est, gt = est[:take], (None if gt is None else gt[:take])
        names = [f"{self.taken + i:06d}" for i in range(take)] if names is None else [str(n) for n in names[:take]]
        event = None
        if est.is_cuda:
            from .. import ops
            c, e, n = ops.disparity_images(est, gt if want_error else None, self.max_disp, self.color, want_error, self.enc16)
            host = {}
            for key, t in (("disp", c), ("error", e), ("disp16", n)):
                if t is not None:
                    spare = self._free.get(tuple(t.shape))
                    host[key] = spare.pop() if spare else torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
                    host[key].copy_(t, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        else:
            host = {}
            if self.color:
                host["disp"] = quantize_host(disp_to_color_host(est, self.max_disp))
            if want_error:
                host["error"] = quantize_host(error_image_host(est, gt))
            if self.enc16:
                host["disp16"] = encode16_host(est)
        self._pending.append((names, host, event))
        self.taken += take
        return take

    def flush(self) -> List[str]:
        """Write the PNG files of everything added since the last flush and return their paths.  (Waits for the copies' events: free
        after the caller's synchronisation.)"""
        paths = []
        if self._pending:
            os.makedirs(self.directory, exist_ok=True)
        for names, host, event in self._pending:
            if event is not None:
                event.synchronize()
            for key, t in host.items():
                a = t.numpy()
                for i, name in enumerate(names):
                    paths.append(write_png(os.path.join(self.directory, f"{key}_{name}.png"), a[i]))
                if event is not None:
                    self._free.setdefault(tuple(t.shape), []).append(t)
        self._pending = []
        return paths
