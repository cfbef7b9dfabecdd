"""Regenerates tests/golden/train_batch.npz from the reference's own StereoDataset.__getitem__ (needs the reference checkout):

    python tests/golden/make_golden_train_batch.py

models/coreContinuous_IGEV/stereo_datasets.py is imported as it is; what it imports and this machine lacks (cv2, torchvision, skimage,
imageio) is replaced by empty stand-in modules — none of them is used between the augmentor and the return of __getitem__ except
cv2.resize for flow_low_res, whose stand-in returns zeros (that output of the reference is NOT recorded).  A StereoDataset without
augmentor (aug_params=None) is given one ground-truth crop through its `disparity_reader`, so lines 148-212 run unchanged on it:
to_pixel_samples / make_coord and the branch that (sparse, without_mutli_scale) select.  np.random.choice is wrapped: the drawn index
lists are recorded, in call order.

Per case k (CASES below; mode, h_lr x w_lr -> Q = h_lr * w_lr, scale, the crop's recipe):
    c{k}_crop     fp32 [h_hr, w_hr]   the ground-truth crop (h_hr = round(h_lr * scale), as stereo_datasets.py:122-123)
    c{k}_draw     int64 [k]           what np.random.choice returned (absent when the branch draws nothing)
    c{k}_coord    fp32 [Q', 2]        the reference's hr_coord  (absent when the reference raised)
    c{k}_flow     fp32 [1, Q']        the reference's hr_flow
    c{k}_low      fp32 [h_lr//4, w_lr//4]  NOT the reference (cv2 is missing): F.interpolate(crop, mode="bilinear",
                                      align_corners=False) / float32(4 * scale) by torch on the CPU; finite crops only
    c{k}_meta     fp64 [6]            mode id (0 dense, 1 dense_all, 2 sparse, 3 sparse_ordered), h_lr, w_lr, scale, V = #(crop > 0),
                                      1 when the reference raised "sample_q is too small" (sparse_ordered with V > Q)
The file is written with fixed zip timestamps: a second run gives the same bytes.
"""
from __future__ import annotations

import io
import os
import sys
import types
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402

MODES = {"dense": 0, "dense_all": 1, "sparse": 2, "sparse_ordered": 3}
# (mode, h_lr, w_lr, scale, number of valid pixels V or None for an all-positive dense crop, inf / NaN planted)
CASES = [
    ("dense", 8, 12, 1.375, None, False),          # 11 x 16
    ("dense", 8, 12, 2.95, None, True),            # 24 x 35, inf and NaN
    ("dense", 8, 12, 1.0, None, False),            # N == Q: every pixel once
    ("dense_all", 8, 12, 1.0, None, False),
    ("dense_all", 6, 11, 1.0, None, True),
    ("sparse", 8, 12, 1.375, 0, False),            # V = 0
    ("sparse", 8, 12, 1.375, 40, False),           # V < Q
    ("sparse", 8, 12, 1.375, 96, False),           # V == Q
    ("sparse", 8, 12, 1.375, 130, False),          # V > Q
    ("sparse", 8, 12, 1.375, 176, False),          # V == N
    ("sparse", 8, 12, 1.375, 50, True),            # inf (valid), -inf and NaN (invalid)
    ("sparse_ordered", 8, 12, 1.375, 0, False),
    ("sparse_ordered", 8, 12, 1.375, 40, False),
    ("sparse_ordered", 8, 12, 1.375, 96, False),
    ("sparse_ordered", 8, 12, 1.375, 130, False),  # the reference asserts
    ("sparse_ordered", 8, 12, 1.0, 96, False),     # V == N == Q
    ("sparse_ordered", 8, 12, 1.375, 50, True),
]


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


def import_stereo_datasets():
    import importlib
    for name in ("cv2", "torchvision", "torchvision.transforms", "skimage", "imageio"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = _Stub(name)
    sys.path.insert(0, REF)
    pkg = types.ModuleType("models")
    pkg.__path__ = [REF + "/models"]
    sys.modules["models"] = pkg
    import models.coreContinuous_IGEV.stereo_datasets as sd
    return sd


def make_crop(k, h, w, v, nonfinite):
    """A crop with exactly `v` values > 0 (None: all positive), at seeded positions."""
    g = torch.Generator().manual_seed(7100 + k)
    n = h * w
    crop = torch.rand(n, generator=g) * 60 + 0.5
    if v is not None:
        order = torch.randperm(n, generator=g)
        bad = order[v:]
        crop[bad] = -torch.rand(bad.numel(), generator=g) * 3      # invalid: negative ...
        crop[bad[::3]] = 0.0                                       # ... or exactly zero
        if nonfinite:
            crop[order[0]] = float("inf")                          # valid
            crop[bad[1]] = float("-inf")
            crop[bad[2]] = float("nan")
    elif nonfinite:
        crop[3], crop[n // 2], crop[n - 2] = float("inf"), float("nan"), float("-inf")
    return crop.view(h, w).contiguous()


def run_reference(sd, mode, h_lr, w_lr, scale, crop):
    """One __getitem__ of the reference on `crop` -> (hr_coord, hr_flow, draws, raised)."""
    sparse, single = mode.startswith("sparse"), mode in ("dense_all", "sparse_ordered")
    ds = sd.StereoDataset(aug_params=None, sparse=sparse, reader=lambda path: crop.numpy().copy(), multi_training=True,
                          scale_min=scale, scale_max=scale, inp_size=[h_lr, w_lr], without_mutli_scale=single)
    ds.image_list, ds.disparity_list = [["left", "right"]], ["disp"]
    sd.frame_utils.read_gen = lambda path: np.zeros((h_lr, w_lr, 3), dtype=np.uint8)
    sd.cv2.resize = lambda flow, dsize, interpolation=None: np.zeros((dsize[1], dsize[0]), dtype=np.float32)
    draws = []
    choice = np.random.choice

    def recording_choice(a, size=None, replace=True, p=None):
        out = choice(a, size, replace=replace, p=p)
        draws.append(np.asarray(out, dtype=np.int64).copy())
        return out

    np.random.choice = recording_choice
    try:
        out = ds[0]
    except AssertionError as e:
        assert "sample_q is too small" in str(e)
        return None, None, draws, True
    finally:
        np.random.choice = choice
    return out[3], out[4], draws, False


def main():
    torch.set_num_threads(1)
    sd = import_stereo_datasets()
    arrs = {}
    for k, (mode, h_lr, w_lr, scale, v, nonfinite) in enumerate(CASES):
        h, w = round(h_lr * scale), round(w_lr * scale)
        crop = make_crop(k, h, w, v, nonfinite)
        n_valid = int((crop > 0).sum())
        assert v is None or n_valid == v, (k, n_valid, v)
        np.random.seed(9000 + k)
        coord, flow, draws, raised = run_reference(sd, mode, h_lr, w_lr, scale, crop)
        assert len(draws) <= 1
        arrs[f"c{k}_crop"] = crop
        arrs[f"c{k}_meta"] = np.asarray([MODES[mode], h_lr, w_lr, scale, n_valid, float(raised)], dtype=np.float64)
        if draws:
            arrs[f"c{k}_draw"] = draws[0]
        if not raised:
            assert coord.dtype == torch.float32 and flow.dtype == torch.float32 and coord.shape[0] == flow.shape[1]
            arrs[f"c{k}_coord"], arrs[f"c{k}_flow"] = coord, flow
        if bool(torch.isfinite(crop).all()):
            low = F.interpolate(crop[None, None], (h_lr // 4, w_lr // 4), mode="bilinear", align_corners=False)[0, 0]
            arrs[f"c{k}_low"] = low / torch.tensor(4.0 * scale, dtype=torch.float32)
        print(f"case {k} {mode} {h}x{w} Q={h_lr * w_lr} V={n_valid}: draws {[len(d) for d in draws]}, "
              f"{'raised' if raised else tuple(coord.shape)}")

    path = os.path.join(HERE, "train_batch.npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrs):
            a = arrs[name]
            a = np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a)
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))  # fixed: the file regenerates bit for bit
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)
    print(f"wrote train_batch.npz ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
