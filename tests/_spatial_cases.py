"""Shared by tests/test_spatial_cpu.py and tests/test_spatial_gpu.py: the committed fixture tests/golden/spatial.npz (written by
tests/golden/make_golden_spatial.py from the reference's own augmentor classes) as calls of `spatial_pair`, and seeded inputs.  A helper
module, not a test file; nothing here reads the reference."""
import os

import numpy as np
import torch

from anystereo.harness import spatial as SP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial.npz")
_CACHE = {}


def fixture_cases():
    """[(name, image1, image2 uint8 [1,3,H,W], disp fp32 [1,H,W], valid uint8 [1,H,W] | None, [SpatialParams], out_size | None,
    want)] with want = dict(st1, st2 uint8 [3,ch,cw]; disp fp32 [ch,cw]; valid uint8 [ch,cw] | None; out1, out2 uint8 [3,oh,ow] | None)."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    z = np.load(GOLDEN)
    chw = lambda a: torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1))))  # noqa: E731
    im1, im2 = chw(z["img1"]).unsqueeze(0), chw(z["img2"]).unsqueeze(0)
    disp = torch.from_numpy(np.ascontiguousarray(z["flow"][..., 0])).unsqueeze(0)
    assert not z["flow"][..., 1].any()
    valid = torch.from_numpy(z["valid"]).unsqueeze(0)
    cases, k = [], 0
    while f"c{k}_par" in z.files:
        cls, rescale, fx, fy, flip, y0, x0, ch, cw, dy2, oh, ow = z[f"c{k}_par"].tolist()
        p = SP.SpatialParams(bool(rescale), fx, fy, SP.FLIPS[int(flip)], int(y0), int(x0), int(ch), int(cw), int(dy2))
        sparse = int(cls) >= 2
        flow = z[f"c{k}_stflow"]
        assert not flow[..., 1].any()                                  # the y component: zero (or -0.0) throughout
        want = {"st1": chw(z[f"c{k}_st1"]), "st2": chw(z[f"c{k}_st2"]),
                "disp": torch.from_numpy(np.ascontiguousarray(flow[..., 0].astype(np.float32))),   # the dataset's .float()
                "valid": None, "out1": None, "out2": None}
        if sparse:
            v = z[f"c{k}_stvalid"]
            assert v.min() >= 0 and v.max() <= 1
            want["valid"] = torch.from_numpy(np.ascontiguousarray(v.astype(np.uint8)))
        if oh:
            want["out1"], want["out2"] = chw(z[f"c{k}_out1"]), chw(z[f"c{k}_out2"])
        cases.append((f"case{k}-cls{int(cls)}-{p.flip}", im1, im2, disp, valid if sparse else None, [p], (int(oh), int(ow)) if oh else None, want))
        k += 1
    assert k >= 16
    _CACHE["cases"] = cases
    return cases


def bits(t: torch.Tensor) -> torch.Tensor:
    """fp32 compared bit for bit (-0.0 is not 0.0, a NaN equals itself)."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def random_frames(batch: int, h: int, w: int, seed: int, sparse: bool = False):
    g = torch.Generator().manual_seed(seed)
    im1 = torch.randint(0, 256, (batch, 3, h, w), generator=g, dtype=torch.uint8)
    im2 = torch.randint(0, 256, (batch, 3, h, w), generator=g, dtype=torch.uint8)
    disp = torch.rand((batch, h, w), generator=g) * 90 + 0.25
    valid = None
    if sparse:
        valid = (torch.rand((batch, h, w), generator=g) < 0.4).to(torch.uint8)
        valid[:, 0, ::2], valid[:, ::3, 0] = 1, 1
    return im1, im2, disp, valid


def hashed_params(batch: int, h: int, w: int, crop_sizes, sparse: bool, seed: int = 3):
    """`draw_spatial` with every flip mode in turn (the spec's `do_flip` is one mode per spec, so one draw per sample; the flip is
    taken with probability 1 here, so that every mode does occur)."""
    import dataclasses
    out = []
    for b in range(batch):
        flip = (False, "hf", "h", "v")[b % 4]
        spec = SP.SpatialSpec.sparse(do_flip=flip, wo_crop=b % 2 == 1) if sparse else SP.SpatialSpec.flow(do_flip=flip, yjitter=b % 3 != 2)
        spec = dataclasses.replace(spec, h_flip_prob=1.0, v_flip_prob=1.0)
        out += SP.draw_spatial(spec, seed, 100 + b, 1, h, w, [crop_sizes[b]])
    return out
