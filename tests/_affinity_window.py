"""Shared by tests/test_liif_windows_{cpu,gpu}.py: the float64 restatement of AffinityFeature for a win x win window
(liif.py:432-446: normalise, Unfold with padding win // 2, drop the centre, dot, clamp at 0) and the upsampler builder of the
liif_windows fixture (tests/golden/make_golden_windows.py)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
META = json.load(open(os.path.join(GOLD, "liif_windows.json")))


def gold(name="liif_windows"):
    return np.load(os.path.join(GOLD, name + ".npz"))


def affinity_dots(x, win):
    """-> (dots [B,n,H,W] float64 before the clamp, inmap [n,H,W] bool: the neighbour lies inside the map)."""
    x = x.double()
    b, c, h, w = x.shape
    r, mid = win // 2, (win * win) // 2
    xh = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    u = F.unfold(xh, win, padding=r).reshape(b, c, win * win, h, w)
    nb = torch.cat([u[:, :, :mid], u[:, :, mid + 1:]], dim=2)
    ones = F.unfold(torch.ones(1, 1, h, w, dtype=torch.float64), win, padding=r).reshape(win * win, h, w)
    inmap = torch.cat([ones[:mid], ones[mid + 1:]], dim=0) > 0
    return (nb * xh.unsqueeze(2)).sum(dim=1), inmap


def affinity_ref(x, win, with_x=False):
    aff = affinity_dots(x, win)[0].clamp_min(0)
    return torch.cat([x.double(), aff], dim=1) if with_x else aff


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.isfinite(a).all(), f"{what}: non-finite values"
    err = (a - b).abs().max().item()
    lim = atol + rtol * b.abs().max().item()
    print(f"{what}: max abs err {err:.3e} (limit {lim:.3e})")
    assert err <= lim, f"{what}: max abs err {err:.3e} > {lim:.3e}"


def fixture_inputs(device="cpu", batch=1):
    from anystereo.harness.synthetic import det_uniform
    return [det_uniform((batch, 176, 4, 6), 81).to(device), det_uniform((batch, 32, 8, 12), 82).to(device)], [176, 32]


def build_upsampler(win_h, win_w, mode, device="cpu"):
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.nn import liif as NL
    _, chans = fixture_inputs()
    aff = {"win_w": win_w, "win_h": win_h, "dilation": [1, 2, 4, 8]}
    up = NL.liif_out_multi_scale_Training(encoder_dim=sum(chans), mlphidden_list=[128, 64, 64], pos_dim=0, affinity_settings=aff,
                                          number_input=2, chanels=chans, unfold=mode).eval()
    fill_module_deterministic(up, base_seed=7, gain=2.0)
    return up.to(device)
