"""CPU (-m "not gpu"): host-side logic — the C-ABI library loads and exports every declared symbol,
the model mirror has the reference's state_dict, the plain-C oracle agrees with the PyTorch oracle,
and the product path refuses to run without the GPU (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_library_exports_every_declared_symbol():
    from anystereo import _lib
    hdr = open(os.path.join(ROOT, "include", "anystereo_hip.h")).read()
    declared = set(re.findall(r"\b(as_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("as_conv_desc")
    assert len(declared) >= 20
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/anystereo_hip.h but not exported"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    bound = _lib.load()
    assert bound.as_abi_version() == 38
    assert bound.as_last_error_string() is not None


def test_conv_desc_layout_matches_header():
    """ctypes mirror of as_conv_desc: field order/count as in the header."""
    from anystereo import _lib
    hdr = open(os.path.join(ROOT, "include", "anystereo_hip.h")).read()
    body = hdr[hdr.index("typedef struct {"):hdr.index("} as_conv_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            m = re.search(r"([A-Za-z_0-9]+)\s*(\[[A-Z_]+\])?\s*$", part.strip())
            names.append(m.group(1))
    assert names == [f[0] for f in _lib.ConvDesc._fields_]


def test_argument_validation_without_gpu():
    """Host-side shape checks run before any launch, so they are testable on a CPU-only box."""
    from anystereo import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    assert lib.as_corr_sampler_fwd(None, one, one, 1, 1, 1, 1, 4, 2, 0, None) == -1
    assert b"null" in lib.as_last_error_string()
    assert lib.as_corr_sampler_fwd(one, one, one, 1, 1, 1, 1, 4, 3, 0, None) == -1
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 97, 2, 2, 48, 8, None) == -2
    assert lib.as_conv_pack_size(162, 64, 1) == 6 * 1 * 32 * 64
    assert lib.as_conv_pack_size(384, 256, 3) == 48 * 9 * 8 * 256
    assert lib.as_conv_pack_size(8, 8, 5) == -1
    # round-6 entry points: argument checks come before any launch
    assert lib.as_stamp(None, 0, None) == -1 and lib.as_stamp(one, -1, None) == -1
    assert lib.as_liif_query_rows(None, 1, 8, one, None) == -1 and lib.as_liif_query_rows(one, 1, 0, one, None) == -1
    assert lib.as_ir_block_pack_bytes(16, 96, 24) == (3 * 1 * 2 + 3 * 1 * 2 * 2) * 64 * 8 * 2
    assert lib.as_ir_block_pack_bytes(24, 144, 24) == (5 * 2 * 2 + 5 * 1 * 2 * 2) * 64 * 8 * 2   # 144 -> 160 expanded channels, Cin 24 -> 32
    assert lib.as_ir_block_pack_bytes(0, 96, 24) == -1
    assert lib.as_ir_block(None, one, one, one, 1, 16, 96, 24, 8, 8, 1, 0, None) == -1
    assert lib.as_ir_block(one, one, one, one, 1, 16, 96, 24, 8, 8, 3, 0, None) == -1          # stride
    assert lib.as_ir_block(one, one, one, one, 1, 16, 96, 24, 8, 8, 1, 1, None) == -1          # residual needs Cin == Cout
    assert lib.as_ir_block(one, one, one, one, 1, 16, 96, 200, 8, 8, 1, 0, None) == -2         # Cout <= 160
    d = _lib.ConvDesc()
    assert lib.as_conv2d(ctypes.byref(d), None) == -1


def test_product_path_has_no_cpu_fallback():
    from anystereo import ops
    from anystereo.models import __models__, default_args
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.geo_corr_lookup(None, [torch.zeros(1, 2, 8, 8)], torch.zeros(1, 1, 2, 8), 4)
    model = __models__["continuous_RAFTStereo"](default_args("continuous_RAFTStereo")).eval()
    from anystereo.harness.synthetic import synthetic_pair
    i1, i2 = synthetic_pair(1, 32, 64)
    with torch.no_grad(), pytest.raises(RuntimeError):
        model(i1, i2, iters=1, test_mode=True, hr_coord=torch.zeros(1, 4, 2), scale=torch.ones(1, 1))


def test_training_resamplers_have_no_library_fallback():
    """Row a8 in training (pool2x / interp, update.py:94-102): a tensor the HIP path does not take is an ERROR, not a silent
    ATen call (round-5 review item 8) — CPU tensors and integer dtypes are refused before any launch."""
    from anystereo.nn import update as U
    x = torch.randn(1, 8, 6, 10, requires_grad=True)
    with pytest.raises(RuntimeError, match="CUDA"):
        U.pool2x(x)
    with pytest.raises(RuntimeError, match="CUDA"):
        U.interp(x, torch.empty(1, 1, 12, 20))
    src = open(os.path.join(ROOT, "any-stereo_amd", "anystereo", "nn", "update.py")).read()
    body = src[src.index("def pool2x(x):"):src.index("class BasicMultiUpdateBlock")]
    assert "F.avg_pool2d(" not in body and "F.interpolate(" not in body


def test_state_dict_matches_reference(golden):
    """Parameter names and shapes are the reference's (captured by make_golden.py)."""
    import json
    from anystereo.models import __models__, default_args
    path = os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")
    ref = json.load(open(path))
    for key in ("continuous_IGEVStereo", "continuous_RAFTStereo"):
        sd = __models__[key](default_args(key)).state_dict()
        mine = {k: list(v.shape) for k, v in sd.items()}
        assert mine == ref[key], (set(mine) ^ set(ref[key]))
    # checkpoints saved through nn.DataParallel carry a `module.` prefix (train_continuous_IGEV.py:184,243)
    from anystereo.harness.checkpoint import load_reference_state_dict
    m = __models__["continuous_RAFTStereo"](default_args("continuous_RAFTStereo"))
    load_reference_state_dict(m, {"module." + k: v for k, v in m.state_dict().items()})


def test_c_oracle_matches_python_oracle():
    import numpy as np
    from oracle import ops as O
    so = os.path.join(ROOT, "oracle", "_build", "libcorr_sampler_ref.so")
    if not os.path.exists(so):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True)
    lib = ctypes.CDLL(so)
    g = torch.Generator().manual_seed(3)
    n, h1, w1, w2, r = 2, 3, 17, 11, 4
    vol = torch.randn(n, h1, w1, w2, generator=g)
    coords = torch.stack([torch.rand(n, h1, w1, generator=g) * (w2 + 10) - 5, torch.zeros(n, h1, w1)], 1).contiguous()
    out = np.zeros((n, 2 * r + 1, h1, w1), np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.ref_corr_sampler_forward_f32(vol.numpy().ctypes.data_as(fp), coords.numpy().ctypes.data_as(fp),
                                     out.ctypes.data_as(fp), n, h1, w1, w2, r)
    assert np.abs(out - O.corr_sampler_forward(vol, coords, r).numpy()).max() < 1e-6
    gr = torch.randn(n, 2 * r + 1, h1, w1, generator=g)
    vg = np.zeros((n, h1, w1, w2), np.float32)
    lib.ref_corr_sampler_backward_f32(coords.numpy().ctypes.data_as(fp), gr.numpy().ctypes.data_as(fp),
                                      vg.ctypes.data_as(fp), n, h1, w1, w2, r)
    assert np.abs(vg - O.corr_sampler_backward(vol, coords, gr, r).numpy()).max() < 1e-6


def test_library_carries_its_source_hash(monkeypatch):
    """build.py compiles the hash of the native sources into the library; the binding refuses a library built from other sources
    (the .so is git-ignored but travels with the snapshot: a stale binary must not run silently on the GPU box)."""
    from anystereo import _lib, _srchash
    info = _lib.library_info()
    assert info["matches_sources"] is True and len(info["src_hash"]) == 16 and info["abi"] == _lib.load().as_abi_version()
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_srchash, "source_hash", lambda key: "0" * 16)
    with pytest.raises(RuntimeError, match="built from other sources"):
        _lib.load()
    monkeypatch.setenv("ANYSTEREO_ALLOW_STALE_LIB", "1")
    _lib.load()


def test_c_oracle_under_sanitizers():
    """The plain-C oracle of sampler_kernel.cu under AddressSanitizer + UBSan on its edge cases (windows outside the row, W2 = 1,
    radius > row, huge coordinates) — GPU sanitizers are unavailable on the pool, the CPU build is what can be checked."""
    import subprocess
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "asan"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(ROOT, "oracle", "_build", "corr_sampler_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sanitizer run clean" in r.stdout


def test_query_grid_harness(golden):
    """§8(f1): pad_for_multi_train semantics (evaluation.py:67-89) pinned by reference outputs."""
    import json
    from anystereo.harness.query import pad_for_multi_train
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "query_grid.json")))
    for case in ref:
        img = torch.zeros(1, 3, case["H"], case["W"])
        i1, i2, coord, pads = pad_for_multi_train(img, img, case["scale"], divis_by=case["divis_by"])
        assert list(i1.shape[-2:]) == case["padded"], case
        assert pads == case["pad_num"]
        assert list(coord.shape) == case["coord_shape"]
        got = [coord[0].tolist(), coord[-1].tolist(), float(coord.double().sum())]
        assert abs(got[2] - case["coord_sum"]) < 1e-3 * max(1.0, abs(case["coord_sum"]))
        assert max(abs(a - b) for a, b in zip(got[0] + got[1], case["first"] + case["last"])) < 1e-6


def test_loss_and_metrics_match_reference(golden):
    """§8(f2)/(f3): sequence_loss_multiscale and EPE/D1/Thres against values captured from the reference
    (tests/golden/make_golden.py, loss_metrics.npz)."""
    from anystereo.harness import metrics as M
    g = golden("loss_metrics")
    gt, valid = g["gt"], g["valid"]
    preds = [g[f"pred{i}"] for i in range(5)]
    loss, met = M.sequence_loss_multiscale(preds, gt, valid, max_disp=700)
    assert abs(loss.item() - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    for k, gk in (("epe", "epe_m"), ("1px", "px1"), ("3px", "px3")):
        assert abs(met[k] - float(g[gk])) <= 1e-6
    # the synchronisation-free form (masked sums over the stacked predictions) against the same reference numbers, and its gradient
    # against the reference statement's
    loss2, met2 = M.sequence_loss_multiscale(preds, gt, valid, max_disp=700, sync_free=True)
    assert abs(loss2.item() - float(g["loss"])) <= 2e-6 * abs(float(g["loss"]))
    for k, gk in (("epe", "epe_m"), ("1px", "px1"), ("3px", "px3")):
        assert abs(float(met2[k]) - float(g[gk])) <= 2e-6
    pa = [p.clone().requires_grad_(True) for p in preds]
    pb = [p.clone().requires_grad_(True) for p in preds]
    M.sequence_loss_multiscale(pa, gt, valid, max_disp=700)[0].backward()
    M.sequence_loss_multiscale(pb, gt, valid, max_disp=700, sync_free=True)[0].backward()
    for a, b in zip(pa, pb):
        assert (a.grad - b.grad).abs().max().item() <= 1e-7 * max(1e-30, a.grad.abs().max().item()) + 1e-12
    est, g3 = preds[-1][:, 0].reshape(2, 20, 25), gt[:, 0].reshape(2, 20, 25)
    m3 = (g3 > 0) & (g3 < 192)
    assert abs(M.epe_metric(est, g3, m3).item() - float(g["EPE"])) <= 1e-6
    assert abs(M.d1_metric(est, g3, m3).item() - float(g["D1"])) <= 1e-7
    assert abs(M.thres_metric(est, g3, m3, 2.0).item() - float(g["Thres2"])) <= 1e-7
    # single prediction: the reference would divide by zero (n-1); we keep gamma unadjusted instead of raising
    l1, _ = M.sequence_loss_multiscale(preds[-1:], gt, valid)
    assert torch.isfinite(l1)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_loss_ignores_nonfinite_ground_truth_at_invalid_pixels(bad):
    """Middlebury PFM ground truth holds inf at invalid pixels (frame_utils.readDispMiddlebury returns it raw,
    evaluation.py replaces isinf explicitly); the reference loss drops them by boolean indexing (train_continuous_IGEV.py:84-86).
    Both forms of the loss must give the same finite value, metrics and gradients as on sanitised ground truth."""
    from anystereo.harness import metrics as M
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(2, 1, 300, generator=g) * 100 + 1
    preds = [gt + torch.randn(2, 1, 300, generator=g) * (i + 1) for i in range(4)]
    gt_bad = gt.clone()
    gt_bad[0, 0, 7] = bad
    gt_bad[1, 0, 123] = bad
    valid_in = torch.ones_like(gt)
    valid_in[0, 0, 7] = 0
    valid_in[1, 0, 123] = 0
    gt_clean = gt.clone()
    gt_clean[0, 0, 7] = 0.0
    gt_clean[1, 0, 123] = 0.0
    want_p = [p.clone().requires_grad_(True) for p in preds]
    want, want_m = M.sequence_loss_multiscale(want_p, gt_clean, valid_in, max_disp=700)
    want.backward()
    for sync_free in (False, True):
        pp = [p.clone().requires_grad_(True) for p in preds]
        loss, met = M.sequence_loss_multiscale(pp, gt_bad, valid_in, max_disp=700, sync_free=sync_free)
        assert torch.isfinite(loss), (sync_free, loss)
        assert abs(loss.item() - want.item()) <= 2e-6 * abs(want.item())
        loss.backward()
        for a, b in zip(pp, want_p):
            assert torch.isfinite(a.grad).all(), sync_free
            assert (a.grad - b.grad).abs().max().item() <= 1e-7 * b.grad.abs().max().item() + 1e-12
        for k in ("epe", "1px", "3px"):
            assert abs(float(met[k]) - float(want_m[k])) <= 2e-6, (sync_free, k)


def test_fetch_optimizer_schedule():
    """AdamW + linear one-cycle: peak lr after 1 % of num_steps+100, linear decay afterwards
    (train_continuous_IGEV.py:125-134)."""
    from anystereo.harness.metrics import fetch_optimizer
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt, sched = fetch_optimizer(2e-4, 1e-5, 900, p)
    assert opt.defaults["eps"] == 1e-8 and opt.defaults["weight_decay"] == 1e-5
    lrs = []
    for _ in range(1000):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step(); sched.step()
    assert abs(max(lrs) - 2e-4) < 1e-12 and lrs.index(max(lrs)) == 9
    assert lrs[0] == pytest.approx(2e-4 / 25) and lrs[-1] < lrs[500] < lrs[100]
    assert fetch_optimizer(2e-4, 1e-5, 900, p, lr_fixed=True)[1] is None


def test_train_step_semantics():
    """Step ordering of train_continuous_IGEV.py:214-239 on a differentiable stand-in model: the gradient is clipped to
    norm 1 before AdamW sees it, and the schedule advances once per step."""
    from anystereo.harness.metrics import fetch_optimizer, train_step

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.tensor([3.0, -2.0]))

        def forward(self, image1, image2, iters=2, hr_coord=None, scale=None):
            base = (image1.mean() * self.w[0] + image2.mean() * self.w[1]) * 100.0
            preds = [base + hr_coord[..., :1].transpose(1, 2) * (i + 1) for i in range(iters)]
            return None, preds

    torch.manual_seed(0)
    m = Toy().train()
    opt, sched = fetch_optimizer(1e-2, 0.0, 50, m.parameters())
    b, q = 2, 40
    batch = (torch.rand(b, 3, 8, 8), torch.rand(b, 3, 8, 8), torch.rand(b, q, 2), torch.rand(b, 1, q) * 100 + 1, torch.ones(b, 1))
    w0, lr0 = m.w.detach().clone(), opt.param_groups[0]["lr"]
    loss, met = train_step(m, opt, sched, None, batch, train_iters=3, max_disp=192)
    assert torch.isfinite(loss) and set(met) == {"epe", "1px", "3px"}
    assert m.w.grad.norm().item() <= 1.0 + 1e-5, "gradient must be clipped to norm 1 before the step"
    assert not torch.equal(m.w.detach(), w0) and opt.param_groups[0]["lr"] != lr0
