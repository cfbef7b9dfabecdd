"""CPU: the evaluation harness (anystereo/harness/evaluate.py) against the reference's metrics_utils outputs
(tests/golden/eval_metrics.npz, written by tests/golden/make_golden_eval.py), its filter / guard rules, the image-mean
aggregation, the rank merge over gloo, and the argument checks of the two new C entries (no launch happens)."""
import ctypes
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = [(2, 24, 80), (1, 37, 131), (2, 64, 200)]
REGIONS = ("all", "noc", "occ")
METRICS = ("EPE", "D1", "Thres1", "Thres2", "Thres3")


@pytest.fixture(scope="module")
def fx(golden):
    return golden("eval_metrics")


def _check_against(res, want, what):
    """res: Evaluator.result(); want [N,3,5] fp32 from the reference.  EPE to rel 1e-5, the count ratios to 1e-6 absolute."""
    for r, region in enumerate(REGIONS):
        for m, metric in enumerate(METRICS):
            got = res[region][metric]
            assert len(got) == want.shape[0]
            for i, g in enumerate(got):
                w = float(want[i, r, m])
                if metric == "EPE":
                    assert abs(g - w) <= 1e-5 * abs(w), (what, region, metric, i, g, w)
                else:
                    assert abs(g - w) <= 1e-6, (what, region, metric, i, g, w)


def _valid_for(protocol, valid_gt):
    # the fixture's valid_gt is 0 / 1; middlebury / eth3d test `valid_gt >= -0.5` (evaluation.py:154,500): holes are -1 there
    return valid_gt * 2 - 1 if protocol in ("middlebury", "eth3d") else valid_gt


@pytest.mark.parametrize("protocol", ["things", "kitti", "middlebury", "eth3d"])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_evaluator_matches_reference_metrics(fx, protocol, k):
    from anystereo.harness.evaluate import Evaluator
    b = SHAPES[k][0]
    ev = Evaluator(protocol)
    est, dl, dr = fx[f"s{k}_est"], fx[f"s{k}_dl"], fx[f"s{k}_dr"]
    assert tuple(dl.shape) == SHAPES[k]
    valid = _valid_for(protocol, fx[f"s{k}_valid_gt"])
    if protocol == "things":
        ev.update(est, dl, valid, gt_right=dr)
        want = fx[f"s{k}_filter"]
    else:
        ev.update(est, dl, valid, noc=fx[f"s{k}_occ_mask"])
        want = fx[f"s{k}_plain"]
    res = ev.result()
    assert res["images"] == {"seen": b, "all": b, "noc": b, "occ": b}
    _check_against(res, want, (protocol, k))


def test_lr_consistency_host_matches_reference_mask(fx):
    from anystereo.harness.evaluate import lr_consistency_host
    for k, (b, h, w) in enumerate(SHAPES):
        got = lr_consistency_host(fx[f"s{k}_dl"], fx[f"s{k}_dr"])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (b, h, w)
        col = torch.arange(w).float()
        near = ((col - fx[f"s{k}_l2r2l"]).abs() - 3.0).abs() < 1e-3
        assert near.float().mean().item() <= 0.005
        assert torch.equal(got[~near], fx[f"s{k}_occ_mask"][~near])


def test_inf_estimates_count_as_zero(fx):
    from anystereo.harness.evaluate import metric_rows_host
    est, dl = fx["s0_est"][:1], fx["s0_dl"]
    assert torch.isinf(est).sum() >= 5
    zeroed = torch.where(torch.isinf(est), torch.zeros_like(est), est)
    assert torch.equal(metric_rows_host(est, dl), metric_rows_host(zeroed, dl))


def test_filter_rule_skips_the_small_region(fx):
    """"things": 4 non-occluded pixels of 1920 with gt > 0 -> the noc region is skipped, all and occ count."""
    from anystereo.harness.evaluate import Evaluator
    assert fx["case_filter_skip"].tolist() == [0, 1, 0]
    ev = Evaluator("things")
    ev.update(fx["s0_est"][1, :1], fx["s0_dl"][:1], fx["case_filter_valid_gt"], gt_right=fx["s0_dr"][:1])
    res = ev.result()
    assert res["images"] == {"seen": 1, "all": 1, "noc": 0, "occ": 1}
    assert res["noc"] == {m: [0.0] for m in METRICS}
    want = fx["case_filter_out"].unsqueeze(0)
    for r in (0, 2):
        for m, metric in enumerate(METRICS):
            g, w = res[REGIONS[r]][metric][0], float(want[0, r, m])
            assert abs(g - w) <= (1e-5 * abs(w) if metric == "EPE" else 1e-6), (REGIONS[r], metric, g, w)
    # the plain protocols have no such rule: the same image counts in every region
    ev = Evaluator("kitti")
    ev.update(fx["s0_est"][1, :1], fx["s0_dl"][:1], fx["case_filter_valid_gt"], noc=fx["s0_occ_mask"][:1])
    assert ev.result()["images"] == {"seen": 1, "all": 1, "noc": 1, "occ": 1}


@pytest.mark.parametrize("protocol", ["things", "kitti"])
def test_guard_skips_an_image_without_non_occluded_pixels(fx, protocol):
    from anystereo.harness.evaluate import Evaluator
    ev = Evaluator(protocol)
    kw = {"gt_right": fx["s0_dr"][:1]} if protocol == "things" else {"noc": fx["s0_occ_mask"][:1]}
    ev.update(fx["s0_est"][1, :1], fx["s0_dl"][:1], fx["case_guard_valid_gt"], **kw)
    res = ev.result()
    assert res["images"] == {"seen": 1, "all": 0, "noc": 0, "occ": 0}
    # followed by an ordinary image: only that one counts, in every region
    ev.update(fx["s1_est"][1], fx["s1_dl"], fx["s1_valid_gt"], **({"gt_right": fx["s1_dr"]} if protocol == "things" else {"noc": fx["s1_occ_mask"]}))
    res = ev.result()
    assert res["images"] == {"seen": 2, "all": 1, "noc": 1, "occ": 1}
    _check_against(res, fx["s1_filter" if protocol == "things" else "s1_plain"][1:2], (protocol, "guard"))
    # an image whose occluded region alone is empty keeps its all / noc numbers
    ev = Evaluator(protocol)
    noc_only = fx["s1_valid_gt"] * fx["s1_occ_mask"].float()
    ev.update(fx["s1_est"][1], fx["s1_dl"], noc_only, **({"gt_right": fx["s1_dr"]} if protocol == "things" else {"noc": fx["s1_occ_mask"]}))
    res = ev.result()
    assert res["images"] == {"seen": 1, "all": 1, "noc": 1, "occ": 0}
    assert res["all"] == res["noc"] and res["occ"]["EPE"] == [0.0]


def test_image_mean_over_three_updates(fx):
    """Five images in three updates of different shapes: every image weighs the same.  Expected values from the per-image
    functions of harness/metrics.py."""
    from anystereo.harness import metrics as M
    from anystereo.harness.evaluate import Evaluator
    ev = Evaluator("kitti")
    per_image = {(r, m): [] for r in range(3) for m in range(5)}
    for k in range(3):
        est, dl, occ = fx[f"s{k}_est"], fx[f"s{k}_dl"], fx[f"s{k}_occ_mask"].bool()
        valid = fx[f"s{k}_valid_gt"] >= 0.5
        ev.update(est, dl, fx[f"s{k}_valid_gt"], noc=fx[f"s{k}_occ_mask"])
        e = torch.where(torch.isinf(est[0]), torch.zeros_like(est[0]), est[0])
        for i in range(dl.shape[0]):
            for r, mask in enumerate((valid, valid & occ, valid & ~occ)):
                a = (e[i:i + 1], dl[i:i + 1], mask[i:i + 1])
                vals = [M.epe_metric(*a), M.d1_metric(*a), M.thres_metric(*a, 1.0), M.thres_metric(*a, 2.0), M.thres_metric(*a, 3.0)]
                for m, v in enumerate(vals):
                    per_image[(r, m)].append(float(v))
    res = ev.result()
    assert res["images"] == {"seen": 5, "all": 5, "noc": 5, "occ": 5}
    for (r, m), vals in per_image.items():
        want = sum(vals) / len(vals)
        got = res[REGIONS[r]][METRICS[m]][0]
        assert abs(got - want) <= (1e-5 * want if m == 0 else 1e-6), (REGIONS[r], METRICS[m], got, want)


def test_max_disp_and_thresholds(fx):
    from anystereo.harness.evaluate import Evaluator, metric_rows_host
    est, dl = fx["s2_est"][1:], fx["s2_dl"]
    rows = metric_rows_host(est, dl, None, None, float("-inf"), 10.0, (0.5, 1.5, 4.0))
    m = dl < 10.0
    err = (dl - est[0]).abs()
    for i in range(dl.shape[0]):
        assert rows[0, i, 0] == m[i].sum() and rows[0, i, 12] == 0 and rows[0, i, 18] == (dl[i] > 0).sum()
        assert [int(x) for x in rows[0, i, 3:6]] == [int((m[i] & (err[i] > t)).sum()) for t in (0.5, 1.5, 4.0)]
    ev = Evaluator("kitti", max_disp=10.0, thres=(0.5, 1.5, 4.0))
    ev.update(est, dl)
    assert abs(ev.result()["all"]["Thres3"][0] - float((rows[0, :, 5] / rows[0, :, 0]).mean())) < 1e-12


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _images(z):
    """The fixture's five images as single-image updates: (est [2,1,H,W], gt, valid_gt, gt_right)."""
    out = []
    for k in range(3):
        for i in range(SHAPES[k][0]):
            out.append(tuple(z[f"s{k}_{n}"][..., i:i + 1, :, :] for n in ("est", "dl", "valid_gt", "dr")))
    return out


def _merge_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import sys
    sys.path.insert(0, os.path.join(ROOT, "any-stereo_amd"))
    import numpy as np
    from anystereo.harness import dist
    from anystereo.harness.evaluate import Evaluator
    torch.set_num_threads(2)
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval_metrics.npz"))
    imgs = _images({k: torch.from_numpy(z[k]) for k in z.files})
    r, w, _ = dist.init("gloo")
    single = Evaluator("things")
    for est, gt, valid, right in imgs:
        single.update(est, gt, valid, gt_right=right)
    ev = Evaluator("things")
    for i in dist.shard_indices(len(imgs), r, w):
        est, gt, valid, right = imgs[i]
        ev.update(est, gt, valid, gt_right=right)
    ev.merge()
    same_rows = torch.equal(ev.rows(), single.rows())
    res, want = ev.result(), single.result()
    dist.finalize()
    q.put((r, same_rows, res == want, res["images"]))


def test_merge_over_ranks_world2():
    """A dataset of 5 images sharded round-robin over 2 gloo ranks: the merged rows and result equal the single-process ones exactly."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(30)
        assert p.exitcode == 0
    for r, same_rows, same_result, images in res:
        assert same_rows and same_result, r
        assert images == {"seen": 5, "all": 5, "noc": 5, "occ": 5}


def test_abi_argument_validation_without_gpu():
    """Null pointers and non-positive sizes -> AS_ERR_BAD_ARG (-1), H or W below 2 for the consistency mask -> AS_ERR_BAD_SHAPE (-2);
    both before any launch, so no GPU is needed."""
    from anystereo import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    assert lib.as_abi_version() == 38
    buf = (ctypes.c_double * 64)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    inf = float("inf")
    assert lib.as_disp_metrics(null, p, null, null, p, p, 1, 1, 4, 4, -inf, inf, 1.0, 2.0, 3.0, null) == -1
    assert b"disp_metrics" in lib.as_last_error_string()
    assert lib.as_disp_metrics(p, p, null, null, p, null, 1, 1, 4, 4, -inf, inf, 1.0, 2.0, 3.0, null) == -1
    assert lib.as_disp_metrics(p, p, null, null, p, p, 0, 1, 4, 4, -inf, inf, 1.0, 2.0, 3.0, null) == -1
    assert lib.as_disp_metrics(p, p, null, null, p, p, 1, 1, 4, -4, -inf, inf, 1.0, 2.0, 3.0, null) == -1
    assert lib.as_lr_consistency(null, p, p, 1, 4, 4, 3.0, null) == -1
    assert b"lr_consistency" in lib.as_last_error_string()
    assert lib.as_lr_consistency(p, p, p, 0, 4, 4, 3.0, null) == -1
    assert lib.as_lr_consistency(p, p, p, 1, 1, 4, 3.0, null) == -2
    assert lib.as_lr_consistency(p, p, p, 1, 4, 1, 3.0, null) == -2
    for bad in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, -1, 4), (1, 1, 4, 0)):
        assert lib.as_disp_metrics_partial_elems(*bad) < 0, bad
    assert lib.as_disp_metrics_partial_elems(3, 2, 64, 200) == 3 * 2 * 7 * 19  # one row of 19 per 2048-pixel chunk
    assert lib.as_disp_metrics_partial_elems(1, 1, 24, 80) == 19
    assert lib.as_disp_metrics_partial_elems(1, 1, 1024, 2048) == 1024 * 19       # 2^21 pixels: still one trip per block
    assert lib.as_disp_metrics_partial_elems(1, 1, 1030, 2040) == 513 * 19        # above: two trips, 4096 pixels per chunk


def test_ops_refuse_cpu_tensors():
    from anystereo import ops
    z = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_metrics(z, z)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.lr_consistency(z, z)
