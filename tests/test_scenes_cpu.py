"""Procedural scenes without a GPU (anystereo/harness/scenes.py): the plain-torch restatements of csrc/scenes/scenes.hip — which
tests/test_scenes_gpu.py holds bit-equal to the kernels — against the model's own properties and an independent float64 loop; the
derived layers against the library's host entry; the refusals of the scn_* entries, which validate before they touch a device.
"""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from _headers import declared_symbols
from anystereo.harness import scenes as H
from anystereo.nn.liif import make_coord

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SPEC = H.SceneSpec()
SEEDS = tuple(range(32))
# lr_consistency_host(gt, gt_right) against the exact mask, scene (seed, index 0) for seeds 0..31 at 64x128 with the default spec:
# the smallest share of agreeing pixels measured on the restatement (mean 0.9598); DESIGN.md "Procedural scenes" records both
LR_AGREEMENT_MEASURED_MIN = 0.9477


@functools.lru_cache(maxsize=None)
def _gt(seed, h=64, w=128):
    d, r, n = H.ground_truth(SPEC, seed, [(h, w)], [0])
    return d[0], r[0], n[0]


def test_same_seed_and_index_same_tensors_other_index_differs():
    a = H.render_pair(SPEC, 5, 3, 2, 24, 48)
    b = H.render_pair(SPEC, 5, 3, 2, 24, 48)
    assert a[0].shape == (2, 3, 24, 48) and a[0].dtype == torch.float32
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0][1], H.render_pair(SPEC, 5, 4, 1, 24, 48)[0][0])  # sample b of a batch is scene index0 + b
    assert not torch.equal(a[0][0], a[0][1]) and not torch.equal(a[0], H.render_pair(SPEC, 6, 3, 2, 24, 48)[0])
    for img in a:
        assert float(img.min()) >= 0.0 and float(img.max()) <= 254.999 and float(img.std()) > 10.0
    g1, g2 = H.ground_truth(SPEC, 5, [(24, 48)], [3]), H.ground_truth(SPEC, 5, [(24, 48)], [4])
    assert all(torch.equal(x[0], y[0]) for x, y in zip(g1, H.ground_truth(SPEC, 5, [(24, 48)], [3])))
    assert not torch.equal(g1[0][0], g2[0][0])
    assert g1[2][0].dtype == torch.uint8 and float(g1[0][0].min()) > 0.0


def test_validate_rejects_a_non_positive_plane_and_bad_ranges():
    assert SPEC.validate() is SPEC
    with pytest.raises(ValueError, match="plane can reach"):
        H.SceneSpec(d_min=0.02).validate()            # 0.02 - 0.05 * 0.375 - 0.05 * 0.5 < 0
    with pytest.raises(ValueError, match="background plane can reach"):
        H.SceneSpec(bg_min=0.01, bg_slope=0.01).validate()
    with pytest.raises(ValueError, match="n_layers"):
        H.SceneSpec(n_layers=9).validate()
    with pytest.raises(ValueError, match="n_layers"):
        H.SceneSpec(n_layers=0).validate()
    with pytest.raises(ValueError, match="slopes"):
        H.SceneSpec(slope_max=0.06).validate()
    with pytest.raises(ValueError, match="plane can reach"):
        H.render_pair(H.SceneSpec(d_min=0.02), 0, 0, 1, 8, 16)  # every call validates
    H.SceneSpec(n_layers=1, d_min=0.0, d_max=0.0).validate()   # no foreground layer, nothing to prove about one


def test_layers_equal_the_librarys_host_derivation():
    from anystereo import _scenes_lib as S
    lib = S.load()
    for seed, index, nl in [(0, 0, 6), (1, 5, 8), (77, 123456, 2), (2 ** 40 + 5, 9, 1), (3, -1, 8)]:
        spec = H.SceneSpec(n_layers=nl)
        out = (C.c_float * (nl * S.SCN_LAYER_FLOATS))()
        S.check(lib.scn_layers(C.byref(spec.c_struct()), seed, index, out), "scn_layers")
        got = np.array(out, dtype=np.float32).reshape(nl, S.SCN_LAYER_FLOATS)
        want = np.array([L.row() for L in H.layers(spec, seed, index)], dtype=np.float32)
        assert np.array_equal(got, want), (seed, index, nl)
        assert want[0, 0] == S.KIND_PLANE and set(want[1:, 0]) <= {S.KIND_ELLIPSE, S.KIND_PARALLELOGRAM}
        assert (np.abs(want[:, 7]) <= 0.05).all() and (np.abs(want[:, 8]) <= 0.05).all()


def test_dense_ground_truth_is_disparity_at_make_coord():
    h, w = 37, 53
    d, r, n = H.ground_truth(SPEC, 2, [(h, w)], [7])
    coord = make_coord([h, w]).view(1, -1, 2)
    at, noc = H.disparity_at(SPEC, 2, [7], coord, [w], noc=True)
    assert at.shape == (1, 1, h * w) and noc.shape == (1, h * w)
    assert torch.equal(d[0].view(-1), at.view(-1)) and torch.equal(n[0].view(-1), noc.view(-1))
    assert torch.equal(r[0].view(-1), H.disparity_at(SPEC, 2, [7], coord, [w], view="right").view(-1))


def test_disparity_scales_exactly_with_the_width():
    w = 53
    coord = (torch.rand(2, 400, 2, generator=torch.Generator().manual_seed(1)) * 2.4 - 1.2)
    one = H.disparity_at(SPEC, 4, [1, 2], coord, [w, w])
    two = H.disparity_at(SPEC, 4, [1, 2], coord, [2 * w, 2 * w])
    assert torch.equal(two, 2 * one)


def _noc_points(seed, h=64, w=128):
    """(u, v, d as a fraction of the width) of the noc pixels of scene (seed, 0)."""
    coord = make_coord([h, w]).view(1, -1, 2)
    d, noc = H.disparity_at(SPEC, seed, [0], coord, [1.0], noc=True)
    keep = noc.view(-1) == 1
    u, v = (coord[0, :, 1] + 1.0) * 0.5, (coord[0, :, 0] + 1.0) * 0.5
    return u[keep], v[keep], d.view(-1)[keep]


@pytest.mark.parametrize("seed", [0, 3, 11])
def test_right_view_returns_the_left_disparity_on_noc_pixels(seed):
    u, v, d = _noc_points(seed)
    assert u.numel() > 1000
    ur = u - d
    coord_r = torch.stack((v * 2.0 - 1.0, ur * 2.0 - 1.0), dim=-1).view(1, -1, 2)
    dr = H.disparity_at(SPEC, seed, [0], coord_r, [1.0], view="right").view(-1)
    assert float((dr - d).abs().max()) <= 1e-6


@pytest.mark.parametrize("seed", [0, 3, 11])
def test_pair_is_photo_consistent_on_noc_pixels(seed):
    u, v, d = _noc_points(seed)
    left = H.colour_at_host(SPEC, seed, 0, u, v, "left")
    right = H.colour_at_host(SPEC, seed, 0, u - d, v, "right")
    assert left.shape == (3, u.numel())
    assert float((left - right).abs().max()) <= 1e-2


def _loop_reference(Ls, aspect, h, w, tie=1e-6):
    """Visible layer and noc per pixel in float64, one pixel and one layer at a time, from the derived layers alone; `unsure` marks a
    pixel whose two best disparities, in either view, lie within `tie`."""
    def plane(L, u, v):
        return L.alpha + L.beta * (u - L.cu) + L.gamma * (v - L.cv)

    def inside(L, u, v):
        if L.kind == 0:
            return True
        du, dv = u - L.cu, (v - L.cv) * aspect
        p, q = (du + L.k * dv) / L.a, dv / L.b
        return p * p + q * q <= 1.0 if L.kind == 1 else (abs(p) <= 1.0 and abs(q) <= 1.0)

    def best_two(cands):
        cands = sorted(cands, key=lambda c: -c[0])
        return cands[0], (cands[1][0] if len(cands) > 1 else float("-inf"))

    layer = np.zeros((h, w), dtype=np.int64)
    noc = np.zeros((h, w), dtype=np.uint8)
    unsure = np.zeros((h, w), dtype=bool)
    for i in range(h):
        v = (i + 0.5) / h
        for j in range(w):
            u = (j + 0.5) / w
            (d, l), second = best_two([(plane(L, u, v), k) for k, L in enumerate(Ls) if inside(L, u, v)])
            ur = u - d
            right = []
            for k, L in enumerate(Ls):
                ul = (ur + L.alpha - L.beta * L.cu + L.gamma * (v - L.cv)) / (1.0 - L.beta)
                if inside(L, ul, v):
                    right.append((plane(L, ul, v), k))
            (dr, lr), second_r = best_two(right)
            layer[i, j], noc[i, j] = l, int(lr == l and ur >= 0.0)
            unsure[i, j] = (d - second < tie) or (dr - second_r < tie)
    return layer, noc, unsure


@pytest.mark.parametrize("seed", [0, 1, 2, 5])
def test_float64_loop_gives_the_same_visible_layer_and_noc(seed):
    h, w = 24, 48
    Ls = H.layers(SPEC, seed, 0)
    want_layer, want_noc, unsure = _loop_reference(Ls, SPEC.aspect, h, w)
    u, v = H._grid_uv(h, w, "cpu")
    got_layer, d = H._seen_left(Ls, SPEC, u, v)
    got_noc = H.ground_truth(SPEC, seed, [(h, w)], [0], want=("noc",))[2][0]
    assert float(unsure.mean()) <= 0.01, f"{unsure.mean():.4f} of the pixels left out"
    keep = ~torch.from_numpy(unsure)
    assert torch.equal(got_layer.view(h, w)[keep], torch.from_numpy(want_layer)[keep])
    assert torch.equal(got_noc[keep], torch.from_numpy(want_noc)[keep])
    assert len(set(want_layer.reshape(-1).tolist())) >= 3  # a scene, not a plane


def test_occluded_share_of_every_default_scene():
    shares = [1.0 - float(_gt(seed)[2].float().mean()) for seed in SEEDS]
    print("occluded share: min %.4f max %.4f" % (min(shares), max(shares)))
    assert all(0.03 <= s <= 0.30 for s in shares), shares


def test_lr_consistency_agrees_with_the_exact_mask():
    """The `things` protocol forms its mask from (gt, gt_right) by a 3-pixel left-right check; on these scenes the exact mask is known.
    Measured on this restatement: minimum 0.9478, mean 0.9598 over the 32 scenes (a prototype of the model gave 0.938 / 0.963)."""
    from anystereo.harness.evaluate import lr_consistency_host
    agree = []
    for seed in SEEDS:
        d, r, n = _gt(seed)
        agree.append(float((lr_consistency_host(d[None], r[None]) == n[None]).float().mean()))
    print("lr agreement: min %.4f mean %.4f" % (min(agree), sum(agree) / len(agree)))
    assert all(a >= LR_AGREEMENT_MEASURED_MIN - 0.02 for a in agree), agree
    d, r, n = _gt(0)
    assert not torch.equal(d, r)  # a right view of its own, unlike the rolled pair's


def test_scene_train_batch_on_the_cpu():
    batch, h, w = 3, 16, 32
    out = H.scene_train_batch(SPEC, 9, step=4, batch=batch, h_lr=h, w_lr=w, rank=1, world=2)
    assert len(out) == 6
    im1, im2, hr_coord, hr_disp, scale, low = out
    q = h * w
    assert im1.shape == im2.shape == (batch, 3, h, w) and hr_coord.shape == (batch, q, 2) and hr_disp.shape == (batch, 1, q)
    assert scale.shape == (batch, 1) and low.shape == (batch, h // 4, w // 4) and low.dtype == torch.float32
    scales = H.scene_scales(9, 4, batch, 1.0, 2.95, rank=1, world=2)
    assert scale.view(-1).tolist() == scales and all(1.0 <= s <= 2.95 for s in scales) and len(set(scales)) == batch
    indices = H.train_batch_indices(4, batch, rank=1, world=2)
    assert indices == [27, 28, 29]
    widths = [round(w * s) for s in scales]
    assert torch.equal(hr_disp, H.disparity_at(SPEC, 9, indices, hr_coord, widths))
    assert torch.equal(im1, H.render_pair(SPEC, 9, indices[0], batch, h, w)[0])
    again = H.scene_train_batch(SPEC, 9, step=4, batch=batch, h_lr=h, w_lr=w, rank=1, world=2)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    other = H.scene_train_batch(SPEC, 9, step=5, batch=batch, h_lr=h, w_lr=w, rank=1, world=2)
    assert not torch.equal(other[0], im1) and not torch.equal(other[4], scale)
    assert len(H.scene_train_batch(SPEC, 9, 0, 1, h, w, low_disp=False)) == 5


def test_scene_pairs_tuples():
    for protocol in ("things", "kitti"):
        pairs = list(H.scene_pairs(SPEC, 1, 2, 16, 32, protocol=protocol))
        assert len(pairs) == 2
        i1, i2, gt, valid, extra = pairs[1]
        assert i1.shape == i2.shape == (1, 3, 16, 32) and gt.shape == valid.shape == extra.shape == (1, 16, 32)
        assert extra.dtype == (torch.float32 if protocol == "things" else torch.uint8) and bool((valid == 1).all())
        assert torch.equal(gt[0], H.ground_truth(SPEC, 1, [(16, 32)], [1], want=("disp",))[0][0])


def test_evaluate_tool_takes_scenes():
    spec = importlib.util.spec_from_file_location("evaluate_tool_scenes", os.path.join(ROOT, "tools", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    a = ev.parse_args(["--scenes"])
    assert a.scenes is True and a.scene_layers is None
    assert ev.parse_args(["--scenes", "--scene-layers", "3"]).scene_layers == 3
    a = ev.parse_args([])
    assert a.scenes is False and a.scene_layers is None
    for bad in (["--scene-layers", "3"], ["--scenes", "--scene-layers", "9"], ["--scenes", "--uint8"]):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)


def test_entries_refuse_before_any_launch():
    """Every scn_* entry validates on the host first, so the codes come back on a machine without a device."""
    from anystereo import _scenes_lib as S
    lib = S.load()
    assert lib.scn_abi_version() == 1 and S.library_info()["matches_sources"] is True
    declared = declared_symbols("scenes")
    assert declared == set(S.SIGNATURES), declared ^ set(S.SIGNATURES)
    assert set(S.LAUNCHING) < set(S.SIGNATURES)
    ok = C.byref(SPEC.c_struct())
    p, odd = 0x10000, 0x10002   # never dereferenced: every call below is refused
    mul, idx = (C.c_float * 1)(1.0), (C.c_int * 1)(0)

    def msg():
        return lib.scn_last_error_string().decode()

    assert lib.scn_render_pair(None, p, 1, 4, 4, ok, 0, 0, None) == S.SCN_ERR_BAD_ARG and "null" in msg()
    assert lib.scn_render_pair(p, p, 0, 4, 4, ok, 0, 0, None) == S.SCN_ERR_BAD_ARG and "positive" in msg()
    assert lib.scn_render_pair(p, p, 1, 4, -1, ok, 0, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_render_pair(p, odd, 1, 4, 4, ok, 0, 0, None) == S.SCN_ERR_BAD_ARG and "aligned" in msg()
    assert lib.scn_render_pair(p, p, 1, 4, 4, None, 0, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_render_pair(p, p, 3, 16384, 16384, ok, 0, 0, None) == S.SCN_ERR_BAD_SHAPE and "2^31" in msg()
    assert lib.scn_render_pair(p, p, 70000, 1, 1, ok, 0, 0, None) == S.SCN_ERR_BAD_SHAPE
    for nl in (0, 9):
        bad = H.SceneSpec(n_layers=nl).c_struct()
        assert lib.scn_render_pair(p, p, 1, 4, 4, C.byref(bad), 0, 0, None) == S.SCN_ERR_BAD_ARG and "n_layers" in msg()
        assert lib.scn_disparity_at(p, p, None, 1, 4, mul, idx, 0, C.byref(bad), 0, None) == S.SCN_ERR_BAD_ARG
        assert lib.scn_layers(C.byref(bad), 0, 0, (C.c_float * 16)()) == S.SCN_ERR_BAD_ARG
    assert lib.scn_render_pair(p, p, 1, 4, 4, C.byref(H.SceneSpec(octaves=7).c_struct()), 0, 0, None) == S.SCN_ERR_BAD_ARG

    def table(*rows):
        return (S.GtSample * len(rows))(*[S.GtSample(*r) for r in rows])

    assert lib.scn_ground_truth(None, 1, ok, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_ground_truth(table((p, None, None, 4, 4, 0)), 0, ok, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_ground_truth(table((None, None, None, 4, 4, 0)), 1, ok, 0, None) == S.SCN_ERR_BAD_ARG and "no output" in msg()
    assert lib.scn_ground_truth(table((p, None, None, 4, 0, 0)), 1, ok, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_ground_truth(table((p, odd, None, 4, 4, 0)), 1, ok, 0, None) == S.SCN_ERR_BAD_ARG and "aligned" in msg()
    assert lib.scn_ground_truth(table((p, None, None, 65536, 32768, 0)), 1, ok, 0, None) == S.SCN_ERR_BAD_SHAPE
    # a bad ninth sample refuses the whole call: nothing is launched for the first eight
    rows = [(p, None, None, 4, 4, i) for i in range(8)] + [(p, None, None, 0, 4, 8)]
    assert lib.scn_ground_truth(table(*rows), 9, ok, 0, None) == S.SCN_ERR_BAD_ARG and "sample 8" in msg()

    assert lib.scn_disparity_at(None, p, None, 1, 4, mul, idx, 0, ok, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_disparity_at(p, p, None, 1, 4, None, idx, 0, ok, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_disparity_at(p, p, None, 1, 0, mul, idx, 0, ok, 0, None) == S.SCN_ERR_BAD_ARG
    assert lib.scn_disparity_at(p + 4, p, None, 1, 4, mul, idx, 0, ok, 0, None) == S.SCN_ERR_BAD_ARG and "aligned" in msg()
    assert lib.scn_disparity_at(p, p, p, 1, 4, mul, idx, 1, ok, 0, None) == S.SCN_ERR_BAD_ARG and "left view" in msg()
    assert lib.scn_disparity_at(p, p, None, 1, 2 ** 30, mul, idx, 0, ok, 0, None) == S.SCN_ERR_BAD_SHAPE
    with pytest.raises(RuntimeError, match="code -1"):
        S.check(lib.scn_render_pair(None, None, 1, 1, 1, ok, 0, 0, None), "render_pair")


def test_python_refusals():
    coord = torch.zeros(1, 4, 2)
    with pytest.raises(ValueError, match="left view"):
        H.disparity_at(SPEC, 0, [0], coord, [1.0], noc=True, view="right")
    with pytest.raises(ValueError, match="view"):
        H.disparity_at(SPEC, 0, [0], coord, [1.0], view="up")
    with pytest.raises(ValueError, match="float32"):
        H.disparity_at(SPEC, 0, [0], coord.double(), [1.0])
    with pytest.raises(ValueError, match="values for 1 samples"):
        H.disparity_at(SPEC, 0, [0, 1], coord, [1.0])
    with pytest.raises(ValueError, match="want"):
        H.ground_truth(SPEC, 0, [(4, 4)], [0], want=("depth",))
    with pytest.raises(ValueError, match="protocol"):
        list(H.scene_pairs(SPEC, 0, 1, 8, 16, protocol="sintel"))
    with pytest.raises(TypeError):
        H.render_pair({"n_layers": 3}, 0, 0, 1, 8, 16)
