"""Procedural scenes on the device (csrc/scenes/scenes.hip through anystereo/harness/scenes.py): every kernel bit-equal to its
plain-torch restatement (which tests/test_scenes_cpu.py holds against the model), every launching scn_* entry under the guarded,
poisoned allocator of tests/_guarded.py, refused calls launching nothing, and the two consumers — evaluate() and Trainer.step —
running on scenes.
"""
import ctypes as C
import math

import pytest
import torch

import _guarded as GD
from anystereo.harness import scenes as H
from anystereo.nn.liif import make_coord

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEC = H.SceneSpec()

CALLS = {}  # scn_* symbol -> calls made while a guarded context was active


@pytest.fixture(scope="module", autouse=True)
def _counted_library():
    from anystereo import _scenes_lib as S
    with GD.counted(S, CALLS):
        yield


# ---- device == host, bit for bit -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_layers", [1, 2, 8])
@pytest.mark.parametrize("hw", [(1, 1), (7, 13), (37, 53), (64, 128)])
def test_render_pair_equals_host(hw, n_layers):
    spec = H.SceneSpec(n_layers=n_layers)
    got = H.render_pair(spec, 11, 5, 3, hw[0], hw[1], DEV)
    want = H.render_pair_host(spec, 11, 5, 3, hw[0], hw[1])
    for g, w_, name in zip(got, want, ("image1", "image2")):
        assert g.is_cuda and g.shape == (3, 3) + hw and g.dtype == torch.float32
        assert torch.equal(g.cpu(), w_), f"{name}: {int((g.cpu() != w_).sum())} of {w_.numel()} values differ"


@pytest.mark.parametrize("sizes", [[(37, 53), (64, 128), (1, 300)], [(5 + i, 9 + 2 * i) for i in range(9)]], ids=["ragged3", "ragged9"])
def test_ground_truth_equals_host(sizes):
    indices = list(range(3, 3 + len(sizes)))
    got = H.ground_truth(SPEC, 7, sizes, indices, DEV)
    want = H.ground_truth_host(SPEC, 7, sizes, indices)
    for name, gs, ws, dt in zip(("disp", "disp_right", "noc"), got, want, (torch.float32, torch.float32, torch.uint8)):
        for hw, g, w_ in zip(sizes, gs, ws):
            assert g.shape == hw and g.dtype == dt and torch.equal(g.cpu(), w_), (name, hw)
    only = H.ground_truth(SPEC, 7, sizes, indices, DEV, want=("disp_right",))  # null outputs are skipped, not written
    assert only[0] == [None] * len(sizes) and only[2] == [None] * len(sizes)
    assert all(torch.equal(a, b) for a, b in zip(only[1], got[1]))


@pytest.mark.parametrize("q", [1, 255, 257, 5000])
def test_disparity_at_equals_host(q):
    coord = torch.rand(2, q, 2, generator=torch.Generator().manual_seed(q)) * 2.6 - 1.3   # beyond [-1, 1] on both sides
    coord[0, 0], coord[1, -1] = torch.tensor([1.0, -1.0]), torch.tensor([-1.0, 1.0])      # exactly +-1
    coord[0, q // 2], coord[1, q // 2] = torch.tensor([-3.0, 2.5]), torch.tensor([1.0, 1.0])
    got, noc = H.disparity_at(SPEC, 9, [4, 8], coord.to(DEV), [128.0, 300.0], noc=True)
    want, want_noc = H.disparity_at_host(SPEC, 9, [4, 8], coord, [128.0, 300.0], noc=True)
    assert got.shape == (2, 1, q) and noc.shape == (2, q) and noc.dtype == torch.uint8
    assert torch.equal(got.cpu(), want) and torch.equal(noc.cpu(), want_noc)
    right = H.disparity_at(SPEC, 9, [4, 8], coord.to(DEV), [128.0, 300.0], view="right")
    assert torch.equal(right.cpu(), H.disparity_at_host(SPEC, 9, [4, 8], coord, [128.0, 300.0], view="right"))


def test_dense_equals_queries_at_make_coord_on_the_device():
    h, w = 37, 53
    d, _, n = H.ground_truth(SPEC, 2, [(h, w)], [7], DEV, want=("disp", "noc"))
    at, noc = H.disparity_at(SPEC, 2, [7], make_coord([h, w]).view(1, -1, 2).to(DEV), [w], noc=True)
    assert torch.equal(d[0].view(-1), at.view(-1)) and torch.equal(n[0].view(-1), noc.view(-1))


# ---- memory hygiene ------------------------------------------------------------------------------------------------------------

def test_render_pair_hygiene():
    GD.hygiene(lambda put: H.render_pair(SPEC, 3, 2, 3, 37, 53, DEV), DEV)


def test_ground_truth_hygiene():
    sizes = [(5 + i, 9 + 2 * i) for i in range(9)] + [(37, 53)]   # two launches, the second with two samples
    GD.hygiene(lambda put: H.ground_truth(SPEC, 3, sizes, list(range(len(sizes))), DEV), DEV)
    GD.hygiene(lambda put: H.ground_truth(SPEC, 3, sizes[:3], [0, 1, 2], DEV, want=("noc",)), DEV)


def test_disparity_at_hygiene():
    coord = torch.rand(9, 257, 2, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2   # nine samples: two launches
    mul = [float(50 + b) for b in range(9)]
    GD.hygiene(lambda put: H.disparity_at(SPEC, 3, list(range(9)), put(coord), mul, noc=True), DEV)
    GD.hygiene(lambda put: H.disparity_at(SPEC, 3, list(range(9)), put(coord), mul, view="right"), DEV)


def test_refused_calls_launch_nothing():
    from anystereo import _scenes_lib as S
    from anystereo import ops
    lib = S.load()
    ok = C.byref(SPEC.c_struct())
    nine = C.byref(H.SceneSpec(n_layers=9).c_struct())
    mul, idx = (C.c_float * 2)(1.0, 1.0), (C.c_int * 2)(0, 1)
    for pattern in GD.PATTERNS:
        with GD.guarded(pattern) as g:
            a = torch.empty((2, 3, 8, 16), device=DEV)
            b = torch.empty((2, 3, 8, 16), device=DEV)
            d = torch.empty((8, 16), device=DEV)
            n = torch.empty((8, 16), device=DEV, dtype=torch.uint8)
            o = torch.empty((2, 1, 64), device=DEV)
            coord = g.place(torch.zeros(2, 64, 2), DEV)
            s = ops._stream()
            assert lib.scn_render_pair(ops._p(a), ops._p(b), 2, 8, 16, nine, 0, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_render_pair(ops._p(a), None, 2, 8, 16, ok, 0, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_render_pair(ops._p(a), ops._p(b), 2, 0, 16, ok, 0, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_render_pair(ops._p(a), b.data_ptr() + 2, 2, 8, 16, ok, 0, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_render_pair(ops._p(a), ops._p(b), 70000, 8, 16, ok, 0, 0, s) == S.SCN_ERR_BAD_SHAPE
            rows = [S.GtSample(d.data_ptr(), None, n.data_ptr(), 8, 16, i) for i in range(8)] + [S.GtSample(d.data_ptr(), None, None, 8, 0, 8)]
            assert lib.scn_ground_truth((S.GtSample * 9)(*rows), 9, ok, 0, s) == S.SCN_ERR_BAD_ARG   # the ninth sample refuses the first eight
            assert lib.scn_ground_truth((S.GtSample * 9)(*rows), 8, nine, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_disparity_at(ops._p(coord), ops._p(o), n.data_ptr(), 2, 64, mul, idx, 1, ok, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_disparity_at(ops._p(coord), ops._p(o), None, 2, 64, None, idx, 0, ok, 0, s) == S.SCN_ERR_BAD_ARG
            assert lib.scn_disparity_at(ops._p(coord), ops._p(o), None, 2, 2 ** 30, mul, idx, 0, ok, 0, s) == S.SCN_ERR_BAD_SHAPE
            with pytest.raises(RuntimeError, match="positive"):
                H.render_pair(SPEC, 0, 0, 0, 8, 16, DEV)
            assert g.nothing_written()
            g.check()


def test_every_launching_scenes_symbol_ran_under_a_guard():
    from anystereo import _scenes_lib as S
    missing = [n for n in S.LAUNCHING if not CALLS.get(n)]
    assert not missing, f"never called under a guard: {missing}"
    # what is left launches nothing: three queries of the library itself and the host's derivation
    assert set(S.SIGNATURES) - set(S.LAUNCHING) == {"scn_abi_version", "scn_last_error_string", "scn_source_hash", "scn_layers"}


# ---- the consumers -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.models import __models__, default_args
    m = __models__["continuous_IGEVStereo"](default_args("continuous_IGEVStereo")).eval()
    fill_module_deterministic(m, base_seed=1)
    return m.to(DEV)


@pytest.mark.parametrize("protocol", ["things", "kitti"])
def test_evaluate_runs_on_scenes(model, protocol):
    from anystereo.harness import evaluate as E
    ev = E.Evaluator(protocol)
    res = E.evaluate(model, H.scene_pairs(SPEC, 21, 4, 64, 128, protocol=protocol, device=DEV), scale=1.5, iters=3, protocol=protocol,
                     evaluator=ev)
    assert res["pairs"] == 4 and res["images"] == {"seen": 4, "all": 4, "noc": 4, "occ": 4}
    rows = ev.rows()[0]                       # [images, 19]: the pixels of region all / noc / occ at columns 0 / 6 / 12
    assert bool((rows[:, 0] == 64 * 128).all()) and bool((rows[:, 6] > 0).all()) and bool((rows[:, 12] > 0).all())
    assert bool((rows[:, 6] + rows[:, 12] == rows[:, 0]).all())
    for region in E.REGIONS:
        assert all(math.isfinite(v[0]) for v in res[region].values())
    # the rolled pair (synthetic_pair(shift=6)) has a constant ground truth, the right view's equal to it: nothing is occluded but
    # the columns that leave the frame, which is what its evaluation has always counted
    gt = torch.full((1, 64, 128), 6.0, device=DEV)
    if protocol == "things":
        from anystereo import ops
        rolled = ops.lr_consistency(gt, gt.clone(), 3.0)
        assert bool((rolled[..., 6:] == 1).all())
        _, _, scene_gt, _, scene_right = next(iter(H.scene_pairs(SPEC, 21, 1, 64, 128, protocol=protocol, device=DEV)))
        assert int((ops.lr_consistency(scene_gt, scene_right, 3.0)[..., 16:] == 0).sum()) > 100   # occlusions inside the frame
    else:
        flat = E.Evaluator(protocol)
        flat.update(gt.clone(), gt, torch.ones_like(gt), noc=torch.ones((1, 64, 128), dtype=torch.uint8, device=DEV))
        assert flat.result()["images"]["occ"] == 0


def test_two_trainer_steps_on_scene_batches():
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo")
    m = __models__["continuous_IGEVStereo"](args)
    fill_module_deterministic(m, base_seed=1)
    tr = Trainer(m.to(DEV), lr=2e-4, num_steps=1000, train_iters=2, max_disp=args.max_disp, graph=False, supervise_init=True)
    losses = []
    for step in range(2):
        batch = H.scene_train_batch(SPEC, 5, step, 2, 64, 128, mode="dense", device=DEV)
        assert len(batch) == 6 and all(t.is_cuda for t in batch) and batch[2].shape == (2, 64 * 128, 2)
        assert torch.equal(batch[3], H.disparity_at(SPEC, 5, H.train_batch_indices(step, 2), batch[2],
                                                    [round(128 * s) for s in batch[4].view(-1).tolist()]))
        loss, _ = tr.step(batch)
        losses.append(float(loss))
    assert all(math.isfinite(v) for v in losses), losses
