"""GPU: which captured pass a call selects, and what a cached one keeps alive (anystereo/graphs.py behind `model.enable_graph`).
Models: the default IGEV and RAFT (64x128) with the deterministic fill, 3 GRU iterations, queried on the x1.5 grid (96x192) — the
smallest sizes at which the graphed forward / encode paths exist.

Limits.  Replays of one entry, and a re-capture of the same pass: equal bits (the same kernels on the same operands).  Graph against
eager: 1e-4, the whole-forward replay tests' pin (tests/test_liif_variants.py).  Everything else is counted or compared by identity."""
import gc
import weakref

import pytest
import torch

from anystereo import ops
from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
from anystereo.models.base import default_args
from anystereo.nn import liif as NL

pytestmark = pytest.mark.gpu
DEV = "cuda"
ITERS = 3
H, W = 64, 128
FAMILIES = {"igev": "continuous_IGEVStereo", "raft": "continuous_RAFTStereo"}
_CACHE = {}


def build(family, cls=None):
    from anystereo.models import __models__
    mname = FAMILIES[family]
    model = (cls or __models__[mname])(default_args(mname)).eval()
    fill_module_deterministic(model, base_seed=1)
    return model.to(DEV)


def inputs():
    if "inputs" not in _CACHE:
        img1, img2 = synthetic_pair(1, H, W, shift=6, seed=99)
        coord = NL.make_coord([round(H * 1.5), round(W * 1.5)]).unsqueeze(0).to(DEV)
        _CACHE["inputs"] = (img1.to(DEV), img2.to(DEV), coord, torch.tensor([[1.5]], device=DEV))
    return _CACHE["inputs"]


def setup(family):
    """(model, its eager forward), built once per family; every test leaves the model as it found it (graphs off, no stamps)."""
    if family not in _CACHE:
        model = build(family)
        _CACHE[family] = (model, forward(model))
    return _CACHE[family]


def forward(model):
    img1, img2, coord, scale = inputs()
    with torch.no_grad():
        return model(img1, img2, iters=ITERS, test_mode=True, hr_coord=coord.clone(), scale=scale)


def encode(model, at):
    img1, img2 = inputs()[:2]
    with torch.no_grad():
        return model.encode(img1, img2, iters=ITERS, at=at)


def same_field(a, b):
    _, _, coord, scale = inputs()
    return a.at == b.at and all(torch.equal(a.low(at=k), b.low(at=k)) and
                                torch.equal(a.query(coord.clone(), scale, at=k), b.query(coord.clone(), scale, at=k)) for k in a.at)


def test_selection_rules():
    """The key: weights fingerprint and precision select another entry; the LRU keeps `graph_cache_size`; train() / load_state_dict() /
    _apply() drop every entry."""
    model = build("igev")  # its weights are changed below: not the shared one
    model.graph_cache_size = 2
    model.enable_graph(True)
    o1, o1b = forward(model), forward(model)
    assert len(model._graphs) == 1 and torch.equal(o1, o1b)
    w_old = model._weights_fingerprint()
    with torch.no_grad():
        p = model.context_zqr_convs[0].weight  # -> cz | cr | cq of the 1/4-resolution GRU -> every disparity update
        p.add_(1e-3 * p)
    w_new = model._weights_fingerprint()
    assert w_new != w_old
    o2 = forward(model)
    assert [(k.kind, k.precision, k.weights) for k in model._graphs] == [("forward", "split", w_old), ("forward", "split", w_new)]
    assert not torch.equal(o2, o1)
    try:
        ops.set_precision("fp32")
        forward(model)
        # the entry of the old weights was the least recently used one
        assert [(k.kind, k.precision, k.weights) for k in model._graphs] == [("forward", "split", w_new), ("forward", "fp32", w_new)]
        assert all(k.iters == ITERS and k.at is None and k.stamps is None and k.shapes[0] == (1, 3, H, W) for k in model._graphs)
    finally:
        ops.set_precision("split")
    assert len(model._graphs) == 2
    model.train()
    model.eval()
    assert len(model._graphs) == 0
    forward(model)
    assert len(model._graphs) == 1
    model.load_state_dict(model.state_dict())
    assert len(model._graphs) == 0
    forward(model)
    assert len(model._graphs) == 1
    model.to(DEV)
    assert len(model._graphs) == 0
    model.enable_graph(False)
    d = (o2 - forward(model)).abs().max().item()
    print(f"[selection rules] graph at the new weights against eager at the new weights: max |d| = {d:.3e}")
    assert d <= 1e-4


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_forward_and_encode_share_the_cache(family):
    model, _ = setup(family)
    try:
        model.graph_cache_size = 2
        model.enable_graph(True)
        f1, e1 = forward(model), encode(model, (1, ITERS))
        assert [k.kind for k in model._graphs] == ["forward", "encode"]
        assert [k.at for k in model._graphs] == [None, (1, ITERS)]
        assert torch.equal(forward(model), f1) and same_field(encode(model, (1, ITERS)), e1)
        assert torch.equal(forward(model), f1) and len(model._graphs) == 2
        model.graph_cache_size = 1
        model.enable_graph(True)
        assert torch.equal(forward(model), f1) and [k.kind for k in model._graphs] == ["forward"]
        assert same_field(encode(model, (1, ITERS)), e1) and [k.kind for k in model._graphs] == ["encode"]
        assert torch.equal(forward(model), f1) and [k.kind for k in model._graphs] == ["forward"]  # captured again
    finally:
        model.__dict__.pop("graph_cache_size", None)
        model.enable_graph(False)


def test_stamps_identity():
    """The key holds the Stamps object: a new Stamps selects a new entry, and the old one lives as long as the graph that writes into
    its buffer.  Object lifetime only — no graph whose Stamps is gone is ever replayed."""
    model, _ = setup("igev")
    try:
        s1 = model.stamps = ops.Stamps(DEV)
        model.enable_graph(True)
        forward(model)
        r = s1.read()
        assert "pass_begin" in r and "pass_end" in r and r["pass_end"] > r["pass_begin"]
        w1 = weakref.ref(s1)
        del s1
        s2 = model.stamps = ops.Stamps(DEV)
        forward(model)
        assert len(model._graphs) == 2 and [k.stamps is s for k, s in zip(model._graphs, (w1(), s2))] == [True, True]
        r = s2.read()
        assert "pass_begin" in r and "pass_end" in r and r["pass_end"] > r["pass_begin"]
        gc.collect()
        assert w1() is not None  # its entry is cached
        model.enable_graph(False)
        gc.collect()
        assert w1() is None
    finally:
        model.__dict__.pop("stamps", None)
        model.enable_graph(False)
    assert ops._ACTIVE_STAMPS is None


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_pixel_grid_outlives_its_cache(family):
    model, _ = setup(family)
    try:
        model.enable_graph(True)
        forward(model)
        grids = list(model._pixel_grids.values())
        assert len(grids) == 1 and tuple(grids[0].shape) == (1, H // 4, W // 4, 1)
        ent = next(iter(model._graphs.values()))
        assert any(t is grids[0] for t in ent.refs)
        w = weakref.ref(grids[0])
        del grids, ent
        before = forward(model)
        model._pixel_grids.clear()
        gc.collect()
        assert w() is not None  # the entry holds the tensor its lookup nodes were given
        assert torch.equal(forward(model), before) and torch.equal(forward(model), before)
        assert len(model._graphs) == 1 and not model._pixel_grids  # replays: no Python ran, nothing was re-created
        model.enable_graph(False)
        gc.collect()
        assert w() is None
    finally:
        model.enable_graph(False)


def test_capture_failure_leaves_no_trace():
    """A Python exception on the host during the first warm-up pass (before any capture begins): nothing is cached, the marker sink is
    reset, and the same inputs capture on a sound model."""
    from anystereo.models import __models__

    class Broken(__models__[FAMILIES["igev"]]):
        def _hot_update(self, *a, **k):
            raise RuntimeError("no update block today")

    broken = build("igev", Broken)
    broken.stamps = ops.Stamps(DEV)
    broken.enable_graph(True)
    with pytest.raises(RuntimeError, match="no update block today"):
        forward(broken)
    assert len(broken._graphs) == 0 and ops._ACTIVE_STAMPS is None
    assert not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
    del broken
    model, eager = setup("igev")
    try:
        model.enable_graph(True)
        g1, g2 = forward(model), forward(model)
        assert len(model._graphs) == 1 and torch.equal(g1, g2)
        d = (g1 - eager).abs().max().item()
        print(f"[after a failed capture] replay against eager: max |d| = {d:.3e}")
        assert d <= 1e-4
    finally:
        model.enable_graph(False)
