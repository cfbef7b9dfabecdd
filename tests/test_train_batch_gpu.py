"""GPU (-m gpu): multi-scale training batches made on the device (csrc/train_batch.hip: as_train_queries, as_low_disp) against their
plain-torch restatements on the CPU (harness/batches.py), against properties that do not depend on the restatement, against the
reference's own arrays where the mode draws nothing (tests/golden/train_batch.npz), and through one training step.

Every comparison is bit for bit (int32 views, so inf and NaN count).  Shapes: h_lr x w_lr = 8 x 12 (Q = 96) and 6 x 11 (Q = 66, not
a multiple of a wave); ragged crops from N == Q over an odd width and 33 x 67 (two scan tiles, the last one ragged) to 70 x 150 (six
tiles); B from 1 to 9, one above the 8 samples a launch carries."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ["dense", "dense_all", "sparse", "sparse_ordered"]
SIZES = {96: [(8, 12), (11, 16), (24, 35), (33, 67), (70, 150)], 66: [(6, 11), (11, 16), (24, 35), (33, 67), (70, 150)]}
MAX_B = 9


def bits(t):
    return t.contiguous().view(torch.int32)


def make_crops(q, mode):
    """MAX_B ragged crops on the CPU.  Sparse modes: about 40 % of the values are <= 0 (V > Q but for the smallest crop), sample 5
    has no valid pixel, sample 6 only valid ones, samples 7 (24 x 35) and 8 (33 x 67, two tiles) have V < Q < N, so Q - V of their
    invalid pixels are drawn; every other even sample holds +inf (valid), -inf and NaN (invalid)."""
    from anystereo.harness.synthetic import det_uniform
    sparse_range = {5: (-80.0, -0.5), 6: (0.5, 60.0), 7: (-400.0, 30.0), 8: (-3000.0, 60.0)}
    crops = []
    for b in range(MAX_B):
        size = SIZES[q][0] if mode == "dense_all" else SIZES[q][b % len(SIZES[q])]
        lo, hi = (0.5, 60.0) if mode.startswith("dense") else sparse_range.get(b, (-40.0, 60.0))
        c = det_uniform(size, 500 + 10 * b + q, lo, hi)
        if b not in (5, 6) and b % 2 == 0:
            c.view(-1)[1], c.view(-1)[c.numel() // 2], c.view(-1)[c.numel() - 1] = float("inf"), float("nan"), float("-inf")
        crops.append(c.contiguous())
    return crops


_cache = {}


def both(q, mode):
    """(crops, host result for MAX_B samples, device result for MAX_B samples), each computed once and left unchanged."""
    if (q, mode) not in _cache:
        from anystereo import ops
        from anystereo.harness.batches import train_queries_host
        crops = make_crops(q, mode)
        want = train_queries_host(crops, q, mode, seed=2024)
        got = tuple(t.cpu() for t in ops.train_queries([c.to(DEV) for c in crops], q, mode, 2024))
        _cache[(q, mode)] = (crops, want, got)
    return _cache[(q, mode)]


@pytest.mark.parametrize("q", [96, 66])
@pytest.mark.parametrize("mode", MODES)
def test_train_queries_equal_the_host_restatement(mode, q):
    from anystereo import ops
    crops, want, got = both(q, mode)
    for b in range(1, MAX_B + 1):  # a result row depends on (seed, b, mode) alone: the first b rows of the full batch
        res = got if b == MAX_B else tuple(t.cpu() for t in ops.train_queries([c.to(DEV) for c in crops[:b]], q, mode, 2024))
        for name, g, w in zip(("hr_coord", "hr_disp", "index", "n_valid"), res, want):
            assert g.dtype == w.dtype and g.shape == w[:b].shape, (name, b, g.shape)
            assert torch.equal(bits(g), bits(w[:b])), (name, b, mode, q)


@pytest.mark.parametrize("q", [96, 66])
@pytest.mark.parametrize("mode", MODES)
def test_train_queries_properties(mode, q):
    from anystereo.nn.liif import make_coord
    crops, _, (coord, disp, index, n_valid) = both(q, mode)
    assert tuple(coord.shape) == (MAX_B, q, 2) and tuple(disp.shape) == (MAX_B, 1, q) and tuple(index.shape) == (MAX_B, q)
    for b, crop in enumerate(crops):
        flat, idx = crop.reshape(-1), index[b].long()
        assert int(idx.min()) >= 0 and int(idx.max()) < flat.numel()
        assert idx.unique().numel() == q, (b, "a pixel drawn twice")
        assert torch.equal(bits(disp[b, 0]), bits(flat[idx]))
        assert torch.equal(bits(coord[b]), bits(make_coord(list(crop.shape))[idx]))
        v = int((flat > 0).sum())
        if mode.startswith("dense"):
            assert int(n_valid[b]) == flat.numel()
            if flat.numel() == q:
                assert torch.equal(idx.sort().values, torch.arange(q))  # every pixel exactly once
            continue
        assert int(n_valid[b]) == v
        head = idx[:min(v, q)]
        assert bool((flat[head] > 0).all()) and not bool((flat[idx[min(v, q):]] > 0).any())
        if v <= q:
            assert torch.equal(head, (flat > 0).nonzero().view(-1))
    if mode == "dense_all":
        assert torch.equal(index, torch.arange(q, dtype=torch.int32).expand(MAX_B, q))
    if mode == "dense":  # another seed, another draw; the same seed, the same draw
        from anystereo import ops
        dev = [c.to(DEV) for c in crops[:2]]
        assert torch.equal(ops.train_queries(dev, q, mode, 2024)[2].cpu(), index[:2])
        assert not torch.equal(ops.train_queries(dev, q, mode, 2025)[2].cpu()[1], index[1])


@pytest.mark.parametrize("mode", ["sparse", "sparse_ordered"])
def test_sparse_list_over_more_tiles_than_one_scan_chunk(mode):
    """725 x 725 = 525 625 pixels are 257 tiles of 2048: the scan block, which takes 256 tile counts at a time, carries its sum
    into a second chunk.  V < Q, so the queries reach into the invalid part of the list, which lies behind all valid pixels."""
    from anystereo import ops
    from anystereo.harness.batches import train_queries_host
    from anystereo.harness.synthetic import det_uniform
    crop = det_uniform((725, 725), 900, -1.0, 1e-4)
    v = int((crop > 0).sum())
    assert 0 < v < 96
    want = train_queries_host([crop], 96, mode, seed=5)
    got = ops.train_queries([crop.to(DEV)], 96, mode, 5)
    for name, g, w in zip(("hr_coord", "hr_disp", "index", "n_valid"), got, want):
        assert torch.equal(bits(g.cpu()), bits(w)), (name, mode)
    assert int(got[3][0]) == v


@pytest.mark.parametrize("out_hw", [(2, 3), (1, 2), (17, 70)])
def test_low_disp_equals_the_host_restatement(out_hw):
    """The kernel's division is IEEE (hipcc rounds fp32 division correctly by default) and the restatement divides by a tensor, so
    the two agree bit for bit; ATen's CUDA division by a host SCALAR would not (it multiplies by the reciprocal)."""
    from anystereo import ops
    from anystereo.harness.batches import low_disp_host
    from anystereo.harness.synthetic import det_uniform
    sizes = [SIZES[96][b % 5] for b in range(MAX_B)]
    crops = [det_uniform(s, 700 + b, -3.0, 190.0) for b, s in enumerate(sizes)]
    scales = [1.0, 1.375, 2.95, 2.77, 1.3, 1.0, 2.0, 1.9, 2.5]
    want = low_disp_host(crops, scales, out_hw)
    for b in (1, 2, 8, MAX_B):
        got = ops.low_disp([c.to(DEV) for c in crops[:b]], scales[:b], out_hw).cpu()
        assert got.dtype == torch.float32 and tuple(got.shape) == (b,) + tuple(out_hw)
        d = (got - want[:b]).abs().max().item()
        print(f"[low_disp B={b} -> {out_hw}] max |d| = {d:.3e}")
        assert torch.equal(bits(got), bits(want[:b])), (b, d)


def test_build_train_batch_does_not_wait_for_the_stream():
    """Nothing in build_train_batch may wait for the device (a host-to-device copy from pageable memory would: it waits for all
    work queued on the stream), so the host can run ahead of the training step.  With matrix products of several hundred
    milliseconds queued in front, the call returns while they are still running; its results are right once they are done.

    The margin, for whoever sees this fail once: 40 fp32 products of 8192^3 are 4.4e13 flop, about 0.3 s at the chip's fp32
    matrix rate, and the call is about 70 us of host time, so a slower GPU only widens it.  Only a host stall of a few hundred
    milliseconds between `busy.record()` and `busy.query()` fails it without a fault in the code; a wait in the call fails it
    every time."""
    from anystereo.harness.batches import build_train_batch, low_disp_host, train_queries_host
    from anystereo.harness.synthetic import det_uniform, synthetic_pair
    scales = [1.0, 2.95, 1.375]
    disps = [det_uniform((round(8 * s), round(12 * s)), 950 + k, -20.0, 40.0) for k, s in enumerate(scales)]
    i1, i2 = (t.to(DEV) for t in synthetic_pair(3, 8, 12))
    dev_disps = [d.to(DEV) for d in disps]
    for mode in ("dense", "sparse"):
        build_train_batch(i1, i2, dev_disps, scales, seed=1, mode=mode)  # first use: allocations, the library
    a = torch.ones(8192, 8192, device=DEV)
    torch.mm(a, a)
    torch.cuda.synchronize()
    for mode in ("dense", "sparse"):
        busy = torch.cuda.Event()
        for _ in range(40):
            a_sq = torch.mm(a, a)
        busy.record()
        out = build_train_batch(i1, i2, dev_disps, scales, seed=9, mode=mode)
        still_running = not busy.query()
        torch.cuda.synchronize()
        del a_sq
        assert still_running, f"build_train_batch({mode}) returned only after the work queued before it had finished"
        want = train_queries_host(disps, 96, mode, 9)
        assert torch.equal(bits(out[2].cpu()), bits(want[0])) and torch.equal(bits(out[3].cpu()), bits(want[1]))
        assert out[4].is_cuda and torch.equal(out[4].cpu(), torch.tensor(scales).view(3, 1))
        assert torch.equal(bits(out[5].cpu()), bits(low_disp_host(disps, scales, (2, 3))))


def test_modes_without_a_draw_equal_the_reference(golden):
    """dense_all and sparse_ordered draw nothing: the device's arrays are the reference's, bit for bit."""
    from anystereo import ops
    fx = golden("train_batch")
    seen = 0
    for k in range(17):
        mode_id, h_lr, w_lr, _, v, raised = fx[f"c{k}_meta"].tolist()
        if int(mode_id) not in (1, 3):
            continue
        mode, q, crop = MODES[int(mode_id)], int(h_lr * w_lr), fx[f"c{k}_crop"]
        coord, disp, index, n_valid = (t.cpu() for t in ops.train_queries([crop.to(DEV)], q, mode, 0))
        assert int(n_valid[0]) == (int(v) if mode == "sparse_ordered" else crop.numel())
        if raised:  # V > Q: the first Q valid pixels, and V for harness.batches.validate
            assert torch.equal(index[0].long(), (crop.reshape(-1) > 0).nonzero().view(-1)[:q])
        else:
            assert torch.equal(bits(coord[0]), bits(fx[f"c{k}_coord"])) and torch.equal(bits(disp[0]), bits(fx[f"c{k}_flow"])), k
        seen += 1
    assert seen == 8


def test_training_step_on_a_device_built_batch():
    """One eager step of harness.metrics.train_step (IGEV tiny case, 2 iterations, supervise_init so low_disp is consumed) fed from
    build_train_batch on the device: a finite loss, equal to the loss of the same step fed from build_train_batch on the CPU.
    The test prints the time of each step: the first one also pays the first use of every kernel and library plan."""
    from anystereo.harness.batches import build_train_batch
    from anystereo.harness.metrics import train_step
    from anystereo.harness.synthetic import det_uniform, fill_module_deterministic, tiny_train_case
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo")
    model = __models__[args.model](args)
    fill_module_deterministic(model, base_seed=1)
    model = model.to(DEV).train()
    model.freeze_bn()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    _, _, img1, img2, _, _, _ = tiny_train_case("igev")
    disps = [det_uniform((96, 192), 800 + b, 0.5, 40.0) for b in range(2)]
    scales = [1.5, 1.5]
    on_dev = build_train_batch(img1.to(DEV), img2.to(DEV), [d.to(DEV) for d in disps], scales, seed=31, q=300)
    on_cpu = build_train_batch(img1, img2, disps, scales, seed=31, q=300)
    assert len(on_dev) == len(on_cpu) == 6 and tuple(on_dev[2].shape) == (2, 300, 2) and tuple(on_dev[5].shape) == (2, 16, 32)
    for a, b in zip(on_dev[2:], on_cpu[2:]):
        assert a.is_cuda and torch.equal(bits(a.cpu()), bits(b))
    import time
    losses, secs = [], []
    for batch in (on_dev, tuple(t.to(DEV) for t in on_cpu)):
        model.load_state_dict(state)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
        t0 = time.perf_counter()
        loss, _ = train_step(model, opt, None, None, batch, 2, max_disp=args.max_disp, supervise_init=True)
        torch.cuda.synchronize()
        losses.append(loss.item())
        secs.append(time.perf_counter() - t0)
    print(f"[train step on a device-built batch] loss {losses[0]:.6f} (device batch), {losses[1]:.6f} (host batch); the steps took "
          f"{secs[0]:.2f} s (with the first use of every kernel and library plan) and {secs[1]:.2f} s")
    assert torch.isfinite(torch.tensor(losses[0])) and losses[0] == losses[1], losses
