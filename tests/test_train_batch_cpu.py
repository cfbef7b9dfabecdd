"""CPU: multi-scale training batches (anystereo/harness/batches.py, csrc/train_batch.hip).  The plain-torch restatement of
`as_train_queries` replays the reference's own draws and equals the reference's StereoDataset.__getitem__ bit for bit
(tests/golden/train_batch.npz, written by tests/golden/make_golden_train_batch.py); the keyed bijection is a permutation and draws
uniformly; the two C entries refuse every host-detectable misuse before any launch.

Limits.  Queries and gathered ground truth: equal, bit for bit (NaN payloads included).  Uniformity: both chi-square statistics below
scipy.stats.chi2.ppf(1 - 1e-6, 175) = 278.7 (the statistic's mean is 175; np.random.choice itself gives 161).  low_disp against torch's
bilinear F.interpolate on the CPU: |d| <= 8 * 2^-24 * max|crop| / (4 s) — the resize is a convex combination formed with at most
seven fp32 roundings (1 - l1 twice, four products and two sums per stage share them) and one for the division, each at most
2^-24 relative to a magnitude no larger than max|crop|; ATen's CPU kernel orders the same products differently."""
import ctypes

import pytest
import torch

N_CASES = 17
MODE_NAMES = ["dense", "dense_all", "sparse", "sparse_ordered"]
CHI2_LIMIT = 278.7


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def fx(golden):
    f = golden("train_batch")
    assert sum(1 for k in f if k.endswith("_meta")) == N_CASES
    return f


def case(fx, k):
    mode_id, h_lr, w_lr, scale, v, raised = fx[f"c{k}_meta"].tolist()
    return MODE_NAMES[int(mode_id)], int(h_lr), int(w_lr), scale, int(v), bool(raised), fx[f"c{k}_crop"]


def test_fixture_covers_the_cases(fx):
    """V = 0, V < Q, V == Q, V > Q, V == N in both sparse modes, a crop with inf and NaN in every mode, the reference's assert."""
    seen = {m: set() for m in MODE_NAMES}
    nonfinite = set()
    for k in range(N_CASES):
        mode, h_lr, w_lr, _, v, raised, crop = case(fx, k)
        q, n = h_lr * w_lr, crop.numel()
        assert v == int((crop > 0).sum())
        for name, hit in (("V=0", v == 0), ("V<Q", 0 < v < q), ("V==Q", v == q), ("V>Q", v > q), ("V==N", v == n)):
            if hit:
                seen[mode].add(name)
        if crop.isinf().any() and crop.isnan().any():
            nonfinite.add(mode)
        assert raised == (mode == "sparse_ordered" and v > q)
    assert seen["sparse"] == {"V=0", "V<Q", "V==Q", "V>Q", "V==N"}
    assert seen["sparse_ordered"] == {"V=0", "V<Q", "V==Q", "V>Q", "V==N"}
    assert nonfinite == set(MODE_NAMES)


@pytest.mark.parametrize("k", range(N_CASES))
def test_replay_of_the_reference_draws_is_bit_equal(fx, k):
    from anystereo.harness.batches import train_queries_host, validate
    mode, h_lr, w_lr, _, v, raised, crop = case(fx, k)
    q = h_lr * w_lr
    draw = fx.get(f"c{k}_draw")
    assert (draw is not None) == (mode in ("dense", "sparse"))
    coord, disp, index, n_valid = train_queries_host([crop], q, mode, seed=5, indices=[draw])
    assert coord.dtype == disp.dtype == torch.float32 and index.dtype == n_valid.dtype == torch.int32
    assert tuple(coord.shape) == (1, q, 2) and tuple(disp.shape) == (1, 1, q) and tuple(index.shape) == (1, q)
    assert n_valid.tolist() == [v if mode.startswith("sparse") else crop.numel()]
    assert torch.equal(bits(disp[0, 0]), bits(crop.reshape(-1)[index[0].long()]))
    if raised:
        with pytest.raises(ValueError, match="sample_q is too small"):
            validate(n_valid, q, mode)
        assert torch.equal(index[0].long(), (crop.reshape(-1) > 0).nonzero().view(-1)[:q])  # the first Q valid pixels
        return
    validate(n_valid, q, mode)
    assert torch.equal(bits(coord[0]), bits(fx[f"c{k}_coord"])), (coord[0] - fx[f"c{k}_coord"]).abs().max()
    assert torch.equal(bits(disp[0]), bits(fx[f"c{k}_flow"]))


@pytest.mark.parametrize("k", range(N_CASES))
def test_low_disp_host_against_torch_bilinear(fx, k):
    from anystereo.harness.batches import low_disp_host
    mode, h_lr, w_lr, scale, _, _, crop = case(fx, k)
    if f"c{k}_low" not in fx:
        assert not torch.isfinite(crop).all()
        return
    want = fx[f"c{k}_low"]
    got = low_disp_host([crop], [scale], (h_lr // 4, w_lr // 4))
    assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + tuple(want.shape)
    d = (got[0] - want).abs().max().item()
    tol = 8 * 2.0 ** -24 * crop.abs().max().item() / (4 * scale)
    print(f"[low_disp_host case {k} {tuple(crop.shape)} -> {tuple(want.shape)} x{scale}] max |d| = {d:.3e}, limit {tol:.3e}")
    assert d <= tol, (k, d, tol)


@pytest.mark.parametrize("n", [1, 2, 3, 96, 176, 840, 2211])
def test_bijection_is_a_permutation(n):
    from anystereo.harness.batches import MODES, permute, round_keys
    j = torch.arange(n)
    for seed in (0, 1, 2, 77, 2 ** 31, 2 ** 63 + 12345, 2 ** 64 - 1):
        for b, mode in ((0, "dense"), (3, "sparse"), (9, "dense")):
            assert mode in MODES
            p = permute(j, n, round_keys(seed, b, mode))
            assert p.dtype == torch.int64 and torch.equal(p.sort().values, j), (n, seed, b, mode)


def test_bijection_is_a_permutation_of_the_largest_cfg4_crop():
    """472 x 944 = 445 568 pixels, the crop of a 160 x 320 input at scale 2.95 (19 bits: halves of 9 and 10)."""
    from anystereo.harness.batches import permute, round_keys
    n = 472 * 944
    j = torch.arange(n)
    for seed, b, mode in ((0, 0, "dense"), (12345, 3, "sparse"), (2 ** 63 + 5, 1, "dense")):
        assert torch.equal(permute(j, n, round_keys(seed, b, mode)).sort().values, j), (seed, b, mode)


def test_draws_are_uniform():
    """N = 176, Q = 96, seeds 0..3999: the inclusion counts of the pixels (variance E (1 - Q/N) of a draw without replacement, and
    the factor (N-1)/N because the counts of a seed sum to Q) and the counts of the first drawn pixel, as chi-square statistics
    with N - 1 degrees of freedom.  Deterministic: fixed seeds, integer arithmetic."""
    from anystereo.harness.batches import ROUNDS, permute, round_keys
    n, q, seeds = 176, 96, 4000
    keys = torch.tensor([round_keys(s, 0, "dense") for s in range(seeds)], dtype=torch.int64)
    draws = permute(torch.arange(q).expand(seeds, q), n, [keys[:, r:r + 1] for r in range(ROUNDS)])
    assert tuple(draws.shape) == (seeds, q) and int(draws.min()) >= 0 and int(draws.max()) < n
    assert all(len(set(row)) == q for row in draws[:50].tolist())
    assert torch.equal(draws[7], permute(torch.arange(q), n, round_keys(7, 0, "dense")))  # the batched keys are the per-seed ones
    cnt = torch.bincount(draws.reshape(-1), minlength=n).double()
    e = seeds * q / n
    chi_incl = float(((cnt - e) ** 2 / (e * (1 - q / n))).sum() * (n - 1) / n)
    first = torch.bincount(draws[:, 0], minlength=n).double()
    e1 = seeds / n
    chi_first = float(((first - e1) ** 2 / e1).sum())
    print(f"[uniformity N={n} Q={q} seeds={seeds}] inclusion chi2 = {chi_incl:.1f}, first-draw chi2 = {chi_first:.1f}, limit {CHI2_LIMIT}")
    assert chi_incl < CHI2_LIMIT and chi_first < CHI2_LIMIT


def test_seed_and_sample_select_the_draw():
    from anystereo.harness.batches import train_queries_host
    crop = torch.arange(1, 177, dtype=torch.float32).view(11, 16)
    a = train_queries_host([crop, crop], 96, "dense", seed=11)
    b = train_queries_host([crop, crop], 96, "dense", seed=11)
    c = train_queries_host([crop, crop], 96, "dense", seed=12)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[2][0], a[2][1])      # another sample of the batch, the same crop
    assert not torch.equal(a[2], c[2])            # another seed
    s = train_queries_host([crop - 100], 96, "sparse", seed=11)  # 76 valid pixels, 20 drawn invalid ones
    assert not torch.equal(s[2][0, 76:], train_queries_host([crop - 100], 96, "sparse", seed=13)[2][0, 76:])
    assert torch.equal(s[2][0, :76].long(), torch.arange(100, 176))


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_host_restatement_properties(mode):
    """What must hold whatever the draw: distinct pixels, values and coordinates gathered at `index`, valid pixels first."""
    from anystereo.harness.batches import train_queries_host
    from anystereo.harness.synthetic import det_uniform
    from anystereo.nn.liif import make_coord
    q = 96
    sizes = [(8, 12)] if mode == "dense_all" else [(8, 12), (11, 16), (24, 35), (33, 67)]
    lo = 0.5 if mode.startswith("dense") else -30.0
    crops = [det_uniform(s, 40 + i, lo, 40.0) for i, s in enumerate(sizes)]
    coord, disp, index, n_valid = train_queries_host(crops, q, mode, seed=3)
    for b, crop in enumerate(crops):
        idx = index[b].long()
        assert idx.unique().numel() == q
        assert torch.equal(disp[b, 0], crop.reshape(-1)[idx])
        assert torch.equal(coord[b], make_coord(list(crop.shape))[idx])
        if mode.startswith("sparse"):
            v = int((crop > 0).sum())
            assert int(n_valid[b]) == v
            head = idx[:min(v, q)]
            assert bool((crop.reshape(-1)[head] > 0).all())
            if v <= q:
                assert torch.equal(head, (crop.reshape(-1) > 0).nonzero().view(-1))


def test_build_train_batch_has_the_trainer_layout():
    from anystereo.harness.batches import build_train_batch
    from anystereo.harness.synthetic import det_uniform, synthetic_pair
    from anystereo.harness.train import synthetic_train_batch
    h, w, scales = 8, 12, [1.0, 2.95]
    i1, i2 = synthetic_pair(2, h, w)
    disps = [det_uniform((round(h * s), round(w * s)), 60 + k, 0.5, 40.0) for k, s in enumerate(scales)]
    got = build_train_batch(i1, i2, disps, scales, seed=1)
    want = synthetic_train_batch(2, h, w, low_disp=True)
    assert len(got) == len(want) == 6
    for g, t in zip(got, want):
        assert g.shape == t.shape and g.dtype == t.dtype
    assert got[0] is i1 and got[1] is i2 and torch.equal(got[4], torch.tensor(scales).view(2, 1))
    assert len(build_train_batch(i1, i2, disps, scales, seed=1, low_disp=False)) == 5
    assert build_train_batch(i1, i2, disps, scales, seed=1, q=50)[2].shape == (2, 50, 2)
    with pytest.raises(ValueError, match="sample_q is too small"):
        build_train_batch(i1, i2, [disps[1], disps[1]], [2.95, 2.95], seed=1, mode="sparse_ordered", check=True)
    with pytest.raises(ValueError, match="mode"):
        build_train_batch(i1, i2, disps, scales, seed=1, mode="random")


def test_ops_refuse_cpu_tensors():
    from anystereo import ops
    z = torch.ones(8, 12)
    with pytest.raises(RuntimeError, match="train_queries.*CUDA"):
        ops.train_queries([z], 96, "dense", 0)
    with pytest.raises(RuntimeError, match="low_disp.*CUDA"):
        ops.low_disp([z], [1.0], (2, 3))
    with pytest.raises(RuntimeError, match="mode"):
        ops.train_queries([z], 96, "random", 0)


def test_abi_argument_validation_without_gpu():
    """Every host-detectable misuse returns AS_ERR_BAD_ARG (-1) or AS_ERR_BAD_SHAPE (-2) with a message, before any launch: the pointers
    below are never dereferenced on the device."""
    from anystereo import _lib
    lib = _lib.load()
    assert lib.as_abi_version() == 38
    buf = (ctypes.c_float * 64)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    I = ctypes.c_int

    def table(*ptrs):
        return _lib.ptr_array(list(ptrs))[0]

    def ints(*v):
        return (I * len(v))(*v)

    F = ctypes.c_float

    def tq(crops=table(p.value), h=ints(11), w=ints(16), b=1, q=96, mode=0, coord=p, disp=p, index=p, nv=p, scale=None, scale_out=null,
           ws=p, ws_bytes=1 << 20):
        return lib.as_train_queries(crops, h, w, b, q, mode, 7, coord, disp, index, nv, scale, scale_out, ws, ws_bytes, null)

    def says(word=b"train_queries"):
        return word in lib.as_last_error_string()

    for kw in ({"crops": None}, {"h": None}, {"w": None}, {"coord": null}, {"disp": null}, {"index": null}, {"nv": null},
               {"crops": table(0)}, {"crops": table(p.value, 0), "h": ints(11, 11), "w": ints(16, 16), "b": 2},
               {"b": 0}, {"b": -1}, {"q": 0}, {"q": -5}, {"h": ints(0)}, {"w": ints(-16)}, {"mode": 4}, {"mode": -1},
               {"coord": ctypes.c_void_p(p.value + 4)},
               {"scale_out": p}, {"scale": (F * 1)(0.0)}, {"scale": (F * 1)(float("nan")), "scale_out": p}, {"scale": (F * 1)(float("inf"))},
               {"mode": 2, "ws": null}, {"mode": 3, "ws": null}, {"mode": 2, "ws": ctypes.c_void_p(p.value + 2)},
               {"mode": 2, "ws_bytes": 4 * (176 + 1) - 1}, {"mode": 3, "ws_bytes": 0}):
        assert tq(**kw) == -1 and says(), kw
    for kw in ({"q": 177}, {"q": 177, "mode": 2}, {"q": 177, "mode": 3},             # N < Q
               {"q": 96, "mode": 1}, {"q": 177, "mode": 1},                           # dense_all: N != Q
               {"h": ints(11, 8), "w": ints(16, 12), "crops": table(p.value, p.value), "b": 2, "q": 97},   # the second sample is short
               {"h": ints(65536), "w": ints(65536), "q": 96},                         # N above 2^31-1
               {"h": ints(32768, 32768), "w": ints(32768, 32768), "crops": table(p.value, p.value), "b": 2, "q": 1 << 30}):
        assert tq(**kw) == -2 and says(), kw

    # the workspace formula: 4 * sum (N + ceil(N / 2048)) in the sparse modes, nothing in the dense ones
    assert lib.as_train_queries_ws_bytes(ints(33), ints(67), 1, 2) == 4 * (2211 + 2)
    assert lib.as_train_queries_ws_bytes(ints(33, 8, 64), ints(67, 12, 32), 3, 3) == 4 * (2211 + 2 + 96 + 1 + 2048 + 1)
    assert lib.as_train_queries_ws_bytes(ints(33), ints(67), 1, 0) == 0 and lib.as_train_queries_ws_bytes(ints(33), ints(67), 1, 1) == 0
    assert lib.as_train_queries_ws_bytes(ints(33), ints(67), 1, 4) == -1 and says()
    assert lib.as_train_queries_ws_bytes(ints(33), ints(0), 1, 2) == -1 and says()
    assert lib.as_train_queries_ws_bytes(None, ints(67), 1, 2) == -1 and says()
    assert lib.as_train_queries_ws_bytes(ints(65536), ints(65536), 1, 2) == -2 and says()

    def ld(crops=table(p.value), h=ints(11), w=ints(16), scale=(F * 1)(1.375), out=p, b=1, h_out=2, w_out=3):
        return lib.as_low_disp(crops, h, w, scale, out, b, h_out, w_out, null)

    for kw in ({"crops": None}, {"h": None}, {"w": None}, {"scale": None}, {"out": null}, {"crops": table(0)}, {"b": 0}, {"h_out": 0},
               {"w_out": -1}, {"h": ints(0)}, {"w": ints(-3)}, {"scale": (F * 1)(0.0)}, {"scale": (F * 1)(-1.0)},
               {"scale": (F * 1)(float("nan"))}, {"scale": (F * 1)(float("inf"))}):
        assert ld(**kw) == -1 and says(b"low_disp"), kw
    for kw in ({"h": ints(65536), "w": ints(65536)}, {"h_out": 65536, "w_out": 65536}, {"h_out": 65535 * 4 + 1, "w_out": 1}):
        assert ld(**kw) == -2 and says(b"low_disp"), kw
