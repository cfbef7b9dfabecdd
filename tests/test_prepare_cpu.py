"""CPU: the geometry of arbitrary-scale evaluation stated once (`query.query_plan`), the plain-torch restatements of the two kernels of
csrc/prepare.hip (`query.query_grid_host`, `query.bicubic_pad_host`) against the project's host path and against the reference's own
pad_for_multi_train (tests/golden/prepare_pair.npz, written by tests/golden/make_golden_prepare.py), and the argument checks of the
two C entries (no launch happens).

Limits.  Query grid, crop branch: equal.  `resized` branch: max |d| <= 2.4e-7 — ATen interpolates the 2-D coordinate image, the
separable form two 1-D tables; the two round differently on 7-38 % of the values, by at most one fp32 ulp at 1.0 (1.19e-7); the limit
is twice that.  Padded images: max |d| <= 1e-3 grey levels on the 0..255 scale — a direct fp32 restatement differs from ATen's CPU
result by 2e-4 .. 3e-4 at these shapes (3.0e-4 on this fixture's images, at 45x70 x1.3); the limit is about 4 x that.  Scale 1.0: equal."""
import ctypes
import json
import math
import os

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
# (H, W, scale, divis_by): the first five are the fixture's cases, in its order
SHAPES = [(40, 64, 1.0, 32), (64, 96, 2.0, 32), (37, 53, 1.5, 32), (45, 70, 1.3, 16), (33, 65, 2.95, 32), (375, 1242, 2.0, 32),
          (1988, 2964, 1.5, 32)]
RESIZED = [False, False, True, True, True, True, True]
GRID_TOL = 2.4e-7
IMAGE_TOL = 1e-3
B = 2


@pytest.fixture(scope="module")
def fx(golden):
    f = golden("prepare_pair")
    assert [tuple(c) for c in f["cases"].tolist()] == [tuple(float(v) for v in s) for s in SHAPES[:5]]
    return f


_host = {}


def host_coord(k):
    """hr_coord [H*W,2] and p of the project's host path at SHAPES[k] (computed once)."""
    if k not in _host:
        from anystereo.harness.query import pad_for_multi_train
        h, w, s, div = SHAPES[k]
        z = torch.zeros(1, 3, h, w)
        i1, _, coord, p = pad_for_multi_train(z, z, s, divis_by=div)
        _host[k] = (coord, p, tuple(i1.shape[-2:]))
    return _host[k]


def check_grid(got, want, resized, what):
    """got [B,Q,2] against want [Q,2] under the two limits of the module docstring; prints the figure first."""
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,) + tuple(want.shape), (what, got.shape, want.shape)
    for b in range(B):
        d = (got[b] - want).abs().max().item()
        print(f"[query grid {what} b={b}] resized={resized} max |d| = {d:.3e}")
        if resized:
            assert d <= GRID_TOL, (what, b, d)
        else:
            assert torch.equal(got[b], want), (what, b, d)


def test_query_plan_reproduces_query_grid_json():
    from anystereo.harness.query import query_plan
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "query_grid.json")))
    assert len(cases) == 5
    for c in cases:
        pl = query_plan(c["H"], c["W"], c["scale"], c["divis_by"])
        assert [pl.h_pad, pl.w_pad] == c["padded"], c
        assert list(pl.p) == c["pad_num"], c
        assert [pl.h_want * pl.w_want, 2] == c["coord_shape"], c
        assert (pl.h_pad % c["divis_by"], pl.w_pad % c["divis_by"]) == (0, 0)
        assert pl.h_crop == pl.h_hr - pl.p[0] - pl.p[1] and pl.w_crop == pl.w_hr - pl.p[2] - pl.p[3]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_query_plan_matches_pad_for_multi_train(k):
    from anystereo.harness.query import query_plan
    h, w, s, div = SHAPES[k]
    pl = query_plan(h, w, s, div)
    coord, p, padded = host_coord(k)
    assert (pl.h_pad, pl.w_pad) == padded and list(pl.p) == p and pl.resized == RESIZED[k]
    assert (pl.h_want, pl.w_want) == (h, w) and tuple(coord.shape) == (pl.h_want * pl.w_want, 2)
    assert (pl.h_lr, pl.w_lr) == ((h, w) if s <= 1 else (math.ceil(h / s), math.ceil(w / s)))
    assert pl.h_pad == pl.h_lr + pl.pad[0] + pl.pad[1] and pl.w_pad == pl.w_lr + pl.pad[2] + pl.pad[3]


@pytest.mark.parametrize("h,w,scale,div", [(40, 64, 2, 16), (37, 53, 3, 16), (33, 65, 4, 32), (64, 96, 1, 32)])
def test_query_plan_fixed_matches_pad_for_multi_train_fixed(h, w, scale, div):
    from anystereo.harness.query import pad_for_multi_train_fixed, query_grid_host, query_plan
    z = torch.zeros(1, 3, h, w)
    i1, _, coord, p = pad_for_multi_train_fixed(z, z, scale, divis_by=div)
    pl = query_plan(h, w, scale, div, fixed=True)
    assert (pl.h_pad, pl.w_pad) == tuple(i1.shape[-2:]) and list(pl.p) == p
    assert (pl.h_lr, pl.w_lr) == (h, w) and (pl.h_want, pl.w_want) == (h * scale, w * scale) and not pl.resized
    assert (pl.h_hr, pl.w_hr) == (pl.h_pad * scale, pl.w_pad * scale)
    assert tuple(coord.shape) == (pl.h_want * pl.w_want, 2)
    check_grid(query_grid_host(pl, B), coord, False, f"fixed {h}x{w} x{scale}")


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_query_grid_host_vs_pad_for_multi_train(k):
    from anystereo.harness.query import query_grid_host, query_plan
    h, w, s, div = SHAPES[k]
    check_grid(query_grid_host(query_plan(h, w, s, div), B), host_coord(k)[0], RESIZED[k], f"{h}x{w} x{s}")


@pytest.mark.parametrize("k", range(5))
def test_query_grid_host_vs_reference_fixture(fx, k):
    from anystereo.harness.query import query_grid_host, query_plan
    h, w, s, div = SHAPES[k]
    check_grid(query_grid_host(query_plan(h, w, s, div), B), fx[f"c{k}_coord"], RESIZED[k], f"fixture {h}x{w} x{s}")


@pytest.mark.parametrize("k", range(5))
def test_bicubic_pad_host_vs_reference_fixture(fx, k):
    from anystereo.harness.query import bicubic_pad_host, query_plan
    h, w, s, div = SHAPES[k]
    pl = query_plan(h, w, s, div)
    assert not torch.equal(fx[f"c{k}_image1"][0], fx[f"c{k}_image1"][1])
    for name in ("1", "2"):
        img, want = fx[f"c{k}_image{name}"], fx[f"c{k}_pad{name}"]
        assert img.dtype == torch.uint8 and tuple(img.shape) == (B, 3, h, w)
        got = bicubic_pad_host(img, pl)
        assert got.dtype == torch.float32 and got.shape == want.shape
        d = (got - want).abs().max().item()
        print(f"[bicubic_pad_host {h}x{w} x{s} image{name}] max |d| = {d:.3e}, values {want.min().item():.1f} .. {want.max().item():.1f}")
        if s == 1.0:
            assert torch.equal(got, want)
        else:
            assert d <= IMAGE_TOL, (k, name, d)
        assert torch.equal(bicubic_pad_host(img.float(), pl), got)  # uint8 and the same values as float: the same bits
    if s > 1.0:  # the overshoot of the bicubic kernel is kept, not clamped to 0..255
        assert fx[f"c{k}_pad1"].min().item() < 0 and fx[f"c{k}_pad1"].max().item() > 255


def test_abi_argument_validation_without_gpu():
    """Null pointers, non-positive sizes -> AS_ERR_BAD_ARG (-1); an empty crop, a frame to up-scale, more than 2^31-1 elements, B above
    65535 -> AS_ERR_BAD_SHAPE (-2); all before any launch, so no GPU is needed."""
    from anystereo import _lib
    lib = _lib.load()
    assert lib.as_abi_version() == 38
    buf = (ctypes.c_float * 64)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    ok = (1, 8, 8, 4, 4, 0, 0, 0, 0)  # B, H, W, h_lr, w_lr, pads
    for ptrs in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        assert lib.as_prepare_pair(*ptrs, 0, *ok, null) == -1
        assert b"prepare_pair" in lib.as_last_error_string()
    for bad in ((0, 8, 8, 4, 4, 0, 0, 0, 0), (1, 0, 8, 4, 4, 0, 0, 0, 0), (1, 8, -8, 4, 4, 0, 0, 0, 0), (1, 8, 8, 0, 4, 0, 0, 0, 0),
                (1, 8, 8, 4, 0, 0, 0, 0, 0), (1, 8, 8, 4, 4, -1, 0, 0, 0), (1, 8, 8, 4, 4, 0, 0, 0, -2)):
        assert lib.as_prepare_pair(p, p, p, p, 1, *bad, null) == -1, bad
        assert b"prepare_pair" in lib.as_last_error_string()
    for bad in ((1, 8, 8, 9, 4, 0, 0, 0, 0), (65536, 8, 8, 4, 4, 0, 0, 0, 0), (4, 16384, 16384, 8192, 8192, 0, 0, 0, 0),
                (1, 8, 8, 4, 4, 0, 0, 0, 2 ** 30)):
        assert lib.as_prepare_pair(p, p, p, p, 0, *bad, null) == -2, bad
        assert b"prepare_pair" in lib.as_last_error_string()

    good = (1, 12, 12, 2, 2, 2, 2, 8, 8)  # B, h_hr, w_hr, p (4), h_want, w_want
    assert lib.as_query_grid(null, *good, null) == -1
    assert b"query_grid" in lib.as_last_error_string()
    assert lib.as_query_grid(ctypes.c_void_p(ctypes.addressof(buf) + 4), *good, null) == -1  # not 8-byte aligned
    assert b"query_grid" in lib.as_last_error_string() and b"aligned" in lib.as_last_error_string()
    for bad in ((0, 12, 12, 2, 2, 2, 2, 8, 8), (1, 0, 12, 2, 2, 2, 2, 8, 8), (1, 12, -1, 2, 2, 2, 2, 8, 8), (1, 12, 12, 2, 2, 2, 2, 0, 8),
                (1, 12, 12, 2, 2, 2, 2, 8, 0), (1, 12, 12, -1, 2, 2, 2, 8, 8)):
        assert lib.as_query_grid(p, *bad, null) == -1, bad
        assert b"query_grid" in lib.as_last_error_string()
    for bad in ((1, 12, 12, 6, 6, 2, 2, 8, 8), (1, 12, 12, 2, 2, 10, 2, 8, 8),     # an empty crop
                (65536, 12, 12, 2, 2, 2, 2, 8, 8), (1, 12, 12, 2, 2, 2, 2, 32768, 32768), (64, 12, 12, 2, 2, 2, 2, 4096, 4096)):
        assert lib.as_query_grid(p, *bad, null) == -2, bad
        assert b"query_grid" in lib.as_last_error_string()


def test_ops_refuse_cpu_tensors_and_cpu_device():
    from anystereo import ops
    from anystereo.harness.query import prepare_on_device, query_plan
    pl = query_plan(8, 16, 1.5, 32)
    z = torch.zeros(1, 3, 8, 16)
    with pytest.raises(RuntimeError, match="prepare_pair.*CUDA"):
        ops.prepare_pair(z, z, pl)
    with pytest.raises(RuntimeError, match="prepare_pair.*CUDA"):
        ops.prepare_pair(z.to(torch.uint8), z.to(torch.uint8), pl)
    with pytest.raises(RuntimeError, match="query_grid.*CUDA"):
        ops.query_grid(pl, 1, "cpu")
    with pytest.raises(RuntimeError, match="prepare_pair.*CUDA"):
        prepare_on_device(z, z, 1.5)


def test_registered_operators_have_no_cpu_kernel():
    import anystereo  # noqa: F401
    z = torch.zeros(1, 3, 8, 16)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.anystereo.prepare_pair(z, z, 1.5, 32, False)
    with pytest.raises(NotImplementedError, match="CPU"):
        torch.ops.anystereo.query_grid(z, 1.5, 32, False)


def test_evaluate_refuses_an_unknown_prep():
    from anystereo.harness.evaluate import evaluate
    with pytest.raises(ValueError, match="prep"):
        evaluate(torch.nn.Identity(), [], scale=1.0, iters=1, prep="gpu")
