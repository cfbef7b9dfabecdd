"""CPU: the evaluation pictures (anystereo/harness/images.py) against the reference's own Disp_to_color and disp_error_image_func
outputs (tests/golden/eval_images.npz, written by tests/golden/make_golden_images.py), the 16-bit encoding, the PNG writer and
reader, the argument checks of as_disp_images (no launch happens) and evaluate() with an ImageSink on CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

CASES = [(2, 13, 37, 192.0), (1, 7, 250, 192.0), (2, 24, 203, 400.0), (1, 1, 5, 192.0)]


@pytest.fixture(scope="module")
def fx(golden):
    return golden("eval_images")


def _quantize_like_save_image(v):
    """The issue's definition, stated once more with numpy: (uint8) clamp(fl(fl(v * 255) + 0.5), 0, 255), truncating."""
    x = (v.numpy().astype(np.float32) * np.float32(255.0) + np.float32(0.5)).astype(np.float32)
    return torch.from_numpy(np.clip(x, 0.0, 255.0).astype(np.uint8))


def test_fixture_holds_the_cases_it_is_meant_to(fx):
    assert [tuple(r) for r in fx["cases"].tolist()] == [tuple(float(x) for x in c) for c in CASES]
    for k, (b, h, w, md) in enumerate(CASES):
        for name, shape in (("disp", (b, h, w)), ("gt", (b, h, w)), ("est", (b, h, w)), ("color", (b, h, w, 3)), ("error", (b, h, w, 3))):
            assert tuple(fx[f"c{k}_{name}"].shape) == shape and fx[f"c{k}_{name}"].dtype == torch.float32
        assert not torch.isnan(fx[f"c{k}_disp"]).any()
    for k in (0, 1, 2):
        disp, est, gt = fx[f"c{k}_disp"], fx[f"c{k}_est"], fx[f"c{k}_gt"]
        assert torch.isposinf(disp).any() and torch.isneginf(disp).any() and (disp == CASES[k][3]).any() and (disp < 0).any()
        assert torch.isnan(est).any() and torch.isposinf(est).any() and torch.isneginf(est).any() and (gt <= 0).any()
        # all ten bands, black, and both regimes' planted ground truths are there
        colours = {tuple(px) for px in (fx[f"c{k}_error"] * 255).round().to(torch.uint8).reshape(-1, 3).tolist()}
        assert len(colours) == 11 and (0, 0, 0) in colours
        assert (gt == 30).sum() >= 27 and (gt == 100).sum() >= 27


@pytest.mark.parametrize("k", range(4))
def test_disp_to_color_host_equals_reference(fx, k):
    from anystereo.harness.images import disp_to_color_host, quantize_host
    got = disp_to_color_host(fx[f"c{k}_disp"], CASES[k][3])
    assert got.dtype == torch.float32 and torch.equal(got, fx[f"c{k}_color"])
    assert torch.equal(quantize_host(got), _quantize_like_save_image(fx[f"c{k}_color"]))
    assert torch.equal(disp_to_color_host(fx[f"c{k}_disp"].unsqueeze(1), CASES[k][3]), got)  # [B,1,H,W]


@pytest.mark.parametrize("k", range(4))
def test_error_image_host_equals_reference(fx, k):
    from anystereo.harness.images import ERROR_BANDS, error_image_host, quantize_host
    got = error_image_host(fx[f"c{k}_est"], fx[f"c{k}_gt"])
    assert got.dtype == torch.float32 and torch.equal(got, fx[f"c{k}_error"])
    q = quantize_host(got)
    assert torch.equal(q, _quantize_like_save_image(fx[f"c{k}_error"]))
    # quantising c / 255 gives the integer c back: the legend's ten colours, clipped by the image
    b, h, w, _ = CASES[k]
    for i, c in enumerate(ERROR_BANDS):
        if 20 * i < w:
            assert q[0, 0, 20 * i].tolist() == list(c) and q[-1, min(h, 10) - 1, min(20 * i + 19, w - 1)].tolist() == list(c)


def test_quantize_host_rule():
    from anystereo.harness.images import quantize_host
    v = torch.tensor([0.0, 1.0, -0.2, 1.7, 0.5, 127.4999 / 255, 127.5 / 255, float("nan"), float("inf"), float("-inf"), -0.0, 1e-8])
    assert torch.equal(quantize_host(v)[:5], torch.tensor([0, 255, 0, 255, 128], dtype=torch.uint8))
    assert quantize_host(v)[7:].tolist() == [0, 255, 0, 0, 0]
    fin = v[:7]
    assert torch.equal(quantize_host(fin), _quantize_like_save_image(fin))


def test_encode16_host():
    from anystereo.harness.images import decode16, encode16_host
    g = torch.Generator().manual_seed(3)
    d = torch.rand(4000, generator=g) * 255.9
    enc = encode16_host(d)
    assert enc.dtype == torch.uint8 and tuple(enc.shape) == (4000, 2)
    back = torch.from_numpy(decode16(enc.numpy()))
    assert ((back - d).abs() <= 1.0 / 512).all()
    # clamps, NaN, ties to even, byte order
    s = torch.tensor([-3.0, float("-inf"), 0.0, 255.998046875, 256.0, 1e9, float("inf"), float("nan"), 0.001953125, 0.005859375, 1.0, 1.00390625])
    n = (encode16_host(s)[:, 0].int() << 8) | encode16_host(s)[:, 1].int()
    assert n.tolist() == [0, 0, 0, 65535, 65535, 65535, 65535, 0, 0, 2, 256, 257]
    assert encode16_host(torch.tensor([1.00390625])).tolist() == [[1, 1]] and encode16_host(torch.tensor([1.0])).tolist() == [[1, 0]]
    assert tuple(encode16_host(torch.zeros(2, 3, 5)).shape) == (2, 3, 5, 2)


@pytest.mark.parametrize("hw", [(1, 1), (7, 5), (13, 37)])
@pytest.mark.parametrize("c", [3, 2])
def test_png_round_trip(tmp_path, hw, c):
    from anystereo.harness.images import read_png, write_png
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w + c)
    a = torch.randint(0, 256, (h, w, c), generator=g, dtype=torch.uint8)
    path = write_png(str(tmp_path / "a.png"), a)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    assert data[24] == (8 if c == 3 else 16) and data[25] == (2 if c == 3 else 0)  # bit depth, colour type
    back = read_png(path)
    assert back.dtype == np.uint8 and back.shape == (h, w, c) and np.array_equal(back, a.numpy())
    assert np.array_equal(read_png(write_png(str(tmp_path / "b.png"), a.numpy())), a.numpy())  # numpy in
    # a flipped byte anywhere in the image data or the header fails a CRC
    for at in (20, len(data) - 20):
        bad = bytearray(data)
        bad[at] ^= 0x40
        open(str(tmp_path / "bad.png"), "wb").write(bytes(bad))
        with pytest.raises(ValueError, match="CRC"):
            read_png(str(tmp_path / "bad.png"))


@pytest.mark.parametrize("c", [3, 2])
def test_png_is_read_by_another_decoder(tmp_path, c):
    """PIL, where it is installed, decodes the files to the same arrays."""
    Image = pytest.importorskip("PIL.Image")
    from anystereo.harness.images import write_png
    a = torch.randint(0, 256, (13, 37, c), generator=torch.Generator().manual_seed(c), dtype=torch.uint8)
    im = np.asarray(Image.open(write_png(str(tmp_path / "a.png"), a)))
    if c == 3:
        assert np.array_equal(im, a.numpy())
    else:
        assert np.array_equal(im.astype(np.uint16), (a[..., 0].to(torch.int32) << 8 | a[..., 1].to(torch.int32)).numpy().astype(np.uint16))


def test_write_png_refuses_other_arrays(tmp_path):
    from anystereo.harness.images import read_png, write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match="write_png"):
            write_png(str(tmp_path / "x.png"), bad)
    open(str(tmp_path / "n.png"), "wb").write(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        read_png(str(tmp_path / "n.png"))


def test_abi_argument_validation_without_gpu():
    """Every refusal of as_disp_images comes before the launch, so no GPU is needed: AS_ERR_BAD_ARG (-1) for a NULL disp, no output,
    error without gt, a non-positive size, a threshold that is not finite and positive, an output off a 4-byte boundary;
    AS_ERR_BAD_SHAPE (-2) above 2^31-1 output bytes."""
    from anystereo import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    lib = _lib.load()
    assert lib.as_abi_version() == 38
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    p, null = ctypes.c_void_p(base), ctypes.c_void_p(0)
    inf, nan = float("inf"), float("nan")

    def call(disp=p, gt=p, color=p, error=p, enc16=p, b=1, h=4, w=4, md=192.0, at=3.0, rt=0.05):
        return lib.as_disp_images(disp, gt, color, error, enc16, b, h, w, md, at, rt, null)

    assert call(disp=null) == -1
    assert b"disp_images" in lib.as_last_error_string()
    assert call(color=null, error=null, enc16=null) == -1
    assert b"disp_images" in lib.as_last_error_string()
    assert call(gt=null) == -1                      # error requested without gt
    assert b"disp_images" in lib.as_last_error_string()
    for size in ({"b": 0}, {"h": 0}, {"w": 0}, {"b": -1}, {"h": -3}, {"w": -4}):
        assert call(**size) == -1, size
    for name in ("md", "at", "rt"):
        for v in (0.0, -1.0, inf, -inf, nan):
            assert call(**{name: v}) == -1, (name, v)
            assert b"disp_images" in lib.as_last_error_string()
    for off in (1, 2, 3):
        q = ctypes.c_void_p(base + off)
        assert call(color=q) == -1 and call(error=q) == -1 and call(enc16=q) == -1, off
        assert call(color=q, error=null, enc16=null) == -1 and call(gt=null, color=null, error=null, enc16=q) == -1
        assert b"disp_images" in lib.as_last_error_string()
    # 3 * B * H * W = 2^31 + 1 and far above; B * H * W itself beyond 32 bits
    assert call(b=1, h=1, w=715827883) == -2
    assert b"disp_images" in lib.as_last_error_string()
    assert call(b=3, h=46341, w=46341) == -2
    assert call(b=65536, h=65536, w=4) == -2
    assert call(color=null, error=null, b=2, h=32768, w=16384) == -2  # the bound is on the pixel count, whichever outputs are asked for


def test_op_refuses_cpu_tensors_and_bad_arguments_before_the_device():
    from anystereo import ops
    z = torch.zeros(1, 4, 4)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_images(z)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.disparity_images_out(z, None, torch.zeros(1, 4, 4, 3, dtype=torch.uint8), None, None)


class _Stub(torch.nn.Module):
    """Returns the pair's known disparity plus seeded noise, in the models' test_mode output shape [B,1,Q]."""

    def __init__(self, gts):
        super().__init__()
        self.gts, self.at, self.preds = gts, 0, []

    def forward(self, i1, i2, iters=0, test_mode=True, hr_coord=None, scale=None):
        gt = self.gts[self.at]
        self.at += 1
        g = torch.Generator().manual_seed(900 + self.at)
        pred = (gt + (torch.rand(gt.shape, generator=g) - 0.5) * 8.0).reshape(gt.shape[0], 1, -1)
        self.preds.append(pred)
        return pred


def _cpu_pairs():
    pairs = []
    for i, bs in enumerate((1, 2, 1)):
        g = torch.Generator().manual_seed(40 + i)
        h, w = 12, 40
        gt = torch.rand(bs, h, w, generator=g) * 60.0 - 6.0
        pairs.append((torch.rand(bs, 3, h, w, generator=g) * 255.0, torch.rand(bs, 3, h, w, generator=g) * 255.0, gt,
                      torch.ones(bs, h, w), torch.ones(bs, h, w, dtype=torch.uint8)))
    return pairs


def test_evaluate_with_image_sink_on_cpu(tmp_path):
    from anystereo.harness import images as I
    from anystereo.harness.evaluate import evaluate
    pairs = _cpu_pairs()
    plain = evaluate(_Stub([p[2] for p in pairs]), pairs, scale=1.0, iters=1, protocol="kitti")
    assert set(plain) == {"all", "noc", "occ", "images", "pairs", "seconds", "pairs_per_s"}

    stub = _Stub([p[2] for p in pairs])
    sink = I.ImageSink(str(tmp_path / "all"), enc16=True)
    res = evaluate(stub, pairs, scale=1.0, iters=1, protocol="kitti", images=sink)
    assert set(res) == set(plain) | {"images_written"} and res["images_written"] == 12 and res["pairs"] == 4
    for key in ("all", "noc", "occ", "images", "pairs"):
        assert res[key] == plain[key], key  # the sink changes no number
    assert sorted(os.listdir(str(tmp_path / "all"))) == sorted(f"{kind}_{i:06d}.png" for kind in ("disp", "error", "disp16") for i in range(4))
    est = torch.cat([p.reshape(-1, 12, 40) for p in stub.preds])
    gt = torch.cat([p[2] for p in pairs])
    want = {"disp": I.quantize_host(I.disp_to_color_host(est, 192.0)), "error": I.quantize_host(I.error_image_host(est, gt)),
            "disp16": I.encode16_host(est)}
    for kind, w in want.items():
        for i in range(4):
            assert np.array_equal(I.read_png(str(tmp_path / "all" / f"{kind}_{i:06d}.png")), w[i].numpy()), (kind, i)
    assert sink.flush() == []  # nothing is written twice

    # limit: three images of the four, the middle batch taken whole; colour only
    sink = I.ImageSink(str(tmp_path / "some"), error=False, limit=3)
    res = evaluate(_Stub([p[2] for p in pairs]), pairs, scale=1.0, iters=1, protocol="kitti", images=sink)
    assert res["images_written"] == 3 and sink.taken == 3
    assert sorted(os.listdir(str(tmp_path / "some"))) == [f"disp_{i:06d}.png" for i in range(3)]
    sink = I.ImageSink(str(tmp_path / "two"), limit=2)
    assert sink.add(est[:1], gt[:1]) == 1 and sink.add(est[1:], gt[1:]) == 1 and sink.add(est, gt) == 0
    assert sorted(os.path.basename(p) for p in sink.flush()) == ["disp_000000.png", "disp_000001.png", "error_000000.png", "error_000001.png"]


def test_image_sink_names_and_missing_gt(tmp_path):
    from anystereo.harness import images as I
    est = torch.rand(2, 5, 9) * 100
    sink = I.ImageSink(str(tmp_path), max_disp=400.0)
    assert sink.add(est, names=["left_a", "left_b"]) == 2  # no gt: no error map
    paths = sink.flush()
    assert sorted(os.path.basename(p) for p in paths) == ["disp_left_a.png", "disp_left_b.png"]
    assert np.array_equal(I.read_png(str(tmp_path / "disp_left_b.png")), I.quantize_host(I.disp_to_color_host(est, 400.0))[1].numpy())
    with pytest.raises(ValueError, match="names"):
        sink.add(est, names=["one"])
    with pytest.raises(ValueError, match="does not match"):
        sink.add(est, torch.zeros(2, 5, 8))
    with pytest.raises(ValueError, match="no picture"):
        I.ImageSink(str(tmp_path), color=False, error=False)
    # an error-only sink without gt writes nothing: such a batch neither counts against the limit nor uses up a default name
    sink = I.ImageSink(str(tmp_path / "err"), color=False, limit=2)
    assert sink.add(est) == 0 and sink.taken == 0 and sink.flush() == []
    assert sink.add(est, est + 1.0) == 2 and sink.taken == 2
    assert sorted(os.path.basename(p) for p in sink.flush()) == ["error_000000.png", "error_000001.png"]
