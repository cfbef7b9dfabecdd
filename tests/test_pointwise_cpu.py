"""CPU: which descriptors the streaming 1x1 convolution accepts (as_conv1x1_stream_ok: host arithmetic, no device) and which
shapes ops.conv1x1 routes to it (ops.pw_stream_route, ANYSTEREO_PW_STREAM)."""
import ctypes as C
import inspect

import pytest

from anystereo import _lib as L
from anystereo import ops

FAKE = 1 << 20  # _ok never dereferences a data pointer

# the pointwise layers of the cfg-2 pre-loop whose launches as_conv2d does not split over K: (Cin, Cout, B, H, W)
TABLE = [(16, 96, 2, 272, 480), (32, 16, 2, 272, 480), (64, 96, 1, 272, 480), (24, 144, 2, 136, 240), (96, 96, 2, 136, 240),
         (32, 16, 1, 1, 195840), (144, 24, 2, 136, 240), (96, 128, 1, 136, 240), (96, 48, 1, 136, 240), (96, 24, 2, 136, 240),
         (48, 8, 1, 136, 240), (32, 192, 2, 68, 120), (192, 32, 2, 68, 120), (144, 32, 2, 68, 120), (128, 128, 1, 68, 120)]


def desc(cin, cout, b, h, w, ks=1, srcs=None, **kw):
    """The descriptor ops.conv1x1 builds for a split-precision call (with the split-K scratch ops.conv2d would hand as_conv2d)."""
    lib = L.load()
    d = L.ConvDesc()
    for i, c in enumerate(srcs or [cin]):
        d.src[i], d.src_c[i] = FAKE, c
    d.n_src = len(srcs or [cin])
    d.wpack = d.out = FAKE
    d.out_ctot = cout
    d.B, d.H, d.W, d.Cin, d.Cout, d.KS = b, h, w, cin, cout, ks
    d.stride, d.act, d.epilogue, d.precision = 1, L.ACT_NONE, L.EPI_LINEAR, 1
    n_ws = lib.as_conv_ws_elems(b, cout, h, w)
    if n_ws > 0:
        d.ws, d.ws_elems = FAKE, n_ws
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def ok(d) -> bool:
    return bool(L.load().as_conv1x1_stream_ok(C.byref(d)))


@pytest.mark.parametrize("shape", TABLE, ids=lambda s: "%dto%d_%dx%dx%d" % s)
def test_ok_accepts_the_pre_loop_shapes(shape):
    d = desc(*shape)
    assert ops.conv_plan(d)["ksplit"] == 1
    assert ok(d)


def test_ok_accepts_sources_on_chunk_boundaries():
    assert ok(desc(48, 48, 1, 68, 120, srcs=[32, 16]))
    assert ok(desc(20, 8, 1, 5, 33))  # a last chunk that is partly padding


def test_ok_rejects():
    base = (32, 48, 2, 136, 240)
    assert ok(desc(*base))
    assert not ok(desc(*base, ks=3)), "3x3"
    assert not ok(desc(*base, ks=3, stride=2)), "stride 2"
    assert not ok(desc(*base, stride=2)), "stride 2 (as_conv2d's own validation)"
    blocked = desc(*base)
    blocked.src_bs[0] = 1
    assert not ok(blocked), "a blocked source"
    assert not ok(desc(*base, out_bs=FAKE, out_bs_ctot=48)), "a blocked result"
    assert not ok(desc(*base, dual=1, src2=FAKE, wpack2=FAKE, out_ctot=96, out_coff2=48)), "a dual launch"
    gru = desc(*base, epilogue=L.EPI_GRU_Q, z=FAKE)
    gru.h = FAKE
    assert not ok(gru), "another epilogue"
    assert not ok(desc(*base, precision=0)), "fp32 precision"
    assert not ok(desc(40, 48, 2, 136, 240, srcs=[24, 16])), "a first source of 24 channels"
    assert not ok(desc(160, 96, 2, 136, 240)), "Cin above 128 with Cout above 64"
    assert ok(desc(160, 64, 2, 136, 240)) and ok(desc(128, 96, 2, 136, 240))
    assert not ok(desc(96, 576, 2, 136, 240)), "a weight image above 80 KB"
    assert ok(desc(64, 192, 2, 136, 240))
    lib = L.load()
    prev = lib.as_get_fast16()
    lib.as_set_fast16(1)
    try:
        assert not ok(desc(*base)), "fast16"
    finally:
        lib.as_set_fast16(prev)
    assert ok(desc(*base))


@pytest.mark.parametrize("shape", [(960, 160, 2, 17, 30), (256, 32, 1, 17, 30)], ids=["960to160", "256to32_inside_the_limits"])
def test_ok_rejects_a_k_split_launch(shape):
    d = desc(*shape)
    assert ops.conv_plan(d)["ksplit"] > 1
    assert not ok(d)
    d.ws, d.ws_elems = 0, 0  # without scratch as_conv2d cannot split K
    assert ops.conv_plan(d)["ksplit"] == 1
    assert ok(d) == (shape[1] <= 64)  # 960 -> 160: Cin above 128 with Cout above 64


def test_route_is_a_pure_function_of_the_shape():
    assert list(inspect.signature(ops.pw_stream_route).parameters) == ["cin", "cout", "pixels"]
    shapes = [(cin, cout, b * h * w) for cin, cout, b, h, w in TABLE] + [(960, 160, 1020), (1, 1, 1), (128, 128, 2040)]
    first = [ops.pw_stream_route(*s) for s in shapes]
    assert all(isinstance(r, bool) for r in first)
    assert first == [ops.pw_stream_route(*s) for s in reversed(shapes)][::-1]  # no state, no order dependence
    assert any(first), "the rule routes the large-map layers it was measured on"
    assert not ops.pw_stream_route(960, 160, 1020)  # the small maps stay on as_conv2d


def test_knob_zero_routes_nothing(monkeypatch):
    """ANYSTEREO_PW_STREAM=0: ops.conv1x1 hands every call to ops.conv2d before it looks at the shape."""
    calls = []
    monkeypatch.setattr(ops, "conv2d", lambda srcs, pack, **k: calls.append(k) or "conv2d")
    monkeypatch.setattr(ops, "pw_stream_route", lambda *a: calls.append("route") or True)

    class Pack:
        split, ks, cin, cout = True, 1, 16, 96

    class Src:  # conv1x1 must not touch the tensor either
        shape = (2, 16, 272, 480)

    monkeypatch.setenv("ANYSTEREO_PW_STREAM", "0")
    assert ops.conv1x1([Src()], Pack(), act=L.ACT_RELU6) == "conv2d"
    assert calls == [{"act": L.ACT_RELU6, "add": None, "add_coff": 0, "out": None, "out_coff": 0, "h": None}]
