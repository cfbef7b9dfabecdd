"""Photometric augmentation without a GPU: the numpy restatement (anystereo/harness/augment.py) against the committed PIL fixture and,
where PIL can be imported, against PIL itself on every input; the integer forms of the two means on ties; draw_params; the
library's binding and every refusal of aug_photometric_pair with host-side arguments (a refused call launches nothing, so it needs
no device).  All comparisons are byte equality.
"""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import _augment_cases as K
from _headers import declared_symbols
from anystereo.harness import augment as A


# ---- the fixture ---------------------------------------------------------------------------------------------------------------

def test_host_equals_the_pil_fixture():
    sets = K.fixture_sets()
    assert len(sets) >= 40
    orders = {sp[0].image1.order for _, _, _, sp, _, _, _ in sets}
    assert len(orders) == 24
    for name, i1, i2, sp, lut, o1, o2 in sets:
        g1, g2 = A.photometric_pair_host(i1, i2, sp, gamma_lut=lut)
        assert g1.dtype == torch.uint8 and torch.equal(g1, o1) and torch.equal(g2, o2), (name, sp[0])
        f1, f2 = A.photometric_pair_host(i1.float(), i2.float(), sp, out_dtype=torch.float32, gamma_lut=lut)
        assert f1.dtype == torch.float32 and torch.equal(f1, o1.float()) and torch.equal(f2, o2.float()), name


def test_fp32_inputs_are_quantised_once():
    i1, i2 = K.random_pair(1, 7, 9, 3)
    noise = (torch.rand(i1.shape, generator=torch.Generator().manual_seed(1)) - 0.5) * 0.98
    sp = K.mixed_params(1, 7, 9)
    want = A.photometric_pair_host(i1, i2, sp)
    got = A.photometric_pair_host(i1.float() + noise, i2.float() - noise, sp)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    lo, hi = torch.full((1, 3, 7, 9), -3.0), torch.full((1, 3, 7, 9), 300.0)
    ident = [A.SampleParams()]
    got = A.photometric_pair_host(lo, hi, ident)
    assert bool((got[0] == 0).all()) and bool((got[1] == 255).all())


# ---- against PIL itself, exhaustively ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def colours():
    v = np.arange(1 << 24, dtype=np.int32).reshape(4096, 4096)
    return v >> 16, (v >> 8) & 255, v & 255


def _pil_image(colours, mode):
    Image = pytest.importorskip("PIL.Image")
    return Image.fromarray(np.stack(colours, -1).astype(np.uint8), mode)


def test_rgb_to_hsv_equals_pil_on_every_colour(colours):
    want = np.array(_pil_image(colours, "RGB").convert("HSV"))
    for c, got in enumerate(A.rgb_to_hsv(*colours)):
        assert np.array_equal(got, want[..., c]), "HSV"[c]


def test_hsv_to_rgb_equals_pil_on_every_colour(colours):
    want = np.array(_pil_image(colours, "HSV").convert("RGB"))
    for c, got in enumerate(A.hsv_to_rgb(*colours)):
        assert np.array_equal(got, want[..., c]), "RGB"[c]


def test_grey_equals_pil_on_every_colour(colours):
    want = np.array(_pil_image(colours, "RGB").convert("L"))
    assert np.array_equal(A.grey(*colours), want)


@pytest.mark.parametrize("f", [0, 0.25, 0.6, 1, 1.17, 1.4, 2])
def test_blend_equals_the_enhancers_on_every_value_and_level(f):
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    x, d = np.meshgrid(np.arange(256), np.arange(256))   # [level, value]
    want = np.array(Image.blend(Image.fromarray(d.astype(np.uint8), "L"), Image.fromarray(x.astype(np.uint8), "L"), f))
    assert np.array_equal(blend_u8(x, d, f), want)
    # the three enhancers are that blend: brightness with level 0, saturation with the pixel's grey, contrast with int(mean + 0.5)
    rgb = np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    im = Image.fromarray(rgb)
    r, g, b = (rgb[..., c].astype(np.int32) for c in range(3))
    l = A.grey(r, g, b)
    m = A.contrast_level(int(l.sum()), l.size)
    for enh, level in ((ImageEnhance.Brightness, 0), (ImageEnhance.Color, l), (ImageEnhance.Contrast, m)):
        want = np.array(enh(im).enhance(f))
        got = np.stack([blend_u8(c, level, f) for c in (r, g, b)], -1)
        assert np.array_equal(got, want), enh.__name__


def blend_u8(x, d, f):
    return A.blend(x, d, float(np.float32(f))).astype(np.uint8)


@pytest.mark.parametrize("gamma,gain", [(0.8, 1.0), (1.2, 1.3), (2.0, 0.9)])
def test_gamma_table_equals_image_point(gamma, gain):
    Image = pytest.importorskip("PIL.Image")
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    raw = [int((255 + 1 - 1e-3) * gain * pow(e / 255.0, gamma)) for e in range(256)]   # adjust_gamma's list, entries above 255 included
    want = np.array(Image.fromarray(ramp).point(raw * 3))[0, :, 0]
    p = A.ImageParams(gamma=gamma, gain=gain)
    lut = A.gamma_table([A.SampleParams(p, p)])
    assert lut.shape == (1, 2, 256) and np.array_equal(lut[0, 0], want) and np.array_equal(lut[0, 1], want)
    if gain > 1:
        assert max(raw) > 255 and int(want.max()) == 255   # Image.point clips its table, it neither wraps nor raises


# ---- the two means in integers -------------------------------------------------------------------------------------------------

def _tie_cases():
    ns = [1, 2, 3, 7, 8, 24 * 40, 37 * 53, 2 * 37 * 53, 160 * 320, 2 * 160 * 320, 540 * 960, 2 * 540 * 960, 2 * 540 * 960 - 1]
    for n in ns:
        for k in (0, 1, 100, 127, 254):
            base = k * n
            for s in {base, base + n // 2, base + n // 2 + 1, base + (n + 1) // 2, max(base + n // 2 - 1, 0), base + n - 1, base + 1}:
                if s <= 255 * n:
                    yield s, n
        yield 255 * n, n


def test_integer_means_equal_the_float_ones_on_ties_and_near_ties():
    ties = 0
    for s, n in _tie_cases():
        assert A.contrast_level(s, n) == int(s / n + 0.5), (s, n)            # ImageEnhance.Contrast: int(Stat.mean[0] + 0.5)
        assert s // n == int(np.float64(s) / np.float64(n)), (s, n)         # numpy's float64 mean stored into uint8
        ties += (2 * s) % (2 * n) == n
    assert ties >= 20   # exact k + 0.5 means were among them
    # and through the images: a pair whose stacked mean grey is exactly 119.5, and a channel mean of exactly k + 1/2
    a = torch.full((1, 3, 2, 4), 119, dtype=torch.uint8)
    b = torch.full((1, 3, 2, 4), 120, dtype=torch.uint8)
    sp = [A.SampleParams(A.ImageParams(contrast=0.0), A.ImageParams(contrast=0.0), shared=True, rects=((0, 0, 1, 1),))]
    o1, o2 = A.photometric_pair_host(a, b, sp)
    assert bool((o1 == 120).all()) and bool((o2 == 120).all())
    b2 = b.clone()
    b2[0, :, 0, :] = 121                                  # channel mean 120.5 -> the rectangle holds 120
    ident = [A.SampleParams(rects=((3, 1, 9, 9),))]
    _, o2 = A.photometric_pair_host(a, b2, ident)
    assert int(o2[0, 0, 1, 3]) == 120 and torch.equal(o2[0, :, 0], b2[0, :, 0])


# ---- draw_params ---------------------------------------------------------------------------------------------------------------

def test_draw_params_is_a_function_of_its_inputs():
    spec = A.PhotoSpec.flow()
    a, b = A.draw_params(spec, 7, 100, 16, 160, 320), A.draw_params(spec, 7, 100, 16, 160, 320)
    assert a == b
    assert A.draw_params(spec, 7, 108, 8, 160, 320) == a[8:]                 # a sample is (seed, index), whatever batch holds it
    assert A.draw_params(spec, 8, 100, 16, 160, 320) != a


@pytest.mark.parametrize("name", ["flow", "sparse"])
def test_draw_params_ranges_and_shares(name):
    spec = getattr(A.PhotoSpec, name)(gamma=(0.8, 1.2, 0.9, 1.1))
    n, h, w = 2000, 160, 320
    ps = A.draw_params(spec, 3, 0, n, h, w)
    f32 = lambda v: float(np.float32(v))  # noqa: E731
    lo_shift, hi_shift = spec.hue[0] * 255, spec.hue[1] * 255
    for sp in ps:
        sp.validate(h, w)
        assert sp.image1 == sp.image2 or not sp.shared
        for p in (sp.image1, sp.image2):
            for rng, v in ((spec.brightness, p.brightness), (spec.contrast, p.contrast), (spec.saturation, p.saturation)):
                assert f32(rng[0]) <= v <= f32(rng[1])
            signed = p.hue_shift if p.hue_shift < 128 else p.hue_shift - 256
            assert math.trunc(lo_shift) <= signed <= math.trunc(hi_shift)
            assert spec.gamma[0] <= p.gamma <= spec.gamma[1] and spec.gamma[2] <= p.gain <= spec.gamma[3]
        assert len(sp.rects) <= 2
        for x0, y0, dx, dy in sp.rects:
            assert 0 <= x0 < w and 0 <= y0 < h and 50 <= dx < 100 and 50 <= dy < 100
    assert len({sp.image1.order for sp in ps}) == 24
    for share, prob in ((sum(not sp.shared for sp in ps) / n, spec.asymmetric_prob), (sum(bool(sp.rects) for sp in ps) / n, spec.eraser_prob)):
        assert abs(share - prob) <= 4 * math.sqrt(prob * (1 - prob) / n), (share, prob)
    erased = [sp for sp in ps if sp.rects]
    assert {len(sp.rects) for sp in erased} == {1, 2}


def test_the_constructors_carry_the_reference_constants():
    f, s = A.PhotoSpec.flow(), A.PhotoSpec.sparse()
    assert (f.brightness, f.contrast, f.saturation, f.asymmetric_prob, f.eraser_prob, f.eraser_bounds) == ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), 0.2, 0.5, (50, 100))
    assert f.hue == (-0.5 / 3.14, 0.5 / 3.14) and s.hue == (-0.3 / 3.14, 0.3 / 3.14)
    assert (s.brightness, s.contrast, s.saturation, s.asymmetric_prob, s.eraser_prob) == ((0.7, 1.3), (0.7, 1.3), (0.7, 1.3), 0.0, 0.5)
    assert not f.has_gamma and A.PhotoSpec.flow(gamma=(0.8, 1.2, 1, 1)).has_gamma
    assert A.hue_shift_of(0.1) == 25 and A.hue_shift_of(-0.1) == 231 and A.hue_shift_of(0.0) == 0


# ---- the library ---------------------------------------------------------------------------------------------------------------

def test_library_loads_and_binds_every_symbol_of_the_header():
    import os
    from anystereo import _augment_lib as L
    lib = L.load()
    assert lib.aug_abi_version() == 1
    info = L.library_info()
    assert info["matches_sources"] is True and info["abi"] == 1
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "anystereo_augment.h")).read()
    declared = declared_symbols("augment")
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    assert set(L.LAUNCHING) == {"aug_photometric_pair"}
    for h, w in ((3, 5), (160, 320), (540, 960), (4096, 4096)):
        assert lib.aug_workspace_bytes(4, h, w) == A.workspace_bytes(4, h, w)
    assert lib.aug_workspace_bytes(0, 4, 4) == -1
    assert C.sizeof(L.Sample) == 104 and C.sizeof(L.ImageParams) == 32
    for name in ("AUG_MAX_BATCH", "AUG_MAX_RECTS", "AUG_TILE", "AUG_MAX_PARTS"):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == getattr(L, name)
    assert (A.TILE, A.MAX_PARTS, A.MAX_RECTS) == (L.AUG_TILE, L.AUG_MAX_PARTS, L.AUG_MAX_RECTS)


def _host_call(lib, **kw):
    """aug_photometric_pair with HOST buffers and one change: only for calls that must be refused (a refusal precedes any launch)."""
    from anystereo import _augment_lib as L
    B, h, w = kw.get("B", 2), kw.get("h", 8), kw.get("w", 16)
    bufs = kw["bufs"]
    a = {"image1": bufs["in1"].ctypes.data, "image2": bufs["in2"].ctypes.data, "in_dtype": L.AUG_U8, "out1": bufs["out1"].ctypes.data,
         "out2": bufs["out2"].ctypes.data, "out_dtype": L.AUG_U8, "B": B, "h": h, "w": w, "samples": A.c_samples([A.SampleParams()] * 2),
         "gamma_lut": None, "workspace": bufs["ws"].ctypes.data, "workspace_bytes": bufs["ws"].nbytes, "stream": None}
    a.update({k: v for k, v in kw.items() if k in a})
    return lib.aug_photometric_pair(*a.values())


def test_every_refusal_returns_its_code_and_a_message():
    from anystereo import _augment_lib as L
    lib = L.load()
    n = 2 * 3 * 8 * 16
    bufs = {k: np.zeros(n * 4, dtype=np.uint8)[:n] for k in ("in1", "in2", "out1", "out2")}   # room for the fp32 cases
    big = {k: np.zeros(n * 4 + 8, dtype=np.uint8) for k in ("in1", "in2", "out1", "out2")}
    bufs["ws"] = np.zeros(2 * 5, dtype=np.uint64)
    base = lambda k: big[k].ctypes.data + (-big[k].ctypes.data) % 8  # noqa: E731

    def sample(**kw):
        s = A.c_samples([A.SampleParams(), A.SampleParams()])
        for k, v in kw.items():
            if k == "order":
                s[1].img[1].order[:] = v
            elif k == "factor":
                s[1].img[0].factor[1] = v
            elif k == "hue":
                s[1].img[1].hue_shift = v
            elif k == "n_rects":
                s[1].n_rects = v
            elif k == "rect":
                s[1].n_rects = 1
                s[1].rect[0][:] = v
            elif k == "shared":
                s[1].shared = v
        return s

    cases = [
        ("null image", dict(image1=None), L.AUG_ERR_BAD_ARG),
        ("null output", dict(out2=None), L.AUG_ERR_BAD_ARG),
        ("null samples", dict(samples=None), L.AUG_ERR_BAD_ARG),
        ("null workspace", dict(workspace=None), L.AUG_ERR_BAD_ARG),
        ("dtype", dict(in_dtype=2), L.AUG_ERR_BAD_ARG),
        ("misaligned fp32 input", dict(image1=base("in1") + 2, image2=base("in2"), in_dtype=L.AUG_F32), L.AUG_ERR_BAD_ARG),
        ("misaligned fp32 output", dict(out1=base("out1"), out2=base("out2") + 1, out_dtype=L.AUG_F32), L.AUG_ERR_BAD_ARG),
        ("misaligned workspace", dict(workspace=bufs["ws"].ctypes.data + 4), L.AUG_ERR_BAD_ARG),
        ("B = 0", dict(B=0), L.AUG_ERR_BAD_ARG),
        ("h < 0", dict(h=-8), L.AUG_ERR_BAD_ARG),
        ("w = 0", dict(w=0), L.AUG_ERR_BAD_ARG),
        ("2^31 elements", dict(h=1 << 15, w=1 << 15), L.AUG_ERR_BAD_SHAPE),
        ("2^31 elements, large B", dict(B=1 << 30, h=1 << 20, w=1 << 20), L.AUG_ERR_BAD_SHAPE),
        ("order repeats", dict(samples=sample(order=(0, 1, 1, 3))), L.AUG_ERR_BAD_ARG),
        ("order out of range", dict(samples=sample(order=(0, 1, 2, 4))), L.AUG_ERR_BAD_ARG),
        ("negative factor", dict(samples=sample(factor=-0.5)), L.AUG_ERR_BAD_ARG),
        ("factor nan", dict(samples=sample(factor=float("nan"))), L.AUG_ERR_BAD_ARG),
        ("factor inf", dict(samples=sample(factor=float("inf"))), L.AUG_ERR_BAD_ARG),
        ("hue 256", dict(samples=sample(hue=256)), L.AUG_ERR_BAD_ARG),
        ("hue -1", dict(samples=sample(hue=-1)), L.AUG_ERR_BAD_ARG),
        ("three rectangles", dict(samples=sample(n_rects=3)), L.AUG_ERR_BAD_ARG),
        ("empty rectangle", dict(samples=sample(rect=(1, 1, 0, 4))), L.AUG_ERR_BAD_ARG),
        ("negative extent", dict(samples=sample(rect=(1, 1, 4, -1))), L.AUG_ERR_BAD_ARG),
        ("origin right of the frame", dict(samples=sample(rect=(16, 1, 4, 4))), L.AUG_ERR_BAD_ARG),
        ("origin below the frame", dict(samples=sample(rect=(1, 8, 4, 4))), L.AUG_ERR_BAD_ARG),
        ("negative origin", dict(samples=sample(rect=(-1, 1, 4, 4))), L.AUG_ERR_BAD_ARG),
        ("shared = 2", dict(samples=sample(shared=2)), L.AUG_ERR_BAD_ARG),
        ("small workspace", dict(workspace_bytes=2 * 5 * 8 - 1), L.AUG_ERR_WORKSPACE),
        ("out1 is image1", dict(out1=bufs["in1"].ctypes.data), L.AUG_ERR_ALIAS),
        ("out2 inside image1", dict(out2=bufs["in1"].ctypes.data + n - 1), L.AUG_ERR_ALIAS),
        ("out1 overlaps out2", dict(out2=bufs["out1"].ctypes.data + 5), L.AUG_ERR_ALIAS),
        ("out is the workspace", dict(out1=bufs["ws"].ctypes.data), L.AUG_ERR_ALIAS),
    ]
    for what, change, code in cases:
        rc = _host_call(lib, bufs=bufs, **change)
        msg = lib.aug_last_error_string().decode()
        assert rc == code, (what, rc, msg)
        assert msg.startswith("aug_photometric_pair") and len(msg) > 25, (what, msg)
    assert all(not b.any() for b in bufs.values())   # and none of them touched a buffer


def test_python_refuses_before_the_library():
    i1, i2 = K.random_pair(1, 4, 6, 0)
    with pytest.raises(ValueError, match="permutation"):
        A.photometric_pair(i1, i2, [A.SampleParams(A.ImageParams(order=(0, 0, 1, 2)))])
    with pytest.raises(ValueError, match="rectangle"):
        A.photometric_pair(i1, i2, [A.SampleParams(rects=((6, 0, 1, 1),))])
    with pytest.raises(ValueError, match="parameter sets"):
        A.photometric_pair(i1, i2, [])
    with pytest.raises(TypeError):
        A.photometric_pair(i1.double(), i2.double(), [A.SampleParams()])
    # CPU tensors run the restatement.  Factors of 1 and a shift of 0 still send every pixel through PIL's HSV bytes and back, as
    # ColorJitter does: only greys are sure to return unchanged
    o1, o2 = A.photometric_pair(i1, i2, [A.SampleParams()])
    w1, w2 = A.photometric_pair_host(i1, i2, [A.SampleParams()])
    assert torch.equal(o1, w1) and torch.equal(o2, w2)
    g1 = i1[:, :1].expand(-1, 3, -1, -1).contiguous()
    o1, _ = A.photometric_pair(g1, i2, [A.SampleParams()])
    assert torch.equal(o1, g1)
