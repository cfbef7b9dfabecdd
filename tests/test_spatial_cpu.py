"""Spatial augmentation without a GPU (anystereo/harness/spatial.py, libanystereo_spatial.so's host side): the numpy restatement
against the committed fixture of the reference's own augmentor classes, the fp32 linear resize against fp64, the parameter draws,
and the library's validation.  Nothing here reads the reference or needs cv2."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _spatial_cases as K
from anystereo.harness import spatial as SP

EPS = 8 * 2.0 ** -24          # the limit low_disp_host's test uses: a handful of fp32 roundings of values bounded by max|v|


# ---- the restatement == the reference's composition ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", K.fixture_cases(), ids=[c[0] for c in K.fixture_cases()])
def test_host_equals_the_reference_fixture(case):
    name, im1, im2, disp, valid, params, out_size, want = case
    # spatial_transform's outputs: the crop itself
    o1, o2, disps, valids = SP.spatial_pair_host(im1, im2, disp, params, valid=valid)
    assert o1.dtype == torch.uint8 and torch.equal(o1[0], want["st1"]), f"{name}: image1"
    assert torch.equal(o2[0], want["st2"]), f"{name}: image2"
    assert disps[0].dtype == torch.float32 and disps[0].shape == want["disp"].shape
    assert torch.equal(K.bits(disps[0]), K.bits(want["disp"])), f"{name}: disparity, {int((K.bits(disps[0]) != K.bits(want['disp'])).sum())} differ"
    if valid is None:
        assert valids is None
    else:
        assert valids[0].dtype == torch.uint8 and torch.equal(valids[0], want["valid"]), f"{name}: validity"
    if out_size is not None:  # the __call__ tail of the *WoCrop classes
        r1, r2, rd, rv = SP.spatial_pair_host(im1, im2, disp, params, valid=valid, out_size=out_size)
        assert torch.equal(r1[0], want["out1"]) and torch.equal(r2[0], want["out2"]), f"{name}: final resize"
        assert torch.equal(K.bits(rd[0]), K.bits(want["disp"]))
        f1, f2, _, _ = SP.spatial_pair_host(im1.float(), im2.float(), disp, params, valid=valid, out_size=out_size, out_dtype=torch.float32)
        assert f1.dtype == torch.float32 and torch.equal(f1[0], want["out1"].float()) and torch.equal(f2[0], want["out2"].float())


def test_fixture_covers_what_it_should():
    cases = K.fixture_cases()
    ps = [c[5][0] for c in cases]
    assert {p.flip for p in ps} == set(SP.FLIPS)
    assert {p.dy2 for p in ps} >= {-2, 0, 2}
    assert {p.rescale for p in ps} == {True, False}
    assert any(p.rescale and p.scale_x < 1 for p in ps) and any(p.rescale and p.scale_x > 1 for p in ps)
    assert any(p.scale_x == 0.8828125 and p.frame(40, 64)[1] == 56 for p in ps)       # 56.5 -> 56: half to even
    assert any(p.scale_x == 0.8 == p.scale_y for p in ps) and any(p.scale_x == 41 / 64 for p in ps)   # clipped at the scale floor
    sparse = [c for c in cases if c[4] is not None]
    assert any(p.scale_x == 1.5 for p in (c[5][0] for c in sparse))                   # scatter ties x * 1.5 = k + 0.5
    origins = {(c[5][0].y0, c[5][0].x0) for c in sparse}
    assert (0, 0) in origins and any(c[5][0].rescale and (c[5][0].y0 + 24, c[5][0].x0 + 40) == c[5][0].frame(40, 64) for c in sparse)
    assert bool(sparse[0][4][0, 0].any()) and bool(sparse[0][4][0, :, 0].any())       # valid pixels in row 0 and column 0
    for c in sparse:                                                                  # ... which a rescale drops
        p, w_ = c[5][0], c[7]
        if p.rescale and p.flip == "none" and p.y0 == 0 and p.x0 == 0:
            assert not bool(w_["valid"][0].any()) and not bool(w_["valid"][:, 0].any())


def test_identity_parameters_return_the_inputs():
    im1, im2, disp, valid = K.random_frames(2, 9, 13, seed=5, sparse=True)
    disp[0, 2, 3], disp[1, 0, 0] = float("inf"), -0.0
    p = [SP.SpatialParams(ch=9, cw=13)] * 2
    o1, o2, ds, vs = SP.spatial_pair_host(im1, im2, disp, p, valid=valid)
    assert torch.equal(o1, im1) and torch.equal(o2, im2)
    assert all(torch.equal(K.bits(d), K.bits(disp[b])) for b, d in enumerate(ds)) and all(torch.equal(v, valid[b]) for b, v in enumerate(vs))


# ---- fp32 against fp64 ----------------------------------------------------------------------------------------------------------

def _linear64(src, fx, fy):
    """The linear resize's formula with the blend in fp64: the taps (i, t) are the formula's own — s is cast to fp32 there, so t is an
    fp32 number and the fp64 evaluation takes it exactly — and the two passes are evaluated in double.  The taps come from
    `SP.lin_axis`, the code under test: this checks the blend's rounding, not the tap rule.  The tap rule's only independent check
    is the fixture, whose maker states it a second time (scalar loops in tests/golden/make_golden_spatial.py)."""
    h, w = src.shape
    y0, y1, ty = SP.lin_axis(np.arange(SP._rint(h * fy)), fy, h)
    x0, x1, tx = SP.lin_axis(np.arange(SP._rint(w * fx)), fx, w)
    s, ty, tx = src.astype(np.float64), ty.astype(np.float64)[:, None], tx.astype(np.float64)
    r0 = s[y0][:, x0] * (1 - tx) + s[y0][:, x1] * tx
    r1 = s[y1][:, x0] * (1 - tx) + s[y1][:, x1] * tx
    return r0 * (1 - ty) + r1 * ty


@pytest.mark.parametrize("scale", [0.87, 1.0, (1.3, 1.17), 2.0, (0.8828125, 1.41), (2 ** 0.5, 2 ** -0.2)], ids=str)
@pytest.mark.parametrize("h,w", [(40, 64), (96, 160)])
def test_linear_resize_against_fp64(h, w, scale):
    fx, fy = scale if isinstance(scale, tuple) else (scale, scale)
    src = np.random.RandomState(h + int(1000 * fx)).randint(0, 256, (h, w)).astype(np.float32)
    v32 = SP.resize_linear_host(src, fx, fy)
    v64 = _linear64(src, fx, fy)
    assert v32.dtype == np.float32 and v32.shape == v64.shape == (SP._rint(h * fy), SP._rint(w * fx))
    bound = EPS * float(np.abs(src).max())
    err = float(np.abs(v32.astype(np.float64) - v64).max())
    window = np.abs((v64 - np.floor(v64)) - 0.5) < EPS * 255
    b32 = np.clip(np.floor(v32 + np.float32(0.5)), 0, 255)
    b64 = np.clip(np.floor(v64 + 0.5), 0, 255)
    share = float(window.mean())
    print(f"{h}x{w} scale {scale}: max |v32 - v64| = {err / (2.0 ** -24 * 255):.2f} * 2^-24 * 255, window {100 * share:.3f} %")
    assert err <= bound
    if scale in (1.0, 2.0):      # dyadic weights, 8-bit values: every fp32 operation is exact
        assert err == 0.0 and np.array_equal(b32, b64)
    else:
        assert np.array_equal(b32[~window], b64[~window])
        assert share <= 0.01


# ---- the draws ------------------------------------------------------------------------------------------------------------------

def test_draw_spatial_is_reproducible_and_valid():
    sizes = [(round(32 * s), round(64 * s)) for s in (1.0, 1.65, 2.3, 2.95)]
    for spec in (SP.SpatialSpec.flow(do_flip="h"), SP.SpatialSpec.sparse(wo_crop=True), SP.SpatialSpec.sparse(do_flip="v")):
        a = SP.draw_spatial(spec, 11, 40, 4, 135, 240, sizes)
        assert a == SP.draw_spatial(spec, 11, 40, 4, 135, 240, sizes)
        assert a[1:] == SP.draw_spatial(spec, 11, 41, 3, 135, 240, sizes[1:])           # a sample depends on its own index alone
        assert a != SP.draw_spatial(spec, 12, 40, 4, 135, 240, sizes)
        for p, (ch, cw) in zip(a, sizes):
            p.validate(135, 240)
            assert (p.ch, p.cw) == (ch, cw)


def _stats(spec, n, h, w, crop):
    ps = SP.draw_spatial(spec, 7, 0, n, h, w, [crop] * n)
    for p in ps:
        p.validate(h, w)
        fh, fw = p.frame(h, w)
        assert 0 <= p.y0 and p.y0 + p.ch <= fh and 0 <= p.x0 and p.x0 + p.cw <= fw and 0 <= p.y0 + p.dy2 and p.y0 + p.dy2 + p.ch <= fh
    return ps


def test_draw_spatial_distributions_flow():
    n, h, w, crop = 4000, 200, 320, (96, 160)
    ps = _stats(SP.SpatialSpec.flow(crop, do_flip="hf", yjitter=True), n, h, w, crop)
    tol = 4 * math.sqrt(0.25 / n)                                                     # four sigma of a frequency
    assert all(p.rescale for p in ps)                                                 # spatial_aug_prob 1.0
    assert abs(np.mean([p.flip == "hf" for p in ps]) - 0.5) < tol and {p.flip for p in ps} == {"none", "hf"}
    assert abs(np.mean([p.scale_x != p.scale_y for p in ps]) - 0.8) < tol             # stretched
    sx = np.array([p.scale_x for p in ps])
    assert 2 ** -0.4 <= sx.min() < 2 ** -0.3 and 2 ** 0.5 < sx.max() <= 2 ** 0.6                  # 2^U(-0.2, 0.4) times 2^U(-0.2, 0.2)
    big = (150, 240)                                                                  # a crop whose scale floor lies inside the range
    floor = max((150 + 8) / 200, (240 + 8) / 320)
    sb = np.array([[p.scale_x, p.scale_y] for p in _stats(SP.SpatialSpec.flow(big), n, h, w, big)])
    assert sb.min() == floor and (sb == floor).any() and (sb == floor).mean() < 0.5 and sb.max() > 2 ** 0.5
    assert {p.dy2 for p in ps} == {-2, -1, 0, 1, 2} and min(p.y0 for p in ps) == 2 and min(p.x0 for p in ps) == 2
    assert abs(np.mean([p.dy2 == 0 for p in ps]) - 0.2) < tol
    ps = _stats(SP.SpatialSpec.flow(crop, do_flip="v", yjitter=False), n, h, w, crop)
    assert abs(np.mean([p.flip == "v" for p in ps]) - 0.1) < tol and {p.dy2 for p in ps} == {0} and min(p.y0 for p in ps) == 0
    assert {p.flip for p in _stats(SP.SpatialSpec.flow(crop), 200, h, w, crop)} == {"none"}


def test_draw_spatial_distributions_sparse():
    n, h, w, crop = 4000, 200, 320, (96, 160)
    tol = 4 * math.sqrt(0.25 / n)
    ps = _stats(SP.SpatialSpec.sparse(crop, do_flip="h"), n, h, w, crop)
    assert abs(np.mean([p.rescale for p in ps]) - 0.8) < tol                          # spatial_aug_prob 0.8
    assert all(p.scale_x == p.scale_y for p in ps) and abs(np.mean([p.flip == "h" for p in ps]) - 0.5) < tol
    floor = max(97 / 200, 161 / 320)
    sx = np.array([p.scale_x for p in ps if p.rescale])
    assert sx.min() >= max(floor, 2 ** -0.2) and sx.max() <= 2 ** 0.4 and all(p.scale_x == 1.0 for p in ps if not p.rescale)
    # the margins: origins pile up at both borders (clipped), far more often than a uniform draw would put them there
    at_lo = np.mean([p.x0 == 0 for p in ps])
    at_hi = np.mean([p.x0 + p.cw == p.frame(h, w)[1] for p in ps])
    assert at_lo > 0.1 and at_hi > 0.1 and np.mean([p.y0 + p.ch == p.frame(h, w)[0] for p in ps]) > 0.05
    ps = _stats(SP.SpatialSpec.sparse(crop, wo_crop=True), n, h, w, crop)
    assert np.mean([p.x0 == 0 for p in ps]) < 0.05 and all(p.x0 + p.cw < p.frame(h, w)[1] for p in ps)   # randint's open end, no margin


def test_draw_spatial_raises_when_the_crop_cannot_fit():
    with pytest.raises(ValueError, match="cannot fit"):                               # not rescaled, and the crop is the frame: randint(0, 0)
        SP.draw_spatial(SP.SpatialSpec(kind="sparse", spatial_aug_prob=0.0, min_pad=1, yjitter=False), 1, 0, 1, 40, 64, [(40, 64)])
    with pytest.raises(ValueError, match="cannot fit"):
        SP.draw_spatial(SP.SpatialSpec(kind="sparse", spatial_aug_prob=0.0, min_pad=1, yjitter=False), 1, 0, 1, 40, 64, [(41, 64)])
    with pytest.raises(ValueError):                                                   # the scale floor would pass 8
        SP.draw_spatial(SP.SpatialSpec.flow(), 1, 0, 1, 8, 8, [(80, 80)])
    with pytest.raises(ValueError, match="leaves"):
        SP.SpatialParams(ch=10, cw=10, y0=31).validate(40, 64)
    with pytest.raises(ValueError, match="dy2"):
        SP.SpatialParams(ch=10, cw=10, y0=1, dy2=-2).validate(40, 64)
    with pytest.raises(ValueError, match="outside"):
        SP.SpatialParams(rescale=True, scale_x=0.1, ch=1, cw=1).validate(40, 64)


# ---- the library, host side -----------------------------------------------------------------------------------------------------

def test_library_loads_and_validates_without_a_gpu():
    from anystereo import _spatial_lib as L
    lib = L.load()
    assert lib.spt_abi_version() == 1
    assert L.library_info()["matches_sources"] is True
    fh, fw = C.c_int(), C.c_int()
    assert lib.spt_frame_size(40, 64, 1, 0.8828125, 0.8828125, C.byref(fh), C.byref(fw)) == L.SPT_OK and (fh.value, fw.value) == (35, 56)
    assert lib.spt_frame_size(40, 64, 1, 1.5, 0.6875, C.byref(fh), C.byref(fw)) == L.SPT_OK and (fh.value, fw.value) == (28, 96)   # 27.5 -> 28
    assert lib.spt_frame_size(40, 64, 0, 99.0, float("nan"), C.byref(fh), C.byref(fw)) == L.SPT_OK and (fh.value, fw.value) == (40, 64)
    for sx, sy in ((0.1249, 1.0), (1.0, 8.01), (float("nan"), 1.0), (1.0, float("inf")), (-1.0, 1.0)):
        assert lib.spt_frame_size(40, 64, 1, sx, sy, C.byref(fh), C.byref(fw)) == L.SPT_ERR_BAD_ARG
    assert lib.spt_frame_size(40, 64, 1, 0.125, 8.0, C.byref(fh), C.byref(fw)) == L.SPT_OK and (fh.value, fw.value) == (320, 8)
    assert lib.spt_frame_size(0, 64, 0, 1.0, 1.0, C.byref(fh), C.byref(fw)) == L.SPT_ERR_BAD_ARG
    assert lib.spt_frame_size(40, 64, 0, 1.0, 1.0, None, C.byref(fw)) == L.SPT_ERR_BAD_ARG
    assert lib.spt_last_error_string().decode().startswith("spt_frame_size")

    P = SP.SpatialParams
    val = lambda ps, B=None, H=40, W=64, oh=0, ow=0: lib.spt_validate(SP.c_samples(ps), len(ps) if B is None else B, H, W, oh, ow)  # noqa: E731
    good = P(True, 1.25, 1.25, "hf", 26, 40, 24, 40, 0)
    assert val([good, good]) == L.SPT_OK
    assert val([good, P(ch=20, cw=30)], oh=16, ow=28) == L.SPT_OK
    assert val([good, P(ch=20, cw=30)]) == L.SPT_ERR_CROP                               # ragged crops need an out size
    assert val([good], oh=16, ow=0) == L.SPT_ERR_BAD_ARG
    assert val([good], B=0) == L.SPT_ERR_BAD_ARG
    assert val([P(True, 8.5, 1.0, ch=4, cw=4)]) == L.SPT_ERR_BAD_ARG
    assert val([P(True, 1.0, 0.12, ch=4, cw=4)]) == L.SPT_ERR_BAD_ARG
    assert val([P(True, 1.25, 1.25, "none", 27, 40, 24, 40, 0)]) == L.SPT_ERR_CROP      # one row past the 50 x 80 frame
    assert val([P(True, 1.25, 1.25, "none", 26, 41, 24, 40, 0)]) == L.SPT_ERR_CROP
    assert val([P(ch=24, cw=40, y0=-1)]) == L.SPT_ERR_CROP
    assert val([P(ch=24, cw=40, y0=1, dy2=-2)]) == L.SPT_ERR_CROP                       # y0 + dy2 < 0
    assert val([P(ch=24, cw=40, y0=15, dy2=2)]) == L.SPT_ERR_CROP                       # y0 + dy2 + ch > 40
    assert val([P(ch=24, cw=40, y0=14, dy2=2)]) == L.SPT_OK
    assert val([P(ch=0, cw=40)]) == L.SPT_ERR_BAD_ARG
    s = SP.c_samples([good])
    s[0].flip = 4
    assert lib.spt_validate(s, 1, 40, 64, 0, 0) == L.SPT_ERR_BAD_ARG
    s[0].flip, s[0].rescale = 0, 2
    assert lib.spt_validate(s, 1, 40, 64, 0, 0) == L.SPT_ERR_BAD_ARG
    assert val([P(ch=4, cw=4)], H=1 << 15, W=1 << 15) == L.SPT_ERR_BAD_SHAPE            # 3 B H W >= 2^31
    assert val([P(ch=4, cw=4)] * 2, oh=1 << 15, ow=1 << 14) == L.SPT_ERR_BAD_SHAPE      # the output's 3 B h w
    assert lib.spt_validate(None, 1, 40, 64, 0, 0) == L.SPT_ERR_BAD_ARG

    # spt_spatial_pair refuses before it launches: every call below is refused (the pointers are never dereferenced)
    base, vp = 1 << 20, C.c_void_p
    dptr, vptr = (vp * 1)(base + 0x60000), (vp * 1)(base + 0x70000)
    one = SP.c_samples([P(ch=24, cw=40)])

    def call(image1=base, image2=base + 0x10000, in_dtype=0, disp=base + 0x20000, valid=None, samples=one, out1=base + 0x40000, out2=base + 0x50000,
             out_dtype=0, oh=0, ow=0, dp=dptr, vo=None):
        return lib.spt_spatial_pair(image1, image2, in_dtype, disp, valid, 1, 40, 64, samples, out1, out2, out_dtype, oh, ow, dp, vo, None)
    assert call(image1=None) == L.SPT_ERR_BAD_ARG
    assert call(disp=None) == L.SPT_ERR_BAD_ARG
    assert call(dp=None) == L.SPT_ERR_BAD_ARG
    assert call(dp=(vp * 1)(None)) == L.SPT_ERR_BAD_ARG
    assert call(valid=base + 0x30000) == L.SPT_ERR_BAD_ARG                              # valid without valid_out
    assert call(vo=vptr) == L.SPT_ERR_BAD_ARG
    assert call(in_dtype=2) == L.SPT_ERR_BAD_ARG
    assert call(in_dtype=1, image1=base + 2) == L.SPT_ERR_BAD_ARG                       # misaligned fp32
    assert call(out_dtype=1, out2=base + 0x50001) == L.SPT_ERR_BAD_ARG
    assert call(disp=base + 0x20002) == L.SPT_ERR_BAD_ARG
    assert call(dp=(vp * 1)(base + 0x60001)) == L.SPT_ERR_BAD_ARG
    assert call(samples=SP.c_samples([P(ch=24, cw=40, y0=17)])) == L.SPT_ERR_CROP
    assert call(samples=SP.c_samples([P(True, 9.0, 1.0, ch=24, cw=40)])) == L.SPT_ERR_BAD_ARG
    assert call(out1=base + 100) == L.SPT_ERR_ALIAS                                     # inside image1
    assert call(out2=base + 0x20000 + 40 * 64 * 4 - 1) == L.SPT_ERR_ALIAS               # the last byte of disp
    assert call(out2=base + 0x40000 + 24 * 40 * 3 - 1) == L.SPT_ERR_ALIAS               # the last byte of out1
    assert call(dp=(vp * 1)(base + 0x40000 + 8)) == L.SPT_ERR_ALIAS                     # a crop inside out1
    assert call(valid=base + 0x30000, vo=(vp * 1)(base + 0x60000 + 24 * 40 * 4 - 1)) == L.SPT_ERR_ALIAS   # valid_out[0] on disp_out[0]
    assert call(valid=base + 0x30000, vo=(vp * 1)(base + 0x30000 + 5)) == L.SPT_ERR_ALIAS                 # valid_out[0] inside valid
    assert lib.spt_last_error_string().decode().startswith("spt_spatial_pair")
