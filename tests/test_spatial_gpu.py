"""Spatial augmentation on the device (csrc/spatial/spatial.hip through anystereo/harness/spatial.py): the kernels bit-equal to the numpy
restatement (which tests/test_spatial_cpu.py holds against the fixture of the reference's own classes) on the fixture's cases and on
hashed parameters, every call under the guarded, poisoned allocator of tests/_guarded.py, refused calls launching nothing, and the
consumer.  Nothing here reads the reference.
"""
import ctypes as C

import pytest
import torch

import _guarded as GD
import _spatial_cases as K
from _cache_hygiene import hand_the_cache_back_zeroed
from anystereo.harness import spatial as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CALLS = {}  # spt_* symbol -> calls made while a guarded context was active


@pytest.fixture(scope="module", autouse=True)
def _counted_library():
    from anystereo import _spatial_lib as L
    try:
        with GD.counted(L, CALLS):
            yield
    finally:
        hand_the_cache_back_zeroed(DEV)


def _equal(got, want, what):
    """(out1, out2, disps, valids) on the device against the host's, bit for bit."""
    g1, g2, gd, gv = got
    w1, w2, wd, wv = want
    for g, w_, name in ((g1, w1, "image1"), (g2, w2, "image2")):
        assert g.is_cuda and g.shape == w_.shape and g.dtype == w_.dtype, (what, name, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w_), f"{what} {name}: {int((g.cpu() != w_).sum())} of {w_.numel()} values differ"
    assert len(gd) == len(wd) and (gv is None) == (wv is None)
    for b, (g, w_) in enumerate(zip(gd, wd)):
        assert g.is_cuda and g.dtype == torch.float32 and g.shape == w_.shape, (what, b, tuple(g.shape))
        assert torch.equal(K.bits(g.cpu()), K.bits(w_)), f"{what} disp {b}: {int((K.bits(g.cpu()) != K.bits(w_)).sum())} of {w_.numel()} differ"
    for b, (g, w_) in enumerate(zip(gv or [], wv or [])):
        assert g.is_cuda and g.dtype == torch.uint8 and torch.equal(g.cpu(), w_), f"{what} valid {b}"


def _guarded_equal(im1, im2, disp, valid, params, out_size, out_dtype, want, what, skew=0):
    """The call under both fill patterns: inputs placed between poisoned neighbours, all guards intact, the result bit-equal to the
    host's — which no poisoned byte survives, as 0xFF and 0x47 differ in every byte — and the inputs unchanged."""
    for pattern in GD.PATTERNS:
        with GD.guarded(pattern) as g:
            d1, d2, dd = g.place(im1, DEV, skew), g.place(im2, DEV), g.place(disp, DEV)
            dv = None if valid is None else g.place(valid, DEV, skew)
            got = SP.spatial_pair(d1, d2, dd, params, valid=dv, out_size=out_size, out_dtype=out_dtype)
            g.check()
            _equal(got, want, f"{what}, fill 0x{pattern:02X}")
            assert torch.equal(d1.cpu(), im1) and torch.equal(d2.cpu(), im2) and torch.equal(K.bits(dd.cpu()), K.bits(disp))
            g.check()


# ---- kernel == restatement -----------------------------------------------------------------------------------------------------

def test_kernel_equals_restatement_on_the_fixture():
    for name, im1, im2, disp, valid, params, out_size, want in K.fixture_cases():
        host = SP.spatial_pair_host(im1, im2, disp, params, valid=valid)
        assert torch.equal(host[0][0], want["st1"]) and torch.equal(K.bits(host[2][0]), K.bits(want["disp"]))    # the reference's own result
        _guarded_equal(im1, im2, disp, valid, params, None, torch.uint8, host, name)
        if out_size is not None:
            host = SP.spatial_pair_host(im1, im2, disp, params, valid=valid, out_size=out_size)
            assert torch.equal(host[0][0], want["out1"]) and torch.equal(host[1][0], want["out2"])
            _guarded_equal(im1, im2, disp, valid, params, out_size, torch.uint8, host, name + " resized")


# 45 x 70: odd planes; LR 12 x 20 at scales 1.0 .. 2.0: ragged crops 12 x 20 .. 24 x 40 (more than one block of 256 pixels);
# B = 1, 8 (a full launch table) and 9 (two chunks); every flip mode in turn, y-jitter on and off
@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("batch", [1, 8, 9])
def test_kernel_equals_restatement_on_hashed_parameters(batch, sparse):
    h, w, lr = 45, 70, (12, 20)
    im1, im2, disp, valid = K.random_frames(batch, h, w, seed=batch, sparse=sparse)
    scales = [1.0 + b / 8.0 for b in range(batch)]
    ragged = K.hashed_params(batch, h, w, [(round(lr[0] * s), round(lr[1] * s)) for s in scales], sparse)
    fixed = K.hashed_params(batch, h, w, [(20, 33)] * batch, sparse, seed=4)
    assert batch < 4 or ({p.flip for p in ragged} == set(SP.FLIPS) and len({(p.ch, p.cw) for p in ragged}) > 3)
    assert batch < 8 or sparse or {p.dy2 != 0 for p in ragged + fixed} == {True, False}
    for params, out_size in ((ragged, lr), (fixed, None)):
        for in_f32, out_dtype in ((False, torch.uint8), (True, torch.float32), (False, torch.float32), (True, torch.uint8)):
            if batch == 8 and in_f32 != (out_dtype == torch.float32):
                continue                                                            # the mixed pairs run at B = 1 and 9
            a1, a2 = (im1.float(), im2.float()) if in_f32 else (im1, im2)
            want = SP.spatial_pair_host(a1, a2, disp, params, valid=valid, out_size=out_size, out_dtype=out_dtype)
            _guarded_equal(a1, a2, disp, valid, params, out_size, out_dtype, want, f"B={batch} f32_in={in_f32} {out_dtype} out_size={out_size}",
                           skew=4 if batch == 9 else 0)


def test_fp32_input_is_quantised_once_on_the_device():
    im1, im2, disp, _ = K.random_frames(2, 45, 70, seed=9)
    noise = (torch.rand(im1.shape, generator=torch.Generator().manual_seed(1)) - 0.5) * 0.98
    f1, f2 = im1.float() + noise, im2.float() * 1.3 - 20.0                          # image2 leaves [0, 255] on both sides
    params = K.hashed_params(2, 45, 70, [(20, 33), (24, 40)], False)
    want = SP.spatial_pair_host(f1, f2, disp, params, out_size=(12, 20))
    _equal(SP.spatial_pair(f1.to(DEV), f2.to(DEV), disp.to(DEV), params, out_size=(12, 20)), want, "quantise")
    assert torch.equal(want[0], SP.spatial_pair_host(im1, im2, disp, params, out_size=(12, 20))[0])   # the noise rounds away


def test_identity_parameters_return_the_inputs():
    im1, im2, disp, valid = K.random_frames(2, 37, 53, seed=5, sparse=True)
    disp[0, 2, 3], disp[1, 0, 0] = float("inf"), -0.0
    p = [SP.SpatialParams(ch=37, cw=53)] * 2
    for dt in (torch.uint8, torch.float32):
        a1, a2 = im1.to(dt), im2.to(dt)
        o1, o2, ds, vs = SP.spatial_pair(a1.to(DEV), a2.to(DEV), disp.to(DEV), p, valid=valid.to(DEV), out_dtype=dt)
        assert torch.equal(o1.cpu(), a1) and torch.equal(o2.cpu(), a2)
        assert torch.equal(K.bits(torch.stack(ds).cpu()), K.bits(disp)) and torch.equal(torch.stack(vs).cpu(), valid)
    o1, o2, ds, vs = SP.spatial_pair(im1.to(DEV), im2.to(DEV), disp.to(DEV), p)
    assert vs is None and torch.equal(K.bits(torch.stack(ds).cpu()), K.bits(disp)) and torch.equal(o2.cpu(), im2)


# ---- refused calls -------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing():
    from anystereo import _spatial_lib as L
    from anystereo import ops
    lib = L.load()
    P_ = SP.SpatialParams
    ok = SP.c_samples([P_(True, 1.25, 1.25, "hf", 3, 5, 8, 16, 1), P_(ch=8, cw=16)])
    for pattern in GD.PATTERNS:
        with GD.guarded(pattern) as g:
            z8 = torch.zeros(2, 3, 16, 32, dtype=torch.uint8)
            i1, i2 = g.place(z8, DEV), g.place(z8, DEV)
            dd, vv = g.place(torch.zeros(2, 16, 32), DEV), g.place(torch.zeros(2, 16, 32, dtype=torch.uint8), DEV)
            o1 = torch.empty((2, 3, 8, 16), device=DEV, dtype=torch.uint8)
            o2 = torch.empty((2, 3, 8, 16), device=DEV, dtype=torch.uint8)
            f1 = torch.empty((2, 3, 8, 16), device=DEV, dtype=torch.float32)
            dc = [torch.empty((8, 16), device=DEV, dtype=torch.float32) for _ in range(2)]
            vc = [torch.empty((8, 16), device=DEV, dtype=torch.uint8) for _ in range(2)]
            s, P = ops._stream(), ops._p
            table = lambda ts: (C.c_void_p * 2)(*[t if isinstance(t, int) or t is None else t.data_ptr() for t in ts])  # noqa: E731

            def call(samples=ok, image1=P(i1), image2=P(i2), in_dtype=0, disp=P(dd), valid=P(vv), B=2, h=16, w=32, out1=P(o1), out2=P(o2), out_dtype=0,
                     oh=0, ow=0, dp=table(dc), vp=table(vc)):
                return lib.spt_spatial_pair(image1, image2, in_dtype, disp, valid, B, h, w, samples, out1, out2, out_dtype, oh, ow, dp, vp, s)
            bad = lambda *ps: SP.c_samples(list(ps))  # noqa: E731
            assert call(image2=None) == L.SPT_ERR_BAD_ARG
            assert call(samples=None) == L.SPT_ERR_BAD_ARG
            assert call(dp=None) == L.SPT_ERR_BAD_ARG
            assert call(dp=table([dc[0], None])) == L.SPT_ERR_BAD_ARG
            assert call(vp=None) == L.SPT_ERR_BAD_ARG                               # valid without valid_out
            assert call(out_dtype=3) == L.SPT_ERR_BAD_ARG
            assert call(out1=f1.data_ptr() + 2, out2=P(f1), out_dtype=1) == L.SPT_ERR_BAD_ARG
            assert call(disp=dd.data_ptr() + 2) == L.SPT_ERR_BAD_ARG
            assert call(dp=table([dc[0], dc[1].data_ptr() + 1])) == L.SPT_ERR_BAD_ARG
            assert call(h=0) == L.SPT_ERR_BAD_ARG
            assert call(B=-1) == L.SPT_ERR_BAD_ARG
            assert call(h=1 << 15, w=1 << 15) == L.SPT_ERR_BAD_SHAPE
            assert call(oh=8, ow=0) == L.SPT_ERR_BAD_ARG
            assert call(samples=bad(P_(ch=8, cw=16), P_(True, 0.12, 1.0, ch=1, cw=1))) == L.SPT_ERR_BAD_ARG     # the second sample refuses the first
            assert call(samples=bad(P_(ch=8, cw=16), P_(True, 1.0, 8.5, ch=8, cw=16))) == L.SPT_ERR_BAD_ARG
            assert call(samples=bad(P_(ch=8, cw=16), P_(True, float("nan"), 1.0, ch=8, cw=16))) == L.SPT_ERR_BAD_ARG
            assert call(samples=bad(P_(ch=8, cw=16), P_(ch=8, cw=16, y0=9))) == L.SPT_ERR_CROP                  # 9 + 8 > 16
            assert call(samples=bad(P_(ch=8, cw=16), P_(True, 1.25, 1.25, "v", 12, 25, 8, 16, 0))) == L.SPT_ERR_CROP    # 25 + 16 > 40
            assert call(samples=bad(P_(ch=8, cw=16), P_(ch=8, cw=16, y0=1, dy2=-2))) == L.SPT_ERR_CROP
            assert call(samples=bad(P_(ch=8, cw=16), P_(ch=8, cw=16, y0=7, dy2=2))) == L.SPT_ERR_CROP
            assert call(samples=bad(P_(ch=8, cw=16), P_(ch=8, cw=15))) == L.SPT_ERR_CROP                        # ragged without an out size
            assert call(out1=P(i1)) == L.SPT_ERR_ALIAS
            assert call(out2=i2.data_ptr() + 3071) == L.SPT_ERR_ALIAS
            assert call(out2=o1.data_ptr() + 8) == L.SPT_ERR_ALIAS
            assert call(out1=dd.data_ptr() + 4095) == L.SPT_ERR_ALIAS
            assert call(dp=table([dc[0], dc[0].data_ptr() + 256])) == L.SPT_ERR_ALIAS                           # two crops overlap
            assert call(dp=table([dc[0], o2.data_ptr() + 4])) == L.SPT_ERR_ALIAS
            assert call(vp=table([vc[0], vv.data_ptr() + 1023])) == L.SPT_ERR_ALIAS
            assert lib.spt_last_error_string().decode().startswith("spt_spatial_pair")
            with pytest.raises(ValueError, match="leaves"):
                SP.spatial_pair(i1, i2, dd, [P_(ch=8, cw=16), P_(ch=8, cw=16, x0=17)], valid=vv)
            with pytest.raises(ValueError, match="one size"):
                SP.spatial_pair(i1, i2, dd, [P_(ch=8, cw=16), P_(ch=8, cw=15)], valid=vv)
            assert g.nothing_written()
            assert not bool(i1.any()) and not bool(dd.any())
            g.check()
            assert call() == L.SPT_OK                                               # the same call, nothing changed: it runs
            assert not g.is_poisoned(o1) and not g.is_poisoned(o2) and not any(g.is_poisoned(t) for t in dc + vc)
            g.check()


def test_every_launching_spatial_symbol_ran_under_a_guard():
    from anystereo import _spatial_lib as L
    missing = [n for n in L.LAUNCHING if not CALLS.get(n)]
    assert not missing, f"never called under a guard: {missing}"
    # what is left launches nothing: three queries of the library itself, the frame-size rule and the host's validation
    assert set(L.SIGNATURES) - set(L.LAUNCHING) == {"spt_abi_version", "spt_last_error_string", "spt_source_hash", "spt_frame_size", "spt_validate"}


# ---- the consumer --------------------------------------------------------------------------------------------------------------

def test_scene_train_batch_without_spatial_is_unchanged():
    from anystereo.harness import scenes as H
    spec = H.SceneSpec()
    plain = H.scene_train_batch(spec, 5, 3, 4, 64, 128, mode="dense", device=DEV)
    again = H.scene_train_batch(spec, 5, 3, 4, 64, 128, mode="dense", device=DEV, spatial=None, frame_hw=None)
    assert len(plain) == len(again) == 6
    for a, b in zip(plain, again):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    r1, r2 = H.render_pair(spec, 5, 12, 4, 64, 128, DEV)
    assert torch.equal(plain[0], r1) and torch.equal(plain[1], r2)                  # still the rendered pair itself


@pytest.mark.parametrize("kind", ["flow", "sparse"])
def test_scene_train_batch_with_a_spatial_spec(kind):
    from anystereo.harness import augment as A, scenes as H
    spec = H.SceneSpec()
    spatial = SP.SpatialSpec.flow(do_flip="h") if kind == "flow" else SP.SpatialSpec.sparse(wo_crop=True)
    kw = dict(mode="dense" if kind == "flow" else "sparse", device=DEV, augment=A.PhotoSpec.flow(), spatial=spatial, frame_hw=(135, 240))
    one = H.scene_train_batch(spec, 5, 3, 4, 32, 64, 1.0, 2.95, **kw)
    two = H.scene_train_batch(spec, 5, 3, 4, 32, 64, 1.0, 2.95, **kw)
    plain = H.scene_train_batch(spec, 5, 3, 4, 32, 64, 1.0, 2.95, mode=kw["mode"], device=DEV)
    assert len(one) == len(two) == len(plain) == 6
    for a, b, p in zip(one, two, plain):
        assert a.is_cuda and a.shape == p.shape and a.dtype == p.dtype              # the shapes Trainer.step takes
        assert torch.equal(a, b)
    assert float(one[0].min()) >= 0 and float(one[1].max()) <= 255 and torch.equal(one[0], one[0].round())
