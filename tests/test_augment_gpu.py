"""Photometric augmentation on the device (csrc/augment/augment.hip through anystereo/harness/augment.py): the kernels byte-equal to
the numpy restatement (which tests/test_augment_cpu.py holds against PIL itself) and to the committed PIL fixture, the launching
entry under the guarded, poisoned allocator of tests/_guarded.py, refused calls launching nothing, and the consumers.  Nothing here
imports PIL or reads the reference.
"""
import math

import pytest
import torch

import _augment_cases as K
import _guarded as GD
from _cache_hygiene import hand_the_cache_back_zeroed
from anystereo.harness import augment as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CALLS = {}  # aug_* symbol -> calls made while a guarded context was active


@pytest.fixture(scope="module", autouse=True)
def _counted_library():
    from anystereo import _augment_lib as L
    try:
        with GD.counted(L, CALLS):
            yield
    finally:
        hand_the_cache_back_zeroed(DEV)   # this module's freed blocks hold random image bytes and partial sums


def _equal(got, want, what):
    for g, w_, name in zip(got, want, ("image1", "image2")):
        assert g.is_cuda and g.shape == w_.shape and g.dtype == w_.dtype, (what, name, g.dtype, tuple(g.shape))
        assert torch.equal(g.cpu(), w_), f"{what} {name}: {int((g.cpu() != w_).sum())} of {w_.numel()} values differ"


# ---- kernel == restatement -----------------------------------------------------------------------------------------------------

# 3x5: less than one thread group; 24x40: planes that keep their 8-byte alignment; 37x53: an odd plane size, so planes start at every
# byte offset and the last group of 8 is partial; 160x320, B = 5: the training shape, 25 blocks per image; B = 9: two chunks
@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("batch,h,w", [(2, 3, 5), (9, 24, 40), (9, 37, 53), (5, 160, 320)])
def test_kernel_equals_restatement(batch, h, w, dtype):
    i1, i2 = K.random_pair(batch, h, w, seed=h * w)
    params = K.mixed_params(batch, h, w)
    assert {sp.shared for sp in params} == {True, False} and any(not sp.rects for sp in params)
    lut = torch.from_numpy(A.gamma_table(params))
    if dtype == torch.float32:
        i1, i2 = i1.float(), i2.float()
    for out_dtype in (torch.uint8, torch.float32):
        want = A.photometric_pair_host(i1, i2, params, out_dtype=out_dtype, gamma_lut=lut)
        got = A.photometric_pair(i1.to(DEV), i2.to(DEV), params, out_dtype=out_dtype, gamma_lut=lut.to(DEV))
        _equal(got, want, f"{batch}x{h}x{w} {dtype} -> {out_dtype}")
    got = A.photometric_pair(i1.to(DEV), i2.to(DEV), params)                       # no table: the identity
    _equal(got, A.photometric_pair_host(i1, i2, params), "no gamma table")


def test_fp32_input_is_quantised_once_on_the_device():
    i1, i2 = K.random_pair(2, 37, 53, seed=9)
    noise = (torch.rand(i1.shape, generator=torch.Generator().manual_seed(1)) - 0.5) * 0.98
    f1, f2 = i1.float() + noise, i2.float() * 1.3 - 20.0                           # image2 leaves [0, 255] on both sides
    params = K.mixed_params(2, 37, 53)
    _equal(A.photometric_pair(f1.to(DEV), f2.to(DEV), params), A.photometric_pair_host(f1, f2, params), "quantise")


def test_kernel_equals_the_pil_fixture():
    for name, i1, i2, sp, lut, o1, o2 in K.fixture_sets():
        got = A.photometric_pair(i1.to(DEV), i2.to(DEV), sp, gamma_lut=None if lut is None else lut.to(DEV))
        _equal(got, (o1, o2), name)


@pytest.fixture(scope="module")
def hue_reference():
    """Every colour through the restatement's hue with shifts 37 and 255: computed once, RGB -> HSV shared by the two."""
    import numpy as np
    img = K.all_colours()
    h, s, v = A.rgb_to_hsv(*(img[0, c].numpy().astype(np.int32) for c in range(3)))
    want = [torch.from_numpy(np.stack(A.hsv_to_rgb((h + shift) & 255, s, v)).astype(np.uint8)).unsqueeze(0) for shift in (37, 255)]
    return img, want[0], want[1]


@pytest.mark.parametrize("shift", [37, 255])
def test_hue_on_every_colour(hue_reference, shift):
    img, want37, want255 = hue_reference
    d = img.to(DEV)
    other = 255 if shift == 37 else 37
    got1, got2 = A.photometric_pair(d, d, K.hue_only(shift, other))                 # the two inputs may be one tensor
    want1, want2 = (want37, want255) if shift == 37 else (want255, want37)
    for g, w_ in ((got1, want1), (got2, want2)):
        diff = (g != w_.to(DEV))
        assert not bool(diff.any()), f"{int(diff.sum())} of 2^24 colours differ, the first at index {int(diff.view(3, -1).any(0).nonzero()[0])}"


def test_shared_samples_take_the_mean_of_both_images():
    i1 = torch.full((1, 3, 12, 20), 40, dtype=torch.uint8)
    i2 = torch.full((1, 3, 12, 20), 200, dtype=torch.uint8)
    p = A.ImageParams(order=(1, 0, 2, 3), contrast=0.5)
    o1, o2 = A.photometric_pair(i1.to(DEV), i2.to(DEV), [A.SampleParams(p, p, shared=True)])
    assert bool((o1 == 80).all()) and bool((o2 == 160).all())                       # level 120: 120 + 0.5 (x - 120)
    o1, o2 = A.photometric_pair(i1.to(DEV), i2.to(DEV), [A.SampleParams(p, p, shared=False)])
    assert bool((o1 == 40).all()) and bool((o2 == 200).all())                       # each image's own mean
    # a tie: the stacked mean grey is exactly 119.5 and rounds up
    a, b = torch.full((1, 3, 2, 4), 119, dtype=torch.uint8), torch.full((1, 3, 2, 4), 120, dtype=torch.uint8)
    z = A.ImageParams(contrast=0.0)
    o1, o2 = A.photometric_pair(a.to(DEV), b.to(DEV), [A.SampleParams(z, z, shared=True)])
    assert bool((o1 == 120).all()) and bool((o2 == 120).all())


def test_eraser_fills_clipped_rectangles_with_the_mean_after_the_jitter():
    i1, i2 = K.random_pair(1, 12, 20, seed=4)
    p = A.ImageParams(order=(0, 1, 2, 3), brightness=0.5, contrast=1.2, saturation=0.8, hue_shift=9)
    rects = ((19, 11, 50, 50), (0, 0, 50, 50))
    jit1, jit2 = A.photometric_pair_host(i1, i2, [A.SampleParams(p, p, shared=True)])
    o1, o2 = A.photometric_pair(i1.to(DEV), i2.to(DEV), [A.SampleParams(p, p, shared=True, rects=rects)])
    mean = jit2[0].view(3, -1).long().sum(1) // (12 * 20)                           # of the JITTERED image2, floored
    assert not torch.equal(mean, i2[0].view(3, -1).long().sum(1) // (12 * 20))
    assert torch.equal(o2.cpu(), mean.to(torch.uint8).view(1, 3, 1, 1).expand(1, 3, 12, 20))   # the second rectangle covers the frame
    assert torch.equal(o1.cpu(), jit1)                                              # image1 is untouched
    _, o2 = A.photometric_pair(i1.to(DEV), i2.to(DEV), [A.SampleParams(p, p, shared=True, rects=rects[:1])])
    want = jit2.clone()
    want[0, :, 11, 19] = mean.to(torch.uint8)
    assert torch.equal(o2.cpu(), want)                                              # one pixel: the rest of the 50 x 50 is outside
    # a channel mean of exactly k + 1/2 is floored
    b2 = torch.full((1, 3, 2, 4), 120, dtype=torch.uint8)
    b2[0, :, 0, :] = 121
    _, o2 = A.photometric_pair(b2.to(DEV), b2.to(DEV), [A.SampleParams(rects=((3, 1, 9, 9),))])
    assert int(o2[0, 0, 1, 3]) == 120 and torch.equal(o2[0, :, 0].cpu(), b2[0, :, 0])


# ---- memory hygiene ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
def test_photometric_pair_hygiene(dtype):
    batch, h, w = 9, 37, 53                                                         # two chunks, odd planes
    i1, i2 = K.random_pair(batch, h, w, seed=2)
    if dtype == torch.float32:
        i1, i2 = i1.float(), i2.float()
    params = K.mixed_params(batch, h, w)
    lut = torch.from_numpy(A.gamma_table(params))
    placed = []

    def run(put, skew=0):
        d1, d2, dl = put(i1, skew), put(i2), put(lut)
        out = A.photometric_pair(d1, d2, params, out_dtype=dtype, gamma_lut=dl)
        placed.append((d1, d2, dl))
        assert torch.equal(d1, i1.to(DEV)) and torch.equal(d2, i2.to(DEV)) and torch.equal(dl, lut.to(DEV))   # inputs unchanged
        return out
    got = GD.hygiene(run, DEV)
    _equal(got, A.photometric_pair_host(i1, i2, params, out_dtype=dtype, gamma_lut=lut), "hygiene")
    es = 1 if dtype == torch.uint8 else 4
    got = GD.hygiene(lambda put: run(put, skew=3 * es), DEV)                        # image1 off every vector alignment
    _equal(got, A.photometric_pair_host(i1, i2, params, out_dtype=dtype, gamma_lut=lut), "hygiene, skewed")
    assert len(placed) == 6


def test_refused_calls_launch_nothing():
    from anystereo import _augment_lib as L
    from anystereo import ops
    lib = L.load()
    ok = A.c_samples([A.SampleParams(rects=((1, 1, 4, 4),))] * 2)

    def bad(**kw):
        s = A.c_samples([A.SampleParams()] * 2)
        if "order" in kw:
            s[1].img[0].order[:] = kw["order"]
        if "factor" in kw:
            s[0].img[1].factor[2] = kw["factor"]
        if "hue" in kw:
            s[1].img[1].hue_shift = kw["hue"]
        if "rect" in kw:
            s[1].n_rects = 1
            s[1].rect[0][:] = kw["rect"]
        if "n_rects" in kw:
            s[1].n_rects = kw["n_rects"]
        return s
    for pattern in GD.PATTERNS:
        with GD.guarded(pattern) as g:
            i1 = g.place(torch.zeros(2, 3, 8, 16, dtype=torch.uint8), DEV)
            i2 = g.place(torch.zeros(2, 3, 8, 16, dtype=torch.uint8), DEV)
            o1 = torch.empty((2, 3, 8, 16), device=DEV, dtype=torch.uint8)
            o2 = torch.empty((2, 3, 8, 16), device=DEV, dtype=torch.uint8)
            f1 = torch.empty((2, 3, 8, 16), device=DEV, dtype=torch.float32)
            ws = torch.empty((2 * 5 * 8,), device=DEV, dtype=torch.uint8)             # poisoned, unlike an int64 workspace
            s = ops._stream()
            P = ops._p

            def call(samples=ok, image1=P(i1), image2=P(i2), in_dtype=0, out1=P(o1), out2=P(o2), out_dtype=0, B=2, h=8, w=16, lut=None,
                     wsp=P(ws), nws=80):
                return lib.aug_photometric_pair(image1, image2, in_dtype, out1, out2, out_dtype, B, h, w, samples, lut, wsp, nws, s)
            assert call(image2=None) == L.AUG_ERR_BAD_ARG
            assert call(samples=None) == L.AUG_ERR_BAD_ARG
            assert call(wsp=None) == L.AUG_ERR_BAD_ARG
            assert call(out_dtype=3) == L.AUG_ERR_BAD_ARG
            assert call(out1=f1.data_ptr() + 2, out2=P(f1), out_dtype=1) == L.AUG_ERR_BAD_ARG
            assert call(wsp=ws.data_ptr() + 4) == L.AUG_ERR_BAD_ARG
            assert call(h=0) == L.AUG_ERR_BAD_ARG
            assert call(B=-1) == L.AUG_ERR_BAD_ARG
            assert call(h=1 << 15, w=1 << 15) == L.AUG_ERR_BAD_SHAPE
            assert call(samples=bad(order=(3, 2, 1, 1))) == L.AUG_ERR_BAD_ARG       # the second sample refuses the first
            assert call(samples=bad(factor=-1.0)) == L.AUG_ERR_BAD_ARG
            assert call(samples=bad(factor=float("nan"))) == L.AUG_ERR_BAD_ARG
            assert call(samples=bad(hue=256)) == L.AUG_ERR_BAD_ARG
            assert call(samples=bad(n_rects=3)) == L.AUG_ERR_BAD_ARG
            assert call(samples=bad(rect=(0, 0, 0, 1))) == L.AUG_ERR_BAD_ARG
            assert call(samples=bad(rect=(16, 0, 1, 1))) == L.AUG_ERR_BAD_ARG
            assert call(samples=bad(rect=(0, 8, 1, 1))) == L.AUG_ERR_BAD_ARG
            assert call(nws=79) == L.AUG_ERR_WORKSPACE
            assert call(out1=P(i1)) == L.AUG_ERR_ALIAS
            assert call(out2=i2.data_ptr() + 767) == L.AUG_ERR_ALIAS
            assert call(out2=o1.data_ptr() + 8) == L.AUG_ERR_ALIAS
            assert call(out1=P(ws)) == L.AUG_ERR_ALIAS
            assert lib.aug_last_error_string().decode().startswith("aug_photometric_pair")
            with pytest.raises(ValueError, match="rectangle"):
                A.photometric_pair(i1, i2, [A.SampleParams(rects=((0, 0, 1, 0),))] * 2)
            assert g.nothing_written()
            assert not bool(i1.any()) and not bool(i2.any())
            g.check()
            assert call() == L.AUG_OK                                              # the same call, nothing changed: it runs
            assert not g.is_poisoned(o1) and not g.is_poisoned(o2)
            g.check()


def test_every_launching_augment_symbol_ran_under_a_guard():
    from anystereo import _augment_lib as L
    missing = [n for n in L.LAUNCHING if not CALLS.get(n)]
    assert not missing, f"never called under a guard: {missing}"
    # what is left launches nothing: three queries of the library itself and the host's size formula
    assert set(L.SIGNATURES) - set(L.LAUNCHING) == {"aug_abi_version", "aug_last_error_string", "aug_source_hash", "aug_workspace_bytes"}


# ---- the consumers -------------------------------------------------------------------------------------------------------------

def test_scene_train_batch_augments_the_images_and_nothing_else():
    from anystereo.harness import scenes as H
    spec, photo = H.SceneSpec(), A.PhotoSpec.flow()
    plain = H.scene_train_batch(spec, 5, 3, 4, 64, 128, mode="dense", device=DEV)
    again = H.scene_train_batch(spec, 5, 3, 4, 64, 128, mode="dense", device=DEV, augment=None)
    aug = H.scene_train_batch(spec, 5, 3, 4, 64, 128, mode="dense", device=DEV, augment=photo)
    assert len(plain) == len(again) == len(aug) == 6
    for a, b in zip(plain, again):
        assert torch.equal(a, b)
    r1, r2 = H.render_pair(spec, 5, 12, 4, 64, 128, DEV)                            # step 3, batch 4: scenes 12 .. 15
    assert torch.equal(plain[0], r1) and torch.equal(plain[1], r2)                  # augment=None: the rendered pair itself
    params = A.draw_params(photo, 5, H.train_batch_indices(3, 4)[0], 4, 64, 128)
    want = A.photometric_pair_host(plain[0].cpu(), plain[1].cpu(), params, out_dtype=torch.float32)
    _equal(aug[:2], want, "scene_train_batch(augment=flow)")
    assert not torch.equal(aug[0], plain[0])
    for a, b in zip(plain[2:], aug[2:]):
        assert torch.equal(a, b)                                                    # queries, ground truth, scales, low_disp


def test_two_trainer_steps_on_augmented_scene_batches():
    from anystereo.harness import scenes as H
    from anystereo.harness.synthetic import fill_module_deterministic
    from anystereo.harness.train import Trainer
    from anystereo.models import __models__, default_args
    args = default_args("continuous_IGEVStereo")
    m = __models__["continuous_IGEVStereo"](args)
    fill_module_deterministic(m, base_seed=1)
    tr = Trainer(m.to(DEV), lr=2e-4, num_steps=1000, train_iters=2, max_disp=args.max_disp, graph=False, supervise_init=True)
    losses = []
    # the 3-D convolutions' solver search is cached per configuration for the whole process: searched here as the deterministic
    # training tests of the suite search them (tests/test_init_head_gpu.py), so that they find what they would have found first
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        for step in range(2):
            batch = H.scene_train_batch(H.SceneSpec(), 5, step, 2, 64, 128, mode="dense", device=DEV, augment=A.PhotoSpec.flow())
            assert len(batch) == 6 and all(t.is_cuda for t in batch) and batch[0].dtype == torch.float32
            assert float(batch[0].min()) >= 0 and float(batch[1].max()) <= 255 and torch.equal(batch[0], batch[0].round())
            loss, _ = tr.step(batch)
            losses.append(float(loss))
    finally:
        torch.backends.cudnn.deterministic = prev
    assert all(math.isfinite(v) for v in losses), losses
    # the same order of magnitude as the scenes test's un-augmented steps: the second loss is not far above the first
    assert losses[1] <= 10.0 * losses[0], losses
