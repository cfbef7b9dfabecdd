"""The implicit upsampler with 5x5 and 7x7 affinity windows (lsp_width / lsp_height), without a GPU: construction and state-dict
parity against tests/golden/liif_windows.json, the windows the reference cannot run, the RAFT family's window, the argument
checks of the new C entry points, the fixture generator, and the float64 restatement the GPU tests compare against."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from _affinity_window import GOLD, META, affinity_ref, build_upsampler, close, fixture_inputs, gold

from anystereo import _lib as L
from anystereo.models import __models__
from anystereo.models.base import default_args
from anystereo.nn import liif as NL

CASES = sorted(META["cases"])


@pytest.mark.parametrize("name", CASES)
def test_constructor_matches_reference(name):
    ent = META["cases"][name]
    up = build_upsampler(ent["win"], ent["win"], ent["mode"])
    assert {k: list(v.shape) for k, v in up.state_dict().items()} == ent["state_dict"]
    assert up.imnet.layers[0].weight.shape[1] == ent["in_dim"]
    up.load_state_dict({k: torch.zeros(s) for k, s in ent["state_dict"].items()})
    assert up.window == (ent["win"], ent["win"])


def test_first_layer_widths_of_the_default_upsampler():
    assert [build_upsampler(w, w, "with_v2ISU").imnet.layers[0].weight.shape[1] for w in (3, 5, 7)] == [228, 260, 308]


@pytest.mark.parametrize("name", sorted(META["dead"]))
def test_windows_the_reference_cannot_run_fail_loudly(name):
    """Same constructor success and parameters as the reference, an error naming the reference's failure at forward."""
    ent = META["dead"][name]
    assert not ent["ok"] and ent["error"] == "RuntimeError"
    up = build_upsampler(ent["win_h"], ent["win_w"], ent["mode"])
    assert {k: list(v.shape) for k, v in up.state_dict().items()} == ent["state_dict"]
    assert up.imnet.layers[0].weight.shape[1] == ent["in_dim"]
    with pytest.raises(RuntimeError) as e:
        up(fixture_inputs()[0], torch.from_numpy(gold()["coord"]).clone(), torch.tensor([[1.5]]))
    assert "liif.py" in str(e.value)


def test_windows_outside_the_supported_set_are_not_built():
    with pytest.raises(NotImplementedError) as e:
        build_upsampler(9, 9, "with_v2ISU")
    assert "(3, 5, 7)" in str(e.value)
    with pytest.raises(NotImplementedError):
        NL.AffinityFeature(4, 4, 1, 0)


def test_window_routing_flags():
    """Only the 3x3 window may reach the one-kernel tail and its early rows."""
    coord = torch.zeros(1, 4, 2)
    for win in (5, 7):
        up = build_upsampler(win, win, "with_v2ISU")
        assert up._default_variant and up.window == (win, win)

        class Cuda:  # fused_ok reads is_cuda / shape only
            is_cuda, shape = True, (1, 16, 4, 6)

        assert not up.fused_ok([[Cuda()], [Cuda()]], Cuda())
        up.precompute_static([[None], [None]], 1, None, coord)  # returns before it touches its arguments
        assert "_early_static" not in up.__dict__


def test_models_construct_with_the_reference_key_shapes():
    for name, (mname, _, opt) in META["models"].items():
        model = __models__[mname](default_args(mname, **opt))
        want = META["model_state_dict"][name]
        assert {k: list(v.shape) for k, v in model.state_dict().items() if k.startswith("liif_up.")} == want, name
        sd = model.state_dict()
        model.load_state_dict({k: torch.zeros(want[k]) if k in want else v for k, v in sd.items()})


def test_raft_takes_both_window_sides_from_lsp_width():
    """prune_raft_stereo.py:184-185 never reads lsp_height; continuous_IGEVstereo.py:163-164 does."""
    raft = __models__["continuous_RAFTStereo"](default_args("continuous_RAFTStereo", lsp_width=5, lsp_height=3))
    assert raft.liif_up.window == (5, 5)
    assert all((sf.win_h, sf.win_w) == (5, 5) for sf in raft.liif_up.to_sf_l2)
    igev = __models__["continuous_IGEVStereo"](default_args("continuous_IGEVStereo", lsp_width=5, lsp_height=3))
    assert igev.liif_up.window == (3, 5)


def test_c_abi_rejects_bad_arguments_before_any_device_call():
    """Null pointers, non-positive sizes, a window outside {3, 5, 7} -> AS_ERR_BAD_ARG (-1); a plane of 2^31 pixels or more, a
    batch stride smaller than the tensor -> AS_ERR_BAD_SHAPE (-2); each with a message."""
    lib = L.load()
    buf = (ctypes.c_float * 16)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)

    def fwd(x=p, out=p, ws=p, b=1, c=4, h=2, w=2, win=5, with_x=0):
        return lib.as_affinity_window(x, out, ws, b, c, h, w, win, with_x, null)

    def bwd(x=p, aff=p, aff_bs=24 * 4, g=p, g_bs=24 * 4, gx=null, gx_bs=0, dx=p, ws=p, b=1, c=4, h=2, w=2, win=5):
        return lib.as_affinity_window_bwd(x, aff, aff_bs, g, g_bs, gx, gx_bs, dx, ws, b, c, h, w, win, null)

    def msg():
        return lib.as_last_error_string().decode()

    for call, names in ((fwd, ("x", "out", "ws")), (bwd, ("x", "aff", "g", "dx", "ws"))):
        for n in names:
            assert call(**{n: null}) == -1 and "null pointer" in msg(), n
        for n in ("b", "c", "h", "w"):
            for v in (0, -3):
                assert call(**{n: v}) == -1 and "non-positive" in msg(), (n, v)
        for win in (0, 1, 2, 4, 6, 8, 9, -5):
            assert call(win=win) == -1 and "win must be 3, 5 or 7" in msg(), win
        assert call(h=65536, w=32768) == -2 and "plane" in msg()
        assert call(h=46341, w=46341) == -2
    assert bwd(aff_bs=24 * 4 - 1) == -2 and "batch stride" in msg()
    assert bwd(g_bs=0) == -2
    assert bwd(gx=p, gx_bs=15) == -2
    assert lib.as_affinity_window_ws_bytes(2, 3, 5) == 120 and lib.as_affinity_window_ws_bytes(0, 3, 5) == 0
    assert lib.as_abi_version() == 38


def test_ops_reject_bad_arguments():
    from anystereo import ops
    x = torch.zeros(1, 4, 3, 3)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.affinity_window(x, 5, True)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.affinity_window_backward(x, x, x, 5, True)
    for win in (4, 9, 5.0, True, None):
        with pytest.raises(RuntimeError, match="win must be one of"):
            ops._req_window(win, "affinity_window")


def test_evaluate_tool_hands_lsp_window_to_the_model():
    import importlib.util
    spec = importlib.util.spec_from_file_location("evaluate_tool", os.path.join(os.path.dirname(GOLD), "..", "tools", "evaluate.py"))
    ev = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ev)
    args = ev.model_args(ev.parse_args(["--pairs", "1", "--lsp-window", "7", "--model-max-disp", "256"]))
    assert (args.lsp_width, args.lsp_height, args.max_disp) == (7, 7, 256)
    args = ev.model_args(ev.parse_args(["--pairs", "1"]))
    assert (args.lsp_width, args.lsp_height, args.max_disp) == (3, 3, 192)
    with pytest.raises(SystemExit):
        ev.parse_args(["--lsp-window", "9"])


def test_fixture_regenerates_bit_equal():
    sys.path.insert(0, GOLD)
    try:
        import make_golden as MG
    finally:
        sys.path.remove(GOLD)
    if not os.path.isdir(MG.REF):
        pytest.skip("the reference checkout the golden generators import is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_windows.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bit-equal" in r.stdout and "differing" not in r.stdout


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_fixture(name):
    win = META["cases"][name]["win"]
    got = affinity_ref(fixture_inputs()[0][0], win)
    assert tuple(got.shape) == (1, win * win - 1, 4, 6)
    close(got, torch.from_numpy(gold()[f"{name}__aff"]), 1e-5, 1e-6, name)


def test_restatement_equals_the_oracle_at_3x3():
    from oracle import ops as O
    x = fixture_inputs()[0][0]
    close(affinity_ref(x, 3), O.affinity(x.double()), 1e-12, 1e-12, "3x3")
