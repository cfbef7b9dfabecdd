"""CPU: disparity ranges above 256 (geometry volumes of D = max_disp / 4 > 64) without a device.

  * oracle/model.py at max_disp 384 and 768 against tests/golden/model_igev_large_disp.npz (the imported reference) under the
    project's parity bar of 1e-3 px: the fixture and the bar are attainable by the reference arithmetic alone;
  * the fixture's generator reproduces the stored arrays bit for bit (needs the reference checkout the generator imports: without
    it nothing can be regenerated and the test skips);
  * the fixture's volume arrays (geometry encoding volume, gwc volume beyond d = 64) against the oracle, and that they notice a
    volume cut at d = 64, which the outputs do not;
  * tools/evaluate.py hands --model-max-disp to the model's arguments; tools/codegen_diff.py::symbols;
  * as_gwc_volume_fwd / as_geo_pyramid return their documented codes for null pointers and oversized shapes before any launch.
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ops as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("tag", ["A", "B"])
def test_oracle_model_large_disp_vs_reference(tag, golden):
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    from oracle.model import OracleIGEV
    g = golden("model_igev_large_disp")
    max_disp, H, W, shift, seed = (int(v) for v in g[f"{tag}_case"])
    args = default_args("continuous_IGEVStereo", max_disp=max_disp)
    model = __models__["continuous_IGEVStereo"](args).eval()
    fill_module_deterministic(model, base_seed=1)
    ref = OracleIGEV(args).eval()
    ref.load_state_dict(model.state_dict())
    img1, img2 = synthetic_pair(1, H, W, shift=shift, seed=seed)
    ran = 0
    with torch.no_grad():
        for s, k in ((1.0, "1p0"), (1.5, "1p5")):
            if f"{tag}_test_{k}" not in g:
                continue
            coord = O.make_coord([round(H * s), round(W * s)]).view(1, -1, 2)
            up = ref(img1, img2, iters=3, test_mode=True, hr_coord=coord.clone(), scale=torch.tensor([[s]]))
            want = g[f"{tag}_test_{k}"]
            assert up.shape == want.shape
            epe = (up - want).abs().mean().item()
            assert epe < 1e-3, f"shape {tag} scale {s}: oracle vs reference {epe:.3e} (bar 1e-3)"
            ran += 1
        coord = O.make_coord([H, W]).view(1, -1, 2)
        init_disp, _ = ref(img1, img2, iters=1, test_mode=False, hr_coord=coord.clone(), scale=torch.tensor([[1.0]]))
        assert init_disp.shape == g[f"{tag}_init_disp"].shape
        assert (init_disp - g[f"{tag}_init_disp"]).abs().mean().item() < 1e-3
    assert ran == (2 if tag == "A" else 1)


def test_large_disp_fixture_regenerates_bit_equal():
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden as MG
    finally:
        sys.path.remove(GOLDEN)
    if not os.path.isdir(MG.REF):
        pytest.skip("the reference checkout the golden generators import is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_large_disp.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bit-equal" in r.stdout and "differing" not in r.stdout


def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(os.path.dirname(GOLDEN), "..", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_evaluate_tool_hands_model_max_disp_to_the_model():
    """tools/evaluate.py --model-max-disp N reaches the model's construction arguments; --max-disp stays the evaluator's."""
    ev = _load_tool("evaluate")
    a = ev.parse_args(["--pairs", "1", "--model-max-disp", "384", "--max-disp", "100"])
    assert a.model_max_disp == 384 and a.max_disp == 100.0
    assert ev.model_args(a).max_disp == 384
    a = ev.parse_args(["--pairs", "1", "--max-disp", "100"])
    assert a.model_max_disp is None and ev.model_args(a).max_disp == 192
    a = ev.parse_args(["--model", "continuous_RAFTStereo"])
    assert ev.model_args(a).max_disp == 700


@pytest.mark.parametrize("tag", ["A", "B"])
def test_oracle_volumes_large_disp_vs_reference(tag, golden):
    """The fixture's arrays that DO depend on the volume beyond d = 64 (the outputs hardly do, see make_golden_large_disp.py): the
    geometry encoding volume and the d >= 64 part of the gwc volume, oracle against the imported reference at the bound
    test_preloop_tensors_vs_oracle holds (2e-4 of the tensor's maximum); and the check notices a volume whose d >= 64 is
    zeroed."""
    from _preloop import capture_preloop, check_preloop
    from anystereo.harness.synthetic import fill_module_deterministic, synthetic_pair
    from anystereo.models import __models__, default_args
    from oracle.model import OracleIGEV
    g = golden("model_igev_large_disp")
    max_disp, H, W, shift, seed = (int(v) for v in g[f"{tag}_case"])
    args = default_args("continuous_IGEVStereo", max_disp=max_disp)
    model = __models__["continuous_IGEVStereo"](args).eval()
    fill_module_deterministic(model, base_seed=1)
    img1, img2 = synthetic_pair(1, H, W, shift=shift, seed=seed)
    coord = O.make_coord([H, W]).view(1, -1, 2)

    class Cut(OracleIGEV):
        def _hot_gwc(self, match_left, match_right):
            v = super()._hot_gwc(match_left, match_right).clone()
            v[:, :, 64:] = 0
            return v

    def volumes(cls):
        ref = cls(args).eval()
        ref.load_state_dict(model.state_dict())
        cap = capture_preloop(ref, img1, img2, coord, torch.tensor([[1.0]]))
        gwc = OracleIGEV._hot_gwc(ref, cap["match_left"], cap["match_right"])
        return {"gev": cap["gev"], "gwc_hi": gwc[:, :, 64:].contiguous().float()}

    worst = check_preloop(volumes(OracleIGEV), g, tag, 2e-4, "oracle")
    print(f"[large disp oracle {tag}] " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    if tag == "A":  # shape B: W/4 = 32, every d >= 64 is zeros in the reference too
        assert float(g["A.gwc_hi.sums"][1]) > 0
        cut = volumes(Cut)["gev"].reshape(-1)[::int(g["stride"])]
        moved = (cut.double() - g["A.gev"].double()).abs().max().item() / g["A.gev"].abs().max().item()
        print(f"[large disp oracle A] gev with d >= 64 of the gwc volume zeroed: {moved:.1e} of its maximum")
        # measured 4.9e-2; what matters is an order of magnitude above the 5e-4 that test_preloop_tensors_vs_reference allows the GPU
        assert moved > 10 * 5e-4, f"A.gev moves by only {moved:.2e} when d >= 64 of the gwc volume is zeroed"


def test_codegen_diff_ignores_a_functions_place_in_its_file():
    """tools/codegen_diff.py::symbols hashes a function's assembly without its index in the file (local labels, the loop
    comments that repeat it, and their column padding), and still tells two instruction streams apart."""
    cd = _load_tool("codegen_diff")

    def asm(idx, insn, pad):
        return (f"\t.globl\tk ; -- Begin function k\nk:\n\ts_load_dword s0, s[4:5], 0x0\n.LBB{idx}_1:{pad}; =>This Inner Loop Header: Depth=1\n"
                f"\t{insn}\n\ts_cbranch_scc1 .LBB{idx}_1\n; %bb.2:{pad};   in Loop: Header=BB{idx}_1 Depth=1\n\ts_endpgm\n.Lfunc_end{idx}:\n"
                "\t; -- End function\n")

    def sym(text, tmp=[0]):
        import tempfile
        with tempfile.NamedTemporaryFile("w", suffix=".s", delete=False) as f:
            f.write(text)
        try:
            return cd.symbols(f.name)
        finally:
            os.unlink(f.name)

    a, b, c = sym(asm(4, "v_add_f32 v0, v0, v1", " " * 23)), sym(asm(12, "v_add_f32 v0, v0, v1", " " * 22)), sym(asm(4, "v_sub_f32 v0, v0, v1", " " * 23))
    assert list(a) == ["k"] and a == b and a != c


def test_volume_entry_points_validate_without_gpu():
    """Host-side checks of as_gwc_volume_fwd / as_geo_pyramid run before any launch: null pointers, sizes, and today's limits on D
    (gwc: D <= 64; geo pyramid: G*D*33*4 B <= 160 KiB).  -1 = AS_ERR_BAD_ARG, -2 = AS_ERR_BAD_SHAPE."""
    import ctypes
    from anystereo import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)
    err = lambda: lib.as_last_error_string().decode()  # noqa: E731
    assert lib.as_gwc_volume_fwd(None, one, one, 1, 96, 2, 70, 48, 8, None) == -1 and "null" in err()
    assert lib.as_gwc_volume_fwd(one, one, None, 1, 96, 2, 70, 48, 8, None) == -1
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 96, 2, 70, 0, 8, None) == -1
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 96, 2, 70, 65, 8, None) == -2 and "D=65" in err()
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 96, 2, 70, 96, 8, None) == -2 and "D=96" in err()
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 96, 2, 70, 48, 6, None) == -2                      # G % 4
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 80, 2, 70, 48, 4, None) == -2                      # C/G = 20
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 128, 2, 70, 64, 16, None) == -2 and "LDS slab" in err()
    assert lib.as_gwc_volume_fwd(one, one, one, 2, 96, 40000, 70, 48, 8, None) == -2 and "B*H" in err()
    assert lib.as_gwc_volume_fwd(one, one, one, 1, 96, 3000, 2000, 48, 8, None) == -2 and "32-bit" in err()
    lv, keep = _lib.ptr_array([16, 16, 16, 16])
    nul, keep2 = _lib.ptr_array([16, 0])
    assert lib.as_geo_pyramid(None, lv, 1, 8, 48, 2, 37, 2, None) == -1 and "null" in err()
    assert lib.as_geo_pyramid(one, None, 1, 8, 48, 2, 37, 2, None) == -1
    assert lib.as_geo_pyramid(one, nul, 1, 8, 48, 2, 37, 2, None) == -1 and "null level 1" in err()
    assert lib.as_geo_pyramid(one, lv, 1, 8, 48, 2, 37, 5, None) == -1
    assert lib.as_geo_pyramid(one, lv, 1, 8, 4, 2, 37, 4, None) == -1                                 # D >> (L-1) == 0
    assert lib.as_geo_pyramid(one, lv, 1, 8, 156, 2, 37, 2, None) == -2 and "160 KiB" in err()        # G*D = 1248 > 1240
    assert lib.as_geo_pyramid(one, lv, 1, 8, 192, 2, 37, 2, None) == -2 and "G*D=1536" in err()
    assert lib.as_geo_pyramid(one, lv, 2, 8, 48, 40000, 37, 2, None) == -2 and "B*H" in err()
    assert lib.as_geo_pyramid(one, lv, 1, 8, 155, 1000, 1000, 2, None) == -2 and "1.75 GiB" in err()
