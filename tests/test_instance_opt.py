"""CPU: the surface of the registration's second stage (create_warp, run_instance_opt, warp_volume and their C ABI), and the
torch restatement tests/_instopt_ref.py against the fixtures captured from the reference's own functions in fp32
(tools/make_golden_instopt.py -> tests/golden/instopt_golden.npz).  The GPU kernels are held to the same restatement (in
float64) and fixtures in test_instance_opt_gpu.py."""
import inspect
import os

import numpy as np
import pytest
import torch

import _instopt_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "instopt_golden.npz"))
NEW_SYMBOLS = ("amx_instance_opt_smooth3", "amx_instance_opt_scratch_bytes", "amx_instance_opt_grad", "amx_instance_opt_adam_step",
               "amx_instance_opt", "amx_run_instance_opt_scratch_bytes", "amx_run_instance_opt", "amx_warp3d")
RUNS = [(c, n, 0) for c in IR.case_names() for n in IR.NITERS[c]] + [(IR.SMOOTH_CASE, IR.SMOOTH_NITER, 3), (IR.SMOOTH_CASE, IR.SMOOTH_NITER, 5)] \
    + [(c, 1, 0) for c in IR.NITER1_CASES]


def test_surface_has_the_reference_signatures():
    from anatomix_amd import _lib
    from anatomix_amd import registration as R
    sig = inspect.signature(R.run_instance_opt)
    assert list(sig.parameters) == ["disp_hr", "features_fix", "features_mov", "grid_sp_adam", "lambda_weight", "sizes",
                                    "selected_niter", "selected_smooth", "lr"]
    assert sig.parameters["lr"].default == 1
    assert list(inspect.signature(R.create_warp).parameters) == ["disp_hr", "sizes", "grid_sp_adam"]
    sig = inspect.signature(R.warp_volume)
    assert list(sig.parameters) == ["vol", "disp_hr", "mode"] and sig.parameters["mode"].default == "bilinear"
    assert list(inspect.signature(R.instance_opt_grad).parameters) == ["weight", "patch_fix", "patch_mov", "lambda_weight"]
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
    assert "instance_optimization.py:269-399" in header and "run_convex_adam_with_network_feats.py:238-266" in header


@pytest.mark.parametrize("case,niter,smooth", RUNS)
def test_restatement_is_the_reference(case, niter, smooth):
    """The fp32 restatement reproduces the reference's output bit for bit (the generator asserts it on the whole field; here
    on what the fixture keeps)."""
    disp, fix, mov = IR.inputs(case)
    out, _ = IR.run(disp, fix, mov, IR.CASES[case][3], IR.LAMBDA, niter, smooth)
    key = f"{case}|n{niter}|s{smooth}"
    if key + "|full" in G.files:
        assert np.array_equal(out, G[key + "|full"])
    else:
        assert np.array_equal(out.reshape(-1)[G[f"{case}|idx"].astype(np.int64)], G[key + "|val"])
    if niter > 1:
        assert float(G[key + "|ref_vs_f64"]) <= 1e-4


def test_fixture_conditions():
    assert float(G["far|out_of_range_share"]) >= 0.25
    assert float(G["warp|near_half_share"]) <= 0.005
    vol, lab, wd = IR.warp_inputs()
    assert np.array_equal(IR.warp(vol, wd, "bilinear"), G["warp|bilinear|full"])
    assert np.array_equal(IR.warp(lab, wd, "nearest"), G["warp|nearest|full"].astype(np.float32))
    assert abs(float(IR.near_half_mask(wd).mean()) - float(G["warp|near_half_share"])) < 1e-12


def test_argument_checks_come_before_any_library_call():
    """CPU tensors: every one of these must raise ValueError, not the RuntimeError that a CPU tensor gets once the arguments
    are accepted."""
    from anatomix_amd.registration import create_warp, instance_opt_grad, run_instance_opt, warp_volume
    disp, feat = torch.zeros(1, 3, 8, 8, 8), torch.zeros(1, 4, 8, 8, 8)
    for niter in (0, -3):
        with pytest.raises(ValueError, match="selected_niter"):
            run_instance_opt(disp, feat, feat, 2, 0.75, (8, 8, 8), niter, 0)
    with pytest.raises(ValueError, match="at least 2"):
        run_instance_opt(disp, feat, feat, 8, 0.75, (8, 8, 8), 5, 0)                 # a 1 x 1 x 1 grid
    with pytest.raises(ValueError, match="at least 2"):
        create_warp(disp, (8, 8, 8), 5)
    with pytest.raises(ValueError, match="grid_sp_adam"):
        run_instance_opt(disp, feat, feat, 0, 0.75, (8, 8, 8), 5, 0)
    with pytest.raises(ValueError, match="do not match"):
        run_instance_opt(disp, feat, torch.zeros(1, 5, 8, 8, 8), 2, 0.75, (8, 8, 8), 5, 0)
    with pytest.raises(ValueError, match="does not match"):
        run_instance_opt(torch.zeros(1, 3, 8, 8, 6), feat, feat, 2, 0.75, (8, 8, 8), 5, 0)
    with pytest.raises(ValueError, match="does not match"):
        run_instance_opt(disp, feat, feat, 2, 0.75, (8, 8, 10), 5, 0)
    with pytest.raises(ValueError):
        instance_opt_grad(torch.zeros(1, 3, 4, 4, 1), torch.zeros(1, 2, 4, 4, 1), torch.zeros(1, 2, 4, 4, 1), 0.75)
    with pytest.raises(ValueError):
        instance_opt_grad(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 2, 4, 4, 5), 0.75)
    with pytest.raises(ValueError, match="mode"):
        warp_volume(feat, disp, mode="bicubic")
    with pytest.raises(ValueError, match="do not match"):
        warp_volume(feat, torch.zeros(1, 3, 8, 8, 6))
    # accepted arguments on the CPU: there is no CPU path
    with pytest.raises(RuntimeError, match="GPU"):
        run_instance_opt(disp, feat, feat, 2, 0.75, (8, 8, 8), 5, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        warp_volume(feat, disp)
