"""CPU: the surface of the registration metrics and driver (label overlap / Dice, Jacobian determinant, convex_adam and its
command line), and the restatement tests/_regmetrics_ref.py against the fixtures captured from the reference's own functions and
from sklearn (tools/make_golden_regmetrics.py -> tests/golden/regmetrics_golden.npz, regdriver_cli.json).  The GPU kernels are
held to the same restatement (in float64) and fixtures in test_registration_metrics_gpu.py."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import _regmetrics_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
G = np.load(os.path.join(GOLD, "regmetrics_golden.npz"))
NEW_SYMBOLS = ("amx_label_overlap", "amx_jacobian_det_scratch_bytes", "amx_jacobian_det")


def test_header_table_and_library_agree():
    from anatomix_amd import _lib
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name
    assert "convex_adam_utils.py:226-282" in header and "run_convex_adam_with_network_feats.py:283-295" in header
    unit = open(os.path.join(ROOT, "anatomix_amd", "csrc", "amx_regmetrics.hip")).read()
    assert "launch_label_overlap(" in unit and "launch_jacobian_det(" in unit
    assert "amx_regmetrics" in open(os.path.join(ROOT, "anatomix_amd", "csrc", "Makefile")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name          # the built library exports it
        assert name.replace("_scratch_bytes", "") in integration, name      # the table writes `name(_scratch_bytes)`


def test_surface():
    from anatomix_amd import registration as R
    assert list(inspect.signature(R.generate_grid).parameters) == ["imgshape"]
    assert list(inspect.signature(R.JacobianDet).parameters) == ["y_pred", "sample_grid"]
    sig = inspect.signature(R.jacobian_determinant)
    assert list(sig.parameters) == ["disp_hr", "return_stats"] and sig.parameters["return_stats"].default is False
    sig = inspect.signature(R.label_overlap)
    assert list(sig.parameters) == ["a", "b", "bins"] and sig.parameters["bins"].default == 1024
    assert list(inspect.signature(R.dice_score).parameters) == ["fixed_seg", "moved_seg"]
    sig = inspect.signature(R.convex_adam)
    want = ["expname", "lambda_weight", "grid_sp", "disp_hw", "selected_niter", "selected_smooth", "ckpt_path", "hf_variant",
            "grid_sp_adam", "ic", "result_path", "fixed_image", "moving_image", "use_mask", "fixed_mask", "moving_mask",
            "fixed_minclip", "fixed_maxclip", "moving_minclip", "moving_maxclip", "warp_seg", "fixed_seg", "moving_seg",
            "downscale_feat_scalar", "num_downs", "ngf", "output_nc", "norm", "interp", "pooling", "model", "weights_path"]
    assert list(sig.parameters) == want
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(ckpt_path=None, hf_variant=None, grid_sp_adam=2, ic=True, result_path='./', fixed_image=None,
                            moving_image=None, use_mask=False, fixed_mask=None, moving_mask=None, fixed_minclip=None,
                            fixed_maxclip=None, moving_minclip=None, moving_maxclip=None, warp_seg=False, fixed_seg=None,
                            moving_seg=None, downscale_feat_scalar=0.1, num_downs=4, ngf=16, output_nc=16, norm="batch",
                            interp="nearest", pooling="Max", model=None, weights_path=None)
    assert [k for k, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == ["model", "weights_path"]
    sig = inspect.signature(R.register_volumes)
    assert list(sig.parameters)[:3] == ["fixedim", "movingim", "model"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in list(sig.parameters.items())[3:])
    assert sig.parameters["grid_sp_adam"].default == 2 and sig.parameters["ic"].default is True
    assert sig.parameters["downscale_feat_scalar"].default == 0.1


@pytest.mark.parametrize("shape", MR.GRID_SHAPES)
def test_generate_grid(shape):
    from anatomix_amd.registration import generate_grid
    want = G["grid|{}x{}x{}".format(*shape)]
    for got in (MR.generate_grid(shape), generate_grid(shape)):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _recorded(key, arr):
    """(values of arr where the fixture has them, the fixture's values)"""
    if key + "|full" in G.files:
        return arr, G[key + "|full"]
    return arr.reshape(-1)[G[key + "|idx"]], G[key + "|val"]


@pytest.mark.parametrize("shape,kind", MR.jac_cases())
@pytest.mark.parametrize("ident", [0, 1])
def test_jacobian_restatement_and_cpu_path_are_the_reference(shape, kind, ident):
    """fp32 on the CPU: the restatement and the package's JacobianDet reproduce the recorded reference values bit for bit; the
    float64 restatement is the determinant of the forward differences in axis order, which is what the kernel's header promises."""
    from anatomix_amd.registration import JacobianDet
    disp = MR.jac_field(shape, kind)
    key = MR.jac_key(shape, kind, ident)
    y, grid = MR.reference_inputs(disp, ident)
    for fn in (MR.jacobian_det, JacobianDet):
        got, want = _recorded(key, fn(y, grid)[0].numpy())
        assert got.dtype == np.float32 and np.array_equal(got, want)
    j64 = MR.jacobian_f64(disp, ident)
    assert int((j64 <= 0).sum()) == int(G[key + "|nonpos64"])
    assert np.allclose(MR.jacobian_stats(j64), G[key + "|stats64"], rtol=1e-12, atol=0, equal_nan=True)
    u = disp.astype(np.float64)
    base = u[:, :-1, :-1, :-1]
    m = np.stack([u[:, 1:, :-1, :-1] - base, u[:, :-1, 1:, :-1] - base, u[:, :-1, :-1, 1:] - base], axis=-1)    # [b, ..., A]
    m = np.moveaxis(m, 0, -2) + (np.eye(3) if ident else 0.0)                                                  # [..., b, A]
    assert np.abs(np.linalg.det(m) - j64).max() <= 1e-12 * max(1.0, np.abs(j64).max())


def test_jacobiandet_accepts_the_numpy_grid():
    from anatomix_amd.registration import JacobianDet, generate_grid
    y, grid = MR.reference_inputs(MR.jac_field((5, 3, 2), "fold"), 1)
    assert torch.equal(JacobianDet(y, generate_grid((5, 3, 2))), MR.jacobian_det(y, grid))
    with pytest.raises(ValueError):
        JacobianDet(torch.zeros(1, 4, 4, 1, 3), generate_grid((4, 4, 1)))


@pytest.mark.parametrize("case", MR.DICE_CASES)
def test_dice_from_counts_is_sklearn(case):
    from anatomix_amd.registration import dice_from_counts
    fix, mov = MR.dice_pair(case)
    counts, bad = MR.overlap_counts(fix, mov, 1024)
    assert bad == 0
    want = float(G["dice|" + case])
    for fn, c in ((MR.dice_from_counts, counts), (dice_from_counts, torch.from_numpy(counts))):
        got, per = fn(c)
        assert abs(got - want) <= 1e-12, (got, want)
        assert sorted(per) == sorted(np.unique(fix).astype(int).tolist()[1:])


def test_dice_needs_a_label_beyond_the_smallest():
    from anatomix_amd.registration import dice_from_counts
    counts = torch.zeros(8, 3, dtype=torch.int64)
    counts[3] = torch.tensor([10, 10, 10])
    with pytest.raises(ValueError, match="no label"):
        dice_from_counts(counts)


def test_overlap_argument_checks_need_no_gpu():
    from anatomix_amd.registration import label_overlap
    with pytest.raises(ValueError, match="bins"):
        label_overlap(torch.zeros(4), torch.zeros(4), bins=0)
    with pytest.raises(ValueError, match="bins"):
        label_overlap(torch.zeros(4), torch.zeros(4), bins=1025)
    with pytest.raises(RuntimeError, match="GPU"):
        label_overlap(torch.zeros(4), torch.zeros(4))


def test_parser_is_the_reference_parser():
    from anatomix_amd.registration import build_parser
    want = json.load(open(os.path.join(GOLD, "regdriver_cli.json")))
    got = MR.describe_parser(build_parser())
    assert len(want["flags"]) == 29
    assert [f["dest"] for f in got["flags"]] == [f["dest"] for f in want["flags"]]
    for g, w in zip(got["flags"], want["flags"]):
        assert g == w, (g, w)
    assert got["exclusive_groups"] == want["exclusive_groups"] == [{"required": True, "dests": ["ckpt_path", "hf_variant"]}]
    p = build_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["--fixed", "f", "--moving", "m", "--exp_name", "e"])                                  # no weights source
    with pytest.raises(SystemExit):
        p.parse_args(["--fixed", "f", "--moving", "m", "--exp_name", "e", "--ckpt_path", "c", "--hf_variant", "anatomix"])
    a = p.parse_args(["--fixed", "f", "--moving", "m", "--exp_name", "e", "--ckpt_path", "c", "--no-ic"])
    assert a.ic is False and a.selected_niter == 80 and a.lambda_weight == 0.75 and a.disp_hw == 1


def test_result_names():
    from anatomix_amd.registration import result_names
    assert result_names("/data/x.nii.gz", 2, 1, 0.75, 2, True, "run") == (
        "disp_x_g2_hw1_l0.75_ga2_icTrue_run.nii.gz", "moved_x_g2_hw1_l0.75_ga2_icTrue_run.nii.gz",
        "labels_moved_x_g2_hw1_l0.75_ga2_icTrue_run.nii.gz")
    assert result_names("x.nii", 4, 3, 1.0, 1, False, "e")[0] == "disp_x_g4_hw3_l1.0_ga1_icFalse_e.nii.gz"
    assert result_names("dir/a.b.nii.gz", 2, 2, 0.5, 2, True, "e")[1] == "moved_a.b_g2_hw2_l0.5_ga2_icTrue_e.nii.gz"
    assert result_names("a.b.nii", 2, 2, 0.5, 2, True, "e")[2] == "labels_moved_a.b_g2_hw2_l0.5_ga2_icTrue_e.nii.gz"


def test_convex_adam_argument_errors_come_before_any_work():
    from anatomix_amd.registration import convex_adam
    base = dict(expname="e", lambda_weight=0.75, grid_sp=2, disp_hw=1, selected_niter=5, selected_smooth=0,
                fixed_image="missing_fixed.nii.gz", moving_image="missing_moving.nii.gz")
    with pytest.raises(ValueError, match="exactly one"):
        convex_adam(**base)                                                                   # neither
    with pytest.raises(ValueError, match="exactly one"):
        convex_adam(**base, ckpt_path="a.pth", hf_variant="anatomix")                         # both
    with pytest.raises(ValueError, match="warp_seg"):
        convex_adam(**base, ckpt_path="a.pth", warp_seg=True, fixed_seg="s.nii.gz")
    with pytest.raises(ValueError, match="use_mask"):
        convex_adam(**base, ckpt_path="a.pth", use_mask=True, moving_mask="m.nii.gz")
    with pytest.raises(ValueError, match="required"):
        convex_adam("e", 0.75, 2, 1, 5, 0, ckpt_path="a.pth")
    with pytest.raises(FileNotFoundError):
        convex_adam(**base, ckpt_path="no_such_checkpoint.pth")
