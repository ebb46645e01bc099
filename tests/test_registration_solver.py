"""CPU: the surface of the registration's discrete stage (coupled_convex, inverse_consistency, run_stage1_registration and
their C ABI), and the numpy restatement tests/_solver_ref.py against the fixtures captured from the reference's own
functions in fp32 (tools/make_golden_solver.py -> tests/golden/solver_golden.npz).  The GPU kernels are held to the same
restatement and fixtures in test_registration_solver_gpu.py."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _solver_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "solver_golden.npz"))
CASES = SR.case_names()
NEW_SYMBOLS = ("amx_coupled_convex", "amx_coupled_convex_scratch_bytes", "amx_coupled_convex_step",
               "amx_coupled_convex_step_scratch_bytes", "amx_inverse_consistency", "amx_inverse_consistency_scratch_bytes",
               "amx_resize_trilinear3d", "amx_stage1_registration", "amx_stage1_registration_scratch_bytes")


def regular_mesh(hw, dtype=torch.float32):
    k = 2 * hw + 1
    return F.affine_grid(hw * torch.eye(3, 4).unsqueeze(0), (1, 1, k, k, k), align_corners=True) \
        .permute(0, 4, 1, 2, 3).reshape(3, -1, 1).to(dtype)


def test_surface_has_the_reference_signatures():
    from anatomix_amd import _lib
    from anatomix_amd.registration import coupled_convex, inverse_consistency, run_stage1_registration
    assert list(inspect.signature(coupled_convex).parameters) == ["ssd", "ssd_argmin", "disp_mesh_t", "grid_sp", "shape"]
    sig = inspect.signature(inverse_consistency)
    assert list(sig.parameters) == ["disp_field1s", "disp_field2s", "iterations"]
    assert sig.parameters["iterations"].default == 20
    assert [p.default for p in list(sig.parameters.values())[:2]] == [inspect.Parameter.empty] * 2
    sig = inspect.signature(run_stage1_registration)
    assert list(sig.parameters) == ["features_fix_smooth", "features_mov_smooth", "disp_hw", "grid_sp", "sizes", "n_ch", "ic"]
    assert all(p.default is inspect.Parameter.empty for p in sig.parameters.values())
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert name + "(" in header, name


def test_label_order_of_the_mesh():
    """The kernel generates mesh[m] = (m % k, (m / k) % k, m / k^2) - disp_hw; that is the order (and, up to the rounding of
    affine_grid's linspace, the values) of the mesh run_stage1_registration builds."""
    for hw in (1, 2, 3):
        assert np.abs(SR.mesh(hw) - regular_mesh(hw).reshape(3, -1).numpy()).max() < 1e-6


@pytest.mark.parametrize("case", CASES)
def test_restatement_coupled_convex_against_reference(case):
    """Discrete: a voxel disagrees if any component differs by more than 1e-4 (one flipped label moves 27 outputs by at
    least 1/27).  Share of disagreeing voxels <= 27 x (share of voxels with a margin below 1e-5 in any iteration), and never
    above 1 %."""
    for tag, rev in (("fwd", False), ("bwd", True)):
        ssd, amin, hw, g, sizes = SR.ssd_of(case, rev)
        keep = ssd.copy()
        soft, aux = SR.coupled_convex(ssd, amin)
        assert np.array_equal(ssd, keep)
        want = G[f"{case}|{tag}|soft_x27"].astype(np.float32) / np.float32(27)
        near, dis = SR.near_tie_share(aux["margins"]), SR.disagree_share(soft, want)
        print(f"{case}|{tag}: near-tie share {near:.3e} disagree {dis:.3e} (generator: {float(G[f'{case}|{tag}|near_tie_share']):.3e}, "
              f"{float(G[f'{case}|{tag}|ref_disagree']):.3e})")
        assert dis <= 27 * near and dis <= 0.01
        assert np.abs(soft).max() <= hw + 1e-4


@pytest.mark.parametrize("case", CASES)
def test_restatement_continuous_parts_against_reference(case):
    """inverse_consistency and the resize: max abs error <= 2e-6 x max|reference| (fp32 stencils)."""
    fix, _, hw, g, sizes = SR.features(case)
    h, w, d = fix.shape[1:]
    a, b = SR.smooth_fields((h, w, d), 7, 6.0 / max(h, w, d))
    for it in (1, 15):
        got = dict(zip("ab", SR.inverse_consistency(a, b, it)))
        for nm in "ab":
            idx, want = G[f"{case}|ic{it}|{nm}|idx"], G[f"{case}|ic{it}|{nm}|val"]
            e = np.abs(got[nm].reshape(-1)[idx] - want).max()
            print(f"{case}|ic{it}|{nm}: max abs {e:.3e} of max|ref| {np.abs(want).max():.3e}")
            assert e <= 2e-6 * np.abs(want).max()
            key = f"{case}|ic{it}|{nm}|full"
            if key in G.files:
                assert np.abs(got[nm] - G[key]).max() <= 2e-6 * np.abs(G[key]).max()
    scale = np.array([h - 1, w - 1, d - 1], np.float32) / 2 * g
    for nm, size in (("up", tuple(sizes)), ("odd", (h + 3, 2 * w - 1, d - 2))):
        got = SR.resize_trilinear(a, size, scale, flip=True)
        idx, want = G[f"{case}|resize_{nm}|idx"], G[f"{case}|resize_{nm}|val"]
        e = np.abs(got.reshape(-1)[idx] - want).max()
        print(f"{case}|resize_{nm}: max abs {e:.3e} of max|ref| {np.abs(want).max():.3e}")
        assert e <= 2e-6 * np.abs(want).max()


@pytest.mark.parametrize("case", CASES)
def test_restatement_stage1_against_reference(case):
    """run_stage1_registration: ic=False is the discrete field (share criterion); ic=True continues it through the sweeps and
    the upsampling (continuous bound; the reference ran its own correlate, the restatement the oracle's)."""
    fix, mov, hw, g, sizes = SR.features(case)
    soft = SR.run_stage1(fix, mov, hw, g, sizes, False)
    want = G[f"{case}|stage1|soft_x27"].astype(np.float32) / np.float32(27)
    assert soft.shape == want.shape
    dis = SR.disagree_share(soft, want)
    near = max(float(G[f"{case}|fwd|near_tie_share"]), 0.0)
    print(f"{case}|stage1 ic=False: disagree {dis:.3e}, near-tie share {near:.3e}")
    assert dis <= 27 * near and dis <= 0.01
    hr = SR.run_stage1(fix, mov, hw, g, sizes, True)
    assert hr.shape == (3,) + tuple(sizes)
    idx, val = G[f"{case}|stage1_ic|idx"], G[f"{case}|stage1_ic|val"]
    e = np.abs(hr.reshape(-1)[idx] - val).max()
    print(f"{case}|stage1 ic=True: max abs {e:.3e} of max|ref| {np.abs(val).max():.3e}")
    assert e <= 2e-6 * np.abs(val).max()


def test_cpu_tensors_and_irregular_meshes_are_refused():
    from anatomix_amd.registration import coupled_convex, inverse_consistency, run_stage1_registration
    ssd = torch.rand(27, 4, 5, 6)
    amin = ssd.argmin(0)
    with pytest.raises(RuntimeError, match="GPU"):
        coupled_convex(ssd, amin, regular_mesh(1), 2, (8, 10, 12))
    with pytest.raises(RuntimeError, match="GPU"):
        inverse_consistency(torch.zeros(1, 3, 4, 5, 6), torch.zeros(1, 3, 4, 5, 6))
    with pytest.raises(RuntimeError, match="GPU"):
        run_stage1_registration(torch.rand(1, 4, 4, 5, 6), torch.rand(1, 4, 4, 5, 6), 1, 2, (8, 10, 12), 4, True)
    for bad in (regular_mesh(1) * 0.5, regular_mesh(2), regular_mesh(1).flip(1), torch.zeros(3, 27, 1)):
        with pytest.raises(ValueError, match="regular"):
            coupled_convex(ssd, amin, bad, 2, (8, 10, 12))
    with pytest.raises(ValueError):
        coupled_convex(torch.rand(28, 4, 5, 6), None, regular_mesh(1), 2, (8, 10, 12))
    # the half mesh of the reference's own caller is the same regular mesh
    with pytest.raises(RuntimeError, match="GPU"):
        coupled_convex(ssd, amin, regular_mesh(1, torch.float16), 2, (8, 10, 12))
