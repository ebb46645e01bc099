"""GPU: coupled_convex, inverse_consistency, the trilinear resize and run_stage1_registration through the C ABI
(csrc/amx_regsolve.hip) against the numpy restatement (tests/_solver_ref.py) and the fixtures captured from the reference's
own functions in fp32 (tools/make_golden_solver.py -> tests/golden/solver_golden.npz).

Bounds.  Continuous kernels: max abs error <= 5e-6 x max|reference| (fp32 with a different summation order).  The discrete
solver: a voxel DISAGREES if any component differs by more than 1e-4; the share of disagreeing voxels must be at most
27 x (share of voxels whose margin in the restatement is below 1e-5 in any iteration) and never above 1 %."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _solver_ref as SR

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "solver_golden.npz"))
CASES = SR.case_names()


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def regular_mesh(hw, dtype=torch.float32):
    k = 2 * hw + 1
    return F.affine_grid(hw * torch.eye(3, 4).unsqueeze(0), (1, 1, k, k, k), align_corners=True) \
        .permute(0, 4, 1, 2, 3).reshape(3, -1, 1).to(dtype)


def assert_discrete(got, want, near, what):
    dis = SR.disagree_share(got, want)
    print(f"{what}: disagree {dis:.3e}, near-tie share {near:.3e}")
    assert dis <= 27 * near and dis <= 0.01, what


def assert_close(got, want, what, rel=5e-6):
    e = float(np.abs(np.asarray(got, np.float32) - want).max())
    print(f"{what}: max abs {e:.3e} of max|ref| {np.abs(want).max():.3e}")
    assert e <= rel * np.abs(want).max(), what


@pytest.mark.parametrize("case", CASES)
def test_coupled_convex_against_restatement_and_reference(case):
    from anatomix_amd.registration import coupled_convex
    for tag, rev in (("fwd", False), ("bwd", True)):
        ssd, amin, hw, g, sizes = SR.ssd_of(case, rev)
        want, aux = SR.coupled_convex(ssd, amin)
        near = SR.near_tie_share(aux["margins"])
        d_ssd, d_amin = cu(ssd), cu(amin)
        keep = d_ssd.clone()
        got = coupled_convex(d_ssd, d_amin, regular_mesh(hw).to(dev()), g, sizes)
        assert got.shape == (1, 3) + ssd.shape[1:] and got.dtype == torch.float32
        assert torch.equal(d_ssd, keep)                                    # documented difference: ssd is not modified
        assert_discrete(got[0].cpu().numpy(), want, near, f"{case}|{tag} vs restatement")
        ref = G[f"{case}|{tag}|soft_x27"].astype(np.float32) / np.float32(27)
        assert_discrete(got[0].cpu().numpy(), ref, near, f"{case}|{tag} vs reference fixture")
        assert got.abs().max().item() <= hw + 1e-4
        # the argmin recomputed on the device, and the half mesh of the reference's own caller: same result
        assert torch.equal(coupled_convex(d_ssd, None, regular_mesh(hw, torch.float16), g, sizes), got)


@pytest.mark.parametrize("case", CASES)
def test_coupled_convex_teacher_forced(case):
    """One iteration from the restatement's state picks the restatement's label at every voxel whose margin is >= 1e-5: an
    error cannot hide behind the coupling.  No allowance."""
    from anatomix_amd.registration import coupled_convex_step
    ssd, amin, hw, g, sizes = SR.ssd_of(case)
    _, aux = SR.coupled_convex(ssd)
    d_ssd = cu(ssd)
    for j in range(7):
        lab, soft = coupled_convex_step(d_ssd, [cu(s)[None] for s in aux["soft"][:j]])
        clear = aux["margins"][j] >= 1e-5
        wrong = int(((lab.cpu().numpy() != aux["labels"][j]) & clear).sum())
        print(f"{case} iteration {j}: {int(clear.sum())} of {clear.size} voxels with a clear margin, {wrong} wrong labels")
        assert wrong == 0
        if clear.all():
            assert np.abs(soft[0].cpu().numpy() - aux["soft"][j]).max() <= 1e-6


@pytest.mark.parametrize("case", CASES)
def test_inverse_consistency_and_resize_against_reference(case):
    from anatomix_amd.registration import inverse_consistency, resize_trilinear
    fix, _, hw, g, sizes = SR.features(case)
    h, w, d = fix.shape[1:]
    a, b = SR.smooth_fields((h, w, d), 7, 6.0 / max(h, w, d))
    da, db = cu(a)[None], cu(b)[None]
    ka, kb = da.clone(), db.clone()
    for it in (1, 15):
        ga, gb = inverse_consistency(da, db, iterations=it)
        assert torch.equal(da, ka) and torch.equal(db, kb)
        ma, mb = SR.inverse_consistency(a, b, it)
        for nm, got, mine in (("a", ga, ma), ("b", gb, mb)):
            got = got[0].cpu().numpy()
            assert_close(got.reshape(-1)[G[f"{case}|ic{it}|{nm}|idx"]], G[f"{case}|ic{it}|{nm}|val"], f"{case}|ic{it}|{nm} fixture")
            assert_close(got, mine, f"{case}|ic{it}|{nm} restatement")
    scale = np.array([h - 1, w - 1, d - 1], np.float32) / 2 * g
    for nm, size in (("up", tuple(sizes)), ("odd", (h + 3, 2 * w - 1, d - 2))):
        got = resize_trilinear(da, size, scale, flip_channels=True)[0].cpu().numpy()
        assert got.shape == (3,) + tuple(size)
        assert_close(got.reshape(-1)[G[f"{case}|resize_{nm}|idx"]], G[f"{case}|resize_{nm}|val"], f"{case}|resize_{nm} fixture")
        assert_close(got, SR.resize_trilinear(a, size, scale, flip=True), f"{case}|resize_{nm} restatement")


def test_ragged_sizes_against_restatement():
    from anatomix_amd.registration import coupled_convex, inverse_consistency, resize_trilinear
    rs = np.random.RandomState(3)
    for shape in ((5, 8, 16), (9, 17, 33), (31, 7, 19), (2, 3, 5)):
        # displacements of up to a third of the volume: part of the samples fall outside (zero padding)
        a, b = SR.smooth_fields(shape, 11 + shape[0], 2.5)
        for it in (0, 1, 2, 5):
            ga, gb = inverse_consistency(cu(a)[None], cu(b)[None], it)
            ma, mb = SR.inverse_consistency(a, b, it)
            assert_close(ga[0].cpu().numpy(), ma, f"ic {shape} x{it} a")
            assert_close(gb[0].cpu().numpy(), mb, f"ic {shape} x{it} b")
        x = rs.randn(5, *shape).astype(np.float32)
        for size in ((shape[0] * 2, shape[1] * 2, shape[2] * 2), (7, 5, 3), (shape[0], shape[1], shape[2]), (1, 40, 9)):
            for flip, scale in ((False, None), (True, None), (True, [1.5, -2.0, 0.25, 3.0, 1.0])):
                got = resize_trilinear(cu(x)[None], size, scale, flip)[0].cpu().numpy()
                assert_close(got, SR.resize_trilinear(x, size, scale, flip), f"resize {shape} -> {size} flip {flip}")
            want = F.interpolate(torch.from_numpy(x)[None], size=size, mode="trilinear", align_corners=False)[0].numpy()
            assert_close(resize_trilinear(cu(x)[None], size)[0].cpu().numpy(), want, f"resize {shape} -> {size} vs F.interpolate")
        for hw in (1, 2, 3):
            ssd = rs.rand((2 * hw + 1) ** 3, *shape).astype(np.float32)
            ssd = SR.box3(SR.box3(ssd))
            want, aux = SR.coupled_convex(ssd)
            got = coupled_convex(cu(ssd), None, SR_mesh(hw), 1, shape)[0].cpu().numpy()
            assert_discrete(got, want, SR.near_tie_share(aux["margins"]), f"coupled {shape} hw {hw}")


def SR_mesh(hw):
    return torch.from_numpy(SR.mesh(hw)).reshape(3, -1, 1)


def test_known_answer_rolled_features():
    """The moving features are the fixed ones rolled by ROLL grid cells plus noise.  The three figures are conditions on the
    input that the reference's own fp32 output meets (tools/make_golden_solver.py asserts them)."""
    from anatomix_amd.registration import run_stage1_registration
    fix, mov, hw, g, sizes = SR.features("roll48")
    df, dm = cu(fix)[None], cu(mov)[None]
    roll = torch.tensor(SR.ROLL, dtype=torch.float32, device=dev()).view(1, 3, 1, 1, 1)
    soft = run_stage1_registration(df, dm, hw, g, sizes, fix.shape[0], False)
    assert soft.shape == (1, 3, 48, 48, 48)
    ok = ((soft - roll).abs()[..., 4:-4, 4:-4, 4:-4] <= 0.05).all(1).float().mean().item()
    print(f"ic=False: within 0.05 grid units of the roll on {ok:.5f} of the interior")
    assert ok >= 0.99
    hr = run_stage1_registration(df, dm, hw, g, sizes, fix.shape[0], True)
    assert hr.shape == (1, 3) + tuple(sizes)
    c = 4 * g
    e_up = (hr - g * roll).abs()[..., c:-c, c:-c, c:-c].max().item()
    rev = run_stage1_registration(dm, df, hw, g, sizes, fix.shape[0], True)
    e_anti = (hr + rev).abs()[..., c:-c, c:-c, c:-c].max().item()
    print(f"ic=True: |hr - grid_sp * roll| max {e_up:.4f} voxel, |run(fix, mov) + run(mov, fix)| max {e_anti:.4f} voxel")
    assert e_up <= 0.1 and e_anti <= 0.1


@pytest.mark.parametrize("case", CASES)
def test_stage1_is_its_pieces_and_matches_the_reference(case):
    """amx_stage1_registration equals the pieces called one by one through Python (same kernels, same order: torch.equal) and
    leaves its inputs alone; against the reference's fixtures the discrete field meets the share criterion."""
    from anatomix_amd.registration import (correlate, coupled_convex, inverse_consistency, resize_trilinear,
                                           run_stage1_registration)
    fix, mov, hw, g, sizes = SR.features(case)
    n_ch = fix.shape[0]
    h, w, d = fix.shape[1:]
    df, dm = cu(fix)[None], cu(mov)[None]
    kf, km = df.clone(), dm.clone()
    soft = run_stage1_registration(df, dm, hw, g, sizes, n_ch, False)
    hr = run_stage1_registration(df, dm, hw, g, sizes, n_ch, True)
    assert torch.equal(df, kf) and torch.equal(dm, km)
    mesh = regular_mesh(hw).to(dev())
    ssd, amin = correlate(df, dm, hw, g, sizes, n_ch)
    s1 = coupled_convex(ssd, amin, mesh, g, sizes)
    assert torch.equal(s1, soft)
    ssd_, amin_ = correlate(dm, df, hw, g, sizes, n_ch)
    s2 = coupled_convex(ssd_, amin_, mesh, g, sizes)
    scale = torch.tensor([h - 1, w - 1, d - 1], dtype=torch.float32, device=dev()).view(1, 3, 1, 1, 1) / 2
    ice, _ = inverse_consistency((s1 / scale).flip(1), (s2 / scale).flip(1), iterations=15)
    pieces = resize_trilinear(ice, sizes, (scale.view(-1) * g).tolist(), flip_channels=True)
    assert torch.equal(pieces, hr)
    near = float(G[f"{case}|fwd|near_tie_share"])
    ref = G[f"{case}|stage1|soft_x27"].astype(np.float32) / np.float32(27)
    assert_discrete(soft[0].cpu().numpy(), ref, near, f"{case}|stage1 ic=False vs reference fixture")
    idx, val = G[f"{case}|stage1_ic|idx"], G[f"{case}|stage1_ic|val"]
    e = float(np.abs(hr[0].cpu().numpy().reshape(-1)[idx] - val).max())
    print(f"{case}|stage1 ic=True vs reference fixture: max abs {e:.3e} of max|ref| {np.abs(val).max():.3e}")
    assert e <= 5e-6 * np.abs(val).max()          # the discrete fields are the reference's; the rest is continuous


def test_full_size_properties():
    """Registration size (256^3 pair: 28 x 128^3 features): properties that need no CPU reference."""
    from anatomix_amd.registration import run_stage1_registration
    torch.manual_seed(0)
    fix = torch.rand(1, 28, 128, 128, 128, device=dev())
    mov = torch.roll(fix, (1, 0, -1), (2, 3, 4))
    roll = torch.tensor([1.0, 0.0, -1.0], device=dev()).view(1, 3, 1, 1, 1)
    soft = run_stage1_registration(fix, mov, 1, 2, (256, 256, 256), 28, False)
    assert soft.shape == (1, 3, 128, 128, 128) and torch.isfinite(soft).all()
    assert soft.abs().max().item() <= 1 + 1e-4
    assert (soft - roll)[..., 4:-4, 4:-4, 4:-4].abs().max().item() <= 1e-6
    hr = run_stage1_registration(fix, mov, 1, 2, (256, 256, 256), 28, True)
    assert hr.shape == (1, 3, 256, 256, 256) and torch.isfinite(hr).all()
    e = (hr - 2 * roll)[..., 8:-8, 8:-8, 8:-8].abs().max().item()
    print(f"full size: |hr - 2 * roll| max {e:.4f} voxel in the interior")
    assert e <= 0.1
    assert torch.equal(run_stage1_registration(fix, mov, 1, 2, (256, 256, 256), 28, True), hr)      # no float atomics
    assert torch.equal(run_stage1_registration(fix, mov, 1, 2, (256, 256, 256), 28, False), soft)


def test_errors_are_reported():
    import ctypes
    from anatomix_amd import _lib
    from anatomix_amd.registration import run_stage1_registration
    lib = _lib.load()
    buf = torch.zeros(1 << 20, dtype=torch.float32, device=dev())
    p, st = _lib.ptr(buf), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = buf.numel() * 4
    calls = [
        lambda: lib.amx_coupled_convex(p, None, 4, 4, 4, 4, p, p, nb, st),                          # disp_hw = 4
        lambda: lib.amx_coupled_convex(p, None, 0, 4, 4, 1, p, p, nb, st),                          # zero size
        lambda: lib.amx_coupled_convex(p, None, 4, 4, 4, 1, p, p, 16, st),                          # short scratch
        lambda: lib.amx_coupled_convex(None, None, 4, 4, 4, 1, p, p, nb, st),                       # null
        lambda: lib.amx_coupled_convex_step(p, None, 2, 4, 4, 4, 1, p, None, p, nb, st),            # history missing
        lambda: lib.amx_coupled_convex_step(p, p, 7, 4, 4, 4, 1, p, None, p, nb, st),               # iteration out of range
        lambda: lib.amx_inverse_consistency(p, p, 4, 4, -1, 15, p, p, p, nb, st),                   # negative size
        lambda: lib.amx_inverse_consistency(p, p, 4, 4, 4, 15, p, p, p, nb, st),                    # aliased
        lambda: lib.amx_resize_trilinear3d(p, 3, 4, 4, 4, None, 8, 8, 8, None, 0, st),              # null output
        lambda: lib.amx_resize_trilinear3d(p, 3, 4, 4, 4, p, 8, 8, 8, None, 0, st),                 # aliased
        lambda: lib.amx_stage1_registration(p, p, 4, 4, 4, 4, 4, 2, 1, 8, 8, 8, p, p, nb, st),      # disp_hw = 4
        lambda: lib.amx_stage1_registration(p, p, 4, 4, 4, 4, 1, 2, 1, 8, 8, 8, p, p, 1024, st),    # short scratch
        lambda: lib.amx_stage1_registration(p, p, 4, 0, 4, 4, 1, 2, 1, 8, 8, 8, p, p, nb, st),      # zero size
    ]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.AmxError):
            _lib.check(call())
    assert buf.abs().max().item() == 0.0                                   # nothing was launched
    with pytest.raises(_lib.AmxError):
        run_stage1_registration(torch.rand(1, 4, 4, 4, 4, device=dev()), torch.rand(1, 4, 4, 4, 4, device=dev()), 4, 2,
                                (8, 8, 8), 4, True)
