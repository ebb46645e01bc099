"""GPU: the Adam instance optimisation and the warp through the C ABI (csrc/amx_reginstopt.hip) against the torch restatement
(tests/_instopt_ref.py, run on the CPU: float64 for single kernels, torch.optim.Adam for the update) and the fixtures captured
from the reference's own functions in fp32 (tools/make_golden_instopt.py -> tests/golden/instopt_golden.npz).

Bounds.  Continuous kernels: max abs error <= 5e-6 x max|reference| (fp32 with another summation order).  The gradient of
one teacher-forced iteration: (5e-6 + 10 x e32) x max|grad|, e32 being the fp32 reference's own distance from float64 for
that tensor (fixture); the trajectories: (5e-6 + 10 x ref_vs_f64) x max|reference| with ref_vs_f64 from the fixture.  No
bound comes from the code under test.  Every test prints the figure it measured before it asserts."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _instopt_ref as IR

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "instopt_golden.npz"))
CASES = IR.case_names()
RUNS = [(c, n, 0) for c in CASES for n in IR.NITERS[c]] + [(IR.SMOOTH_CASE, IR.SMOOTH_NITER, 3), (IR.SMOOTH_CASE, IR.SMOOTH_NITER, 5)] \
    + [(c, 1, 0) for c in IR.NITER1_CASES]


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def relmax(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


@functools.lru_cache(maxsize=None)
def state(case):
    """The fp32 restatement's trajectory on the CPU, computed once per case and left unchanged: pooled features and the state
    at the start of iterations 0 .. 6."""
    disp, fix, mov = IR.inputs(case)
    g = IR.CASES[case][3]
    _, trace = IR.run(disp, fix, mov, g, IR.LAMBDA, 7, 0, record=tuple(range(7)))
    return IR.pooled(fix, g), IR.pooled(mov, g), trace


@pytest.mark.parametrize("shape", [(12, 10, 14), (5, 3, 2), (33, 17, 9)])
def test_fused_smoothing_is_three_box_passes_and_self_adjoint(shape):
    from anatomix_amd.registration import apply_avg_pool3d, instance_opt_smooth3
    rs = np.random.RandomState(5)
    x, y = cu(rs.randn(1, 3, *shape).astype(np.float32)), cu(rs.randn(1, 3, *shape).astype(np.float32))
    keep = x.clone()
    got, want = instance_opt_smooth3(x), apply_avg_pool3d(x, 3, 3)
    assert torch.equal(x, keep)
    e = (got - want).abs().max().item() / want.abs().max().item()
    print(f"smooth3 {shape}: rel max {e:.3e} against three amx_box_filter3d launches, bit-equal: {torch.equal(got, want)}")
    assert e <= 5e-6
    cpu = x.double().cpu()
    for _ in range(3):          # zero padding written out: torch's CPU avg_pool3d refuses an extent below the kernel size
        cpu = F.avg_pool3d(F.pad(cpu, (1,) * 6), 3, stride=1)
    assert relmax(got.cpu().numpy(), cpu.numpy()) <= 5e-6
    lhs, rhs = (got.double() * y.double()).sum().item(), (x.double() * instance_opt_smooth3(y).double()).sum().item()
    print(f"smooth3 {shape}: <Sx, y> {lhs:.9e}  <x, Sy> {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs))


@pytest.mark.parametrize("case", CASES)
def test_one_iteration_teacher_forced(case):
    """instance_opt_grad from the restatement's state at iterations 0, 1 and 4 against the float64 restatement started from the
    same fp32 state.  Every voxel counts."""
    from anatomix_amd.registration import instance_opt_grad
    pf, pm, trace = state(case)
    dpf, dpm = cu(pf)[None], cu(pm)[None]
    kf, km = dpf.clone(), dpm.clone()
    for it in IR.TF_ITERS:
        wgt = IR.tt(trace[it]["weight"])
        g64, ds64, loss64, reg64, _ = IR.iteration(wgt, IR.tt(pf)[None], IR.tt(pm)[None], IR.LAMBDA, torch.float64)
        dw = wgt.to(dev())
        kw = dw.clone()
        grad, ds, loss, reg = instance_opt_grad(dw, dpf, dpm, IR.LAMBDA)
        grad2, _, loss2, reg2 = instance_opt_grad(dw, dpf, dpm, IR.LAMBDA)
        assert torch.equal(dw, kw) and torch.equal(dpf, kf) and torch.equal(dpm, km)
        assert grad.shape == dw.shape and ds.shape == dw.shape
        e32 = float(G[f"{case}|it{it}|e32"])
        e_ds, e_g = relmax(ds.cpu().numpy(), ds64.numpy()), relmax(grad.cpu().numpy(), g64.numpy())
        e_l, e_r = abs(loss.item() - loss64.item()) / abs(loss64.item()), abs(reg.item() - reg64.item()) / abs(reg64.item())
        print(f"{case} iteration {it}: disp_sample {e_ds:.3e}  grad {e_g:.3e} (e32 {e32:.3e}, bound {5e-6 + 10 * e32:.3e})  "
              f"loss {e_l:.3e}  reg {e_r:.3e}")
        assert e_ds <= 5e-6
        assert e_l <= 1e-5 and e_r <= 1e-5
        assert e_g <= 5e-6 + 10 * e32
        assert loss.item() == loss2.item() and reg.item() == reg2.item() and torch.equal(grad, grad2)


@pytest.mark.parametrize("case", CASES)
def test_update_teacher_forced(case):
    """One update from the restatement's weight, gradient and moments at iterations 1 and 5 against torch.optim.Adam on the CPU
    (the restatement's next weight)."""
    from anatomix_amd.registration import instance_opt_adam_step
    _, _, trace = state(case)
    for it in IR.ADAM_ITERS:
        st = trace[it]
        wgt, m, v = cu(st["weight"]), cu(st["exp_avg"]), cu(st["exp_avg_sq"])
        instance_opt_adam_step(wgt, cu(st["grad"]), m, v, st["t"], IR.LR)
        want = trace[it + 1]
        e = [relmax(a.cpu().numpy(), want[k]) for a, k in ((wgt, "weight"), (m, "exp_avg"), (v, "exp_avg_sq"))]
        print(f"{case} update {st['t']}: weight {e[0]:.3e}  exp_avg {e[1]:.3e}  exp_avg_sq {e[2]:.3e}")
        assert max(e) <= 1e-6


@pytest.mark.parametrize("case,niter,smooth", RUNS)
def test_trajectory_against_the_reference(case, niter, smooth):
    from anatomix_amd.registration import run_instance_opt
    H, W, D, g, c, _ = IR.CASES[case]
    disp, fix, mov = (cu(a)[None] for a in IR.inputs(case))
    keep = [t.clone() for t in (disp, fix, mov)]
    out = run_instance_opt(disp, fix, mov, g, IR.LAMBDA, (H, W, D), niter, smooth, lr=IR.LR)
    assert out.shape == (1, 3, H, W, D) and out.dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip((disp, fix, mov), keep))
    key = f"{case}|n{niter}|s{smooth}"
    got = out[0].cpu().numpy()
    if key + "|full" in G.files:
        want = G[key + "|full"]
    else:
        got, want = got.reshape(-1)[G[f"{case}|idx"].astype(np.int64)], G[key + "|val"]
    bound = 5e-6 + (10 * float(G[key + "|ref_vs_f64"]) if niter > 1 else 0.0)
    e = relmax(got, want)
    print(f"{key}: rel max {e:.3e} of max|ref| {np.abs(want).max():.3f}, bound {bound:.3e}")
    assert e <= bound


@pytest.mark.parametrize("case,niter,smooth", [("floor3", 5, 0), (IR.SMOOTH_CASE, 3, 5)])
def test_run_is_its_pieces(case, niter, smooth):
    """amx_run_instance_opt equals pooling, resize, amx_instance_opt, resize (and the box passes) called one by one: same
    kernels, same order."""
    from anatomix_amd.registration import (apply_avg_pool3d, create_warp, instance_opt, resize_trilinear, run_instance_opt,
                                           smooth_merged_features)
    H, W, D, g, c, _ = IR.CASES[case]
    disp, fix, mov = (cu(a)[None] for a in IR.inputs(case))
    whole = run_instance_opt(disp, fix, mov, g, IR.LAMBDA, (H, W, D), niter, smooth)
    pf, pm = smooth_merged_features(None, fix, g, 1.0), smooth_merged_features(None, mov, g, 1.0)
    net = create_warp(disp, (H, W, D), g)
    assert isinstance(net, torch.nn.Sequential) and net[0].weight.shape == (1, 3, H // g, W // g, D // g) and net[0].weight.is_cuda
    assert net[0].bias is None
    assert relmax(net[0].weight.detach().cpu().numpy(), IR.initial_weight(IR.inputs(case)[0], g).numpy()) <= 5e-6
    w0 = net[0].weight.detach().clone()
    fitted, w_end = instance_opt(w0, pf, pm, IR.LAMBDA, niter)
    assert torch.equal(w0, net[0].weight.detach()) and not torch.equal(w_end, w0)
    pieces = resize_trilinear(fitted, (H, W, D), [float(g)] * 3)
    if smooth:
        pieces = apply_avg_pool3d(pieces, smooth, 3)
    assert torch.equal(pieces, whole)
    assert torch.equal(run_instance_opt(disp, fix, mov, g, IR.LAMBDA, (H, W, D), niter, smooth), whole)      # no float atomics
    # any selected_smooth outside {3, 5} means none, as the reference's `in [3, 5]`
    if not smooth:
        assert torch.equal(run_instance_opt(disp, fix, mov, g, IR.LAMBDA, (H, W, D), niter, 4), whole)


def test_warp_against_grid_sample():
    from anatomix_amd.registration import warp_volume
    vol, lab, wd = IR.warp_inputs()
    dv, dl, dd = cu(vol)[None], cu(lab)[None], cu(wd)[None]
    keep = dd.clone()
    got = warp_volume(dv, dd)[0].cpu().numpy()
    want = G["warp|bilinear|full"]
    e = relmax(got, want)
    print(f"warp bilinear {IR.WARP_SHAPE}: rel max {e:.3e}")
    assert got.shape == want.shape and e <= 5e-6
    near = warp_volume(dl, dd, mode="nearest")[0].cpu().numpy()
    assert torch.equal(dd, keep)
    skip = IR.near_half_mask(wd)
    print(f"warp nearest: {skip.mean():.4%} of the voxels within 1e-4 of a half-integer coordinate left out")
    assert skip.mean() <= 0.005
    wrong = (near[0] != G["warp|nearest|full"][0].astype(np.float32)) & ~skip
    assert int(wrong.sum()) == 0
    # a displacement far outside, infinite or NaN samples nothing: zeros, and no access out of range
    bad = dd.clone()
    bad[0, 0, :4] = 1e30
    bad[0, 1, 4:8] = float("nan")
    bad[0, 2, 8:12] = float("-inf")
    for mode in ("bilinear", "nearest"):
        out = warp_volume(dv, bad, mode=mode)
        assert out[0, :, :12].abs().max().item() == 0.0 and torch.isfinite(out).all()


def test_non_finite_weights_do_not_leave_the_volume():
    """Non-finite and huge displacements: every corner is out of range, the data term contributes nothing there."""
    from anatomix_amd.registration import instance_opt_grad
    pf, pm, trace = state("g1")
    wgt = cu(trace[0]["weight"]).clone()
    wgt[0, 0, 3, 3, 3] = 1e30
    wgt[0, 1, 8, 5, 9] = -1e30
    grad, ds, loss, reg = instance_opt_grad(wgt, cu(pf)[None], cu(pm)[None], IR.LAMBDA)
    assert torch.isfinite(loss) and torch.isfinite(grad[0, :, 0, 0, 13]).all()
    wgt[0, 2, 6, 6, 6] = float("nan")
    grad, ds, loss, reg = instance_opt_grad(wgt, cu(pf)[None], cu(pm)[None], IR.LAMBDA)
    assert torch.isfinite(loss) and torch.isnan(ds[0, 2, 6, 6, 6])


def test_errors_are_reported():
    from anatomix_amd import _lib
    from anatomix_amd.registration import run_instance_opt
    lib = _lib.load()
    buf = torch.zeros(1 << 20, dtype=torch.float32, device=dev())
    p, st = _lib.ptr(buf), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = ctypes.c_void_p(buf.data_ptr() + 4096)
    nb = buf.numel() * 4
    calls = [
        lambda: lib.amx_instance_opt_smooth3(p, p, 4, 4, 4, st),                                         # aliased
        lambda: lib.amx_instance_opt_smooth3(p, None, 4, 4, 4, st),                                      # null
        lambda: lib.amx_instance_opt_grad(p, p, p, 2, 4, 4, 1, 0.75, q, None, None, p, nb, st),          # extent below 2
        lambda: lib.amx_instance_opt_grad(p, p, p, 0, 4, 4, 4, 0.75, q, None, None, p, nb, st),          # no channels
        lambda: lib.amx_instance_opt_grad(p, p, p, 2, 4, 4, 4, 0.75, q, None, None, p, 16, st),          # short scratch
        lambda: lib.amx_instance_opt_grad(p, None, p, 2, 4, 4, 4, 0.75, q, None, None, p, nb, st),       # null
        lambda: lib.amx_instance_opt_grad(p, p, p, 2, 4, 4, 4, 0.75, p, None, None, p, nb, st),          # grad aliases weight
        lambda: lib.amx_instance_opt_adam_step(p, p, p, p, 64, 1.0, 0, st),                              # step 0
        lambda: lib.amx_instance_opt_adam_step(p, p, p, None, 64, 1.0, 1, st),                           # null
        lambda: lib.amx_instance_opt(p, p, p, 2, 4, 4, 4, 0.75, 1.0, 0, q, p, nb, st),                   # niter 0
        lambda: lib.amx_instance_opt(p, p, p, 2, 4, 4, 4, 0.75, 1.0, -1, q, p, nb, st),                  # niter < 0
        lambda: lib.amx_instance_opt(p, p, p, 2, 1, 4, 4, 0.75, 1.0, 5, q, p, nb, st),                   # extent below 2
        lambda: lib.amx_instance_opt(p, p, p, 2, 4, 4, 4, 0.75, 1.0, 5, q, p, 1024, st),                 # short scratch
        lambda: lib.amx_instance_opt(p, p, p, 2, 4, 4, 4, 0.75, 1.0, 5, None, p, nb, st),                # null
        lambda: lib.amx_instance_opt(p, p, p, 2, 4, 4, 4, 0.75, 0.0, 5, q, p, nb, st),                   # lr 0
        lambda: lib.amx_run_instance_opt(p, p, p, 2, 8, 8, 8, 2, 0.75, 0, 0, 1.0, q, p, nb, st),         # niter 0
        lambda: lib.amx_run_instance_opt(p, p, p, 2, 8, 8, 8, 8, 0.75, 5, 0, 1.0, q, p, nb, st),         # a 1^3 grid
        lambda: lib.amx_run_instance_opt(p, p, p, 2, 8, 8, 8, 0, 0.75, 5, 0, 1.0, q, p, nb, st),         # grid_sp_adam 0
        lambda: lib.amx_run_instance_opt(p, p, p, 2, 8, 8, 8, 2, 0.75, 5, 0, 1.0, q, p, 1024, st),       # short scratch
        lambda: lib.amx_run_instance_opt(p, p, p, 2, 8, 8, 8, 2, 0.75, 5, 0, 1.0, None, p, nb, st),      # null
        lambda: lib.amx_warp3d(p, 1, p, 8, 8, 8, 2, q, st),                                              # unknown mode
        lambda: lib.amx_warp3d(p, 1, p, 8, 1, 8, 0, q, st),                                              # extent below 2
        lambda: lib.amx_warp3d(p, 0, p, 8, 8, 8, 0, q, st),                                              # no channels
        lambda: lib.amx_warp3d(p, 1, p, 8, 8, 8, 0, p, st),                                              # aliased
    ]
    for call in calls:
        with pytest.raises(_lib.AmxError):
            _lib.check(call())
        assert lib.amx_last_error().decode() != ""
    assert buf.abs().max().item() == 0.0                                   # nothing was launched
    # a selected_smooth outside {3, 5} asks for scratch without the two full-resolution fields, like 0
    assert lib.amx_run_instance_opt_scratch_bytes(2, 8, 8, 8, 2, 4) == lib.amx_run_instance_opt_scratch_bytes(2, 8, 8, 8, 2, 0)
    assert lib.amx_run_instance_opt_scratch_bytes(2, 8, 8, 8, 2, 3) > lib.amx_run_instance_opt_scratch_bytes(2, 8, 8, 8, 2, 0)
    with pytest.raises(ValueError):
        run_instance_opt(torch.zeros(1, 3, 8, 8, 8, device=dev()), torch.zeros(1, 2, 8, 8, 8, device=dev()),
                         torch.zeros(1, 2, 8, 8, 8, device=dev()), 2, 0.75, (8, 8, 8), 0, 0)
