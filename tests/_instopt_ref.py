"""CPU restatement of the registration's second stage (create_warp / run_instance_opt of the reference's
instance_optimization.py:225-399 and the warp its driver applies, run_convex_adam_with_network_feats.py:238-266), and the
seeded inputs of its test cases.

TEST INFRASTRUCTURE ONLY: imported by the tests, tools/make_golden_instopt.py and tools/instopt_bench.py, never by the
product path.  Stock torch ops in the reference's order with torch autograd for the backward and torch.optim.Adam for the
update; the ``dtype`` argument runs the same maths in float32 (bit-identical to the reference on the CPU, which the generator
asserts) or in float64 (the yardstick the kernels' error is measured against).
"""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32

# case -> (H, W, D, grid_sp_adam, channels, amplitude of the initial displacement in voxels)
CASES = {
    "ext3": (24, 20, 28, 2, 8, 1.5),          # three different extents
    "floor3": (31, 22, 29, 3, 4, 1.5),        # floor division on every axis
    "g1": (12, 10, 14, 1, 3, 3.0),            # g = 1, grid smaller than a workgroup tile
    "c28": (16, 16, 16, 2, 28, 1.5),          # the workload's channel count
    "far": (20, 24, 16, 2, 6, 8.0),           # most samples near or beyond the border: short trajectories only
}
NITERS = {"ext3": (2, 5, 20, 80), "floor3": (2, 5, 20, 80), "g1": (2, 5, 20, 80), "c28": (2, 5, 20, 80), "far": (2, 5)}
SMOOTH_CASE = "ext3"                          # selected_smooth = 3 and 5 are taken on this case, 5 iterations
SMOOTH_NITER = 5
NITER1_CASES = ("floor3", "g1")               # the gradient-free niter = 1 run is taken on these
TF_ITERS = (0, 1, 4)                          # teacher-forced single iterations start from the state at these
ADAM_ITERS = (1, 5)
LAMBDA = 0.75
LR = 1.0
ROLL = (1, -1, 2)
WARP_SHAPE = (20, 18, 22)


def case_names():
    return list(CASES)


def grid_of(case):
    H, W, D, g, _, _ = CASES[case]
    return H // g, W // g, D // g


def _smooth(rs, shape, passes):
    a = rs.rand(*shape).astype(F32)
    for _ in range(passes):
        for ax in (-3, -2, -1):
            a = (a + np.roll(a, 1, ax) + np.roll(a, -1, ax)) / F32(3)
    return ((a - a.min()) / (a.max() - a.min())).astype(F32)


def smooth_field(shape, seed, amp, passes=4):
    """[3, *shape] smooth field, zero mean, max |.| = amp."""
    rs = np.random.RandomState(seed)
    a = _smooth(rs, (3,) + tuple(shape), passes)
    a = a - a.mean()
    return (a / np.abs(a).max() * F32(amp)).astype(F32)


def inputs(case):
    """(disp_hr [3, H, W, D] in voxels, feat_fix, feat_mov [C, H, W, D]), all fp32 numpy."""
    H, W, D, g, c, amp = CASES[case]
    rs = np.random.RandomState(4321 + 7 * list(CASES).index(case))
    fix = _smooth(rs, (c, H, W, D), 4)
    mov = (np.roll(fix, ROLL, (1, 2, 3)) + F32(0.05) * _smooth(rs, (c, H, W, D), 4)).astype(F32)
    disp = smooth_field((H, W, D), 99 + list(CASES).index(case), amp)
    return disp, fix, mov


def warp_inputs():
    """(vol [2, H, W, D], labels [1, H, W, D] with integer values, disp [3, H, W, D] of 2 voxels amplitude)."""
    rs = np.random.RandomState(2024)
    vol = _smooth(rs, (2,) + WARP_SHAPE, 1)
    lab = np.floor(_smooth(rs, (1,) + WARP_SHAPE, 2) * F32(7.999)).astype(F32)
    return vol, lab, smooth_field(WARP_SHAPE, 77, 2.0)


def tt(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---- the pieces ----------------------------------------------------------------------------------------------------------

def pooled(feat, g):
    """step 1: [C, H, W, D] numpy -> avg_pool3d(g, stride g) [C, h, w, d] numpy fp32 (computed in fp32, as the reference)."""
    return F.avg_pool3d(tt(feat)[None], g, stride=g)[0].numpy()


def initial_weight(disp_hr, g, dtype=torch.float32):
    """step 2 (create_warp): trilinear resize to the grid, divided by g.  [3, H, W, D] numpy -> [1, 3, h, w, d] tensor."""
    H, W, D = disp_hr.shape[1:]
    lr = F.interpolate(tt(disp_hr, dtype)[None], size=(H // g, W // g, D // g), mode="trilinear", align_corners=False)
    return lr / g


def smooth3(x, k=3):
    for _ in range(3):
        x = F.avg_pool3d(x, k, stride=1, padding=k // 2)
    return x


def sample_coords(ds):
    """Unnormalised sample coordinates (float64 numpy [3, h, w, d], axis order h, w, d) of a displacement [3, h, w, d] given in
    voxels of its own grid: what grid_sample makes of identity + ds / ((n - 1) / 2) with align_corners=False."""
    ds = np.asarray(ds, np.float64)
    out = np.empty_like(ds)
    for a, n in enumerate(ds.shape[1:]):
        shp = [1, 1, 1]
        shp[a] = n
        ident = ((2 * np.arange(n) + 1) / n - 1).reshape(shp)
        out[a] = ((ident + ds[a] / ((n - 1) / 2) + 1) * n - 1) / 2
    return out


def out_of_range_share(ds):
    """Share of voxels whose sample has at least one of its eight corners outside the volume."""
    co = sample_coords(ds)
    bad = np.zeros(co.shape[1:], bool)
    for a, n in enumerate(co.shape[1:]):
        bad |= (co[a] < 0) | (co[a] > n - 1)
    return float(bad.mean())


def iteration(weight, pfix, pmov, lam, dtype=torch.float32):
    """steps 3-7 from a given weight [1, 3, h, w, d]: returns (grad [1, 3, h, w, d], disp_sample [1, 3, h, w, d], loss, reg,
    grad_sample [1, 3, h, w, d]) as tensors of ``dtype``."""
    wgt = weight.detach().to(dtype).clone().requires_grad_(True)
    pf, pm = pfix.to(dtype), pmov.to(dtype)
    h, w, d = wgt.shape[2:]
    smoothed = smooth3(wgt)
    smoothed.retain_grad()
    ds = smoothed.permute(0, 2, 3, 4, 1)
    reg = lam * (((ds[0, :, 1:, :] - ds[0, :, :-1, :]) ** 2).mean() + ((ds[0, 1:, :, :] - ds[0, :-1, :, :]) ** 2).mean()
                 + ((ds[0, :, :, 1:] - ds[0, :, :, :-1]) ** 2).mean())
    # the reference builds this tensor from Python floats: float32 there, ``dtype`` here
    scale = torch.tensor([(h - 1) / 2, (w - 1) / 2, (d - 1) / 2], dtype=dtype).unsqueeze(0)
    grid0 = F.affine_grid(torch.eye(3, 4, dtype=dtype).unsqueeze(0), (1, 1, h, w, d), align_corners=False)
    grid = grid0.view(-1, 3) + (ds.reshape(-1, 3) / scale).flip(1)
    sampled = F.grid_sample(pm, grid.view(1, h, w, d, 3), align_corners=False, mode="bilinear")
    loss = ((sampled - pf).pow(2).mean(1) * 12).mean()
    (loss + reg).backward()
    return wgt.grad.detach(), smoothed.detach(), loss.detach(), reg.detach(), smoothed.grad.detach()


def run(disp_hr, feat_fix, feat_mov, g, lam, niter, smooth, lr=LR, dtype=torch.float32, record=()):
    """steps 1-10.  numpy in; returns (disp_hr_out [3, H, W, D] numpy of ``dtype``, trace).  trace[i] for i in ``record`` holds
    the state at the START of iteration i (weight, exp_avg, exp_avg_sq, t = i + 1 for the update that follows) and that
    iteration's grad / disp_sample / loss / reg, all numpy."""
    if niter <= 0:
        raise ValueError("niter >= 1")
    H, W, D = disp_hr.shape[1:]
    pf, pm = tt(pooled(feat_fix, g), dtype)[None], tt(pooled(feat_mov, g), dtype)[None]
    weight = torch.nn.Parameter(initial_weight(disp_hr, g, dtype))
    opt = torch.optim.Adam([weight], lr=lr)
    trace = {}
    ds = None
    for it in range(niter):
        opt.zero_grad()
        grad, ds, loss, reg, _ = iteration(weight, pf, pm, lam, dtype)
        if it in record:
            st = opt.state.get(weight, {})
            zero = torch.zeros_like(weight)
            trace[it] = {"weight": weight.detach().numpy().copy(), "grad": grad.numpy().copy(), "disp_sample": ds.numpy().copy(),
                         "loss": float(loss), "reg": float(reg), "t": it + 1,
                         "exp_avg": st.get("exp_avg", zero).numpy().copy(), "exp_avg_sq": st.get("exp_avg_sq", zero).numpy().copy()}
        weight.grad = grad
        opt.step()
    out = F.interpolate(ds * g, size=(H, W, D), mode="trilinear", align_corners=False)
    if smooth in (3, 5):
        out = smooth3(out, smooth)
    return out[0].numpy(), trace


def warp(vol, disp, mode="bilinear", dtype=torch.float32):
    """The driver's grid_sample: vol [c, H, W, D], disp [3, H, W, D] in voxels -> [c, H, W, D] numpy."""
    H, W, D = vol.shape[1:]
    grid1 = F.affine_grid(torch.eye(3, 4, dtype=dtype).unsqueeze(0), (1, 1, H, W, D), align_corners=False)
    disp0 = tt(disp, dtype)[None].permute(0, 2, 3, 4, 1)
    denom = torch.tensor([H - 1, W - 1, D - 1]).view(1, 1, 1, 1, 3)
    disp0 = (disp0 / denom * 2).flip(4)
    return F.grid_sample(tt(vol, dtype)[None], (grid1 + disp0).to(dtype), align_corners=False, mode=mode)[0].numpy()


def near_half_mask(disp, tol=1e-4):
    """Voxels whose sample coordinate lies within ``tol`` of a half-integer on any axis: where nearest mode's rounding is
    decided by the last bits of the coordinate."""
    co = sample_coords(disp)
    frac = np.abs(co - np.floor(co) - 0.5)
    return (frac < tol).any(0)
