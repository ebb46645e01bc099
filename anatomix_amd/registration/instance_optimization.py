"""``merge_features`` with the surface of ``anatomix.registration.instance_optimization`` (reference :16-119): MIND-SSC
descriptors of the two images concatenated in front of the (already down-scaled) network features.  The descriptor runs
on the HIP kernel; the masked branch's distance-transform fill is host logic exactly as in the reference (scipy on the
CPU) and only its MIND-SSC call is accelerated.  ``run_stage1_registration`` (:122-222), the discrete stage from the
smoothed features to the displacement field, is one call into the C ABI (csrc/amx_regsolve.hip), and so is
``run_instance_opt`` (:269-399), the Adam instance optimisation on top of it (csrc/amx_reginstopt.hip): forward, backward and
update are hand-written kernels, four launches per iteration, with no autograd graph.  ``create_warp`` (:225-266) is kept for
surface parity and ``warp_volume`` is the ``grid_sample`` the reference's driver applies with the fitted field.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from .convex_adam_utils import MINDSSC, _f32c, resize_trilinear


def _fill_outside_mask(img, mask_vol):
    """instance_optimization.py:59-81: voxels outside the (eroded) mask take the value of the nearest inside voxel, found
    on the 2x subsampled grid with a Euclidean distance transform and brought back with trilinear interpolation."""
    from scipy.ndimage import distance_transform_edt as edt

    h, w, d = img.shape[-3:]
    avg = F.avg_pool3d(F.pad(mask_vol.view(1, 1, h, w, d), (1,) * 6, mode="replicate"), 3, stride=1)
    mask = (avg > 0.9).float()
    _, idx = edt((mask[0, 0, ::2, ::2, ::2] == 0).squeeze().cpu().numpy(), return_indices=True)
    idx = [torch.from_numpy(i).to(img.device).long() for i in idx]
    sub = img[..., ::2, ::2, ::2].reshape(-1)
    # flat index into the subsampled volume with the reference's own integer arithmetic (left to right: ((i0*D)//2*W)//2, :71);
    # equal to i0*(D/2)*(W/2) + i1*(D/2) + i2 on even extents.  An odd extent does not survive the subsample / x2 round trip: the
    # masked assignment below then raises IndexError, as the reference does (fixture flag `odd_dim_raises`).
    flat = idx[0] * d // 2 * w // 2 + idx[1] * d // 2 + idx[2]
    filled = F.interpolate(sub[flat].unsqueeze(0).unsqueeze(0), scale_factor=2, mode="trilinear")
    keep = mask.view(-1) != 0
    filled.view(-1)[keep] = img.reshape(-1)[keep]
    return filled


def merge_features(use_mask, pred_fixed, pred_moving, mask_fixed, mask_moving, fixed_img, moving_img):
    """Returns (mind_fixed, mind_moving, merged_fixed, merged_moving); merged = cat([mind, pred], 1)
    (instance_optimization.py:16-119; MINDSSC(img, 1, 2) as there).  When only the grid_sp-pooled merged features are
    needed, ``convex_adam_utils.smooth_merged_features`` produces them without this full-resolution concat."""
    if use_mask:
        fixed_img = _fill_outside_mask(fixed_img, mask_fixed)
        moving_img = _fill_outside_mask(moving_img, mask_moving)
        pred_fixed = pred_fixed * mask_fixed[None, None, ...]
        pred_moving = pred_moving * mask_moving[None, None, ...]
    mind_fixed = MINDSSC(fixed_img, 1, 2)
    mind_moving = MINDSSC(moving_img, 1, 2)
    return (mind_fixed, mind_moving, torch.cat([mind_fixed, pred_fixed], dim=1), torch.cat([mind_moving, pred_moving], dim=1))


def run_stage1_registration(features_fix_smooth, features_mov_smooth, disp_hw, grid_sp, sizes, n_ch, ic):
    """instance_optimization.py:122-222 as one ``amx_stage1_registration`` call: both ``correlate`` directions, both
    ``coupled_convex`` solves, 15 ``inverse_consistency`` sweeps and the trilinear upsampling, enqueued on the current
    stream without host synchronisation.  features_* [1, n_ch, H // grid_sp, W // grid_sp, D // grid_sp]; sizes = (H, W, D).
    As in the reference, ``ic=False`` returns the coarse ``disp_soft`` [1, 3, h, w, d] in grid units (not upsampled) and
    ``ic=True`` returns [1, 3, H, W, D] in voxels.  fp32 throughout (the reference's own caller runs the solver in half)."""
    f = _f32c(features_fix_smooth, "run_stage1_registration")
    m = _f32c(features_mov_smooth, "run_stage1_registration")
    H, W, D = (int(v) for v in sizes)
    g = int(grid_sp)
    h, w, d = H // g, W // g, D // g
    if tuple(f.shape) != (1, n_ch, h, w, d) or tuple(m.shape) != tuple(f.shape):
        raise ValueError(f"run_stage1_registration: features {tuple(f.shape)} / {tuple(m.shape)} do not match (1, {n_ch}, {h}, {w}, {d})")
    lib = _lib.load()
    ic = bool(ic)
    out = torch.empty((1, 3, H, W, D) if ic else (1, 3, h, w, d), dtype=torch.float32, device=f.device)
    with torch.cuda.device(f.device):
        nb = lib.amx_stage1_registration_scratch_bytes(h, w, d, int(disp_hw), int(ic))
        sc = _lib.scratch(nb, f.device)
        _lib.check(lib.amx_stage1_registration(_lib.ptr(f), _lib.ptr(m), int(n_ch), h, w, d, int(disp_hw), g, int(ic), H, W, D,
                                               _lib.ptr(out), _lib.ptr(sc), nb, _lib.stream(f.device)))
    return out


def _opt_grid(sizes, grid_sp_adam, what):
    H, W, D = (int(v) for v in sizes)
    g = int(grid_sp_adam)
    if g < 1:
        raise ValueError(f"{what}: grid_sp_adam >= 1 (got {g})")
    h, w, d = H // g, W // g, D // g
    if min(h, w, d) < 2:
        raise ValueError(f"{what}: the optimisation grid ({h}, {w}, {d}) needs at least 2 per axis")
    return H, W, D, g, h, w, d


def create_warp(disp_hr, sizes, grid_sp_adam):
    """instance_optimization.py:225-266: ``nn.Sequential(nn.Conv3d(3, 1, (h, w, d), bias=False))`` whose weight is disp_hr
    [1, 3, H, W, D] resized to the grid and divided by grid_sp_adam, on disp_hr's device.  Surface parity only:
    ``run_instance_opt`` keeps the grid in a plain buffer and does not go through a module."""
    H, W, D, g, h, w, d = _opt_grid(sizes, grid_sp_adam, "create_warp")
    if tuple(disp_hr.shape) != (1, 3, H, W, D):
        raise ValueError(f"create_warp: disp_hr {tuple(disp_hr.shape)} does not match (1, 3, {H}, {W}, {D})")
    net = nn.Sequential(nn.Conv3d(3, 1, (h, w, d), bias=False)).to(disp_hr.device)
    net[0].weight.data[:] = resize_trilinear(disp_hr, (h, w, d), [1.0 / g] * 3)
    return net


def run_instance_opt(disp_hr, features_fix, features_mov, grid_sp_adam, lambda_weight, sizes, selected_niter, selected_smooth,
                     lr=1):
    """instance_optimization.py:269-399 as one ``amx_run_instance_opt`` call: the grid_sp_adam pooling of both feature
    volumes, the initial grid, ``selected_niter`` Adam iterations (four launches each) and the upsampling / final smoothing,
    enqueued on the current stream without host synchronisation.  disp_hr [1, 3, H, W, D] in voxels, features_* [1, C, H, W, D];
    returns [1, 3, H, W, D].  The field comes from the last iteration's forward, as in the reference, whose
    ``selected_niter <= 0`` fails with a NameError: a ValueError here.  The inputs are not modified."""
    if int(selected_niter) <= 0:
        raise ValueError(f"run_instance_opt: selected_niter >= 1 (got {selected_niter})")
    H, W, D, g, h, w, d = _opt_grid(sizes, grid_sp_adam, "run_instance_opt")
    if disp_hr.dim() != 5 or tuple(disp_hr.shape) != (1, 3, H, W, D):
        raise ValueError(f"run_instance_opt: disp_hr {tuple(disp_hr.shape)} does not match (1, 3, {H}, {W}, {D})")
    if features_fix.dim() != 5 or tuple(features_fix.shape[2:]) != (H, W, D) or features_fix.shape[0] != 1 \
            or features_fix.shape[1] < 1 or tuple(features_mov.shape) != tuple(features_fix.shape):
        raise ValueError(f"run_instance_opt: features {tuple(features_fix.shape)} / {tuple(features_mov.shape)} do not match "
                         f"(1, C, {H}, {W}, {D})")
    x = _f32c(disp_hr, "run_instance_opt")
    f = _f32c(features_fix, "run_instance_opt")
    m = _f32c(features_mov, "run_instance_opt")
    c = f.shape[1]
    smooth = int(selected_smooth) if selected_smooth in (3, 5) else 0
    lib = _lib.load()
    out = torch.empty((1, 3, H, W, D), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nb = lib.amx_run_instance_opt_scratch_bytes(c, H, W, D, g, smooth)
        sc = _lib.scratch(nb, x.device)
        _lib.check(lib.amx_run_instance_opt(_lib.ptr(x), _lib.ptr(f), _lib.ptr(m), c, H, W, D, g, float(lambda_weight),
                                            int(selected_niter), smooth, float(lr), _lib.ptr(out), _lib.ptr(sc), nb,
                                            _lib.stream(x.device)))
    return out


def _grid_state(weight, patch_fix, patch_mov, what):
    if weight.dim() != 5 or weight.shape[0] != 1 or weight.shape[1] != 3:
        raise ValueError(f"{what}: weight [1, 3, h, w, d] (got {tuple(weight.shape)})")
    h, w, d = (int(v) for v in weight.shape[2:])
    if min(h, w, d) < 2:
        raise ValueError(f"{what}: the optimisation grid ({h}, {w}, {d}) needs at least 2 per axis")
    if patch_fix.dim() != 5 or patch_fix.shape[0] != 1 or patch_fix.shape[1] < 1 or tuple(patch_fix.shape[2:]) != (h, w, d) \
            or tuple(patch_mov.shape) != tuple(patch_fix.shape):
        raise ValueError(f"{what}: features {tuple(patch_fix.shape)} / {tuple(patch_mov.shape)} do not match (1, C, {h}, {w}, {d})")
    return h, w, d


def instance_opt_grad(weight, patch_fix, patch_mov, lambda_weight):
    """One iteration's forward and backward from a given grid (``amx_instance_opt_grad``): weight [1, 3, h, w, d], pooled
    features [1, C, h, w, d] -> (grad [1, 3, h, w, d], disp_sample [1, 3, h, w, d], loss, reg); loss and reg are 0-dim device
    tensors.  What run_instance_opt iterates, exposed so that each kernel can be held against autograd on its own."""
    h, w, d = _grid_state(weight, patch_fix, patch_mov, "instance_opt_grad")
    x = _f32c(weight, "instance_opt_grad")
    f = _f32c(patch_fix, "instance_opt_grad")
    m = _f32c(patch_mov, "instance_opt_grad")
    c = f.shape[1]
    lib = _lib.load()
    grad, ds = torch.empty_like(x), torch.empty_like(x)
    loss2 = torch.empty(2, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nb = lib.amx_instance_opt_scratch_bytes(c, h, w, d)
        sc = _lib.scratch(nb, x.device)
        _lib.check(lib.amx_instance_opt_grad(_lib.ptr(x), _lib.ptr(f), _lib.ptr(m), c, h, w, d, float(lambda_weight),
                                             _lib.ptr(grad), _lib.ptr(ds), _lib.ptr(loss2), _lib.ptr(sc), nb, _lib.stream(x.device)))
    return grad, ds, loss2[0], loss2[1]


def instance_opt(weight, patch_fix, patch_mov, lambda_weight, niter, lr=1):
    """The loop alone (``amx_instance_opt``): ``niter`` iterations from weight [1, 3, h, w, d] -> (disp_sample of the last
    iteration's forward, the weight after niter - 1 updates).  ``weight`` itself is not modified."""
    if int(niter) <= 0:
        raise ValueError(f"instance_opt: niter >= 1 (got {niter})")
    h, w, d = _grid_state(weight, patch_fix, patch_mov, "instance_opt")
    x = _f32c(weight, "instance_opt").clone()
    f = _f32c(patch_fix, "instance_opt")
    m = _f32c(patch_mov, "instance_opt")
    c = f.shape[1]
    lib = _lib.load()
    fitted = torch.empty_like(x)
    with torch.cuda.device(x.device):
        nb = lib.amx_instance_opt_scratch_bytes(c, h, w, d)
        sc = _lib.scratch(nb, x.device)
        _lib.check(lib.amx_instance_opt(_lib.ptr(x), _lib.ptr(f), _lib.ptr(m), c, h, w, d, float(lambda_weight), float(lr),
                                        int(niter), _lib.ptr(fitted), _lib.ptr(sc), nb, _lib.stream(x.device)))
    return fitted, x


def instance_opt_smooth3(field):
    """``apply_avg_pool3d(field, 3, 3)`` of a [1, 3, h, w, d] field in one launch (``amx_instance_opt_smooth3``); it is its own
    adjoint."""
    if field.dim() != 5 or field.shape[0] != 1 or field.shape[1] != 3:
        raise ValueError(f"instance_opt_smooth3: field [1, 3, h, w, d] (got {tuple(field.shape)})")
    x = _f32c(field, "instance_opt_smooth3")
    h, w, d = (int(v) for v in x.shape[2:])
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().amx_instance_opt_smooth3(_lib.ptr(x), _lib.ptr(out), h, w, d, _lib.stream(x.device)))
    return out


def instance_opt_adam_step(weight, grad, exp_avg, exp_avg_sq, t, lr=1):
    """Step ``t`` (1-based) of torch.optim.Adam(lr) on contiguous fp32 device tensors, IN PLACE (``amx_instance_opt_adam_step``)."""
    for nm, v in (("weight", weight), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if not (v.is_cuda and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == weight.numel()):
            raise ValueError(f"instance_opt_adam_step: {nm} must be a contiguous fp32 device tensor of the weight's size")
    with torch.cuda.device(weight.device):
        _lib.check(_lib.load().amx_instance_opt_adam_step(_lib.ptr(weight), _lib.ptr(grad), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                                          weight.numel(), float(lr), int(t), _lib.stream(weight.device)))
    return weight


def warp_volume(vol, disp_hr, mode="bilinear"):
    """The two ``F.grid_sample`` calls of the reference's driver (run_convex_adam_with_network_feats.py:238-266): vol
    [1, C, H, W, D] sampled at identity + disp_hr [1, 3, H, W, D] (voxels), zeros outside, align_corners=False.  mode
    "bilinear" (the image) or "nearest" (the label map; half-way cases round to even)."""
    if mode not in _lib.WARP:
        raise ValueError(f"warp_volume: mode 'bilinear' or 'nearest' (got {mode!r})")
    if vol.dim() != 5 or vol.shape[0] != 1 or vol.shape[1] < 1 or disp_hr.dim() != 5 \
            or tuple(disp_hr.shape) != (1, 3) + tuple(vol.shape[2:]):
        raise ValueError(f"warp_volume: vol {tuple(vol.shape)} / disp_hr {tuple(disp_hr.shape)} do not match [1, C, H, W, D] / [1, 3, H, W, D]")
    if min(vol.shape[2:]) < 2:
        raise ValueError(f"warp_volume: at least 2 voxels per axis (got {tuple(vol.shape[2:])})")
    v = _f32c(vol, "warp_volume")
    x = _f32c(disp_hr, "warp_volume")
    c, (H, W, D) = v.shape[1], (int(n) for n in v.shape[2:])
    out = torch.empty_like(v)
    with torch.cuda.device(v.device):
        _lib.check(_lib.load().amx_warp3d(_lib.ptr(v), c, _lib.ptr(x), H, W, D, _lib.WARP[mode], _lib.ptr(out), _lib.stream(v.device)))
    return out
