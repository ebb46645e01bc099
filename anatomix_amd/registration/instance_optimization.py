"""``merge_features`` with the surface of ``anatomix.registration.instance_optimization`` (reference :16-119): MIND-SSC
descriptors of the two images concatenated in front of the (already down-scaled) network features.  The descriptor runs
on the HIP kernel; the masked branch's distance-transform fill is host logic exactly as in the reference (scipy on the
CPU) and only its MIND-SSC call is accelerated.  ``run_stage1_registration`` (:122-222), the discrete stage from the
smoothed features to the displacement field, is one call into the C ABI (csrc/amx_regsolve.hip).  The Adam instance
optimisation of that reference module (create_warp, run_instance_opt) is not part of this package.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _lib
from .convex_adam_utils import MINDSSC, _f32c, _stream


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
        sc = torch.empty(max(nb, 1), dtype=torch.uint8, device=f.device)
        _lib.check(lib.amx_stage1_registration(_lib.ptr(f), _lib.ptr(m), int(n_ch), h, w, d, int(disp_hw), g, int(ic), H, W, D,
                                               _lib.ptr(out), _lib.ptr(sc), nb, _stream(f.device)))
    return out
