"""The registration driver with the surface of ``anatomix/registration/run_convex_adam_with_network_feats.py``: ``convex_adam``
(reference :26-327) takes two NIfTI volumes and writes the displacement field, the moved image, the moved label map and a Dice
score, and ``python -m anatomix_amd.registration.run_convex_adam_with_network_feats`` has the reference's command line
(:330-499).  ``register_volumes`` is its in-memory body, composed from this package's public functions in the reference's order
(:152-266).  Files go through ``anatomix_amd.io.nifti`` (no nibabel); the Dice score comes from device-side label counts
(``metrics.dice_score``, no sklearn); the Jacobian statistics of the fitted map are reported next to it."""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch
import torch.nn.functional as F

from ..io.nifti import load_nifti, save_nifti
from .convex_adam_utils import (JACOBIAN_STATS, apply_avg_pool3d, extract_features, jacobian_statistics, load_model,
                                resize_trilinear)
from .instance_optimization import instance_opt, merge_features, run_instance_opt, run_stage1_registration, warp_volume
from .metrics import dice_score


def _instance_opt_from_coarse(disp_lr, features_fix, features_mov, grid_sp_adam, lambda_weight, sizes, selected_niter, selected_smooth):
    """What the reference's ``run_instance_opt`` does with the coarse field that stage 1 returns under ``ic=False``
    (instance_optimization.py:225-266, :309-399): ``create_warp`` resizes whatever grid it is given to the optimisation grid and
    divides by grid_sp_adam.  ``run_instance_opt`` of this package takes full-resolution fields only, so the same steps are
    composed here."""
    H, W, D = sizes
    g = int(grid_sp_adam)
    grid = (H // g, W // g, D // g)
    weight = resize_trilinear(disp_lr, grid, [1.0 / g] * 3)
    with torch.no_grad():
        patch_fix = F.avg_pool3d(features_fix, g, stride=g)
        patch_mov = F.avg_pool3d(features_mov, g, stride=g)
    fitted, _ = instance_opt(weight, patch_fix, patch_mov, lambda_weight, selected_niter, lr=1)
    disp_hr = resize_trilinear(fitted, (H, W, D), [float(g)] * 3)
    if selected_smooth in [3, 5]:
        disp_hr = apply_avg_pool3d(disp_hr, selected_smooth, num_repeats=3)
    return disp_hr


def _device_volume(arr, dev, what, shape):
    t = arr if torch.is_tensor(arr) else torch.from_numpy(np.ascontiguousarray(arr))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"register_volumes: {what} has shape {tuple(t.shape)}, the fixed image {tuple(shape)}")
    return t.float().to(dev)


def register_volumes(fixedim, movingim, model, *, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth, grid_sp_adam=2,
                     ic=True, mask_fixed=None, mask_moving=None, fixed_minclip=None, fixed_maxclip=None, moving_minclip=None,
                     moving_maxclip=None, fixed_seg=None, moving_seg=None, downscale_feat_scalar=0.1):
    """The body of the reference's ``convex_adam`` between loading and saving (:152-266) on volumes in memory.  fixedim, movingim:
    numpy [H, W, D]; masks and label maps: numpy or tensors of that shape, both of a pair or neither.  Returns a dict with
    ``disp_hr`` [1, 3, H, W, D] (voxels), ``moved`` [1, 1, H, W, D], ``moved_seg`` (or None), ``dice`` / ``dice_per_label`` (or None),
    ``jacobian`` (the six ``JACOBIAN_STATS`` of the map x + disp_hr) and ``case_time`` (seconds, timed where the reference times:
    from the pooled features to the end of the instance optimisation).  As in the reference ``selected_niter <= 0`` skips the
    instance optimisation, and ``ic=False`` hands it the coarse stage-1 field; the two together raise ValueError (the reference
    fails there with a shape error in grid_sample)."""
    fixedim, movingim = np.ascontiguousarray(fixedim), np.ascontiguousarray(movingim)
    if fixedim.ndim != 3 or fixedim.shape != movingim.shape:
        raise ValueError(f"register_volumes: fixed {fixedim.shape} and moving {movingim.shape} must be 3-D volumes of one shape")
    if (mask_fixed is None) != (mask_moving is None):
        raise ValueError("register_volumes: give both masks or neither")
    if (fixed_seg is None) != (moving_seg is None):
        raise ValueError("register_volumes: give both label maps or neither")
    if not ic and selected_niter <= 0:
        raise ValueError("register_volumes: ic=False needs selected_niter >= 1 (stage 1 then returns the coarse field, which only the "
                         "instance optimisation brings to full resolution)")
    dev = next(model.parameters()).device
    use_mask = mask_fixed is not None
    if use_mask:
        mask_fixed = _device_volume(mask_fixed, dev, "mask_fixed", fixedim.shape)
        mask_moving = _device_volume(mask_moving, dev, "mask_moving", fixedim.shape)
    if fixed_seg is not None:
        fixed_seg = _device_volume(fixed_seg, dev, "fixed_seg", fixedim.shape)
        moving_seg = _device_volume(moving_seg, dev, "moving_seg", fixedim.shape)
    fixed_ch0 = torch.from_numpy(fixedim[np.newaxis, np.newaxis, ...]).float().to(dev)
    moving_ch0 = torch.from_numpy(movingim[np.newaxis, np.newaxis, ...]).float().to(dev)

    pred_fixed, pred_moving = extract_features(fixedim, movingim, model, fixed_minclip, fixed_maxclip, moving_minclip, moving_maxclip)
    pred_fixed = pred_fixed * downscale_feat_scalar
    pred_moving = pred_moving * downscale_feat_scalar
    _, _, features_fix, features_mov = merge_features(use_mask, pred_fixed, pred_moving, mask_fixed, mask_moving, fixed_ch0, moving_ch0)
    H, W, D = (int(v) for v in features_fix.shape[-3:])

    torch.cuda.synchronize(dev)
    t0 = time.time()
    with torch.no_grad():
        features_fix_smooth = F.avg_pool3d(features_fix, grid_sp, stride=grid_sp)
        features_mov_smooth = F.avg_pool3d(features_mov, grid_sp, stride=grid_sp)
    n_ch = features_fix_smooth.shape[1]
    disp_hr = run_stage1_registration(features_fix_smooth, features_mov_smooth, disp_hw, grid_sp, (H, W, D), n_ch, ic)
    if selected_niter > 0:
        if ic:
            disp_hr = run_instance_opt(disp_hr, features_fix, features_mov, grid_sp_adam, lambda_weight, (H, W, D), selected_niter,
                                       selected_smooth, lr=1)
        else:
            disp_hr = _instance_opt_from_coarse(disp_hr, features_fix, features_mov, grid_sp_adam, lambda_weight, (H, W, D),
                                                selected_niter, selected_smooth)
    torch.cuda.synchronize(dev)
    case_time = time.time() - t0

    out = {"disp_hr": disp_hr, "moved": warp_volume(moving_ch0, disp_hr, "bilinear"), "moved_seg": None, "dice": None,
           "dice_per_label": None, "case_time": case_time}
    if fixed_seg is not None:
        out["moved_seg"] = warp_volume(moving_seg[None, None], disp_hr, "nearest")
        out["dice"], out["dice_per_label"] = dice_score(fixed_seg, out["moved_seg"])
    out["jacobian"] = jacobian_statistics(disp_hr)
    return out


def result_names(moving_image, grid_sp, disp_hw, lambda_weight, grid_sp_adam, ic, expname):
    """The reference's file names (:146-150, :269-325) for the displacement field, the moved image and the moved label map."""
    fname = os.path.basename(moving_image)
    stem = fname[:-7] if fname.endswith(".nii.gz") else os.path.splitext(fname)[0]
    tail = "{}_g{}_hw{}_l{}_ga{}_ic{}_{}.nii.gz".format(stem, grid_sp, disp_hw, lambda_weight, grid_sp_adam, ic, expname)
    return "disp_" + tail, "moved_" + tail, "labels_moved_" + tail


def convex_adam(expname, lambda_weight, grid_sp, disp_hw, selected_niter, selected_smooth, ckpt_path=None, hf_variant=None,
                grid_sp_adam=2, ic=True, result_path='./', fixed_image=None, moving_image=None, use_mask=False, fixed_mask=None,
                moving_mask=None, fixed_minclip=None, fixed_maxclip=None, moving_minclip=None, moving_maxclip=None, warp_seg=False,
                fixed_seg=None, moving_seg=None, downscale_feat_scalar=0.1, num_downs=4, ngf=16, output_nc=16, norm="batch",
                interp="nearest", pooling="Max", *, model=None, weights_path=None):
    """run_convex_adam_with_network_feats.py:26-327, argument for argument.  Extensions of this package, keyword-only: ``model``
    (an already loaded network: nothing is loaded) and ``weights_path`` (passed to ``load_model``).  Writes ``disp_*`` as
    [H, W, D, 3], ``moved_*`` and, with ``warp_seg``, ``labels_moved_*`` under the reference's names with the fixed image's affine,
    prints the case time, the Dice score and the Jacobian statistics, and returns the dict of ``register_volumes`` with the
    paths added as ``disp_path``, ``moved_path`` and ``labels_moved_path`` (the reference returns None)."""
    if fixed_image is None or moving_image is None:
        raise ValueError("convex_adam: fixed_image and moving_image are required")
    if warp_seg and (fixed_seg is None or moving_seg is None):
        raise ValueError("convex_adam: warp_seg=True needs both fixed_seg and moving_seg")
    if use_mask and (fixed_mask is None or moving_mask is None):
        raise ValueError("convex_adam: use_mask=True needs both fixed_mask and moving_mask")
    if model is None:
        print('Loading model')
        model = load_model(ckpt_path=ckpt_path, hf_variant=hf_variant, num_downs=num_downs, ngf=ngf, output_nc=output_nc, norm=norm,
                           interp=interp, pooling=pooling, weights_path=weights_path)

    fixedim, affine_mtx, _ = load_nifti(fixed_image)
    movingim = load_nifti(moving_image)[0]
    masks = (load_nifti(fixed_mask)[0], load_nifti(moving_mask)[0]) if use_mask else (None, None)
    segs = (load_nifti(fixed_seg)[0], load_nifti(moving_seg)[0]) if warp_seg else (None, None)

    print('Running network on input images')
    res = register_volumes(fixedim, movingim, model, lambda_weight=lambda_weight, grid_sp=grid_sp, disp_hw=disp_hw,
                           selected_niter=selected_niter, selected_smooth=selected_smooth, grid_sp_adam=grid_sp_adam, ic=ic,
                           mask_fixed=masks[0], mask_moving=masks[1], fixed_minclip=fixed_minclip, fixed_maxclip=fixed_maxclip,
                           moving_minclip=moving_minclip, moving_maxclip=moving_maxclip, fixed_seg=segs[0], moving_seg=segs[1],
                           downscale_feat_scalar=downscale_feat_scalar)
    print('case time: ', res["case_time"])

    names = result_names(moving_image, grid_sp, disp_hw, lambda_weight, grid_sp_adam, ic, expname)
    disp_path, moved_path, labels_path = (os.path.join(result_path, n) for n in names)
    res["labels_moved_path"] = None
    if warp_seg:
        save_nifti(labels_path, res["moved_seg"].squeeze().cpu().numpy(), affine_mtx)
        res["labels_moved_path"] = labels_path
        print('Dice: {}'.format(res["dice"]))
    save_nifti(disp_path, res["disp_hr"].permute(0, 2, 3, 4, 1).squeeze().cpu().numpy(), affine_mtx)
    save_nifti(moved_path, res["moved"].squeeze().cpu().numpy(), affine_mtx)
    res["disp_path"], res["moved_path"] = disp_path, moved_path
    print('Jacobian: ' + ', '.join('{} {:.6g}'.format(k, res["jacobian"][k]) for k in JACOBIAN_STATS))
    return res


def build_parser():
    """The reference's command line (:331-464): flags, defaults, dests, the required ones and the exclusive checkpoint group."""
    parser = argparse.ArgumentParser(description="Run ConvexAdam optimization with network features on the HIP kernels.")
    parser.add_argument("--fixed", type=str, required=True, help="Path to the fixed image *.nii.gz file (required).")
    parser.add_argument("--moving", type=str, required=True, help="Path to the moving image *.nii.gz file (required).")
    parser.add_argument("--exp_name", type=str, required=True, help="Experiment name, part of the output file names (required).")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt_path", type=str, default=None, help="Path to a local .pth model checkpoint.")
    src.add_argument("--hf_variant", type=str, default=None, help="Registered variant name (e.g. 'anatomix', 'anatomix-dev').")
    for flag, typ, default, what in (("--num_downs", int, 4, "Number of downsampling layers in the U-Net"),
                                     ("--ngf", int, 16, "Channel multiplier of the U-Net"),
                                     ("--output_nc", int, 16, "Number of output feature channels"),
                                     ("--norm", str, "batch", "Normalization type ('batch', 'instance', 'none')"),
                                     ("--interp", str, "nearest", "Decoder upsampling mode ('nearest' or 'trilinear')"),
                                     ("--pooling", str, "Max", "Pooling type ('Max' or 'Avg')")):
        parser.add_argument(flag, type=typ, default=default, help=f"{what}. Default {default!r}. Only used with --ckpt_path.")
    parser.add_argument("--result_path", type=str, default='./', help="Directory for the results. Default: current directory.")
    parser.add_argument("--lambda_weight", type=float, default=0.75, help="Diffusion regularisation weight of the Adam stage. Default 0.75.")
    parser.add_argument("--grid_sp", type=int, default=2, help="Grid spacing of the discrete stage. Default 2.")
    parser.add_argument("--disp_hw", type=int, default=1, help="Half-width of the discrete search space. Default 1.")
    parser.add_argument('--selected_niter', type=int, default=80, help="Iterations of the Adam instance optimisation. Default 80.")
    parser.add_argument('--selected_smooth', type=int, default=0, help="Final box smoothing (3 or 5; anything else: none). Default 0.")
    parser.add_argument('--grid_sp_adam', type=int, default=2, help="Grid spacing of the Adam stage. Default 2.")
    parser.add_argument('--no-ic', action='store_false', dest='ic', help='Disable inverse consistency.')
    parser.add_argument('--use_mask', action='store_true', help='Use a registration mask.')
    parser.add_argument('--path_mask_fixed', type=str, default=None, help="With --use_mask: the *.nii.gz mask of the fixed image.")
    parser.add_argument('--path_mask_moving', type=str, default=None, help="With --use_mask: the *.nii.gz mask of the moving image.")
    parser.add_argument('--fixed_minclip', type=float, default=None, help="Clip the fixed image's intensities from below at this value.")
    parser.add_argument('--fixed_maxclip', type=float, default=None, help="Clip the fixed image's intensities from above at this value.")
    parser.add_argument('--moving_minclip', type=float, default=None, help="Clip the moving image's intensities from below at this value.")
    parser.add_argument('--moving_maxclip', type=float, default=None, help="Clip the moving image's intensities from above at this value.")
    parser.add_argument('--warp_seg', action='store_true', help='Warp the moving label map with the estimated deformation.')
    parser.add_argument('--path_seg_fixed', type=str, default=None, help="With --warp_seg: the *.nii.gz label map of the fixed image.")
    parser.add_argument('--path_seg_moving', type=str, default=None, help="With --warp_seg: the *.nii.gz label map of the moving image.")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    return convex_adam(expname=args.exp_name, lambda_weight=args.lambda_weight, grid_sp=args.grid_sp, disp_hw=args.disp_hw,
                       selected_niter=args.selected_niter, selected_smooth=args.selected_smooth, ckpt_path=args.ckpt_path,
                       hf_variant=args.hf_variant, grid_sp_adam=args.grid_sp_adam, ic=args.ic, result_path=args.result_path,
                       fixed_image=args.fixed, moving_image=args.moving, use_mask=args.use_mask, fixed_mask=args.path_mask_fixed,
                       moving_mask=args.path_mask_moving, fixed_minclip=args.fixed_minclip, fixed_maxclip=args.fixed_maxclip,
                       moving_minclip=args.moving_minclip, moving_maxclip=args.moving_maxclip, warp_seg=args.warp_seg,
                       fixed_seg=args.path_seg_fixed, moving_seg=args.path_seg_moving, num_downs=args.num_downs, ngf=args.ngf,
                       output_nc=args.output_nc, norm=args.norm, interp=args.interp, pooling=args.pooling)


if __name__ == "__main__":
    main()
