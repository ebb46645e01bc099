"""Feature side of the registration pipeline with the surface of ``anatomix.registration.convex_adam_utils``:
model loading, min-max normalisation and sliding-window feature extraction (reference lines 16-78, 134-221), and the
feature post-processing that runs on the extracted tensors before the convex optimisation -- ``MINDSSC`` (:311-406),
``apply_avg_pool3d`` (:105-131) and the SSD correlation volume ``correlate`` (:409-491) -- on the HIP kernels of
``csrc/amx_regfeat.hip``; and the discrete solver that follows them, ``coupled_convex`` (:494-552) and
``inverse_consistency`` (:555-603), on the kernels of ``csrc/amx_regsolve.hip``.  The Adam instance optimisation lives in
``instance_optimization.py`` (its regulariser, ``diffusion_regularizer`` :81-102, is fused into the gradient kernel of
``csrc/amx_reginstopt.hip``).  The Jacobian utilities ``generate_grid`` and ``JacobianDet`` (:226-282) are here too, the
determinant and its statistics on the kernel of ``csrc/amx_regmetrics.hip`` (``jacobian_determinant`` is the direct route
from a displacement field); the label-overlap side of that file is in ``metrics.py``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from .. import _lib
from ..model.load_from_hf import ANATOMIX_VARIANTS, _load_handling_compile, load_from_hf  # noqa: F401
from ..model.network import Unet
from .sliding_window import sliding_window_inference


def load_model(ckpt_path=None, hf_variant=None, *, num_downs=4, ngf=16, output_nc=16, norm="batch", interp="nearest",
               pooling="Max", device=None, weights_path=None):
    """convex_adam_utils.py:16-78.  Exactly one of ``ckpt_path`` / ``hf_variant``; the architecture arguments are
    keyword-only and only used with ``ckpt_path`` (a variant brings its own).  ``hf_variant`` goes through
    ``load_from_hf`` (Hub download, or the local ``weights_path=`` extension of this package where there is no network),
    so the returned model ALWAYS carries loaded weights.  Returned in eval mode on ``device`` (default: cuda if present)."""
    if (ckpt_path is None) == (hf_variant is None):
        raise ValueError("Provide exactly one of `ckpt_path` or `hf_variant`.")
    if hf_variant is not None:
        model = load_from_hf(hf_variant, weights_path=weights_path)
    elif ckpt_path == "scratch":
        raise ValueError("'scratch' is not supported for registration; registration requires pretrained weights.")
    else:
        if not os.path.isfile(ckpt_path):
            raise FileNotFoundError(f"Checkpoint file not found: {ckpt_path}")
        model = Unet(3, 1, output_nc, num_downs, ngf=ngf, norm=norm, interp=interp, pooling=pooling)
        model = _load_handling_compile(model, torch.load(ckpt_path, map_location="cpu"))
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model.to(device)
    model.eval()
    return model


def minmax(arr, minclip=None, maxclip=None):
    """convex_adam_utils.py:134-156.  The reference's condition ``not (minclip is None) & (maxclip is
    None)`` parses as ``not (both None)``: clipping is applied as soon as EITHER bound is given
    (np.clip accepts None for the other).  No zero-range guard, as in the reference."""
    if not ((minclip is None) and (maxclip is None)):
        arr = np.clip(arr, minclip, maxclip)
    return (arr - arr.min()) / (arr.max() - arr.min())


def extract_features(img_fixed, img_moving, model, fixminclip=None, fixmaxclip=None, movminclip=None, movmaxclip=None,
                     group=None):
    """convex_adam_utils.py:159-221: min-max normalise, then 128^3 / overlap 0.8 / gaussian(0.25)
    sliding-window inference of both volumes.  Returns (fixed_features, moving_features), each
    [1, C, D, H, W] on the model's device."""
    dev = next(model.parameters()).device
    outs = []
    for img, lo, hi in ((img_fixed, fixminclip, fixmaxclip), (img_moving, movminclip, movmaxclip)):
        im = torch.from_numpy(np.ascontiguousarray(minmax(img, lo, hi)))[None, None, ...].float().to(dev)
        with torch.no_grad():
            outs.append(sliding_window_inference(im, (128, 128, 128), 2, model, overlap=0.8, mode="gaussian",
                                                 sigma_scale=0.25, group=group))
    return outs[0], outs[1]


# ---- feature post-processing on the HIP kernels (fp32, batch 1, like the reference's tensors) -------------------------

def _f32c(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the registration feature kernels run on the GPU (got a {t.device} tensor); there is no CPU path")
    return _lib.f32c(t)


def MINDSSC(img, radius=2, dilation=2):
    """convex_adam_utils.py:311-406.  img [1, 1, H, W, D] -> MIND-SSC descriptor [1, 12, H, W, D] (fp32).  Unlike the
    reference there is no host synchronisation: the global mean used for the variance clamp (:389-393) stays on the GPU."""
    if img.dim() != 5 or img.shape[0] != 1 or img.shape[1] != 1:
        raise ValueError(f"MINDSSC expects [1, 1, H, W, D] (got {tuple(img.shape)})")
    lib = _lib.load()
    x = _f32c(img, "MINDSSC")
    _, _, h, w, d = x.shape
    out = torch.empty((1, 12, h, w, d), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        nb = lib.amx_mindssc_scratch_bytes(h, w, d)
        sc = torch.empty(nb, dtype=torch.uint8, device=x.device)
        _lib.check(lib.amx_mindssc(_lib.ptr(x), h, w, d, int(radius), int(dilation), _lib.ptr(out), _lib.ptr(sc), nb,
                                   _lib.stream(x.device)))
    return out


def apply_avg_pool3d(disp_hr, kernel_size, num_repeats):
    """convex_adam_utils.py:105-131: ``num_repeats`` x F.avg_pool3d(kernel_size, padding=kernel_size // 2, stride=1).
    disp_hr [1, C, H, W, D] (forward only: the instance optimisation does not differentiate through this function, its
    smoothing and adjoint are ``instance_opt_smooth3``)."""
    if disp_hr.dim() != 5 or disp_hr.shape[0] != 1:
        raise ValueError(f"apply_avg_pool3d expects [1, C, H, W, D] (got {tuple(disp_hr.shape)})")
    if disp_hr.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("apply_avg_pool3d on the HIP kernels is forward-only")
    lib = _lib.load()
    x = _f32c(disp_hr, "apply_avg_pool3d")
    _, c, h, w, d = x.shape
    with torch.cuda.device(x.device):
        for _ in range(int(num_repeats)):
            y = torch.empty_like(x)
            _lib.check(lib.amx_box_filter3d(_lib.ptr(x), _lib.ptr(y), c, h, w, d, int(kernel_size), _lib.stream(x.device)))
            x = y
    return x


def smooth_merged_features(mind, pred, grid_sp, downscale_feat_scalar=0.1):
    """``F.avg_pool3d(cat([mind, pred * downscale_feat_scalar], 1), grid_sp, stride=grid_sp)`` in one pass
    (run_convex_adam_with_network_feats.py:164-205 + instance_optimization.py:111-117) without materialising the scaled
    copy and the 28-channel concat at full resolution.  mind [1, 12, H, W, D] or None, pred [1, C, H, W, D]."""
    lib = _lib.load()
    b = _f32c(pred, "smooth_merged_features")
    a = None if mind is None else _f32c(mind, "smooth_merged_features")
    _, cb, h, w, d = b.shape
    ca = 0 if a is None else a.shape[1]
    g = int(grid_sp)
    out = torch.empty((1, ca + cb, h // g, w // g, d // g), dtype=torch.float32, device=b.device)
    with torch.cuda.device(b.device):
        _lib.check(lib.amx_avg_pool3d_cat(_lib.ptr(a), ca, 1.0, _lib.ptr(b), cb, float(downscale_feat_scalar), h, w, d, g,
                                          _lib.ptr(out), _lib.stream(b.device)))
    return out


def correlate(mind_fix, mind_mov, disp_hw, grid_sp, shape, ch=12):
    """convex_adam_utils.py:409-491.  mind_fix, mind_mov [1, ch, H/grid_sp, W/grid_sp, D/grid_sp] ->
    (ssd [(2 disp_hw + 1)^3, h, w, d], ssd_argmin int64 [h, w, d])."""
    lib = _lib.load()
    f = _f32c(mind_fix, "correlate")
    m = _f32c(mind_mov, "correlate")
    h, w, d = int(shape[0]) // grid_sp, int(shape[1]) // grid_sp, int(shape[2]) // grid_sp
    if tuple(f.shape) != (1, ch, h, w, d) or tuple(m.shape) != tuple(f.shape):
        raise ValueError(f"correlate: features {tuple(f.shape)} / {tuple(m.shape)} do not match (1, {ch}, {h}, {w}, {d})")
    k = 2 * int(disp_hw) + 1
    ssd = torch.empty((k ** 3, h, w, d), dtype=torch.float32, device=f.device)
    amin = torch.empty((h, w, d), dtype=torch.int64, device=f.device)
    with torch.cuda.device(f.device):
        nb = lib.amx_correlate_scratch_bytes(h, w, d, int(disp_hw))
        sc = torch.empty(nb, dtype=torch.uint8, device=f.device)
        _lib.check(lib.amx_correlate_ssd(_lib.ptr(f), _lib.ptr(m), ch, h, w, d, int(disp_hw), _lib.ptr(ssd), _lib.ptr(amin),
                                         _lib.ptr(sc), nb, _lib.stream(f.device)))
    return ssd, amin


def _disp_hw_of(n_labels):
    for hw in (1, 2, 3):
        if (2 * hw + 1) ** 3 == n_labels:
            return hw
    raise ValueError(f"ssd has {n_labels} displacement labels; expected (2 disp_hw + 1)^3 with disp_hw in {{1, 2, 3}}")


def _check_regular_mesh(disp_mesh_t, disp_hw):
    """The kernels generate the mesh from the label index, so only the regular mesh of run_stage1_registration is
    accepted: F.affine_grid(disp_hw * eye(3, 4), (1, 1, k, k, k), align_corners=True) as [3, k^3(, 1)], any float dtype.
    Checked by shape and the two extreme rows."""
    n = (2 * disp_hw + 1) ** 3
    if disp_mesh_t is None or disp_mesh_t.numel() != 3 * n or disp_mesh_t.shape[0] != 3:
        raise ValueError(f"coupled_convex: disp_mesh_t must be the regular [3, {n}] displacement mesh of "
                         f"run_stage1_registration (got {None if disp_mesh_t is None else tuple(disp_mesh_t.shape)})")
    m = disp_mesh_t.reshape(3, n)
    ends = torch.stack([m[:, 0], m[:, n - 1]]).float().cpu().tolist()
    if ends != [[-float(disp_hw)] * 3, [float(disp_hw)] * 3]:
        raise ValueError("coupled_convex: only the regular integer mesh -disp_hw .. disp_hw of run_stage1_registration is "
                         f"supported (the kernel generates it from the label index); got extreme rows {ends}")


def coupled_convex(ssd, ssd_argmin, disp_mesh_t, grid_sp, shape):
    """convex_adam_utils.py:494-552.  ssd [(2 disp_hw + 1)^3, h, w, d] and ssd_argmin [h, w, d] (or None: recomputed) as
    ``correlate`` returns them, (h, w, d) = shape // grid_sp -> disp_soft [1, 3, h, w, d] in grid units.  ``disp_mesh_t``
    is accepted for signature compatibility and must be the regular mesh (see _check_regular_mesh); ``disp_hw`` is inferred
    from ``ssd.shape[0]``.  Two documented differences from the reference: ``ssd`` is NOT modified (the reference
    accumulates the coupling penalty into it through a view -- the accumulation itself is reproduced), and the result is
    fp32 whatever the mesh's dtype (the reference returns the mesh's dtype, half in its own caller)."""
    hw = _disp_hw_of(int(ssd.shape[0]))
    _check_regular_mesh(disp_mesh_t, hw)
    s = _f32c(ssd, "coupled_convex")
    h, w, d = int(shape[0]) // grid_sp, int(shape[1]) // grid_sp, int(shape[2]) // grid_sp
    if tuple(s.shape[1:]) != (h, w, d):
        raise ValueError(f"coupled_convex: ssd {tuple(s.shape)} does not match the grid ({h}, {w}, {d})")
    amin = None
    if ssd_argmin is not None:
        if not ssd_argmin.is_cuda or ssd_argmin.numel() != h * w * d:
            raise ValueError("coupled_convex: ssd_argmin must be a device tensor of h * w * d labels (or None)")
        amin = ssd_argmin.to(torch.int64).contiguous()
    lib = _lib.load()
    out = torch.empty((1, 3, h, w, d), dtype=torch.float32, device=s.device)
    with torch.cuda.device(s.device):
        nb = lib.amx_coupled_convex_scratch_bytes(h, w, d)
        sc = torch.empty(nb, dtype=torch.uint8, device=s.device)
        _lib.check(lib.amx_coupled_convex(_lib.ptr(s), _lib.ptr(amin), h, w, d, hw, _lib.ptr(out), _lib.ptr(sc), nb,
                                          _lib.stream(s.device)))
    return out


def coupled_convex_step(ssd, soft_history):
    """One iteration of ``coupled_convex`` from given state (extension of this package; ``coupled_convex`` is seven of
    these on the device).  ``soft_history``: the soft fields s_0 .. s_{j-1} so far, each [1, 3, h, w, d] (empty: the plain
    argmin).  Returns (labels int64 [h, w, d], s_j [1, 3, h, w, d])."""
    hw = _disp_hw_of(int(ssd.shape[0]))
    s = _f32c(ssd, "coupled_convex_step")
    h, w, d = (int(v) for v in s.shape[1:])
    j = len(soft_history)
    hist = None
    if j:
        hist = torch.stack([_f32c(t, "coupled_convex_step").reshape(3, h, w, d) for t in soft_history]).contiguous()
    lib = _lib.load()
    out = torch.empty((1, 3, h, w, d), dtype=torch.float32, device=s.device)
    lab = torch.empty((h, w, d), dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        nb = lib.amx_coupled_convex_step_scratch_bytes(h, w, d)
        sc = _lib.scratch(nb, s.device)
        _lib.check(lib.amx_coupled_convex_step(_lib.ptr(s), _lib.ptr(hist), j, h, w, d, hw, _lib.ptr(out), _lib.ptr(lab),
                                               _lib.ptr(sc), nb, _lib.stream(s.device)))
    return lab, out


def inverse_consistency(disp_field1s, disp_field2s, iterations=20):
    """convex_adam_utils.py:555-603.  Two fields [1, 3, h, w, d] in normalised coordinates (channel 0 = last axis) ->
    (disp_field1i, disp_field2i) after ``iterations`` Jacobi sweeps, one kernel launch per sweep; inputs untouched."""
    a = _f32c(disp_field1s, "inverse_consistency")
    b = _f32c(disp_field2s, "inverse_consistency")
    if a.dim() != 5 or a.shape[0] != 1 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError(f"inverse_consistency expects two [1, 3, h, w, d] fields (got {tuple(a.shape)}, {tuple(b.shape)})")
    _, _, h, w, d = a.shape
    lib = _lib.load()
    o1, o2 = torch.empty_like(a), torch.empty_like(b)
    with torch.cuda.device(a.device):
        nb = lib.amx_inverse_consistency_scratch_bytes(h, w, d)
        sc = _lib.scratch(nb, a.device)
        _lib.check(lib.amx_inverse_consistency(_lib.ptr(a), _lib.ptr(b), h, w, d, int(iterations), _lib.ptr(o1), _lib.ptr(o2),
                                               _lib.ptr(sc), nb, _lib.stream(a.device)))
    return o1, o2


def resize_trilinear(x, size, scale=None, flip_channels=False):
    """``F.interpolate(x.flip(1) * scale.view(1, -1, 1, 1, 1), size=size, mode="trilinear", align_corners=False)`` in one
    pass (extension of this package; flip and scale optional): x [1, C, h, w, d] -> [1, C, *size].  ``scale``: C floats."""
    t = _f32c(x, "resize_trilinear")
    if t.dim() != 5 or t.shape[0] != 1:
        raise ValueError(f"resize_trilinear expects [1, C, h, w, d] (got {tuple(t.shape)})")
    _, c, h, w, d = t.shape
    H, W, D = (int(v) for v in size)
    sc = None
    if scale is not None:
        vals = [float(v) for v in scale]
        if len(vals) != c:
            raise ValueError(f"resize_trilinear: {len(vals)} scales for {c} channels")
        sc = (ctypes.c_float * c)(*vals)
    lib = _lib.load()
    out = torch.empty((1, c, max(H, 0), max(W, 0), max(D, 0)), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _lib.check(lib.amx_resize_trilinear3d(_lib.ptr(t), c, h, w, d, _lib.ptr(out), H, W, D, sc, int(bool(flip_channels)),
                                              _lib.stream(t.device)))
    return out


def stage1_inputs(img_fixed, img_moving, model, grid_sp=2, disp_hw=1, downscale_feat_scalar=0.1, fixminclip=None,
                  fixmaxclip=None, movminclip=None, movmaxclip=None, group=None):
    """Everything the reference computes between loading the two volumes and its convex solver
    (run_convex_adam_with_network_feats.py:153-205 -> instance_optimization.run_stage1_registration's ``correlate`` call):
    min-max + sliding-window features of both volumes, MIND-SSC(1, 2) of both, ``cat(mind, 0.1 * features)`` pooled by
    ``grid_sp``, and the SSD correlation volume fixed -> moving.  img_* are numpy volumes [H, W, D].
    Returns a dict(features_fix_smooth, features_mov_smooth, ssd, ssd_argmin, mind_fixed, mind_moving, pred_fixed,
    pred_moving); all device tensors, no host synchronisation after the inputs are uploaded."""
    pred_f, pred_m = extract_features(img_fixed, img_moving, model, fixminclip, fixmaxclip, movminclip, movmaxclip, group=group)
    dev = pred_f.device
    out = {"pred_fixed": pred_f, "pred_moving": pred_m}
    smooth = []
    for name, img, lo, hi, pred in (("fixed", img_fixed, fixminclip, fixmaxclip, pred_f), ("moving", img_moving, movminclip, movmaxclip, pred_m)):
        im = torch.from_numpy(np.ascontiguousarray(minmax(img, lo, hi)))[None, None, ...].float().to(dev)
        mind = MINDSSC(im, 1, 2)                                      # merge_features, instance_optimization.py:107-108
        out["mind_" + name] = mind
        smooth.append(smooth_merged_features(mind, pred, grid_sp, downscale_feat_scalar))
    out["features_fix_smooth"], out["features_mov_smooth"] = smooth
    h, w, d = (int(v) for v in pred_f.shape[-3:])
    out["ssd"], out["ssd_argmin"] = correlate(smooth[0], smooth[1], disp_hw, grid_sp, (h, w, d), smooth[0].shape[1])
    return out


# ---- Jacobian determinant (csrc/amx_regmetrics.hip) -------------------------------------------------------------------------

JACOBIAN_STATS = ("folding_fraction", "min", "max", "mean", "log_mean", "log_std")


def generate_grid(imgshape):
    """convex_adam_utils.py:226-246: the integer coordinate grid [H, W, D, 3] of a volume, numpy int64.  Component c holds the
    index along axis 2 - c (the last component is the index along the first axis), exactly as the reference builds it."""
    h, w, d = (int(v) for v in imgshape[:3])
    i, j, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(d), indexing="ij")
    return np.stack([k, j, i], axis=-1)


def _jacobian_call(field, add_identity, want_field, want_stats):
    """field: contiguous fp32 device tensor [3, H, W, D], channel a along axis a."""
    lib = _lib.load()
    _, h, w, d = (int(v) for v in field.shape)
    jdet = torch.empty((h - 1, w - 1, d - 1), dtype=torch.float32, device=field.device) if want_field else None
    stats = torch.empty(6, dtype=torch.float32, device=field.device) if want_stats else None
    with torch.cuda.device(field.device):
        nb = lib.amx_jacobian_det_scratch_bytes(h, w, d) if want_stats else 0
        sc = torch.empty(max(nb, 8), dtype=torch.uint8, device=field.device) if want_stats else None
        _lib.check(lib.amx_jacobian_det(_lib.ptr(field), h, w, d, int(add_identity), _lib.ptr(jdet), _lib.ptr(stats), _lib.ptr(sc),
                                        nb, _lib.stream(field.device)))
    return jdet, stats


def jacobian_determinant(disp_hr, return_stats=False):
    """Jacobian determinant of the map x + disp_hr for a displacement field [1, 3, H, W, D] in voxels (channel a along axis a,
    what ``run_instance_opt`` returns and ``warp_volume`` takes) -> [1, H-1, W-1, D-1] of forward differences, equal to the
    reference's ``JacobianDet(disp_hr.permute(0, 2, 3, 4, 1).flip(-1), generate_grid((H, W, D)))`` without forming the grid.
    With ``return_stats`` also a float32 device tensor of the six ``JACOBIAN_STATS`` taken over that field in the same pass."""
    if disp_hr.dim() != 5 or disp_hr.shape[0] != 1 or disp_hr.shape[1] != 3 or min(disp_hr.shape[2:]) < 2:
        raise ValueError(f"jacobian_determinant expects [1, 3, H, W, D] with H, W, D >= 2 (got {tuple(disp_hr.shape)})")
    x = _f32c(disp_hr, "jacobian_determinant")
    jdet, stats = _jacobian_call(x[0], 1, True, bool(return_stats))
    return (jdet[None], stats) if return_stats else jdet[None]


def jacobian_statistics(disp_hr):
    """The six ``JACOBIAN_STATS`` of the map x + disp_hr ([1, 3, H, W, D], voxels) as a dict of floats, without writing the
    determinant field (one pass over the displacement field; reads the result back, so it synchronises)."""
    if disp_hr.dim() != 5 or disp_hr.shape[0] != 1 or disp_hr.shape[1] != 3 or min(disp_hr.shape[2:]) < 2:
        raise ValueError(f"jacobian_statistics expects [1, 3, H, W, D] with H, W, D >= 2 (got {tuple(disp_hr.shape)})")
    _, stats = _jacobian_call(_f32c(disp_hr, "jacobian_statistics")[0], 1, False, True)
    return dict(zip(JACOBIAN_STATS, stats.tolist()))


def JacobianDet(y_pred, sample_grid):
    """convex_adam_utils.py:249-282.  y_pred [N, H, W, D, 3] (component c along axis 2 - c, as ``generate_grid``) and the grid
    (tensor or numpy, broadcastable) -> [N, H-1, W-1, D-1].  On a device tensor the sum is formed as the reference forms it, its
    components are put into axis order and the kernel differences that map (add_identity = 0), one call per sample; on a CPU
    tensor this is the reference's arithmetic in plain torch."""
    if not torch.is_tensor(sample_grid):
        sample_grid = torch.from_numpy(np.ascontiguousarray(sample_grid)).to(y_pred.device)
    if y_pred.dim() != 5 or y_pred.shape[-1] != 3 or min(y_pred.shape[1:4]) < 2:
        raise ValueError(f"JacobianDet expects [N, H, W, D, 3] with H, W, D >= 2 (got {tuple(y_pred.shape)})")
    J = y_pred + sample_grid
    if not J.is_cuda:
        base = J[:, :-1, :-1, :-1, :]
        dy, dx, dz = J[:, 1:, :-1, :-1, :] - base, J[:, :-1, 1:, :-1, :] - base, J[:, :-1, :-1, 1:, :] - base
        det0 = dx[..., 0] * (dy[..., 1] * dz[..., 2] - dy[..., 2] * dz[..., 1])
        det1 = dx[..., 1] * (dy[..., 0] * dz[..., 2] - dy[..., 2] * dz[..., 0])
        det2 = dx[..., 2] * (dy[..., 0] * dz[..., 1] - dy[..., 1] * dz[..., 0])
        return det0 - det1 + det2
    maps = J.float().flip(-1).permute(0, 4, 1, 2, 3).contiguous()
    return torch.stack([_jacobian_call(m, 0, True, False)[0] for m in maps])
