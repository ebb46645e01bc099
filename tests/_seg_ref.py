"""Independent restatement, in plain torch and for any floating dtype, of the segmentation loss the reference takes from MONAI
(``DiceCELoss`` / ``DiceLoss`` with ``softmax=True, to_onehot_y=True``; train_segmentation.py:105-111), of its closed-form
gradient and of the 1x1x1 head in front of it.  It imports nothing from anatomix_amd.  MONAI cannot be imported here: parity with
it is unpinned, the documented algorithm is what these lines state.

    p = softmax(z, 1), t = one_hot(y, C);  per sample b and class c: I = sum_v p t, P = sum_v p, G = sum_v t
    dice = mean over (b, c in S) of 1 - (2 I + smooth_nr) / (G + P + smooth_dr),  S = {1 .. C-1}, or {0 .. C-1} with include_background
    ce   = mean over all B V voxels of -log p[y]      (all classes)
    loss = lambda_dice dice + lambda_ce ce
"""
import numpy as np
import torch


def one_hot(y, C, dtype):
    """y [B, 1, ...] (any dtype; truncated toward zero as .long()) -> [B, C, V]"""
    idx = y.reshape(y.shape[0], 1, -1).long()
    t = torch.zeros((y.shape[0], C, idx.shape[2]), dtype=dtype)
    return t.scatter_(1, idx, 1.0)


def head_logits(x, w, b):
    """z = W x + b per voxel: x [B, F, ...], w [C, F], b [C] -> [B, C, ...]"""
    z = torch.einsum("cf,bfv->bcv", w, x.reshape(x.shape[0], x.shape[1], -1)) + b.view(1, -1, 1)
    return z.reshape((x.shape[0], w.shape[0]) + tuple(x.shape[2:]))


def dice_ce(z, y, include_background=False, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0, lambda_ce=1.0):
    """(total, dice, ce) in z's dtype."""
    B, C = z.shape[:2]
    zz = z.reshape(B, C, -1)
    t = one_hot(y, C, z.dtype)
    m = zz.max(dim=1, keepdim=True).values
    e = (zz - m).exp()
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    I, P, G = (p * t).sum(2), p.sum(2), t.sum(2)
    f = 1.0 - (2.0 * I + smooth_nr) / (G + P + smooth_dr)
    if not include_background:
        f = f[:, 1:]
    dice = f.sum() / f.numel()
    logp = (zz - m) - s.log()
    ce = -(logp * t).sum() / (B * zz.shape[2])
    return lambda_dice * dice + lambda_ce * ce, dice, ce


def closed_form_grad(z, y, include_background=False, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0, lambda_ce=1.0):
    """d loss / d z written out: with N = B |S| and den = G + P + smooth_dr,
    d dice / d p_c(v) = alpha_bc t_c(v) + beta_bc, alpha = -2 / (N den), beta = (2 I + smooth_nr) / (N den^2), both 0 outside S;
    through the softmax  p_k (g_k - sum_c p_c g_c);  the cross-entropy part is (p_k - t_k) / (B V)."""
    B, C = z.shape[:2]
    zz = z.reshape(B, C, -1)
    V = zz.shape[2]
    t = one_hot(y, C, z.dtype)
    p = torch.softmax(zz, dim=1)
    I, P, G = (p * t).sum(2), p.sum(2), t.sum(2)
    first = 0 if include_background else 1
    N = B * (C - first)
    den = G + P + smooth_dr
    alpha, beta = -2.0 / (N * den), (2.0 * I + smooth_nr) / (N * den * den)
    alpha[:, :first] = 0
    beta[:, :first] = 0
    g = alpha.unsqueeze(2) * t + beta.unsqueeze(2)
    dz = lambda_dice * p * (g - (p * g).sum(1, keepdim=True)) + lambda_ce * (p - t) / (B * V)
    return dz.reshape(z.shape)


def make_inputs(B, F, C, spatial, seed=1):
    """RandomState(seed): normal features, W ~ N(0, 1 / F), b ~ N(0, 0.1) (variances), uniform labels with the last class of
    sample 0 relabelled to 0, so that one (b, c) has G = 0; logits for the logits mode (normal, scale 2).  numpy, fp32 / int64."""
    rs = np.random.RandomState(seed)
    x = rs.randn(B, F, *spatial).astype(np.float32)
    w = (rs.randn(C, F) / np.sqrt(F)).astype(np.float32)
    b = (rs.randn(C) * np.sqrt(0.1)).astype(np.float32)
    y = rs.randint(0, C, size=(B, 1) + tuple(spatial)).astype(np.int64)
    y[0][y[0] == C - 1] = 0
    z = (2.0 * rs.randn(B, C, *spatial)).astype(np.float32)
    return x, w, b, y, z
