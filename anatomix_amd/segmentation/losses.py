"""The losses and the post-transform of the reference's segmentation finetuning (train_segmentation.py:84-86, :105-111,
:144-146, :200), which it takes from MONAI: ``DiceCELoss`` / ``DiceLoss`` with ``softmax=True, to_onehot_y=True``, and
softmax -> argmax.  CUDA tensors run on csrc/amx_segloss.hip (forward, backward, arg-max; the 1x1x1 head fused in
``head_dice_ce``); CPU tensors evaluate the same definition with torch ops (``dice_ce_torch``).

Definition (MONAI is not a dependency; parity with an installed MONAI is not pinned): p = softmax(logits, 1),
t = one_hot(labels), per sample b and class c  I = sum_v p t, P = sum_v p, G = sum_v t,
    dice = mean over (b, c in S) of 1 - (2 I + smooth_nr) / (G + P + smooth_dr)     S: all classes, without 0 unless include_background
    ce   = mean over all voxels of -log p[label]                                     every class, as nn.CrossEntropyLoss
    loss = lambda_dice * dice + lambda_ce * ce
A label outside [0, C) makes the loss NaN and is counted in ``last_bad_labels``."""
from __future__ import annotations


import torch
import torch.nn as nn

from .. import _lib
from ..model.network import Unet
from ..model.vit3d.architectures import PrimusV2

MAX_CLASSES, MAX_HEAD_CHANNELS = 32, 64
CALLS = {"head": 0, "logits": 0}          # how often each fused autograd Function ran (tests, diagnostics)


def dice_ce_torch(logits, labels, include_background=True, smooth_nr=1e-5, smooth_dr=1e-5, lambda_dice=1.0, lambda_ce=1.0):
    """The definition above in torch ops, in the dtype of ``logits`` (differentiable): (total, dice, ce, bad label count)."""
    B, C = logits.shape[:2]
    z = logits.reshape(B, C, -1)
    y = labels.reshape(B, -1).long()
    logp = torch.log_softmax(z, dim=1)
    p = logp.exp()
    t = (y.unsqueeze(1) == torch.arange(C, device=z.device).view(1, C, 1)).to(z.dtype)
    inter, psum, gsum = (p * t).sum(2), p.sum(2), t.sum(2)
    f = 1.0 - (2.0 * inter + smooth_nr) / (gsum + psum + smooth_dr)
    dice = (f if include_background else f[:, 1:]).mean()
    ce = -(logp * t).sum() / (B * z.shape[2]) if lambda_ce != 0 else torch.zeros((), dtype=z.dtype, device=z.device)
    bad = ((y < 0) | (y >= C)).sum()
    nan = torch.full((), float("nan"), dtype=z.dtype, device=z.device)
    total, dice, ce = (torch.where(bad > 0, nan, v) for v in (lambda_dice * dice + lambda_ce * ce, dice, ce))
    return total, dice, ce, bad


def _envelope(classes, feat):
    if not 2 <= classes <= MAX_CLASSES:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_INVALID, f"segmentation loss kernels: 2 <= classes <= {MAX_CLASSES} (got {classes})")
    if feat is not None and not 1 <= feat <= MAX_HEAD_CHANNELS:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_INVALID,
                                    f"segmentation loss kernels: 1 <= head input channels <= {MAX_HEAD_CHANNELS} (got {feat})")


def _labels_arg(labels, B, V):
    """Contiguous labels [B * V] in one of the dtypes the kernels read directly, and its dtype code."""
    if labels.numel() != B * V or labels.shape[0] != B:
        raise ValueError(f"labels {tuple(labels.shape)} do not match the input's batch {B} and {V} voxels ([B, 1, D, H, W])")
    if labels.dtype not in (torch.float32, torch.int64, torch.uint8):
        labels = labels.float() if labels.is_floating_point() else labels.long()
    return labels.contiguous(), _lib.SEG_LABEL[str(labels.dtype).split(".")[1]]


class _Cfg:
    def __init__(self, loss):
        self.include_background = bool(loss.include_background)
        self.smooth_nr, self.smooth_dr = float(loss.smooth_nr), float(loss.smooth_dr)
        self.lambda_dice, self.lambda_ce = float(loss.lambda_dice), float(loss.lambda_ce)

    def tail(self):
        return (int(self.include_background), self.smooth_nr, self.smooth_dr, self.lambda_dice, self.lambda_ce)


class _SegLossFn(torch.autograd.Function):
    """([total, dice, ce], bad label count) of amx_seg_loss_forward; the backward is amx_seg_loss_backward from the saved
    inputs and statistics.  ``weight`` None: ``x`` holds the logits [B, C, ...]; otherwise the features [B, F, ...] of the
    head ``weight`` [C, F], ``bias`` [C] or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, labels, cfg):
        head = weight is not None
        B = x.shape[0]
        C = weight.shape[0] if head else x.shape[1]
        F = x.shape[1] if head else 0
        _envelope(C, F if head else None)
        V = x[0, 0].numel()
        xc = _lib.f32c(x.detach())
        w = _lib.f32c(weight.detach()).reshape(C, F) if head else None
        b = _lib.f32c(bias.detach()) if (head and bias is not None) else None
        lab, lt = _labels_arg(labels, B, V)
        lib = _lib.load()
        dev = xc.device
        loss3 = torch.empty(3, dtype=torch.float32, device=dev)
        stats = torch.empty((B, C, 3), dtype=torch.float32, device=dev)
        bad = torch.empty(1, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            nb = lib.amx_seg_loss_scratch_bytes(B, V, C, F)
            sc = _lib.scratch(nb, dev)
            _lib.check_envelope(lib.amx_seg_loss_forward(_lib.ptr(xc), F, _lib.ptr(w), _lib.ptr(b), _lib.ptr(lab), lt, B, C, V, *cfg.tail(),
                                _lib.ptr(loss3), _lib.ptr(stats), _lib.ptr(bad), _lib.ptr(sc), nb, _lib.stream(dev)))
        CALLS["head" if head else "logits"] += 1
        ctx.save_for_backward(xc, w, b, lab, stats)
        ctx.cfg, ctx.lt, ctx.dims = cfg, lt, (B, C, F, V)
        ctx.x_meta = (x.shape, x.dtype)
        ctx.w_meta = (weight.shape, weight.dtype) if head else None
        ctx.b_dtype = bias.dtype if (head and bias is not None) else None
        ctx.mark_non_differentiable(bad)
        return loss3, bad

    @staticmethod
    def backward(ctx, gout, _gb):
        xc, w, b, lab, stats = ctx.saved_tensors
        B, C, F, V = ctx.dims
        head = F > 0
        lib = _lib.load()
        dev = xc.device
        g = _lib.f32c(gout.detach())           # d / d {total, dice, ce}: the kernel reads element 0; the components are handed out detached
        dx = torch.empty_like(xc)
        dw = torch.empty((C, F), dtype=torch.float32, device=dev) if head else None
        db = torch.empty(C, dtype=torch.float32, device=dev) if head else None
        with torch.cuda.device(dev):
            nb = lib.amx_seg_loss_scratch_bytes(B, V, C, F) if head else 0
            sc = _lib.scratch(nb, dev) if head else None
            _lib.check_envelope(lib.amx_seg_loss_backward(_lib.ptr(xc), F, _lib.ptr(w), _lib.ptr(b), _lib.ptr(lab), ctx.lt, B, C, V,
                                *ctx.cfg.tail(), _lib.ptr(stats), _lib.ptr(g), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(sc), nb,
                                _lib.stream(dev)))
        gx = dx.view(ctx.x_meta[0]).to(ctx.x_meta[1]) if ctx.needs_input_grad[0] else None
        gw = dw.view(ctx.w_meta[0]).to(ctx.w_meta[1]) if (head and ctx.needs_input_grad[1]) else None
        gb = db.to(ctx.b_dtype) if (ctx.b_dtype is not None and ctx.needs_input_grad[2]) else None
        return gx, gw, gb, None, None


_UNIMPLEMENTED = dict(sigmoid=False, other_act=None, squared_pred=False, jaccard=False, batch=False, weight=None, ce_weight=None,
                      label_smoothing=0.0, soft_label=False)


class _SegLoss(nn.Module):
    def __init__(self, include_background, to_onehot_y, softmax, reduction, smooth_nr, smooth_dr, lambda_dice, lambda_ce, other):
        super().__init__()
        name = type(self).__name__
        for k, v in other.items():
            if k not in _UNIMPLEMENTED:
                raise TypeError(f"{name}: unexpected keyword argument {k!r}")
            if (v is not None) if _UNIMPLEMENTED[k] is None else (v != _UNIMPLEMENTED[k]):
                raise NotImplementedError(f"{name}: {k}={v!r} is not implemented")
        if not to_onehot_y:
            raise NotImplementedError(f"{name}: to_onehot_y=False is not implemented (labels are class indices [B, 1, D, H, W])")
        if not softmax:
            raise NotImplementedError(f"{name}: softmax=False is not implemented")
        if reduction != "mean":
            raise NotImplementedError(f"{name}: reduction={reduction!r} is not implemented (only 'mean')")
        if lambda_dice < 0.0 or lambda_ce < 0.0:
            raise ValueError("lambda_dice and lambda_ce should be no less than 0.0.")
        self.include_background, self.to_onehot_y, self.softmax, self.reduction = include_background, to_onehot_y, softmax, reduction
        self.smooth_nr, self.smooth_dr = float(smooth_nr), float(smooth_dr)
        self.lambda_dice, self.lambda_ce = float(lambda_dice), float(lambda_ce)
        self.last_components = None       # (dice, ce) of the last call, detached tensors on the input's device
        self.last_bad_labels = None       # number of labels outside [0, C) in the last call, a tensor on the input's device

    def _remember(self, total, dice, ce, bad):
        self.last_components, self.last_bad_labels = (dice.detach(), ce.detach()), bad.detach()
        return total

    def _remember_fused(self, loss3, bad):
        comps = loss3.detach()
        return self._remember(loss3[0], comps[1], comps[2], bad.view(()))

    def forward(self, input, target):
        if input.dim() < 3:
            raise ValueError(f"{type(self).__name__}: logits [B, C, spatial...] (got {tuple(input.shape)})")
        if input.is_cuda:
            if target.device != input.device:
                raise ValueError("labels and logits are on different devices")
            return self._remember_fused(*_SegLossFn.apply(input, None, None, target, _Cfg(self)))
        if target.numel() != input.shape[0] * input[0, 0].numel():
            raise ValueError(f"labels {tuple(target.shape)} do not match logits {tuple(input.shape)}")
        return self._remember(*dice_ce_torch(input, target, self.include_background, self.smooth_nr, self.smooth_dr, self.lambda_dice,
                                             self.lambda_ce))


class DiceCELoss(_SegLoss):
    """monai.losses.DiceCELoss for ``softmax=True, to_onehot_y=True`` (train_segmentation.py:105-107), MONAI's keyword names
    and defaults; any option that is not implemented raises NotImplementedError naming it.  ``forward(logits [B, C, D, H, W],
    labels [B, 1, D, H, W])`` returns the 0-dim loss on the logits' device without a host synchronisation."""

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, squared_pred=False,
                 jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, weight=None, lambda_dice=1.0,
                 lambda_ce=1.0, label_smoothing=0.0, ce_weight=None):
        super().__init__(include_background, to_onehot_y, softmax, reduction, smooth_nr, smooth_dr, lambda_dice, lambda_ce,
                         dict(sigmoid=sigmoid, other_act=other_act, squared_pred=squared_pred, jaccard=jaccard, batch=batch, weight=weight,
                              label_smoothing=label_smoothing, ce_weight=ce_weight))


class DiceLoss(_SegLoss):
    """monai.losses.DiceLoss for ``softmax=True, to_onehot_y=True`` (train_segmentation.py:109-111): the Dice term alone."""

    def __init__(self, include_background=True, to_onehot_y=False, sigmoid=False, softmax=False, other_act=None, squared_pred=False,
                 jaccard=False, reduction="mean", smooth_nr=1e-5, smooth_dr=1e-5, batch=False, weight=None, soft_label=False):
        super().__init__(include_background, to_onehot_y, softmax, reduction, smooth_nr, smooth_dr, 1.0, 0.0,
                         dict(sigmoid=sigmoid, other_act=other_act, squared_pred=squared_pred, jaccard=jaccard, batch=batch, weight=weight,
                              soft_label=soft_label))


def _single_conv_head(head):
    """The nn.Conv3d of a head that is STRUCTURALLY one 1x1x1 convolution (stride 1, no padding, one group) inside
    containers whose forward is pure composition, with nothing else but identities; None otherwise."""
    from ..registration.sliding_window import _COMPOSITION_ONLY, _is_affine_leaf

    convs = []

    def structural(m):
        kids = list(m.children())
        if not kids:
            if isinstance(m, nn.Conv3d):
                convs.append(m)
                return _is_affine_leaf(m)
            return isinstance(m, nn.Identity)
        pure = (isinstance(m, nn.Sequential) and type(m).forward is nn.Sequential.forward) or \
               (type(m).__module__, type(m).__name__) in _COMPOSITION_ONLY
        return pure and all(structural(k) for k in kids)

    return convs[0] if (structural(head) and len(convs) == 1) else None


def head_dice_ce(features, head, labels, loss):
    """``loss(head(features), labels)`` without the logits in memory: features [B, F, D, H, W] (what the Unet returns), ``head``
    a 1x1x1-convolution head (``UnetOutBlock``, ``nn.Conv3d(F, C, 1)``), ``loss`` a ``DiceCELoss`` / ``DiceLoss`` of this
    package.  Differentiable with respect to the features, the head's weight and its bias."""
    if not isinstance(loss, _SegLoss):
        raise TypeError(f"head_dice_ce: loss must be a DiceCELoss or DiceLoss of anatomix_amd.segmentation (got {type(loss).__name__})")
    conv = _single_conv_head(head)
    if conv is None:
        raise ValueError("head_dice_ce: the head must be made of exactly one 1x1x1 convolution")
    if not features.is_cuda:
        raise RuntimeError(f"head_dice_ce runs on the GPU (got a {features.device} tensor); on the CPU call loss(head(features), labels)")
    if features.dim() != 5 or features.shape[1] != conv.in_channels:
        raise ValueError(f"head_dice_ce: features [B, {conv.in_channels}, D, H, W] (got {tuple(features.shape)})")
    if conv.weight.device != features.device or labels.device != features.device:
        raise ValueError("head_dice_ce: features, head and labels must be on one device")
    return loss._remember_fused(*_SegLossFn.apply(features, conv.weight, conv.bias, labels, _Cfg(loss)))


def finetune_loss(model, inputs, labels, loss):
    """``loss(model(inputs), labels)`` (train_segmentation.py:144-145).  When ``model`` is ``nn.Sequential(Unet, head)`` or
    ``nn.Sequential(PrimusV2, head)`` with a head made of one 1x1x1 convolution -- decided from the structure alone -- the head and
    the loss run fused (``head_dice_ce``) on the network's dense features (for the ViT those of ``PrimusV2.forward``, whose decoder
    ``train_decoder`` routes); any other model takes the plain composition."""
    if (isinstance(model, nn.Sequential) and type(model).forward is nn.Sequential.forward and len(model) == 2 and
            isinstance(model[0], (Unet, PrimusV2)) and isinstance(loss, _SegLoss) and inputs.is_cuda and _single_conv_head(model[1]) is not None):
        return head_dice_ce(model[0](inputs), model[1], labels, loss)
    return loss(model(inputs), labels)


def predict_labels(features_or_logits, head=None):
    """The post-transform of train_segmentation.py:84-86 (softmax, argmax over the channels; the softmax does not change an
    arg-max) -> uint8 [B, 1, D, H, W], the lowest index on ties.  With ``head`` (one 1x1x1 convolution) the input holds the
    Unet's features and the logits are never written."""
    x = features_or_logits
    if x.dim() < 3:
        raise ValueError(f"predict_labels: [B, C, spatial...] (got {tuple(x.shape)})")
    conv = None
    if head is not None:
        conv = _single_conv_head(head)
        if conv is None or not x.is_cuda:
            with torch.no_grad():
                x, conv = head(x), None
    out_shape = (x.shape[0], 1) + tuple(x.shape[2:])
    if not x.is_cuda:
        return x.detach().argmax(dim=1, keepdim=True).to(torch.uint8)
    C = conv.out_channels if conv is not None else x.shape[1]
    F = x.shape[1] if conv is not None else 0
    if conv is not None and F != conv.in_channels:
        raise ValueError(f"predict_labels: features [B, {conv.in_channels}, ...] (got {tuple(x.shape)})")
    _envelope(C, F if conv is not None else None)
    xc = _lib.f32c(x.detach())
    w = _lib.f32c(conv.weight.detach()).reshape(C, F) if conv is not None else None
    b = _lib.f32c(conv.bias.detach()) if (conv is not None and conv.bias is not None) else None
    out = torch.empty(out_shape, dtype=torch.uint8, device=xc.device)
    with torch.cuda.device(xc.device):
        _lib.check_envelope(_lib.load().amx_seg_argmax(_lib.ptr(xc), F, _lib.ptr(w), _lib.ptr(b), x.shape[0], C, xc[0, 0].numel(),
                            _lib.ptr(out), _lib.stream(xc.device)))
    return out
