"""``load_model`` (reference :36-116), ``data_handler`` (:235-305), ``get_val_transforms`` (:219-228) and ``save_ckp`` with the
surface of ``anatomix.segmentation.segmentation_utils``.  The training transforms (:159-216) are ``augment.augment_batch``."""
from __future__ import annotations

import os
import re
from collections import OrderedDict
from glob import glob

import numpy as np

import torch
import torch.nn as nn

from ..model.load_from_hf import ANATOMIX_VARIANTS, _load_handling_compile, load_from_hf
from ..model.network import Unet


class UnetOutBlock(nn.Sequential):
    """monai.networks.blocks.UnetOutBlock(spatial_dims, in_channels, out_channels) restated: one 1x1x1 convolution with a
    bias, under the parameter names MONAI gives it (``conv.conv.weight``, ``conv.conv.bias``), so that a finetuning
    checkpoint of the reference loads.  Pure composition (no forward of its own): the sliding-window inference and
    ``finetune_loss`` recognise it as a per-voxel affine head."""

    def __init__(self, spatial_dims, in_channels, out_channels, dropout=None):
        if spatial_dims != 3:
            raise NotImplementedError(f"UnetOutBlock: spatial_dims = 3 (got {spatial_dims})")
        if dropout:
            raise NotImplementedError("UnetOutBlock: dropout is not implemented")
        super().__init__(OrderedDict(conv=nn.Sequential(OrderedDict(conv=nn.Conv3d(in_channels, out_channels, kernel_size=1)))))


def load_model(n_classes, device, *, ckpt_path=None, hf_variant=None, num_downs=4, ngf=16, output_nc=16, norm="batch",
               interp="nearest", pooling="Max"):
    """segmentation_utils.py:36-116.  Exactly one of ``ckpt_path`` / ``hf_variant``; ``ckpt_path='scratch'`` is a random
    initialisation; the architecture arguments are keyword-only and only used with ``ckpt_path`` (a variant brings its own).
    Returns ``nn.Sequential(Unet, UnetOutBlock(3, feat, n_classes + 1))`` on ``device``."""
    if (ckpt_path is None) == (hf_variant is None):
        raise ValueError("Provide exactly one of `ckpt_path` or `hf_variant`.")
    if hf_variant is not None:
        print(f"Transferring from HuggingFace variant '{hf_variant}'.")
        model = load_from_hf(hf_variant).to(device)
        feat_channels = ANATOMIX_VARIANTS[hf_variant]["output_channels"]
    elif ckpt_path == "scratch":
        print("Training from random initialization.")
        model = Unet(3, 1, output_nc, num_downs, ngf=ngf, norm=norm, interp=interp, pooling=pooling).to(device)
        feat_channels = output_nc
    else:
        if not os.path.isfile(ckpt_path):
            raise FileNotFoundError(f"Checkpoint file not found: {ckpt_path}")
        print("Transferring from local checkpoint.")
        model = Unet(3, 1, output_nc, num_downs, ngf=ngf, norm=norm, interp=interp, pooling=pooling).to(device)
        model = _load_handling_compile(model, torch.load(ckpt_path, map_location="cpu")).to(device)
        feat_channels = output_nc
    fin_layer = UnetOutBlock(3, feat_channels, n_classes + 1).to(device)
    return nn.Sequential(model, fin_layer).to(device)


def save_ckp(state, checkpoint_dir):
    """segmentation_utils.py:122-133: ``torch.save`` of a checkpoint dict to the given file."""
    torch.save(state, checkpoint_dir)


def natural_key(text):
    """Sort key of the natural order: runs of digits compare as integers, everything else as text (a number sorts before text
    at the same position).  The reference calls ``natsort.natsorted``; natsort is not a dependency and parity with it is NOT
    pinned (it differs, for one, on signs, decimal points and locale-aware text)."""
    return [(0, int(tok), "") if tok.isdigit() else (1, 0, tok) for tok in re.split(r"(\d+)", str(text)) if tok != ""]


def natural_sorted(items):
    return sorted(items, key=natural_key)


def data_handler(basedir, finetuning_amount=3, iters_per_epoch=75, batch_size=3, seed=12345):
    """segmentation_utils.py:235-305.  ``basedir`` holds imagesTr, labelsTr, imagesVal and labelsVal with *.nii.gz files.  The two
    natural-sorted training lists are permuted by ``RandomState(seed).permutation`` (the same permutation for both), cut to
    ``finetuning_amount`` and repeated ``max(1, iters_per_epoch * batch_size // finetuning_amount)`` times; the validation lists are
    natural-sorted.  Returns (training images, training segmentations, validation images, validation segmentations)."""
    trimages = natural_sorted(glob(os.path.join(basedir, "./imagesTr/*.nii.gz")))
    trsegs = natural_sorted(glob(os.path.join(basedir, "./labelsTr/*.nii.gz")))
    assert len(trimages) > 0
    assert len(trimages) == len(trsegs)
    trimages = np.random.RandomState(seed=seed).permutation(trimages).tolist()[:finetuning_amount]
    trsegs = np.random.RandomState(seed=seed).permutation(trsegs).tolist()[:finetuning_amount]
    repeats = max(1, iters_per_epoch * batch_size // finetuning_amount)
    vaimages = natural_sorted(glob(os.path.join(basedir, "./imagesVal/*.nii.gz")))
    vasegs = natural_sorted(glob(os.path.join(basedir, "./labelsVal/*.nii.gz")))
    return trimages * repeats, trsegs * repeats, vaimages, vasegs


def get_val_transforms():
    """segmentation_utils.py:219-228 after loading: the ScaleIntensity of the whole image alone.  Returns a callable that maps a
    float32 device image [B, 1, D, H, W] to its rescaled copy (``augment.scale_intensity``)."""
    from .augment import scale_intensity
    return scale_intensity
