"""``load_model`` with the surface of ``anatomix.segmentation.segmentation_utils`` (reference :36-116)."""
from __future__ import annotations

import os
from collections import OrderedDict

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
