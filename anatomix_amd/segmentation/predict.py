"""Label maps from a finetuned segmentation checkpoint:

    python -m anatomix_amd.segmentation.predict --images A.nii.gz B.nii.gz --ckpt best.pth --n_classes 4 --out_dir OUT [...]

The reference has no such script: ``anatomix/segmentation/train_segmentation.py`` stops at the validation loss (:194-200), and a
user assembles the inference by hand from MONAI's ``sliding_window_inference``, the ``AsDiscrete(argmax=True)`` post-transform
(:84-86) and nibabel.  This module is that assembly.  The flags that describe the model (``--n_classes``, ``--num_downs``,
``--ngf``, ``--output_nc``, ``--norm``, ``--interp``, ``--pooling``) are ``train_segmentation``'s, ``--roi`` is its ``--crop_size``
and the default overlap 0.7 its validation call's; ``--ckpt`` takes what that script writes (``best_dict_epoch*.pth``: the
state dict of ``nn.Sequential(Unet, head)``, or ``epoch*.pth`` with it under ``state_dict``).

``segment_volume`` is one ``amx_sliding_window`` call (``amx_vit_sliding_window`` for a finetuned ViT) (``registration.sliding_window.sliding_window_volume(out="labels")``): the
windows, their average, the 1x1x1 head and the arg-max run behind the C ABI and neither the features nor the logits of the volume
are read back.  There is no host path."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch
import torch.nn as nn

from ..io.nifti import load_nifti, save_nifti
from ..registration.metrics import dice_score
from ..registration.sliding_window import sliding_window_volume
from ..model.network import Unet
from .segmentation_utils import UnetOutBlock, get_val_transforms


def segment_volume(model, image, roi=128, overlap=0.7, mode="constant"):
    """uint8 [D, H, W] labels of ``image`` (a [D, H, W] device tensor, any real dtype): ``model`` is ``nn.Sequential(Unet, head)``
    as ``load_model`` returns it, or ``nn.Sequential(PrimusV2, head)`` with ``roi`` the ViT's input shape, the image is rescaled by ``get_val_transforms()`` and the windows are
    ``sliding_window_inference(image, roi, 4, model, overlap)``'s (train_segmentation.py:194-199), then softmax + arg-max (:84-86;
    the lowest class on ties)."""
    if not (isinstance(model, nn.Sequential) and len(model) == 2):
        raise TypeError("segment_volume: model must be nn.Sequential(Unet or PrimusV2, head) as load_model returns it")
    if not torch.is_tensor(image) or image.dim() != 3:
        raise ValueError(f"segment_volume: image [D, H, W] (got {tuple(getattr(image, 'shape', ()))})")
    if not image.is_cuda:
        raise RuntimeError(f"segment_volume runs on the GPU: there is no host path (got a {image.device} tensor)")
    x = get_val_transforms()(image.detach().float()[None, None])
    with torch.no_grad():
        return sliding_window_volume(x, roi, model[0], overlap=overlap, mode=mode, head=model[1], out="labels")[0, 0]


def build_parser():
    """``--images`` / ``--ckpt`` / ``--out_dir``, the model flags of ``train_segmentation`` with its defaults, then the inference's."""
    parser = argparse.ArgumentParser(description="Segment NIfTI volumes with a finetuned anatomix checkpoint")
    parser.add_argument('--images', type=str, nargs='+', required=True, help="Image *.nii.gz files to segment")
    parser.add_argument('--ckpt', type=str, required=True,
                        help="Finetuned checkpoint of train_segmentation (state dict of Sequential(Unet, head), bare or under 'state_dict')")
    parser.add_argument('--n_classes', type=int, default=4, help="Number of classes to segment. Does not include background class")
    parser.add_argument('--num_downs', type=int, default=4, help="Number of downsampling layers in the U-Net. Default 4.")
    parser.add_argument('--ngf', type=int, default=16, help="Channel multiplier for the U-Net. Default 16.")
    parser.add_argument('--output_nc', type=int, default=16, help="Number of output feature channels of the U-Net. Default 16.")
    parser.add_argument('--norm', type=str, default='batch', help="Normalization type ('batch', 'instance', 'none'). Default 'batch'.")
    parser.add_argument('--interp', type=str, default='nearest', help="Decoder upsampling mode ('nearest' or 'trilinear'). Default 'nearest'.")
    parser.add_argument('--pooling', type=str, default='Max', help="Pooling type ('Max' or 'Avg'). Default 'Max'.")
    parser.add_argument('--out_dir', type=str, default='segmentations', help="Directory that receives <name>_seg.nii.gz (and dice.json)")
    parser.add_argument('--labels', type=str, nargs='+', default=None, help="Label *.nii.gz files, one per image: report the Dice against them")
    parser.add_argument('--roi', type=int, default=128, help="Sliding-window size (the crop size the model was finetuned on)")
    parser.add_argument('--overlap', type=float, default=0.7, help="Sliding-window overlap")
    parser.add_argument('--device', type=str, default='cuda', help="Device to run on (a GPU: there is no host path)")
    return parser


def _load_finetuned(opt, device):
    """``Sequential(Unet, head)`` of the architecture flags with the checkpoint's weights, in eval mode."""
    if not os.path.isfile(opt.ckpt):
        raise FileNotFoundError(f"Checkpoint file not found: {opt.ckpt}")
    model = nn.Sequential(Unet(3, 1, opt.output_nc, opt.num_downs, ngf=opt.ngf, norm=opt.norm, interp=opt.interp, pooling=opt.pooling),
                          UnetOutBlock(3, opt.output_nc, opt.n_classes + 1))      # load_model's composition (segmentation_utils.py:113-115)
    state = torch.load(opt.ckpt, map_location="cpu")
    if isinstance(state, dict) and "state_dict" in state:
        state = state["state_dict"]
    model.load_state_dict(state, strict=True)
    return model.to(device).eval()


def _stem(path):
    name = os.path.basename(path)
    for ext in (".nii.gz", ".nii"):
        if name.endswith(ext):
            return name[:-len(ext)]
    return os.path.splitext(name)[0]


def predict(opt):
    """Writes ``<out_dir>/<name>_seg.nii.gz`` (uint8, the image's affine) per image; with ``--labels`` also prints the Dice per class
    and writes ``<out_dir>/dice.json`` = {name: {"mean": macro Dice, "per_class": {label: Dice}}} (``registration.metrics.dice_score``:
    the classes that occur in the label file, background dropped).  Returns {"paths": [...], "dice": {...} or None}."""
    device = torch.device(opt.device)
    if device.type != "cuda":
        raise RuntimeError("predict runs on the GPU: there is no host path")
    if opt.labels is not None and len(opt.labels) != len(opt.images):
        raise ValueError(f"--labels: {len(opt.labels)} files for {len(opt.images)} images")
    os.makedirs(opt.out_dir, exist_ok=True)
    model = _load_finetuned(opt, device)
    paths, dice = [], ({} if opt.labels is not None else None)
    for k, path in enumerate(opt.images):
        data, affine, _ = load_nifti(path)
        image = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(device)
        seg = segment_volume(model, image, roi=opt.roi, overlap=opt.overlap)
        out_path = os.path.join(opt.out_dir, _stem(path) + "_seg.nii.gz")
        save_nifti(out_path, seg.cpu().numpy(), affine, dtype=np.uint8)
        paths.append(out_path)
        print(f"{path} -> {out_path}")
        if dice is not None:
            lab = torch.from_numpy(np.ascontiguousarray(load_nifti(opt.labels[k])[0]).astype(np.uint8)).to(device)
            if lab.shape != seg.shape:
                raise ValueError(f"{opt.labels[k]}: label shape {tuple(lab.shape)} does not match the image's {tuple(seg.shape)}")
            mean, per = dice_score(lab, seg)
            dice[_stem(path)] = {"mean": mean, "per_class": {str(l): v for l, v in per.items()}}
            print("  dice: mean {:.4f}  ".format(mean) + "  ".join(f"class {l}: {v:.4f}" for l, v in per.items()))
    if dice is not None:
        with open(os.path.join(opt.out_dir, "dice.json"), "w") as f:
            json.dump(dice, f, indent=1)
    return {"paths": paths, "dice": dice}


def main(argv=None):
    return predict(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
