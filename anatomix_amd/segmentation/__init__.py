"""Segmentation finetuning with the surface of ``anatomix.segmentation`` (reference: segmentation_utils.py,
train_segmentation.py): ``load_model`` and the Dice + cross-entropy loss, the validation Dice loss and the arg-max
post-transform that MONAI provides there, on the HIP kernels of csrc/amx_segloss.hip; the training transforms on the device
(``augment``, csrc/amx_segaug.hip) and the finetuning loop (``python -m anatomix_amd.segmentation.train_segmentation``).  MONAI is
not a dependency; its documented algorithms are restated (DESIGN.md sections 4.14, 4.15) and parity with an installed MONAI is not
pinned."""
from .segmentation_utils import UnetOutBlock, data_handler, get_val_transforms, load_model, save_ckp  # noqa: F401
from .augment import (adjust_contrast, affine_resample, augment_batch, bias_field, draw_params, gaussian_noise, gaussian_sharpen,  # noqa: F401
                      gaussian_smooth, gibbs_noise, scale_intensity)
from .losses import DiceCELoss, DiceLoss, finetune_loss, head_dice_ce, predict_labels  # noqa: F401
