"""Segmentation finetuning with the surface of ``anatomix.segmentation`` (reference: segmentation_utils.py,
train_segmentation.py): ``load_model`` and the Dice + cross-entropy loss, the validation Dice loss and the arg-max
post-transform that MONAI provides there, on the HIP kernels of csrc/amx_segloss.hip.  MONAI is not a dependency; its
documented algorithm is restated and parity with an installed MONAI is not pinned."""
from .segmentation_utils import UnetOutBlock, load_model  # noqa: F401
from .losses import DiceCELoss, DiceLoss, finetune_loss, head_dice_ce, predict_labels  # noqa: F401
