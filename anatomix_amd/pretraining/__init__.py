"""MI355X-side mirror of the reference's contrastive-pretraining pieces (reference: pretraining/models/).

  SupPatchNCELoss ... pretraining/models/supcl_model.py:16-226     (HIP forward+backward kernel, amx_supcon_loss)
  PatchSampleF ...... pretraining/models/pretraining_networks.py:264-519  (projection heads: HIP forward + backward,
                      amx_mlp_head_forward / _backward)
  contrastive_step .. the per-batch body of SupCLModel.optimize_parameters / forward / calculate_NCE_loss
                      (supcl_model.py:603-661, 723-843) without the option parsing / logging around it.
  FusedAdamW ........ torch.optim.AdamW as built at supcl_model.py:510-516, 584-590: one HIP launch per optimizer (amx_adamw_step)
  grad_norms ........ clip_grad_norm_ of supcl_model.py:631-655 without its pass over the gradients: the norms of both networks in one
                      call (amx_grad_norms), the clip inside the optimizer launch of FusedAdamW(max_norm=...) (amx_adamw_step_clip_dev)
  pretrain_anatomix . the launcher and training loop (scripts/pretrain_anatomix.py, trainers/train.py) over the step, with
                      schedulers.py (get_scheduler) and checkpoints.py (base_model.py:245-466); step.validation_loss for its evaluation
  augment ........... the TorchIO branch of H5SupCLDataset (pretraining/data/h5supcl_dataset.py:122-178, 260-303) on the device:
                      flip + affine, blur, noise, bias field, gamma, motion (HIP kernels of csrc/amx_preaug.hip; torch.fft for motion)
  AugmentedTwoViewLoader  the loader that feeds the step: H5SupCLDataset + augment_pair + the crop, collated device batches
The UNet inside the step runs forward and backward on the HIP kernels (anatomix_amd.model.train).
"""
from .supcon import SupPatchNCELoss
from .patch_sample import PatchSampleF
from .step import contrastive_step, GraphedContrastiveStep, StepRecord
from .data_parallel import GradientBuckets
from .optim import FusedAdamW, grad_norms
from .data import H5SupCLDataset, random_crop
from . import augment, loader
from .augment import augment_pair, draw_params
from .loader import AugmentedTwoViewLoader

__all__ = ["SupPatchNCELoss", "PatchSampleF", "contrastive_step", "GraphedContrastiveStep", "StepRecord", "GradientBuckets", "FusedAdamW", "grad_norms", "H5SupCLDataset", "random_crop",
           "augment", "loader", "augment_pair", "draw_params", "AugmentedTwoViewLoader"]
