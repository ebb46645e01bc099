"""Few-shot segmentation finetuning with the surface of ``anatomix/segmentation/train_segmentation.py``:

    python -m anatomix_amd.segmentation.train_segmentation --dataset DIR --pretrained_ckpt CKPT [...]

The loop is the reference's (:88-257): ``data_handler`` picks and repeats the training pairs, every epoch shuffles them into
batches, each batch goes through the augmentation chain, ``finetune_loss`` (UNet, fused 1x1x1 head, Dice + CE), backward and
Adam with cosine annealing; every ``val_interval`` epochs the validation volumes run through the sliding window into the Dice
loss and the checkpoints are written.  What differs from the reference:
  * the unique training volumes are loaded once (``anatomix_amd.io.nifti``), rescaled and kept on the device, and the augmentation
    is ``augment.augment_batch`` on the device instead of MONAI transforms in CPU workers.  One ``numpy.random.RandomState(seed)``
    drives the epoch shuffles and ``augment.draw_params`` in a fixed order (per epoch: the permutation, then per batch its
    parameters), so a run is reproducible from ``--seed``; MONAI's own random streams are not reproduced;
  * the optimizer is ``FusedAdamW(weight_decay=0)``, whose update then is ``torch.optim.Adam``'s;
  * TensorBoard and the image plots are not reproduced: the scalars go to ``<out_dir>/runs/<exp_name>/log.jsonl`` and to the
    reference's print lines (plus one line with the epoch's learning rate);
  * ``--seed``, ``--out_dir`` (the reference always writes under ``finetuning_runs``) and ``--no_augment`` (every random transform
    off: the batch is the random crop, resampled to the crop size by the identity and rescaled)."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from ..io.nifti import load_nifti
from ..pretraining.optim import FusedAdamW
from ..registration.sliding_window import sliding_window_inference
from . import augment
from .losses import DiceCELoss, DiceLoss, finetune_loss
from .segmentation_utils import data_handler, get_val_transforms, load_model, save_ckp


def build_parser():
    """The reference's flags in its order (:263-353), then ``--seed``, ``--out_dir`` and ``--no_augment``."""
    parser = argparse.ArgumentParser(description='')
    parser.add_argument('--dataset', type=str, default='./dataset/', help="Directory where image and label *.nii.gz files are stored.")
    parser.add_argument('--n_epochs', type=int, default=500,
                        help="Number of epochs. An epoch is defined as n_iters_per_epoch training batches")
    parser.add_argument('--n_iters_per_epoch', type=int, default=75, help="Number of training batches per epoch")
    parser.add_argument('--n_classes', type=int, default=4, help="Number of classes to segment. Does not include background class")
    parser.add_argument('--val_interval', type=int, default=2, help="Do a valid. and checkpointing loop every val_interval epochs")
    parser.add_argument('--lr', type=float, default=2e-4, help="Adam step size")
    parser.add_argument('--crop_size', type=int, default=128, help="Crop size to train on")
    parser.add_argument('--batch_size', type=int, default=4, help="Batch size to train with")
    parser.add_argument('--train_amount', type=int, default=3, help="No. of training samples to use for few-shot training")
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--pretrained_ckpt', type=str, default=None,
                     help="Path to a local .pth checkpoint, or 'scratch' for random initialization.")
    src.add_argument('--hf_variant', type=str, default=None,
                     help="HuggingFace Hub variant to download from neeldey/anatomix (e.g. 'anatomix', 'anatomix-dev').")
    only = "Only used with --pretrained_ckpt."
    parser.add_argument('--num_downs', type=int, default=4, help=f"Number of downsampling layers in the U-Net. Default 4. {only}")
    parser.add_argument('--ngf', type=int, default=16, help=f"Channel multiplier for the U-Net. Default 16. {only}")
    parser.add_argument('--output_nc', type=int, default=16, help=f"Number of output feature channels of the U-Net. Default 16. {only}")
    parser.add_argument('--norm', type=str, default='batch', help=f"Normalization type ('batch', 'instance', 'none'). Default 'batch'. {only}")
    parser.add_argument('--interp', type=str, default='nearest',
                        help=f"Decoder upsampling mode ('nearest' or 'trilinear'). Default 'nearest'. {only}")
    parser.add_argument('--pooling', type=str, default='Max', help=f"Pooling type ('Max' or 'Avg'). Default 'Max'. {only}")
    parser.add_argument('--exp_name', type=str, default='demo', help="Prefix to attach to training logs in folder and file names")
    parser.add_argument('--seed', type=int, default=0, help="Seed of the head's initialisation, the epoch shuffles and the augmentation")
    parser.add_argument('--out_dir', type=str, default='finetuning_runs', help="Directory that receives checkpoints/ and runs/")
    parser.add_argument('--no_augment', action='store_true', help="Switch every random transform off (crop and rescale only)")
    return parser


def _load_pair(image_path, label_path, device):
    """One image / label pair resident on the device: (float32 [D, H, W] rescaled to [0, 1], uint8 [D, H, W])."""
    img = augment.make_resident(load_nifti(image_path)[0], device)
    lab = torch.from_numpy(np.ascontiguousarray(load_nifti(label_path)[0]).astype(np.uint8)).to(device)
    if lab.shape != img.shape:
        raise ValueError(f"{label_path}: label shape {tuple(lab.shape)} does not match the image's {tuple(img.shape)}")
    return img, lab


def _probe_unet(unet, batch, crop, device):
    """The UNet's own refusal of a shape it cannot train on, raised before anything is loaded or stepped."""
    from ..model import train as unet_train
    reason = unet_train.unsupported_reason(unet, torch.empty((batch, 1, crop, crop, crop), device=device), [])
    if reason is not None:
        raise RuntimeError("anatomix_amd.Unet: this call cannot run on the HIP kernels (" + reason + ").")


def finetune(dataset='./dataset/', n_epochs=500, n_iters_per_epoch=75, n_classes=4, val_interval=2, lr=2e-4, crop_size=128, batch_size=4,
             train_amount=3, pretrained_ckpt=None, hf_variant=None, num_downs=4, ngf=16, output_nc=16, norm='batch', interp='nearest',
             pooling='Max', exp_name='demo', seed=0, out_dir='finetuning_runs', no_augment=False, on_batch=None, device=None):
    """The reference's ``main(opt)`` with its options as keyword arguments.  ``on_batch(epoch, step, inputs, labels, params)`` is
    called with every training batch (1-based epoch and step, the augmented tensors, and ``draw_params``' dict with the batch's
    image paths added under ``files``) before its forward.  Returns a dict: ``step_losses`` (every step), ``epoch_losses``
    (per-epoch means), ``val_losses`` ((epoch, value) pairs), ``learning_rates`` (per epoch) and ``paths`` (``checkpoints``,
    ``best``, ``log``)."""
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise RuntimeError("finetune runs on the GPU: there is no host path")
    ckpt_dir = os.path.join(out_dir, "checkpoints", exp_name)
    run_dir = os.path.join(out_dir, "runs", exp_name)
    os.makedirs(ckpt_dir, exist_ok=True)
    os.makedirs(run_dir, exist_ok=True)

    trimages, trsegs, vaimages, vasegs = data_handler(dataset, train_amount, n_iters_per_epoch, batch_size)
    print('Training cache: {} images {} segs'.format(len(trimages), len(trsegs)))
    print('Validation set: {} images {} segs'.format(len(vaimages), len(vasegs)))

    torch.manual_seed(seed)
    model = load_model(n_classes, device, ckpt_path=pretrained_ckpt, hf_variant=hf_variant, num_downs=num_downs, ngf=ngf,
                       output_nc=output_nc, norm=norm, interp=interp, pooling=pooling)
    _probe_unet(model[0], batch_size, crop_size, device)

    resident = {}
    for ip, lp in zip(trimages, trsegs):
        if ip not in resident:
            resident[ip] = _load_pair(ip, lp, device)
    rescale = get_val_transforms()
    val_set = []
    for ip, lp in zip(vaimages, vasegs):
        img = torch.from_numpy(np.ascontiguousarray(load_nifti(ip)[0], dtype=np.float32)).to(device)
        lab = torch.from_numpy(np.ascontiguousarray(load_nifti(lp)[0]).astype(np.uint8)).to(device)
        val_set.append((rescale(img[None, None]), lab[None, None]))

    loss_function = DiceCELoss(softmax=True, to_onehot_y=True, include_background=False)
    valloss_function = DiceLoss(softmax=True, to_onehot_y=True, include_background=False)
    optimizer = FusedAdamW(model.parameters(), lr, weight_decay=0)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=n_epochs)

    rng = np.random.RandomState(seed)
    log_path = os.path.join(run_dir, "log.jsonl")
    out = dict(step_losses=[], epoch_losses=[], val_losses=[], learning_rates=[], paths=dict(checkpoints=[], best=[], log=log_path))
    best_val_loss, best_loss_epoch = 10000000000, None
    epoch_len = len(trimages) // batch_size
    with open(log_path, "w") as log:
        def record(**kw):
            log.write(json.dumps(kw) + "\n")
            log.flush()

        for epoch in range(n_epochs):
            cur_lr = float(optimizer.param_groups[0]["lr"])
            out["learning_rates"].append(cur_lr)
            print("-" * 10)
            print("epoch {:04d}/{:04d}".format(epoch + 1, n_epochs))
            print(f"learning rate: {cur_lr:.8e}")
            model.train()
            epoch_loss, step = 0, 0
            order = rng.permutation(len(trimages))
            for start in range(0, len(order), batch_size):
                step += 1
                names = [trimages[i] for i in order[start:start + batch_size]]
                vols, labs = [resident[n][0] for n in names], [resident[n][1] for n in names]
                params = augment.draw_params(rng, crop_size, [tuple(v.shape) for v in vols], len(vols))
                params["files"] = names
                if no_augment:
                    for k in params["on"]:
                        params["on"][k][:] = False
                    params["affine"][:] = np.eye(3)
                inputs, labels = augment.augment_batch(vols, labs, params)
                if on_batch is not None:
                    on_batch(epoch + 1, step, inputs, labels, params)
                optimizer.zero_grad()
                loss = finetune_loss(model, inputs, labels, loss_function)
                loss.backward()
                optimizer.step()
                value = loss.item()
                epoch_loss += value
                out["step_losses"].append(value)
                print(f"{step}/{epoch_len}, train_loss: {value:.4f}")
                record(kind="train", epoch=epoch + 1, step=step, global_step=epoch_len * epoch + step, train_loss=value, lr=cur_lr)
            epoch_loss /= step
            out["epoch_losses"].append(epoch_loss)
            scheduler.step()
            print(f"epoch {epoch + 1} average loss: {epoch_loss:.4f}")

            if (epoch + 1) % val_interval != 0:
                continue
            model.eval()
            with torch.no_grad():
                val_loss, valstep = 0.0, 0
                for val_images, val_labels in val_set:
                    val_outputs = sliding_window_inference(val_images, (crop_size,) * 3, 4, model, overlap=0.7)
                    val_loss = val_loss + valloss_function(val_outputs, val_labels)
                    valstep += 1
                if valstep:
                    val_loss = float(val_loss / valstep)
                    if val_loss < best_val_loss:
                        best_val_loss, best_loss_epoch = val_loss, epoch + 1
                        path = os.path.join(ckpt_dir, "best_dict_epoch{:04d}.pth".format(epoch + 1))
                        torch.save(model.state_dict(), path)
                        out["paths"]["best"].append(path)
                        print("saved new best loss model")
                    print("current epoch: {} current mean dice: {:.4f} best mean dice: {:.4f} at epoch {}".format(
                        epoch + 1, val_loss, best_val_loss, best_loss_epoch))
                    out["val_losses"].append((epoch + 1, val_loss))
                    record(kind="val", epoch=epoch + 1, val_loss_mean_dice=val_loss)
            path = os.path.join(ckpt_dir, "epoch{:04d}.pth".format(epoch + 1))
            save_ckp({"state_dict": model.state_dict(), "optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict()}, path)
            out["paths"]["checkpoints"].append(path)
    return out


def main(argv=None, on_batch=None):
    opt = build_parser().parse_args(argv)
    return finetune(**vars(opt), on_batch=on_batch)


if __name__ == "__main__":
    main()
