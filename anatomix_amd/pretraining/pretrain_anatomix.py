"""Contrastive pretraining end to end: the reference's launcher and training loop (pretraining/scripts/pretrain_anatomix.py,
pretraining/trainers/train.py, the SupCLModel / BaseModel methods it drives) over this package's HIP step.

    python -m anatomix_amd.pretraining.pretrain_anatomix --dataroot <dir with train_data.hdf5 / val_data.hdf5> --name demo

What is the reference's: the launcher's flags (``build_parser``: its flags first, in its order, with its defaults), the trainer
options the launcher does not pass (``TRAINER_DEFAULTS``: the defaults of BaseOptions / TrainOptions / SupCLModel), the seeds, the
``total_iters`` bookkeeping (``total_iters += batch_size``; an optimizer step when ``total_iters % grad_accum_iters == 0``), the
evaluation every ``evaluation_freq`` with its ``>`` comparison on ``n_val_during_train``, ``best_val``, the files of
``checkpoints.py``, ``--continue_train`` (the train state is peeked for ``total_iters``, the numbered networks are loaded, then the
optimizers and schedulers are restored; no iteration is replayed), the schedulers of ``schedulers.py`` stepped at the end of every
epoch (``plateau``: after every evaluation), ``save_latest_freq`` / ``save_freq`` / ``max_iters`` / ``stop_epoch``.

What differs, on purpose:
  * The step is ``contrastive_step`` -- or, with ``--graph auto``, ``grad_accum_iters == 1`` and a batch of the captured shape,
    its HIP-graph replay ``GraphedContrastiveStep``; any other batch (the trailing incomplete one) runs eagerly.  The warm-up steps
    a capture needs are undone (weights, BatchNorm statistics and optimizer state are put back), so N batches are N steps.
  * Gradient clipping (``--clip_grad``) is ``FusedAdamW(max_norm=...)``: one launch pair for both norms, the clip inside the
    optimizer launch; the logged norms are those before clipping, as in the reference.
  * The loss scaler is OFF and ``"scaler": None`` goes into the train state: the step's precision (``--precision``, bf16 storage
    with fp32 accumulation by default) is this package's own and not autocast, there is nothing to scale.
  * ``data_dependent_initialize`` builds the heads from one forward + backward of the first batch as the reference does, but its
    gradients are dropped; the reference leaves them to be added to the first step's.
  * TensorBoard, the visuals and the NIfTI dumps are replaced by ``log.jsonl`` (the mechanism of ``train_segmentation``): one JSON
    object per line, kinds ``train`` (total_iters, epoch, loss, per_layer, lr, grad_norm_G, grad_norm_F; every ``print_freq``)
    and ``val`` (total_iters, epoch, loss, best, n).  The ``display_*`` flags are accepted and ignored.
  * ``--netG primus --primus_version v2`` trains ``PrimusV2`` (built as the reference's ``define_G`` builds it,
    pretraining_networks.py:107-148) with single-scale NCE on the decoded volume (``nce_layers = [-1]``, supcl_model.py:403-410): eager
    steps, the decoder on the sampled rows only (``PrimusV2.forward_train_sampled``), ``--primus_train_route {hip,torch}`` (default
    ``hip``) for the attention cores and the blocks' linears, ``--primus_train_tokenizer {torch,hip}`` (default ``torch``) for the
    conv tokenizer's stem and stages, ``--primus_train_norm {torch,hip}`` (default ``torch``) for the blocks' token LayerNorms, the
    SwiGLU gate product and the final norm and ``--primus_train_decoder {torch,hip}`` (default ``torch``) for the dense decoder and a
    spatial output norm (``--primus_out_norm demean`` / ``instance``, which the rows route does not take) -- the command line's four
    further flags.  What is not on those kernels (LayerScale, the
    tokenizer's ``proj``, the heads) is fp32 torch autograd, and ``--precision`` (the UNet's storage precision) has no effect on it: the reference's bf16 autocast + GradScaler around the Primus step (supcl_model.py:565-574) is not
    reproduced.  ``netG.txt`` is written as the reference writes it.  Validation volumes have the network's input shape; a crop whose
    token grid the engine forward does not take (not a multiple of 64 tokens, e.g. ``--crop_size 48``) is validated on the torch modules.
  * Refused with the reason: ``--netG primus`` with ``--primus_version v1`` (the default; there is no Primus v1 here), a patch size
    other than 8, a ``crop_size`` that is no multiple of 8, a non-zero ``--primus_drop_path_rate`` or ``--graph on``; ``--ndims 2``,
    ``--gpu_ids -1`` (there is no host path), ``--pretrained_name`` together with ``--continue_train`` (the reference calls them
    mutually exclusive and then silently prefers one)."""
import argparse
import contextlib
import copy
import io
import json
import math
import os
import random
import time
from argparse import Namespace

import numpy as np
import torch

from . import checkpoints as ckpt
from .schedulers import get_scheduler, update_learning_rate

EXTRA_FLAGS = ("precision", "graph", "loader_seed", "out_log")
PRIMUS_TRAIN_ROUTES = ("hip", "torch")

# what the trainer's own parser would give for the options the launcher does not pass (tests/golden/pretrain_cli.json)
TRAINER_DEFAULTS = dict(
    easy_label="experiment_name", skip_connection=False, actG="relu", actF="relu", init_gain=0.02, no_dropout=True,
    validation_prefix="image_seg_3d", data_ndims=3, view_order=False, load_mask=False, normalize=True, augment=True, geo_augment=True,
    inten_augment=True, blur=True, noise=True, bias=True, gamma=True, motion=True, resize=False, epoch="latest", verbose=False, suffix="",
    display_id=None, save_by_iter=False, epoch_count=0, phase="train", stop_epoch=99999999, partial_train="1", beta1=0.9, beta2=0.999,
    eps=1e-8, pool_size=0, lr_decay_iters=50, unfreeze_layers="", last_id=65, use_mlp=True)


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ("yes", "true", "t", "y", "1"):
        return True
    if v.lower() in ("no", "false", "f", "n", "0"):
        return False
    raise argparse.ArgumentTypeError("Boolean value expected.")


def primus_out_norm_mode(v):
    s = str(v).strip().lower()
    names = {"instance": ("instance", "instancenorm", "in", "true", "t", "yes", "y", "1"), "demean": ("demean", "center"),
             "layernorm": ("layernorm", "layer", "ln"), "layernorm_affine": ("layernorm_affine", "layernorm-affine", "ln_affine"),
             "none": ("none", "identity", "off", "false", "f", "no", "n", "0")}
    for mode, spellings in names.items():
        if s in spellings:
            return mode
    raise argparse.ArgumentTypeError("expected one of none|instance|demean|layernorm|layernorm_affine (or a bool); got %r" % v)


def build_parser(primus_route=False):
    """The launcher's flags in its order (scripts/pretrain_anatomix.py with options/primus_options.py), then ``--precision``,
    ``--graph``, ``--loader_seed`` and ``--out_log``; ``primus_route=True`` (the command line, ``main``) adds
    ``--primus_train_route``, ``--primus_train_tokenizer``, ``--primus_train_norm`` and ``--primus_train_decoder`` behind them."""
    parser = argparse.ArgumentParser(description="Pretrain anatomix with configurable arguments.")
    add = parser.add_argument
    add("--ckpt_dir", type=str, default="../checkpoints/pretrain/", help="models are saved here")
    add("--dataroot", type=str, default="../../synthetic-data-generation/h5_w_segs/", help="path to images")
    add("--name", type=str, default="demo", help="name of the run you're launching")
    add("--n_epochs", type=int, default=0, help="number of epochs with the initial learning rate")
    add("--n_epochs_decay", type=int, default=4, help="number of epochs to start linearly decaying learning rate to zero")
    add("--crop_size", type=int, default=128, help="crop size")
    add("--batch_size", type=int, default=1, help="input batch size in terms of number of contrastive paired volumes")
    add("--dataset_mode", type=str, default="h5supcl", help="chooses datasets")
    add("--model", type=str, default="supcl", help="chooses which model to use. only `supcl` supported as of now")
    add("--nce_T", type=float, default=0.33, help="NCE temperature")
    add("--ndims", type=int, default=3, help="network dimension: 2|3. only 3 supported as of now.")
    add("--input_nc", type=int, default=1, help="number of input image channels")
    add("--output_nc", type=int, default=16, help="number of network output feature channels")
    add("--ngf", type=int, default=16, help="number of filters in the first conv layer")
    add("--num_downs", type=int, default=4, help="number of downsamples in encoder")
    add("--netF", type=str, default="mlp_sample", help="specify the feature network type. we use a patch sampling MLP")
    add("--n_mlps", type=int, default=3, help="number of MLP layers in netF")
    add("--num_threads", type=int, default=0, help="number of threads for loading data")
    add("--lr", type=float, default=2e-4, help="initial learning rate for adam")
    add("--weight_decay", type=float, default=1e-5, help="weight decay for adamw")
    add("--print_freq", type=int, default=100, help="frequency of showing training results on console")
    add("--display_ncols", type=int, default=2,
        help="if positive, display all images in a single web panel with certain number of images per row.")
    add("--display_slice", type=int, default=64, help="the slice index to display if inputs are 3D volumes")
    add("--display_freq", type=int, default=100, help="frequency of showing training results on screen")
    add("--save_latest_freq", type=int, default=400, help="frequency of saving the latest results")
    add("--save_freq", type=int, default=4000, help="frequency of saving checkpoints at the end of iterationss")
    add("--evaluation_freq", type=int, default=200, help="evaluation freq")
    add("--load_mode", type=str, default="twoview", help="load entries randomly (train) or in order (test time)")
    add("--num_patches", type=int, default=512, help="number of patches")
    add("--lr_policy", type=str, default="const_linear", help="specify learning rate policy to use")
    add("--init_type", type=str, default="kaiming", help="network initialization strategy")
    add("--n_val_during_train", type=int, default=50, help="number of batches to sample during a validation step")
    add("--lambda_NCE", type=float, default=1, help="weight for NCE loss")
    add("--netF_nc", type=int, default=256, help="number of neurons for netF, the patch sampling MLP")
    add("--normG", type=str, default="batch", help="instance/batch/no/layer norm for base network")
    add("--normF", type=str, default="batch", help="instance/batch/no/layer norm for MLP")
    add("--norm_eps_G", type=float, default=1e-5, help="epsilon in base-network (UNet) norm layers")
    add("--norm_eps_F", type=float, default=1e-5, help="epsilon in MLP (netF) norm layers")
    add("--netG", type=str, default="unet", choices=["unet", "primus"], help="base network architecture")
    add("--grad_accum_iters", type=int, default=1, help="Gradient accumulation iterations")
    add("--clip_grad", type=str, default="False", help="whether to clip gradients of netG and netF (True/False)")
    add("--max_norm_G", type=float, default=2.0, help="gradient clip norm max for base network (netG)")
    add("--max_norm_F", type=float, default=2.0, help="gradient clip norm max for MLP head (netF)")
    add("--continue_train", type=str, default="False", help="continue training: load the latest model (True/False)")
    add("--max_iters", type=int, default=0, help="hard cap on total_iters; 0 disables. Useful for smoke tests.")
    add("--pretrained_name", type=str, default="None",
        help="warm-start network weights from another run's checkpoint dir (loads <ckpt_dir>/<pretrained_name>/<epoch>_net_{G,F}.pth). "
             "'None' disables. Mutually exclusive with --continue_train.")
    add("--pretrained_G_only_ckpt", type=str, default="None",
        help="warm-start only the base network (netG) from a specific .pth file; the MLP head (netF) stays randomly initialized. "
             "'None' disables.")
    add("--gpu_ids", type=int, default=0, help="gpu ids: e.g. 0  0,1,2, 0,2. use -1 for CPU")
    add("--nce_layers", type=str, default="27,31,38,45,52,65", help="comma-separated list of layers for NCE loss")
    add("--nce_weights", type=str, default="1,1,1,1,1,1", help="comma-separated list of weights for NCE loss layers")
    add("--seed", type=int, default=1234567, help="Seed for torch, np, and random packages")
    add("--apply_same_inten_augment", type=str, default="False",
        help="Whether to perform the same intensity augmentation on view 1 & 2 (True/False)")
    add("--pool_type", type=str, default="Max", choices=["Max", "Avg"], help="pooling type for downsampling")
    add("--interp_type", type=str, default="nearest", choices=["nearest", "trilinear"], help="interpolation type for upsampling")
    add("--weigh_rarity", type=str, default="False",
        help="weight patches by inverse class frequency in the contrastive loss to counter class imbalance (True/False)")
    add("--balance_denominator", type=str, default="False",
        help="balance the contrastive denominator (BCL-style) so every class contributes equal repulsion mass regardless of patch "
             "count (True/False)")
    add("--weighting_mode", type=str, default="raw", choices=["raw", "sqrt"],
        help="how class counts map to rarity weights for --weigh_rarity / --balance_denominator: 'raw' (inverse counts, default) or "
             "'sqrt' (inverse sqrt counts, a softer correction). No effect unless one of those flags is set.")
    add("--primus_version", type=str, default="v1", choices=["v1", "v2"],
        help="v1 (single-conv patch embed) or v2 (deeper residual patch embed; v2 requires --primus_patch_size 8).")
    add("--primus_config", type=str, default="B", choices=["S", "B", "M", "L"],
        help="ViT scale as depth/heads/embedding width: S=12/6/396, B=12/12/792, M=16/12/864, or L=24/16/1056.")
    add("--primus_patch_size", type=int, default=8,
        help="Tokenizer patch size (isotropic); crop_size must be divisible by it. v2 requires 8.")
    add("--primus_drop_path_rate", type=float, default=0.0,
        help="Maximum probability of skipping a transformer block during training; 0 disables stochastic depth.")
    add("--primus_num_register_tokens", type=int, default=0,
        help="Number of learned tokens included in attention but discarded before decoding; 0 disables them.")
    add("--primus_v2_in_eps", type=float, default=1e-5,
        help="InstanceNorm3d eps in the v2 deeper tokenizer (v2 only; default 1e-5 matches upstream). Also used as the "
             "--primus_out_norm eps.")
    add("--primus_qk_norm", type=str2bool, nargs="?", const=True, default=False,
        help="Enable QK-norm (per-head LayerNorm on q,k) in the ViT attention. Adds eva.blocks.*.attn.{q,k}_norm params (changes "
             "the state_dict).")
    add("--primus_out_norm", type=primus_out_norm_mode, nargs="?", const="instance", default="none",
        choices=["none", "instance", "demean", "layernorm", "layernorm_affine"],
        help="Decoded-volume norm: instance/demean operate spatially per channel; layernorm modes operate across channels per voxel; "
             "none disables. Only layernorm_affine adds parameters. A bare flag or true selects instance; false selects none. Uses "
             "--primus_v2_in_eps.")
    add("--primus_register_init_std", type=float, default=0.02,
        help="Init std for register tokens (upstream 1e-6). Only used when --primus_num_register_tokens > 0.")
    # ---- this package's own
    add("--precision", type=str, default="bf16", help="storage precision of the UNet's HIP training path (bf16: what the reference's "
                                                       "autocast trains in; f16, bf16x2 / strict); ignored with --netG primus")
    add("--graph", type=str, default="auto", choices=["auto", "off"],
        help="auto: replay the step from a HIP graph when grad_accum_iters is 1 and the batch has the captured shape; off: always eager")
    add("--loader_seed", type=int, default=0, help="seed of the loader's epoch order and augmentation parameters")
    add("--out_log", type=str, default=None, help="path of the JSON-lines log (default <ckpt_dir>/<name>/log.jsonl)")
    if primus_route:
        add("--primus_train_route", type=str, default="hip", choices=list(PRIMUS_TRAIN_ROUTES),
            help="--netG primus: who runs the attention cores and the blocks' linear layers under autograd: hip (this package's "
                 "kernels, PrimusV2.train_attention / train_linear) or torch")
        add("--primus_train_tokenizer", type=str, default="torch", choices=list(PRIMUS_TRAIN_ROUTES),
            help="--netG primus: who runs the conv tokenizer's stem and stages under autograd: torch (vendor convolutions) or hip (this "
                 "package's kernels, PrimusV2.train_tokenizer)")
        add("--primus_train_norm", type=str, default="torch", choices=list(PRIMUS_TRAIN_ROUTES),
            help="--netG primus: who runs the blocks' token LayerNorms, the SwiGLU gate product and the final norm under autograd: torch "
                 "(the modules) or hip (this package's kernels, PrimusV2.train_norm)")
        add("--primus_train_decoder", type=str, default="torch", choices=list(PRIMUS_TRAIN_ROUTES),
            help="--netG primus: who runs the dense patch decoder and a spatial output norm (demean, instance) under autograd: torch "
                 "(vendor transposed convolutions) or hip (this package's kernels, PrimusV2.train_decoder)")
    return parser


def options_from_args(args):
    """The trainer's option namespace from the launcher's arguments: what the launcher puts on the trainer's command line, parsed
    as the trainer parses it (string booleans, ``--gpu_ids`` as a list, 'None' as None), over ``TRAINER_DEFAULTS``."""
    opt = Namespace(**TRAINER_DEFAULTS)
    for k, v in vars(args).items():
        setattr(opt, k, v)
    opt.checkpoints_dir = args.ckpt_dir
    del opt.ckpt_dir
    for k in ("clip_grad", "continue_train", "apply_same_inten_augment", "weigh_rarity", "balance_denominator"):
        setattr(opt, k, str2bool(str(getattr(args, k))))
    opt.gpu_ids = [int(s) for s in str(args.gpu_ids).split(",") if int(s) >= 0]
    for k in ("pretrained_name", "pretrained_G_only_ckpt"):
        if getattr(opt, k) in (None, "None"):
            setattr(opt, k, None)
    opt.isTrain = True
    if not hasattr(opt, "primus_train_route"):
        opt.primus_train_route = "hip"
    if not hasattr(opt, "primus_train_tokenizer"):
        opt.primus_train_tokenizer = "torch"
    if not hasattr(opt, "primus_train_norm"):
        opt.primus_train_norm = "torch"
    if not hasattr(opt, "primus_train_decoder"):
        opt.primus_train_decoder = "torch"
    return opt


def _refusals(opt):
    if opt.netG == "primus":
        if opt.primus_version != "v2":
            raise NotImplementedError(f"--netG primus --primus_version {opt.primus_version}: there is no Primus v1 class in this package "
                                      "(its single-conv patch embed was never built); pass --primus_version v2")
        if opt.primus_patch_size != 8:
            raise NotImplementedError(f"--primus_patch_size {opt.primus_patch_size}: PrimusV2's deeper patch embed is hardwired to an 8x stride")
        if opt.crop_size <= 0 or opt.crop_size % 8:
            raise NotImplementedError(f"--crop_size {opt.crop_size}: a PrimusV2 input is a positive multiple of the patch size 8")
        if opt.primus_drop_path_rate != 0:
            raise NotImplementedError(f"--primus_drop_path_rate {opt.primus_drop_path_rate}: drop-path (stochastic depth) is not implemented")
        if opt.graph == "on":
            raise NotImplementedError("--graph on with --netG primus: the Primus step is not captured in a HIP graph, it runs eagerly")
        if getattr(opt, "primus_train_route", "hip") not in PRIMUS_TRAIN_ROUTES:
            raise NotImplementedError(f"--primus_train_route {opt.primus_train_route}: one of {PRIMUS_TRAIN_ROUTES}")
        if getattr(opt, "primus_train_tokenizer", "torch") not in PRIMUS_TRAIN_ROUTES:
            raise NotImplementedError(f"--primus_train_tokenizer {opt.primus_train_tokenizer}: one of {PRIMUS_TRAIN_ROUTES}")
        if getattr(opt, "primus_train_norm", "torch") not in PRIMUS_TRAIN_ROUTES:
            raise NotImplementedError(f"--primus_train_norm {opt.primus_train_norm}: one of {PRIMUS_TRAIN_ROUTES}")
        if getattr(opt, "primus_train_decoder", "torch") not in PRIMUS_TRAIN_ROUTES:
            raise NotImplementedError(f"--primus_train_decoder {opt.primus_train_decoder}: one of {PRIMUS_TRAIN_ROUTES}")
    elif opt.netG != "unet":
        raise NotImplementedError(f"--netG {opt.netG}: only the UNet and PrimusV2 are built")
    if opt.ndims != 3:
        raise NotImplementedError(f"--ndims {opt.ndims}: the HIP path is 3-D only (the reference supports only 3 as well)")
    if len(opt.gpu_ids) == 0:
        raise NotImplementedError("--gpu_ids -1: the step runs on HIP kernels, there is no host path")
    if opt.pretrained_name is not None and opt.continue_train:
        raise NotImplementedError("--pretrained_name together with --continue_train: the two are mutually exclusive (resume this run, "
                                  "or warm-start from another)")
    if opt.model != "supcl" or opt.netF != "mlp_sample":
        raise NotImplementedError(f"--model {opt.model} / --netF {opt.netF}: only supcl with mlp_sample exists")


def _init_weights(net, init_type, init_gain):
    """init_weights of the reference (pretraining_networks.py:666-715): conv / linear weights by ``init_type`` with zero biases,
    BatchNorm3d scales ~ N(1, init_gain) with zero shifts."""
    init = torch.nn.init
    for m in net.modules():
        name = m.__class__.__name__
        if hasattr(m, "weight") and ("Conv" in name or "Linear" in name):
            if init_type == "normal":
                init.normal_(m.weight.data, 0.0, init_gain)
            elif init_type == "xavier":
                init.xavier_normal_(m.weight.data, gain=init_gain)
            elif init_type == "kaiming":
                init.kaiming_normal_(m.weight.data, a=0, mode="fan_in")
            elif init_type == "orthogonal":
                init.orthogonal_(m.weight.data, gain=init_gain)
            else:
                raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
            if getattr(m, "bias", None) is not None:
                init.constant_(m.bias.data, 0.0)
        elif "BatchNorm2d" in name or "BatchNorm3d" in name:
            init.normal_(m.weight.data, 1.0, init_gain)
            init.constant_(m.bias.data, 0.0)


def build_networks(opt, device):
    """netG, netF (heads not created yet) and one criterion per nce layer, as SupCLModel.__init__ builds them (supcl_model.py:380-489)."""
    from ..model.network import Unet
    from .patch_sample import PatchSampleF
    from .supcon import SupPatchNCELoss
    if not hasattr(opt, "nce_layers_list"):
        opt.nce_layers_list, opt.nce_weights_list = _layers_and_weights(opt)
    with contextlib.redirect_stdout(io.StringIO()):
        if opt.netG == "primus":
            netG = _build_primus(opt)
        else:
            netG = Unet(opt.ndims, opt.input_nc, opt.output_nc, opt.num_downs, ngf=opt.ngf, norm=opt.normG, final_act="none",
                        activation=opt.actG, pooling=opt.pool_type, interp=opt.interp_type, norm_eps=opt.norm_eps_G)
        netF = PatchSampleF(use_mlp=opt.use_mlp, init_type=opt.init_type, init_gain=opt.init_gain, nc=opt.netF_nc, n_mlps=opt.n_mlps,
                            activation=opt.actF, norm=opt.normF, norm_eps=opt.norm_eps_F)
    if opt.netG != "primus":                    # (define_G: initialize_weights=False for the ViT, pretraining_networks.py:146-148)
        _init_weights(netG, opt.init_type, opt.init_gain)
        netG.precision = opt.precision
    netG = netG.to(device).train()
    crits = [SupPatchNCELoss(opt) for _ in opt.nce_layers_list]
    return netG, netF, crits


def _build_primus(opt):
    """``define_G``'s PrimusV2 (pretraining_networks.py:107-148): the config's depth / heads / width, LayerScale 0.1, the inner
    attention norm, the options' QK norm, output norm, register tokens and eps; no ``init_weights`` pass."""
    from ..model.vit3d import PRIMUS_CONFIGS, PrimusV2
    conf = PRIMUS_CONFIGS[opt.primus_config]
    if opt.primus_num_register_tokens < 0:
        raise ValueError("primus_num_register_tokens must be >= 0 (got %d)" % opt.primus_num_register_tokens)
    ps, cs = opt.primus_patch_size, opt.crop_size
    net = PrimusV2(input_channels=opt.input_nc, num_classes=opt.output_nc, embed_dim=conf["embed_dim"], eva_depth=conf["eva_depth"],
                   eva_numheads=conf["eva_numheads"], patch_embed_size=(ps, ps, ps), input_shape=(cs, cs, cs),
                   drop_path_rate=opt.primus_drop_path_rate, num_register_tokens=opt.primus_num_register_tokens, init_values=0.1,
                   scale_attn_inner=True, qk_norm=opt.primus_qk_norm, out_norm=opt.primus_out_norm, out_norm_eps=opt.primus_v2_in_eps,
                   register_init_std=opt.primus_register_init_std, in_eps=opt.primus_v2_in_eps)
    net.train_attention = net.train_linear = getattr(opt, "primus_train_route", "hip")
    net.train_tokenizer = getattr(opt, "primus_train_tokenizer", "torch")
    net.train_norm = getattr(opt, "primus_train_norm", "torch")
    net.train_decoder = getattr(opt, "primus_train_decoder", "torch")
    return net


def _layers_and_weights(opt):
    if opt.netG == "primus":                    # supcl_model.py:403-410
        print("3D ViT: single-scale NCE on the final feature map (logged as layer -1)")
        return [-1], [1.0]
    layers = [int(i) for i in opt.nce_layers.split(",")] if opt.nce_layers != "" else []
    if opt.nce_weights != "1":
        w = [float(i) for i in opt.nce_weights.split(",")]
        total = float(np.sum(np.asarray(w)))
        w = [i / total for i in w]
    else:
        w = [1.0 / len(layers) for _ in layers]
    if len(w) != len(layers):
        raise ValueError(f"--nce_weights has {len(w)} entries for {len(layers)} --nce_layers")
    return layers, w


class _Snapshot:
    """Weights, buffers and optimizer state before the warm-up steps of a graph capture, put back IN PLACE afterwards (the captured
    graph holds the tensors' addresses): the capture then has trained nothing."""

    def __init__(self, nets, optimizers):
        self.nets, self.optimizers = nets, optimizers
        self.tensors = [(t, t.detach().clone()) for net in nets for t in list(net.parameters()) + list(net.buffers())]
        self.state = {id(p): {k: v.detach().clone() for k, v in st.items() if torch.is_tensor(v)}
                      for o in optimizers for p, st in o.state.items()}

    @torch.no_grad()
    def restore(self):
        for t, saved in self.tensors:
            t.copy_(saved)
        for o in self.optimizers:
            for p, st in o.state.items():
                saved = self.state.get(id(p), {})
                for k, v in st.items():
                    if torch.is_tensor(v):
                        v.copy_(saved[k]) if k in saved else v.zero_()


def _finite_or_none(v):
    return v if isinstance(v, (int, float)) and math.isfinite(v) else None


def pretrain(opt, train_loader=None, val_loader=None, on_step=None, sample_ids=None):
    """The training loop of trainers/train.py on ``opt`` (``options_from_args``).  ``train_loader`` / ``val_loader``: iterables of the
    loader's batches (default: ``AugmentedTwoViewLoader`` over ``opt.dataroot``; validation with ``isTrain=False, batch_size=1,
    crop_size=-1``); a loader with ``set_epoch`` gets the epoch, one with ``dataset`` gives the epoch size.  ``on_step(info)`` is
    called before (``info["phase"] == "start"``) and after (``"end"``, with ``info["record"]``) every iteration; ``info`` also holds
    total_iters, epoch, netG, netF, optimizers, schedulers.  ``sample_ids``: fixed patch coordinates per layer for every training
    step (tests).  Returns a dict(start_iters, total_iters, epoch, best_evaluation_loss, last_eval_loss, save_dir, netG, netF, optimizers,
    schedulers)."""
    from .loader import AugmentedTwoViewLoader
    from .optim import FusedAdamW
    from .step import GraphedContrastiveStep, contrastive_step, validation_loss
    _refusals(opt)
    torch.manual_seed(opt.seed)
    random.seed(opt.seed)
    np.random.seed(opt.seed)
    device = torch.device("cuda", opt.gpu_ids[0])
    save_dir = os.path.join(opt.checkpoints_dir, opt.name)
    os.makedirs(save_dir, exist_ok=True)
    opt.nce_layers_list, opt.nce_weights_list = _layers_and_weights(opt)
    layers, weights = opt.nce_layers_list, opt.nce_weights_list

    if train_loader is None:
        train_loader = AugmentedTwoViewLoader(opt, device=device, seed=opt.loader_seed)
    if val_loader is None:
        val_opt = copy.copy(opt)
        val_opt.isTrain, val_opt.batch_size, val_opt.crop_size = False, 1, -1
        val_loader = AugmentedTwoViewLoader(val_opt, device=device, seed=opt.loader_seed)
    train_size = len(train_loader.dataset) if hasattr(train_loader, "dataset") else len(train_loader) * opt.batch_size
    print(f"The number of training images = {train_size}")

    netG, netF, crits = build_networks(opt, device)
    if opt.netG == "primus" and not os.path.exists(os.path.join(save_dir, "netG.txt")):      # supcl_model.py:449-454
        with open(os.path.join(save_dir, "netG.txt"), "w") as f:
            print(netG, file=f)
    okw = dict(lr=opt.lr, betas=(opt.beta1, opt.beta2), eps=opt.eps, weight_decay=opt.weight_decay)
    opt_G = FusedAdamW(netG.parameters(), max_norm=opt.max_norm_G if opt.clip_grad else None, **okw)
    optimizers, schedulers = [opt_G], []
    nets = {"G": netG}

    total_iters, last_eval_loss, best_evaluation_loss = 0, -1, 9999
    resume = bool(opt.continue_train)
    if resume:
        peek = ckpt.peek_training_state(save_dir)
        if peek is not None:
            total_iters = int(peek["total_iters"])
            opt.epoch = str(total_iters)
            opt.epoch_count = total_iters // train_size
            print(f"Resuming from iter {total_iters} (epoch {opt.epoch_count}); will load {opt.epoch}_net_*.pth and {ckpt.TRAIN_STATE}")
        else:
            print(f"continue_train requested but no {ckpt.TRAIN_STATE} in {save_dir}; starting from scratch")
            resume, opt.continue_train, opt.epoch, opt.epoch_count = False, False, "0", 0
    if resume and ckpt.read_best_val(save_dir) is not None:
        best_evaluation_loss = ckpt.read_best_val(save_dir)
    start_iters = total_iters
    print(f"Starting iters: {start_iters}")

    log_path = opt.out_log or os.path.join(save_dir, "log.jsonl")
    log = open(log_path, "a" if resume else "w")

    def emit(**kw):
        log.write(json.dumps(kw) + "\n")
        log.flush()

    def train_state(epoch):
        ckpt.save_training_state(save_dir, optimizers, schedulers, None,
                                 {"total_iters": total_iters, "epoch": epoch, "best_evaluation_loss": best_evaluation_loss,
                                  "last_eval_loss": last_eval_loss})

    step_kw = dict(nce_weights=weights, num_patches=opt.num_patches, lambda_nce=opt.lambda_NCE)
    graphed, graph_shape, graph_grads = None, None, False
    initialized, stop_now, epoch = False, False, opt.epoch_count
    try:
        for epoch in range(opt.epoch_count, opt.n_epochs + opt.n_epochs_decay + 1):
            if epoch > opt.stop_epoch:
                print(f"stop training at epoch {epoch}")
                break
            if stop_now:
                break
            epoch_start, epoch_iter = time.time(), 0
            if hasattr(train_loader, "set_epoch"):
                train_loader.set_epoch(epoch)
            for data in train_loader:
                A, B, seg = (data[k].to(device).float() if k != "A_seg" else data[k].to(device) for k in ("A", "B", "A_seg"))
                batch_size = A.size(0)
                total_iters += batch_size
                epoch_iter += batch_size
                if not initialized:
                    # data_dependent_initialize + setup (supcl_model.py:539-601, base_model.py:107-144): the heads from one forward +
                    # backward of the first batch, netF's optimizer, the schedulers, then whatever is to be loaded
                    with contextlib.redirect_stdout(io.StringIO()):
                        contrastive_step(netG, netF, crits, A, B, seg, layers, optimizers=None, **step_kw)
                    netF = netF.to(device).train()
                    for p in list(netG.parameters()) + list(netF.parameters()):
                        p.grad = None
                    if opt.use_mlp:
                        nets["F"] = netF
                        optimizers.append(FusedAdamW(netF.parameters(), max_norm=opt.max_norm_F if opt.clip_grad else None, **okw))
                    if len(optimizers) != 2:
                        raise NotImplementedError("--use_mlp False: the step takes (opt_G, opt_F)")
                    schedulers = [get_scheduler(o, opt) for o in optimizers]
                    if resume:
                        ckpt.load_networks(save_dir, opt.epoch, nets, device)
                    elif opt.pretrained_name is not None:
                        ckpt.load_networks(os.path.join(opt.checkpoints_dir, opt.pretrained_name), opt.epoch, nets, device)
                    elif opt.pretrained_G_only_ckpt is not None:
                        ckpt.load_G_only(opt.pretrained_G_only_ckpt, netG, device)
                    if resume:
                        # (total_iters stays the peeked one plus this batch: taking it from the file again would replay an iteration)
                        extras = ckpt.load_training_state(save_dir, optimizers, schedulers, None, device)
                        if extras is not None:
                            best_evaluation_loss = float(extras.get("best_evaluation_loss", best_evaluation_loss))
                            last_eval_loss = float(extras.get("last_eval_loss", last_eval_loss))
                            print(f"Restored training state at iter {extras.get('total_iters')}; best_val={best_evaluation_loss:.6f}")
                    initialized = True
                info = dict(phase="start", total_iters=total_iters, epoch=epoch, netG=netG, netF=netF, optimizers=optimizers,
                            schedulers=schedulers)
                if on_step is not None:
                    on_step(info)

                shape = (tuple(A.shape), tuple(B.shape), tuple(seg.shape))
                # (a Primus step runs eagerly: --graph auto resolves to off for it, --graph on was refused)
                use_graph = (opt.graph == "auto" and opt.netG != "primus" and opt.grad_accum_iters == 1 and
                             (graph_shape is None or shape == graph_shape))
                if use_graph:
                    if graphed is None:
                        graphed = GraphedContrastiveStep(netG, netF, crits, layers, tuple(optimizers), warmup=2, sample_ids=sample_ids,
                                                         **step_kw)
                        graph_shape = shape
                        snap = _Snapshot((netG, netF), optimizers)
                        with contextlib.redirect_stdout(io.StringIO()):
                            graphed._capture(A, B, seg)
                        snap.restore()
                        del snap
                    rec = graphed(A, B, seg)
                    graph_grads = True
                else:
                    if graph_grads:             # the last replay's gradients are still in .grad: an eager backward would add to them
                        for p in list(netG.parameters()) + list(netF.parameters()):
                            p.grad = None
                        graph_grads = False
                    rec = contrastive_step(netG, netF, crits, A, B, seg, layers, optimizers=tuple(optimizers), sample_ids=sample_ids,
                                           grad_accum_iters=opt.grad_accum_iters, iters=total_iters, **step_kw)
                del data

                lr = optimizers[0].param_groups[0]["lr"]
                if total_iters % opt.print_freq == 0:
                    emit(kind="train", total_iters=total_iters, epoch=epoch, loss=rec["loss"], per_layer=dict(rec["per_layer"]), lr=lr,
                         grad_norm_G=_finite_or_none(rec["grad_norm_G"]), grad_norm_F=_finite_or_none(rec["grad_norm_F"]))
                    print(f"(epoch: {epoch}, iters: {total_iters}) NCE: {rec['loss']:.4f} lr {lr:.3g}")
                if total_iters % opt.save_latest_freq == 0:
                    print(f"saving the latest model (epoch {epoch}, total_iters {total_iters})")
                    ckpt.save_networks(save_dir, f"iter_{total_iters}" if opt.save_by_iter else "latest", nets)

                if total_iters % opt.evaluation_freq == 0:
                    ckpt.save_networks(save_dir, total_iters, nets)
                    train_state(epoch)
                    cur, cnt = 0.0, 0
                    print(f"{total_iters} iters, Evaluation starts ...")
                    for vcnt, vdata in enumerate(val_loader):
                        if vcnt > opt.n_val_during_train:
                            break
                        v = validation_loss(netG, netF, crits, vdata["A"].to(device).float(), vdata["B"].to(device).float(),
                                            vdata["A_seg"].to(device), layers, **step_kw)
                        cur += v["loss"]
                        cnt += 1
                    if cnt == 0:
                        raise RuntimeError("the validation loader yielded no batch")
                    cur /= cnt
                    print(f"Best validation loss: {best_evaluation_loss}, current validation loss {cur}")
                    if cur < best_evaluation_loss:
                        best_evaluation_loss = cur
                        ckpt.save_networks(save_dir, "best_val", nets)
                        ckpt.write_best_val(save_dir, best_evaluation_loss)
                    last_eval_loss = cur
                    emit(kind="val", total_iters=total_iters, epoch=epoch, loss=cur, best=best_evaluation_loss, n=cnt)
                    if opt.lr_policy == "plateau":
                        update_learning_rate(schedulers, opt.lr_policy, cur)

                if on_step is not None:
                    info.update(phase="end", record=rec)
                    on_step(info)
                if opt.max_iters > 0 and total_iters >= opt.max_iters:
                    print(f"Reached max_iters={opt.max_iters} at total_iters={total_iters}; saving final train_state and stopping.")
                    ckpt.save_networks(save_dir, total_iters, nets)
                    train_state(epoch)
                    stop_now = True
                    break

            if total_iters % opt.save_freq == 0:
                print("saving the model at the end of epoch %d, iters %d" % (epoch, total_iters))
                ckpt.save_networks(save_dir, "latest", nets)
                ckpt.save_networks(save_dir, total_iters, nets)
                train_state(epoch)
            print("Total iters %d, End of epoch %d / %d \t Time Taken: %d sec"
                  % (total_iters, epoch, opt.n_epochs + opt.n_epochs_decay, time.time() - epoch_start))
            if opt.lr_policy != "plateau" and schedulers:
                update_learning_rate(schedulers, opt.lr_policy)
                print("learning rate = %.7f" % optimizers[0].param_groups[0]["lr"])
    finally:
        log.close()
    return dict(start_iters=start_iters, total_iters=total_iters, epoch=epoch, best_evaluation_loss=best_evaluation_loss, last_eval_loss=last_eval_loss,
                save_dir=save_dir, netG=netG, netF=netF, optimizers=optimizers, schedulers=schedulers)


def main(argv=None):
    args = build_parser(primus_route=True).parse_args(argv)
    return pretrain(options_from_args(args))


if __name__ == "__main__":
    main()
