"""The pretraining loader with the reference's default augmentation: ``H5SupCLDataset`` for reading, view draws and normalisation
(the pinned ones), then the two-view augmentation on the device (``augment.augment_pair``, csrc/amx_preaug.hip) and the crop, in
place of the TorchIO branch of h5supcl_dataset.py:260-303, 350-352 that runs in the reference's CPU workers.  A dataset inside CPU
workers cannot launch kernels, so this is a layer on top of the dataset, not a change to it: ``H5SupCLDataset`` itself keeps
refusing ``opt.augment`` and ``opt.resize``."""
from __future__ import annotations

import copy

import numpy as np
import torch

from .augment import augment_pair, draw_params
from .data import H5SupCLDataset, random_crop

_IMG_KEYS = ("A", "B", "A_seg", "B_seg")


class AugmentedTwoViewLoader:
    """Iterates over the collated batches of the reference's loader: ``A``, ``B``, ``A_seg``, ``B_seg`` as float32 [B, 1, d, h, w] on
    ``device``, ``A_id`` / ``B_id`` int64 [B, 1], ``meta`` a list of subject names, ``keys`` the reference's collated key list.

    ``opt``: the reference's option namespace.  The dataset is built from a copy with ``augment=False, crop_size=0``; with
    ``opt.augment`` and ``opt.isTrain`` every sample is moved to the device and goes through ``augment_pair`` with parameters drawn from
    this loader's ``numpy.random.RandomState``; otherwise samples pass through with the reference's crop rule (``random_crop``, global
    numpy state, training only).  The order of an epoch is a permutation seeded by (seed, epoch) when training, the dataset's order
    otherwise; the trailing incomplete batch is kept.  ``opt.resize`` raises."""

    def __init__(self, opt, device=None, seed=0):
        if getattr(opt, "resize", False):
            raise NotImplementedError("opt.resize (TorchIO Resize, h5supcl_dataset.py:109-117) is not part of the accelerated path")
        self.opt = opt
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"AugmentedTwoViewLoader: the augmentation runs on the GPU and has no host path (got {self.device})")
        plain = copy.copy(opt)
        plain.augment, plain.crop_size = False, 0
        self.dataset = H5SupCLDataset(plain)
        self.isTrain = bool(opt.isTrain)
        self.augment = self.isTrain and bool(getattr(opt, "augment", False))
        self.crop_size = int(getattr(opt, "crop_size", 0) or 0)
        self.batch_size = int(opt.batch_size)
        self.seed = int(seed)
        self.set_epoch(0)

    def set_epoch(self, epoch):
        """Seeds the order and the augmentation parameters of the next iteration: the same (seed, epoch) gives the same batches
        (the dataset's own view draws come from torch's global generator, as in the reference)."""
        self.epoch = int(epoch)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _sample(self, index, rng):
        s = self.dataset[index]
        if not self.augment:
            if self.crop_size > 0 and self.isTrain:
                s = random_crop(s, list(_IMG_KEYS), self.crop_size, self.dataset.dimension)
            for k in _IMG_KEYS:
                s[k] = s[k].contiguous().to(self.device)
            return s
        A, B, seg = (s[k].to(self.device) for k in ("A", "B", "A_seg"))
        params = draw_params(rng, tuple(A.shape[1:]), self.opt)
        s["A"], s["B"], s["A_seg"], s["B_seg"] = augment_pair(A, B, seg, params, crop_size=params["crop_size"])
        return s

    def __iter__(self):
        rng = np.random.RandomState([self.seed & 0x7fffffff, self.epoch & 0x7fffffff])
        n = len(self.dataset)
        order = rng.permutation(n) if self.isTrain else np.arange(n)
        for lo in range(0, n, self.batch_size):
            samples = [self._sample(int(i), rng) for i in order[lo:lo + self.batch_size]]
            shapes = {tuple(s["A"].shape) for s in samples}
            if len(shapes) != 1:
                raise ValueError(f"the samples of one batch must share a shape after the crop (got {sorted(shapes)}); "
                                 "use batch_size 1 or a crop_size no axis is shorter than")
            batch = {k: torch.stack([s[k] for s in samples]) for k in _IMG_KEYS}
            batch["A_id"] = torch.from_numpy(np.stack([s["A_id"] for s in samples]))
            batch["B_id"] = torch.from_numpy(np.stack([s["B_id"] for s in samples]))
            batch["meta"] = [s["meta"] for s in samples]
            batch["keys"] = [tuple(k for _ in samples) for k in _IMG_KEYS]      # default_collate of each sample's key list
            yield batch
