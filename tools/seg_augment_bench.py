"""Times the augmentation chain of segmentation finetuning at the reference's training shape: a batch
[4, 1, 128^3] out of four resident 160 x 192 x 160 volumes, every switch on.

    python tools/seg_augment_bench.py [--out profiles/seg_augment.json]

In one process, the routes alternating, 3 warm-up + 10 timed repetitions each, timed with device events:
  * ``hip``    anatomix_amd.segmentation.augment.augment_batch (csrc/amx_segaug.hip; the Gibbs FFTs are torch.fft on both routes);
  * ``torch``  the same definitions composed from torch ops on the device (slicing, broadcasting, F.conv3d, F.grid_sample);
  * both per stage as well, on the same intermediate tensors;
  * ``step``   one finetune_loss forward + backward + FusedAdamW step of the 6 M UNet with its head at the same batch.
It records medians with min and max, the chain's achieved GB/s on its algorithmic bytes, the largest difference between the two
routes' outputs, and the reference-style host cost: the float32 numpy restatement of the chain (tests/_segaug_ref.py) on one
sample, alone and as 16 samples over 16 threads."""
import argparse
import json
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _timing import TIMED, WARMUP, stats, timed            # noqa: E402
import _segaug_ref as AR                                    # noqa: E402
from anatomix_amd.segmentation import augment as G          # noqa: E402

B, CROP, VOL = 4, 128, (160, 192, 160)
# bytes per output voxel that each stage has to move at least once (fp32 image, uint8 label)
STAGE_BYTES = {"crop_noise_bias": 4 + 1 + 4 + 4 + 1, "contrast": 4 + 4 + 4, "smooth": 3 * 8, "sharpen": 5 * 8 + 12, "affine": 5 + 5, "rescale": 8}


def legendre(x):
    return [torch.ones_like(x), x, (3 * x * x - 1) / 2, (5 * x * x * x - 3 * x) / 2]


class TorchRoute:
    """The chain's definitions from torch ops, every switch on; the per-sample parameters as device tensors."""

    def __init__(self, p, dev):
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)
        self.p, self.dev = p, dev
        self.std, self.coeff, self.gamma, self.alpha = f(p["rand_std"]), f(p["coeff"]), f(p["gamma"]), f(p["sharpen_alpha"])
        self.A = f(p["affine"])
        self.taps = {k: self._taps(p[k]) for k in ("smooth_sigma", "sharpen_sigma1", "sharpen_sigma2")}
        lin = torch.linspace(-1, 1, CROP, device=dev)
        self.P = legendre(lin)
        o = torch.arange(CROP, device=dev, dtype=torch.float32) - (CROP - 1) / 2
        self.o = torch.stack(torch.meshgrid(o, o, o, indexing="ij"), -1)                  # [c, c, c, 3] in (z, y, x)

    def _taps(self, sig):
        w = torch.zeros((B, 3, 9))
        for b in range(B):
            for a in range(3):
                r, t = G.gaussian_taps(sig[b][a])
                w[b, a, 4 - r:4 + r + 1] = torch.tensor(t, dtype=torch.float32)
        return w.to(self.dev)

    def crop_noise_bias(self, vols, labs, noise):
        c = self.p["corner"]
        x = torch.stack([v[c[b][0]:c[b][0] + CROP, c[b][1]:c[b][1] + CROP, c[b][2]:c[b][2] + CROP] for b, v in enumerate(vols)])[:, None]
        y = torch.stack([v[c[b][0]:c[b][0] + CROP, c[b][1]:c[b][1] + CROP, c[b][2]:c[b][2] + CROP] for b, v in enumerate(labs)])[:, None]
        x = x + self.std.view(B, 1, 1, 1, 1) * noise
        f = torch.zeros_like(x)
        for q, (i, j, k) in enumerate(AR.coeff_index()):
            f = f + self.coeff[:, q].view(B, 1, 1, 1, 1) * (self.P[i].view(-1, 1, 1) * self.P[j].view(1, -1, 1) * self.P[k].view(1, 1, -1))
        return x * torch.exp(f), y

    def contrast(self, x):
        mn, mx = x.amin((1, 2, 3, 4), keepdim=True), x.amax((1, 2, 3, 4), keepdim=True)
        return ((x - mn) / (mx - mn + 1e-7)) ** self.gamma.view(B, 1, 1, 1, 1) * (mx - mn) + mn

    def _gauss(self, x, taps):
        x = x.view(1, B, CROP, CROP, CROP)
        x = F.conv3d(x, taps[:, 2].reshape(B, 1, 1, 1, 9), padding=(0, 0, 4), groups=B)
        x = F.conv3d(x, taps[:, 1].reshape(B, 1, 1, 9, 1), padding=(0, 4, 0), groups=B)
        x = F.conv3d(x, taps[:, 0].reshape(B, 1, 9, 1, 1), padding=(4, 0, 0), groups=B)
        return x.view(B, 1, CROP, CROP, CROP)

    def smooth(self, x):
        return self._gauss(x, self.taps["smooth_sigma"])

    def sharpen(self, x):
        b = self._gauss(x, self.taps["sharpen_sigma1"])
        return b + self.alpha.view(B, 1, 1, 1, 1) * (b - self._gauss(b, self.taps["sharpen_sigma2"]))

    def affine(self, x, y):
        src = torch.einsum("bij,zyxj->bzyxi", self.A, self.o) + (CROP - 1) / 2
        grid = (2 * src / (CROP - 1) - 1).flip(-1)
        img = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
        lab = F.grid_sample(y.float(), grid, mode="nearest", padding_mode="zeros", align_corners=True).to(torch.uint8)
        return img, lab

    def rescale(self, x):
        mn, mx = x.amin((1, 2, 3, 4), keepdim=True), x.amax((1, 2, 3, 4), keepdim=True)
        return (x - mn) / (mx - mn)

    def chain(self, vols, labs, noise, table):
        x, y = self.crop_noise_bias(vols, labs, noise)
        x = G._gibbs(x.contiguous(), list(range(B)), table)
        x = self.sharpen(self.smooth(self.contrast(x)))
        x, y = self.affine(x, y)
        return self.rescale(x), y


class HipStages:
    """The stages of augment_batch one by one (the same private calls, in its order)."""

    def __init__(self, table, labs, dev):
        self.t, self.dev, self.ldt = table, dev, labs[0].dtype

    def crop_noise_bias(self, vols, labs, noise):
        return G._crop(self.t, B, (CROP,) * 3, noise, self.ldt, self.dev)

    def contrast(self, x):
        return G._pointwise(x, torch.empty_like(x), G._minmax(x), G._OP_CONTRAST, self.t)

    def smooth(self, x):
        return G._gaussian(x, G._GAUSS_SMOOTH, self.t)

    def sharpen(self, x):
        return G._gaussian(x, G._GAUSS_SHARPEN, self.t)

    def affine(self, x, y):
        self.aff = G._affine(x, y, (CROP,) * 3, self.t)
        return self.aff[0], self.aff[1]

    def rescale(self, x):
        _, _, sc, nb = self.aff
        return G._pointwise(x, torch.empty_like(x), G._stream.minmax_finalize(sc, nb, B, x[0].numel(), self.dev), G._OP_SCALE, self.t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_augment.json"))
    ap.add_argument("--skip_step", action="store_true")
    ap.add_argument("--skip_host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    host = [AR.blob_volume(VOL, 200 + i) for i in range(B)]
    vols = [G.make_resident(img, dev) for img, _ in host]
    labs = [torch.from_numpy(lab.astype(np.uint8)).to(dev) for _, lab in host]
    p = G.draw_params(np.random.RandomState(0), CROP, [VOL] * B, B)
    for b in range(B):
        for k in p["on"]:
            p["on"][k][b] = True
        p["affine"][b] = G.affine_matrix(p["rotate"][b], p["shear"][b], p["scale"][b])
    noise = torch.randn((B, 1, CROP, CROP, CROP), generator=torch.Generator(dev).manual_seed(p["noise_seed"]), device=dev)
    table = G.build_table(vols, labs, p).device(dev)
    tr, hs = TorchRoute(p, dev), HipStages(table, labs, dev)
    res = {"shape": [B, 1, CROP, CROP, CROP], "volumes": list(VOL), "warmup": WARMUP, "timed": TIMED, "device": torch.cuda.get_device_name(0)}

    # whole chain, both routes
    t = timed({"hip": lambda: G.augment_batch(vols, labs, p, noise=noise), "torch": lambda: tr.chain(vols, labs, noise, table)})
    res["chain"] = {k: stats(v) for k, v in t.items()}
    a, b = G.augment_batch(vols, labs, p, noise=noise), tr.chain(vols, labs, noise, table)
    res["chain"]["max_abs_image_difference"] = float((a[0] - b[0]).abs().max())
    res["chain"]["label_disagreement_share"] = float((a[1] != b[1]).float().mean())

    # per stage, on the hip route's intermediates
    x0, y0 = hs.crop_noise_bias(vols, labs, noise)
    x1 = G._gibbs(x0.clone(), list(range(B)), table)
    x2 = hs.contrast(x1)
    x3 = hs.smooth(x2)
    x4 = hs.sharpen(x3)
    x5, y5 = hs.affine(x4, y0)
    res["stages"] = {}
    stage_args = {"crop_noise_bias": (vols, labs, noise), "contrast": (x1,), "smooth": (x2,), "sharpen": (x3,), "affine": (x4, y0), "rescale": (x5,)}
    for name, sargs in stage_args.items():
        t = timed({"hip": lambda: getattr(hs, name)(*sargs), "torch": lambda: getattr(tr, name)(*sargs)})
        res["stages"][name] = {k: stats(v) for k, v in t.items()}
        res["stages"][name]["bytes_per_voxel"] = STAGE_BYTES[name]
        res["stages"][name]["hip_gbps"] = STAGE_BYTES[name] * B * CROP ** 3 / (res["stages"][name]["hip"]["median_ms"] * 1e-3) / 1e9
    t = timed({"gibbs": lambda: G._gibbs(x0.clone(), list(range(B)), table)})
    res["stages"]["gibbs_torch_fft_both_routes"] = stats(t["gibbs"])
    kernel_ms = sum(res["stages"][k]["hip"]["median_ms"] for k in STAGE_BYTES)
    total_bytes = sum(STAGE_BYTES.values()) * B * CROP ** 3
    res["chain"]["algorithmic_bytes"] = total_bytes
    res["chain"]["hip_kernel_stages_ms"] = kernel_ms
    res["chain"]["hip_kernel_stages_gbps"] = total_bytes / (kernel_ms * 1e-3) / 1e9
    del x1, x2, x3, x4, x5, y5

    if not args.skip_step:
        from anatomix_amd.pretraining.optim import FusedAdamW
        from anatomix_amd.segmentation import DiceCELoss, finetune_loss, load_model
        torch.manual_seed(0)
        model = load_model(4, dev, ckpt_path="scratch").train()
        opt = FusedAdamW(model.parameters(), 2e-4, weight_decay=0)
        loss_fn = DiceCELoss(softmax=True, to_onehot_y=True, include_background=False)
        xin, yin = a

        def step():
            opt.zero_grad()
            finetune_loss(model, xin, yin, loss_fn).backward()
            opt.step()
        res["train_step"] = stats(timed({"step": step})["step"])

    if not args.skip_host:
        vol32, lab = vols[0].cpu().numpy(), host[0][1]
        nz = noise[0, 0].cpu().numpy()
        AR.chain_sample(vol32, lab, p, 0, nz, np.float32)
        one = []
        for _ in range(3):
            t0 = time.perf_counter()
            AR.chain_sample(vol32, lab, p, 0, nz, np.float32)
            one.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(lambda i: AR.chain_sample(vol32, lab, p, 0, nz, np.float32), range(16)))
        par = (time.perf_counter() - t0) * 1e3
        res["host_numpy_float32"] = {"one_sample": stats(one), "sixteen_samples_on_16_threads_ms": par, "ms_per_sample_on_16_threads": par / 16,
                                     "threads": 16, "cpus_seen": os.cpu_count()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
