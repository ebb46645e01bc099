"""Times the two-view augmentation of the contrastive pretraining at the reference's training shape: one
pair of 160 x 192 x 160 views with every switch on, cropped to 128^3.

    timeout -k 10 600 python tools/pretrain_augment_bench.py [--out profiles/pretrain_augment.json]

In one process, the routes alternating, 3 warm-up + 10 timed repetitions each, timed with device events:
  * ``hip``    anatomix_amd.pretraining.augment.augment_pair (csrc/amx_preaug.hip; the motion's FFTs are torch.fft on both routes);
  * ``torch``  the same definitions composed from torch ops on the device (F.grid_sample, F.conv3d on a reflect-padded input,
               pointwise ops, torch.fft);
  * both per stage as well, on the same intermediate tensors.
It records medians with min and max, each kernel stage's achieved GB/s on its algorithmic bytes and the largest difference between
the two routes' outputs.  The step time it is to be read against comes from ``python bench.py --workload step`` on the same machine."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _timing import TIMED, WARMUP, stats, timed            # noqa: E402
import _preaug_ref as PR                                    # noqa: E402
from anatomix_amd.pretraining import augment as G           # noqa: E402

VOL, CROP = (160, 192, 160), 128
# bytes per voxel and view that each kernel stage has to move at least once (fp32 image; the label adds 2 bytes to one view)
STAGE_BYTES = {"spatial": 4 + 4 + 1, "blur": 2 * (4 + 4), "intensity": 4 + 4 + 4}


class TorchRoute:
    """The chain's definitions from torch ops, every switch on."""

    def __init__(self, p, dev):
        self.p, self.dev = p, dev
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)      # noqa: E731
        self.M = f(p["map"])
        o = [torch.arange(n, device=dev, dtype=torch.float32) for n in VOL]
        self.o = torch.stack(torch.meshgrid(*o, indexing="ij") + (torch.ones(VOL, device=dev),), -1)      # [D, H, W, 4]
        self.size = f(VOL)
        self.taps, self.radius = [], []
        for a in range(3):
            r = [G.gaussian_taps(rec["sigma"][a]) for rec in p["views"]]
            R = max(t[0] for t in r)
            w = torch.zeros(2, 2 * R + 1)
            for v, (rv, t) in enumerate(r):
                w[v, R - rv:R + rv + 1] = torch.tensor(t, dtype=torch.float32)
            self.taps.append(w.to(dev))
            self.radius.append(R)
        self.std = f([rec["noise_std"] for rec in p["views"]]).view(2, 1, 1, 1)
        self.coeff = f([rec["coeff"] for rec in p["views"]])
        self.gamma = f([rec["gamma"] for rec in p["views"]]).view(2, 1, 1, 1)
        self.lin = [torch.linspace(-1, 1, n, device=dev) for n in VOL]

    def _grid(self, M):
        src = self.o @ M.T                                                        # [D, H, W, 3] in (z, y, x)
        return (2 * src / (self.size - 1) - 1).flip(-1)[None]

    def _sample(self, x, M, pad):
        """x [views, D, H, W]: grid_sample(x - pad, zeros) + pad."""
        g = self._grid(M)
        return F.grid_sample((x - pad)[None], g, mode="bilinear", padding_mode="zeros", align_corners=True)[0] + pad

    def spatial(self, x, lab):
        pad = x.amin((1, 2, 3), keepdim=True)
        out = self._sample(x, self.M, pad)
        olab = F.grid_sample(lab.float()[None, None], self._grid(self.M), mode="nearest", padding_mode="zeros", align_corners=True)[0, 0]
        return out, olab.to(torch.uint8)

    def blur(self, x):
        x = x[None]                                                               # the two views as the channels of a grouped conv
        for a in (2, 1, 0):
            R, dim = self.radius[a], a + 2
            if R == 0:
                continue
            n = x.shape[dim]
            x = torch.cat([x.narrow(dim, 0, R).flip(dim), x, x.narrow(dim, n - R, R).flip(dim)], dim)      # scipy's 'reflect'
            shape = [2, 1, 1, 1, 1]
            shape[dim] = 2 * R + 1
            x = F.conv3d(x, self.taps[a].reshape(shape), groups=2)
        return x[0]

    def intensity(self, x, noise):
        x = x + self.std * noise
        f = torch.zeros_like(x)
        for q, (i, j, k) in enumerate(PR.coeff_index()):
            f = f + self.coeff[:, q].view(2, 1, 1, 1) * (self.lin[0].view(-1, 1, 1) ** i * self.lin[1].view(1, -1, 1) ** j * self.lin[2].view(1, 1, -1) ** k)
        x = x * torch.exp(f)
        return torch.sign(x) * torch.abs(x) ** self.gamma

    def motion(self, x):
        out = []
        for v, rec in enumerate(self.p["views"]):
            xv = x[v]
            W = xv.shape[-1]
            cuts = [int(t * W) for t in rec["motion_times"]] + [W]
            k = torch.fft.fftshift(torch.fft.fft(xv, dim=-1), dim=-1)
            pad = xv.amin()
            for i in range(2):
                M = torch.as_tensor(G.rigid_map(VOL, rec["motion_degrees"][i], rec["motion_translation"][i]).astype(np.float32), device=self.dev)
                moved = self._sample(xv[None], M, pad)[0]
                k[..., cuts[i]:cuts[i + 1]] = torch.fft.fftshift(torch.fft.fft(moved, dim=-1), dim=-1)[..., cuts[i]:cuts[i + 1]]
            out.append(torch.fft.ifft(torch.fft.ifftshift(k, dim=-1), dim=-1).real)
        return torch.stack(out)

    def chain(self, A, B, seg, noise):
        x, lab = self.spatial(torch.stack([A, B]), seg)
        x = self.motion(self.intensity(self.blur(x), noise))
        win = tuple(slice(s, s + CROP) for s in self.p["crop_start"])
        x, lab = x[(slice(None),) + win], lab[win].float()[None].contiguous()
        return x[0][None].contiguous(), x[1][None].contiguous(), lab, lab.clone()


class HipStages:
    """The stages of augment_pair one by one (the same private calls, in its order)."""

    def __init__(self, p, dev):
        self.p, self.t = p, G.build_table(p).device(dev)

    def spatial(self, x, lab):
        return G._spatial(x, lab, self.t, G._minmax(x))

    def blur(self, x):
        return G._blur(x, self.t)

    def intensity(self, x, noise):
        return G._intensity(x, noise, torch.empty_like(x), self.t)

    def motion(self, x):
        return torch.stack([G._motion_one(x[v], r["motion_degrees"], r["motion_translation"], r["motion_times"]) for v, r in enumerate(self.p["views"])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_augment.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    a, lab = PR.blob_volume(VOL, 300)
    b, _ = PR.blob_volume(VOL, 301)
    A, B = torch.from_numpy(a.astype(np.float32)).to(dev), torch.from_numpy((0.5 * a + 0.7 * b).astype(np.float32)).to(dev)
    seg = torch.from_numpy(lab.astype(np.uint8)).to(dev)
    from argparse import Namespace
    p = G.draw_params(np.random.RandomState(0), VOL, Namespace(crop_size=CROP, isTrain=True))
    p["flip_on"], p["flip_axes"], p["affine_on"] = True, np.array([True, False, True]), True
    p["map"] = G.spatial_map(VOL, p["flip_axes"], p["scales"], p["degrees"])
    for rec in p["views"]:
        rec["on"] = dict.fromkeys(rec["on"], True)
    p["views"][0]["sigma"] = np.array([2.0, 2.0, 2.0])                           # the full radius of 8 on every axis
    noise = torch.stack([torch.randn(VOL, generator=torch.Generator(dev).manual_seed(r["noise_seed"]), device=dev) for r in p["views"]])
    tr, hs = TorchRoute(p, dev), HipStages(p, dev)
    V = int(np.prod(VOL))
    res = {"volume": list(VOL), "crop": CROP, "views": 2, "warmup": WARMUP, "timed": TIMED, "device": torch.cuda.get_device_name(0),
           "sigma": [r["sigma"].tolist() for r in p["views"]]}

    # the whole pair, both routes
    t = timed({"hip": lambda: G.augment_pair(A, B, seg, p, crop_size=CROP, noise=noise), "torch": lambda: tr.chain(A, B, seg, noise)})
    res["pair"] = {k: stats(v) for k, v in t.items()}
    x, y = G.augment_pair(A, B, seg, p, crop_size=CROP, noise=noise), tr.chain(A, B, seg, noise)
    res["pair"]["max_abs_image_difference"] = float(max((x[0] - y[0]).abs().max(), (x[1] - y[1]).abs().max()))
    res["pair"]["max_abs_image"] = float(max(x[0].abs().max(), x[1].abs().max()))
    res["pair"]["label_disagreement_share"] = float((x[2] != y[2]).float().mean())
    del x, y

    # per stage, on the hip route's intermediates
    x0 = torch.stack([A, B])
    x1, y1 = hs.spatial(x0, seg)
    x2 = hs.blur(x1)
    x3 = hs.intensity(x2, noise)
    stage_args = {"spatial": (x0, seg), "blur": (x1,), "intensity": (x2, noise), "motion": (x3,)}
    res["stages"] = {}
    for name, sargs in stage_args.items():
        t = timed({"hip": lambda: getattr(hs, name)(*sargs), "torch": lambda: getattr(tr, name)(*sargs)})
        s = res["stages"][name] = {k: stats(v) for k, v in t.items()}
        d = (getattr(hs, name)(*sargs), getattr(tr, name)(*sargs))
        d = [o[0] if isinstance(o, tuple) else o for o in d]
        s["max_abs_difference"] = float((d[0] - d[1]).abs().max())
        if name in STAGE_BYTES:
            s["bytes_per_voxel_and_view"] = STAGE_BYTES[name]
            for k in ("hip", "torch"):
                s[k + "_gbps"] = STAGE_BYTES[name] * 2 * V / (s[k]["median_ms"] * 1e-3) / 1e9
    res["stages"]["motion"]["note"] = "torch.fft on both routes; the rigid moves are the spatial kernel on the hip route, grid_sample on the other"
    t = timed({"minmax": lambda: G._minmax(x0)})
    res["stages"]["minmax_of_the_pad_value"] = stats(t["minmax"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
