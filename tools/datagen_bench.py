"""Times step 2 of the synthetic data generation at the reference's shape: 8 label maps of 128^3, two views
each, every switch on, uint8 out.

    python tools/datagen_bench.py [--out profiles/datagen.json]

In one process, the routes alternating, 3 warm-up + 10 timed repetitions each, timed with device events:
  * ``hip``    anatomix_amd.datagen.views.generate_views (csrc/amx_synth.hip and csrc/amx_segaug.hip; the forward FFT of the spike and
               the two FFTs of Gibbs are torch.fft);
  * ``torch``  the same definitions composed from stock torch ops on the same device (gather, F.interpolate, fftn / ifftn, F.conv3d);
  * every stage of the hip route alone, on the route's own intermediates, and the new stages on the torch route as well;
  * ``copy``   a float32 copy of the batch's size, the streaming rate tools/bw_probe.py measures, for the bytes/s beside it.
It records medians with min and max, pairs per second, per kernel stage its algorithmic bytes per view voxel and the achieved GB/s on
them, and the largest difference between the two routes' outputs."""
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
import _datagen_ref as DR                                   # noqa: E402
import _segaug_ref as AR                                    # noqa: E402
from anatomix_amd.datagen import views as V                 # noqa: E402
from anatomix_amd.segmentation import augment as SA         # noqa: E402

B, N, SCALES = 8, 128, (4, 8, 16, 32)
SHAPE = (N, N, N)
R = 2 * B
# bytes per view voxel that each kernel stage has to move at least once (fp32 views, uint8 labels shared by the two views of a sample;
# the coarse grids are 1/64 of a volume and less and are left out)
STAGE_BYTES = {"gmm_minmax": 4 + 0.5, "appearance": 4 + 0.5 + 4, "rescale": 8, "bias": 4 + 1 + 4 + 1, "spike_logk": 8, "spike_wave": 8,
               "contrast": 4 + 8, "smooth": 3 * 8, "sharpen": 5 * 8 + 12, "lowres": 8, "tail_u8": 4 + 4 + 1}


class TorchRoute:
    """The definitions from stock torch ops, every switch on; rows [R, 1, D, H, W]."""

    def __init__(self, p, lab, dev):
        f = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=dev)      # noqa: E731
        self.p, self.dev = p, dev
        mean, std = torch.zeros((R, 256), device=dev), torch.zeros((R, 256), device=dev)
        for b in range(B):
            u = p["unique_labels"][b]
            for v in range(2):
                mean[2 * b + v, u], std[2 * b + v, u] = f(p["means"][b][v]), f(p["stds"][b][v])
                if p["zero_background"][b, v]:
                    mean[2 * b + v, u[0]] = std[2 * b + v, u[0]] = 0
        self.mean, self.std = mean, std
        self.lab = lab.view(B, -1).long().repeat_interleave(2, 0)                 # [R, V] indices, made once
        r5 = lambda a: f(a).reshape(R, 1, 1, 1, 1)                                # noqa: E731
        self.coeff, self.gamma, self.alpha, self.factor = f(p["coeff"]).reshape(R, 20), r5(p["gamma"]), r5(p["sharpen_alpha"]), f(p["spike_factor"]).reshape(R)
        self.taps = {k: self._taps(np.asarray(p[k]).reshape(R, 3)) for k in ("smooth_sigma", "sharpen_sigma1", "sharpen_sigma2")}
        self.P = [torch.ones(N, device=dev), torch.linspace(-1, 1, N, device=dev)]
        x = self.P[1]
        self.P += [(3 * x * x - 1) / 2, (5 * x * x * x - 3 * x) / 2]
        self.loc = np.asarray(p["spike_loc"]).reshape(R, 3)
        self.low = [V.low_resolution_shape(SHAPE, z) for z in np.asarray(p["zoom"]).reshape(R)]

    def _taps(self, sig):
        w = torch.zeros((R, 3, 9))
        for r in range(R):
            for a in range(3):
                rad, t = SA.gaussian_taps(sig[r][a])
                w[r, a, 4 - rad:4 + rad + 1] = torch.tensor(t, dtype=torch.float32)
        return w.to(self.dev)

    @staticmethod
    def rescale(x):
        mn, mx = x.amin((1, 2, 3, 4), keepdim=True), x.amax((1, 2, 3, 4), keepdim=True)
        return (x - mn) / (mx - mn)

    def appearance(self, z, grids):
        g = torch.clamp(self.std.gather(1, self.lab) * z.view(R, -1) + self.mean.gather(1, self.lab), min=0).view(R, 1, *SHAPE)
        P = sum(F.interpolate(c.view(R, 1, *c.shape[2:]), scale_factor=s, mode="trilinear") for s, c in zip(SCALES, grids))
        return self.rescale(g) * (1 + self.p["perl_mult_factor"] * P)

    def bias(self, x):
        f = torch.zeros_like(x)
        for q, (i, j, k) in enumerate(AR.coeff_index()):
            f = f + self.coeff[:, q].view(R, 1, 1, 1, 1) * (self.P[i].view(-1, 1, 1) * self.P[j].view(1, -1, 1) * self.P[k].view(1, 1, -1))
        return x * torch.exp(f)

    def spike(self, x):
        dims = (-3, -2, -1)
        k = torch.fft.fftshift(torch.fft.fftn(x, dim=dims), dim=dims)
        log_abs, phase = torch.log(k.abs() + 1e-10), torch.angle(k)
        k_int = self.factor * 2.5 * log_abs.mean((1, 2, 3, 4))
        idx = (torch.arange(R, device=self.dev), 0, *[torch.as_tensor(self.loc[:, a], device=self.dev) for a in range(3)])
        log_abs[idx] = k_int
        k = torch.exp(log_abs) * torch.exp(1j * phase)
        return torch.fft.ifftn(torch.fft.ifftshift(k, dim=dims), dim=dims).real

    def contrast(self, x):
        mn, mx = x.amin((1, 2, 3, 4), keepdim=True), x.amax((1, 2, 3, 4), keepdim=True)
        return ((x - mn) / (mx - mn + 1e-7)) ** self.gamma * (mx - mn) + mn

    def _gauss(self, x, taps):
        x = x.view(1, R, *SHAPE)
        x = F.conv3d(x, taps[:, 2].reshape(R, 1, 1, 1, 9), padding=(0, 0, 4), groups=R)
        x = F.conv3d(x, taps[:, 1].reshape(R, 1, 1, 9, 1), padding=(0, 4, 0), groups=R)
        x = F.conv3d(x, taps[:, 0].reshape(R, 1, 9, 1, 1), padding=(4, 0, 0), groups=R)
        return x.view(R, 1, *SHAPE)

    def smooth(self, x):
        return self._gauss(x, self.taps["smooth_sigma"])

    def sharpen(self, x):
        b = self._gauss(x, self.taps["sharpen_sigma1"])
        return b + self.alpha * (b - self._gauss(b, self.taps["sharpen_sigma2"]))

    def lowres(self, x):
        return torch.cat([F.interpolate(F.interpolate(x[r:r + 1], size=self.low[r], mode="nearest-exact"), size=SHAPE, mode="trilinear",
                                        align_corners=False) for r in range(R)])

    def tail_u8(self, x):
        return (self.rescale(torch.clamp(x, min=0)) * 255).to(torch.uint8)

    def chain(self, z, grids, seg):
        x = self.rescale(self.appearance(z, grids))
        x = self.contrast(self.spike(self.bias(x)))
        x = SA._gibbs(self.smooth(x).contiguous(), list(range(R)), seg)
        return self.tail_u8(self.lowres(self.sharpen(x))).view(B, 2, *SHAPE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datagen.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = V._lib.load()
    labels = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 255]
    lab = torch.from_numpy(np.stack([DR.label_blobs(SHAPE, labels, 500 + b) for b in range(B)])[:, None]).to(dev)
    p = V.draw_params(np.random.RandomState(0), [np.array(labels)] * B, SHAPE, scales=SCALES)
    for k in p["on"]:
        p["on"][k][:] = True
    z, grids = V.draw_fields(p, dev)
    res = {"labels": [B, 1, N, N, N], "views": [B, 2, N, N, N], "scales": list(SCALES), "warmup": WARMUP, "timed": TIMED,
           "device": torch.cuda.get_device_name(0)}
    vox = R * N ** 3

    # the hip route's tables and intermediates, stage by stage (the private calls of generate_views, in its order)
    syn = V._appearance_table(p, B)
    seg, chain, on = V._chain_tables(p, R, SHAPE)
    for k in ("flags", "spike_loc", "spike_factor", "spike_slot", "lowres"):
        syn.host[k] = syn.host[k] | chain.host[k] if k == "flags" else chain.host[k]
    syn.device(dev)
    zr, gr = z.view(R, 1, *SHAPE), [g.view(R, 1, *g.shape[2:]) for g in grids]
    x0, sc, nb = V._appearance(lab, p, zr, gr, syn)
    x0 = x0.view(R, 1, *SHAPE)
    dummy = torch.zeros((R, N ** 3), dtype=torch.uint8, device=dev)
    for r in range(R):
        seg.host["vol"][r], seg.host["lab"][r] = x0[r].data_ptr(), dummy[r].data_ptr()
    seg.device(dev)
    tr = TorchRoute(p, lab, dev)

    t = timed({"hip": lambda: V.generate_views(lab, p, noise=z, grids=grids), "torch": lambda: tr.chain(z, grids, seg)})
    res["chain"] = {k: stats(v) for k, v in t.items()}
    for k in ("hip", "torch"):
        res["chain"][k]["pairs_per_s"] = B / (res["chain"][k]["median_ms"] * 1e-3)
    a, b = V.generate_views(lab, p, noise=z, grids=grids), tr.chain(z, grids, seg)
    d = (a.int() - b.int()).abs()
    res["chain"]["uint8_max_difference"], res["chain"]["uint8_share_different"] = int(d.max()), float((d > 0).float().mean())

    st = V._lib.stream(dev)

    def gmm_minmax():
        V._lib.check_envelope(lib.amx_synth_gmm_minmax(V._lib.ptr(lab), V._lib.ptr(zr), B, N ** 3, *syn.args, V._lib.ptr(sc), nb, st))
    mm0 = V._finalize(sc, nb, R, N ** 3, dev)
    gp = (V.ctypes.c_void_p * len(gr))(*[g.data_ptr() for g in gr])
    scl = (V.ctypes.c_int * len(gr))(*SCALES)
    buf = torch.empty_like(x0)

    def appearance():
        V._lib.check_envelope(lib.amx_synth_appearance(V._lib.ptr(lab), V._lib.ptr(zr), gp, scl, len(gr), V._lib.ptr(mm0), V._lib.ptr(buf), B, *SHAPE,
                              *syn.args, V._lib.ptr(sc), nb, st))
    gmm_minmax()
    mm0 = V._finalize(sc, nb, R, N ** 3, dev)
    x1 = SA._pointwise(x0, torch.empty_like(x0), SA._minmax(x0), SA._OP_SCALE, seg)
    for r in range(R):
        seg.host["vol"][r] = x1[r].data_ptr()
    seg.device(dev)
    x2 = SA._crop(seg, R, SHAPE, None, torch.uint8, dev)[0]
    k2 = torch.view_as_real(torch.fft.fftn(x2[:, 0], dim=(-3, -2, -1)).contiguous())
    mean = torch.empty(R, dtype=torch.float32, device=dev)

    def spike_logk():
        V._lib.check_envelope(lib.amx_synth_logk_mean(V._lib.ptr(k2), R, N ** 3, V._lib.ptr(mean), V._lib.ptr(sc), nb, st))
    spike_logk()
    x3 = x2.clone()

    def spike_wave():
        V._lib.check_envelope(lib.amx_synth_spike(V._lib.ptr(x3), V._lib.ptr(k2), R, V._lib.ptr(mean), R, *SHAPE, *syn.args, st))
    x4 = SA._pointwise(x3, torch.empty_like(x3), SA._minmax(x3), SA._OP_CONTRAST, seg)
    x5 = SA._gaussian(x4, SA._GAUSS_SMOOTH, seg)
    x6 = SA._gibbs(x5.clone(), list(range(R)), seg)
    x7 = SA._gaussian(x6, SA._GAUSS_SHARPEN, seg)
    x8 = V._lowres(x7, syn)
    hip = {"gmm_minmax": gmm_minmax, "appearance": appearance,
           "rescale": lambda: SA._pointwise(x0, buf, mm0, SA._OP_SCALE, seg),
           "bias": lambda: SA._crop(seg, R, SHAPE, None, torch.uint8, dev),
           "spike_logk": spike_logk, "spike_wave": spike_wave,
           "contrast": lambda: SA._pointwise(x3, buf, SA._minmax(x3), SA._OP_CONTRAST, seg),
           "smooth": lambda: SA._gaussian(x4, SA._GAUSS_SMOOTH, seg), "sharpen": lambda: SA._gaussian(x6, SA._GAUSS_SHARPEN, seg),
           "lowres": lambda: V._lowres(x7, syn), "tail_u8": lambda: V._tail(x8, torch.uint8)}
    res["stages"] = {}
    for name, fn in hip.items():
        s = stats(timed({name: fn})[name])
        s["bytes_per_voxel"] = STAGE_BYTES[name]
        s["gbps"] = STAGE_BYTES[name] * vox / (s["median_ms"] * 1e-3) / 1e9
        res["stages"][name] = {"hip": s}
    fft = timed({"spike_fft": lambda: torch.fft.fftn(x2[:, 0], dim=(-3, -2, -1)), "gibbs": lambda: SA._gibbs(x5.clone(), list(range(R)), seg)})
    res["stages"]["spike_forward_fft_torch"] = stats(fft["spike_fft"])
    res["stages"]["gibbs_torch_fft_both_routes"] = stats(fft["gibbs"])
    tor = {"appearance": lambda: tr.appearance(z, grids), "spike": lambda: tr.spike(x2), "lowres": lambda: tr.lowres(x7), "tail_u8": lambda: tr.tail_u8(x8),
           "bias": lambda: tr.bias(x1), "contrast": lambda: tr.contrast(x3), "smooth": lambda: tr.smooth(x4), "sharpen": lambda: tr.sharpen(x6)}
    for name, fn in tor.items():
        res["stages"].setdefault(name, {})["torch"] = stats(timed({name: fn})[name])
    src, dst = torch.empty(vox, dtype=torch.float32, device=dev), torch.empty(vox, dtype=torch.float32, device=dev)
    c = stats(timed({"copy": lambda: dst.copy_(src)})["copy"])
    c["gbps"] = 8 * vox / (c["median_ms"] * 1e-3) / 1e9
    res["copy_fp32"] = c
    kernel_ms = sum(res["stages"][k]["hip"]["median_ms"] for k in STAGE_BYTES)
    res["chain"]["algorithmic_bytes"] = sum(STAGE_BYTES.values()) * vox
    res["chain"]["hip_kernel_stages_ms"] = kernel_ms
    res["chain"]["hip_kernel_stages_gbps"] = res["chain"]["algorithmic_bytes"] / (kernel_ms * 1e-3) / 1e9
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
