"""Times registration stage 1 at the registration size (256^3 pair: 28 x 128^3 pooled features, grid_sp 2, disp_hw 1, inverse
consistency on and off):

  (i)  run_stage1_registration of this package (one amx_stage1_registration call) and each kernel group of it, and
  (ii) the same stage written here as plain torch ops on the same device tensors, fp32 -- the op-by-op composition a user
       would otherwise run, with the per-slice Python loop of the solver ("torch_slices"), and additionally with that loop
       replaced by whole-volume ops ("torch_volume"), which is the most a user gets out of stock ops,

in one process, alternating, after warm-up, device-synchronised (device events around every call), >= 20 repetitions each;
median and spread.  Needs a GPU.  Writes a JSON report (default profiles/regsolve_bench.json) and prints the DESIGN §4.7
rows: time, algorithmic bytes from the shapes, achieved TB/s.

    python tools/regsolve_bench.py [--reps 20] [--warmup 3] [--grid 128] [--out profiles/regsolve_bench.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COEFFS = (0.003, 0.01, 0.03, 0.1, 0.3, 1.0)
HBM_TBS = 8.0


# ---- (ii) the stage as stock torch ops ----------------------------------------------------------------------------------

def t_mesh(hw, dev):
    k = 2 * hw + 1
    m = torch.arange(k ** 3, device=dev)
    return torch.stack([m % k - hw, (m // k) % k - hw, m // (k * k) - hw]).float()


def t_correlate(fix, mov, hw):
    c, h, w, d = fix.shape[1:]
    k = 2 * hw + 1
    pad = F.pad(mov[0], (hw,) * 6)
    ssd = torch.empty((k ** 3, h, w, d), device=fix.device)
    for dz in range(k):
        for dy in range(k):
            for dx in range(k):
                ssd[(dx * k + dy) * k + dz] = (fix[0] - pad[:, dz:dz + h, dy:dy + w, dx:dx + d]).pow(2).sum(0)
    ssd = F.avg_pool3d(F.avg_pool3d(ssd[None], 3, 1, 1), 3, 1, 1)[0]
    return ssd, ssd.argmin(0)


def t_coupled(ssd, amin, mesh, slices):
    n, h, w, d = ssd.shape
    cost = ssd                                            # accumulated in place, like the solver this replaces

    def soften(lab):
        return F.avg_pool3d(mesh[:, lab.reshape(-1)].view(1, 3, h, w, d), 3, 1, 1)
    soft = soften(amin)
    for c in COEFFS:
        if slices:
            lab = torch.empty_like(amin)
            for i in range(h):
                cost[:, i] += c * (mesh.view(3, n, 1, 1) - soft[0, :, i].unsqueeze(1)).pow(2).sum(0)
                lab[i] = cost[:, i].argmin(0)
        else:
            cost += c * (mesh.view(3, n, 1, 1, 1) - soft[0].unsqueeze(1)).pow(2).sum(0)
            lab = cost.argmin(0)
        soft = soften(lab)
    return soft


def t_consistency(a, b, iterations):
    _, _, h, w, d = a.shape
    ident = F.affine_grid(torch.eye(3, 4, device=a.device)[None], (1, 1, h, w, d), align_corners=False)
    for _ in range(iterations):
        na = 0.5 * (a - F.grid_sample(b, ident + a.permute(0, 2, 3, 4, 1), align_corners=False))
        nb = 0.5 * (b - F.grid_sample(a, ident + b.permute(0, 2, 3, 4, 1), align_corners=False))
        a, b = na, nb
    return a, b


def t_stage1(fix, mov, hw, g, sizes, ic, slices):
    mesh = t_mesh(hw, fix.device)
    ssd, amin = t_correlate(fix, mov, hw)
    soft = t_coupled(ssd, amin, mesh, slices)
    if not ic:
        return soft
    ssd, amin = t_correlate(mov, fix, hw)
    soft_ = t_coupled(ssd, amin, mesh, slices)
    h, w, d = soft.shape[2:]
    scale = torch.tensor([h - 1, w - 1, d - 1], device=fix.device, dtype=torch.float32).view(1, 3, 1, 1, 1) / 2
    ice, _ = t_consistency((soft / scale).flip(1), (soft_ / scale).flip(1), 15)
    return F.interpolate(ice.flip(1) * scale * g, size=sizes, mode="trilinear", align_corners=False)


# ---- timing ---------------------------------------------------------------------------------------------------------------

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    s = sorted(ms)
    n = len(s)
    return {"median_ms": s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2]), "min_ms": s[0], "max_ms": s[-1],
            "spread_ms": s[-1] - s[0], "reps": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--channels", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regsolve_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regsolve_bench needs a GPU: a timing taken anywhere else says nothing about this stage")
    from anatomix_amd.registration import (correlate, coupled_convex, inverse_consistency, resize_trilinear,
                                           run_stage1_registration)
    dev = torch.device("cuda:0")
    hw, g, n = 1, 2, args.grid
    sizes = (n * g,) * 3
    torch.manual_seed(0)
    base = torch.rand(1, args.channels, n, n, n, device=dev)
    fix = F.avg_pool3d(base, 3, 1, 1)
    mov = torch.roll(fix, (1, 0, -1), (2, 3, 4)) + 0.01 * torch.randn_like(fix)
    del base
    mesh = t_mesh(hw, dev).view(3, -1, 1)

    # the two sides compute the same thing (checked once, on the interior where nothing depends on near-ties at the border)
    ours = run_stage1_registration(fix, mov, hw, g, sizes, args.channels, True)
    theirs = t_stage1(fix, mov, hw, g, sizes, True, False)
    agree = float(((ours - theirs).abs().amax(1) <= 1e-3).float().mean())
    print(f"amx vs torch composition: {agree:.6f} of the output voxels agree within 1e-3 voxel")
    del ours, theirs

    runs = {}
    for ic in (True, False):
        tag = "ic" if ic else "noic"
        runs[f"amx_stage1_{tag}"] = lambda ic=ic: run_stage1_registration(fix, mov, hw, g, sizes, args.channels, ic)
        runs[f"torch_slices_{tag}"] = lambda ic=ic: t_stage1(fix, mov, hw, g, sizes, ic, True)
        runs[f"torch_volume_{tag}"] = lambda ic=ic: t_stage1(fix, mov, hw, g, sizes, ic, False)
    # the kernel groups of amx_stage1_registration, one by one through the Python surface
    ssd, amin = correlate(fix, mov, hw, g, sizes, args.channels)
    soft = coupled_convex(ssd, amin, mesh, g, sizes)
    scale = torch.tensor([n - 1] * 3, device=dev, dtype=torch.float32).view(1, 3, 1, 1, 1) / 2
    na = (soft / scale).flip(1).contiguous()
    nb = (-soft / scale).flip(1).contiguous()
    ice, _ = inverse_consistency(na, nb, 15)
    up = [float(v) for v in (scale.view(-1) * g)]
    runs["amx_correlate"] = lambda: correlate(fix, mov, hw, g, sizes, args.channels)
    runs["amx_coupled_convex"] = lambda: coupled_convex(ssd, amin, mesh, g, sizes)
    runs["amx_inverse_consistency_15"] = lambda: inverse_consistency(na, nb, 15)
    runs["amx_resize_trilinear"] = lambda: resize_trilinear(ice, sizes, up, True)
    runs["torch_coupled_slices"] = lambda: t_coupled(ssd.clone(), amin, mesh.view(3, -1), True)
    runs["torch_coupled_volume"] = lambda: t_coupled(ssd.clone(), amin, mesh.view(3, -1), False)
    runs["torch_inverse_consistency_15"] = lambda: t_consistency(na, nb, 15)
    runs["torch_interpolate"] = lambda: F.interpolate(ice.flip(1) * scale * g, size=sizes, mode="trilinear", align_corners=False)

    times = {k: [] for k in runs}
    for _ in range(args.warmup):
        for k, fn in runs.items():
            timed(fn)
    for _ in range(args.reps):                              # alternating: every repetition visits every variant once
        for k, fn in runs.items():
            times[k].append(timed(fn)[0])

    plane, labels = n ** 3, (2 * hw + 1) ** 3
    out_vox = sizes[0] * sizes[1] * sizes[2]
    bytes_ = {
        # ssd read in each of the six coupled iterations (iteration 0 reads the argmin), the soft fields kept so far, the raw
        # label field written and read by the box filter, the soft field written
        "amx_coupled_convex": 4 * plane * (6 * labels + sum(3 * j for j in range(1, 7)) + 7 * 9) + 8 * plane,
        # per sweep and field: own 3 channels, about one pass over the other field's 3 channels, 3 channels written
        "amx_inverse_consistency_15": 15 * 2 * 9 * 4 * plane,
        "amx_resize_trilinear": 4 * 3 * (plane + out_vox),
        # raw SSD: both feature sets read, volume written; two box passes read + write it; argmin reads it
        "amx_correlate": 4 * plane * (2 * args.channels + labels * 6) + 8 * plane,
    }
    report = {"device": torch.cuda.get_device_name(0), "grid": [n] * 3, "sizes": list(sizes), "channels": args.channels,
              "disp_hw": hw, "grid_sp": g, "agreement_within_1e-3_voxel": agree, "timings": {}, "acceptance": {}}
    for k, ms in times.items():
        st = stats(ms)
        if k in bytes_:
            st["algorithmic_bytes"] = bytes_[k]
            st["achieved_TBps"] = bytes_[k] / (st["median_ms"] * 1e-3) / 1e12
        report["timings"][k] = st
    for tag in ("ic", "noic"):
        a, t = report["timings"][f"amx_stage1_{tag}"], report["timings"][f"torch_slices_{tag}"]
        v = report["timings"][f"torch_volume_{tag}"]
        report["acceptance"][tag] = {
            "amx_median_ms": a["median_ms"], "torch_slices_median_ms": t["median_ms"], "torch_slices_spread_ms": t["spread_ms"],
            "torch_volume_median_ms": v["median_ms"], "torch_volume_spread_ms": v["spread_ms"],
            "faster_than_slices_by_more_than_its_spread": t["median_ms"] - a["median_ms"] > t["spread_ms"],
            "faster_than_volume_by_more_than_its_spread": v["median_ms"] - a["median_ms"] > v["spread_ms"],
            "speedup_vs_slices": t["median_ms"] / a["median_ms"], "speedup_vs_volume": v["median_ms"] / a["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    for k, st in report["timings"].items():
        extra = f"  {st['algorithmic_bytes'] / 1e6:8.0f} MB  {st['achieved_TBps']:.2f} TB/s of {HBM_TBS}" if "achieved_TBps" in st else ""
        print(f"{k:32s} median {st['median_ms']:9.3f} ms  min {st['min_ms']:9.3f}  max {st['max_ms']:9.3f}{extra}")
    print(json.dumps(report["acceptance"]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
