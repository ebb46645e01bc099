"""Times registration stage 2 (the Adam instance optimisation) at the reference pipeline's own shape: a 256^3 pair, 28 channels,
grid_sp_adam 2 (a 128^3 grid), 80 iterations, selected_smooth 0:

  (i)  run_instance_opt of this package (one amx_run_instance_opt call) and its kernel groups, and
  (ii) the same loop written here from stock torch ops with autograd and torch.optim.Adam on the same device tensors -- the
       composition a user would otherwise run.  It is the yardstick, never the code under test,

in one process, alternating, after warm-up, device-synchronised (device events around every call), >= 20 repetitions each;
median and spread.  Also the A/B of the fused smoothing (instopt_smooth3, one launch) against three amx_box_filter3d
launches at 3 x grid^3.  Needs a GPU.  Writes a JSON report (default profiles/instopt_bench.json) and prints the DESIGN 4.7
rows: time, algorithmic bytes from the shapes, achieved TB/s.

    python tools/instopt_bench.py [--reps 20] [--warmup 3] [--grid 128] [--niter 80] [--out profiles/instopt_bench.json]
    python tools/instopt_bench.py --trace-run      # ONE run_instance_opt call and nothing else: for a kernel trace
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
LAUNCHES_PER_ITERATION = 4                  # smooth, sample + grad, smooth, update (csrc/amx_reginstopt.hip launch_instopt)
LAMBDA = 0.75


# ---- (ii) the stage as stock torch ops ----------------------------------------------------------------------------------

def t_smooth3(x, k=3):
    for _ in range(3):
        x = F.avg_pool3d(x, k, stride=1, padding=k // 2)
    return x


def t_run_instance_opt(disp_hr, feat_fix, feat_mov, g, lam, sizes, niter, smooth, lr=1.0):
    H, W, D = sizes
    h, w, d = H // g, W // g, D // g
    dev = disp_hr.device
    with torch.no_grad():
        pf, pm = F.avg_pool3d(feat_fix, g, stride=g), F.avg_pool3d(feat_mov, g, stride=g)
        w0 = F.interpolate(disp_hr, size=(h, w, d), mode="trilinear", align_corners=False) / g
    weight = torch.nn.Parameter(w0)
    opt = torch.optim.Adam([weight], lr=lr)
    scale = torch.tensor([(h - 1) / 2, (w - 1) / 2, (d - 1) / 2], device=dev).unsqueeze(0)
    for _ in range(niter):
        opt.zero_grad()
        ds = t_smooth3(weight).permute(0, 2, 3, 4, 1)
        reg = lam * (((ds[0, :, 1:, :] - ds[0, :, :-1, :]) ** 2).mean() + ((ds[0, 1:, :, :] - ds[0, :-1, :, :]) ** 2).mean()
                     + ((ds[0, :, :, 1:] - ds[0, :, :, :-1]) ** 2).mean())
        grid0 = F.affine_grid(torch.eye(3, 4, device=dev).unsqueeze(0), (1, 1, h, w, d), align_corners=False)
        grid = grid0.view(-1, 3) + (ds.reshape(-1, 3) / scale).flip(1)
        sampled = F.grid_sample(pm, grid.view(1, h, w, d, 3), align_corners=False, mode="bilinear")
        loss = ((sampled - pf).pow(2).mean(1) * 12).mean()
        (loss + reg).backward()
        opt.step()
    out = F.interpolate(ds.detach().permute(0, 4, 1, 2, 3) * g, size=(H, W, D), mode="trilinear", align_corners=False)
    return t_smooth3(out, smooth) if smooth in (3, 5) else out


def t_warp(vol, disp, mode):
    H, W, D = vol.shape[2:]
    grid1 = F.affine_grid(torch.eye(3, 4, device=vol.device).unsqueeze(0), (1, 1, H, W, D), align_corners=False)
    denom = torch.tensor([H - 1, W - 1, D - 1], device=vol.device).view(1, 1, 1, 1, 3)
    return F.grid_sample(vol, grid1 + (disp.permute(0, 2, 3, 4, 1) / denom * 2).flip(4), align_corners=False, mode=mode)


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


def smooth_noise(shape, dev, passes):
    x = torch.rand(shape, device=dev)
    for _ in range(passes):
        x = F.avg_pool3d(x, 3, 1, 1)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--channels", type=int, default=28)
    ap.add_argument("--niter", type=int, default=80)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "instopt_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("instopt_bench needs a GPU: a timing taken anywhere else says nothing about this stage")
    from anatomix_amd.registration import (apply_avg_pool3d, instance_opt, instance_opt_adam_step, instance_opt_grad,
                                           instance_opt_smooth3, resize_trilinear, run_instance_opt, smooth_merged_features,
                                           warp_volume)
    dev = torch.device("cuda:0")
    g, n, c, niter = 2, args.grid, args.channels, args.niter
    sizes = (n * g,) * 3
    torch.manual_seed(0)
    fix = smooth_noise((1, c) + sizes, dev, 2)
    mov = torch.roll(fix, (1, -1, 2), (2, 3, 4)) + 0.05 * smooth_noise((1, c) + sizes, dev, 2)
    disp = (smooth_noise((1, 3) + sizes, dev, 3) - 0.5) * 6.0

    if args.trace_run:
        run_instance_opt(disp, fix, mov, g, LAMBDA, sizes, niter, 0)
        torch.cuda.synchronize()
        print(f"one run_instance_opt call, niter {niter}: expect 2 pooling + 1 resize + {niter - 1} x {LAUNCHES_PER_ITERATION} + 1 smooth "
              f"+ 1 resize = {5 + (niter - 1) * LAUNCHES_PER_ITERATION} kernel launches of this package")
        return

    # the two sides compute the same thing (checked once on a short trajectory, where fp32 rounding has not yet been amplified)
    ours, theirs = run_instance_opt(disp, fix, mov, g, LAMBDA, sizes, 5, 0), t_run_instance_opt(disp, fix, mov, g, LAMBDA, sizes, 5, 0)
    agree = float((ours - theirs).abs().max() / theirs.abs().max())
    print(f"amx vs torch composition after 5 iterations: max abs difference {agree:.3e} of max|field|")
    del ours, theirs

    pf, pm = smooth_merged_features(None, fix, g, 1.0), smooth_merged_features(None, mov, g, 1.0)
    w0 = resize_trilinear(disp, (n, n, n), [1.0 / g] * 3)
    grad, ds, _, _ = instance_opt_grad(w0, pf, pm, LAMBDA)
    m, v, wa = torch.zeros_like(w0), torch.zeros_like(w0), w0.clone()
    vol = fix[:, :1].contiguous()
    runs = {
        "amx_run_instance_opt": lambda: run_instance_opt(disp, fix, mov, g, LAMBDA, sizes, niter, 0),
        "torch_run_instance_opt": lambda: t_run_instance_opt(disp, fix, mov, g, LAMBDA, sizes, niter, 0),
        "amx_loop_only": lambda: instance_opt(w0, pf, pm, LAMBDA, niter),
        "amx_pooling_both": lambda: (smooth_merged_features(None, fix, g, 1.0), smooth_merged_features(None, mov, g, 1.0)),
        "amx_smooth3_fused": lambda: instance_opt_smooth3(w0),
        "amx_smooth3_three_box_launches": lambda: apply_avg_pool3d(w0, 3, 3),
        "amx_grad_one_iteration_with_loss": lambda: instance_opt_grad(w0, pf, pm, LAMBDA),
        "amx_adam_step": lambda: instance_opt_adam_step(wa, grad, m, v, 3),
        "amx_resize_up": lambda: resize_trilinear(ds, sizes, [float(g)] * 3),
        "amx_warp_bilinear": lambda: warp_volume(vol, disp),
        "amx_warp_nearest": lambda: warp_volume(vol, disp, "nearest"),
        "torch_warp_bilinear": lambda: t_warp(vol, disp, "bilinear"),
        "torch_warp_nearest": lambda: t_warp(vol, disp, "nearest"),
    }
    times = {k: [] for k in runs}
    for _ in range(args.warmup):
        for k, fn in runs.items():
            timed(fn)
    for _ in range(args.reps):                              # alternating: every repetition visits every variant once
        for k, fn in runs.items():
            times[k].append(timed(fn)[0])

    plane, full = n ** 3, sizes[0] * sizes[1] * sizes[2]
    bytes_ = {
        "amx_smooth3_fused": 4 * 3 * plane * 2,                              # the field read and written once
        "amx_smooth3_three_box_launches": 4 * 3 * plane * 2 * 3,
        "amx_adam_step": 4 * 3 * plane * 7,                                  # p, g, m, v read; p, m, v written
        "amx_pooling_both": 2 * 4 * c * (full + plane),
        "amx_resize_up": 4 * 3 * (plane + full),
        "amx_warp_bilinear": 4 * (3 + 1 + 1) * full,
        "amx_warp_nearest": 4 * (3 + 1 + 1) * full,
        # sample + grad: disp_sample read, both feature sets read about once (the gathers of a wave overlap), the gradient written;
        # two smooths around it
        "amx_grad_one_iteration_with_loss": 4 * plane * (2 * c + 6) + 2 * 4 * 3 * plane * 2,
    }
    report = {"device": torch.cuda.get_device_name(0), "grid": [n] * 3, "sizes": list(sizes), "channels": c, "grid_sp_adam": g,
              "niter": niter, "lambda": LAMBDA, "selected_smooth": 0, "launches_per_iteration": LAUNCHES_PER_ITERATION,
              "launches_per_iteration_torch": "see the kernel trace; a few dozen",
              "agreement_after_5_iterations_rel_max": agree, "timings": {}}
    for k, ms in times.items():
        st = stats(ms)
        if k in bytes_:
            st["algorithmic_bytes"] = bytes_[k]
            st["achieved_TBps"] = bytes_[k] / (st["median_ms"] * 1e-3) / 1e12
        report["timings"][k] = st
    a, t = report["timings"]["amx_run_instance_opt"], report["timings"]["torch_run_instance_opt"]
    lo = report["timings"]["amx_loop_only"]
    f3, b3 = report["timings"]["amx_smooth3_fused"], report["timings"]["amx_smooth3_three_box_launches"]
    report["summary"] = {
        "amx_total_ms": a["median_ms"], "torch_total_ms": t["median_ms"], "torch_spread_ms": t["spread_ms"],
        "speedup": t["median_ms"] / a["median_ms"],
        "faster_by_more_than_the_yardsticks_spread": t["median_ms"] - a["median_ms"] > t["spread_ms"],
        "amx_ms_per_iteration": lo["median_ms"] / niter, "torch_ms_per_iteration": t["median_ms"] / niter,
        "smooth3_fused_ms": f3["median_ms"], "smooth3_three_launches_ms": b3["median_ms"],
        "smooth3_fused_wins": f3["median_ms"] < b3["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    for k, st in report["timings"].items():
        extra = f"  {st['algorithmic_bytes'] / 1e6:8.0f} MB  {st['achieved_TBps']:.2f} TB/s of {HBM_TBS}" if "achieved_TBps" in st else ""
        print(f"{k:36s} median {st['median_ms']:9.3f} ms  min {st['min_ms']:9.3f}  max {st['max_ms']:9.3f}{extra}")
    print(json.dumps(report["summary"]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
