"""Times the two registration metrics at the reference pipeline's own shape, a 256^3 pair:

  (i)  dice_score of this package (amx_label_overlap on the device, the score from its counts) against the reference driver's
       route (run_convex_adam_with_network_feats.py:283-295): the moved label map copied device -> host, then
       sklearn.metrics.f1_score(average='macro', labels=np.unique(fixseg)[1:]) on the two host volumes -- or, where sklearn
       is not importable, the same score from numpy.bincount on the host;
  (ii) jacobian_determinant of this package (amx_jacobian_det: the field and its six statistics in one pass) against the
       reference's JacobianDet arithmetic (convex_adam_utils.py:249-282) in stock torch ops on the same device, the grid
       already resident (generate_grid's host work is left out of the yardstick's time).

The yardsticks are written here and never call the code under test.  One process, alternating, after warm-up, device events
around every call, >= 20 repetitions each; median and spread.  Needs a GPU.  Writes a JSON report (default
profiles/regmetrics_bench.json) and prints the DESIGN 4.7 rows: time, algorithmic bytes from the shapes, achieved TB/s.

    python tools/regmetrics_bench.py [--reps 20] [--warmup 2] [--size 256] [--out profiles/regmetrics_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
LABELS = 36                                   # a whole-brain style label map: 35 structures and background


# ---- yardsticks -----------------------------------------------------------------------------------------------------------

def host_dice_sklearn(fixseg, moved_seg_dev):
    from sklearn.metrics import f1_score
    return f1_score(fixseg.flatten(), moved_seg_dev.cpu().numpy().flatten(), average='macro',
                    labels=np.unique(fixseg).astype(int).tolist()[1:])


def host_dice_bincount(fixseg, moved_seg_dev):
    a, b = fixseg.reshape(-1).astype(np.int64), moved_seg_dev.cpu().numpy().reshape(-1).astype(np.int64)
    n = int(max(a.max(), b.max())) + 1
    ca, cb, both = np.bincount(a, minlength=n), np.bincount(b, minlength=n), np.bincount(a[a == b], minlength=n)
    labels = np.nonzero(ca)[0][1:]
    return float(np.mean(2.0 * both[labels] / (ca[labels] + cb[labels])))


def t_jacobian(y_pred, grid):
    J = y_pred + grid
    base = J[:, :-1, :-1, :-1, :]
    dy, dx, dz = J[:, 1:, :-1, :-1, :] - base, J[:, :-1, 1:, :-1, :] - base, J[:, :-1, :-1, 1:, :] - base
    d0 = dx[..., 0] * (dy[..., 1] * dz[..., 2] - dy[..., 2] * dz[..., 1])
    d1 = dx[..., 1] * (dy[..., 0] * dz[..., 2] - dy[..., 2] * dz[..., 0])
    d2 = dx[..., 2] * (dy[..., 0] * dz[..., 1] - dy[..., 1] * dz[..., 0])
    return d0 - d1 + d2


def t_jacobian_stats(y_pred, grid):
    J = t_jacobian(y_pred, grid)
    lg = torch.log(J[J > 0].double())
    return J, torch.stack([(J <= 0).double().mean(), J.min().double(), J.max().double(), J.double().mean(), lg.mean(), lg.std(unbiased=False)])


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


def label_maps(n, rs):
    """Spatially coherent label maps: 16^3 blocks of one label, the moved map shifted by a few voxels with 1 % of its voxels redrawn."""
    coarse = rs.randint(0, LABELS, (n // 16,) * 3)
    fix = np.kron(coarse, np.ones((16,) * 3, dtype=coarse.dtype))
    mov = np.roll(fix, (3, -2, 1), (0, 1, 2))
    redraw = rs.rand(n, n, n) < 0.01
    return fix.astype(np.float64), np.where(redraw, rs.randint(0, LABELS, (n, n, n)), mov).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regmetrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("regmetrics_bench needs a GPU: a timing taken anywhere else says nothing about these kernels")
    from anatomix_amd.registration import dice_score, generate_grid, jacobian_determinant, jacobian_statistics
    from anatomix_amd.registration.metrics import _overlap
    try:
        import sklearn  # noqa: F401
        host_dice, host_route = host_dice_sklearn, "sklearn.metrics.f1_score " + sklearn.__version__
    except ImportError:
        host_dice, host_route = host_dice_bincount, "numpy.bincount"
    dev = torch.device("cuda:0")
    n = args.size
    rs = np.random.RandomState(0)
    fixseg, movseg = label_maps(n, rs)                                  # the fixed map is a host volume in the driver (get_fdata)
    moved_dev = torch.from_numpy(movseg).to(dev)
    fixed_dev = torch.from_numpy(fixseg).float().to(dev)
    torch.manual_seed(0)
    disp = torch.rand((1, 3, n, n, n), device=dev)
    for _ in range(3):
        disp = torch.nn.functional.avg_pool3d(disp, 3, 1, 1)
    disp = ((disp - 0.5) * 40.0).contiguous()                           # smooth, a few voxels, folds here and there
    y_pred = disp.permute(0, 2, 3, 4, 1).flip(-1).contiguous()
    grid = torch.from_numpy(generate_grid((n, n, n))).float().to(dev)[None]

    # both sides compute the same thing
    ours_dice, theirs_dice = dice_score(fixed_dev, moved_dev)[0], host_dice(fixseg, moved_dev)
    jd, st = jacobian_determinant(disp, return_stats=True)
    tj, tst = t_jacobian_stats(y_pred, grid)
    agree_j = float((jd - tj).abs().max() / tj.abs().max())
    print(f"dice {ours_dice:.12f} against {host_route} {theirs_dice:.12f}; jacobian field max abs difference {agree_j:.3e} of max|J|")
    print("stats amx  ", [f"{v:.6g}" for v in st.tolist()])
    print("stats torch", [f"{v:.6g}" for v in tst.tolist()])
    del jd, tj

    runs = {
        "amx_dice_score": lambda: dice_score(fixed_dev, moved_dev),
        "amx_dice_score_with_upload_of_the_fixed_map": lambda: dice_score(torch.from_numpy(fixseg).float().to(dev), moved_dev),
        "amx_label_overlap_kernel": lambda: _overlap(fixed_dev, moved_dev, 1024),
        "host_dice_reference_route": lambda: host_dice(fixseg, moved_dev),
        "amx_jacobian_field_and_stats": lambda: jacobian_determinant(disp, return_stats=True),
        "amx_jacobian_field": lambda: jacobian_determinant(disp),
        "amx_jacobian_stats": lambda: jacobian_statistics(disp),
        "torch_jacobian_field": lambda: t_jacobian(y_pred, grid),
        "torch_jacobian_field_and_stats": lambda: t_jacobian_stats(y_pred, grid),
    }
    times = {k: [] for k in runs}
    for _ in range(args.warmup):
        for k, fn in runs.items():
            timed(fn)
    for _ in range(args.reps):                                          # alternating: every repetition visits every variant once
        for k, fn in runs.items():
            times[k].append(timed(fn)[0])

    vox, out_vox = n ** 3, (n - 1) ** 3
    bytes_ = {
        "amx_label_overlap_kernel": 2 * 4 * vox,                        # two fp32 label volumes read once
        "amx_dice_score": 2 * 4 * vox,
        "amx_jacobian_field_and_stats": 4 * (3 * vox + out_vox),        # the field read once, the determinants written once
        "amx_jacobian_field": 4 * (3 * vox + out_vox),
        "amx_jacobian_stats": 4 * 3 * vox,
    }
    report = {"device": torch.cuda.get_device_name(0), "size": [n] * 3, "labels": LABELS, "host_dice_route": host_route,
              "dice_amx": ours_dice, "dice_host": float(theirs_dice), "jacobian_field_rel_max_difference": agree_j,
              "jacobian_stats_amx": st.tolist(), "jacobian_stats_torch": tst.tolist(), "timings": {}}
    for k, ms in times.items():
        s = stats(ms)
        if k in bytes_:
            s["algorithmic_bytes"] = bytes_[k]
            s["achieved_TBps"] = bytes_[k] / (s["median_ms"] * 1e-3) / 1e12
            s["share_of_hbm_roofline"] = s["achieved_TBps"] / HBM_TBS
        report["timings"][k] = s
    T = report["timings"]
    report["summary"] = {
        "dice_amx_ms": T["amx_dice_score"]["median_ms"], "dice_host_ms": T["host_dice_reference_route"]["median_ms"],
        "dice_speedup": T["host_dice_reference_route"]["median_ms"] / T["amx_dice_score"]["median_ms"],
        "dice_faster_than_yardstick": T["amx_dice_score_with_upload_of_the_fixed_map"]["median_ms"] < T["host_dice_reference_route"]["median_ms"],
        "jacobian_amx_ms": T["amx_jacobian_field_and_stats"]["median_ms"],
        "jacobian_torch_ms": T["torch_jacobian_field_and_stats"]["median_ms"],
        "jacobian_speedup": T["torch_jacobian_field_and_stats"]["median_ms"] / T["amx_jacobian_field_and_stats"]["median_ms"],
        "jacobian_field_speedup": T["torch_jacobian_field"]["median_ms"] / T["amx_jacobian_field"]["median_ms"],
        "jacobian_faster_than_yardstick": T["amx_jacobian_field"]["median_ms"] < T["torch_jacobian_field"]["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    for k, s in T.items():
        extra = f"  {s['algorithmic_bytes'] / 1e6:8.0f} MB  {s['achieved_TBps']:.2f} TB/s of {HBM_TBS}" if "achieved_TBps" in s else ""
        print(f"{k:46s} median {s['median_ms']:10.3f} ms  min {s['min_ms']:10.3f}  max {s['max_ms']:10.3f}{extra}")
    print(json.dumps(report["summary"]))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
