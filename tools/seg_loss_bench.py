"""Times what follows the UNet in one segmentation finetuning step (forward + backward of the 1x1x1 head and the Dice + CE loss)
at the reference's defaults -- features [4, 16, 128^3], 5 classes, int64 labels -- by three routes in one process, alternating,
after warm-up, with device events around every call:

  (1) head_dice_ce: the fused head + loss kernels (logits never in memory),
  (2) the logits-mode loss kernels behind a torch Conv3d head,
  (3) all torch: Conv3d plus the loss written here from stock torch ops on the GPU -- the composition a user would otherwise
      run.  It is the yardstick, never the code under test.

Needs a GPU.  Prints one JSON line (times, achieved GB/s of (1) against the algorithmic bytes, peak memory of each route, the
routes' agreement) and writes it to --out (default profiles/seg_loss.json).

    python tools/seg_loss_bench.py [--reps 10] [--warmup 3] [--batch 4] [--feat 16] [--classes 5] [--crop 128]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_dice_ce(logits, labels, smooth_nr=1e-5, smooth_dr=1e-5):
    """DiceCELoss(softmax=True, to_onehot_y=True, include_background=False) from stock torch ops, as MONAI composes it:
    softmax, one-hot, per-(b, c) sums over the voxels, plus nn.CrossEntropyLoss on all classes."""
    p = torch.softmax(logits, 1)
    t = torch.zeros_like(p).scatter_(1, labels.long(), 1.0)
    axes = (2, 3, 4)
    inter, den = (p[:, 1:] * t[:, 1:]).sum(axes), t[:, 1:].sum(axes) + p[:, 1:].sum(axes)
    dice = (1.0 - (2.0 * inter + smooth_nr) / (den + smooth_dr)).mean()
    return dice + torch.nn.functional.cross_entropy(logits, labels[:, 0].long())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--feat", type=int, default=16)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seg_loss.json"))
    a = ap.parse_args()
    if a.reps < 10 or a.warmup < 3:
        raise SystemExit("at least 3 warm-up and 10 timed repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("seg_loss_bench needs a GPU: a CPU time says nothing about the kernels")
    from anatomix_amd.segmentation import DiceCELoss, head_dice_ce

    dev = torch.device("cuda:0")
    B, F, C, S = a.batch, a.feat, a.classes, a.crop
    V = S ** 3
    g = torch.Generator(device="cpu").manual_seed(1)
    x = torch.randn(B, F, S, S, S, generator=g).to(dev).requires_grad_(True)
    labels = torch.randint(0, C, (B, 1, S, S, S), generator=g).to(dev)
    head = torch.nn.Conv3d(F, C, 1).to(dev)
    loss = DiceCELoss(softmax=True, to_onehot_y=True, include_background=False)
    leaves = [x, head.weight, head.bias]

    def route1():
        return head_dice_ce(x, head, labels, loss)

    def route2():
        return loss(head(x), labels)

    def route3():
        return torch_dice_ce(head(x), labels)

    routes = {"fused_head_loss": route1, "logits_loss_after_conv3d": route2, "all_torch": route3}

    def step(fn):
        for t in leaves:
            t.grad = None
        v = fn()
        v.backward()
        return v

    values, grads, peak = {}, {}, {}
    for name, fn in routes.items():
        for _ in range(a.warmup):
            step(fn)
        for t in leaves:                                     # so that the gradients a step returns count as its memory
            t.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        values[name] = float(step(fn).detach())
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        grads[name] = [t.grad.detach().clone() for t in leaves]
    times = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, fn in routes.items():                      # alternating, so that drift of the clock hits every route alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(fn)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    # algorithmic bytes of route (1): forward x + labels; backward x twice (logits, then dz . x), labels, dx written
    lab_b = labels.element_size()
    fwd_bytes, bwd_bytes = V * B * (4 * F + lab_b), V * B * (3 * 4 * F + lab_b)
    ref = "all_torch"
    agree = {name: {"loss_rel": abs(values[name] - values[ref]) / abs(values[ref]),
                    "grad_rel_max": max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(grads[name], grads[ref]))}
             for name in routes if name != ref}
    med = {k: statistics.median(v) for k, v in times.items()}
    report = {
        "device": torch.cuda.get_device_name(0), "shape": {"features": [B, F, S, S, S], "classes": C, "labels": "int64"},
        "what": "forward + backward of head and DiceCELoss per call, device events, median of reps", "reps": a.reps, "warmup": a.warmup,
        "ms": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in times.items()},
        "fused_algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
        "fused_achieved_GBps": (fwd_bytes + bwd_bytes) / (med["fused_head_loss"] * 1e-3) / 1e9,
        "speedup_of_fused_over_all_torch": med["all_torch"] / med["fused_head_loss"],
        "peak_memory_above_inputs_MB": {k: v / 2 ** 20 for k, v in peak.items()},
        "loss": values, "agreement_with_all_torch": agree,
    }
    line = json.dumps(report)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
