"""Forward + backward of the EVA blocks' linear layers at the model's training shape (M = 4 x 4104 token rows), on both routes of
``train_linear``: "hip" (``_LinearFn``: amx_linear_forward + amx_linear_backward, f16 operands and fp32 sums) and "torch" (F.linear
under torch autograd, fp32 vendor GEMMs).  Measured: the three layer shapes of PrimusV2-S (396 -> 396, 396 -> 1056, 1056 -> 396, each
with a bias and all three gradients), and one whole ``EvaBlock`` (``train_attention = "hip"``, QK-norm, rotary embedding, LayerScale)
with its seven linears on either route.

The protocol of tools/attn_train_time.py: the two routes alternate in one process, device events around forward + backward,
1 warm-up + 3 timed rounds; the peak of torch's allocated memory above the inputs is recorded per route (for "hip" that includes the
shared scratch buffer).  No threshold: the numbers are recorded as measured.

    python tools/linear_train_time.py [--out profiles/linear_train_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anatomix_amd.model.vit3d.architectures import EvaBlock, _LinearFn, build_rope_table  # noqa: E402

B, N_TOK, N_PREFIX, HEADS, DIM, HIDDEN = 4, 4104, 8, 6, 396, 1056
LAYERS = {"q_proj / v_proj / attn.proj (396 -> 396)": (DIM, DIM), "mlp.fc1_g / fc1_x (396 -> 1056)": (DIM, HIDDEN),
          "mlp.fc2 (1056 -> 396)": (HIDDEN, DIM)}
WARMUP, TIMED = 1, 3
ROUTES = ("hip", "torch")


def measure(dev, run):
    """``run(route)`` -> tensors; per route the timed milliseconds, the peak allocation above what is allocated now, the last result."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    ms, peak, last = {r: [] for r in ROUTES}, {}, {}
    for it in range(WARMUP + TIMED):
        for route in ROUTES:
            torch.cuda.reset_peak_memory_stats(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g = run(route)
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ms[route].append(a.elapsed_time(b))
                peak[route] = max(peak.get(route, 0), torch.cuda.max_memory_allocated(dev) - base)
            last[route] = [t.detach() for t in g]
            del g
    rel = lambda x, y: ((x.double() - y.double()).norm() / y.double().norm()).item()
    return {"routes": {r: {"ms": [round(v, 3) for v in ms[r]], "median_ms": round(float(np.median(ms[r])), 3),
                           "peak_allocated_mib_above_inputs": round(peak[r] / 2 ** 20, 1)} for r in ROUTES},
            "hip_over_torch_time": round(float(np.median(ms["hip"]) / np.median(ms["torch"])), 3),
            "hip_vs_torch_rel_l2_max": max(rel(x, y) for x, y in zip(last["hip"], last["torch"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_train_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_train_time: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    M = B * N_TOK
    res = {"tool": "tools/linear_train_time.py", "device": torch.cuda.get_device_name(0), "rows": M,
           "what": "forward + backward (dx, dW, db), device events, "
                   f"{WARMUP} warm-up + {TIMED} timed rounds, routes alternating in one process", "layers": {}}
    for name, (K, N) in LAYERS.items():
        x = torch.randn(B, N_TOK, K, device=dev, requires_grad=True)
        w = (torch.randn(N, K, device=dev) / K ** 0.5).requires_grad_(True)
        b = torch.randn(N, device=dev, requires_grad=True)
        dy = torch.randn(B, N_TOK, N, device=dev)

        def run(route):
            y = _LinearFn.apply(x, w, b) if route == "hip" else F.linear(x, w, b)
            return (y,) + torch.autograd.grad(y, [x, w, b], dy)

        res["layers"][name] = dict(K=K, N=N, gflop_forward_and_backward=round(6.0 * M * K * N / 1e9, 1), **measure(dev, run))
        del x, w, b, dy

    blk = EvaBlock(DIM, HEADS, HIDDEN, 0.1, True, True).to(dev)
    blk.attn.train_core = "hip"
    table = build_rope_table((16, 16, 16), DIM // HEADS).to(dev)
    x = torch.randn(B, N_TOK, DIM, device=dev, requires_grad=True)
    dy = torch.randn(B, N_TOK, DIM, device=dev)
    params = list(blk.parameters())

    def run_block(route):
        blk.attn.train_linear = blk.mlp.train_linear = route
        y = blk(x, table, N_PREFIX)
        return (y,) + torch.autograd.grad(y, [x] + params, dy)

    res["eva_block"] = dict(what="one EvaBlock (dim 396, 6 heads, hidden 1056, QK-norm, inner norm, LayerScale), train_attention = hip, "
                                 "gradients of the input and of every parameter", **measure(dev, run_block))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
