"""Forward + backward of the ViT's attention core at the model's training shape, on both routes of ``EvaAttention.train_core``:
"hip" (amx_attention_qknorm_rope_train + amx_attention_backward) and "torch" (per-head LayerNorm, rotation and
F.scaled_dot_product_attention under torch autograd).  (B, N, heads, head_dim) = (4, 4104, 6, 66), QK-norm and rotary embedding on.

The two routes alternate in one process, device events around forward + backward, 1 warm-up + 3 timed rounds; the peak of
torch's allocated memory above the inputs is recorded per route (for "hip" that includes the shared scratch buffer).  No threshold:
the numbers are recorded as measured.

    python tools/attn_train_time.py [--out profiles/attn_train_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anatomix_amd.model.vit3d.architectures import EvaAttention, build_rope_table  # noqa: E402

SHAPE = dict(B=4, N=4104, heads=6, head_dim=66, n_prefix=8)
WARMUP, TIMED = 1, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_train_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_train_time: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    B, N, heads, hd, nreg = (SHAPE[k] for k in ("B", "N", "heads", "head_dim", "n_prefix"))
    E = heads * hd
    torch.manual_seed(0)
    att = EvaAttention(E, heads, True, False).to(dev)
    table = build_rope_table((16, 16, 16), hd).to(dev)
    q, k, v = [torch.randn(B, N, E, device=dev, requires_grad=True) for _ in range(3)]
    dout = torch.randn(B, N, E, device=dev)
    params = [att.q_norm.weight, att.q_norm.bias, att.k_norm.weight, att.k_norm.bias]

    def run(route):
        core = att.core_hip_train if route == "hip" else att.core_torch
        y = core(q, k, v, table, nreg)
        return torch.autograd.grad(y, [q, k, v] + params, dout)

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    ms, peak, grads = {"hip": [], "torch": []}, {}, {}
    for it in range(WARMUP + TIMED):
        for route in ("hip", "torch"):
            torch.cuda.reset_peak_memory_stats(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g = run(route)
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ms[route].append(a.elapsed_time(b))
                peak[route] = max(peak.get(route, 0), torch.cuda.max_memory_allocated(dev) - base)
            grads[route] = [t.detach() for t in g]
            del g
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm()).item()
    res = {
        "tool": "tools/attn_train_time.py", "device": torch.cuda.get_device_name(0), "shape": SHAPE, "qk_norm": True, "rope": True,
        "what": "forward + backward of the attention core (gradients of q, k, v and the four norm vectors), device events, "
                f"{WARMUP} warm-up + {TIMED} timed rounds, routes alternating in one process",
        "routes": {r: {"ms": [round(x, 3) for x in ms[r]], "median_ms": round(float(np.median(ms[r])), 3),
                       "peak_allocated_mib_above_inputs": round(peak[r] / 2 ** 20, 1)} for r in ms},
        "hip_vs_torch_rel_l2": {n: rel(a, b) for n, a, b in zip(("dq", "dk", "dv", "q_norm.weight", "q_norm.bias", "k_norm.weight",
                                                                   "k_norm.bias"), grads["hip"], grads["torch"])},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
