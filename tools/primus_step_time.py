"""One eager contrastive step of PrimusV2-S at 128^3 (one pair of views, 512 patches, ``train_attention = train_linear = "hip"``) on
the two routes of its decoder: "rows" (``PrimusV2.forward_train_sampled``: amx_vit_decode_rows_forward / _backward on the 2 x 512
sampled voxels) and "dense" (``allow_torch_path = True``: the torch modules decode the whole [2, 16, 128^3] volume, PatchSampleF
gathers from it, autograd pushes a dense gradient back).  The same network, views, labels and coordinates on both.

The protocol of tools/linear_train_time.py: the routes alternate in one process, device events around the whole step (forward, heads,
loss, backward, gradient norms; no optimizer), 1 warm-up + 3 timed rounds, medians; the peak of torch's allocated memory above what is
allocated before the step is recorded per route.  No threshold: the numbers are recorded as measured.

    python tools/primus_step_time.py [--out profiles/primus_step_time.json] [--crop 128]
"""
import argparse
import contextlib
import io
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anatomix_amd.model.vit3d import PRIMUS_CONFIGS, PrimusV2  # noqa: E402
from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss, contrastive_step  # noqa: E402

WARMUP, TIMED = 1, 3
ROUTES = ("rows", "dense")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primus_step_time.json"))
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--patches", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("primus_step_time: needs a GPU (a time measured anywhere else says nothing)")
    dev = torch.device("cuda:0")
    S = args.crop
    torch.manual_seed(0)
    conf = PRIMUS_CONFIGS["S"]
    netG = PrimusV2(input_channels=1, num_classes=16, embed_dim=conf["embed_dim"], eva_depth=conf["eva_depth"], eva_numheads=conf["eva_numheads"],
                    patch_embed_size=(8, 8, 8), input_shape=(S, S, S), init_values=0.1, scale_attn_inner=True).to(dev).train()
    netG.train_attention = netG.train_linear = "hip"
    with contextlib.redirect_stdout(io.StringIO()):
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
        netF.create_mlp([torch.zeros(1, 16, 1, 1, 1, device=dev)])
    netF = netF.to(dev).train()
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
    A, B = torch.randn(2, 1, 1, S, S, S, device=dev).unbind(0)
    seg = torch.randint(0, 6, (1, 1, S, S, S), device=dev).float()
    flat = torch.randperm(S ** 3, device=dev)[: args.patches]
    ids = [torch.stack([flat // (S * S), flat // S % S, flat % S], 1)]

    def step(route):
        netG.allow_torch_path = route == "dense"
        for p in list(netG.parameters()) + list(netF.parameters()):
            p.grad = None
        return contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=args.patches, sample_ids=ids)

    torch.cuda.synchronize()
    ms, peak, rec = {r: [] for r in ROUTES}, {}, {}
    for it in range(WARMUP + TIMED):
        for route in ROUTES:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r = step(route)
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ms[route].append(a.elapsed_time(b))
                peak[route] = max(peak.get(route, 0), torch.cuda.max_memory_allocated(dev) - base)
            rec[route] = {k: r[k] for k in ("loss", "grad_norm_G", "grad_norm_F")}
            assert (r["out"] is None) == (route == "rows")
            del r
    out = {"tool": "tools/primus_step_time.py", "device": torch.cuda.get_device_name(0),
           "what": f"one eager contrastive step (no optimizer) of PrimusV2-S at {S}^3, one pair, {args.patches} patches, train_attention = "
                   "train_linear = hip; device events, 1 warm-up + 3 timed rounds, routes alternating in one process",
           "routes": {r: {"ms": [round(v, 2) for v in ms[r]], "median_ms": round(float(np.median(ms[r])), 2),
                          "peak_allocated_mib_above_start": round(peak[r] / 2 ** 20, 1), **rec[r]} for r in ROUTES}}
    out["rows_over_dense_time"] = round(out["routes"]["rows"]["median_ms"] / out["routes"]["dense"]["median_ms"], 3)
    out["dense_minus_rows_ms"] = round(out["routes"]["dense"]["median_ms"] - out["routes"]["rows"]["median_ms"], 2)
    out["loss_rel_difference"] = abs(rec["rows"]["loss"] - rec["dense"]["loss"]) / abs(rec["dense"]["loss"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
