"""The conv tokenizer of PrimusV2-S under autograd on its two routes, ``train_tokenizer`` "torch" (vendor convolutions under torch
autograd) and "hip" (``_TokenizerFn``: amx_tokenizer_train_forward / amx_tokenizer_backward), at 2 x 128^3:

  (a) the tokenizer alone: forward + backward of ``down_projection`` (stem, stages and the torch ``proj``) from a fixed gradient;
  (b) the whole eager contrastive step of tools/primus_step_time.py (rows route of the decoder, ``train_attention = train_linear =
      "hip"``) with the tokenizer on each route, and the peak of torch's allocated memory above what is allocated before the step;
  (c) the bytes of the saved state and of the scratch at that shape.

The protocol of tools/primus_step_time.py: the routes alternate in one process, device events, 1 warm-up + 3 timed rounds, medians.
No threshold: the numbers are recorded as measured.

    python tools/primus_tokenizer_time.py [--out profiles/primus_tokenizer_time.json] [--crop 128]
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
from anatomix_amd import _lib  # noqa: E402
from anatomix_amd.model.vit3d import PRIMUS_CONFIGS, PrimusV2  # noqa: E402
from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss, contrastive_step  # noqa: E402

WARMUP, TIMED = 1, 3
ROUTES = ("torch", "hip")


def timed(dev, runs):
    """{route: (ms list, peak bytes above start, last result)} of ``runs`` = {route: callable}, alternating."""
    ms, peak, last = {r: [] for r in runs}, {}, {}
    for it in range(WARMUP + TIMED):
        for route, fn in runs.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = fn()
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ms[route].append(a.elapsed_time(b))
                peak[route] = max(peak.get(route, 0), torch.cuda.max_memory_allocated(dev) - base)
            last[route] = res
            del res
    return {r: (ms[r], peak[r], last[r]) for r in runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primus_tokenizer_time.json"))
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--patches", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("primus_tokenizer_time: needs a GPU (a time measured anywhere else says nothing)")
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
    x = torch.cat((A, B))
    assert netG.tokenizer_unsupported_reason(x) is None, netG.tokenizer_unsupported_reason(x)
    tok = netG.down_projection
    d_feat = torch.randn(2, conf["embed_dim"], S // 8, S // 8, S // 8, device=dev)

    def alone(route):
        def run():
            netG.train_tokenizer = route
            for p in tok.parameters():
                p.grad = None
            tok(x).backward(d_feat)
            return {n: p.grad for n, p in tok.named_parameters()}
        return run

    def step(route):
        def run():
            netG.train_tokenizer = route
            for p in list(netG.parameters()) + list(netF.parameters()):
                p.grad = None
            r = contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=args.patches, sample_ids=ids)
            assert r["out"] is None
            return {k: r[k] for k in ("loss", "grad_norm_G", "grad_norm_F")}
        return run

    part_a = timed(dev, {r: alone(r) for r in ROUTES})
    grads = {r: part_a[r][2] for r in ROUTES}
    worst = max(((grads["hip"][n] - g).norm() / g.norm().clamp_min(1e-30)).item() for n, g in grads["torch"].items()
                if not (n.endswith("conv.bias") or n.endswith("conv1.bias") or n.endswith("conv2.bias")))
    part_b = timed(dev, {r: step(r) for r in ROUTES})
    lib = _lib.load()
    med = lambda v: round(float(np.median(v)), 2)
    out = {"tool": "tools/primus_tokenizer_time.py", "device": torch.cuda.get_device_name(0),
           "what": f"PrimusV2-S at 2 x {S}^3, train_tokenizer torch vs hip; device events, 1 warm-up + 3 timed rounds, routes alternating in one "
                   f"process; step: one eager contrastive step (no optimizer), one pair, {args.patches} patches, train_attention = train_linear = hip",
           "tokenizer_forward_backward": {r: {"ms": [round(v, 2) for v in part_a[r][0]], "median_ms": med(part_a[r][0]),
                                              "peak_allocated_mib_above_start": round(part_a[r][1] / 2 ** 20, 1)} for r in ROUTES},
           "tokenizer_grad_worst_rel_l2_between_routes_free_masks": worst,
           "step": {r: {"ms": [round(v, 2) for v in part_b[r][0]], "median_ms": med(part_b[r][0]),
                        "peak_allocated_mib_above_start": round(part_b[r][1] / 2 ** 20, 1), **part_b[r][2]} for r in ROUTES},
           "saved_bytes": int(lib.amx_tokenizer_train_saved_bytes(2, S, S, S)), "scratch_bytes": int(lib.amx_tokenizer_train_scratch_bytes(2, S, S, S))}
    out["hip_over_torch_tokenizer_time"] = round(out["tokenizer_forward_backward"]["hip"]["median_ms"] / out["tokenizer_forward_backward"]["torch"]["median_ms"], 3)
    out["hip_over_torch_step_time"] = round(out["step"]["hip"]["median_ms"] / out["step"]["torch"]["median_ms"], 3)
    out["step_loss_rel_difference"] = abs(out["step"]["hip"]["loss"] - out["step"]["torch"]["loss"]) / abs(out["step"]["torch"]["loss"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
