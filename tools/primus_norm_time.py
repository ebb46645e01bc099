"""The token LayerNorms and the SwiGLU gate of PrimusV2-S under autograd on their two routes, ``train_norm`` "torch" (the modules under
torch autograd) and "hip" (``_LayerNormFn`` / ``_GatedLayerNormFn``: amx_layernorm_train_forward / amx_layernorm_backward), at 2 x 128^3
with ``train_attention = train_linear = train_tokenizer = "hip"``:

  (a) the two operators alone, forward + backward from a fixed gradient: a plain norm on [8192, 396] and the gated norm on [8192, 1056];
  (b) one ``EvaBlock`` alone, forward + backward from a fixed gradient on the [2, 4096, 396] token stream;
  (c) the whole eager contrastive step of tools/primus_step_time.py (rows route of the decoder) with its loss and gradient norms, and the
      peak of torch's allocated memory above what is allocated before the step.

The protocol of tools/primus_step_time.py: the routes alternate in one process, device events, 1 warm-up + 3 timed rounds, medians.
No threshold: the numbers are recorded as measured.

    python tools/primus_norm_time.py [--out profiles/primus_norm_time.json] [--crop 128]
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anatomix_amd.model.vit3d import PRIMUS_CONFIGS, PrimusV2  # noqa: E402
from anatomix_amd.model.vit3d import architectures as ARCH  # noqa: E402
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primus_norm_time.json"))
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--patches", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("primus_norm_time: needs a GPU (a time measured anywhere else says nothing)")
    dev = torch.device("cuda:0")
    S = args.crop
    torch.manual_seed(0)
    conf = PRIMUS_CONFIGS["S"]
    E = conf["embed_dim"]
    netG = PrimusV2(input_channels=1, num_classes=16, embed_dim=E, eva_depth=conf["eva_depth"], eva_numheads=conf["eva_numheads"],
                    patch_embed_size=(8, 8, 8), input_shape=(S, S, S), init_values=0.1, scale_attn_inner=True).to(dev).train()
    netG.train_attention = netG.train_linear = netG.train_tokenizer = "hip"
    with contextlib.redirect_stdout(io.StringIO()):
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
        netF.create_mlp([torch.zeros(1, 16, 1, 1, 1, device=dev)])
    netF = netF.to(dev).train()
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
    A, B = torch.randn(2, 1, 1, S, S, S, device=dev).unbind(0)
    seg = torch.randint(0, 6, (1, 1, S, S, S), device=dev).float()
    flat = torch.randperm(S ** 3, device=dev)[: args.patches]
    ids = [torch.stack([flat // (S * S), flat // S % S, flat % S], 1)]
    assert netG.tokenizer_unsupported_reason(torch.cat((A, B))) is None
    T = (S // 8) ** 3
    blk = netG.eva.blocks[0]
    hidden = blk.mlp.norm.normalized_shape[0]
    tok = torch.randn(2, T, E, device=dev)
    d_tok = torch.randn(2, T, E, device=dev)
    xg, gg, dg = (torch.randn(2 * T, hidden, device=dev) for _ in range(3))

    def plain(route):
        layer = blk.norm1
        def run():
            x = tok.detach().requires_grad_(True)
            layer.weight.grad = layer.bias.grad = None
            y = ARCH._layer_norm(layer, x, route)
            y.backward(d_tok)
            return x.grad
        return run

    def gated(route):
        layer = blk.mlp.norm
        def run():
            x, g = xg.detach().requires_grad_(True), gg.detach().requires_grad_(True)
            layer.weight.grad = layer.bias.grad = None
            y = ARCH._GatedLayerNormFn.apply(g, x, layer.weight, layer.bias, layer.eps) if route == "hip" else layer(F.silu(g) * x)
            y.backward(dg)
            return x.grad
        return run

    def block(route):
        def run():
            netG.train_norm = route
            for p in blk.parameters():
                p.grad = None
            x = tok.detach().requires_grad_(True)
            blk(x, netG.rope_table, 0).backward(d_tok)
            return x.grad
        return run

    def step(route):
        def run():
            netG.train_norm = route
            for p in list(netG.parameters()) + list(netF.parameters()):
                p.grad = None
            r = contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=args.patches, sample_ids=ids)
            assert r["out"] is None
            return {k: r[k] for k in ("loss", "grad_norm_G", "grad_norm_F")}
        return run

    rel = lambda res: ((res["hip"][2] - res["torch"][2]).norm() / res["torch"][2].norm()).item()
    med = lambda v: round(float(np.median(v)), 3)
    row = lambda res, extra=lambda r: {}: {r: {"ms": [round(v, 3) for v in res[r][0]], "median_ms": med(res[r][0]),
                                               "peak_allocated_mib_above_start": round(res[r][1] / 2 ** 20, 1), **extra(r)} for r in ROUTES}
    part_p = timed(dev, {r: plain(r) for r in ROUTES})
    part_g = timed(dev, {r: gated(r) for r in ROUTES})
    part_b = timed(dev, {r: block(r) for r in ROUTES})
    part_s = timed(dev, {r: step(r) for r in ROUTES})
    out = {"tool": "tools/primus_norm_time.py", "device": torch.cuda.get_device_name(0),
           "what": f"PrimusV2-S at 2 x {S}^3, train_norm torch vs hip, train_attention = train_linear = train_tokenizer = hip; device events, 1 warm-up "
                   f"+ 3 timed rounds, routes alternating in one process; step: one eager contrastive step (no optimizer), one pair, {args.patches} patches",
           f"layernorm_{2 * T}x{E}_forward_backward": dict(row(part_p), dx_rel_l2_between_routes=rel(part_p)),
           f"gated_layernorm_{2 * T}x{hidden}_forward_backward": dict(row(part_g), dx_rel_l2_between_routes=rel(part_g)),
           "block_forward_backward": dict(row(part_b), dx_rel_l2_between_routes=rel(part_b)),
           "step": row(part_s, lambda r: part_s[r][2])}
    for key in list(out):
        if isinstance(out[key], dict) and "hip" in out[key]:
            out[key]["hip_over_torch_time"] = round(out[key]["hip"]["median_ms"] / out[key]["torch"]["median_ms"], 3)
    out["step_loss_rel_difference"] = abs(out["step"]["hip"]["loss"] - out["step"]["torch"]["loss"]) / abs(out["step"]["torch"]["loss"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
