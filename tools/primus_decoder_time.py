"""The dense patch decoder of PrimusV2-S under autograd on its two routes, ``train_decoder`` "torch" (vendor transposed convolutions and
the modules under torch autograd) and "hip" (``_DecoderFn``: amx_vit_decoder_train_forward / amx_vit_decoder_backward), at 2 x 128^3:

  (a) decoder + ``demean`` alone, forward + backward from a fixed gradient on the [2, 4096, 396] token stream;
  (b) one whole eager contrastive step with ``out_norm = "demean"`` -- the spatial norm forces the dense route -- and the other four
      switches on "hip", with its loss and gradient norms;
  (c) one ``finetune_loss`` step of ``Sequential(PrimusV2-S, Conv3d(16, 4, 1))`` at 1 x 128^3 (Dice + CE), other switches on "hip".

The protocol of tools/primus_norm_time.py: the routes alternate in one process, device events, 1 warm-up + 3 timed rounds, medians, the
peak of torch's allocated memory above what is allocated before the call.  No threshold: the numbers are recorded as measured.  Beside
them: the HBM traffic the kernels of (a) move, counted from the tensor sizes, and the time that traffic takes at the rate of the
project's pooling kernel.

    python tools/primus_decoder_time.py [--out profiles/primus_decoder_time.json] [--crop 128]
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
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anatomix_amd.model.vit3d import PRIMUS_CONFIGS, PrimusV2  # noqa: E402
from anatomix_amd.model.vit3d import architectures as ARCH  # noqa: E402
from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss, contrastive_step  # noqa: E402
from anatomix_amd.segmentation import DiceCELoss, finetune_loss  # noqa: E402

WARMUP, TIMED = 1, 3
ROUTES = ("torch", "hip")
STREAM_RATE_TBS = 3.96          # the pooling kernel, DESIGN 4.14


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


def traffic_bytes(n, tokens, widths):
    """Bytes the kernels of one forward + backward move through HBM, counted from the tensor sizes (every launch reads its inputs and
    writes its outputs once; weights and partials left out): per stage the product's operand and result, the LayerNorm pass, and in the
    backward the recomputed h, the gathered rows, the data gradient, the LayerNorm adjoint in place and both operands of the weight gradient."""
    e, c1, c2, c = widths
    r0 = n * tokens
    tok, a1, a2, out = r0 * e, 8 * r0 * c1, 64 * r0 * c2, 512 * r0 * c
    fwd = (tok + a1) + 2 * a1 + (a1 + a2) + 2 * a2 + (a2 + out) + 3 * out            # products, LN passes, demean statistics + apply
    bwd = 2 * a1 + 2 * a2 + out + 2 * out + out + (a2 + out) + (out + a2) + 3 * a2 + (a1 + a2) + (a2 + a1) + 3 * a1 + (tok + a1) + (a1 + tok)
    return 4 * (fwd + bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "primus_decoder_time.json"))
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--patches", type=int, default=512)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("primus_decoder_time: needs a GPU (a time measured anywhere else says nothing)")
    dev = torch.device("cuda:0")
    S = args.crop
    torch.manual_seed(0)
    conf = PRIMUS_CONFIGS["S"]
    E = conf["embed_dim"]
    netG = PrimusV2(input_channels=1, num_classes=16, embed_dim=E, eva_depth=conf["eva_depth"], eva_numheads=conf["eva_numheads"],
                    patch_embed_size=(8, 8, 8), input_shape=(S, S, S), init_values=0.1, scale_attn_inner=True, out_norm="demean").to(dev).train()
    netG.train_attention = netG.train_linear = netG.train_tokenizer = netG.train_norm = "hip"
    with contextlib.redirect_stdout(io.StringIO()):
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
        netF.create_mlp([torch.zeros(1, 16, 1, 1, 1, device=dev)])
    netF = netF.to(dev).train()
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
    A, B = torch.randn(2, 1, 1, S, S, S, device=dev).unbind(0)
    seg = torch.randint(0, 6, (1, 1, S, S, S), device=dev).float()
    flat = torch.randperm(S ** 3, device=dev)[: args.patches]
    ids = [torch.stack([flat // (S * S), flat // S % S, flat % S], 1)]
    assert netG.decoder_unsupported_reason(torch.cat((A, B))) is None and netG.sampled_unsupported_reason(torch.cat((A, B))) is not None
    T = (S // 8) ** 3
    widths = [netG.up_projection.decode[0][0].in_channels] + [m.out_channels for m in netG.up_projection.modules() if isinstance(m, nn.ConvTranspose3d)]
    tok = torch.randn(2, T, E, device=dev)
    dy = torch.randn(2, 16, S, S, S, device=dev)
    head = nn.Conv3d(16, 4, 1).to(dev)
    model = nn.Sequential(netG, head)
    labels = torch.randint(0, 4, (1, 1, S, S, S), device=dev)
    seg_loss = DiceCELoss(softmax=True, to_onehot_y=True)

    def decoder(route):
        def run():
            for p in netG.up_projection.parameters():
                p.grad = None
            x = tok.detach().requires_grad_(True)
            if route == "hip":
                y = ARCH.decode_dense(x, netG.up_projection, netG.out_norm, netG.grid)
            else:
                y = netG.out_norm(netG.up_projection(x.transpose(1, 2).reshape(2, E, *netG.grid)))
            y.backward(dy)
            return x.grad
        return run

    def step(route):
        def run():
            netG.train_decoder = route
            for p in list(netG.parameters()) + list(netF.parameters()):
                p.grad = None
            r = contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=args.patches, sample_ids=ids)
            assert torch.is_tensor(r["out"])
            return {k: r[k] for k in ("loss", "grad_norm_G", "grad_norm_F")}
        return run

    def finetune(route):
        def run():
            netG.train_decoder = route
            for p in model.parameters():
                p.grad = None
            v = finetune_loss(model, A, labels, seg_loss)
            v.backward()
            return {"loss": float(v.detach())}
        return run

    med = lambda v: round(float(np.median(v)), 3)
    row = lambda res, extra=lambda r: {}: {r: {"ms": [round(v, 3) for v in res[r][0]], "median_ms": med(res[r][0]),
                                               "peak_allocated_mib_above_start": round(res[r][1] / 2 ** 20, 1), **extra(r)} for r in ROUTES}
    part_d = timed(dev, {r: decoder(r) for r in ROUTES})
    part_s = timed(dev, {r: step(r) for r in ROUTES})
    part_f = timed(dev, {r: finetune(r) for r in ROUTES})
    rel = ((part_d["hip"][2] - part_d["torch"][2]).norm() / part_d["torch"][2].norm()).item()
    nbytes = traffic_bytes(2, T, widths)
    out = {"tool": "tools/primus_decoder_time.py", "device": torch.cuda.get_device_name(0),
           "what": f"PrimusV2-S at 2 x {S}^3, out_norm demean, train_decoder torch vs hip, the other four switches on hip; device events, 1 warm-up "
                   f"+ 3 timed rounds, routes alternating in one process; step: one eager contrastive step (no optimizer), one pair, {args.patches} "
                   f"patches, dense route; finetune: Sequential(PrimusV2-S, Conv3d(16, 4, 1)), Dice + CE, 1 x {S}^3, forward + backward",
           "decoder_widths": widths,
           "decoder_demean_forward_backward": dict(row(part_d), d_tokens_rel_l2_between_routes=rel),
           "step": row(part_s, lambda r: part_s[r][2]),
           "finetune_step": row(part_f, lambda r: part_f[r][2]),
           "hip_decoder_hbm_traffic_mb": round(nbytes / 1e6, 1),
           "hip_decoder_traffic_time_ms_at_3.96_tb_s": round(nbytes / (STREAM_RATE_TBS * 1e12) * 1e3, 3)}
    for key in list(out):
        if isinstance(out[key], dict) and "hip" in out[key]:
            out[key]["hip_over_torch_time"] = round(out[key]["hip"]["median_ms"] / out[key]["torch"]["median_ms"], 3)
    out["hip_decoder_time_over_traffic_time"] = round(out["decoder_demean_forward_backward"]["hip"]["median_ms"] /
                                                      out["hip_decoder_traffic_time_ms_at_3.96_tb_s"], 1)
    out["step_loss_rel_difference"] = abs(out["step"]["hip"]["loss"] - out["step"]["torch"]["loss"]) / abs(out["step"]["torch"]["loss"])
    out["finetune_loss_rel_difference"] = abs(out["finetune_step"]["hip"]["loss"] - out["finetune_step"]["torch"]["loss"]) / abs(out["finetune_step"]["torch"]["loss"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
