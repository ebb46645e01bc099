"""What gradient clipping costs in the replayed contrastive step: three routes in ONE process, alternated, at 128^3 with the
paper-default step (6 M UNet, six tapped layers, 512 patches, bf16 storage, AdamW lr 2e-4):

  (a) off     GraphedContrastiveStep with FusedAdamW(max_norm=None): the norms only measure (_grad_norms)
  (b) fused   FusedAdamW(max_norm=M): amx_grad_norms (two launches for both networks) + the clip inside the optimizer launch
  (c) torch   torch.nn.utils.clip_grad_norm_(max_norm=M) per network captured in the graph, then the unclipped FusedAdamW

    python tools/ubench/clip_step_bench.py [--size 128] [--rounds 7] [--steps 50] [--out clip_step_bench.json]

Each round times `steps` calls of every route (host clock around calls that end in the step's own host read, then a device
synchronise), the routes taking turns; reported per route: median, min and max of the per-step time over the rounds.  The
run-to-run spread of (a) (max - min over its rounds) is the margin of any comparison.  The routes differ only in the TAIL of the
step (norms + optimizers), so the kernel count is that of the tail: torch.profiler around one EAGER run of each route's tail after
the timed rounds (kernels inside a replayed graph are traced incompletely -- the same profiler reported 192 / 50 / 40 kernels for
replays of ~700 -- and the profiler is off while timing).  Needs a GPU; there is no fall-back."""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import anatomix_amd                                                             # noqa: E402
from anatomix_amd.pretraining import FusedAdamW, GraphedContrastiveStep, PatchSampleF, SupPatchNCELoss   # noqa: E402
from oracle import pretrain_inputs as PI, unet_ref as R                          # noqa: E402


class TorchClipStep(GraphedContrastiveStep):
    """Route (c): the clip as torch does it, inside the graph."""

    def __init__(self, *a, max_norm, **kw):
        super().__init__(*a, **kw)
        self.max_norm = max_norm

    def _tail(self, total, layer_losses):
        gG = torch.nn.utils.clip_grad_norm_(self.netG.parameters(), self.max_norm, foreach=True)
        gF = torch.nn.utils.clip_grad_norm_(self.netF.parameters(), self.max_norm, foreach=True)
        for opt in self.optimizers:
            opt.step()
        return torch.stack([total.detach(), gG.detach(), gF.detach()] + layer_losses)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max_norm", type=float, default=2.0)
    ap.add_argument("--num_patches", type=int, default=512)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_step_bench: needs a GPU")
    dev = torch.device("cuda:0")
    kw = R.VARIANTS["anatomix"]
    with contextlib.redirect_stdout(io.StringIO()):
        netG = anatomix_amd.Unet(**kw)
        netG.load_state_dict(R.synthetic_state_dict(kw, 3, gain=2 ** 0.5))
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
        netF.create_mlp([torch.zeros(1, c, 1, 1, 1, device=dev) for c in (128, 256, 128, 64, 32, 16)])
    netG.precision = "bf16"
    netG, netF = netG.to(dev).train(), netF.to(dev).train()
    nopt = Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw")
    A, B, seg = [t.to(dev) for t in PI.step_inputs(args.size)]
    okw = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)

    def route(name):
        g, f = copy.deepcopy(netG), copy.deepcopy(netF)
        crits = [SupPatchNCELoss(nopt) for _ in PI.NCE_LAYERS]
        m = args.max_norm if name == "fused" else None
        opts = (FusedAdamW(g.parameters(), max_norm=m, **okw), FusedAdamW(f.parameters(), max_norm=m, **okw))
        common = dict(num_patches=args.num_patches, warmup=3)
        if name == "torch":
            return TorchClipStep(g, f, crits, PI.NCE_LAYERS, opts, max_norm=args.max_norm, **common)
        return GraphedContrastiveStep(g, f, crits, PI.NCE_LAYERS, opts, **common)

    names = ("off", "fused", "torch")
    steps = {n: route(n) for n in names}
    first = {}
    for n in names:
        torch.manual_seed(5)
        recs = [steps[n](A, B, seg) for _ in range(args.warmup)]
        first[n] = dict(loss=recs[-1]["loss"], grad_norm_G=recs[-1]["grad_norm_G"], grad_norm_F=recs[-1]["grad_norm_F"])
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                steps[n](A, B, seg)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / args.steps * 1e3)
    kernels = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        for n in names:
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                steps[n]._tail(steps[n].total, steps[n].layer_losses)      # on the gradients the last replay left
                torch.cuda.synchronize()
            evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
            kernels[n] = len(evs)
    except Exception as e:                                      # (a profiler that cannot trace is a missing number, not a wrong one)
        kernels = {"error": repr(e)}
    res = dict(device=torch.cuda.get_device_name(0), size=args.size, num_patches=args.num_patches, max_norm=args.max_norm,
               rounds=args.rounds, steps_per_round=args.steps, last_warmup_record=first, kernels_in_tail=kernels,
               ms_per_step={n: dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v) for n, v in times.items()})
    a, b, c = (res["ms_per_step"][n]["median"] for n in names)
    res["spread_off_ms"] = res["ms_per_step"]["off"]["max"] - res["ms_per_step"]["off"]["min"]
    res["fused_minus_off_ms"], res["torch_minus_off_ms"] = b - a, c - a
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
