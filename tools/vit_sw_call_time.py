"""Whole-volume sliding-window inference of the 3D ViT (`anatomix-dev-vit`, synthetic weights) on one volume at the reference's
operating point (roi 128^3, overlap 0.8, gaussian, sigma_scale 0.25: 343 windows at 256^3), three routes in one process:

  generic   sliding_window_inference(x, roi, 4, lambda w: vit(w), ...)   the generic window loop (torch.cat of the window slices,
                                                                         `acc += wmap * pred` per window) -- the only route before
                                                                         amx_vit_forward_windows existed
  routed    sliding_window_inference(x, roi, 4, vit, ...)                amx_vit_forward_windows per batch of 4, Python schedule
  call      sliding_window_volume(x, roi, vit, ...)                      amx_vit_sliding_window, one C call

Device events around each call, the routes alternating, 1 warm-up and 3 timed rounds.  Prints one JSON line; --out also writes it.

    python tools/vit_sw_call_time.py [--size 256] [--depth 12] [--out profiles/vit_sw_call_time.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _timing  # noqa: E402

from anatomix_amd.model.vit3d import PrimusV2  # noqa: E402
from anatomix_amd.registration.sliding_window import sliding_window_inference, sliding_window_volume, window_starts  # noqa: E402
from oracle import vit_ref as V  # noqa: E402

WARMUP, TIMED = 1, 3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--depth", type=int, default=None, help="EVA blocks (default: the variant's)")
    ap.add_argument("--out", type=str, default=None)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("vit_sw_call_time: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda:0")
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"])
    if opt.depth is not None:
        kw["eva_depth"] = opt.depth
    vit = PrimusV2(**kw)
    vit.load_state_dict(V.synthetic_state_dict(kw, 0), strict=True)
    vit = vit.to(dev).eval()
    roi, size = tuple(kw["input_shape"]), (opt.size,) * 3
    x = V.synthetic_input(7, 1, size).to(dev)
    sw = dict(overlap=0.8, mode="gaussian", sigma_scale=0.25)
    keep = {}

    def route(name, fn):
        def run():
            with torch.no_grad():
                keep[name] = None                  # one result volume alive at a time
                keep[name] = fn()
        return run

    routes = {
        "generic": route("generic", lambda: sliding_window_inference(x, roi, 4, lambda w: vit(w), **sw)),
        "routed": route("routed", lambda: sliding_window_inference(x, roi, 4, vit, **sw)),
        "call": route("call", lambda: sliding_window_volume(x, roi, vit, **sw)),
    }
    ms = {k: [] for k in routes}
    for it in range(WARMUP + TIMED):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= WARMUP:
                ms[k].append(a.elapsed_time(b))
    windows = len(window_starts(size, roi, 0.8))
    ref = keep["generic"].double()
    res = {"tool": "vit_sw_call_time", "device": torch.cuda.get_device_name(0), "size": list(size), "roi": list(roi), "depth": kw["eva_depth"],
           "windows": windows, "warmup": WARMUP,
           "routed_rel_l2": float((keep["routed"].double() - ref).norm() / ref.norm()),
           "call_rel_l2": float((keep["call"].double() - ref).norm() / ref.norm()),
           **{k: dict(_timing.stats(v), windows_per_s=windows / (sorted(v)[len(v) // 2] * 1e-3)) for k, v in ms.items()}}
    line = json.dumps(res)
    print(line)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
