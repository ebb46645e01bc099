"""Whole-volume sliding-window inference, the Python-scheduled route against the single C call, on one 256^3 volume with the 6 M
network at the reference's operating point (roi 128^3, overlap 0.8, gaussian, sigma_scale 0.25: 343 windows):

  features   sliding_window_inference(x, roi, 4, unet, ...)                      vs  sliding_window_volume(x, roi, unet, ...)
  labels     predict_labels(sliding_window_inference(x, roi, 4, Sequential(unet, head), ...))
                                                                                 vs  sliding_window_volume(..., head=head, out="labels")

The four routes alternate in one process after warm-up (tools/_timing.py: device events around each call, the call's own
synchronising range check included on both sides).  Prints one JSON line; --out also writes it to a file.

    python tools/sw_call_time.py [--size 256] [--roi 128] [--out profiles/sw_call_time.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _timing  # noqa: E402

import anatomix_amd  # noqa: E402
from anatomix_amd.registration.sliding_window import sliding_window_inference, sliding_window_volume, window_starts  # noqa: E402
from anatomix_amd.segmentation.losses import predict_labels  # noqa: E402
from oracle import unet_ref as R  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--roi", type=int, default=128)
    ap.add_argument("--classes", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    opt = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("sw_call_time: needs a GPU (a timing from anywhere else says nothing)")
    dev = torch.device("cuda:0")
    kw = R.VARIANTS["anatomix"]
    unet = anatomix_amd.Unet(**kw)
    unet.load_state_dict(R.synthetic_state_dict(kw, 0), strict=True)
    unet = unet.to(dev).eval()
    torch.manual_seed(0)
    head = torch.nn.Conv3d(kw["output_nc"], opt.classes, 1).to(dev).eval()
    full = torch.nn.Sequential(unet, head)
    size, roi = (opt.size,) * 3, (opt.roi,) * 3
    x = R.synthetic_input(7, 1, size).to(dev)
    sw = dict(overlap=0.8, mode="gaussian", sigma_scale=0.25)
    keep = {}

    def route(name, fn):
        def run():
            with torch.no_grad():
                keep[name] = fn()
        return run

    routes = {
        "features_python": route("features_python", lambda: sliding_window_inference(x, roi, 4, unet, **sw)),
        "features_call": route("features_call", lambda: sliding_window_volume(x, roi, unet, **sw)),
        "labels_python": route("labels_python", lambda: predict_labels(sliding_window_inference(x, roi, 4, full, **sw))),
        "labels_call": route("labels_call", lambda: sliding_window_volume(x, roi, unet, head=head, out="labels", **sw)),
    }
    ms = _timing.timed(routes)
    a, b = keep["features_python"], keep["features_call"]
    res = {"tool": "sw_call_time", "device": torch.cuda.get_device_name(0), "size": list(size), "roi": list(roi),
           "windows": len(window_starts(size, roi, 0.8)), "classes": opt.classes, "warmup": _timing.WARMUP,
           "features_rel_l2": float((a.double() - b.double()).norm() / a.double().norm()),
           "features_bit_identical": bool(torch.equal(a, b)),
           "labels_differing_voxels": int((keep["labels_python"] != keep["labels_call"]).sum()),
           **{k: _timing.stats(v) for k, v in ms.items()}}
    line = json.dumps(res)
    print(line)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(line + "\n")
    return res


if __name__ == "__main__":
    main()
