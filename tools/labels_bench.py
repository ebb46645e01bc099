"""Times step 1 of the synthetic data generation at the reference's shape: 8 ensembles of 128^3 with 39
seeded blob templates of about 150 x 120 x 200 each, every ensemble with the foreground mask and the envelope (ball 4) on.

    python tools/labels_bench.py [--out profiles/datagen_labels.json]

3 warm-up + 10 timed repetitions, timed with device events:
  * ``chain``  anatomix_amd.datagen.labels.generate_labels as the command line calls it: the host-side crop of the templates, their
               upload, the tables and every launch;
  * ``chain_device``  the launches alone, on tables and templates already on the device;
  * every stage alone, on the chain's own intermediates.
The comparison is the scipy calls the stages restate, on this machine's host, for ONE ensemble (``scipy_one_ensemble``): one
``affine_transform(order=0, mode='grid-wrap')`` of a padded template, ``median_filter(size=3, mode='nearest')`` of the labels,
``grey_dilation`` and ``grey_erosion`` with ball(4).  Where scipy does not import, that part is left out and the result says so.  The
deformed sphere has no scipy counterpart and is not compared."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _timing import TIMED, WARMUP, stats, timed            # noqa: E402
import _labels_ref as LR                                    # noqa: E402
from anatomix_amd.datagen import labels as L                # noqa: E402

B, S, NT = 8, 128, 39
SHAPE = (S, S, S)


def host_ms(fn, n=3):
    out = []
    for _ in range(n):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "n": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "datagen_labels.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    p = L.draw_params(np.random.RandomState(1), [NT] * B, S)
    p["mask"][:], p["envelope"][:], p["ball"][:] = True, True, 4
    pool = [LR.blob_template((150 + k % 7, 120 - k % 5, 200 + k % 3), 700 + k) for k in range(NT)]
    templates = [[pool[(k + b) % NT] for k in range(NT)] for b in range(B)]
    res = {"ensembles": [B, 1, S, S, S], "templates_per_ensemble": NT, "template_shape": list(pool[0].shape), "warmup": WARMUP, "timed": TIMED,
           "device": torch.cuda.get_device_name(dev)}
    with torch.cuda.device(dev):
        grids = L.draw_noise(p, dev)
        res["chain"] = stats(timed({"chain": lambda: L.generate_labels(templates, p, grids=grids)})["chain"])
        res["chain"]["ensembles_per_s"] = B / (res["chain"]["median_ms"] * 1e-3)
        tab, ens, buf = L._tables(templates, p, SHAPE)
        tab.device(dev), ens.device(dev)
        dbuf = torch.from_numpy(buf).to(dev)
        res["template_bytes"] = int(buf.size)

        def device_chain():
            lab = L._median(L._compose(tab, ens, dbuf, SHAPE, dev), ens, 0)
            mask = L._median(L._sphere(grids, ens, S, dev), ens, L.MASK)
            return L._envelope(lab, mask, L._apply(lab, mask, ens), ens)

        res["chain_device"] = stats(timed({"c": device_chain})["c"])
        res["chain_device"]["ensembles_per_s"] = B / (res["chain_device"]["median_ms"] * 1e-3)
        res["chain_device"]["ms_per_ensemble"] = res["chain_device"]["median_ms"] / B
        res["chain"]["ms_per_ensemble"] = res["chain"]["median_ms"] / B
        composed = L._compose(tab, ens, dbuf, SHAPE, dev)
        lab = L._median(composed, ens, 0)
        sphere = L._sphere(grids, ens, S, dev)
        mask = L._median(sphere, ens, L.MASK)
        applied = lab.clone()
        mx = L._apply(applied, mask, ens)
        # both in-place stages get a scratch copy of their own: apply adds 1 per repetition (uint8, so it wraps, which the timing does not
        # see), and the envelope runs on the labels the chain gives it, not on those
        work_apply, work_env = lab.clone(), applied.clone()
        stages = {"compose": lambda: L._compose(tab, ens, dbuf, SHAPE, dev), "median_labels": lambda: L._median(composed, ens, 0),
                  "sphere_mask": lambda: L._sphere(grids, ens, S, dev), "median_mask": lambda: L._median(sphere, ens, L.MASK),
                  "apply_mask": lambda: L._apply(work_apply, mask, ens), "envelope": lambda: L._envelope(work_env, mask, mx, ens)}
        res["stages"] = {k: stats(timed({k: fn})[k]) for k, fn in stages.items()}
        res["stages"]["sphere_mask"]["note"] = "includes the zero fill of its output"
    try:
        import scipy.ndimage as ndi
    except ImportError:
        res["scipy_one_ensemble"] = "scipy does not import on this machine: not measured"
    else:
        padded = LR.crop_and_pad(pool[0], SHAPE)
        lab0, mask0 = lab[0, 0].cpu().numpy(), mask[0, 0].cpu().numpy()
        ball = LR.ball(4)
        one = {"affine_transform": host_ms(lambda: ndi.affine_transform(padded, p["affine"][0][0], mode="grid-wrap", cval=0.0, order=0)),
               "median_filter": host_ms(lambda: ndi.median_filter(lab0, size=3, mode="nearest")),
               "grey_dilation_ball4": host_ms(lambda: ndi.grey_dilation(mask0, footprint=ball, mode="reflect")),
               "grey_erosion_ball4": host_ms(lambda: ndi.grey_erosion(mask0, footprint=ball, mode="reflect"))}
        one["chain_estimate_ms"] = (NT * one["affine_transform"]["median_ms"] + 2 * one["median_filter"]["median_ms"] +
                                    one["grey_dilation_ball4"]["median_ms"] + one["grey_erosion_ball4"]["median_ms"])
        one["cpu_count"] = os.cpu_count()
        res["scipy_one_ensemble"] = one
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
