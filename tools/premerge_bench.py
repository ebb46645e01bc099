"""Times the merge of step 0 of the data generation at the size of a TotalSegmentator folder: 117 masks of 256 x 256 x 300 voxels
(2.3 GB of uint8), about a third of them ribs and vertebrae, a fifth blank.

  (i)   amx_labels_merge_masks alone, the batch already on the device: device events around the call, after warm-up; median and
        spread; achieved GB/s from the bytes the pass needs (every mask read once, the two merged rows written once);
  (ii)  premerge.merge_masks end to end from host arrays (staging copy, host -> device, launches, read-back): a host clock around
        a call that ends in a device synchronise;
  (iii) the yardstick, written here: the same sums in numpy on the same host (int64 accumulators, one mask at a time).

The three must agree exactly before anything is timed.  Needs a GPU.  Writes a JSON report (default profiles/premerge_bench.json).

    python tools/premerge_bench.py [--files 117] [--shape 256 256 300] [--reps 10] [--warmup 2] [--out profiles/premerge_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def folder(n, shape, rs):
    """n masks: boxes of ones (a structure fills a small part of the volume), every fifth blank; ribs and vertebrae in disjoint
    slabs of the first axis so that nothing overlaps."""
    vols, groups = [], []
    slab = max(shape[0] // n, 1)
    for i in range(n):
        v = np.zeros(shape, np.uint8)
        g = (1, 2, 0)[i % 3]
        if i % 5 != 4:
            lo = [int(rs.randint(0, max(s // 2, 1))) for s in shape]
            hi = [min(l + max(s // 6, 1), s) for l, s in zip(lo, shape)]
            if g:
                lo[0], hi[0] = (i * slab) % shape[0], min((i * slab) % shape[0] + slab, shape[0])
            v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
        vols.append(v)
        groups.append(g)
    return vols, groups


def numpy_merge(vols, groups):
    acc = np.zeros((2,) + vols[0].shape, np.int64)
    sums = []
    for v, g in zip(vols, groups):
        sums.append(int(v.sum(dtype=np.int64)))
        if g:
            acc[g - 1] += v
    return acc[0].astype(np.uint8), acc[1].astype(np.uint8), np.array(sums + [int(acc[0].sum()), int(acc[1].sum())], np.uint64)


def stats(ms):
    s = sorted(ms)
    n = len(s)
    return {"median_ms": s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2]), "min_ms": s[0], "max_ms": s[-1], "reps": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=117)
    ap.add_argument("--shape", type=int, nargs=3, default=[256, 256, 300])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "premerge_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("premerge_bench needs a GPU: a timing taken anywhere else says nothing about this kernel")
    from anatomix_amd import _lib
    from anatomix_amd.datagen import premerge
    dev = torch.device("cuda:0")
    shape = tuple(args.shape)
    n = args.files
    vols, groups = folder(n, shape, np.random.RandomState(0))
    voxels = int(np.prod(shape))
    stride = (voxels + 15) // 16 * 16

    # (iii) the yardstick, and the answer everything else must give
    host_ms = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        ref = numpy_merge(vols, groups)
        host_ms.append((time.perf_counter() - t0) * 1e3)

    # (ii) end to end
    e2e_ms = []
    for rep in range(args.warmup + args.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = premerge.merge_masks(vols, groups, dev, byte_budget=n * stride)
        torch.cuda.synchronize()
        if rep >= args.warmup:
            e2e_ms.append((time.perf_counter() - t0) * 1e3)
    assert all(np.array_equal(a, b) for a, b in zip(got, ref)), "merge_masks differs from numpy"

    # (i) the kernel alone
    lib = _lib.load()
    batch = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    for i, v in enumerate(vols):
        batch[i, :voxels] = torch.from_numpy(v.reshape(-1)).to(dev)
    merged = torch.empty((2, stride), dtype=torch.uint8, device=dev)
    dsum = torch.empty(n + 2, dtype=torch.int64, device=dev)
    flags = torch.empty(2, dtype=torch.int32, device=dev)
    grp = (ctypes.c_int * n)(*groups)

    def call():
        _lib.check(lib.amx_labels_merge_masks(_lib.ptr(batch), n, voxels, stride, grp, _lib.ptr(merged), _lib.ptr(dsum), _lib.ptr(flags), 0,
                                              _lib.stream(dev)))

    kernel_ms = []
    for rep in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            kernel_ms.append(e0.elapsed_time(e1))
    assert np.array_equal(dsum.cpu().numpy().view(np.uint64), ref[2]) and np.array_equal(merged[0, :voxels].cpu().numpy().reshape(shape), ref[0])

    nbytes = (n + 2) * voxels
    k, e, h = stats(kernel_ms), stats(e2e_ms), stats(host_ms)
    report = {"device": torch.cuda.get_device_name(0), "files": n, "shape": list(shape), "mask_bytes": n * voxels, "algorithmic_bytes": nbytes,
              "kernel": {**k, "GBps": nbytes / (k["median_ms"] * 1e-3) / 1e9},
              "merge_masks_end_to_end": {**e, "GBps": nbytes / (e["median_ms"] * 1e-3) / 1e9},
              "numpy_on_host": {**h, "GBps": nbytes / (h["median_ms"] * 1e-3) / 1e9}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))


if __name__ == "__main__":
    main()
