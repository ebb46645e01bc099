"""The timing loop of the augmentation benches (seg_augment_bench.py, pretrain_augment_bench.py, datagen_bench.py)."""
import numpy as np
import torch

WARMUP, TIMED = 3, 10


def timed(routes):
    """routes: {name: callable}.  Alternates them, WARMUP + TIMED times each -> {name: [ms] * TIMED}."""
    out = {k: [] for k in routes}
    for it in range(WARMUP + TIMED):
        for k, fn in routes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= WARMUP:
                out[k].append(a.elapsed_time(b))
    return out


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "n": len(ms)}
