"""The Dice score the reference's registration driver reports (run_convex_adam_with_network_feats.py:283-295), from label counts
taken on the device by ``amx_label_overlap`` (csrc/amx_regmetrics.hip) instead of copying both label maps to the host for
``sklearn.metrics.f1_score``.  The counts are exact integers; the score is formed from them in double on the host."""
from __future__ import annotations

import torch

from .. import _lib

_DTYPES = {torch.float32: "float32", torch.int64: "int64", torch.uint8: "uint8"}


def _labels(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"{what}: the label-overlap kernel runs on the GPU (got {getattr(t, 'device', type(t).__name__)}); there is no CPU path")
    if t.dtype not in _DTYPES:
        raise ValueError(f"{what}: labels must be float32, uint8 or int64 (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


def _overlap(a, b, bins):
    bins = int(bins)
    if not 1 <= bins <= 1024:
        raise ValueError(f"label_overlap: 1 <= bins <= 1024 (got {bins})")
    a, b = _labels(a, "label_overlap"), _labels(b, "label_overlap")
    if a.numel() != b.numel() or a.numel() < 1:
        raise ValueError(f"label_overlap: the volumes hold {a.numel()} and {b.numel()} voxels")
    out = torch.empty(3 * bins + 1, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.load().amx_label_overlap(_lib.ptr(a), _lib.SEG_LABEL[_DTYPES[a.dtype]], _lib.ptr(b),
                                                 _lib.SEG_LABEL[_DTYPES[b.dtype]], a.numel(), bins, _lib.ptr(out),
                                                 _lib.ptr(out[3 * bins:]), _lib.stream(a.device)))
    return out[:3 * bins].view(bins, 3), out[3 * bins:]


def label_overlap(a, b, bins=1024):
    """Counts [bins, 3] (int64, on the device) = {#(a == l), #(b == l), #(a == l and b == l)} for the labels l in [0, bins) of two
    device tensors of float32, uint8 or int64 labels, of any shape with equal element counts.  Raises ValueError when a voxel of
    either volume is not an integer in [0, bins): sklearn rejects fractional labels, and so does this."""
    counts, bad = _overlap(a, b, bins)
    nbad = int(bad.item())
    if nbad:
        raise ValueError(f"label_overlap: {nbad} voxels hold a value that is not an integer label in [0, {int(bins)})")
    return counts


def dice_from_counts(counts):
    """``f1_score(fixed, moved, average='macro', labels=np.unique(fixed).astype(int).tolist()[1:])`` from the counts of
    ``label_overlap(fixed, moved)``: the labels are the bins that occur in the fixed map with the smallest one dropped, the score
    of a label is 2 both / (#fixed + #moved), and the result their mean.  Returns (macro, {label: score})."""
    rows = counts.tolist()
    labels = [l for l, r in enumerate(rows) if r[0] > 0][1:]
    if not labels:
        raise ValueError("dice_score: no label is left after dropping the smallest label of the fixed map")
    per = {l: 2.0 * rows[l][2] / float(rows[l][0] + rows[l][1]) for l in labels}
    return sum(per.values()) / len(per), per


def dice_score(fixed_seg, moved_seg):
    """The driver's Dice between the fixed label map and the warped moving one (both device tensors, see ``label_overlap``)."""
    return dice_from_counts(label_overlap(fixed_seg, moved_seg).cpu())
