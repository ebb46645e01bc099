"""The device part of step 0 of the reference's data generation (synthetic-data-generation/step0_preprocess_totalsegmentator.py:57-76):
of the mask files of one TotalSegmentator ``segmentations`` folder, which are blank (``segdata.sum() == 0``), and the two merged
volumes (``rib_labels += segdata``, ``vert_labels += segdata``) -- one pass over the masks, ``amx_labels_merge_masks`` of
csrc/amx_labels.hip, one launch per batch of files staged under a byte budget.  Integer sums: bit-exact and reproducible.

There is no host path: a CPU device, other dtypes and shapes outside the envelope raise ``AmxEnvelopeError`` before anything is launched."""
from __future__ import annotations

import ctypes

import numpy as np

from .. import _lib

NEITHER, RIB, VERTEBRA = 0, 1, 2
MAX_FILES_PER_LAUNCH = 256                  # include/anatomix_amd.h: AMX_LABELS_MAX_MERGE
DEFAULT_BYTE_BUDGET = 1 << 30


def group_of(basename):
    """The reference's two substring tests on a file's basename.  (A name with both would be added to both volumes there; here it
    is refused, since a batch entry has one group.)"""
    rib, vert = "rib_" in basename, "vertebrae_" in basename
    if rib and vert:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_INVALID, f"{basename}: names a rib and a vertebra at once")
    return RIB if rib else VERTEBRA if vert else NEITHER


def _refuse(msg, code=_lib.AMX_ERR_SHAPE):
    raise _lib.AmxEnvelopeError(code, msg)


def _check_volume(v, i, shape):
    if not isinstance(v, np.ndarray) or v.dtype != np.uint8:
        _refuse(f"mask {i}: a uint8 numpy array (got {type(v).__name__}{'' if not isinstance(v, np.ndarray) else ' of ' + str(v.dtype)})",
                _lib.AMX_ERR_INVALID)
    if v.size < 1 or v.size >= 2 ** 31:
        _refuse(f"mask {i}: 1 <= voxels < 2^31 (got shape {v.shape})")
    if shape is not None and v.shape != shape:
        _refuse(f"mask {i}: shape {v.shape} differs from the first mask's {shape}")
    return v


def merge_masks(volumes, groups, device, byte_budget=DEFAULT_BYTE_BUDGET, name="the folder"):
    """``volumes``: the masks of one folder, uint8 arrays of one shape (a sequence, or an iterable that yields them one by one so that
    a folder never sits in memory; a sequence is checked as a whole before the first launch, an iterable as its masks arrive).
    ``groups``: per mask NEITHER, RIB or VERTEBRA.  ``byte_budget``: device bytes of one staged batch of masks.
    -> (merged_ribs, merged_verts, sums): the two merged uint8 volumes and uint64 [n + 2], the voxel sum of every mask followed by the
    sums of the two merged volumes.  A merged voxel above 255 raises ``ValueError`` naming ``name``."""
    import torch
    groups = [int(g) for g in groups]
    n = len(groups)
    dev = torch.device(device)
    if dev.type != "cuda":
        _refuse(f"device: a GPU (got {device}); the merge has no host path", _lib.AMX_ERR_INVALID)
    if n < 1:
        _refuse("at least one mask")
    if any(g not in (NEITHER, RIB, VERTEBRA) for g in groups):
        _refuse(f"groups: {NEITHER} (neither), {RIB} (rib) or {VERTEBRA} (vertebra) (got {sorted(set(groups))})", _lib.AMX_ERR_INVALID)
    if int(byte_budget) < 1:
        _refuse(f"byte_budget must be positive (got {byte_budget})", _lib.AMX_ERR_INVALID)
    if isinstance(volumes, (list, tuple)):
        if len(volumes) != n:
            _refuse(f"{len(volumes)} masks for {n} groups", _lib.AMX_ERR_INVALID)
        for i, v in enumerate(volumes):
            _check_volume(v, i, volumes[0].shape if i else None)
    lib = _lib.load()

    shape = voxels = stride = per = host = merged = flags = None
    sums = np.zeros(n + 2, np.uint64)
    start, rows = 0, 0

    def launch():
        nonlocal start, rows
        batch = torch.from_numpy(host[:rows]).to(dev)
        dsum = torch.empty(rows + 2, dtype=torch.int64, device=dev)
        grp = (ctypes.c_int * rows)(*groups[start:start + rows])
        _lib.check_envelope(lib.amx_labels_merge_masks(_lib.ptr(batch), rows, voxels, stride, grp, _lib.ptr(merged), _lib.ptr(dsum),
                                                       _lib.ptr(flags), 1 if start else 0, _lib.stream(dev)))
        got = dsum.cpu().numpy().view(np.uint64)            # (the copy also keeps `batch` alive until the launch is done)
        sums[start:start + rows] = got[:rows]
        sums[n:] = got[rows:]
        start, rows = start + rows, 0

    count = 0
    for i, v in enumerate(volumes):
        if i >= n:
            _refuse(f"more masks than the {n} groups", _lib.AMX_ERR_INVALID)
        _check_volume(v, i, shape)
        if shape is None:
            shape, voxels = v.shape, int(v.size)
            stride = (voxels + 15) // 16 * 16
            per = max(1, min(MAX_FILES_PER_LAUNCH, n, int(byte_budget) // stride))
            host = np.zeros((per, stride), np.uint8)
            merged = torch.empty((2, stride), dtype=torch.uint8, device=dev)
            flags = torch.empty(2, dtype=torch.int32, device=dev)
        host[rows, :voxels] = v.reshape(-1)
        rows, count = rows + 1, count + 1
        if rows == per:
            launch()
    if count != n:
        _refuse(f"{count} masks for {n} groups", _lib.AMX_ERR_INVALID)
    if rows:
        launch()
    over = flags.cpu().numpy()
    for g, what in ((0, "ribs"), (1, "vertebrae")):
        if over[g]:
            raise ValueError(f"{name}: a voxel of the merged {what} is above 255 (the masks overlap); uint8 cannot hold it")
    out = merged.cpu().numpy()
    return out[0, :voxels].reshape(shape), out[1, :voxels].reshape(shape), sums
