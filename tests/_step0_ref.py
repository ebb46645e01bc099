"""numpy restatement of ``anatomix_amd.datagen.premerge.merge_masks`` (the arithmetic of
synthetic-data-generation/step0_preprocess_totalsegmentator.py:57-76 on uint8 masks), and the TotalSegmentator-shaped toy trees the
step-0 tests run on."""
import os

import numpy as np

from anatomix_amd.io.nifti import save_nifti

NEITHER, RIB, VERTEBRA = 0, 1, 2


def merge_masks(volumes, groups, device=None, byte_budget=None, name="the folder"):
    """-> (merged_ribs, merged_verts, sums uint64 [n + 2]); a merged voxel above 255 raises ValueError naming ``name``."""
    groups = [int(g) for g in groups]
    acc, sums, shape = None, [], None
    for v, g in zip(volumes, groups):
        v = np.asarray(v)
        assert v.dtype == np.uint8
        if acc is None:
            shape = v.shape
            acc = np.zeros((2,) + shape, np.int64)
        assert v.shape == shape
        sums.append(int(v.astype(np.int64).sum()))
        if g:
            acc[g - 1] += v
    assert len(sums) == len(groups)
    for g, what in ((0, "ribs"), (1, "vertebrae")):
        if acc[g].max() > 255:
            raise ValueError(f"{name}: a voxel of the merged {what} is above 255")
    return acc[0].astype(np.uint8), acc[1].astype(np.uint8), np.array(sums + [int(acc[0].sum()), int(acc[1].sum())], np.uint64)


def blob(shape, centre, radius, value=1):
    """An ellipsoid of ``value`` in a uint8 volume."""
    grid = np.ogrid[tuple(slice(0, n) for n in shape)]
    dist = sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, np.broadcast_to(radius, 3)))
    return (dist <= 1.0).astype(np.uint8) * np.uint8(value)


def subject_files(shape, seed):
    """{file name: uint8 mask} of one toy subject: disjoint ribs and vertebrae, blanks of every kind, organs."""
    r = np.random.RandomState(seed)
    d, h, w = shape
    files = {}
    for k in range(3):           # ribs in the low third of axis 0, vertebrae in the high third: nothing overlaps
        files[f"rib_left_{k + 1}.nii.gz"] = blob(shape, (d * 0.15, h * (0.2 + 0.3 * k), w * 0.3 + r.randint(0, 3)), (d * 0.1, h * 0.1, w * 0.2))
        files[f"vertebrae_L{k + 1}.nii.gz"] = blob(shape, (d * 0.85, h * (0.2 + 0.3 * k), w * 0.6 - r.randint(0, 3)), (d * 0.1, h * 0.12, w * 0.15))
    files["rib_right_1.nii.gz"] = np.zeros(shape, np.uint8)            # blank rib, blank vertebra, blank organ
    files["vertebrae_C1.nii.gz"] = np.zeros(shape, np.uint8)
    files["adrenal_gland_left.nii.gz"] = np.zeros(shape, np.uint8)
    files["liver.nii.gz"] = blob(shape, (d * 0.5, h * 0.5, w * 0.5), (d * 0.2, h * 0.3, w * 0.3))
    files["aorta.nii.gz"] = blob(shape, (d * 0.5, h * 0.3, w * 0.7), (d * 0.15, h * 0.1, w * 0.1))
    return files


def make_tree(root, shapes, seed=0):
    """``root/s%04d/{ct.nii.gz, segmentations/*.nii.gz}`` per shape -> {subject: (files, affine)}."""
    out = {}
    for i, shape in enumerate(shapes):
        sub = os.path.join(str(root), "s%04d" % i)
        os.makedirs(os.path.join(sub, "segmentations"))
        affine = np.diag([1.5, 1.5 + i, 2.0, 1.0])
        affine[:3, 3] = [-10.0 * (i + 1), 4.0, 7.5]
        save_nifti(os.path.join(sub, "ct.nii.gz"), np.zeros(shape, np.int16), affine=affine)
        files = subject_files(shape, seed + i)
        for k, (name, vol) in enumerate(sorted(files.items())):
            # only the first sorted file carries the subject's affine: the merged files must take theirs from it
            save_nifti(os.path.join(sub, "segmentations", name), vol, affine=affine if k == 0 else np.eye(4))
        out["s%04d" % i] = (files, affine)
    return out


def expected_after(files):
    """File names a processed ``segmentations`` folder holds, and its two merged volumes."""
    keep = sorted(n for n, v in files.items() if v.any() and "rib_" not in n and "vertebrae_" not in n)
    ribs = sum(v.astype(np.int64) for n, v in files.items() if "rib_" in n).astype(np.uint8)
    verts = sum(v.astype(np.int64) for n, v in files.items() if "vertebrae_" in n).astype(np.uint8)
    return sorted(keep + ["all_ribs.nii.gz", "all_vertebrae.nii.gz"]), ribs, verts
