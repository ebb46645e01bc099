"""The command line of the reference's synthetic-data-generation/step0_preprocess_totalsegmentator.py with the merge on the device: in an
unzipped TotalSegmentator v1 dataset, the CT volumes are deleted, and in every ``<subject>/segmentations`` folder the blank label
files are deleted, the ``rib_*`` and ``vertebrae_*`` files are added into ``all_ribs.nii.gz`` / ``all_vertebrae.nii.gz`` (uint8, with
the affine of the folder's first file, written only when not blank) and the individual rib and vertebra files are deleted -- the
tree ``python -m anatomix_amd.datagen.step1_generate_labels --templatedir`` expects.  The reference's three functions and two flags
are kept (``--max_workers`` is accepted and has no meaning here: a folder is a few launches); ``--device`` is new.  A second run over a
processed tree changes nothing.

The emptiness test of every file and both merges are one pass over the masks on the device (``premerge.merge_masks``,
csrc/amx_labels.hip).  Narrower than the reference, and said aloud: a mask must hold integers in 0 .. 255 and every file of a
folder must have one shape -- otherwise the call raises naming the file -- and a merged voxel above 255 raises naming the folder,
where ``astype(np.uint8)`` of the reference's float sum would wrap.  nibabel is not a dependency: files go through ``io/nifti.py``."""
import argparse
import os
from glob import glob

import numpy as np


def build_parser():
    parser = argparse.ArgumentParser(description="")
    parser.add_argument("--totalsegmentator_path", type=str, default="./Totalsegmentator_dataset/", help="Path to unzipped TotalSegmentator v1 dataset")
    parser.add_argument("--max_workers", type=int, default=None, help="Accepted for compatibility; the device merges a folder in a few launches")
    parser.add_argument("--device", type=str, default="cuda:0", help="The GPU to run on (there is no host path)")
    return parser


def delete_ct_images(basedir):
    """Deletes ``<basedir>/<subject>/ct.nii.gz``: only the segmentations are used.  (The reference's glob, ``**`` without
    ``recursive=True``: one directory level.)"""
    cts = sorted(glob(basedir + "/**/ct.nii.gz"))
    if len(cts) == 0:      # the script has run before
        return
    print("Deleting CT intensity volumes...")
    for ct in cts:
        os.remove(ct)
    print("Done deleting.")


def load_mask(fpath, shape=None):
    """A label file as uint8, or the error of a file this step does not cover -> (mask, affine)."""
    from ..io.nifti import load_nifti
    data, affine, _ = load_nifti(fpath)
    if shape is not None and data.shape != shape:
        raise ValueError(f"{fpath}: shape {data.shape} differs from the folder's first file ({shape})")
    if not (np.isfinite(data).all() and (data == np.rint(data)).all()):
        raise ValueError(f"{fpath}: a mask must hold integers (found a fractional or non-finite voxel)")
    if data.size and (data.min() < 0 or data.max() > 255):
        raise ValueError(f"{fpath}: a mask must hold values in 0 .. 255 (found {data.min():g} .. {data.max():g})")
    return data.astype(np.uint8), affine


def merge_vertebrae_and_ribs_worker(segdir, device="cuda:0"):
    """Deletes the blank label files of ``segdir`` and writes its merged rib and vertebra volumes."""
    from ..io.nifti import save_nifti
    from . import premerge
    print(f"Merging labels in {segdir}")
    fpaths = sorted(glob(segdir + "/*.nii.gz"))
    if not fpaths:
        print(f"No label files in {segdir}")
        return
    groups = [premerge.group_of(os.path.basename(p)) for p in fpaths]
    meta = {}

    def masks():
        for fpath in fpaths:
            mask, affine = load_mask(fpath, meta.get("shape"))
            if not meta:
                meta.update(shape=mask.shape, affine=affine)      # the first sorted file supplies both
            yield mask

    ribs, verts, sums = premerge.merge_masks(masks(), groups, device, name=segdir)
    for fpath, total in zip(fpaths, sums[:len(fpaths)]):
        if total == 0:
            # TotalSegmentator includes blank label files for structures that are not present
            os.remove(fpath)
    if sums[len(fpaths)] > 0:
        save_nifti(segdir + "/all_ribs.nii.gz", ribs, affine=meta["affine"], dtype=np.uint8)
    if sums[len(fpaths) + 1] > 0:
        save_nifti(segdir + "/all_vertebrae.nii.gz", verts, affine=meta["affine"], dtype=np.uint8)


def merge_vertebrae_and_ribs(basedir, max_workers=None, device="cuda:0"):
    """The worker over every ``<basedir>/<subject>/segmentations/``; ``max_workers`` is ignored."""
    segdirs = sorted(glob(basedir + "/**/segmentations/"))
    for segdir in segdirs:
        merge_vertebrae_and_ribs_worker(segdir, device=device)


def delete_individual_vertebrae_and_ribs(basedir):
    ribs = sorted(glob(basedir + "/**/segmentations/rib_*.nii.gz"))
    verts = sorted(glob(basedir + "/**/segmentations/vertebrae_*.nii.gz"))
    rmfiles = ribs + verts
    print("Deleting individualized rib and vertebral label files")
    for rmfile in rmfiles:
        os.remove(rmfile)


def main(argv=None):
    args = build_parser().parse_args(argv)
    delete_ct_images(args.totalsegmentator_path)
    merge_vertebrae_and_ribs(args.totalsegmentator_path, args.max_workers, device=args.device)
    delete_individual_vertebrae_and_ribs(args.totalsegmentator_path)
    print("All ready to synthesize label ensembles.")


if __name__ == "__main__":
    main()
