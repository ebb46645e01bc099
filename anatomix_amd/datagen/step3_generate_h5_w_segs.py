"""The command line of the reference's synthetic-data-generation/step3_generate_h5_w_segs.py without h5py or nibabel: the two views of
every label ensemble (``<view1_dir>/view1_<name>``, ``<view2_dir>/view2_<name>``, what step 2 wrote) and the ensemble itself
(``<seg_dir>/<name>``) packed into ``<out_dir>/train_data.hdf5`` and ``<out_dir>/val_data.hdf5`` -- what
``python -m anatomix_amd.pretraining.pretrain_anatomix --dataroot <out_dir>`` reads.  Per subject one group named ``"%06d"`` of its
index in the sorted view list, in it ``img`` uint8 [2, X, Y, Z] and ``seg`` uint8 [X, Y, Z]; the last ``--val_count`` subjects go to the
validation file under their global index.  The reference's flags, defaults and assertion messages are kept; ``--max_workers`` is new:
the gunzip of three files per subject dominates the run, so the files are decoded on a thread pool (at most 16 threads) while the
containers are written in order -- the output does not depend on it.  No GPU is used.  Files are read through ``io/nifti.py`` and
written through ``io/hdf5_write.py``."""
import argparse
import glob
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

MAX_THREADS = 16


def build_parser():
    parser = argparse.ArgumentParser(description="Generate HDF5 files with segmentations from synthesized NIfTI views.")
    parser.add_argument("--view1_dir", type=str, default="synthesized_views/view1", help="Path to directory containing view1 NIfTI files")
    parser.add_argument("--view2_dir", type=str, default="synthesized_views/view2", help="Path to directory containing view2 NIfTI files")
    parser.add_argument("--seg_dir", type=str, default="label_ensembles", help="Path to directory containing segmentation NIfTI files")
    parser.add_argument("--out_dir", type=str, default="./h5_w_segs/", help="Output directory for HDF5 files")
    parser.add_argument("--val_count", type=int, default=100, help="Number of validation samples (from the end)")
    parser.add_argument("--print_every", type=int, default=10, help="Print progress every print_every samples")
    parser.add_argument("--max_workers", type=int, default=None,
                        help="Threads that decode the NIfTI files (default: the CPU count, at most {})".format(MAX_THREADS))
    return parser


def load_subject(view1_path, view2_path, seg_dir):
    """-> (img uint8 [2, X, Y, Z], seg uint8 [X, Y, Z]) as the reference forms them: ``get_fdata().astype(np.uint8)`` of each file."""
    from ..io.nifti import load_nifti
    view1 = load_nifti(view1_path)[0].astype(np.uint8)
    view2 = load_nifti(view2_path)[0].astype(np.uint8)
    combo = np.stack((view1, view2), axis=0)
    seg_filename = os.path.basename(view1_path).split("view1_")[1]
    seg = load_nifti(os.path.join(seg_dir, seg_filename))[0].astype(np.uint8)
    return combo, seg


def _threads(max_workers):
    n = (os.cpu_count() or 1) if max_workers is None else int(max_workers)
    return max(1, min(MAX_THREADS, n))


def _in_order(pool, fn, items, ahead):
    """``fn(item)`` for every item, in order, with at most ``ahead`` results decoded in advance."""
    pending = deque()
    items = iter(items)
    try:
        for item in items:
            pending.append(pool.submit(fn, item))
            if len(pending) >= ahead:
                yield pending.popleft().result()
        while pending:
            yield pending.popleft().result()
    finally:
        for fut in pending:
            fut.cancel()


def _write_split(path, indices, view1s, view2s, seg_dir, pool, ahead, announce):
    from ..io.hdf5_write import H5Writer
    with H5Writer(path) as h5:
        decoded = _in_order(pool, lambda i: load_subject(view1s[i], view2s[i], seg_dir), indices, ahead)
        for idx, i in enumerate(indices):
            announce(idx, i)
            combo, seg = next(decoded)
            grp = h5.create_group("{:06}".format(i))
            grp["img"] = combo
            grp["seg"] = seg


def main(args=None):
    """The reference's ``main(args)``; ``args`` may also be an argument list (or None for ``sys.argv``)."""
    if args is None or isinstance(args, (list, tuple)):
        args = build_parser().parse_args(args)
    os.makedirs(args.out_dir, exist_ok=True)

    view1s = sorted(glob.glob(os.path.join(args.view1_dir, "*.nii.gz")))
    view2s = sorted(glob.glob(os.path.join(args.view2_dir, "*.nii.gz")))

    assert len(view1s) == len(view2s), "Number of view1 and view2 files must match"
    assert len(view1s) > 0, "No view1 files found"

    n_total = len(view1s)
    n_val = args.val_count
    assert 0 <= n_val < n_total, (
        f"--val_count must be in [0, {n_total}), got {n_val}. Only {n_total} "
        "view pairs were found, so this would leave no training samples."
    )
    n_train = n_total - n_val
    every = args.print_every
    threads = _threads(getattr(args, "max_workers", None))

    def training(idx, i):
        if i % every == 0:
            print(f"Processing training sample {i}/{n_train}")

    def validation(idx, i):
        if i % every == 0:
            print(f"Processing validation sample {idx}/{n_val} (global idx {i})")

    with ThreadPoolExecutor(max_workers=threads) as pool:
        _write_split(os.path.join(args.out_dir, "train_data.hdf5"), range(n_train), view1s, view2s, args.seg_dir, pool, 2 * threads, training)
        _write_split(os.path.join(args.out_dir, "val_data.hdf5"), range(n_train, n_total), view1s, view2s, args.seg_dir, pool, 2 * threads,
                     validation)


if __name__ == "__main__":
    main()
