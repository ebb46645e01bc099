"""The command line of the reference's synthetic-data-generation/step2_generate_views.py on the device: every label ensemble
``<ensembledir>/*.nii.gz`` with index in [start_idx, end_idx) becomes ``<savedir>/view1/view1_<name>`` and
``<savedir>/view2/view2_<name>``, uint8 with the identity affine.  The reference's flags are kept (``--max_workers`` is accepted and
has no meaning here: a batch of label maps is one set of launches); ``--batch_size``, ``--seed`` and ``--device`` are new.  Every
volume draws its parameters from its own ``numpy.random.RandomState([seed, index])`` and its noise from a generator seeded by them, so a
volume does not depend on the batch it is generated in."""
import argparse
import os
from glob import glob

import numpy as np


def build_parser():
    parser = argparse.ArgumentParser(description="Generate two paired synthetic views per label ensemble on the GPU")
    parser.add_argument("--start_idx", type=int, default=0, help="Starting index of list of label ensemble files to process")
    parser.add_argument("--end_idx", type=int, default=120000, help="Ending index of list of label ensemble files to process")
    parser.add_argument("--ensembledir", type=str, default="./label_ensembles/", help="Path to where the synthetic label ensembles are saved")
    parser.add_argument("--savedir", type=str, default="./synthesized_views/", help="Path to save synthesized volumes to")
    parser.add_argument("--max_workers", type=int, default=3, help="Accepted for compatibility; the device processes a batch per launch")
    parser.add_argument("--batch_size", type=int, default=8, help="Label maps of one shape generated together")
    parser.add_argument("--seed", type=int, default=0, help="Base seed; volume i draws from RandomState([seed, i])")
    parser.add_argument("--device", type=str, default="cuda:0", help="The GPU to run on (there is no host path)")
    return parser


def load_label_map(path):
    """A label ensemble as uint8 [D, H, W] with its sorted distinct labels; non-integer labels and labels above 255 are refused."""
    from ..io.nifti import load_nifti
    data = load_nifti(path)[0]
    if data.ndim != 3:
        raise ValueError(f"{path}: a 3-D label map (got shape {data.shape})")
    if not np.all(data == np.round(data)) or data.min() < 0 or data.max() > 255:
        raise ValueError(f"{path}: labels must be integers in 0 .. 255")
    lab = data.astype(np.uint8)
    return lab, np.unique(lab)


def run(idx_start, idx_end, savedir, label_fpaths="./label_ensembles/", means_range=(25, 255), stds_range=(5, 20),
        perl_scales=(4, 8, 16, 32), perl_max_std=5.0, perl_mult_factor=0.02, max_workers=None, batch_size=8, seed=0, device="cuda:0"):
    """The reference's ``run`` with its parameters; ``max_workers`` is ignored."""
    import torch
    from ..io.nifti import save_nifti
    from . import views as V
    labs = sorted(glob(label_fpaths + "/*.nii.gz"))
    assert len(labs) > 0
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"--device: a GPU (got {device}); the data generation has no host path")
    os.makedirs("{}/view1/".format(savedir), exist_ok=True)
    os.makedirs("{}/view2/".format(savedir), exist_ok=True)
    todo = list(enumerate(labs))[idx_start:idx_end]

    def flush(batch):
        if not batch:
            return
        params = V.concat_params([q for _, _, q in batch])
        lab = torch.from_numpy(np.stack([l for _, l, _ in batch])[:, None]).to(dev)
        out = V.generate_views(lab, params, dtype=torch.uint8).cpu().numpy()
        for (path, _, _), pair in zip(batch, out):
            for v in range(2):
                save_nifti("{}/view{}/view{}_{}".format(savedir, v + 1, v + 1, os.path.basename(path)), pair[v], affine=np.eye(4), dtype=np.uint8)

    batch = []
    for idx, path in todo:
        print("Synthesizing ensemble {} with seed [{}, {}]".format(os.path.basename(path), seed, idx))
        lab, unique = load_label_map(path)
        if batch and (len(batch) >= batch_size or batch[0][1].shape != lab.shape):
            flush(batch)
            batch = []
        params = V.draw_params(np.random.RandomState([seed, idx]), [unique], lab.shape, scales=perl_scales, perl_max_std=perl_max_std,
                               perl_mult_factor=perl_mult_factor, means_range=means_range, stds_range=stds_range)
        batch.append((path, lab, params))
    flush(batch)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    run(args.start_idx, args.end_idx, savedir=args.savedir, label_fpaths=args.ensembledir, max_workers=args.max_workers,
        batch_size=args.batch_size, seed=args.seed, device=args.device)


if __name__ == "__main__":
    main()
