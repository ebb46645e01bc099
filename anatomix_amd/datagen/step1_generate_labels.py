"""The command line of the reference's synthetic-data-generation/step1_generate_labels.py on the device: ``n_ensembles`` label
ensembles of ``side_length``^3 from the template files ``<templatedir>/**/segmentations/*.nii.gz``, written as
``<savedir>/<identifier>_shapes<n>_<7 chars of A-Z0-9>.nii.gz``, uint8 with the identity affine -- what
``python -m anatomix_amd.datagen.step2_generate_views --ensembledir <savedir>`` reads.  The reference's flags are kept
(``--max_workers`` is accepted and has no meaning here: a batch of ensembles is one set of launches); ``--batch_size``, ``--seed`` and
``--device`` are new.  Ensemble i draws everything from its own ``numpy.random.RandomState([seed, i])`` -- ``labels.draw_params``
first, then per template ``randint(number of files)`` until the file is not empty, then the 7 characters of the name (drawn again
while the name exists) -- and its noise from a generator seeded by them, so an ensemble does not depend on the batch it is generated in."""
import argparse
import os
import string
from glob import glob

import numpy as np

ALPHABET = string.ascii_uppercase + string.digits


def build_parser():
    parser = argparse.ArgumentParser(description="Generate 3D label ensembles on the GPU")
    parser.add_argument("--n_ensembles", type=int, default=120000, help="Number of 3D label ensemble volumes to generate")
    parser.add_argument("--min_templates", type=int, default=20, help="Minimum number of shapes to include in each ensemble")
    parser.add_argument("--max_templates", type=int, default=40, help="Maximum number of shapes to include in each ensemble")
    parser.add_argument("--side_length", type=int, default=128, help="Side length of the generated volumes")
    parser.add_argument("--templatedir", type=str, default="./Totalsegmentator_dataset/", help="Path to unzipped and preprocessed TotalSegmentator data")
    parser.add_argument("--savedir", type=str, default="./label_ensembles/", help="Directory to save the generated label ensembles")
    parser.add_argument("--max_workers", type=int, default=None, help="Accepted for compatibility; the device processes a batch per launch")
    parser.add_argument("--batch_size", type=int, default=8, help="Ensembles generated together")
    parser.add_argument("--seed", type=int, default=0, help="Base seed; ensemble i draws from RandomState([seed, i])")
    parser.add_argument("--device", type=str, default="cuda:0", help="The GPU to run on (there is no host path)")
    return parser


def template_files(templatedir):
    """The reference's glob, sorted so that a seed names the same files on every machine."""
    return sorted(glob(templatedir + "/**/segmentations/*.nii.gz", recursive=True))


def file_name(identifier, n_templates, suffix):
    return "{}_shapes{}_{}.nii.gz".format(identifier, n_templates, suffix)


def draw_suffix(rng):
    return "".join(ALPHABET[i] for i in rng.randint(0, len(ALPHABET), 7))


def draw_templates(rng, files, n, cache, empty):
    """n non-empty templates: ``files[rng.randint(len(files))]``, drawn again while the file holds no non-zero voxel.  ``cache`` keeps
    the volumes of up to 256 files (the oldest leaves first), ``empty`` the files found empty; when that is every file, an error."""
    from ..io.nifti import load_nifti
    out = []
    while len(out) < n:
        path = files[rng.randint(len(files))]
        if path in empty:
            continue
        if path not in cache:
            vol = load_nifti(path)[0].astype(np.uint8)      # as the reference: values of 256 and above wrap
            if not vol.any():
                empty.add(path)
                if len(empty) == len(files):
                    raise ValueError("every template file is empty: nothing to compose")
                continue
            if len(cache) >= 256:
                cache.pop(next(iter(cache)))
            cache[path] = vol
        out.append(cache[path])
    return out


def run(segs, n_vols, min_shapes, max_shapes, savedir, sidelen=128, max_workers=None, batch_size=8, seed=0, device="cuda:0"):
    """The reference's ``main`` with its parameters; ``max_workers`` is ignored.  -> the paths written, in order."""
    import torch
    from ..io.nifti import save_nifti
    from . import labels as L
    assert len(segs) > 0
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"--device: a GPU (got {device}); the data generation has no host path")
    os.makedirs(savedir, exist_ok=True)
    cache, empty, written = {}, set(), []

    def flush(batch):
        if not batch:
            return
        params = L.concat_params([q for _, q, _ in batch])
        out, names = L.generate_labels([t for _, _, t in batch], params, device=dev)
        out = out.cpu().numpy()
        for (rng, q, _), vol, identifier in zip(batch, out, names):
            path = os.path.join(savedir, file_name(identifier, int(q["n_templates"][0]), draw_suffix(rng)))
            while os.path.isfile(path):
                path = os.path.join(savedir, file_name(identifier, int(q["n_templates"][0]), draw_suffix(rng)))
            print("chose {}".format(identifier))
            save_nifti(path, vol[0], affine=np.eye(4), dtype=np.uint8)
            written.append(path)

    batch = []
    for idx in range(n_vols):
        print("Synthesizing ensemble {:05d} with seed [{}, {}]".format(idx + 1, seed, idx))
        rng = np.random.RandomState([seed, idx])
        params = L.draw_params(rng, [(min_shapes, max_shapes)], sidelen)
        batch.append((rng, params, draw_templates(rng, segs, int(params["n_templates"][0]), cache, empty)))
        if len(batch) >= batch_size:
            flush(batch)
            batch = []
    flush(batch)
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch_size < 1:
        raise SystemExit("--batch_size must be at least 1")
    run(template_files(args.templatedir), args.n_ensembles, args.min_templates, args.max_templates, args.savedir, sidelen=args.side_length,
        max_workers=args.max_workers, batch_size=args.batch_size, seed=args.seed, device=args.device)


if __name__ == "__main__":
    main()
