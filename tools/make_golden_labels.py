"""Generates tests/golden/datagen_labels_golden.npz from the REFERENCE's ``crop_and_pad_3d_volume``,
``apply_random_affine_transform`` and ``sample_corruption`` (synthetic-data-generation/datagen_utils.py), on the seeded inputs of
tests/_labels_ref.py.  Run on the build machine only:
    python tools/make_golden_labels.py

``datagen_utils`` imports MONAI at module level, which is not installed; a stub ``monai.transforms`` whose names are placeholders is
put into ``sys.modules`` first (tools/make_golden_datagen.py does the same).  Nothing of the reference is written into this
repository; the fixture holds inputs, draws and outputs only:
  * ``affine/<i>/...``: a seeded blob template, the target size, the five draws of ``apply_random_affine_transform`` recovered by
    re-seeding numpy and replaying them, the 4 x 4 matrix they give, and the reference's output cut to the target size
    (``crop_and_pad_3d_volume`` + ``apply_random_affine_transform(mode='grid-wrap')``).  The crops are smaller than, equal to and larger
    than the target on different axes, with odd and even pads.
  * ``sphere/<S>/...``: radius and centre (numpy's draws replayed), per scale the coarse grid times its std (torch's draws replayed)
    and the negated output of ``sample_corruption`` as packed bits, for S = 16, 32 and 48.

The generator asserts what the tests rely on, and prints the share of voxels within the restatement's margins: the restatement
reproduces both reference functions voxel for voxel (outside the margins), and its median and morphology equal
``scipy.ndimage.median_filter``, ``grey_dilation`` and ``grey_erosion`` with the parameters skimage documents as its own."""
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndi
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _labels_ref as LR                                    # noqa: E402

REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "synthetic-data-generation")

TARGET = (12, 10, 9)
# template shapes (before the crop, which removes `margin` voxels of zeros per face) against the target (12, 10, 9)
AFFINE_CASES = [dict(shape=(7, 15, 9), margin=0, seed=11), dict(shape=(12, 9, 4), margin=0, seed=12), dict(shape=(17, 10, 8), margin=0, seed=13),
                dict(shape=(9, 9, 9), margin=2, seed=14), dict(shape=(13, 12, 11), margin=0, seed=15), dict(shape=(11, 5, 6), margin=1, seed=16)]
SPHERE_CASES = {16: 201, 32: 202, 48: 203}


def reference_module():
    monai = types.ModuleType("monai")
    tr = types.ModuleType("monai.transforms")
    for n in ("ScaleIntensityd", "Compose", "RandBiasFieldd", "RandAdjustContrastd", "RandGaussianSmoothd", "RandGaussianSharpend",
              "RandGibbsNoised", "RandKSpaceSpikeNoised", "RandSimulateLowResolutiond", "ThresholdIntensityd"):
        setattr(tr, n, None)
    monai.transforms = tr
    sys.modules["monai"], sys.modules["monai.transforms"] = monai, tr
    sys.path.insert(0, REF)
    import datagen_utils
    return datagen_utils


def replay_affine_draws(seed):
    """The five draws of apply_random_affine_transform after ``np.random.seed(seed)``, with its default ranges."""
    np.random.seed(seed)
    return dict(scale=np.random.uniform(0.5, 1.5, 3), rotation=np.random.uniform(-180, 180, 3), translation=np.random.uniform(-5, 5, 3),
                shear=np.random.uniform(-0.5, 0.5, 3), reflection=np.random.choice([True, False], 3))


def replay_sphere_draws(S, seed):
    """(radius, centre, grids) of sample_corruption(arrsize=(S, S, S), max_std=5.) after seeding numpy and torch with ``seed``."""
    q = S / 128
    np.random.seed(seed)
    radius = np.random.randint(round(48 * q), round(72 * q))
    centre = np.random.randint(-round(32 * q), round(32 * q), size=3)
    torch.manual_seed(seed)
    grids = []
    for scale in (8 * q, 16 * q, 32 * q):
        cn = int(np.ceil(S / scale))
        std = (5.0 * q - 1.0 * q) * torch.rand((1,), dtype=torch.float32) + 1.0 * q
        grids.append((std * torch.randn((3, cn, cn, cn), dtype=torch.float32)).numpy())
    return radius, centre, grids


def main():
    U = reference_module()
    from anatomix_amd.datagen.labels import affine_matrix
    out = {"affine/target": np.array(TARGET), "affine/count": np.array(len(AFFINE_CASES)), "sphere/sizes": np.array(list(SPHERE_CASES))}
    total = near_total = 0
    for i, c in enumerate(AFFINE_CASES):
        t = LR.blob_template(c["shape"], c["seed"], c["margin"])
        padded = U.crop_and_pad_3d_volume(t, TARGET)
        assert np.array_equal(padded, LR.crop_and_pad(t, TARGET)), i
        np.random.seed(c["seed"])
        ref = U.apply_random_affine_transform(padded, mode="grid-wrap")[:TARGET[0], :TARGET[1], :TARGET[2]]
        d = replay_affine_draws(c["seed"])
        # the matrix as the reference builds it, from the replayed draws
        sc = np.diag(np.where(d["reflection"], -d["scale"], d["scale"]))
        sh = np.eye(3)
        sh[np.triu_indices(3, k=1)] = d["shear"]
        m = np.eye(4)
        m[:3, :3] = sc @ U.get_rotation_matrix(d["rotation"]) @ sh
        m[:3, 3] = d["translation"]
        assert np.array_equal(m, affine_matrix(d["scale"], d["rotation"], d["translation"], d["shear"], d["reflection"])), i
        again = ndi.affine_transform(padded, m, mode="grid-wrap", cval=0.0, order=0)[:TARGET[0], :TARGET[1], :TARGET[2]]
        assert np.array_equal(again, ref), f"case {i}: the replayed draws do not give the reference's matrix"
        got, near = LR.affine_sample(padded, m, TARGET)
        assert np.array_equal(got[~near], ref[~near]), i
        lab, near2 = LR.compose([np.zeros((1, 1, 1), np.uint8) + 1, t], [np.eye(4), m], TARGET)
        assert np.array_equal(lab[~near2] > 0, ref[~near2] > 0), i
        total, near_total = total + near.size, near_total + int(near.sum())
        pads = [P - n for P, n in zip(padded.shape, LR.crop(t).shape)]
        print(f"affine {i}: crop {LR.crop(t).shape} padded {padded.shape} pads {pads}, {int((ref > 0).sum())} voxels set, {int(near.sum())} near a half-integer")
        out.update({f"affine/{i}/template": t, f"affine/{i}/matrix": m, f"affine/{i}/output": ref})
        out.update({f"affine/{i}/{k}": v for k, v in d.items()})
    print(f"compose: {near_total} of {total} voxels within {LR.COMPOSE_MARGIN} of a half-integer")
    for S, seed in SPHERE_CASES.items():
        grid = torch.from_numpy(U.generate_grid_unit((S, S, S)).astype(np.float32))
        np.random.seed(seed)
        torch.manual_seed(seed)
        ref = ~U.sample_corruption(grid, arrsize=(S,) * 3, max_std=5.0, device=torch.device("cpu")).type(torch.bool)
        ref = ref.numpy().squeeze().astype(np.uint8)
        radius, centre, grids = replay_sphere_draws(S, seed)
        got, near = LR.sphere_mask(radius, centre, grids, S)
        bad = int((got != ref)[~near].sum())
        print(f"sphere {S}: radius {radius} centre {centre.tolist()}, {int(ref.sum())} voxels set, {near.mean() * 100:.3f} % within "
              f"{LR.MASK_MARGIN} of a rounding boundary, {bad} mismatches outside, {int((got != ref).sum())} in all")
        assert bad == 0 and near.mean() <= LR.MAX_EXCLUDED, S
        out.update({f"sphere/{S}/radius": np.array(radius), f"sphere/{S}/centre": centre, f"sphere/{S}/mask": np.packbits(ref)})
        for j, g in enumerate(grids):
            out[f"sphere/{S}/grid_{j}"] = g
    # the stencils against the scipy calls skimage documents as its implementation
    r = np.random.RandomState(5)
    for shape in ((9, 11, 7), (12, 10, 9)):
        x = r.randint(0, 256, shape).astype(np.uint8)
        assert np.array_equal(LR.median3(x), ndi.median_filter(x, size=3, mode="nearest"))
        m = (r.uniform(size=shape) > 0.5).astype(np.uint8)
        assert np.array_equal(LR.median3_mask(m), ndi.median_filter(m, size=3, mode="nearest"))
    m = LR.blob_mask((12, 10, 9), 6)
    for rad in (2, 3, 4):
        assert np.array_equal(LR.dilate(m, rad), ndi.grey_dilation(m, footprint=LR.ball(rad), mode="reflect") > 0)
        assert np.array_equal(LR.erode(m, rad), ndi.grey_erosion(m, footprint=LR.ball(rad), mode="reflect") > 0)
    path = os.path.join(ROOT, "tests", "golden", "datagen_labels_golden.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
