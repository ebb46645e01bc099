"""Generates tests/golden/datagen_golden.npz from the REFERENCE's ``sample_gmm`` and ``draw_perlin_volume``
(synthetic-data-generation/datagen_utils.py), on the seeded label maps of tests/_datagen_ref.py.  Run on the build machine only:
    python tools/make_golden_datagen.py

``datagen_utils`` imports MONAI at module level, which is not installed; a stub ``monai.transforms`` whose names are placeholders is
put into ``sys.modules`` first (only ``get_transforms`` would use them, and it is not called).  Nothing of the reference is written
into this repository; the fixture holds inputs and outputs only.  Per case:
  * the label map (uint8), ``means`` and ``stds`` (float32, drawn as step2_generate_views.py:82-94 draws them), the zero-background
    flag (forced through ``zero_bckgnd`` = 1 or 0) and the torch seed;
  * ``z``: the noise field recovered by re-seeding and replaying ``sample_gmm``'s draws (one ``rand(1)`` at the first label, one
    ``randn(count)`` per label that is not skipped), and ``gmm``: the reference's output;
  * ``grid_<s>``: per scale the coarse grid times its drawn std, recovered by replaying ``draw_perlin_volume``'s draws, and ``perlin``: the
    reference's output; ``view`` = gmm * (1 + 0.02 * perlin) as step2_generate_views.py:115 forms it.
The 32 x 64 x 96 case would not fit the size limit of a committed file with three float32 volumes in it: it stores the reference's
outputs at 8192 seeded voxel indices (``index``) and ``z`` at the same indices; the tests replay the full ``z`` from the seed with
tests/_datagen_ref.py::replay_noise (torch's CPU generator) and check it against the stored values.

The generator asserts what the tests rely on: the replayed draws reproduce the reference's outputs bit for bit when pushed through the
same torch expressions, and the float64 restatement agrees with the reference to 2e-6 of its maximum."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _datagen_ref as DR                                   # noqa: E402

REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "synthetic-data-generation")

MANY = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 255] + list(range(100, 130))        # 44 labels, non-contiguous, with 255
CASES = {
    "big": dict(shape=(32, 64, 96), scales=(4, 8, 16, 32), labels=MANY, zero_background=False, seed=101, sampled=8192),
    "mid": dict(shape=(8, 16, 24), scales=(2, 4, 8), labels=[0, 3, 7, 200, 255], zero_background=True, seed=102, sampled=0),
    "odd": dict(shape=(3, 6, 9), scales=(1, 3), labels=[2, 5, 9], zero_background=False, seed=103, sampled=0),
    "odd_zero": dict(shape=(3, 6, 9), scales=(1, 3), labels=[2, 5, 9], zero_background=True, seed=104, sampled=0),
}


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


def main():
    U = reference_module()
    out = {"cases": np.array(list(CASES))}
    for name, c in CASES.items():
        shape, scales = c["shape"], c["scales"]
        lab = DR.label_blobs(shape, c["labels"], c["seed"])
        assert np.unique(lab).tolist() == sorted(c["labels"])
        L = len(c["labels"])
        torch.manual_seed(c["seed"])
        means = U.transform_uniform(torch.rand(L), 25, 255)
        stds = U.transform_uniform(torch.rand(L), 5, 20)
        zb = 1.0 if c["zero_background"] else 0.0
        torch.manual_seed(c["seed"] + 1000)
        gmm = U.sample_gmm(means, stds, lab, zero_bckgnd=zb).numpy()
        z = DR.replay_noise(lab, c["seed"] + 1000, c["zero_background"])
        # the replayed draws through the same torch expressions: bit for bit
        chk = torch.zeros(shape)
        for i, l in enumerate(np.unique(lab)):
            if i == 0 and c["zero_background"]:
                continue
            idx = lab == l
            chk[idx] = stds[i] * torch.from_numpy(z)[idx] + means[i]
        chk = torch.clip(chk, min=0)
        assert np.array_equal(((chk - chk.min()) / (chk.max() - chk.min())).numpy(), gmm), name
        torch.manual_seed(c["seed"] + 2000)
        perl = U.draw_perlin_volume(out_shape=shape, scales=scales, max_std=5.0).numpy()
        grids = DR.replay_grids(shape, scales, c["seed"] + 2000, 5.0)
        chk = torch.zeros(shape)
        for s, g in zip(scales, grids):
            g = torch.from_numpy(g)
            chk += g if s == 1 else torch.nn.functional.interpolate(g[None, None], scale_factor=s, mode="trilinear")[0, 0]
        assert np.array_equal(chk.numpy(), perl), name
        view = (torch.from_numpy(gmm) * (1 + 0.02 * torch.from_numpy(perl))).numpy()
        m, s_ = means.numpy(), stds.numpy()
        for tag, ref, mine in (("gmm", gmm, DR.gmm(lab, m, s_, z, c["zero_background"], np.float64)),
                               ("perlin", perl, DR.perlin(shape, scales, grids, np.float64)),
                               ("view", view, DR.appearance(lab, m, s_, z, c["zero_background"], scales, grids, 0.02, np.float64))):
            err = np.abs(mine - ref).max() / np.abs(ref).max()
            print(f"{name} {tag}: restatement vs reference {err:.2e} of max|ref| {np.abs(ref).max():.4f}")
            assert err <= 2e-6
        out.update({f"{name}/labels": lab, f"{name}/means": m, f"{name}/stds": s_, f"{name}/scales": np.array(scales),
                    f"{name}/zero_background": np.array(c["zero_background"]), f"{name}/seed": np.array(c["seed"] + 1000)})
        for s, g in zip(scales, grids):
            out[f"{name}/grid_{s}"] = g
        if c["sampled"]:
            index = np.sort(np.random.RandomState(c["seed"]).permutation(lab.size)[:c["sampled"]])
            out[f"{name}/index"] = index
            for tag, a in (("z", z), ("gmm", gmm), ("perlin", perl), ("view", view)):
                out[f"{name}/{tag}"] = a.reshape(-1)[index]
        else:
            out.update({f"{name}/z": z, f"{name}/gmm": gmm, f"{name}/perlin": perl, f"{name}/view": view})
    path = os.path.join(ROOT, "tests", "golden", "datagen_golden.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
