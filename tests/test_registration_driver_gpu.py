"""GPU: the registration driver (anatomix_amd/registration/run_convex_adam_with_network_feats.py) end to end on a small pair:
``register_volumes`` against the same public steps called one by one here, ``convex_adam`` from files to files, the Dice it
prints against the count-based restatement on the files it wrote, and the reference's two corner behaviours (``ic=False``,
``selected_niter=0``).

The pair is 48 x 40 x 56, smaller than the 128^3 sliding window, so each volume is one padded window: a smooth image of four
blobs with a matching five-label map, the moving pair being the fixed one translated by (2, -1, 1) voxels, which lies inside the
+-4 voxel search range of grid_sp = 2, disp_hw = 2.  The network is the 6 M UNet with seeded random weights.

Equality with the step-by-step composition is bit for bit unless two runs of that composition themselves differ; then the largest
difference between those two runs is the allowance (printed)."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _regmetrics_ref as MR

pytestmark = pytest.mark.gpu
SHAPE = (48, 40, 56)
SHIFT = (2, -1, 1)
AFFINE = np.array([[1.5, 0.0, 0.0, -30.0], [0.0, -2.0, 0.25, 12.5], [0.0, 0.5, 1.25, 7.0], [0.0, 0.0, 0.0, 1.0]])
KW = dict(lambda_weight=0.75, grid_sp=2, disp_hw=2, selected_niter=10, selected_smooth=0, grid_sp_adam=2)
CENTRES = ((14.0, 12.0, 16.0), (33.0, 14.0, 38.0), (16.0, 28.0, 40.0), (34.0, 27.0, 17.0))
RADII = (8.0, 7.0, 7.5, 6.5)


def dev():
    return torch.device("cuda:0")


def scene(shift):
    """(image, labels) of the four blobs moved by `shift` voxels, float64 as get_fdata() returns them."""
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE], indexing="ij"))
    img = 0.1 + 0.002 * (x[0] + x[1] + x[2])
    lab = np.zeros(SHAPE)
    for n, (c, r) in enumerate(zip(CENTRES, RADII)):
        d2 = sum((x[a] - (c[a] + shift[a])) ** 2 for a in range(3))
        img = img + (0.6 + 0.1 * n) * np.exp(-d2 / (2 * (0.6 * r) ** 2))
        lab[d2 <= r * r] = n + 1
    return img, lab


@functools.lru_cache(maxsize=None)
def pair():
    (fix, fix_lab), (mov, mov_lab) = scene((0, 0, 0)), scene(SHIFT)
    mask = np.zeros(SHAPE)
    mask[4:-4, 4:-4, 4:-4] = 1.0
    return fix, mov, fix_lab, mov_lab, mask, np.roll(mask, SHIFT, (0, 1, 2))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """Checkpoint, the four volumes and the two masks on disk; (paths dict, directory)."""
    from anatomix_amd.io.nifti import save_nifti
    from oracle import unet_ref as R
    d = tmp_path_factory.mktemp("regdriver")
    p = {k: str(d / f"{k}.nii.gz") for k in ("fixed", "moving", "fixed_seg", "moving_seg", "fixed_mask", "moving_mask")}
    p["moving"] = str(d / "case07.moving.nii.gz")
    for k, arr in zip(("fixed", "moving", "fixed_seg", "moving_seg", "fixed_mask", "moving_mask"), pair()):
        save_nifti(p[k], arr.astype(np.float32), AFFINE)
    p["ckpt"] = str(d / "unet6m.pth")
    torch.save(R.synthetic_state_dict(R.VARIANTS["anatomix"], 0), p["ckpt"])
    return p, d


@pytest.fixture(scope="module")
def model(files):
    from anatomix_amd.registration import load_model
    return load_model(ckpt_path=files[0]["ckpt"])


def on_disk(a):
    """What a volume is after its float32 round trip through a file (the driver loads float64 of float32 values)."""
    return a.astype(np.float32).astype(np.float64)


def compose(model, fix, mov, seg=None, masks=None, ic=True, niter=10, smooth=0):
    """The driver's steps, one public call each, in the reference's order."""
    from anatomix_amd.registration import (apply_avg_pool3d, extract_features, instance_opt, merge_features, resize_trilinear,
                                           run_instance_opt, run_stage1_registration, warp_volume)
    H, W, D = SHAPE
    g, ga = KW["grid_sp"], KW["grid_sp_adam"]
    pf, pm = extract_features(fix, mov, model, None, None, None, None)
    pf, pm = pf * 0.1, pm * 0.1
    f0, m0 = (torch.from_numpy(v[None, None]).float().to(dev()) for v in (fix, mov))
    mk = [None, None] if masks is None else [torch.from_numpy(v).float().to(dev()) for v in masks]
    _, _, ff, fm = merge_features(masks is not None, pf, pm, mk[0], mk[1], f0, m0)
    fs, ms = F.avg_pool3d(ff, g, stride=g), F.avg_pool3d(fm, g, stride=g)
    disp = run_stage1_registration(fs, ms, KW["disp_hw"], g, (H, W, D), fs.shape[1], ic)
    if niter > 0 and ic:
        disp = run_instance_opt(disp, ff, fm, ga, KW["lambda_weight"], (H, W, D), niter, smooth, lr=1)
    elif niter > 0:
        w0 = resize_trilinear(disp, (H // ga, W // ga, D // ga), [1.0 / ga] * 3)
        fitted, _ = instance_opt(w0, F.avg_pool3d(ff, ga, stride=ga), F.avg_pool3d(fm, ga, stride=ga), KW["lambda_weight"], niter, lr=1)
        disp = resize_trilinear(fitted, (H, W, D), [float(ga)] * 3)
        if smooth in (3, 5):
            disp = apply_avg_pool3d(disp, smooth, 3)
    out = {"disp_hr": disp, "moved": warp_volume(m0, disp, "bilinear"), "moved_seg": None}
    if seg is not None:
        out["moved_seg"] = warp_volume(torch.from_numpy(seg[None, None]).float().to(dev()), disp, "nearest")
    return out


def assert_same(got, twice, what):
    """got: the driver's dict; twice: two runs of the composition."""
    for k in ("disp_hr", "moved", "moved_seg"):
        if twice[0][k] is None:
            assert got[k] is None
            continue
        allow = (twice[0][k] - twice[1][k]).abs().max().item()
        diff = (got[k] - twice[0][k]).abs().max().item()
        print(f"{what} {k}: shape {tuple(got[k].shape)}, difference from the composition {diff:.3e}, between two runs of the "
              f"composition {allow:.3e}, max |value| {twice[0][k].abs().max().item():.4f}")
        assert got[k].shape == twice[0][k].shape and diff <= allow


def register(model, fix, mov, **kw):
    from anatomix_amd.registration import register_volumes
    return register_volumes(fix, mov, model, **{**KW, **kw})


def test_register_volumes_is_its_composition(model):
    fix, mov, fix_lab, mov_lab, _, _ = pair()
    got = register(model, fix, mov, fixed_seg=fix_lab, moving_seg=mov_lab)
    twice = [compose(model, fix, mov, seg=mov_lab) for _ in range(2)]
    assert got["disp_hr"].shape == (1, 3) + SHAPE and got["moved"].shape == (1, 1) + SHAPE and got["moved_seg"].shape == (1, 1) + SHAPE
    assert_same(got, twice, "ic=True")
    counts, bad = MR.overlap_counts(fix_lab, got["moved_seg"].cpu().numpy(), 1024)
    want, per = MR.dice_from_counts(counts)
    print(f"dice {got['dice']:.15f}, from numpy counts {want:.15f}; case time {got['case_time']:.3f} s; jacobian {got['jacobian']}")
    assert bad == 0 and abs(got["dice"] - want) <= 1e-12 and sorted(got["dice_per_label"]) == sorted(per) == [1, 2, 3, 4]
    assert got["case_time"] > 0 and sorted(got["jacobian"]) == sorted(["folding_fraction", "min", "max", "mean", "log_mean", "log_std"])
    assert got["jacobian"]["min"] <= got["jacobian"]["mean"] <= got["jacobian"]["max"]
    # without label maps
    plain = register(model, fix, mov)
    assert plain["dice"] is None and plain["dice_per_label"] is None
    assert_same(plain, [{**t, "moved_seg": None} for t in twice], "no label maps")


def test_convex_adam_from_files_to_files(files, capsys):
    from anatomix_amd.io.nifti import load_nifti
    from anatomix_amd.registration import convex_adam
    p, d = files
    out_dir = d / "results"
    out_dir.mkdir(exist_ok=True)
    res = convex_adam("drv", 0.75, 2, 2, 10, 0, ckpt_path=p["ckpt"], grid_sp_adam=2, ic=True, result_path=str(out_dir),
                      fixed_image=p["fixed"], moving_image=p["moving"], warp_seg=True, fixed_seg=p["fixed_seg"],
                      moving_seg=p["moving_seg"])
    text = capsys.readouterr().out
    print(text)
    names = ["disp_case07.moving_g2_hw2_l0.75_ga2_icTrue_drv.nii.gz", "moved_case07.moving_g2_hw2_l0.75_ga2_icTrue_drv.nii.gz",
             "labels_moved_case07.moving_g2_hw2_l0.75_ga2_icTrue_drv.nii.gz"]
    assert sorted(os.listdir(out_dir)) == sorted(names)
    assert [os.path.basename(res[k]) for k in ("disp_path", "moved_path", "labels_moved_path")] == names
    disp, aff, _ = load_nifti(res["disp_path"])
    moved, aff_m, _ = load_nifti(res["moved_path"])
    lab, aff_l, _ = load_nifti(res["labels_moved_path"])
    assert disp.shape == SHAPE + (3,) and moved.shape == SHAPE and lab.shape == SHAPE
    for a in (aff, aff_m, aff_l):
        assert np.array_equal(a, AFFINE)
    assert np.array_equal(disp, res["disp_hr"][0].permute(1, 2, 3, 0).cpu().numpy().astype(np.float64))
    assert np.array_equal(moved, res["moved"][0, 0].cpu().numpy().astype(np.float64))
    assert np.array_equal(lab, res["moved_seg"][0, 0].cpu().numpy().astype(np.float64))
    # the Dice it returned and printed, against the count-based restatement on the files
    fix_lab = load_nifti(p["fixed_seg"])[0]
    want, _ = MR.dice_from_counts(MR.overlap_counts(fix_lab, lab, 1024)[0])
    printed = float(re.search(r"^Dice: (\S+)$", text, re.M).group(1))
    before, _ = MR.dice_from_counts(MR.overlap_counts(fix_lab, load_nifti(p["moving_seg"])[0], 1024)[0])
    print(f"Dice returned {res['dice']:.15f}, printed {printed:.15f}, from the files {want:.15f}; before registration {before:.6f}")
    assert abs(res["dice"] - want) <= 1e-12 and abs(printed - want) <= 1e-12
    assert re.search(r"^case time:  \S+$", text, re.M) and re.search(r"^Jacobian: folding_fraction ", text, re.M)
    assert "Loading model" in text and "Running network on input images" in text
    # the translation lies inside the search range: registration must improve the overlap
    assert res["dice"] > before


def test_ic_false_is_its_composition_and_niter_zero_is_stage_one(model):
    fix, mov, _, mov_lab, _, _ = pair()
    got = register(model, fix, mov, ic=False)
    assert got["disp_hr"].shape == (1, 3) + SHAPE
    assert_same(got, [compose(model, fix, mov, ic=False) for _ in range(2)], "ic=False")
    got = register(model, fix, mov, ic=False, selected_smooth=3)
    assert_same(got, [compose(model, fix, mov, ic=False, smooth=3) for _ in range(2)], "ic=False smooth=3")
    stage1 = register(model, fix, mov, selected_niter=0)
    assert_same(stage1, [compose(model, fix, mov, niter=0) for _ in range(2)], "selected_niter=0")
    with pytest.raises(ValueError, match="ic=False"):
        register(model, fix, mov, ic=False, selected_niter=0)


def test_masks_and_shape_errors(model, files):
    from anatomix_amd.registration import convex_adam
    fix, mov, fix_lab, mov_lab, mask_f, mask_m = pair()
    got = register(model, fix, mov, mask_fixed=mask_f, mask_moving=mask_m)
    assert_same(got, [compose(model, fix, mov, masks=(mask_f, mask_m)) for _ in range(2)], "use_mask")
    unmasked = register(model, fix, mov)
    assert not torch.equal(unmasked["disp_hr"], got["disp_hr"])                      # the masks take part
    p, d = files
    out_dir = d / "masked"
    out_dir.mkdir(exist_ok=True)
    res = convex_adam("m", 0.75, 2, 2, 10, 0, result_path=str(out_dir), fixed_image=p["fixed"], moving_image=p["moving"],
                      use_mask=True, fixed_mask=p["fixed_mask"], moving_mask=p["moving_mask"], model=model)
    assert res["labels_moved_path"] is None and res["dice"] is None and len(os.listdir(out_dir)) == 2
    assert_same(res, [compose(model, on_disk(fix), on_disk(mov), masks=(mask_f, mask_m)) for _ in range(2)], "convex_adam use_mask")
    with pytest.raises(ValueError, match="one shape"):
        register(model, fix, mov[:, :, :-2])
    with pytest.raises(ValueError, match="fixed_seg"):
        register(model, fix, mov, fixed_seg=fix_lab[:-1], moving_seg=mov_lab[:-1])
    with pytest.raises(ValueError, match="both masks"):
        register(model, fix, mov, mask_fixed=mask_f)
