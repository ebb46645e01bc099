"""CPU: pins the numpy restatement of the augmentation chain (tests/_segaug_ref.py, the reference of the GPU tests) to independent
implementations -- torch's grid_sample, numpy's leggrid3d, the closed forms of the Gaussian taps and of the Gibbs mask -- and checks
the host side of anatomix_amd.segmentation: ``draw_params``, ``data_handler`` and the command line.  MONAI cannot be imported here,
so parity with MONAI stays unpinned."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _segaug_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# output size / input size of the affine resample: equal and even, one input axis smaller than the output, equal and odd
AFFINE_SIZES = [((16, 16, 16), (16, 16, 16)), ((12, 12, 12), (12, 9, 12)), ((15, 15, 15), (15, 15, 15))]


def _grid_sample(img, A, out_size, mode):
    """The same resample through torch: align_corners=True with the grid 2 idx / (n - 1) - 1 built from the source indices."""
    src = AR.source_index(A, out_size, img.shape, np.float64)
    grid = np.stack([2 * src[a] / (img.shape[a] - 1) - 1 for a in (2, 1, 0)], -1)          # grid_sample wants (x, y, z)
    out = F.grid_sample(torch.from_numpy(img)[None, None], torch.from_numpy(grid)[None], mode=mode, padding_mode="zeros", align_corners=True)
    return out[0, 0].numpy()


@pytest.mark.parametrize("sizes", AFFINE_SIZES, ids=lambda s: "x".join(map(str, s[0])) + "_from_" + "x".join(map(str, s[1])))
@pytest.mark.parametrize("seed", range(6))
def test_affine_restatement_against_grid_sample(sizes, seed):
    out_size, in_size = sizes
    img, lab = AR.blob_volume(in_size, 10 + seed)
    A = AR.seeded_matrix(seed)
    got, glab, src = AR.affine(img, lab, A, out_size, np.float64)
    want = _grid_sample(img, A, out_size, "bilinear")
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"affine {out_size} from {in_size} seed {seed}: trilinear err / max {err:.3e}")
    assert err <= 1e-12
    # nearest: away from half-integers (where torch and the restatement both round, but from differently rounded coordinates)
    margin = AR.half_integer_margin(src)
    sure = margin >= 1e-4
    excluded = 1.0 - sure.mean()
    wlab = _grid_sample(lab, A, out_size, "nearest")
    print(f"  nearest: excluded {100 * excluded:.3f} % of voxels, labels present {np.unique(glab).tolist()}")
    assert excluded <= 0.0024
    assert np.array_equal(glab[sure], wlab[sure].astype(np.uint8))
    assert len(np.unique(glab)) > 1


def test_affine_identity_returns_the_inputs():
    img, lab = AR.blob_volume((15, 15, 15), 3)
    got, glab, _ = AR.affine(img, lab, np.eye(3), (15, 15, 15), np.float64)
    assert np.array_equal(got, img) and np.array_equal(glab, lab.astype(np.uint8))


def test_affine_rounds_half_to_even():
    # a shift by exactly half a voxel along the last axis: source index x + 0.5 -> 0, 2, 2, 4, 4, ...
    lab = np.tile(np.arange(6, dtype=np.float64), (2, 2, 1))
    _, glab, _ = AR.affine(lab, lab, np.eye(3), (2, 2, 5), np.float64)      # size_in 6, size_out 5: centres differ by 0.5
    assert glab[0, 0].tolist() == [0, 2, 2, 4, 4]


def test_legendre_field_against_leggrid3d():
    from numpy.polynomial.legendre import leggrid3d
    shape = (7, 12, 9)
    coeff = np.random.RandomState(0).uniform(0, 0.05, 20)
    c3 = np.zeros((4, 4, 4))
    for q, (i, j, k) in enumerate(AR.coeff_index()):
        c3[i, j, k] = np.float32(coeff[q])
    assert len(AR.coeff_index()) == 20 and AR.coeff_index() == sorted(AR.coeff_index())
    want = leggrid3d(*[np.linspace(-1, 1, n) for n in shape], c3)
    got = AR.bias_exponent(shape, coeff, np.float64)
    assert np.abs(got - want).max() <= 1e-14


@pytest.mark.parametrize("sigma,radius", [(0.0, 1), (0.05, 1), (0.1, 1), (0.5, 2), (0.75, 3), (1.0, 4)])
def test_gaussian_taps(sigma, radius):
    from anatomix_amd.segmentation.augment import gaussian_taps
    for fn in (AR.gaussian_taps, gaussian_taps):
        r, taps = fn(sigma)
        taps = np.asarray(taps)
        assert r == radius and len(taps) == 2 * radius + 1
        assert np.array_equal(taps, taps[::-1]) and (taps >= 0).all()
        if sigma == 0.0:
            assert taps.tolist() == [0.0, 1.0, 0.0]
            continue
        # the erf form integrates the normal density over each voxel: the taps add up to P(|x| <= tail + 0.5)
        assert abs(taps.sum() - math.erf((radius + 0.5) * 0.70710678 / sigma)) <= 1e-15
        assert abs(taps[radius] - math.erf(0.5 * 0.70710678 / sigma)) <= 1e-15
    assert np.array_equal(np.asarray(gaussian_taps(sigma)[1]), AR.gaussian_taps(sigma)[1])


def test_gaussian_of_sigma_zero_is_the_identity_and_padding_is_zero():
    x = np.random.RandomState(1).rand(5, 6, 7)
    assert np.array_equal(AR.gaussian(x, (0.0, 0.0, 0.0), np.float64), x)
    one = np.ones((9, 9, 9))
    r, taps = AR.gaussian_taps(0.75)
    got = AR.gaussian(one, (0.75, 0.0, 0.0), np.float64)
    t32 = taps.astype(np.float32).astype(np.float64)
    assert abs(got[4, 4, 4] - t32.sum()) <= 1e-15 and abs(got[0, 4, 4] - t32[r:].sum()) <= 1e-15     # the border loses the taps outside


def test_gibbs_with_alpha_zero_returns_the_input():
    """alpha = 0: r = max(shape) sqrt(2) / 2, the half diagonal of a square.  On 8 x 8 x 4 the sphere holds all of k-space (corner
    distance 5.17 < r = 5.66) and the input comes back.  On the cube 8^3 it holds all but the eight corner voxels (distance
    sqrt(3) 3.5 = 6.06), so there the definition removes exactly those eight frequencies and nothing else."""
    flat = np.random.RandomState(3).rand(8, 8, 4)
    got = AR.gibbs(flat, AR.gibbs_radius(0.0, flat.shape), np.float64)
    print(f"gibbs alpha 0 on 8x8x4: max change {np.abs(got - flat).max():.3e}")
    assert np.abs(got - flat).max() <= 1e-14
    x0 = np.random.RandomState(2).rand(8, 8, 8)
    r = AR.gibbs_radius(0.0, x0.shape)
    assert abs(float(r) - 4 * math.sqrt(2.0)) <= 1e-6
    ax = (2.0 * np.arange(8) - 7) ** 2
    kept = (ax[:, None, None] + ax[None, :, None] + ax[None, None, :]) <= 4.0 * float(r) ** 2
    corners = np.zeros((8, 8, 8), bool)
    corners[np.ix_([0, 7], [0, 7], [0, 7])] = True
    assert np.array_equal(~kept, corners)
    want = np.fft.ifftn(np.fft.ifftshift(np.fft.fftshift(np.fft.fftn(x0)) * kept)).real       # x0 without the eight corner frequencies
    assert np.abs(AR.gibbs(x0, r, np.float64) - want).max() <= 1e-14
    assert np.abs(AR.gibbs(x0, np.float32(100.0), np.float64) - x0).max() <= 1e-14           # a sphere that holds the cube: the identity
    low = AR.gibbs(x0, AR.gibbs_radius(0.9, x0.shape), np.float64)                            # r = 0.566: the centre's 8 voxels at 0.866 are out
    assert np.abs(low).max() <= 1e-14


def test_draw_params_is_seeded_and_in_range():
    from anatomix_amd.segmentation.augment import draw_params
    shapes = [(37, 30, 41), (16, 16, 16), (20, 33, 17)]
    a = draw_params(np.random.RandomState(7), 16, shapes, 3)
    b = draw_params(np.random.RandomState(7), 16, shapes, 3)
    c = draw_params(np.random.RandomState(8), 16, shapes, 3)
    for k in a:
        if k == "on":
            assert all(np.array_equal(a["on"][s], b["on"][s]) for s in a["on"])
        else:
            assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["coeff"], c["coeff"])
    assert set(a["on"]) == set(AR.SWITCH_NAMES)
    n = 2000
    p = draw_params(np.random.RandomState(0), 16, [shapes[i % 3] for i in range(n)], n)
    for i in range(n):
        for ax in range(3):
            assert 0 <= p["corner"][i, ax] <= shapes[i % 3][ax] - 16
    assert (p["corner"][1::3] == 0).all() and p["corner"][0::3].max(0).tolist() == [21, 14, 25]
    rng = [("rand_std", 0, 0.1), ("coeff", 0, 0.05), ("gibbs_alpha", 0, 0.33), ("gamma", 0.5, 4.5), ("smooth_sigma", 0, 0.1),
           ("sharpen_sigma1", 0.5, 1.0), ("sharpen_alpha", 10, 30), ("rotate", -math.pi / 4, math.pi / 4), ("shear", -0.2, 0.2), ("scale", 0.8, 1.2)]
    for k, lo, hi in rng:
        assert p[k].shape[0] == n and (p[k] >= lo).all() and (p[k] <= hi).all(), k
        assert p[k].max() - p[k].min() > 0.9 * (hi - lo), k
    assert (p["sharpen_sigma2"] >= 0.5).all() and (p["sharpen_sigma2"] <= p["sharpen_sigma1"]).all()
    assert p["coeff"].shape == (n, 20) and 0 <= p["noise_seed"] < 2 ** 31
    for k in AR.SWITCH_NAMES:
        freq, pr = p["on"][k].mean(), AR.PROB[k]
        sd = math.sqrt(pr * (1 - pr) / n)
        print(f"switch {k}: frequency {freq:.4f}, prob {pr}, {abs(freq - pr) / sd:.2f} standard deviations")
        assert abs(freq - pr) <= 4 * sd
    for i in range(50):
        want = AR.affine_matrix(p["rotate"][i], p["shear"][i], p["scale"][i]) if p["on"]["affine"][i] else np.eye(3)
        assert np.abs(p["affine"][i] - want).max() <= 1e-15


def test_affine_matrix_composition():
    from anatomix_amd.segmentation.augment import affine_matrix
    A = affine_matrix((0.3, 0, 0), (0, 0, 0), (1, 1, 1))
    assert np.allclose(A, [[1, 0, 0], [0, math.cos(0.3), -math.sin(0.3)], [0, math.sin(0.3), math.cos(0.3)]])
    S = affine_matrix((0, 0, 0), (0.1, 0.2, 0.3), (1, 1, 1))
    assert np.array_equal(S, [[1, 0.1, 0.2], [0.3, 1, 0], [0, 0, 1]])
    assert np.array_equal(affine_matrix((0, 0, 0), (0, 0, 0), (0.9, 1.1, 1.2)), np.diag([0.9, 1.1, 1.2]))
    full = affine_matrix((0.1, -0.2, 0.3), (0.05, -0.1, 0.15), (0.9, 1.1, 1.2))
    parts = (affine_matrix((0.1, 0, 0)) @ affine_matrix((0, -0.2, 0)) @ affine_matrix((0, 0, 0.3)) @ affine_matrix(shear=(0.05, -0.1, 0.15))
             @ affine_matrix(scale=(0.9, 1.1, 1.2)))
    assert np.abs(full - parts).max() <= 1e-15


def test_data_handler_natural_order_and_selection(tmp_path):
    from anatomix_amd.segmentation import data_handler
    from anatomix_amd.segmentation.segmentation_utils import natural_sorted
    names = ["case2", "case10", "case1b", "case1", "case01x", "Case3"]
    for sub in ("imagesTr", "labelsTr", "imagesVal", "labelsVal"):
        (tmp_path / sub).mkdir()
        for n in (names if sub.endswith("Tr") else names[:3]):
            (tmp_path / sub / f"{n}.nii.gz").write_bytes(b"")
    # digit runs as integers, the rest as text; a number sorts before text at the same position ("case1" < "case1b" as prefixes,
    # "case01x" has the same leading number 1 as "case1b" and then "x" > "b"; upper case before lower case as in plain text order)
    expected = ["Case3", "case1", "case1b", "case01x", "case2", "case10"]
    assert [os.path.basename(p)[:-7] for p in natural_sorted(str(tmp_path / "imagesTr" / f"{n}.nii.gz") for n in names)] == expected
    tri, trs, vai, vas = data_handler(str(tmp_path), finetuning_amount=4, iters_per_epoch=5, batch_size=3)
    perm = np.random.RandomState(12345).permutation(len(expected))
    picked = [expected[i] for i in perm[:4]]
    repeats = max(1, 5 * 3 // 4)
    assert [os.path.basename(p)[:-7] for p in tri] == picked * repeats and len(tri) == 4 * 3
    assert [os.path.basename(p)[:-7] for p in trs] == picked * repeats
    assert all("imagesTr" in p for p in tri) and all("labelsTr" in p for p in trs)
    assert [os.path.basename(p)[:-7] for p in vai] == ["case1b", "case2", "case10"] == [os.path.basename(p)[:-7] for p in vas]
    assert len(data_handler(str(tmp_path), finetuning_amount=6, iters_per_epoch=1, batch_size=2)[0]) == 6      # repeats never below 1
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(AssertionError):
        data_handler(str(empty))


def test_command_line_against_the_reference_fixture():
    from anatomix_amd.segmentation.train_segmentation import build_parser
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "segtrain_cli.json")))
    mine = AR.describe_parser(build_parser())
    n = len(want["flags"])
    assert n == 18
    for a, b in zip(mine["flags"], want["flags"]):
        assert a == b, (a, b)
    assert mine["exclusive_groups"] == want["exclusive_groups"] == [{"required": True, "dests": ["pretrained_ckpt", "hf_variant"]}]
    extra = {f["dest"]: f for f in mine["flags"][n:]}
    assert list(extra) == ["seed", "out_dir", "no_augment"]
    assert extra["seed"]["default"] == 0 and extra["out_dir"]["default"] == "finetuning_runs" and extra["no_augment"]["default"] is False
    opt = build_parser().parse_args(["--pretrained_ckpt", "scratch"])
    assert opt.crop_size == 128 and opt.lr == 2e-4 and opt.train_amount == 3 and not opt.no_augment
    with pytest.raises(SystemExit):
        build_parser().parse_args([])
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--pretrained_ckpt", "a.pth", "--hf_variant", "anatomix"])


def test_sample_record_layout_matches_the_library():
    from anatomix_amd import _lib
    from anatomix_amd.segmentation.augment import SAMPLE_DTYPE
    assert _lib.load().amx_segaug_sample_bytes() == SAMPLE_DTYPE.itemsize == 536
