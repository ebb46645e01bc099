"""CPU: pins the numpy restatement of the pretraining augmentation (tests/_preaug_ref.py, the reference of the GPU tests) to
independent definitions -- torch.nn.functional.grid_sample in float64, scipy.ndimage.gaussian_filter,
numpy.polynomial.polynomial.polygrid3d and the 3-D FFT form of the motion composite -- and checks ``draw_params``: ranges, the
documented draw order, that a switched-off transform still consumes its numbers, and ``apply_same_inten_augment``.  Parity with TorchIO
is unpinned (it is not installed)."""
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _preaug_ref as PR

from anatomix_amd.pretraining import augment as G

SHAPES = [(12, 10, 8), (9, 11, 7)]


def _grid_sample(img, M, mode, pad):
    """grid_sample(x - pad, zeros padding, align_corners=True) + pad at the source indices of M, all in float64."""
    S = img.shape
    o = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in S], indexing="ij"), -1)
    src = o @ M[:, :3].T + M[:, 3]
    g = torch.from_numpy(np.stack([2 * src[..., a] / (S[a] - 1) - 1 for a in (2, 1, 0)], -1))[None]
    x = torch.from_numpy(np.asarray(img, np.float64) - pad)[None, None]
    return torch.nn.functional.grid_sample(x, g, mode=mode, padding_mode="zeros", align_corners=True)[0, 0].numpy() + pad


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("seed", range(6))
def test_resample_is_grid_sample(seed, shape):
    img, lab = PR.blob_volume(shape, 10 + seed)
    M = PR.seeded_map(seed, shape)
    M = M.astype(np.float32).astype(np.float64)                     # what the device receives, so both sides see one map
    pad = img.min()
    got, glab, src = PR.resample(img, lab, M, pad, np.float64)
    want = _grid_sample(img, M, "bilinear", pad)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    sure = PR.half_integer_margin(src) >= 1e-4                       # grid_sample rounds its own (normalised, de-normalised) index
    wlab = _grid_sample(lab, M, "nearest", 0.0)
    assert 1 - sure.mean() <= 0.0029 and np.array_equal(glab[sure], wlab[sure].astype(np.uint8))
    if seed == 0:                                                    # flip-only: exact copies
        assert PR.is_integral_map(M) and np.array_equal(got, img[::-1, :, ::-1]) and np.array_equal(glab, lab[::-1, :, ::-1].astype(np.uint8))


def test_spatial_map_of_the_module_is_the_restatement():
    r = np.random.RandomState(4)
    for shape in SHAPES:
        for _ in range(4):
            flips, scales, degrees = r.uniform(size=3) < 0.5, r.uniform(0.6, 1.4, 3), r.uniform(-45, 45, 3)
            np.testing.assert_allclose(G.spatial_map(shape, flips, scales, degrees), PR.spatial_map(shape, flips, scales, degrees), atol=1e-12)
            np.testing.assert_allclose(G.spatial_map(shape, flips), PR.spatial_map(shape, flips), atol=0)
            t = r.uniform(-10, 10, 3)
            np.testing.assert_allclose(G.rigid_map(shape, degrees / 4, t), PR.rigid_map(shape, degrees / 4, t), atol=1e-12)
    # the forward map moves the centre to itself and scales along the rotated axes
    M = PR.spatial_map((9, 9, 9), (False,) * 3, (2.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    np.testing.assert_allclose(M @ np.array([8.0, 4.0, 4.0, 1.0]), [6.0, 4.0, 4.0], atol=1e-12)


@pytest.mark.parametrize("sigma", [(0.0, 0.05, 2.0), (2.0, 0.7, 0.0), (1.3, 2.0, 0.05), (0.124, 0.126, 1e-16)])
def test_blur_is_scipy_gaussian_filter(sigma):
    import scipy.ndimage as ndi
    for shape in [(3, 10, 8), (12, 3, 8), (12, 10, 3), (9, 11, 7)]:       # an axis of length 3 under a radius of 8
        img, _ = PR.blob_volume(shape, 3)
        want = ndi.gaussian_filter(img, sigma)
        got = PR.blur(img, sigma, np.float64, round_taps=False)
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max(), (shape, sigma)
        got = PR.blur(img, sigma, np.float64)                             # taps rounded to float32: 2^-24 each
        assert np.abs(got - want).max() <= 3 * 2.0 ** -23 * np.abs(want).max(), (shape, sigma)
    for s in sigma:
        r, taps = G.gaussian_taps(s)
        r2, taps2 = PR.gaussian_taps(s)
        assert r == r2 == (int(4 * s + 0.5) if s > 1e-15 else 0) and r <= G.MAX_RADIUS and np.array_equal(taps, taps2)
        assert abs(taps.sum() - 1) < 1e-15


def test_bias_field_is_polygrid3d():
    from numpy.polynomial.polynomial import polygrid3d
    r = np.random.RandomState(5)
    for shape in SHAPES:
        coeff = r.uniform(-0.5, 0.5, 20).astype(np.float32).astype(np.float64)
        c = np.zeros((4, 4, 4))
        for q, (i, j, k) in enumerate(PR.coeff_index()):
            c[i, j, k] = coeff[q]
        want = polygrid3d(*[np.linspace(-1, 1, n) for n in shape], c)
        got = PR.bias_exponent(shape, coeff, np.float64)
        assert len(PR.coeff_index()) == 20 and np.abs(got - want).max() <= 1e-14
    x = np.array([[[-2.0, 0.0, 3.0]]])
    assert np.allclose(PR.gamma(x, 2.0, np.float64), [[[-4.0, 0.0, 9.0]]])


@pytest.mark.parametrize("shape", SHAPES)
def test_motion_1d_route_is_the_3d_definition(shape):
    img, _ = PR.blob_volume(shape, 6)
    r = np.random.RandomState(7)
    deg, tr = r.uniform(-10, 10, (2, 3)), r.uniform(-3, 3, (2, 3))
    times = np.array([1 / 3, 2 / 3]) + r.uniform(-0.1, 0.1, 2)
    a = PR.motion(img, deg, tr, times, np.float64)
    b = PR.motion_1d(img, deg, tr, times, np.float64)
    assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max()
    assert np.abs(a - img).max() > 1e-3                                # it does something
    # no move at all: the composite of three copies of one spectrum is the image
    same = PR.motion(img, np.zeros((2, 3)), np.zeros((2, 3)), times, np.float64)
    assert np.abs(same - img).max() <= 1e-13


def _opt(**kw):
    o = dict(isTrain=True, crop_size=0, augment=True, geo_augment=True, inten_augment=True, blur=True, noise=True, bias=True, gamma=True,
             motion=True, apply_same_inten_augment=False)
    o.update(kw)
    return Namespace(**o)


def test_draw_params_ranges_and_rates():
    rng = np.random.RandomState(0)
    n = 400
    P = [G.draw_params(rng, (12, 10, 8), _opt(crop_size=6)) for _ in range(n)]
    for p in P:
        assert (0.6 <= p["scales"]).all() and (p["scales"] <= 1.4).all() and (np.abs(p["degrees"]) <= 45).all()
        assert p["crop_size"] == 6 and all(0 <= s <= e - 6 for s, e in zip(p["crop_start"], (12, 10, 8)))
        assert (p["map"] is None) == (not p["flip_axes"].any() and not p["affine_on"])
        for v in p["views"]:
            assert (0 <= v["sigma"]).all() and (v["sigma"] <= 2).all() and 0 <= v["noise_std"] <= 0.25 and 0 <= v["noise_seed"] < 2 ** 31 - 1
            assert (np.abs(v["coeff"]) <= 0.5).all() and v["coeff"].shape == (20,) and np.exp(-0.4) <= v["gamma"] <= np.exp(0.4)
            assert (np.abs(v["motion_degrees"]) <= 10).all() and (np.abs(v["motion_translation"]) <= 10).all()
            assert abs(v["motion_times"][0] - 1 / 3) <= 0.1 and abs(v["motion_times"][1] - 2 / 3) <= 0.1
    rate = lambda f: np.mean([f(p) for p in P])                       # noqa: E731  (binomial sd at n = 400 is <= 0.025)
    assert abs(rate(lambda p: p["flip_on"]) - 0.9) < 0.08 and abs(rate(lambda p: p["affine_on"]) - 0.5) < 0.1
    for name, prob in G.INTENSITY_SWITCHES:
        assert abs(rate(lambda p: p["views"][0]["on"][name]) - prob) < 0.1, name
    assert any(p["views"][0]["on"]["blur"] != p["views"][1]["on"]["blur"] for p in P)


def test_draw_params_order_and_switches_consume_their_numbers():
    shape = (12, 10, 8)
    p = G.draw_params(np.random.RandomState(42), shape, _opt(crop_size=6))
    r = np.random.RandomState(42)                                     # the documented order, replayed
    flip_on, flips = r.uniform() < 0.9, r.uniform(size=3) < 0.5
    affine_on, scales, degrees = r.uniform() < 0.5, r.uniform(0.6, 1.4, 3), r.uniform(-45, 45, 3)
    assert p["flip_on"] == flip_on and np.array_equal(p["flip_axes"], flips & flip_on) and p["affine_on"] == affine_on
    assert np.array_equal(p["scales"], scales) and np.array_equal(p["degrees"], degrees)
    for v in p["views"]:
        assert v["on"]["blur"] == (r.uniform() < 0.33) and np.array_equal(v["sigma"], r.uniform(0, 2, 3))
        assert v["on"]["noise"] == (r.uniform() < 0.33) and v["noise_std"] == r.uniform(0, 0.25) and v["noise_seed"] == r.randint(0, 2 ** 31 - 1)
        assert v["on"]["bias"] == (r.uniform() < 0.5) and np.array_equal(v["coeff"], r.uniform(-0.5, 0.5, 20))
        assert v["on"]["gamma"] == (r.uniform() < 0.5) and v["gamma"] == float(np.exp(r.uniform(-0.4, 0.4)))
        assert v["on"]["motion"] == (r.uniform() < 0.33) and np.array_equal(v["motion_degrees"], r.uniform(-10, 10, (2, 3)))
        assert np.array_equal(v["motion_translation"], r.uniform(-10, 10, (2, 3)))
        assert np.array_equal(v["motion_times"], np.arange(1, 3) / 3.0 + r.uniform(-0.1, 0.1, 2))
    assert p["crop_start"] == tuple(int(r.randint(3, n - 3)) - 3 for n in shape)
    # every flag off: nothing is on, the same numbers are drawn, so the stream afterwards is where it was
    a, b = np.random.RandomState(42), np.random.RandomState(42)
    G.draw_params(a, shape, _opt(crop_size=6))
    q = G.draw_params(b, shape, _opt(crop_size=6, geo_augment=False, inten_augment=False))
    assert a.uniform() == b.uniform()
    assert q["map"] is None and not q["flip_on"] and not q["affine_on"] and not any(any(v["on"].values()) for v in q["views"])
    assert np.array_equal(q["scales"], p["scales"]) and np.array_equal(q["views"][1]["coeff"], p["views"][1]["coeff"])
    one = G.draw_params(np.random.RandomState(42), shape, _opt(blur=False, motion=False))
    assert not any(v["on"]["blur"] or v["on"]["motion"] for v in one["views"]) and one["crop_start"] is None and one["crop_size"] == 0
    assert [v["on"]["noise"] for v in one["views"]] == [v["on"]["noise"] for v in p["views"]]
    # an axis no longer than the window draws nothing (random_crop's rule); validation never crops
    s = G.draw_params(np.random.RandomState(1), (9, 6, 5), _opt(crop_size=6))
    r = np.random.RandomState(1)
    G.draw_params(r, (9, 6, 5), _opt())
    assert s["crop_start"] == (int(r.randint(3, 6)) - 3, 0, 0)
    assert G.draw_params(np.random.RandomState(1), shape, _opt(crop_size=6, isTrain=False))["crop_start"] is None


def test_apply_same_inten_augment_copies_the_record():
    shape = (12, 10, 8)
    a, b = np.random.RandomState(9), np.random.RandomState(9)
    p = G.draw_params(a, shape, _opt(apply_same_inten_augment=True))
    q = G.draw_params(b, shape, _opt())
    assert a.uniform() == b.uniform()                                 # view B's numbers are drawn either way
    A, B = p["views"]
    assert A is not B and A["on"] == B["on"] and A["noise_seed"] == B["noise_seed"] and A["noise_std"] == B["noise_std"]
    for k in ("sigma", "coeff", "motion_degrees", "motion_translation", "motion_times"):
        assert np.array_equal(A[k], B[k]) and A[k] is not B[k]
    assert A["gamma"] == B["gamma"] == q["views"][0]["gamma"] and q["views"][1]["noise_seed"] != q["views"][0]["noise_seed"]


def test_the_record_layout_and_the_host_refusals():
    from anatomix_amd import _lib
    assert _lib.load().amx_preaug_view_bytes() == G.VIEW_DTYPE.itemsize == 356
    x = torch.zeros(1, 4, 4, 4)
    for fn in (lambda t: G.blur(t, 1.0), lambda t: G.gamma(t, 1.2), lambda t: G.bias_field(t, np.zeros(20)), lambda t: G.flip_affine(t),
               lambda t: G.add_noise(t, 0.1, t), lambda t: G.motion(t, np.zeros((2, 3)), np.zeros((2, 3)), [0.3, 0.6])):
        with pytest.raises(RuntimeError, match="no host path"):
            fn(x)
    p = G.draw_params(np.random.RandomState(0), (4, 4, 4), _opt())
    with pytest.raises(RuntimeError, match="no host path"):
        G.augment_pair(x, x, x, p)
