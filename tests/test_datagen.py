"""CPU: step 2 of the synthetic data generation (anatomix_amd.datagen).  The numpy restatement tests/_datagen_ref.py, which the GPU
tests (tests/test_datagen_gpu.py) compare the kernels with, is pinned here: ``gmm`` and ``perlin`` to the reference's recorded outputs
(tests/golden/datagen_golden.npz, made by tools/make_golden_datagen.py), ``low_resolution`` to F.interpolate, the plane-wave form of the
k-space spike to its FFT definition.  Also the seeded parameter draws, the parser, the record layout, and the share of voxels of the
GPU chain cases that sit close enough to a uint8 step to round either way."""
import functools
import os

import numpy as np
import pytest
import torch

import _datagen_ref as DR
from anatomix_amd import _lib
from anatomix_amd.datagen import views as V

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen_golden.npz")


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD))


def case_names():
    return [str(n) for n in np.load(GOLD)["cases"]]


@pytest.mark.parametrize("name", case_names())
def test_restatement_against_the_reference_fixture(name):
    """2e-6 of max |reference|: the float32 rounding of the reference itself (measured 9e-8 for the GMM, 1.6e-7 for the texture)."""
    c = DR.load_case(gold(), name)
    lab, shape = c["labels"], c["labels"].shape
    mine = {"gmm": DR.gmm(lab, c["means"], c["stds"], c["z"], c["zero_background"], np.float64),
            "perlin": DR.perlin(shape, c["scales"], c["grids"], np.float64),
            "view": DR.appearance(lab, c["means"], c["stds"], c["z"], c["zero_background"], c["scales"], c["grids"], 0.02, np.float64)}
    for tag, a in mine.items():
        ref = c[tag].astype(np.float64)
        err = float(np.abs(DR.at(a, c["index"]) - ref).max() / np.abs(ref).max())
        print(f"{name} {tag}: restatement vs reference {err:.3e} (bound 2e-6), max|ref| {np.abs(ref).max():.4f}")
        assert err <= 2e-6, (name, tag, err)


def test_fixture_covers_the_cases():
    g = gold()
    shapes = {n: g[f"{n}/labels"].shape for n in case_names()}
    assert shapes["big"] == (32, 64, 96) and shapes["mid"] == (8, 16, 24) and shapes["odd"] == (3, 6, 9)
    assert tuple(g["big/scales"]) == (4, 8, 16, 32) and tuple(g["mid/scales"]) == (2, 4, 8) and tuple(g["odd/scales"]) == (1, 3)
    assert g["big/grid_32"].shape == (1, 2, 3)                                      # one axis with a single coarse point
    u = np.unique(g["big/labels"])
    assert u.size > 40 and 255 in u and np.any(np.diff(u) > 1)
    assert {bool(g[f"{n}/zero_background"]) for n in case_names()} == {True, False}
    assert os.path.getsize(GOLD) < 1_000_000


@pytest.mark.parametrize("zoom", [0.5, 0.61, 0.77, 0.93, 1.0])
def test_low_resolution_against_interpolate(zoom):
    """float32 against float32: the same index arithmetic, another order of the three blends -- a few roundings of values below
    max |x|, bounded by 2e-6 max |x| (16 eps); zoom 1 is the identity bit for bit."""
    shape = (17, 24, 31)
    x = np.random.RandomState(3).standard_normal(shape).astype(np.float32)
    t = torch.from_numpy(x)[None, None]
    low = torch.nn.functional.interpolate(t, size=DR.low_resolution_shape(shape, zoom), mode="nearest-exact")
    want = torch.nn.functional.interpolate(low, size=shape, mode="trilinear", align_corners=False)[0, 0].numpy()
    got = DR.low_resolution(x, zoom, np.float32)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"zoom {zoom}: restatement vs F.interpolate {err:.3e}")
    assert err <= 2e-6
    if zoom == 1.0:
        assert np.array_equal(got, x)
    assert V.low_resolution_shape(shape, zoom) == DR.low_resolution_shape(shape, zoom)


SPIKE_LOCS = {(6, 8, 10): [(0, 0, 0), (5, 7, 9), (3, 4, 5), (0, 4, 5), (2, 0, 7)],
              (16, 16, 16): [(0, 0, 0), (15, 15, 15), (8, 8, 8), (0, 8, 3)]}


@pytest.mark.parametrize("shape", list(SPIKE_LOCS))
def test_spike_plane_wave_against_the_fft_definition(shape):
    """float64: both are exact up to rounding, 1e-9 of max |x| is three orders above what the two FFTs leave (1e-11 measured).
    Locations: a corner, the far corner, the centre n // 2 (DC) and index 0 of an even axis."""
    x = np.random.RandomState(4).uniform(0, 1, shape)
    for loc in SPIKE_LOCS[shape]:
        for k_int, factor in ((None, 1.0), (None, 0.97), (3.5, 1.0)):
            want = DR.spike_fft(x, loc, k_int, factor)
            got = DR.spike(x, loc, k_int, factor, np.float64)
            err = float(np.abs(got - want).max() / np.abs(want).max())
            print(f"{shape} loc {loc} k_intensity {k_int} factor {factor}: {err:.3e}, spike moved the image by {np.abs(want - x).max():.3e}")
            assert err <= 1e-9 and np.abs(want - x).max() > 1e-6


def test_draw_params_is_seeded_and_in_range():
    labels = [np.array([0, 1, 2]), np.array([5]), np.arange(0, 256, 5)]
    shape = (16, 24, 32)
    p, q = (V.draw_params(np.random.RandomState(7), labels, shape) for _ in range(2))
    r = V.draw_params(np.random.RandomState(8), labels, shape)
    for k in ("coeff", "spike_loc", "spike_factor", "gamma", "smooth_sigma", "gibbs_alpha", "sharpen_sigma1", "sharpen_sigma2",
              "sharpen_alpha", "zoom", "perl_std", "zero_background", "noise_seed"):
        assert np.array_equal(p[k], q[k]), k
    assert all(np.array_equal(p["on"][k], q["on"][k]) for k in DR.SWITCH_NAMES) and set(p["on"]) == set(DR.SWITCH_NAMES)
    assert not np.array_equal(p["coeff"], r["coeff"])
    assert p["scales"] == (4, 8, 16, 32) and p["perl_mult_factor"] == 0.02 and p["perl_std"].shape == (3, 2, 4)
    for b, l in enumerate(labels):
        assert p["means"][b].shape == p["stds"][b].shape == (2, l.size)
        assert (p["means"][b] >= 25).all() and (p["means"][b] <= 255).all() and (p["stds"][b] >= 5).all() and (p["stds"][b] <= 20).all()
    assert not p["zero_background"][1].any()                                   # one label: never a zero background
    rng = dict(coeff=(0, 0.075), spike_factor=(0.95, 1.1), gamma=(0.5, 2), smooth_sigma=(0, 0.333), gibbs_alpha=(0, 0.333),
               sharpen_sigma1=(0.5, 1), sharpen_alpha=(10, 30), zoom=(0.5, 1), perl_std=(0, 5))
    for k, (lo, hi) in rng.items():
        assert (p[k] >= lo).all() and (p[k] <= hi).all(), k
    assert (p["sharpen_sigma2"] >= 0.5).all() and (p["sharpen_sigma2"] <= p["sharpen_sigma1"]).all()
    assert (p["spike_loc"] >= 0).all() and (p["spike_loc"] < np.array(shape)).all()
    # the frequencies of the switches over many draws: within five standard deviations of their probabilities
    many = V.draw_params(np.random.RandomState(9), [np.array([0, 1])] * 400, (4, 4, 4), scales=(2,))
    for k in DR.SWITCH_NAMES:
        f, pr = many["on"][k].mean(), DR.PROB[k]
        assert abs(f - pr) <= 5 * np.sqrt(pr * (1 - pr) / 800), (k, f)
    assert abs(many["zero_background"].mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / 800)
    # a sample drawn alone equals itself inside a batch built from single draws
    one = [V.draw_params(np.random.RandomState([5, i]), [l], shape) for i, l in enumerate(labels)]
    cat = V.concat_params(one)
    assert np.array_equal(cat["coeff"][1], one[1]["coeff"][0]) and np.array_equal(cat["on"]["spike"][2], one[2]["on"]["spike"][0])
    assert len(cat["means"]) == 3 and np.array_equal(cat["means"][2], one[2]["means"][0]) and cat["noise_seed"].shape == (3,)


def test_parser_defaults():
    from anatomix_amd.datagen.step2_generate_views import build_parser
    a = build_parser().parse_args([])
    assert (a.start_idx, a.end_idx, a.ensembledir, a.savedir, a.max_workers) == (0, 120000, "./label_ensembles/", "./synthesized_views/", 3)
    assert (a.batch_size, a.seed, a.device) == (8, 0, "cuda:0")
    b = build_parser().parse_args(["--start_idx", "3", "--end_idx", "9", "--batch_size", "2", "--seed", "11", "--max_workers", "1"])
    assert (b.start_idx, b.end_idx, b.batch_size, b.seed, b.max_workers) == (3, 9, 2, 11, 1)


def test_label_maps_are_checked(tmp_path):
    from anatomix_amd.datagen.step2_generate_views import load_label_map
    from anatomix_amd.io.nifti import save_nifti
    good = DR.label_blobs((4, 6, 8), [0, 3, 255], 1)
    save_nifti(str(tmp_path / "a.nii.gz"), good.astype(np.float32))
    lab, u = load_label_map(str(tmp_path / "a.nii.gz"))
    assert lab.dtype == np.uint8 and np.array_equal(lab, good) and u.tolist() == [0, 3, 255]
    for name, bad in (("frac", good.astype(np.float32) + 0.5), ("high", good.astype(np.int16) + 1)):
        save_nifti(str(tmp_path / f"{name}.nii.gz"), bad)
        with pytest.raises(ValueError, match="integers in 0 .. 255"):
            load_label_map(str(tmp_path / f"{name}.nii.gz"))


def test_view_record_layout_matches_the_library():
    assert _lib.load().amx_synth_view_bytes() == V.VIEW_DTYPE.itemsize == 2352
    assert V.VIEW_DTYPE.fields["mean"][1] == 264 and V.VIEW_DTYPE.fields["spike_loc"][1] == 2316 and V.VIEW_DTYPE.fields["lowres"][1] == 2340


def test_host_checks_raise_without_a_device():
    with pytest.raises(RuntimeError, match="no host path"):
        V.synthesize_views(torch.zeros(1, 1, 4, 4, 4, dtype=torch.uint8), {})
    with pytest.raises(RuntimeError, match="no host path"):
        V.kspace_spike_noise(torch.zeros(1, 1, 4, 4, 4), (0, 0, 0))
    with pytest.raises(RuntimeError, match="no host path"):
        V.simulate_low_resolution(torch.zeros(1, 1, 4, 4, 4), 0.5)
    with pytest.raises(RuntimeError, match="no host path"):
        V.augment_views(torch.zeros(1, 2, 4, 4, 4), {})
    with pytest.raises(_lib.AmxEnvelopeError):
        V.coarse_shapes((32, 64, 96), (4, 5))
    with pytest.raises(ValueError, match="0 .. 255"):
        V.rank_table([0, 256])
    with pytest.raises(ValueError, match="sorted"):
        V.rank_table([3, 1])
    assert V.rank_table([2, 5, 255])[[2, 5, 255]].tolist() == [0, 1, 2]


@pytest.mark.parametrize("pattern", list(DR.PATTERNS))
def test_few_voxels_of_the_chain_cases_sit_on_a_uint8_step(pattern):
    """The uint8 condition of the GPU test on the reference alone: at most 1 % of the voxels of a chain case (its six views
    together, each with the band of its own bound) lie within 255 x bound of an integer >= 1, so that the GPU test's 2 % leaves room."""
    case = DR.chain_case(V.draw_params, pattern)
    inside = []
    for r, (ref64, e32) in enumerate(DR.chain_reference(case)):
        inside.append(DR.uint8_band(ref64, DR.BOUND(e32)))
        print(f"{pattern} row {r}: e32 {e32:.2e}, bound {DR.BOUND(e32):.2e}, {100 * inside[-1].mean():.3f} % of the voxels within the band")
        assert np.isfinite(ref64).all() and ref64.min() == 0.0 and ref64.max() == 1.0
    share = float(np.mean(inside))
    print(f"{pattern}: {100 * share:.3f} % of the case's voxels within the band")
    assert share <= 0.01, (pattern, share)
