"""GPU: step 2 of the synthetic data generation (csrc/amx_synth.hip through anatomix_amd.datagen.views), every new entry alone and
``generate_views`` as a chain, against the float64 numpy restatement tests/_datagen_ref.py (which tests/test_datagen.py pins to the
reference's recorded outputs, F.interpolate and the FFT definition; parity with MONAI is unpinned).

Bound, the project's own (tests/test_seg_augment_gpu.py::check_image): max |got - ref64| <= (5e-6 + 10 x e32) x max |ref64|, with e32 the
distance of the float32 evaluation of the same restatement from its float64 evaluation, computed here per case and printed; nothing
comes from the code under test.  Two runs must agree bit for bit, inputs one element off the 16-byte alignment must give the same
bits, a sample generated alone must equal the same sample in a batch of 3 (bit for bit in the appearance stage, within the bound for
the chain, whose FFTs are batched)."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _datagen_ref as DR
from anatomix_amd import _lib
from anatomix_amd.datagen import views as V
from test_seg_augment_gpu import check_image, cu, dev, e32_of, offset_by_one

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen_golden.npz")


@functools.lru_cache(maxsize=None)
def fixture_case(name):
    return DR.load_case(dict(np.load(GOLD)), name)


def appearance_params(c, B=1):
    """The fixture's case as both views of B samples; view 1 has the other zero-background flag, so both run at every shape."""
    u = np.unique(c["labels"])
    return dict(shape=c["labels"].shape, scales=c["scales"], perl_mult_factor=0.02, unique_labels=[u] * B,
                means=[np.stack([c["means"]] * 2)] * B, stds=[np.stack([c["stds"]] * 2)] * B,
                zero_background=np.array([[c["zero_background"], not c["zero_background"]]] * B))


@functools.lru_cache(maxsize=None)
def appearance_reference(name):
    """Per view (ref64, e32), computed once."""
    c = fixture_case(name)
    return [e32_of(lambda dt, zb=zb: DR.appearance(c["labels"], c["means"], c["stds"], c["z"], zb, c["scales"], c["grids"], 0.02, dt))
            for zb in (c["zero_background"], not c["zero_background"])]


@pytest.mark.parametrize("name", ["big", "mid", "odd", "odd_zero"])
def test_appearance_against_the_restatement_and_the_reference(name):
    c = fixture_case(name)
    p = appearance_params(c)
    lab = cu(c["labels"])[None, None]
    z = cu(np.stack([c["z"]] * 2))[None]
    grids = [cu(np.stack([g] * 2))[None] for g in c["grids"]]
    out = V.synthesize_views(lab, p, noise=z, grids=grids)
    assert out.shape == (1, 2) + c["labels"].shape and out.dtype == torch.float32
    for v, (ref64, e32) in enumerate(appearance_reference(name)):
        check_image(f"appearance {name} view {v}", out[0, v], ref64, e32)
    # the reference's own recorded output (view 0 has the fixture's flag), under the same bound
    got = DR.at(out[0, 0].double().cpu().numpy(), c["index"])
    err = float(np.abs(got - c["view"]).max() / np.abs(c["view"]).max())
    print(f"appearance {name}: against the reference's recorded view {err:.3e}")
    assert err <= DR.BOUND(appearance_reference(name)[0][1])
    assert torch.equal(out, V.synthesize_views(lab, p, noise=z, grids=grids)), "two runs differ"
    off = V.synthesize_views(offset_by_one(lab), p, noise=offset_by_one(z), grids=[offset_by_one(g) for g in grids])
    assert torch.equal(out, off), "inputs one element off the alignment give other bits"
    # alone against the first sample of a batch of 3 whose other samples differ
    p3 = appearance_params(c, 3)
    lab3 = torch.cat([lab, lab.flip(-1), lab.flip(-2)])
    z3 = torch.cat([z, -z, z.flip(-1)])
    grids3 = [torch.cat([g, -g, 2 * g]) for g in grids]
    out3 = V.synthesize_views(lab3, p3, noise=z3, grids=grids3)
    assert torch.equal(out3[0], out[0]), "a sample alone differs from the same sample in a batch"
    assert not torch.equal(out3[1], out[0])


def test_appearance_pass_one_statistics():
    """amx_synth_gmm_minmax alone: the minimum and maximum of g, which is never stored."""
    c = fixture_case("mid")
    p = appearance_params(c)
    lab, z = cu(c["labels"])[None, None], cu(np.stack([c["z"]] * 2))[None]
    t = V._appearance_table(p, 1).device(dev())
    n, vox = 2, c["labels"].size
    sc, nb = V._scratch(n, vox, dev())
    _lib.check_envelope(_lib.load().amx_synth_gmm_minmax(_lib.ptr(lab), _lib.ptr(z), 1, vox, *t.args, _lib.ptr(sc), nb, _lib.stream(dev())))
    mm = V._finalize(sc, nb, n, vox, dev()).cpu().numpy()
    for v, zb in enumerate((c["zero_background"], not c["zero_background"])):
        g64, e32 = e32_of(lambda dt: DR.gmm_raw(c["labels"], c["means"], c["stds"], c["z"], zb, dt))
        print(f"view {v}: min {mm[v, 0]} max {mm[v, 1]} against {g64.min()} {g64.max()}, e32 {e32:.2e}")
        assert abs(mm[v, 0] - g64.min()) <= DR.BOUND(e32) * g64.max() and abs(mm[v, 1] - g64.max()) <= DR.BOUND(e32) * g64.max()


def test_appearance_leaves_the_statistics_of_its_output():
    """The partials of pass 2 finalize to the minimum and maximum of the views it wrote, exactly."""
    c = fixture_case("odd")
    p = appearance_params(c)
    lab, z = cu(c["labels"])[None, None], cu(np.stack([c["z"]] * 2))[None]
    grids = [cu(np.stack([g] * 2))[None] for g in c["grids"]]
    t = V._appearance_table(p, 1).device(dev())
    out, sc, nb = V._appearance(lab, p, z.view(2, 1, *z.shape[2:]), [g.view(2, 1, *g.shape[2:]) for g in grids], t)
    mm = V._finalize(sc, nb, 2, c["labels"].size, dev())
    want = torch.stack([out[0].flatten(1).min(1).values, out[0].flatten(1).max(1).values], 1)
    assert torch.equal(mm, want)


SPIKE_CASES = [((6, 8, 10), [(0, 0, 0), (3, 4, 5), (0, 4, 5)]), ((16, 16, 16), [(15, 15, 15), (8, 8, 8), (0, 8, 3)])]


@pytest.mark.parametrize("shape,locs", SPIKE_CASES, ids=["6x8x10", "16x16x16"])
def test_kspace_spike_noise(shape, locs):
    """One view per location (a corner, the centre n // 2 = DC, index 0 of an even axis), the default intensity with its factor and a
    fixed one.  Also amx_synth_logk_mean alone."""
    x = np.random.RandomState(4).uniform(0, 1, (len(locs), 1) + shape).astype(np.float32)
    d = cu(x)
    factors = [1.0, 0.97, 1.08][:len(locs)]
    got = V.kspace_spike_noise(d, locs, factor=factors)
    fixed = V.kspace_spike_noise(d, locs, k_intensity=3.5)
    for i, loc in enumerate(locs):
        ref64, e32 = e32_of(lambda dt: DR.spike(x[i, 0], loc, None, factors[i], dt))
        check_image(f"spike {shape} loc {loc} default", got[i, 0], ref64, e32)
        assert np.abs(ref64 - x[i, 0]).max() > 1e-4
        ref64, e32 = e32_of(lambda dt: DR.spike(x[i, 0], loc, 3.5, 1.0, dt))
        check_image(f"spike {shape} loc {loc} fixed", fixed[i, 0], ref64, e32)
    assert torch.equal(got, V.kspace_spike_noise(d, locs, factor=factors))
    assert torch.equal(got, V.kspace_spike_noise(offset_by_one(d), locs, factor=factors))
    alone = V.kspace_spike_noise(d[1:2], locs[1], factor=factors[1])
    ref64, e32 = e32_of(lambda dt: DR.spike(x[1, 0], locs[1], None, factors[1], dt))
    check_image(f"spike {shape} alone", alone[0, 0], ref64, e32)
    # the reduction alone
    k = torch.view_as_real(torch.fft.fftn(d[:, 0], dim=(-3, -2, -1)).contiguous())
    mean = torch.empty(len(locs), dtype=torch.float32, device=dev())
    sc, nb = V._scratch(len(locs), x[0].size, dev())
    _lib.check_envelope(_lib.load().amx_synth_logk_mean(_lib.ptr(k), len(locs), x[0].size, _lib.ptr(mean), _lib.ptr(sc), nb, _lib.stream(dev())))
    want = np.array([np.log(np.abs(np.fft.fftn(x[i, 0].astype(np.float64))) + 1e-10).mean() for i in range(len(locs))])
    err = np.abs(mean.cpu().numpy() - want).max() / np.abs(want).max()
    print(f"mean log|k| {shape}: {err:.3e}")
    assert err <= 5e-6 + 10 * 1.2e-7          # a mean of float32 logarithms accumulated in double: float32 rounding of its terms


@pytest.mark.parametrize("zoom", [0.5, 0.61, 0.77, 0.93, 1.0])
def test_simulate_low_resolution(zoom):
    shape = (17, 24, 31)
    x = np.random.RandomState(3).standard_normal((2, 1) + shape).astype(np.float32)
    d = cu(x)
    got = V.simulate_low_resolution(d, zoom)
    for i in range(2):
        ref64, e32 = e32_of(lambda dt: DR.low_resolution(x[i, 0], zoom, dt))
        check_image(f"low resolution zoom {zoom} sample {i}", got[i, 0], ref64, e32)
    if zoom == 1.0:
        assert torch.equal(got, d)
    assert torch.equal(got, V.simulate_low_resolution(d, zoom))
    assert torch.equal(got, V.simulate_low_resolution(offset_by_one(d), zoom))
    assert torch.equal(got[1:2], V.simulate_low_resolution(d[1:2], zoom))
    # per view: the second view with another zoom leaves the first as it was
    two = V.simulate_low_resolution(d, [zoom, 0.7])
    assert torch.equal(two[0], got[0])


@pytest.mark.parametrize("shape", [(17, 24, 31), (16, 16, 16)])
def test_clip_rescale(shape):
    x = np.random.RandomState(6).standard_normal((3, 1) + shape).astype(np.float32)
    x[2] = -np.abs(x[2])                                  # nothing above 0: min == max == 0 after the clip
    d = cu(x)
    got, u8 = V.clip_rescale(d), V.clip_rescale(d, torch.uint8)
    for i in range(2):
        ref64, e32 = e32_of(lambda dt: DR.tail(x[i, 0], dt))
        check_image(f"tail {shape} sample {i}", got[i, 0], ref64, e32)
    assert torch.count_nonzero(got[2]) == 0 and torch.count_nonzero(u8[2]) == 0
    assert u8.dtype == torch.uint8 and torch.equal(u8, (got * 255).to(torch.uint8))
    assert int(u8.max()) == 255 and int(u8.min()) == 0
    assert torch.equal(got, V.clip_rescale(offset_by_one(d))) and torch.equal(u8, V.clip_rescale(offset_by_one(d), torch.uint8))


# ---- the chain ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def chain_case(pattern):
    return DR.chain_case(V.draw_params, pattern)


@functools.lru_cache(maxsize=None)
def chain_reference(pattern):
    return DR.chain_reference(chain_case(pattern))


def chain_inputs(pattern):
    labs, p, z, grids = chain_case(pattern)
    return cu(np.stack(labs))[:, None], p, cu(z), [cu(g) for g in grids]


def one_sample(p, b):
    q = {k: (v[b:b + 1] if isinstance(v, (list, np.ndarray)) else v) for k, v in p.items() if k != "on"}
    q["on"] = {k: v[b:b + 1] for k, v in p["on"].items()}
    return q


@pytest.mark.parametrize("pattern", list(DR.PATTERNS))
def test_generate_views_against_the_restatement(pattern):
    lab, p, z, grids = chain_inputs(pattern)
    got = V.generate_views(lab, p, dtype=torch.float32, noise=z, grids=grids)
    assert got.shape == (3, 2) + DR.CHAIN_SHAPE and got.dtype == torch.float32
    ref = chain_reference(pattern)
    for r, (ref64, e32) in enumerate(ref):
        check_image(f"chain {pattern} sample {r // 2} view {r % 2}", got[r // 2, r % 2], ref64, e32)
    assert torch.equal(got, V.generate_views(lab, p, dtype=torch.float32, noise=z, grids=grids)), "two runs of the chain differ"
    off = V.generate_views(offset_by_one(lab), p, dtype=torch.float32, noise=offset_by_one(z), grids=[offset_by_one(g) for g in grids])
    assert torch.equal(got, off), "inputs one element off the alignment give other bits"
    # a sample alone: within the bound (the FFTs of the spike and of Gibbs are batched)
    alone = V.generate_views(lab[1:2], one_sample(p, 1), dtype=torch.float32, noise=z[1:2], grids=[g[1:2] for g in grids])
    for v in range(2):
        check_image(f"chain {pattern} sample 1 alone view {v}", alone[0, v], *ref[2 + v])
    # augment_views on the appearance model's output is the same chain
    views = V.synthesize_views(lab, p, noise=z, grids=grids)
    assert torch.equal(V.augment_views(views, p), got)

    # uint8: the same pass truncates 255 y
    u8 = V.generate_views(lab, p, dtype=torch.uint8, noise=z, grids=grids)
    assert u8.dtype == torch.uint8 and torch.equal(u8, (got * 255).to(torch.uint8))
    inside = []
    for r, (ref64, e32) in enumerate(ref):
        mine = u8[r // 2, r % 2].cpu().numpy().astype(np.int64)
        want = np.trunc(255.0 * ref64).astype(np.int64)
        band = DR.uint8_band(ref64, DR.BOUND(e32))
        inside.append(band)
        print(f"chain {pattern} row {r} uint8: {int((mine != want).sum())} voxels differ, {100 * band.mean():.3f} % within the band")
        assert np.abs(mine - want).max() <= 1
        assert not ((mine != want) & ~band).any(), "a uint8 value differs where 255 ref64 is not within 255 bound of an integer >= 1"
    assert np.mean(inside) <= 0.02


def test_generate_views_draws_its_fields_from_the_seed():
    lab, p, _, _ = chain_inputs("mixed")
    a, b = (V.generate_views(lab, p) for _ in range(2))
    assert a.dtype == torch.uint8 and torch.equal(a, b) and int(a.max()) == 255
    alone = V.generate_views(lab[2:3], one_sample(p, 2))
    diff = (alone[0].int() - a[2].int()).abs()
    assert int(diff.max()) <= 1                                   # its own seed: the same fields whatever the batch
    z, grids = V.draw_fields(p, dev())
    z1, grids1 = V.draw_fields(one_sample(p, 2), dev())
    assert torch.equal(z[2:3], z1) and all(torch.equal(g[2:3], h) for g, h in zip(grids, grids1))


def test_envelope_refusals():
    lab, p, z, grids = chain_inputs("off")
    with pytest.raises(RuntimeError, match="no host path"):
        V.generate_views(lab.cpu(), p)
    with pytest.raises(TypeError, match="uint8"):
        V.generate_views(lab.float(), p)
    with pytest.raises(ValueError, match=r"\[B, 1, D, H, W\]"):
        V.generate_views(lab[:, 0], p)
    with pytest.raises(TypeError, match="float32"):
        V.generate_views(lab, p, noise=z.double(), grids=grids)
    with pytest.raises(ValueError, match="both or neither"):
        V.generate_views(lab, p, noise=z)
    with pytest.raises(TypeError, match="dtype"):
        V.generate_views(lab, p, dtype=torch.float16)
    bad = dict(p, scales=(4, 5))
    with pytest.raises(_lib.AmxEnvelopeError):
        V.generate_views(lab, bad)
    with pytest.raises(ValueError, match="drawn for"):
        V.generate_views(lab[..., :28], p)
    one = dict(one_sample(p, 0), unique_labels=[np.array([3])], means=[np.ones((2, 1))], stds=[np.ones((2, 1))],
               zero_background=np.array([[True, False]]))
    with pytest.raises(ValueError, match="constant volume"):
        V.generate_views(torch.full_like(lab[:1], 3), one)
    with pytest.raises(ValueError, match="loc"):
        V.kspace_spike_noise(z, (16, 0, 0))
    with pytest.raises(ValueError, match="zoom"):
        V.simulate_low_resolution(z, 1.5)
    # the library's own checks, without the Python layer in front
    lib = _lib.load()
    t = V._Table(2)
    t.host["flags"], t.host["nlabels"] = V.ZERO_BACKGROUND, 1
    t.device(dev())
    sc, nb = V._scratch(2, 64, dev())
    u = torch.zeros(64, dtype=torch.uint8, device=dev())
    f = torch.zeros(128, dtype=torch.float32, device=dev())
    assert lib.amx_synth_gmm_minmax(_lib.ptr(u), _lib.ptr(f), 1, 64, *t.args, _lib.ptr(sc), nb, None) == _lib.AMX_ERR_INVALID
    t.host["flags"] = 0
    gp, scales = (ctypes.c_void_p * 1)(f.data_ptr()), (ctypes.c_int * 1)(3)
    assert lib.amx_synth_appearance(_lib.ptr(u), _lib.ptr(f), gp, scales, 1, _lib.ptr(f), _lib.ptr(f), 1, 4, 4, 4, *t.args, _lib.ptr(sc), nb,
                                    None) == _lib.AMX_ERR_SHAPE
    t.host["flags"], t.host["lowres"] = V.LOWRES, 9
    assert lib.amx_synth_lowres(_lib.ptr(f), _lib.ptr(f[64:]), 1, 4, 4, 4, *t.args, None) == _lib.AMX_ERR_INVALID
    assert lib.amx_synth_clip_minmax(_lib.ptr(f), 2, 64, _lib.ptr(sc), 8, None) == _lib.AMX_ERR_WORKSPACE


def test_command_line_round_trip(tmp_path):
    """A directory of uint8 label maps becomes view1/ and view2/ files that load back as uint8 in [0, 255]; a volume does not depend
    on the batch it was generated in."""
    from anatomix_amd.datagen.step2_generate_views import main
    from anatomix_amd.io.nifti import load_nifti, save_nifti
    src = tmp_path / "label_ensembles"
    src.mkdir()
    for i, labels in enumerate(DR.CHAIN_LABELS):
        save_nifti(str(src / f"ensemble_{i}.nii.gz"), DR.label_blobs((32, 32, 32), labels, 40 + i), dtype=np.uint8)
    outs = []
    for bs in (3, 1):
        out = tmp_path / f"views_{bs}"
        main(["--ensembledir", str(src), "--savedir", str(out), "--batch_size", str(bs), "--seed", "5", "--end_idx", "3"])
        outs.append(out)
    for i in range(3):
        for v in (1, 2):
            a, aff, hdr = load_nifti(str(outs[0] / f"view{v}" / f"view{v}_ensemble_{i}.nii.gz"))
            b = load_nifti(str(outs[1] / f"view{v}" / f"view{v}_ensemble_{i}.nii.gz"))[0]
            assert hdr["datatype"] == 2 and a.shape == (32, 32, 32) and np.array_equal(aff, np.eye(4))
            assert a.min() == 0 and a.max() == 255 and np.array_equal(a, np.round(a))
            assert np.abs(a - b).max() <= 1
