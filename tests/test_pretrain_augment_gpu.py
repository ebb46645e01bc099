"""GPU: the two-view augmentation of the contrastive pretraining (csrc/amx_preaug.hip through anatomix_amd.pretraining.augment and
.loader), each transform alone and the whole chain, against the float64 numpy restatement tests/_preaug_ref.py (which
tests/test_pretrain_augment.py pins to grid_sample, scipy's gaussian_filter, polygrid3d and the 3-D FFT definition; parity with TorchIO
is unpinned).

Bound, the project's own: max |got - ref64| <= (5e-6 + 10 x e32) x max |ref64|, with e32 the distance of the
float32 evaluation of the same restatement from its float64 evaluation, computed here per case and printed; nothing comes from the
code under test.  Labels must agree exactly at every voxel whose source index is at least 1e-4 from a half-integer on all three
axes, and at most 0.5 % of the voxels may be excluded that way; flip-only and identity maps must be exact everywhere.

Shapes: (12, 10, 8), the fixture's, V % 4 == 0; (9, 11, 7), V and H W odd, so the scalar access forms run, and every axis is shorter
than the sigma-2 radius of 8, so the reflection repeats; (37, 35, 70), which crosses the blur's tiles on every axis by a non-multiple:
32 planes of the z march, 32 rows and 64 columns of the plane tile, 1024 columns of the flattened plane (the issue's 37 x 30 x 41 stays
inside one 32 x 64 plane tile, so H and W were raised past it)."""
import functools
import os
import shutil
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _preaug_ref as PR

pytestmark = pytest.mark.gpu

SHAPES = {"fixture": (12, 10, 8), "odd": (9, 11, 7), "tiles": (37, 35, 70)}
ON = dict.fromkeys(PR.INTENSITY, True)
OFF = dict.fromkeys(PR.INTENSITY, False)
PATTERNS = {"on": (True, ON, ON), "off": (False, OFF, OFF), "a_only": (True, ON, OFF), "b_only": (True, OFF, ON)}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_view_train_data.hdf5")


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def offset_by_one(t):
    """The same values one element into a larger buffer: contiguous, base not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.is_contiguous() and (out.data_ptr() % 16 != 0 or t.element_size() == 1)
    return out


@functools.lru_cache(maxsize=None)
def pair(case):
    """Two views (float32 numpy, as the device holds them) and their label map (float64 numpy) of one shape."""
    a, lab = PR.blob_volume(SHAPES[case], 200)
    b, _ = PR.blob_volume(SHAPES[case], 201)
    return np.stack([a, 0.5 * a + 0.7 * b]).astype(np.float32), lab


def check_image(tag, got, ref64, e32):
    got = got.detach().double().cpu().numpy()
    err, bound = float(np.abs(got - ref64).max() / np.abs(ref64).max()), 5e-6 + 10 * e32
    print(f"{tag}: max err / max|ref64| {err:.3e} bound {bound:.3e} (e32 {e32:.2e}, max|ref64| {np.abs(ref64).max():.4f})")
    assert got.shape == ref64.shape and np.isfinite(got).all() and err <= bound, (tag, err, bound)


def check_labels(tag, got, want, src, exact=False):
    sure = np.ones(want.shape, bool) if exact else PR.half_integer_margin(src) >= 1e-4
    excluded = 1.0 - sure.mean()
    wrong = int((got.cpu().numpy()[sure] != want[sure]).sum())
    print(f"{tag}: {wrong} wrong labels of {int(sure.sum())}, {100 * excluded:.3f} % excluded, labels present {np.unique(want).tolist()}")
    assert excluded <= 0.005 and wrong == 0


def e32_of(fn):
    a, b = fn(np.float64), fn(np.float32)
    return a, float(np.abs(b.astype(np.float64) - a).max() / np.abs(a).max())


ALONE = [(c, u) for c in SHAPES for u in (False, True) if not (u and c == "tiles")]
ALONE_IDS = [f"{c}{'_unaligned' if u else ''}" for c, u in ALONE]


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_flip_affine(case, unaligned):
    from anatomix_amd.pretraining.augment import flip_affine
    x, lab = pair(case)
    shape = SHAPES[case]
    xd, ld = cu(x), cu(lab).to(torch.uint8)
    if unaligned:
        xd, ld = offset_by_one(xd), offset_by_one(ld)
    keep = xd.clone()
    for seed in range(6):
        M = PR.seeded_map(seed, shape)
        got, glab = flip_affine(xd, ld, matrix=M)
        assert got.shape == xd.shape and glab.shape == ld.shape and glab.dtype == torch.uint8
        for v in range(2):
            ref, e32 = e32_of(lambda dt: PR.resample(x[v], lab, M, x[v].min(), dt)[0])
            check_image(f"flip_affine {case} map {seed} view {v}", got[v], ref, e32)
        _, want, src = PR.resample(x[0], lab, M, 0.0, np.float64)
        check_labels(f"flip_affine {case} map {seed}", glab, want, src, exact=PR.is_integral_map(M))
    assert torch.equal(xd, keep)
    # flips and the identity copy bit for bit; flip_axes builds the same map
    got, glab = flip_affine(xd, ld, flip_axes=(True, False, True))
    assert torch.equal(got, xd.flip(1, 3)) and torch.equal(glab, ld.flip(0, 2))
    got, glab = flip_affine(xd, ld)
    assert torch.equal(got, xd) and torch.equal(glab, ld)
    one, none = flip_affine(xd[0], None, scales=(0.8, 1.1, 1.3), degrees=(10.0, -30.0, 45.0))
    two, _ = flip_affine(xd, ld, scales=(0.8, 1.1, 1.3), degrees=(10.0, -30.0, 45.0))
    assert none is None and torch.equal(one[0], two[0])


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_blur(case, unaligned):
    from anatomix_amd.pretraining.augment import blur
    x, _ = pair(case)
    xd = offset_by_one(cu(x)) if unaligned else cu(x)
    keep = xd.clone()
    for sig in (np.array([[0.0, 0.05, 2.0], [2.0, 0.7, 0.0]]), np.array([[1.3, 2.0, 0.05], [0.124, 0.126, 1.9]]), np.array([[2.0] * 3, [0.0] * 3])):
        got = blur(xd, sig)                                          # radii 0, 0, 8 / 8, 3, 0; 5, 8, 0 / 0, 1, 8; 8, 8, 8 / none
        for v in range(2):
            ref, e32 = e32_of(lambda dt: PR.blur(x[v], sig[v], dt))
            check_image(f"blur {case} sigma {sig[v].tolist()} view {v}", got[v], ref, e32)
    assert torch.equal(got[1], xd[1]), "sigma 0 on every axis is a copy"
    assert torch.equal(xd, keep)
    assert torch.equal(blur(xd[0], 1.0)[0], blur(xd, [[1.0] * 3, [0.3] * 3])[0])


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_noise_bias_field_and_gamma(case, unaligned):
    from anatomix_amd.pretraining.augment import add_noise, bias_field, gamma
    x, _ = pair(case)
    x = x - np.float32(0.3)                                           # some negative voxels for the gamma's sign rule
    nz = torch.randn((2,) + SHAPES[case], generator=torch.Generator().manual_seed(5)).numpy()
    xd, nd = cu(x), cu(nz)
    if unaligned:
        xd, nd = offset_by_one(xd), offset_by_one(nd)
    keep = xd.clone()
    stds, gammas = [0.25, 0.0], [float(np.exp(-0.4)), float(np.exp(0.4))]
    coeff = np.random.RandomState(3).uniform(-0.5, 0.5, (2, 20))
    got_n, got_b, got_g = add_noise(xd, stds, nd), bias_field(xd, coeff), gamma(xd, gammas)
    assert torch.equal(xd, keep)
    for v in range(2):
        ref, e32 = e32_of(lambda dt: PR.add_noise(x[v], stds[v], nz[v], dt))
        check_image(f"add_noise {case} view {v}", got_n[v], ref, e32)
        ref, e32 = e32_of(lambda dt: PR.bias_field(x[v], coeff[v], dt))
        check_image(f"bias_field {case} view {v}", got_b[v], ref, e32)
        ref, e32 = e32_of(lambda dt: PR.gamma(x[v], gammas[v], dt))
        check_image(f"gamma {case} view {v}", got_g[v], ref, e32)
    assert torch.equal(got_n[1], xd[1]), "std 0 adds nothing"
    assert bool((got_g[xd < 0] < 0).all()) and bool((got_g[xd == 0] == 0).all())


@pytest.mark.parametrize("case", list(SHAPES))
def test_motion(case):
    from anatomix_amd.pretraining.augment import motion
    x, _ = pair(case)
    r = np.random.RandomState(8)
    deg, tr = r.uniform(-10, 10, (2, 3)), r.uniform(-10, 10, (2, 3))
    times = np.array([1 / 3, 2 / 3]) + r.uniform(-0.1, 0.1, 2)
    xd = cu(x[0])
    got = motion(xd, deg, tr, times)
    ref, e32 = e32_of(lambda dt: PR.motion(x[0], deg, tr, times, dt))           # the 3-D definition
    check_image(f"motion {case}", got, ref, e32)
    assert torch.equal(xd, cu(x[0])) and torch.equal(got, motion(xd, deg, tr, times))


@functools.lru_cache(maxsize=None)
def chain_params(case, pattern):
    """Seeded parameters with the pattern's switches forced, every range at a value that exercises it, and the crop of 6."""
    from anatomix_amd.pretraining.augment import draw_params, spatial_map
    shape = SHAPES[case]
    p = draw_params(np.random.RandomState(21), shape, Namespace(crop_size=6, isTrain=True))
    spatial, on_a, on_b = PATTERNS[pattern]
    p["flip_axes"], p["affine_on"] = np.array([True, False, True]), spatial
    p["flip_on"] = spatial
    p["map"] = spatial_map(shape, p["flip_axes"], p["scales"], p["degrees"]) if spatial else None
    for rec, on in zip(p["views"], (on_a, on_b)):
        rec["on"] = dict(on)
    p["views"][0]["sigma"] = np.array([2.0, 0.9, 1.4])
    return p


@functools.lru_cache(maxsize=None)
def chain_noise(case):
    return torch.randn((2,) + SHAPES[case], generator=torch.Generator().manual_seed(6)).numpy()


@functools.lru_cache(maxsize=None)
def chain_reference(case, pattern):
    """(images64 [2], label, source indices, e32 [2]) of the whole volumes (the crop is checked as a window of them), computed once and
    left unchanged."""
    x, lab = pair(case)
    p, nz = dict(chain_params(case, pattern), crop_size=0), chain_noise(case)
    v64, y, src = PR.chain(x[0], x[1], lab, p, nz, np.float64)
    v32, _, _ = PR.chain(x[0], x[1], lab, p, nz, np.float32)
    return v64, y, src, [float(np.abs(b.astype(np.float64) - a).max() / np.abs(a).max()) for a, b in zip(v64, v32)]


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("case", list(SHAPES))
def test_chain_against_the_restatement(case, pattern):
    from anatomix_amd.pretraining.augment import augment_pair
    x, lab = pair(case)
    p = chain_params(case, pattern)
    A, B, seg, nz = cu(x[0])[None], cu(x[1])[None], cu(lab).float()[None], cu(chain_noise(case))
    keep = (A.clone(), B.clone(), seg.clone())
    out = augment_pair(A, B, seg, p, crop_size=6, noise=nz)
    assert all(t.shape == (1, 6, 6, 6) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() for t in out)
    assert torch.equal(A, keep[0]) and torch.equal(B, keep[1]) and torch.equal(seg, keep[2]), "an input was modified"
    whole = augment_pair(A, B, seg, p, noise=nz)                      # crop_size 0: the whole volumes
    win = (slice(None),) + tuple(slice(s, s + 6) for s in p["crop_start"])
    assert whole[0].shape == A.shape and all(torch.equal(w[win], o) for w, o in zip(whole, out)), "the crop is a window of the whole"
    v64, y, src, e32 = chain_reference(case, pattern)
    for v in range(2):
        check_image(f"chain {case} {pattern} view {v}", whole[v][0], v64[v], e32[v])
    assert torch.equal(out[2], out[3]) and out[2].data_ptr() != out[3].data_ptr()
    check_labels(f"chain {case} {pattern}", whole[2][0], y, src, exact=src is None)
    again = augment_pair(A, B, seg, p, crop_size=6, noise=nz)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), "two runs of one pair differ"
    shifted = augment_pair(offset_by_one(A), offset_by_one(B), offset_by_one(seg.to(torch.uint8)), p, crop_size=6, noise=offset_by_one(nz))
    assert all(torch.equal(a, b) for a, b in zip(out, shifted))
    # a view with every switch off (and no spatial transform) is its input, bit for bit
    if pattern == "off":
        assert torch.equal(whole[0], A) and torch.equal(whole[1], B) and torch.equal(whole[2], seg)


def test_a_view_that_is_off_passes_every_kernel_bit_for_bit():
    """A on / B off and the reverse through each kernel directly: the off view of the stage's output is its input."""
    from anatomix_amd.pretraining import augment as G
    for case in SHAPES:
        x, lab = pair(case)
        xd, ld = cu(x), cu(lab).to(torch.uint8)
        nz = cu(chain_noise(case))
        for off in (0, 1):
            p = chain_params(case, "a_only" if off == 1 else "b_only")
            t = G.build_table(p)
            t.host["flags"][off] = 0
            t.device(dev())
            sp, slab = G._spatial(xd, ld, t, G._minmax(xd))
            bl = G._blur(xd, t)
            it = G._intensity(xd, nz, torch.empty_like(xd), t)
            for name, got in (("spatial", sp), ("blur", bl), ("intensity", it)):
                assert torch.equal(got[off], xd[off]), (case, name, off)
                assert not torch.equal(got[1 - off], xd[1 - off]), (case, name, off)
            assert torch.equal(slab, ld) == (off == 0)              # the label follows view A's switch


def test_noise_defaults_to_the_seeded_generators():
    from anatomix_amd.pretraining.augment import augment_pair
    case = "fixture"
    x, lab = pair(case)
    p = chain_params(case, "on")
    A, B, seg = cu(x[0]), cu(x[1]), cu(lab).to(torch.uint8)
    nz = torch.stack([torch.randn(SHAPES[case], generator=torch.Generator(dev()).manual_seed(r["noise_seed"]), device=dev()) for r in p["views"]])
    a, b = augment_pair(A, B, seg, p), augment_pair(A, B, seg, p, noise=nz)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_outside_the_envelope_raises_before_any_launch():
    from anatomix_amd import _lib
    from anatomix_amd.pretraining import augment as G
    x = torch.rand(2, 8, 8, 8, device=dev())
    with pytest.raises(_lib.AmxEnvelopeError, match="radius 9") as e:
        G.blur(x, 2.2)                                               # int(4 x 2.2 + 0.5) = 9
    assert e.value.code == _lib.AMX_ERR_INVALID
    with pytest.raises(_lib.AmxEnvelopeError, match="bias coefficient 7 is not finite") as e:
        G.bias_field(x, [0.1] * 7 + [float("inf")] + [0.0] * 12)
    assert e.value.code == _lib.AMX_ERR_INVALID
    with pytest.raises(_lib.AmxEnvelopeError, match="gamma"):
        G.gamma(x, float("nan"))
    with pytest.raises(_lib.AmxEnvelopeError, match="map entry"):
        G.flip_affine(x, matrix=np.full((3, 4), np.nan))
    # the C entries themselves: overlapping buffers, a null table
    lib = _lib.load()
    t = G._Table(2)
    t.host["flags"] = G.BLUR | G.SPATIAL
    t.host["radius"] = 1
    t.device(dev())
    out, tmp, mm = torch.empty_like(x), torch.empty_like(x), torch.zeros(2, 2, device=dev())
    st = _lib.stream(dev())
    assert lib.amx_preaug_blur(_lib.ptr(x), _lib.ptr(x), _lib.ptr(tmp), 2, 8, 8, 8, *t.args, st) == _lib.AMX_ERR_INVALID
    assert b"overlap" in lib.amx_last_error()
    assert lib.amx_preaug_blur(_lib.ptr(x), _lib.ptr(out), _lib.ptr(x[1]), 2, 8, 8, 8, *t.args, st) == _lib.AMX_ERR_INVALID
    assert lib.amx_preaug_spatial(_lib.ptr(x), None, 2, 8, 8, 8, _lib.ptr(mm), _lib.ptr(x), None, *t.args, st) == _lib.AMX_ERR_INVALID
    assert lib.amx_preaug_intensity(_lib.ptr(x), None, _lib.ptr(x.view(-1)[4:]), 1, 8, 8, 8, *t.args, st) == _lib.AMX_ERR_INVALID
    assert lib.amx_preaug_blur(_lib.ptr(x), _lib.ptr(out), _lib.ptr(tmp), 2, 8, 8, 8, None, t.args[1], st) == _lib.AMX_ERR_INVALID
    assert lib.amx_preaug_blur(_lib.ptr(x), _lib.ptr(out), _lib.ptr(tmp), 2, 1 << 11, 1 << 10, 1 << 10, *t.args, st) == _lib.AMX_ERR_SHAPE
    t.host["radius"][1, 2] = 9
    assert lib.amx_preaug_blur(_lib.ptr(x), _lib.ptr(out), _lib.ptr(tmp), 2, 8, 8, 8, *t.args, st) == _lib.AMX_ERR_INVALID
    # no host path, one channel, float32
    p = G.draw_params(np.random.RandomState(0), (8, 8, 8), Namespace())
    for fn in (lambda t: G.blur(t, 1.0), lambda t: G.gamma(t, 1.2), lambda t: G.flip_affine(t), lambda t: G.augment_pair(t[:1], t[:1], t[:1], p)):
        with pytest.raises(RuntimeError, match="no host path"):
            fn(x.cpu())
        with pytest.raises(TypeError, match="float32"):
            fn(x.double())
    with pytest.raises(ValueError, match="one channel"):
        G.blur(x[None], 1.0)
    with pytest.raises(ValueError, match="one channel"):
        G.augment_pair(x, x, x, p)                                   # [2, 8, 8, 8]: two channels
    with pytest.raises(ValueError, match="drawn for"):
        G.augment_pair(x[0, :6], x[1, :6], x[0, :6], p)
    with pytest.raises(ValueError, match="crop_size"):
        G.augment_pair(x[0], x[1], x[0], p, crop_size=4)


# ---- the loader -------------------------------------------------------------------------------------------------------------------
def _opt(root, **kw):
    o = dict(dataroot=str(root), isTrain=True, data_ndims=3, load_mask=False, load_mode="twoview", view_order=False, crop_size=6,
             resize=False, augment=True, geo_augment=True, inten_augment=True, blur=True, noise=True, bias=True, gamma=True, motion=True,
             apply_same_inten_augment=False, batch_size=2)
    o.update(kw)
    return Namespace(**o)


@pytest.fixture()
def dataroot(tmp_path):
    shutil.copy(GOLD, tmp_path / "train_data.hdf5")
    shutil.copy(GOLD, tmp_path / "val_data.hdf5")
    return tmp_path


def _batches(loader, epoch=0):
    torch.manual_seed(11)                                             # the dataset's view draws (torch's global generator)
    np.random.seed(12)                                                # random_crop of the pass-through route
    loader.set_epoch(epoch)
    return list(loader)


def test_loader_yields_the_reference_batch_of_augmented_pairs(dataroot):
    from anatomix_amd.pretraining import AugmentedTwoViewLoader, H5SupCLDataset
    opt = _opt(dataroot)
    loader = AugmentedTwoViewLoader(opt, device=dev(), seed=3)
    first = _batches(loader)
    assert len(first) == len(loader) == 3 and opt.augment and opt.crop_size == 6, "the caller's options are not modified"
    for b in first:
        assert set(b) == {"A", "B", "A_seg", "B_seg", "A_id", "B_id", "meta", "keys"}
        for k in ("A", "B", "A_seg", "B_seg"):
            assert b[k].shape == (2, 1, 6, 6, 6) and b[k].dtype == torch.float32 and b[k].device == dev() and b[k].is_contiguous()
        assert torch.isfinite(b["A"]).all() and torch.isfinite(b["B"]).all()
        assert set(b["A_seg"].unique().tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0} and torch.equal(b["A_seg"], b["B_seg"])
        assert b["A_id"].shape == (2, 1) and b["A_id"].dtype == torch.int64 and torch.equal(b["A_id"], b["B_id"])
        assert b["meta"] == ["%06d" % i for i in b["A_id"][:, 0].tolist()]
        assert b["keys"] == [("A", "A"), ("B", "B"), ("A_seg", "A_seg"), ("B_seg", "B_seg")]
    assert sorted(i for b in first for i in b["A_id"][:, 0].tolist()) == list(range(6))
    # the same seed and epoch: the same batches; another epoch: another order or other parameters
    again = _batches(AugmentedTwoViewLoader(opt, device=dev(), seed=3))
    assert all(torch.equal(a[k], b[k]) for a, b in zip(first, again) for k in ("A", "B", "A_seg", "A_id"))
    other = _batches(loader, epoch=1)
    assert any(not torch.equal(a["A"], b["A"]) for a, b in zip(first, other))
    # it augments: with the same draws of the dataset, the pass-through loader gives other images
    plain = _batches(AugmentedTwoViewLoader(_opt(dataroot, augment=False), device=dev(), seed=3))
    assert any(not torch.equal(a["A"], b["A"]) for a, b in zip(first, plain))
    # the dataset itself still refuses, and so does resize
    with pytest.raises(NotImplementedError):
        H5SupCLDataset(opt)
    with pytest.raises(NotImplementedError):
        AugmentedTwoViewLoader(_opt(dataroot, resize=True), device=dev())


def test_loader_without_augmentation_is_the_dataset(dataroot):
    from anatomix_amd.pretraining import AugmentedTwoViewLoader, H5SupCLDataset
    opt = _opt(dataroot, augment=False)
    got = _batches(AugmentedTwoViewLoader(opt, device=dev(), seed=5))
    ds = H5SupCLDataset(opt)                                          # crops by itself with the same rule and the same global draws
    torch.manual_seed(11)
    np.random.seed(12)
    for b in got:
        for n, item in enumerate(b["A_id"][:, 0].tolist()):
            s = ds[item]
            for k in ("A", "B", "A_seg", "B_seg"):
                assert b[k][n].device == dev() and torch.equal(b[k][n].cpu(), s[k]), (item, k)
    # validation: the dataset's order, never cropped, never augmented; the mixed-shape subject needs batch size 1
    val = AugmentedTwoViewLoader(_opt(dataroot, isTrain=False, batch_size=1), device=dev())
    shapes = [tuple(b["A"].shape) for b in _batches(val)]
    assert [b for b in shapes] == [(1, 1, 12, 10, 8)] * 3 + [(1, 1, 9, 11, 7)] + [(1, 1, 12, 10, 8)] * 2
    with pytest.raises(ValueError, match="share a shape"):
        _batches(AugmentedTwoViewLoader(_opt(dataroot, isTrain=False, batch_size=4), device=dev()))
    # whole volumes of mixed shapes, augmented, one per batch
    whole = _batches(AugmentedTwoViewLoader(_opt(dataroot, crop_size=0, batch_size=1), device=dev(), seed=1))
    assert sorted(tuple(b["A"].shape) for b in whole) == sorted(shapes)


def test_loader_batches_feed_the_contrastive_step(dataroot):
    """The paper-default flags, volumes larger than the crop, one pair per batch: the batch goes into ``contrastive_step`` as it is.
    (The fixture's volumes are smaller than the UNet's receptive field, so the loader's dataset is replaced by an in-memory one with
    the same sample dictionary.)"""
    import contextlib
    import io
    import anatomix_amd
    from anatomix_amd.pretraining import AugmentedTwoViewLoader, PatchSampleF, SupPatchNCELoss, contrastive_step
    from oracle import pretrain_inputs as PI, unet_ref as R

    class InMemory:
        dimension = 3

        def __init__(self, n):
            self.items = [PR.blob_volume((72, 80, 72), 400 + i, n_labels=5) for i in range(n)]

        def __len__(self):
            return len(self.items)

        def __getitem__(self, i):
            img, lab = self.items[i]
            seg = torch.from_numpy(lab[None]).float()
            return {"A": torch.from_numpy(img[None]).float(), "B": torch.from_numpy(0.8 * img[None] + 0.05).float(), "A_seg": seg,
                    "B_seg": seg.clone(), "A_id": np.asarray([i]), "B_id": np.asarray([i]), "meta": "%06d" % i, "keys": ["A", "B", "A_seg", "B_seg"]}

    loader = AugmentedTwoViewLoader(_opt(dataroot, crop_size=64, batch_size=1), device=dev(), seed=2)
    loader.dataset = InMemory(2)
    batches = list(loader)
    assert len(batches) == 2 and all(b["A"].shape == (1, 1, 64, 64, 64) for b in batches)
    kw = R.VARIANTS["anatomix"]
    with contextlib.redirect_stdout(io.StringIO()):
        netG = anatomix_amd.Unet(**kw)
        netG.load_state_dict(R.synthetic_state_dict(kw, 3, gain=2 ** 0.5))
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
        netF.create_mlp([torch.zeros(1, c, 1, 1, 1, device=dev()) for c in (128, 256, 128, 64, 32, 16)])
    netG.precision = "bf16"
    netG, netF = netG.to(dev()).train(), netF.to(dev()).train()
    nopt = Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw")
    crits = [SupPatchNCELoss(nopt) for _ in PI.NCE_LAYERS]
    for b in batches:
        rec = contrastive_step(netG, netF, crits, b["A"], b["B"], b["A_seg"], PI.NCE_LAYERS, num_patches=64)
        assert np.isfinite(rec["loss"]) and rec["loss"] > 0
