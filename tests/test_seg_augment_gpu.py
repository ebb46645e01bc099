"""GPU: the augmentation chain of segmentation finetuning (csrc/amx_segaug.hip through anatomix_amd.segmentation.augment), each
transform alone and the whole chain, against the float64 numpy restatement tests/_segaug_ref.py (which tests/test_seg_augment.py pins
to grid_sample, leggrid3d and closed forms; parity with MONAI is unpinned).

Bound, the project's own: max |got - ref64| <= (5e-6 + 10 x e32) x max |ref64|, with e32 the distance of the
float32 evaluation of the same restatement from its float64 evaluation, computed here per case and printed; nothing comes from the
code under test.  Labels must agree exactly at every voxel whose source index is at least 1e-4 from a half-integer on all three
axes, and at most 0.5 % of the voxels may be excluded that way; under an identity matrix (affine off), where the source indices are
exact in both precisions, at every voxel.

Cases: B = 3 with crop 16 out of three volumes of different shapes (one of them exactly the crop); crop 15, so that V % 4 != 0 and the
scalar access form runs; crop 12 out of 20 x 9 x 14, where one axis is smaller than the crop and the affine kernel resamples
12 x 9 x 12 into 12^3."""
import functools

import numpy as np
import pytest
import torch

import _segaug_ref as AR

pytestmark = pytest.mark.gpu

CASES = {"crop16": (16, [(37, 30, 41), (16, 16, 16), (20, 33, 17)]),
         "crop15": (15, [(37, 30, 41), (16, 16, 16), (20, 33, 17)]),
         "crop12_short_axis": (12, [(20, 9, 14)] * 3)}
_ALT = {k: i % 2 == 0 for i, k in enumerate(AR.SWITCH_NAMES)}
PATTERNS = {"on": [dict.fromkeys(AR.SWITCH_NAMES, True)] * 3,
            "off": [dict.fromkeys(AR.SWITCH_NAMES, False)] * 3,
            "mixed": [dict.fromkeys(AR.SWITCH_NAMES, True), dict.fromkeys(AR.SWITCH_NAMES, False), _ALT],
            "mixed2": [{k: not v for k, v in _ALT.items()}, dict.fromkeys(AR.SWITCH_NAMES, True), dict.fromkeys(AR.SWITCH_NAMES, False)]}


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def offset_by_one(t):
    """The same values one element into a larger buffer: contiguous, base not 16-byte aligned."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    out = buf[1:].view(t.shape)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


@functools.lru_cache(maxsize=None)
def volumes(case):
    """Per sample: the resident volume as the device holds it (float32 numpy), its label map (float64 numpy)."""
    from anatomix_amd.segmentation.augment import make_resident
    _, shapes = CASES[case]
    out = []
    for i, s in enumerate(shapes):
        img, lab = AR.blob_volume(s, 100 + i)
        out.append((make_resident(img, dev()).cpu().numpy(), lab))
    return out


@functools.lru_cache(maxsize=None)
def batch_params(case, pattern):
    from anatomix_amd.segmentation.augment import draw_params
    crop, shapes = CASES[case]
    p = draw_params(np.random.RandomState(11), crop, shapes, 3)
    for b, sw in enumerate(PATTERNS[pattern]):
        for k, v in sw.items():
            p["on"][k][b] = v
        p["affine"][b] = AR.affine_matrix(p["rotate"][b], p["shear"][b], p["scale"][b]) if sw["affine"] else np.eye(3)
    return p


@functools.lru_cache(maxsize=None)
def batch_noise(case):
    crop, shapes = CASES[case]
    size = tuple(min(crop, s) for s in shapes[0])
    return torch.randn((3, 1) + size, generator=torch.Generator().manual_seed(5)).numpy()


@functools.lru_cache(maxsize=None)
def chain_reference(case, pattern):
    """Per sample (image64, label, source indices, e32), computed once and left unchanged."""
    p, nz = batch_params(case, pattern), batch_noise(case)
    out = []
    for b, (vol, lab) in enumerate(volumes(case)):
        x64, y, src = AR.chain_sample(vol, lab, p, b, nz[b, 0], np.float64)
        x32, _, _ = AR.chain_sample(vol, lab, p, b, nz[b, 0], np.float32)
        out.append((x64, y, src, float(np.abs(x32.astype(np.float64) - x64).max() / np.abs(x64).max())))
    return out


def check_image(tag, got, ref64, e32):
    got = got.detach().double().cpu().numpy()
    err, bound = float(np.abs(got - ref64).max() / np.abs(ref64).max()), 5e-6 + 10 * e32
    print(f"{tag}: max err / max|ref64| {err:.3e} bound {bound:.3e} (e32 {e32:.2e}, max|ref64| {np.abs(ref64).max():.4f})")
    assert np.isfinite(got).all() and err <= bound, (tag, err, bound)


def check_labels(tag, got, want, src, exact=False):
    """``exact``: the matrix is the identity, so the source indices are the same exact (half-)integers in float32 and float64 and
    the rounding to even is decided alike: every voxel must agree, also where a size difference puts all of them on half-integers."""
    sure = np.ones(want.shape, bool) if exact else AR.half_integer_margin(src) >= 1e-4
    excluded = 1.0 - sure.mean()
    wrong = int((got.cpu().numpy()[sure] != want[sure]).sum())
    print(f"{tag}: {wrong} wrong labels of {int(sure.sum())}, {100 * excluded:.3f} % excluded, labels present {np.unique(want).tolist()}")
    assert excluded <= 0.005 and wrong == 0


def e32_of(fn):
    a, b = fn(np.float64), fn(np.float32)
    return a, float(np.abs(b.astype(np.float64) - a).max() / np.abs(a).max())


@pytest.mark.parametrize("ldt", [torch.float32, torch.uint8], ids=["labels_f32", "labels_u8"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("case", list(CASES))
def test_chain_against_the_restatement(case, pattern, ldt):
    from anatomix_amd.segmentation.augment import augment_batch
    crop, shapes = CASES[case]
    p = batch_params(case, pattern)
    vols = [cu(v) for v, _ in volumes(case)]
    labs = [cu(l).to(ldt) for _, l in volumes(case)]
    keep = [v.clone() for v in vols]
    nz = cu(batch_noise(case))
    img, lab = augment_batch(vols, labs, p, noise=nz)
    assert img.shape == lab.shape == (3, 1, crop, crop, crop) and img.dtype == torch.float32 and lab.dtype == torch.uint8
    assert all(torch.equal(a, b) for a, b in zip(vols, keep)), "a resident volume was modified"
    for b, (x64, y, src, e32) in enumerate(chain_reference(case, pattern)):
        check_image(f"chain {case} {pattern} sample {b}", img[b, 0], x64, e32)
        check_labels(f"chain {case} {pattern} sample {b}", lab[b, 0], y, src, exact=not p["on"]["affine"][b])
    img2, lab2 = augment_batch(vols, labs, p, noise=nz)
    assert torch.equal(img, img2) and torch.equal(lab, lab2), "two runs of the chain differ"
    # resident volumes one element off the 16-byte alignment: the same values
    img3, lab3 = augment_batch([offset_by_one(v) for v in vols], [offset_by_one(l) for l in labs], p, noise=offset_by_one(nz))
    assert torch.equal(img, img3) and torch.equal(lab, lab3)


@pytest.mark.parametrize("case", ["crop16", "crop15"])
def test_a_sample_with_every_switch_off_is_its_rescaled_crop(case):
    from anatomix_amd.segmentation.augment import augment_batch
    crop, _ = CASES[case]
    for pattern, off in (("off", [0, 1, 2]), ("mixed", [1]), ("mixed2", [2])):
        p = batch_params(case, pattern)
        img, lab = augment_batch([cu(v) for v, _ in volumes(case)], [cu(l).float() for _, l in volumes(case)], p, noise=cu(batch_noise(case)))
        for b in off:
            vol, l = volumes(case)[b]
            c = AR.crop(vol, p["corner"][b], (crop,) * 3)
            want = (c - c.min()) / (c.max() - c.min())
            assert want.dtype == np.float32
            assert np.array_equal(img[b, 0].cpu().numpy(), want), (pattern, b)
            assert np.array_equal(lab[b, 0].cpu().numpy(), AR.crop(l, p["corner"][b], (crop,) * 3).astype(np.uint8))


def test_noise_defaults_to_the_seeded_generator():
    from anatomix_amd.segmentation.augment import augment_batch
    case = "crop16"
    p = batch_params(case, "on")
    vols, labs = [cu(v) for v, _ in volumes(case)], [cu(l).to(torch.uint8) for _, l in volumes(case)]
    nz = torch.randn((3, 1, 16, 16, 16), generator=torch.Generator(dev()).manual_seed(p["noise_seed"]), device=dev())
    a, b = augment_batch(vols, labs, p), augment_batch(vols, labs, p, noise=nz)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _inputs(case, unaligned):
    """A batch [3, 1, d, h, w] of crops (the first `size` voxels of each volume) on the device and as numpy."""
    crop, shapes = CASES[case]
    size = tuple(min(crop, s) for s in shapes[0])
    x = np.stack([AR.crop(v, (0, 0, 0), size) for v, _ in volumes(case)])[:, None]
    lab = np.stack([AR.crop(l, (0, 0, 0), size) for _, l in volumes(case)])[:, None]
    xd = cu(x)
    return (offset_by_one(xd) if unaligned else xd), x, lab, size


ALONE = [(c, u) for c in CASES for u in (False, True)]
ALONE_IDS = [f"{c}{'_unaligned' if u else ''}" for c, u in ALONE]


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_scale_intensity_and_adjust_contrast(case, unaligned):
    from anatomix_amd.segmentation.augment import adjust_contrast, scale_intensity
    xd, x, _, _ = _inputs(case, unaligned)
    x = x * 3.0 - 1.0
    xd = offset_by_one(cu(x)) if unaligned else cu(x)
    keep = xd.clone()
    got = scale_intensity(xd)
    gammas = [0.5, 2.2, 4.5]
    got_c = adjust_contrast(xd, gammas)
    assert torch.equal(xd, keep)
    for b in range(3):
        ref, e32 = e32_of(lambda dt: AR.scale_intensity(x[b, 0], dt))
        check_image(f"scale_intensity {case} sample {b}", got[b, 0], ref, e32)
        ref, e32 = e32_of(lambda dt: AR.adjust_contrast(x[b, 0], gammas[b], dt))
        check_image(f"adjust_contrast {case} gamma {gammas[b]} sample {b}", got_c[b, 0], ref, e32)
    flat = torch.full((2, 1, 3, 5, 7), 2.5, device=dev())
    assert bool((scale_intensity(flat) == 0).all()), "min == max gives x * 0"


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_noise_and_bias_field(case, unaligned):
    from anatomix_amd.segmentation.augment import bias_field, gaussian_noise
    xd, x, _, size = _inputs(case, unaligned)
    nz = batch_noise(case)
    stds = [0.02, 0.1, 0.0]
    coeff = np.random.RandomState(3).uniform(0, 0.05, (3, 20))
    got_n = gaussian_noise(xd, stds, offset_by_one(cu(nz)) if unaligned else cu(nz))
    got_b = bias_field(xd, coeff)
    for b in range(3):
        ref, e32 = e32_of(lambda dt: x[b, 0].astype(dt) + AR.f32(stds[b], dt) * nz[b, 0].astype(dt))
        check_image(f"gaussian_noise {case} sample {b}", got_n[b, 0], ref, e32)
        ref, e32 = e32_of(lambda dt: x[b, 0].astype(dt) * np.exp(AR.bias_exponent(size, coeff[b], dt)))
        check_image(f"bias_field {case} sample {b}", got_b[b, 0], ref, e32)
    assert torch.equal(got_n[2], xd[2]), "std 0 adds nothing"


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_gibbs_noise(case, unaligned):
    from anatomix_amd.segmentation.augment import gibbs_noise
    xd, x, _, size = _inputs(case, unaligned)
    alphas = [0.0, 0.2, 0.33]
    keep = xd.clone()
    got = gibbs_noise(xd, alphas)
    assert torch.equal(xd, keep)
    for b in range(3):
        ref, e32 = e32_of(lambda dt: AR.gibbs(x[b, 0], AR.gibbs_radius(alphas[b], size), dt))
        check_image(f"gibbs_noise {case} alpha {alphas[b]} sample {b}", got[b, 0], ref, e32)


@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_gaussian_smooth_and_sharpen(case, unaligned):
    from anatomix_amd.segmentation.augment import gaussian_sharpen, gaussian_smooth
    xd, x, _, _ = _inputs(case, unaligned)
    sig = np.array([[0.0, 0.05, 0.1], [0.3, 0.6, 1.0], [1.0, 0.75, 0.5]])          # radius 1, 1, 1 / 2, 3, 4 / 4, 3, 2
    s1 = np.array([[0.9, 0.6, 1.0], [0.5, 0.75, 0.8], [1.0, 1.0, 1.0]])
    s2 = np.array([[0.5, 0.55, 0.7], [0.5, 0.6, 0.5], [0.9, 0.5, 1.0]])
    alpha = [10.0, 30.0, 17.5]
    keep = xd.clone()
    got_s = gaussian_smooth(xd, sig)
    got_h = gaussian_sharpen(xd, s1, s2, alpha)
    assert torch.equal(xd, keep)
    for b in range(3):
        ref, e32 = e32_of(lambda dt: AR.gaussian(x[b, 0], sig[b], dt))
        check_image(f"gaussian_smooth {case} sigma {sig[b].tolist()} sample {b}", got_s[b, 0], ref, e32)
        ref, e32 = e32_of(lambda dt: AR.sharpen(x[b, 0], s1[b], s2[b], alpha[b], dt))
        check_image(f"gaussian_sharpen {case} sample {b}", got_h[b, 0], ref, e32)
    assert torch.equal(gaussian_smooth(xd, 0.0), xd), "sigma 0 is the identity"


@pytest.mark.parametrize("ldt", [torch.float32, torch.uint8], ids=["labels_f32", "labels_u8"])
@pytest.mark.parametrize("case,unaligned", ALONE, ids=ALONE_IDS)
def test_affine_resample(case, unaligned, ldt):
    from anatomix_amd.segmentation.augment import affine_resample
    crop, _ = CASES[case]
    xd, x, lab, size = _inputs(case, unaligned)
    ld = cu(lab).to(ldt)
    if unaligned:
        ld = offset_by_one(ld)
    A = np.stack([AR.seeded_matrix(s) for s in (0, 1, 2)])
    B = np.stack([AR.seeded_matrix(s) for s in (3, 4, 5)])
    for mats in (A, B):
        got, glab = affine_resample(xd, ld, matrix=mats, spatial_size=crop)
        assert got.shape == glab.shape == (3, 1, crop, crop, crop) and glab.dtype == torch.uint8
        for b in range(3):
            ref, e32 = e32_of(lambda dt: AR.affine(x[b, 0], lab[b, 0], mats[b], (crop,) * 3, dt)[0])
            _, want, src = AR.affine(x[b, 0], lab[b, 0], mats[b], (crop,) * 3, np.float64)
            check_image(f"affine {case} sample {b}", got[b, 0], ref, e32)
            check_labels(f"affine {case} sample {b}", glab[b, 0], want, src)
    # rotate / shear / scale build the same matrix
    r, sh, sc = (0.3, -0.2, 0.5), (0.1, -0.15, 0.05), (0.9, 1.1, 1.05)
    a = affine_resample(xd, ld, rotate=r, shear=sh, scale=sc, spatial_size=crop)
    b = affine_resample(xd, ld, matrix=AR.affine_matrix(r, sh, sc), spatial_size=crop)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the identity at equal sizes returns both inputs bit for bit
    got, glab = affine_resample(xd, ld, matrix=np.eye(3))
    assert torch.equal(got, xd) and torch.equal(glab, ld.to(torch.uint8))


def test_outside_the_envelope_raises_before_any_launch():
    from anatomix_amd._lib import AmxEnvelopeError
    from anatomix_amd.segmentation import augment as G
    x = torch.rand(2, 1, 8, 8, 8, device=dev())
    y = torch.zeros(2, 1, 8, 8, 8, device=dev())
    with pytest.raises(AmxEnvelopeError, match="radius"):
        G.gaussian_smooth(x, 1.5)
    with pytest.raises(AmxEnvelopeError, match="radius"):
        G.gaussian_sharpen(x, 1.5, 0.5, 10.0)
    two = torch.rand(2, 2, 8, 8, 8, device=dev())
    for fn in (G.scale_intensity, lambda t: G.adjust_contrast(t, 2.0), lambda t: G.gaussian_smooth(t, 0.5), lambda t: G.bias_field(t, np.zeros(20)),
               lambda t: G.gibbs_noise(t, 0.1), lambda t: G.affine_resample(t, y, matrix=np.eye(3))):
        with pytest.raises(ValueError, match="one channel"):
            fn(two)
        with pytest.raises(RuntimeError, match="no host path"):
            fn(x.cpu())
        with pytest.raises(TypeError, match="float32"):
            fn(x.double())
    p = G.draw_params(np.random.RandomState(0), 8, [(8, 8, 8)] * 2, 2)
    with pytest.raises(RuntimeError, match="no host path"):
        G.augment_batch([x[0, 0].cpu()] * 2, [y[0, 0].cpu()] * 2, p)
    with pytest.raises(ValueError, match="one channel"):
        G.augment_batch([two[0]] * 2, [y[0, 0]] * 2, p)
    with pytest.raises(TypeError):
        G.augment_batch([x[0, 0].double()] * 2, [y[0, 0]] * 2, p)
    with pytest.raises(AmxEnvelopeError, match="share"):
        G.augment_batch([x[0, 0], torch.rand(8, 6, 8, device=dev())], [y[0, 0], torch.zeros(8, 6, 8, device=dev())],
                        G.draw_params(np.random.RandomState(0), 8, [(8, 8, 8), (8, 6, 8)], 2))
    # a corner outside the volume is refused by the entry, not read
    bad = dict(p, corner=np.array([[0, 0, 1], [0, 0, 0]]))
    with pytest.raises(AmxEnvelopeError, match="leaves the volume"):
        G.augment_batch([x[0, 0]] * 2, [y[0, 0]] * 2, bad)
