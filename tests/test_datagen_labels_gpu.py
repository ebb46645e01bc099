"""GPU: step 1 of the synthetic data generation (csrc/amx_labels.hip through anatomix_amd.datagen.labels), every stage alone and
``generate_labels`` as a chain, against the numpy restatement tests/_labels_ref.py (which tests/test_datagen_labels.py pins to the
reference's recorded outputs and to scipy; parity with skimage is unpinned).

Everything is uint8 and must be EQUAL.  The two stages that round a real coordinate to a voxel leave out the voxels within the
restatement's margins of a rounding boundary (1e-9 of a float64 source coordinate for compose, 1e-4 of a float32 un-normalised
coordinate for the mask); at most 0.5 % of the voxels may be left out, and the share is printed.  The chain is checked without any
wider exclusion: it must equal its own stages run in sequence bit for bit, its compose and mask results are checked under the same
margins, and the numpy medians, apply and envelope run on those two results must equal the chain at every voxel."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import _labels_ref as LR
from anatomix_amd import _lib
from anatomix_amd.datagen import labels as L
from anatomix_amd.datagen import step1_generate_labels as S1
from test_seg_augment_gpu import cu, dev

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen_labels_golden.npz")
SHAPES = [(9, 11, 7), (12, 10, 9), (37, 35, 70)]
IDS = ["9x11x7", "12x10x9", "37x35x70"]


def host(t):
    return t.cpu().numpy()


def check_outside(tag, got, ref, near):
    share = float(near.mean())
    bad = int((got != ref)[~near].sum())
    print(f"{tag}: {share * 100:.4f} % of voxels left out (bound {LR.MAX_EXCLUDED * 100} %), {bad} mismatches outside, {int((got != ref).sum())} in all")
    assert share <= LR.MAX_EXCLUDED
    assert bad == 0


# ---- compose -------------------------------------------------------------------------------------------------------------------

def template_set(shape, count, seed):
    """``count`` blob templates whose crops are smaller than, equal to and larger than ``shape`` on different axes, with odd and even
    pads, some with zero margins that the crop removes."""
    d, h, w = shape
    sizes = [(d, h + 4, max(w - 3, 1)), (max(d - 2, 1), h, w + 1), (d + 5, max(h - 1, 1), w), (max(d // 2, 1), max(h // 2, 1), max(w // 2, 1)),
             (d + 1, h + 2, w + 3), (max(d - 5, 1), max(h - 4, 1), max(w - 1, 1))]
    return [LR.blob_template(tuple(n + 2 * (k % 2) for n in sizes[k % len(sizes)]), seed + k, margin=k % 2) for k in range(count)]


@functools.lru_cache(maxsize=None)
def compose_case(shape):
    """Two ensembles with 6 and 4 overlapping templates, their matrices in the reference's ranges, and the restatement."""
    r = np.random.RandomState(31)
    templates = [template_set(shape, 6, 100), template_set(shape, 4, 200)]
    affine = [np.stack([LR.random_affine(r, L.affine_matrix) for _ in ts]) for ts in templates]
    ref = [LR.compose(ts, a, shape) for ts, a in zip(templates, affine)]
    return templates, affine, ref


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_compose_against_the_restatement(shape):
    templates, affine, ref = compose_case(shape)
    out = L.compose_templates(templates, affine, shape)
    assert out.shape == (2, 1) + shape and out.dtype == torch.uint8
    for b, (lab, near) in enumerate(ref):
        check_outside(f"compose {shape} ensemble {b}", host(out[b, 0]), lab, near)
        # overlapping templates: more than one label survives, and the last template is visible
        assert len(np.unique(lab)) > 2 and lab.max() == len(templates[b]) - 1
    assert torch.equal(out, L.compose_templates(templates, affine, shape)), "two runs differ"
    # every template one byte further into the buffer: a misaligned base
    tab, ens, buf = L._tables(templates, dict(n_templates=[len(t) for t in templates], affine=affine), shape, base_offset=1)
    assert tab.host["offset"][0] == 1
    assert torch.equal(out, L._compose(tab.device(dev()), ens.device(dev()), cu(buf), shape, dev()))
    # an ensemble alone equals the same ensemble in the batch
    assert torch.equal(out[1:], L.compose_templates(templates[1:], affine[1:], shape))


def test_compose_a_single_template_gives_zeros():
    t = [LR.blob_template((12, 10, 9), 5)]
    out = L.compose_templates([t, t], [np.eye(4)[None], np.eye(4)[None]], (12, 10, 9))
    assert not out.any()


def test_compose_the_last_template_wins():
    full = np.ones((9, 11, 7), np.uint8)
    out = L.compose_templates([[full, full, full, full]], [np.stack([np.eye(4)] * 4)], (9, 11, 7))
    assert torch.equal(out, torch.full_like(out, 3))


def test_compose_sixty_four_templates_and_sixty_five_refused():
    shape = (9, 11, 7)
    r = np.random.RandomState(33)
    ts = [LR.blob_template((4, 5, 3), 300 + k) for k in range(65)]
    ms = np.stack([LR.random_affine(r, L.affine_matrix) for _ in range(65)])
    out = L.compose_templates([ts[:64]], [ms[:64]], shape)
    lab, near = LR.compose(ts[:64], ms[:64], shape)
    check_outside("compose 64 templates", host(out[0, 0]), lab, near)
    assert lab.max() > 32
    with pytest.raises(_lib.AmxEnvelopeError, match="64"):
        L.compose_templates([ts], [ms], shape)
    # the entry itself refuses 65 as well, before anything is launched
    tab, ens, buf = L._tables([ts[:64]], dict(n_templates=[64], affine=[ms[:64]]), shape)
    ens.host["count"] = 65
    dbuf, dst = cu(buf), torch.zeros((1, 1) + shape, dtype=torch.uint8, device=dev())
    rc = _lib.load().amx_labels_compose(_lib.ptr(dbuf), dbuf.numel(), *tab.device(dev()).args, 64, *ens.device(dev()).args, _lib.ptr(dst), 1, *shape,
                                        _lib.stream(dev()))
    assert rc == _lib.AMX_ERR_INVALID and not dst.any()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=IDS[:2])
def test_compose_half_integer_translations_match_everywhere(shape):
    """x = o + k + 0.5 is exact in float64: floor(x + 0.5) has one answer, so nothing is left out."""
    ts = template_set(shape, 5, 400)
    ms = np.stack([np.eye(4)] * 5)
    ms[:, :3, 3] = [[0.5, 1.5, -2.5], [-0.5, 3.5, 0.5], [2.5, -4.5, 1.5], [0.5, 0.5, 0.5], [-3.5, 2.5, -0.5]]
    ms[3, 0, 0] = -1.0      # and a reflection
    out = L.compose_templates([ts], [ms], shape)
    lab, near = LR.compose(ts, ms, shape)
    assert near.all(), "every coordinate is a half-integer"
    assert np.array_equal(host(out[0, 0]), lab)


# ---- median --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def median_case(shape):
    r = np.random.RandomState(41)
    x = np.stack([r.randint(0, 256, shape).astype(np.uint8), LR.blob_labels(shape, 40, 42), LR.blob_mask(shape, 43),
                  (r.uniform(size=shape) > 0.5).astype(np.uint8)])
    return x, np.stack([LR.median3(v) for v in x])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_median_is_exact(shape):
    """Random bytes over 0 .. 255, blob labels, a blob mask and a random 0 / 1 mask, one launch."""
    x, ref = median_case(shape)
    assert x[0].min() == 0 and x[0].max() == 255
    d = cu(x)[:, None]
    out = L.median3(d)
    assert np.array_equal(host(out[:, 0]), ref)
    assert np.array_equal(ref[2], LR.median3_mask(x[2])) and np.array_equal(ref[3], LR.median3_mask(x[3]))
    # a switched-off ensemble passes through the same launch unchanged, the others are filtered as before
    part = L.median3(d, on=[True, False, True, False])
    assert torch.equal(part[1], d[1]) and torch.equal(part[3], d[3]) and torch.equal(part[0], out[0]) and torch.equal(part[2], out[2])


def test_median_of_every_value_pair():
    """Neighbourhoods of 13 a's and 14 b's in both orders for all 256 values: the exact element 13, not a median of medians."""
    v = np.arange(256, dtype=np.uint8)
    x = np.zeros((2, 256, 3, 3, 3), np.uint8)
    flat = x.reshape(2, 256, 27)
    flat[0, :, :13], flat[0, :, 13:] = v[:, None], v[::-1, None]      # 14 of the mirrored value: it is the median
    flat[1, :, :14], flat[1, :, 14:] = v[:, None], v[::-1, None]
    vols = x.reshape(512, 1, 3, 3, 3)
    out = host(L.median3(cu(vols)))[:, 0, 1, 1, 1].reshape(2, 256)
    assert np.array_equal(out[0], v[::-1]) and np.array_equal(out[1], v)


# ---- deformed sphere -----------------------------------------------------------------------------------------------------------

def sphere_inputs(S):
    """Three ensembles with different spheres; displacement stds in the reference's range U(q, 5 q)."""
    q = S / 128
    radius = np.array([round(50 * q), round(70 * q), round(60 * q)])
    centre = np.array([[round(20 * q), -round(31 * q), 0], [0, 0, 0], [-round(32 * q), round(10 * q), round(31 * q)]])
    std = np.array([[5 * q, 5 * q, 5 * q], [q, 3 * q, 5 * q], [2 * q, q, 4 * q]])
    r = np.random.RandomState(50 + S)
    grids = [np.stack([r.standard_normal((3, cn, cn, cn)) * std[b, s] for b in range(3)]).astype(np.float32) for s, cn in enumerate((16, 8, 4))]
    return radius, centre, grids


@functools.lru_cache(maxsize=None)
def sphere_reference(S):
    radius, centre, grids = sphere_inputs(S)
    return [LR.sphere_mask(radius[b], centre[b], [g[b] for g in grids], S) for b in range(3)]


@pytest.mark.parametrize("S", [16, 48, 80])
def test_sphere_mask_against_the_restatement(S):
    radius, centre, grids = sphere_inputs(S)
    d = [cu(g) for g in grids]
    out = L.deformed_sphere_mask(radius, centre, d, S)
    assert out.shape == (3, 1, S, S, S) and out.dtype == torch.uint8
    for b, (ref, near) in enumerate(sphere_reference(S)):
        check_outside(f"sphere {S} ensemble {b}", host(out[b, 0]), ref, near)
        assert 0 < ref.sum() < ref.size
    assert torch.equal(out, L.deformed_sphere_mask(radius, centre, d, S)), "two runs differ"
    part = L.deformed_sphere_mask(radius, centre, d, S, on=[False, True, False])
    assert not part[0].any() and not part[2].any() and torch.equal(part[1], out[1])
    alone = L.deformed_sphere_mask(radius[2:], centre[2:], [g[2:] for g in d], S)
    assert torch.equal(alone[0], out[2]), "an ensemble alone differs from the same ensemble in a batch"


@pytest.mark.parametrize("S", [16, 32, 48])
def test_sphere_mask_against_the_reference_fixture(S):
    g = dict(np.load(GOLD))
    grids = [g[f"sphere/{S}/grid_{j}"] for j in range(3)]
    ref = np.unpackbits(g[f"sphere/{S}/mask"])[:S ** 3].reshape(S, S, S)
    radius, centre = int(g[f"sphere/{S}/radius"]), g[f"sphere/{S}/centre"]
    out = L.deformed_sphere_mask(radius, centre, [cu(x)[None] for x in grids], S)
    _, near = LR.sphere_mask(radius, centre, grids, S)
    check_outside(f"sphere {S} against the reference's bits", host(out[0, 0]), ref, near)


# ---- apply and envelope ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def envelope_case(shape):
    """Three ensembles, ball radius 2, 3 and 4; masks that touch the border, so that the reflection matters."""
    lab = np.stack([LR.blob_labels(shape, 12 + 9 * b, 60 + b) for b in range(3)])
    mask = np.stack([LR.blob_mask(shape, 70 + b) for b in range(3)])
    applied = [LR.apply_mask(lab[b], mask[b]) for b in range(3)]
    return lab, mask, applied, [LR.envelope(applied[b], mask[b], 2 + b) for b in range(3)]


@pytest.mark.parametrize("shape", [(9, 11, 9), (37, 35, 70)], ids=["9x11x9", "37x35x70"])
def test_apply_and_envelope_are_exact(shape):
    lab, mask, applied, enveloped = envelope_case(shape)
    assert all(m[0].any() or m[-1].any() or m[:, 0].any() or m[:, :, 0].any() for m in mask), "no mask touches the border"
    dl, dm = cu(lab)[:, None], cu(mask)[:, None]
    out, mx = L.apply_foreground_mask(dl, dm)
    assert np.array_equal(host(out[:, 0]), np.stack(applied))
    assert mx.dtype == torch.int32 and host(mx).tolist() == [int(a.max()) for a in applied]
    env = L.envelope(out, dm, [2, 3, 4], mx)
    for b in range(3):
        assert np.array_equal(host(env[b, 0]), enveloped[b]), f"ball {2 + b}"
        assert enveloped[b].max() == applied[b].max() + 1
    # every radius on every mask
    for r in (2, 3, 4):
        got = host(L.envelope(out, dm, r, mx))[:, 0]
        assert np.array_equal(got, np.stack([LR.envelope(applied[b], mask[b], r) for b in range(3)])), f"ball {r}"
    # switched-off ensembles pass through both launches unchanged; their maximum is still their own
    part, pmx = L.apply_foreground_mask(dl, dm, on=[True, False, True])
    assert torch.equal(part[1], dl[1]) and torch.equal(part[0], out[0]) and host(pmx).tolist() == [int(applied[0].max()), int(lab[1].max()), int(applied[2].max())]
    penv = L.envelope(out, dm, [2, 3, 4], mx, on=[False, True, False])
    assert torch.equal(penv[0], out[0]) and torch.equal(penv[2], out[2]) and torch.equal(penv[1], env[1])


def test_envelope_refuses_an_axis_of_eight():
    lab = torch.zeros((1, 1, 9, 8, 9), dtype=torch.uint8, device=dev())
    mx = torch.zeros(1, dtype=torch.int32, device=dev())
    with pytest.raises(_lib.AmxEnvelopeError, match="at least 9"):
        L.envelope(lab, lab.clone(), 2, mx)
    t = L._ensemble_table(dict(mask=[True], envelope=[True], ball=2), 1).device(dev())
    rc = _lib.load().amx_labels_envelope(_lib.ptr(lab), _lib.ptr(lab), _lib.ptr(mx), 1, 9, 8, 9, *t.args, _lib.stream(dev()))
    assert rc == _lib.AMX_ERR_SHAPE
    # labels written in place while other workgroups read the mask: the two must not overlap
    both = torch.ones((1, 1, 9, 9, 9), dtype=torch.uint8, device=dev())
    rc = _lib.load().amx_labels_envelope(_lib.ptr(both), _lib.ptr(both), _lib.ptr(mx), 1, 9, 9, 9, *t.args, _lib.stream(dev()))
    assert rc == _lib.AMX_ERR_INVALID and b"overlap" in _lib.load().amx_last_error() and bool((both == 1).all())
    with pytest.raises(ValueError, match="2, 3 or 4"):
        L.envelope(torch.zeros((1, 1, 9, 9, 9), dtype=torch.uint8, device=dev()), torch.zeros((1, 1, 9, 9, 9), dtype=torch.uint8, device=dev()), 5, mx)


# ---- the chain -------------------------------------------------------------------------------------------------------------------

COUNTS = (5, 3, 7)


@functools.lru_cache(maxsize=None)
def chain_case(S):
    """Batch 3: unconstrained, foreground_masked, foreground_masked_enveloped, with 5, 3 and 7 templates."""
    p = L.draw_params(np.random.RandomState(80 + S), list(COUNTS), S)
    p["mask"][:], p["envelope"][:] = [False, True, True], [False, False, True]
    base = (max(S // 2, 6), max(2 * S // 3, 7), S + 3)
    templates = [[LR.blob_template(tuple(n + (k + b) % 3 for n in base), 500 + 10 * b + k, margin=k % 2) for k in range(n)] for b, n in enumerate(COUNTS)]
    grids = LR.coarse_grids(S, (1.0, 1.0, 1.0), 90 + S, batch=3)
    grids = [g * p["std"][:, s, None, None, None, None].astype(np.float32) for s, g in enumerate(grids)]
    ref = []
    for b in range(3):
        own = [g[b] for g in grids]
        ref.append(dict(compose=LR.compose(templates[b], p["affine"][b], (S, S, S)),
                        sphere=LR.sphere_mask(p["radius"][b], p["centre"][b], own, S) if p["mask"][b] else None,
                        labels=LR.generate(templates[b], p["affine"][b], S, p["mask"][b], p["envelope"][b], p["radius"][b], p["centre"][b], own, p["ball"][b])))
    return p, templates, grids, ref


def one(p, b):
    """Ensemble b of a batch's parameters as a batch of one."""
    return {k: (v if k == "side_length" else v[b:b + 1]) for k, v in p.items()}


@pytest.mark.parametrize("S", [16, 48])
def test_chain_against_the_restatement(S):
    p, templates, grids, ref = chain_case(S)
    d = [cu(g) for g in grids]
    out, names = L.generate_labels(templates, p, grids=d)
    assert names == list(L.IDENTIFIERS) and out.shape == (3, 1, S, S, S) and out.dtype == torch.uint8
    # 1. the chain is its stages: bit for bit the public stage functions in sequence
    composed = L.compose_templates(templates, p["affine"], (S, S, S))
    sphere = L.deformed_sphere_mask(p["radius"], p["centre"], d, S, on=p["mask"])
    mask = L.median3(sphere, on=p["mask"])
    applied, mx = L.apply_foreground_mask(L.median3(composed), mask, on=p["mask"])
    assert torch.equal(L.envelope(applied, mask, p["ball"], mx, on=p["envelope"]), out), "generate_labels differs from its stages in sequence"
    for b, r in enumerate(ref):
        # 2. the two rounding stages under their margins, at most 0.5 % of the voxels left out
        check_outside(f"chain {S} ensemble {b} compose", host(composed[b, 0]), *r["compose"])
        if p["mask"][b]:
            check_outside(f"chain {S} ensemble {b} sphere", host(sphere[b, 0]), *r["sphere"])
        # 3. everything after them has one answer: the numpy stencils on those two results equal the chain EVERYWHERE
        got = host(out[b, 0])
        want = LR.generate(None, None, S, p["mask"][b], p["envelope"][b], None, None, None, p["ball"][b], composed=host(composed[b, 0]), sphere=host(sphere[b, 0]))
        assert np.array_equal(got, want), f"ensemble {b} ({names[b]}): {int((got != want).sum())} voxels differ from the stencils on the checked stage results"
        print(f"chain {S} ensemble {b} ({names[b]}): {int((got != r['labels']).sum())} voxels differ from the restatement run from its own compose and mask")
        assert got.max() <= COUNTS[b] + 1 and r["labels"].max() <= COUNTS[b] + 1
    assert (out[1] == 0).any() and (out[2] == 0).any(), "the masked ensembles have a background"
    again, _ = L.generate_labels(templates, p, grids=d)
    assert torch.equal(out, again), "two runs differ"
    for b in range(3):
        alone, name = L.generate_labels(templates[b:b + 1], one(p, b), grids=[g[b:b + 1] for g in d])
        assert name == [names[b]] and torch.equal(alone[0], out[b]), f"ensemble {b} alone differs from the same ensemble in the batch"
    # the unconstrained ensemble went through the mask and envelope launches of its batch unchanged: without them it is the same
    off = dict(p, mask=np.zeros(3, bool), envelope=np.zeros(3, bool))
    plain, plain_names = L.generate_labels(templates, off)
    assert plain_names == ["unconstrained"] * 3 and torch.equal(plain[0], out[0]) and not torch.equal(plain[1], out[1])
    # the masked ensemble went through the envelope launch unchanged
    no_env, _ = L.generate_labels(templates, dict(p, envelope=np.zeros(3, bool)), grids=d)
    assert torch.equal(no_env[1], out[1]) and torch.equal(no_env[0], out[0]) and not torch.equal(no_env[2], out[2])


def test_chain_draws_its_noise_per_ensemble():
    """Without ``grids`` the noise comes from each ensemble's own seeded generator: a batch equals its ensembles generated alone."""
    p, templates, _, _ = chain_case(16)
    out, _ = L.generate_labels(templates, p)
    again, _ = L.generate_labels(templates, p)
    assert torch.equal(out, again)
    for b in (1, 2):
        assert torch.equal(L.generate_labels(templates[b:b + 1], one(p, b))[0][0], out[b])
    g = L.draw_noise(p, dev())
    assert [tuple(x.shape) for x in g] == [(3, 3, 16, 16, 16), (3, 3, 8, 8, 8), (3, 3, 4, 4, 4)]
    assert torch.equal(L.generate_labels(templates, p, grids=g)[0], out)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals():
    u8 = torch.zeros((1, 1, 16, 16, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no host path"):
        L.median3(u8)
    with pytest.raises(RuntimeError, match="no host path"):
        L.apply_foreground_mask(u8, u8)
    with pytest.raises(RuntimeError, match="no host path"):
        L.compose_templates([[np.ones((2, 2, 2), np.uint8)]], [np.eye(4)[None]], (9, 9, 9), device="cpu")
    with pytest.raises(RuntimeError, match="no host path"):
        L.deformed_sphere_mask(3, [0, 0, 0], [torch.zeros((1, 3, n, n, n)) for n in (16, 8, 4)], 16)
    d = u8.to(dev())
    with pytest.raises(TypeError, match="uint8"):
        L.median3(d.float())
    with pytest.raises(TypeError, match="uint8"):
        L.apply_foreground_mask(d, d.float())
    with pytest.raises(ValueError, match=r"\[B, 1, D, H, W\]"):
        L.median3(d[0])
    with pytest.raises(TypeError, match="int32"):
        L.envelope(d, d, 2, torch.zeros(1, device=dev()))
    grids = lambda B=1, dt=torch.float32: [torch.zeros((B, 3, n, n, n), dtype=dt, device=dev()) for n in (16, 8, 4)]      # noqa: E731
    with pytest.raises(TypeError, match="float32"):
        L.deformed_sphere_mask(3, [0, 0, 0], grids(dt=torch.float64), 16)
    for S in (24, 8, 272):
        with pytest.raises(_lib.AmxEnvelopeError, match="16"):
            L.deformed_sphere_mask(3, [0, 0, 0], grids(), S)
    with pytest.raises(ValueError, match="grids"):
        L.deformed_sphere_mask(3, [0, 0, 0], grids()[:2] + [torch.zeros((1, 3, 5, 5, 5), device=dev())], 16)
    t = L._ensemble_table(dict(mask=[True], radius=3, centre=[0, 0, 0]), 1).device(dev())
    import ctypes
    gp = (ctypes.c_void_p * 3)(*[g.data_ptr() for g in grids()])
    for S in (24, 8, 272):
        assert _lib.load().amx_labels_sphere_mask(gp, _lib.ptr(d), 1, S, *t.args, _lib.stream(dev())) == _lib.AMX_ERR_SHAPE
    # a non-cube, through the chain
    p = L.draw_params(np.random.RandomState(1), [2], 16)
    p["mask"][:] = True
    tpl = [[LR.blob_template((5, 6, 7), 1), LR.blob_template((5, 6, 7), 2)]]
    with pytest.raises(_lib.AmxEnvelopeError, match="16"):
        L.generate_labels(tpl, dict(p, side_length=24))
    with pytest.raises(_lib.AmxEnvelopeError, match="cube"):
        L._cube((16, 16, 32))
    with pytest.raises(ValueError, match="all zero"):
        L.generate_labels([[tpl[0][0], np.zeros((4, 4, 4), np.uint8)]], p)
    with pytest.raises(ValueError, match="templates are drawn"):
        L.generate_labels([tpl[0][:1]], p)
    with pytest.raises(_lib.AmxEnvelopeError, match="64"):
        L.compose_templates([[np.ones((2, 2, 2), np.uint8)] * 65], [np.stack([np.eye(4)] * 65)], (9, 9, 9))
    with pytest.raises(ValueError, match="finite"):
        L.compose_templates([[np.ones((2, 2, 2), np.uint8)]], [np.full((1, 4, 4), np.nan)], (9, 9, 9))
    with pytest.raises(ValueError, match="envelope needs"):
        L._ensemble_table(dict(mask=[False], envelope=[True]), 1)


# ---- command line ------------------------------------------------------------------------------------------------------------------

NAME = re.compile(r"^(unconstrained|foreground_masked|foreground_masked_enveloped)_shapes(\d+)_([A-Z0-9]{7})\.nii\.gz$")


def test_command_line(tmp_path):
    """Templates in the reference's directory layout, one of them empty; three ensembles at 16^3, which step 2's loader reads."""
    from anatomix_amd.datagen.step2_generate_views import load_label_map
    from anatomix_amd.io.nifti import load_nifti, save_nifti
    for i in range(4):
        seg = tmp_path / "templates" / f"s{i:04d}" / "segmentations"
        seg.mkdir(parents=True)
        vol = np.zeros((14, 12, 10), np.uint8) if i == 1 else LR.blob_template((10 + i, 20 - i, 12), 600 + i, margin=1)
        save_nifti(str(seg / "organ.nii.gz"), vol, affine=np.eye(4), dtype=np.uint8)
    argv = ["--n_ensembles", "3", "--min_templates", "2", "--max_templates", "5", "--side_length", "16", "--templatedir", str(tmp_path / "templates"),
            "--batch_size", "2", "--seed", "5", "--max_workers", "3"]
    runs = []
    for name in ("a", "b"):
        S1.main(argv + ["--savedir", str(tmp_path / name)])
        runs.append(sorted(os.listdir(tmp_path / name)))
    assert len(runs[0]) == 3 and runs[0] == runs[1]
    for f in runs[0]:
        m = NAME.match(f)
        assert m and 2 <= int(m.group(2)) <= 4, f
        lab, unique = load_label_map(str(tmp_path / "a" / f))
        assert lab.shape == (16, 16, 16) and lab.dtype == np.uint8 and unique.max() <= int(m.group(2)) + 1
        assert np.array_equal(load_nifti(str(tmp_path / "a" / f))[1], np.eye(4))
        assert np.array_equal(lab, load_label_map(str(tmp_path / "b" / f))[0]), "a second run with the same seed differs"
    # an ensemble does not depend on its batch
    S1.main(argv[:-6] + ["--batch_size", "1", "--seed", "5", "--savedir", str(tmp_path / "c")])
    assert sorted(os.listdir(tmp_path / "c")) == runs[0]
    for f in runs[0]:
        assert np.array_equal(load_label_map(str(tmp_path / "c" / f))[0], load_label_map(str(tmp_path / "a" / f))[0])
