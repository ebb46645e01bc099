"""CPU: step 1 of the synthetic data generation (anatomix_amd.datagen.labels).  The numpy restatement tests/_labels_ref.py, which the
GPU tests (tests/test_datagen_labels_gpu.py) compare the kernels with, is pinned here: ``compose`` and ``sphere_mask`` to the
reference's recorded outputs (tests/golden/datagen_labels_golden.npz, made by tools/make_golden_labels.py), ``affine_sample``, the
median and the morphology to the scipy calls they restate (skimage is not available).  Also
``affine_matrix`` against the fixture's matrices, the seeded parameter draws, the pad parity, the parser, the file-name pattern and
the record layout."""
import functools
import os
import re

import numpy as np
import pytest

import _labels_ref as LR
from anatomix_amd.datagen import labels as L
from anatomix_amd.datagen import step1_generate_labels as S1

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datagen_labels_golden.npz")


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD))


def affine_cases():
    g = gold()
    return [{k: g[f"affine/{i}/{k}"] for k in ("template", "matrix", "output", "scale", "rotation", "translation", "shear", "reflection")}
            for i in range(int(g["affine/count"]))]


def sphere_case(S):
    g = gold()
    return dict(radius=int(g[f"sphere/{S}/radius"]), centre=g[f"sphere/{S}/centre"], grids=[g[f"sphere/{S}/grid_{j}"] for j in range(3)],
                mask=np.unpackbits(g[f"sphere/{S}/mask"])[:S ** 3].reshape(S, S, S))


def test_compose_restatement_against_the_reference_fixture():
    """Voxel for voxel outside the margin; the fixture's cases have no voxel inside it."""
    target = tuple(int(n) for n in gold()["affine/target"])
    pads = set()
    for i, c in enumerate(affine_cases()):
        padded = LR.crop_and_pad(c["template"], target)
        got, near = LR.affine_sample(padded, c["matrix"], target)
        assert near.sum() == 0 and np.array_equal(got, c["output"]), i
        lab, _ = LR.compose([np.ones((1, 1, 1), np.uint8), c["template"]], [np.eye(4), c["matrix"]], target)
        assert np.array_equal(lab > 0, c["output"] > 0), i
        crop = LR.crop(c["template"]).shape
        pads |= {(np.sign(n - t), (max(t - n, 0)) & 1) for n, t in zip(crop, target)}
    # smaller (odd and even pad), equal and larger than the target all occur
    assert pads >= {(-1, 1), (-1, 0), (0, 0), (1, 0)}


@pytest.mark.parametrize("S", [16, 32, 48])
def test_sphere_restatement_against_the_reference_fixture(S):
    c = sphere_case(S)
    got, near = LR.sphere_mask(c["radius"], c["centre"], c["grids"], S)
    print(f"S = {S}: {near.mean() * 100:.3f} % of voxels within {LR.MASK_MARGIN} of a rounding boundary, {int((got != c['mask']).sum())} mismatches")
    assert near.mean() <= LR.MAX_EXCLUDED
    assert np.array_equal(got[~near], c["mask"][~near])
    assert 0 < c["mask"].sum() < S ** 3


def test_restatement_against_scipy():
    import scipy.ndimage as ndi      # a missing scipy is a failure: this is the only pin of the median and the morphology
    r = np.random.RandomState(5)
    for shape in ((9, 11, 7), (12, 10, 9)):
        x = r.randint(0, 256, shape).astype(np.uint8)
        assert np.array_equal(LR.median3(x), ndi.median_filter(x, size=3, mode="nearest"))
        m = (r.uniform(size=shape) > 0.5).astype(np.uint8)
        assert np.array_equal(LR.median3_mask(m), ndi.median_filter(m, size=3, mode="nearest"))
        assert np.array_equal(LR.median3_mask(m), LR.median3(m))
    m = LR.blob_mask((12, 10, 9), 6)
    for rad, count in ((2, 33), (3, 123), (4, 257)):
        assert LR.ball(rad).sum() == count
        assert np.array_equal(LR.dilate(m, rad), ndi.grey_dilation(m, footprint=LR.ball(rad), mode="reflect") > 0)
        assert np.array_equal(LR.erode(m, rad), ndi.grey_erosion(m, footprint=LR.ball(rad), mode="reflect") > 0)
        assert np.array_equal(LR.erode(m, rad), ~LR.dilate(1 - m, rad))
    vol = LR.blob_template((7, 9, 8), 3)
    for _ in range(6):
        M = LR.random_affine(r, L.affine_matrix)
        got, near = LR.affine_sample(vol, M)
        assert np.array_equal(got[~near], ndi.affine_transform(vol, M, order=0, mode="grid-wrap")[~near])
    for t in ([0.5, 1.5, -2.5], [-0.5, 3.5, 0.5]):
        M = np.eye(4)
        M[:3, 3] = t
        assert np.array_equal(LR.affine_sample(vol, M)[0], ndi.affine_transform(vol, M, order=0, mode="grid-wrap"))


def test_affine_matrix_against_the_fixture():
    for i, c in enumerate(affine_cases()):
        m = L.affine_matrix(c["scale"], c["rotation"], c["translation"], c["shear"], c["reflection"])
        assert m.dtype == np.float64 and np.array_equal(m, c["matrix"]), i
    # scale @ rotation @ shear, Rx @ Ry @ Rz, reflection on the scale
    m = L.affine_matrix([2, 3, 4], [0, 0, 90], [1, 2, 3], [0, 0, 0], [False, True, False])
    assert np.allclose(m, [[0, -2, 0, 1], [-3, 0, 0, 2], [0, 0, 4, 3], [0, 0, 0, 1]], atol=1e-15)
    m = L.affine_matrix([1, 1, 1], [0, 0, 0], [0, 0, 0], [0.1, 0.2, 0.3], [False] * 3)
    assert np.array_equal(m[:3, :3], [[1, 0.1, 0.2], [0, 1, 0.3], [0, 0, 1]])


def replay(rng, spec, S):
    """The documented order of ``draw_params``, written out again."""
    q = S / 128
    out = []
    for n in spec:
        e = {}
        e["n"] = rng.randint(n[0], n[1]) if np.ndim(n) else n
        e["templates"] = [(rng.uniform(0.5, 1.5, 3), rng.uniform(-180, 180, 3), rng.uniform(-5, 5, 3), rng.uniform(-0.5, 0.5, 3), rng.uniform(size=3) < 0.5)
                          for _ in range(e["n"])]
        e["mask"] = rng.uniform() > 0.33333
        e["radius"] = rng.randint(round(48 * q), round(72 * q))
        e["centre"] = rng.randint(-round(32 * q), round(32 * q), size=3)
        e["std"] = rng.uniform(q, 5 * q, 3)
        e["envelope"] = rng.uniform() > 0.5
        e["ball"] = rng.randint(2, 5)
        e["seed"] = rng.randint(0, 2 ** 31 - 1)
        out.append(e)
    return out


def test_draw_params_order_replayed():
    spec = [(3, 6), 4, (2, 3)]
    p = L.draw_params(np.random.RandomState(7), spec, 64)
    want = replay(np.random.RandomState(7), spec, 64)
    assert p["side_length"] == 64
    for b, e in enumerate(want):
        assert p["n_templates"][b] == e["n"] and p["affine"][b].shape == (e["n"], 4, 4)
        for k, (sc, rot, tr, sh, refl) in enumerate(e["templates"]):
            assert np.array_equal(p["scale"][b][k], sc) and np.array_equal(p["rotation"][b][k], rot) and np.array_equal(p["translation"][b][k], tr)
            assert np.array_equal(p["shear"][b][k], sh) and np.array_equal(p["reflection"][b][k], refl)
            assert np.array_equal(p["affine"][b][k], L.affine_matrix(sc, rot, tr, sh, refl))
        assert p["mask"][b] == e["mask"] and p["radius"][b] == e["radius"] and np.array_equal(p["centre"][b], e["centre"])
        assert np.array_equal(p["std"][b], e["std"]) and p["envelope"][b] == (e["envelope"] and e["mask"])
        assert p["ball"][b] == e["ball"] and p["noise_seed"][b] == e["seed"]
    assert L.identifiers(p) == [L.IDENTIFIERS[int(e["mask"]) + int(e["mask"] and e["envelope"])] for e in want]


def test_draw_params_switched_off_draws_consume_their_numbers():
    """Ensembles with every combination of switches occur among 40, and what follows an ensemble never depends on its switches: the
    stream after the batch is where the replay's is."""
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    p = L.draw_params(a, [2] * 40, 128)
    replay(b, [2] * 40, 128)
    assert a.randint(0, 2 ** 31 - 1) == b.randint(0, 2 ** 31 - 1)
    assert set(L.identifiers(p)) == set(L.IDENTIFIERS)
    # an ensemble's draws do not depend on the ensembles before it having their switches on or off: same count of numbers each
    one = L.draw_params(np.random.RandomState(3), [2], 128)
    assert np.array_equal(one["affine"][0], p["affine"][0]) and one["noise_seed"][0] == p["noise_seed"][0]


def test_draw_params_ranges_and_rates():
    p = L.draw_params(np.random.RandomState(11), [(20, 40)] * 600, 128)
    n = p["n_templates"]
    assert n.min() == 20 and n.max() == 39                               # max exclusive
    sc, rot = np.concatenate(p["scale"]), np.concatenate(p["rotation"])
    tr, sh, refl = np.concatenate(p["translation"]), np.concatenate(p["shear"]), np.concatenate(p["reflection"])
    assert 0.5 <= sc.min() < 0.51 and 1.49 < sc.max() <= 1.5 and -180 <= rot.min() < -179 and 179 < rot.max() <= 180
    assert -5 <= tr.min() < -4.99 and 4.99 < tr.max() <= 5 and -0.5 <= sh.min() < -0.49 and 0.49 < sh.max() <= 0.5
    assert abs(refl.mean() - 0.5) < 0.01
    # 600 draws: three standard deviations of a rate r are 3 sqrt(r (1 - r) / 600) <= 0.062
    assert abs(p["mask"].mean() - 2 / 3) < 0.062 and abs(p["envelope"][p["mask"]].mean() - 0.5) < 0.075
    assert not p["envelope"][~p["mask"]].any()
    assert p["radius"].min() == 48 and p["radius"].max() == 71 and p["centre"].min() == -32 and p["centre"].max() == 31
    assert 1 <= p["std"].min() < 1.05 and 4.95 < p["std"].max() <= 5 and set(p["ball"]) == {2, 3, 4}
    small = L.draw_params(np.random.RandomState(1), [3] * 200, 48)      # q = 0.375: round(18), round(27), round(12)
    assert small["radius"].min() == 18 and small["radius"].max() == 26 and small["centre"].min() == -12 and small["centre"].max() == 11
    assert 0.375 <= small["std"].min() and small["std"].max() <= 1.875
    with pytest.raises(ValueError):
        L.draw_params(np.random.RandomState(1), [(2, 2)], 128)           # randint(2, 2): max is exclusive


def test_max_templates_is_exclusive():
    p = L.draw_params(np.random.RandomState(2), [(5, 6)] * 50, 128)
    assert set(p["n_templates"]) == {5}


def test_concat_params():
    parts = [L.draw_params(np.random.RandomState([9, i]), [(2, 5)], 32) for i in range(3)]
    whole = L.concat_params(parts)
    assert whole["side_length"] == 32 and len(whole["affine"]) == 3 and whole["mask"].shape == (3,) and whole["centre"].shape == (3, 3)
    for i, q in enumerate(parts):
        assert np.array_equal(whole["affine"][i], q["affine"][0]) and whole["noise_seed"][i] == q["noise_seed"][0]
    with pytest.raises(ValueError):
        L.concat_params([parts[0], L.draw_params(np.random.RandomState(1), [2], 64)])


def test_pad_parity():
    """crop_and_pad_3d_volume: of an odd pad the extra voxel goes in front; nothing is padded where the crop is larger."""
    assert L.pad_before((5, 12, 20), (12, 12, 12)) == ([4, 0, 0], [12, 12, 20])
    assert L.pad_before((6, 11, 1), (12, 12, 12)) == ([3, 1, 6], [12, 12, 12])
    target = tuple(int(n) for n in gold()["affine/target"])
    for c in affine_cases():
        crop = L.crop_template(c["template"])
        assert np.array_equal(crop, LR.crop(c["template"]))
        before, padded = L.pad_before(crop.shape, target)
        ref = LR.crop_and_pad(c["template"], target)
        assert tuple(padded) == ref.shape
        assert np.array_equal(ref[tuple(slice(b, b + n) for b, n in zip(before, crop.shape))], crop) and ref.sum() == crop.sum()
    with pytest.raises(ValueError, match="all zero"):
        L.crop_template(np.zeros((3, 4, 5), np.uint8))


def test_parser_flags_and_defaults_equal_the_reference():
    a = S1.build_parser().parse_args([])
    assert (a.n_ensembles, a.min_templates, a.max_templates, a.side_length) == (120000, 20, 40, 128)
    assert (a.templatedir, a.savedir, a.max_workers) == ("./Totalsegmentator_dataset/", "./label_ensembles/", None)
    assert (a.batch_size, a.seed, a.device) == (8, 0, "cuda:0")
    b = S1.build_parser().parse_args(["--n_ensembles", "3", "--min_templates", "2", "--max_templates", "5", "--side_length", "16", "--templatedir", "t",
                                      "--savedir", "s", "--max_workers", "4", "--batch_size", "2", "--seed", "11", "--device", "cuda:1"])
    assert (b.n_ensembles, b.min_templates, b.max_templates, b.side_length, b.templatedir, b.savedir) == (3, 2, 5, 16, "t", "s")
    assert (b.max_workers, b.batch_size, b.seed, b.device) == (4, 2, 11, "cuda:1")


NAME = re.compile(r"^(unconstrained|foreground_masked|foreground_masked_enveloped)_shapes(\d+)_([A-Z0-9]{7})\.nii\.gz$")


def test_file_name_pattern():
    rng = np.random.RandomState(4)
    seen = set()
    for identifier in L.IDENTIFIERS:
        name = S1.file_name(identifier, 23, S1.draw_suffix(rng))
        m = NAME.match(name)
        assert m and m.group(1) == identifier and m.group(2) == "23", name
        seen.add(m.group(3))
    assert len(seen) == 3
    assert S1.draw_suffix(np.random.RandomState(4)) == S1.draw_suffix(np.random.RandomState(4))
    chars = set("".join(S1.draw_suffix(rng) for _ in range(200)))
    assert chars == set(S1.ALPHABET) and len(S1.ALPHABET) == 36


def test_template_files_follow_the_reference_layout(tmp_path):
    for rel in ("s0001/segmentations/a.nii.gz", "s0002/segmentations/b.nii.gz", "s0002/other/c.nii.gz", "d.nii.gz"):
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_bytes(b"")
    got = [os.path.relpath(p, tmp_path) for p in S1.template_files(str(tmp_path))]
    assert got == ["s0001/segmentations/a.nii.gz", "s0002/segmentations/b.nii.gz"]


def test_record_layout():
    """The numpy records against the C structs of include/anatomix_amd.h, field by field."""
    assert L.TEMPLATE_DTYPE.itemsize == 144 and L.ENSEMBLE_DTYPE.itemsize == 32
    assert [L.TEMPLATE_DTYPE.fields[k][1] for k in ("offset", "crop", "before", "padded", "reserved", "affine")] == [0, 8, 20, 32, 44, 48]
    assert [L.ENSEMBLE_DTYPE.fields[k][1] for k in ("flags", "first", "count", "radius", "shift", "ball")] == [0, 4, 8, 12, 16, 28]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "anatomix_amd.h")).read()
    for struct, dtype in (("amx_labels_template", L.TEMPLATE_DTYPE), ("amx_labels_ensemble", L.ENSEMBLE_DTYPE)):
        body = hdr.split(f"typedef struct {struct} {{", 1)[1].split("}", 1)[0]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip().split("[")[0] for decl in body.split(";") if decl.strip() for n in decl.strip().split(" ", 1)[1].split(",")]
        assert names == list(dtype.names), (names, dtype.names)


def test_chain_restatement_is_bounded_by_the_template_count():
    """labels <= n + 1: n - 1 from the templates, + 1 from the mask, + 1 from the envelope."""
    S, n = 16, 5
    r = np.random.RandomState(8)
    ts = [LR.blob_template((9, 12, 7), 40 + k) for k in range(n)]
    ms = [LR.random_affine(r, L.affine_matrix) for _ in range(n)]
    grids = LR.coarse_grids(S, (0.3, 0.4, 0.5), 9)
    lab = LR.generate(ts, ms, S, True, True, 6, [1, -1, 0], grids, 2)
    masked = LR.generate(ts, ms, S, True, False, 6, [1, -1, 0], grids, 2)
    plain = LR.generate(ts, ms, S, False, False, 0, [0, 0, 0], None, 2)
    assert plain.max() <= n - 1 and masked.max() <= n and lab.max() == masked.max() + 1 <= n + 1
    # the stages in sequence, from given results of the two rounding stages
    composed, sphere = LR.compose(ts, ms, (S, S, S))[0], LR.sphere_mask(6, [1, -1, 0], grids, S)[0]
    assert np.array_equal(LR.generate(None, None, S, True, True, None, None, None, 2, composed=composed, sphere=sphere), lab)
    m = LR.median3_mask(sphere)
    assert np.array_equal(lab, LR.envelope(LR.apply_mask(LR.median3(composed), m), m, 2))


def test_template_draw_skips_empty_files_and_ends_when_all_are_empty(tmp_path):
    from anatomix_amd.io.nifti import save_nifti
    files = []
    for i in range(3):
        files.append(str(tmp_path / f"t{i}.nii.gz"))
        save_nifti(files[-1], np.zeros((4, 5, 6), np.uint8) if i != 1 else LR.blob_template((4, 5, 6), 1), affine=np.eye(4), dtype=np.uint8)
    cache, empty = {}, set()
    got = S1.draw_templates(np.random.RandomState(0), files, 5, cache, empty)
    assert len(got) == 5 and all(g is cache[files[1]] for g in got) and empty <= {files[0], files[2]}
    # the stream does not depend on what is cached: a fresh cache draws the same files
    a, b = np.random.RandomState(3), np.random.RandomState(3)
    S1.draw_templates(a, files, 4, cache, empty), S1.draw_templates(b, files, 4, {}, set())
    assert a.randint(1 << 30) == b.randint(1 << 30)
    with pytest.raises(ValueError, match="every template file is empty"):
        S1.draw_templates(np.random.RandomState(0), [files[0], files[2]], 1, {}, set())
