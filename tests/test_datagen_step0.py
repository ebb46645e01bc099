"""CPU: the host logic of step 0 of the data generation (anatomix_amd/datagen/step0_preprocess_totalsegmentator.py) with the device
merge replaced by its numpy restatement (tests/_step0_ref.py; tests/test_datagen_premerge_gpu.py holds the kernel to it)."""
import os

import numpy as np
import pytest

import _step0_ref as R
from anatomix_amd import _lib
from anatomix_amd.datagen import premerge
from anatomix_amd.datagen import step0_preprocess_totalsegmentator as S0
from anatomix_amd.io.nifti import load_nifti, save_nifti

SHAPES = [(12, 10, 9), (7, 9, 11)]


@pytest.fixture()
def host_merge(monkeypatch):
    calls = []

    def merge(volumes, groups, device, **kw):
        calls.append((list(groups), device, kw.get("name")))
        return R.merge_masks(volumes, groups, **kw)

    monkeypatch.setattr(premerge, "merge_masks", merge)
    return calls


def _snapshot(root):
    out = {}
    for d, _, names in os.walk(str(root)):
        for n in names:
            p = os.path.join(d, n)
            out[os.path.relpath(p, str(root))] = (open(p, "rb").read(), os.stat(p).st_mtime_ns)
    return out


def test_command_on_a_toy_tree(tmp_path, host_merge, capsys):
    tree = R.make_tree(tmp_path, SHAPES)
    deeper = tmp_path / "s0000" / "extra"
    deeper.mkdir()
    save_nifti(deeper / "ct.nii.gz", np.zeros((2, 2, 2), np.int16))       # two levels down: the reference's glob does not reach it
    S0.main(["--totalsegmentator_path", str(tmp_path), "--max_workers", "3", "--device", "cuda:0"])
    printed = capsys.readouterr().out
    assert "Deleting CT intensity volumes..." in printed and "All ready to synthesize label ensembles." in printed
    assert (deeper / "ct.nii.gz").exists()
    assert len(host_merge) == 2 and all(dev == "cuda:0" for _, dev, _ in host_merge)
    assert sorted(set(host_merge[0][0])) == [0, 1, 2] and str(tmp_path / "s0000") in host_merge[0][2]
    for sub, (files, affine) in tree.items():
        assert not (tmp_path / sub / "ct.nii.gz").exists()
        names, ribs, verts = R.expected_after(files)
        seg = tmp_path / sub / "segmentations"
        assert sorted(os.listdir(seg)) == names
        for fname, want in (("all_ribs.nii.gz", ribs), ("all_vertebrae.nii.gz", verts)):
            data, aff, hdr = load_nifti(seg / fname)
            assert hdr["datatype"] == 2 and np.array_equal(data, want) and want.any()          # uint8
            assert np.allclose(aff, affine) and not np.allclose(affine, np.eye(4))             # the first sorted file's affine
        for fname in ("liver.nii.gz", "aorta.nii.gz"):
            assert np.array_equal(load_nifti(seg / fname)[0], files[fname])
    # a second run changes nothing
    before = _snapshot(tmp_path)
    S0.main(["--totalsegmentator_path", str(tmp_path)])
    assert _snapshot(tmp_path) == before
    assert "Deleting CT" not in capsys.readouterr().out
    assert all(g == 0 for g in host_merge[2][0])                          # all_ribs / all_vertebrae carry neither substring


def test_blank_merges_are_not_written(tmp_path, host_merge):
    seg = tmp_path / "s0001" / "segmentations"
    seg.mkdir(parents=True)
    shape = (6, 5, 4)
    save_nifti(seg / "rib_left_1.nii.gz", np.zeros(shape, np.uint8))
    save_nifti(seg / "vertebrae_T1.nii.gz", R.blob(shape, (3, 2, 2), 2))
    save_nifti(seg / "spleen.nii.gz", R.blob(shape, (2, 2, 2), 1.5, value=3))
    S0.main(["--totalsegmentator_path", str(tmp_path)])
    assert sorted(os.listdir(seg)) == ["all_vertebrae.nii.gz", "spleen.nii.gz"]
    assert np.array_equal(load_nifti(seg / "spleen.nii.gz")[0], R.blob(shape, (2, 2, 2), 1.5, value=3))


def test_documented_narrowing_names_the_file(tmp_path, host_merge):
    shape = (6, 5, 4)

    def folder(tag):
        seg = tmp_path / tag / "s0001" / "segmentations"
        seg.mkdir(parents=True)
        save_nifti(seg / "aorta.nii.gz", R.blob(shape, (3, 2, 2), 2))
        return seg

    seg = folder("fraction")
    save_nifti(seg / "rib_left_1.nii.gz", R.blob(shape, (3, 2, 2), 2).astype(np.float32) * 0.5)
    with pytest.raises(ValueError, match="rib_left_1.nii.gz.*integers"):
        S0.merge_vertebrae_and_ribs(str(tmp_path / "fraction"))
    seg = folder("large")
    save_nifti(seg / "rib_left_1.nii.gz", R.blob(shape, (3, 2, 2), 2).astype(np.int16) * 256)
    with pytest.raises(ValueError, match="rib_left_1.nii.gz.*0 .. 255"):
        S0.merge_vertebrae_and_ribs(str(tmp_path / "large"))
    seg = folder("negative")
    save_nifti(seg / "liver.nii.gz", -R.blob(shape, (3, 2, 2), 2).astype(np.int16))
    with pytest.raises(ValueError, match="liver.nii.gz.*0 .. 255"):
        S0.merge_vertebrae_and_ribs(str(tmp_path / "negative"))
    seg = folder("shape")
    save_nifti(seg / "vertebrae_L1.nii.gz", R.blob((6, 5, 5), (3, 2, 2), 2))
    with pytest.raises(ValueError, match="vertebrae_L1.nii.gz.*shape"):
        S0.merge_vertebrae_and_ribs(str(tmp_path / "shape"))
    seg = folder("overlap")
    for k in range(2):
        save_nifti(seg / f"rib_left_{k}.nii.gz", R.blob(shape, (3, 2, 2), 2, value=128))
    with pytest.raises(ValueError, match="overlap.*above 255"):
        S0.merge_vertebrae_and_ribs(str(tmp_path / "overlap"))
    for tag in ("fraction", "large", "negative", "shape", "overlap"):      # a refused folder is left as it was
        assert "all_ribs.nii.gz" not in os.listdir(tmp_path / tag / "s0001" / "segmentations")


def test_parser_and_groups():
    """The reference's two flags with its defaults (step0_preprocess_totalsegmentator.py:151-163), plus --device."""
    parser = S0.build_parser()
    assert vars(parser.parse_args([])) == {"totalsegmentator_path": "./Totalsegmentator_dataset/", "max_workers": None, "device": "cuda:0"}
    assert premerge.group_of("rib_left_12.nii.gz") == premerge.RIB and premerge.group_of("vertebrae_T9.nii.gz") == premerge.VERTEBRA
    assert premerge.group_of("all_ribs.nii.gz") == premerge.NEITHER and premerge.group_of("all_vertebrae.nii.gz") == premerge.NEITHER
    assert premerge.group_of("liver.nii.gz") == premerge.NEITHER


def test_merge_masks_refuses_before_any_launch():
    """No host path and no launch outside the envelope: every refusal here happens before the library is even loaded."""
    v = np.zeros((4, 4, 4), np.uint8)
    for volumes, groups, device in (([v], [0], "cpu"), ([], [], "cuda:0"), ([v], [3], "cuda:0"), ([v, v], [0], "cuda:0"),
                                    ([v.astype(np.float32)], [1], "cuda:0"), ([v, np.zeros((4, 4, 5), np.uint8)], [1, 2], "cuda:0"),
                                    ([v, v.tolist()], [1, 2], "cuda:0")):
        with pytest.raises(_lib.AmxEnvelopeError):
            premerge.merge_masks(volumes, groups, device)
    with pytest.raises(_lib.AmxEnvelopeError):
        premerge.merge_masks([v], [1], "cuda:0", byte_budget=0)
