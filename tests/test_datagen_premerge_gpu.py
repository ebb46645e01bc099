"""GPU: the device merge of step 0 (amx_labels_merge_masks of csrc/amx_labels.hip through anatomix_amd.datagen.premerge) against
the numpy restatement tests/_step0_ref.py -- integer sums, so everything must be EQUAL -- and the data generation as a chain at toy
size: step 0, 1, 2 and 3, then a pretraining batch from the containers."""
import functools
import os
from argparse import Namespace
from glob import glob

import numpy as np
import pytest
import torch

import _step0_ref as R
from anatomix_amd import _lib
from anatomix_amd.datagen import premerge
from anatomix_amd.io import H5File
from anatomix_amd.io.nifti import load_nifti, save_nifti

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = {"693": (7, 9, 11), "4096": (16, 16, 16), "20x17x13": (20, 17, 13)}      # 693 and 4420 are no multiples of 16


@functools.lru_cache(maxsize=None)
def case(tag, n):
    """n masks of shape SHAPES[tag] with groups mixed among 0, 1 and 2, several blank files, labels other than 1 (3 and 7), sparse
    enough that a merged voxel stays below 256 -- and the restatement's answer."""
    shape = SHAPES[tag]
    r = np.random.RandomState(1000 * n + len(tag))
    groups = [int(g) for g in r.randint(0, 3, n)]
    if n >= 5:
        groups[:3] = [1, 2, 0]
    vols = []
    for i in range(n):
        v = (r.uniform(size=shape) < 0.08).astype(np.uint8) * np.uint8((1, 3, 7)[i % 3])
        if n >= 5 and (i % 4 == 3 or i == n - 1):
            v[:] = 0                                                    # blank files of every group
        vols.append(v)
    return vols, groups, R.merge_masks(vols, groups)


def check(got, ref):
    for g, r in zip(got[:2], ref[:2]):
        assert g.dtype == np.uint8 and g.shape == r.shape and np.array_equal(g, r)
    assert got[2].dtype == np.uint64 and np.array_equal(got[2], ref[2])


@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_merge_equals_numpy(tag, n):
    vols, groups, ref = case(tag, n)
    if n >= 5:
        assert sum(int(s) == 0 for s in ref[2][:n]) >= 2 and ref[2][n] > 0 and ref[2][n + 1] > 0
        assert ref[2][:n].max() > np.count_nonzero(vols[int(ref[2][:n].argmax())])          # the sums are no popcounts
    check(premerge.merge_masks(vols, groups, DEV), ref)
    check(premerge.merge_masks(iter(vols), groups, DEV), ref)                               # masks arriving one by one


@pytest.mark.parametrize("tag", list(SHAPES))
def test_accumulating_launches(tag, monkeypatch):
    """n = 70 under a byte budget of 24 rows: three launches, the last two accumulating; every batch size gives the same answer."""
    vols, groups, ref = case(tag, 70)
    stride = (vols[0].size + 15) // 16 * 16
    lib = _lib.load()
    calls = []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name != "amx_labels_merge_masks":
                return fn

            def wrapped(*a):
                calls.append((a[1], a[8]))                               # n, accumulate
                return fn(*a)
            return wrapped

    monkeypatch.setattr(_lib, "load", lambda: Spy())
    check(premerge.merge_masks(vols, groups, DEV, byte_budget=24 * stride), ref)
    assert calls == [(24, 0), (24, 1), (22, 1)]
    del calls[:]
    check(premerge.merge_masks(vols, groups, DEV, byte_budget=1), ref)                      # one file per launch
    assert len(calls) == 70 and [c[1] for c in calls] == [0] + [1] * 69


def test_folder_without_ribs_or_vertebrae():
    vols, _, _ = case("693", 5)
    got = premerge.merge_masks(vols, [0] * 5, DEV)
    check(got, R.merge_masks(vols, [0] * 5))
    assert got[2][5] == 0 and got[2][6] == 0 and not got[0].any() and not got[1].any()
    assert [int(s) for s in got[2][:5]] == [int(v.sum()) for v in vols]


def test_more_than_one_workgroup_and_a_tail():
    """65 x 67 x 61: 16603 vectors of 16 voxels (65 workgroups) and a tail of 7."""
    shape = (65, 67, 61)
    r = np.random.RandomState(3)
    vols = [(r.uniform(size=shape) < 0.02).astype(np.uint8) * np.uint8(1 + i) for i in range(4)] + [np.zeros(shape, np.uint8)]
    vols[3][-1, -1, -7:] = 9                                             # the tail voxels, and the last full vector
    vols[1][-1, -1, -23:-7] = 5
    groups = [1, 2, 0, 2, 1]
    check(premerge.merge_masks(vols, groups, DEV), R.merge_masks(vols, groups))


def _overflow_case(total, shape=(7, 9, 11)):
    """Four rib files whose voxel (3, 4, 5) sums to ``total`` (the last voxel too: the tail), vertebrae far below."""
    parts = [100, 100, 50, total - 250]
    vols = []
    for p in parts:
        v = np.zeros(shape, np.uint8)
        v[3, 4, 5] = p
        v[-1, -1, -1] = p
        v[0, 0, 0] = 1
        vols.append(v)
    vert = np.zeros(shape, np.uint8)
    vert[1, 1, 1] = 200
    return vols + [vert], [1, 1, 1, 1, 2]


@pytest.mark.parametrize("budget_rows", [8, 2, 1])
def test_overflow(budget_rows):
    """255 passes, 256 raises naming the folder -- in one launch and across accumulating launches (2 and 1 files per launch)."""
    stride = 704
    vols, groups = _overflow_case(255)
    got = premerge.merge_masks(vols, groups, DEV, byte_budget=budget_rows * stride)
    check(got, R.merge_masks(vols, groups))
    assert got[0][3, 4, 5] == 255 and got[0][-1, -1, -1] == 255 and got[1][1, 1, 1] == 200
    vols, groups = _overflow_case(256)
    with pytest.raises(ValueError, match="s0042/segmentations.*ribs.*above 255"):
        premerge.merge_masks(vols, groups, DEV, byte_budget=budget_rows * stride, name="s0042/segmentations")
    # the other group alone
    with pytest.raises(ValueError, match="vertebrae.*above 255"):
        premerge.merge_masks(vols, [2, 2, 2, 2, 0], DEV, byte_budget=budget_rows * stride)


def test_two_runs_agree_bit_for_bit():
    vols, groups, _ = case("20x17x13", 70)
    a = premerge.merge_masks(vols, groups, DEV, byte_budget=30 * 4432)
    b = premerge.merge_masks(vols, groups, DEV, byte_budget=30 * 4432)
    assert a[2].tobytes() == b[2].tobytes() and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_entry_refuses_outside_its_envelope():
    lib = _lib.load()
    dev = torch.device(DEV)
    masks = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
    merged = torch.zeros((2, 32), dtype=torch.uint8, device=dev)
    sums = torch.zeros(4, dtype=torch.int64, device=dev)
    flags = torch.zeros(2, dtype=torch.int32, device=dev)
    import ctypes

    def call(n=2, voxels=20, stride=32, groups=(1, 2), masks=masks, merged=merged):
        grp = (ctypes.c_int * len(groups))(*groups)
        return lib.amx_labels_merge_masks(_lib.ptr(masks), n, voxels, stride, grp, _lib.ptr(merged), _lib.ptr(sums), _lib.ptr(flags), 0,
                                          _lib.stream(dev))

    assert call() == 0
    assert call(n=0) == _lib.AMX_ERR_SHAPE and call(n=257) == _lib.AMX_ERR_SHAPE
    assert call(voxels=0) == _lib.AMX_ERR_SHAPE and call(voxels=33) == _lib.AMX_ERR_SHAPE and call(stride=24, voxels=20) == _lib.AMX_ERR_SHAPE
    assert call(groups=(1, 3)) == _lib.AMX_ERR_INVALID and call(groups=(-1, 0)) == _lib.AMX_ERR_INVALID
    assert call(merged=masks) == _lib.AMX_ERR_INVALID                                       # overlap
    assert call(masks=masks.reshape(-1)[1:33].reshape(1, 32), n=1, groups=(1,)) == _lib.AMX_ERR_INVALID      # misaligned
    assert "16-byte" in lib.amx_last_error().decode()
    torch.cuda.synchronize()


# ---- the chain at toy size -------------------------------------------------------------------------------------------------------

def test_chain_step0_to_step3_and_a_pretraining_batch(tmp_path, capsys):
    from anatomix_amd.datagen import step0_preprocess_totalsegmentator as S0
    from anatomix_amd.datagen import step1_generate_labels as S1
    from anatomix_amd.datagen import step2_generate_views as S2
    from anatomix_amd.datagen import step3_generate_h5_w_segs as S3
    from anatomix_amd.pretraining.loader import AugmentedTwoViewLoader
    root = tmp_path / "Totalsegmentator_dataset"
    tree = R.make_tree(root, [(24, 24, 24), (24, 24, 24)], seed=11)
    S0.main(["--totalsegmentator_path", str(root), "--device", DEV])
    for sub, (files, affine) in tree.items():
        names, ribs, verts = R.expected_after(files)
        seg = root / sub / "segmentations"
        assert sorted(os.listdir(seg)) == names and not (root / sub / "ct.nii.gz").exists()
        got, aff, _ = load_nifti(seg / "all_ribs.nii.gz")
        assert np.array_equal(got, ribs) and np.allclose(aff, affine)
        assert np.array_equal(load_nifti(seg / "all_vertebrae.nii.gz")[0], verts)
    ens, views, out = tmp_path / "label_ensembles", tmp_path / "synthesized_views", tmp_path / "h5_w_segs"
    S1.main(["--n_ensembles", "3", "--min_templates", "2", "--max_templates", "4", "--side_length", "32", "--templatedir", str(root),
             "--savedir", str(ens), "--batch_size", "3", "--device", DEV])
    S2.main(["--ensembledir", str(ens), "--savedir", str(views), "--batch_size", "3", "--device", DEV])
    S3.main(["--view1_dir", str(views / "view1"), "--view2_dir", str(views / "view2"), "--seg_dir", str(ens), "--out_dir", str(out),
             "--val_count", "1"])
    capsys.readouterr()
    names = sorted(os.path.basename(p) for p in glob(str(ens / "*.nii.gz")))
    assert len(names) == 3
    order = sorted(names, key=lambda s: "view1_" + s)
    for i, name in enumerate(order):
        with H5File(str(out / ("train_data.hdf5" if i < 2 else "val_data.hdf5"))) as f:
            img, seg = f["%06d" % i]["img"][...], f["%06d" % i]["seg"][...]
        assert img.shape == (2, 32, 32, 32) and img.dtype == np.uint8 and seg.dtype == np.uint8
        assert np.array_equal(img[0], load_nifti(views / "view1" / ("view1_" + name))[0])
        assert np.array_equal(img[1], load_nifti(views / "view2" / ("view2_" + name))[0])
        assert np.array_equal(seg, load_nifti(ens / name)[0]) and seg.any() and img.any()
    opt = Namespace(dataroot=str(out), isTrain=True, data_ndims=3, load_mask=False, load_mode="twoview", view_order=True, crop_size=0,
                    resize=False, augment=False, batch_size=2)
    batch = next(iter(AugmentedTwoViewLoader(opt, device=DEV, seed=0)))
    assert batch["A"].is_cuda and batch["A"].shape == (2, 1, 32, 32, 32) and batch["A_seg"].shape == (2, 1, 32, 32, 32)
    assert sorted(batch["meta"]) == ["000000", "000001"] and torch.isfinite(batch["A"]).all() and torch.isfinite(batch["B"]).all()
