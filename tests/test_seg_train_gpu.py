"""GPU: the segmentation finetuning driver (anatomix_amd/segmentation/train_segmentation.py) end to end on a tiny dataset: three
training volumes and one validation volume of 40 x 36 x 44 with three labels, written with ``save_nifti``; the seeded synthetic 6 M
checkpoint; crop 32, batch 2, 2 iterations, 2 epochs.  Checks the files it writes, the log, the learning rate, the first batch it
hands to ``on_batch`` against the restatement of the augmentation chain (tests/_segaug_ref.py, bound (5e-6 + 10 x e32) x max|ref64|
as in tests/test_seg_augment_gpu.py), reproducibility from the seed, that the loss falls without augmentation, and the two refusals."""
import contextlib
import io
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import _segaug_ref as AR

pytestmark = pytest.mark.gpu
SHAPE = (40, 36, 44)
LR = 2e-4


def dev():
    return torch.device("cuda:0")


def _write_pair(root, split, name, shape, seed):
    from anatomix_amd.io.nifti import save_nifti
    img, lab = AR.blob_volume(shape, seed, n_labels=3)
    save_nifti(str(root / f"images{split}" / f"{name}.nii.gz"), (100.0 * img).astype(np.float32))
    save_nifti(str(root / f"labels{split}" / f"{name}.nii.gz"), lab.astype(np.float32))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from oracle import unet_ref as R
    root = tmp_path_factory.mktemp("segtrain")
    for sub in ("imagesTr", "labelsTr", "imagesVal", "labelsVal"):
        (root / sub).mkdir()
    for i, name in enumerate(("case2", "case10", "case1")):
        _write_pair(root, "Tr", name, SHAPE, 40 + i)
    _write_pair(root, "Val", "case7", SHAPE, 50)
    ckpt = str(root / "unet6m.pth")
    torch.save(R.synthetic_state_dict(R.VARIANTS["anatomix"], 0), ckpt)
    return root, ckpt


def _run(dataset, out_dir, seed=3):
    from anatomix_amd.segmentation.train_segmentation import main
    root, ckpt = dataset
    seen = []

    def on_batch(epoch, step, inputs, labels, params):
        seen.append((epoch, step, inputs.detach().cpu().clone(), labels.detach().cpu().clone(), params))

    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        out = main(["--dataset", str(root), "--pretrained_ckpt", ckpt, "--crop_size", "32", "--batch_size", "2", "--n_iters_per_epoch", "2",
                    "--n_epochs", "2", "--val_interval", "1", "--train_amount", "2", "--n_classes", "3", "--exp_name", "tiny", "--seed", str(seed),
                    "--out_dir", str(out_dir), "--lr", str(LR)], on_batch=on_batch)
    return out, seen, text.getvalue()


@pytest.fixture(scope="module")
def run(dataset, tmp_path_factory):
    out_dir = tmp_path_factory.mktemp("runs_a")
    return _run(dataset, out_dir) + (out_dir,)


def test_files_log_and_learning_rate(run):
    from anatomix_amd.segmentation import load_model
    out, seen, text, out_dir = run
    print(text)
    ck = out_dir / "checkpoints" / "tiny"
    for e in (1, 2):
        state = torch.load(str(ck / f"epoch{e:04d}.pth"), map_location="cpu")
        assert set(state) == {"state_dict", "optimizer", "scheduler"}
    assert [os.path.basename(p) for p in out["paths"]["checkpoints"]] == ["epoch0001.pth", "epoch0002.pth"]
    best = sorted(p.name for p in ck.glob("best_dict_epoch*.pth"))
    assert len(best) >= 1 and best == [os.path.basename(p) for p in out["paths"]["best"]]
    fresh = load_model(3, dev(), ckpt_path="scratch")
    fresh.load_state_dict(torch.load(str(ck / best[-1]), map_location="cpu"), strict=True)
    lines = [json.loads(l) for l in open(out_dir / "runs" / "tiny" / "log.jsonl")]
    train, val = [l for l in lines if l["kind"] == "train"], [l for l in lines if l["kind"] == "val"]
    assert len(train) == 4 and len(val) == 2 and len(lines) == 6
    assert [(l["epoch"], l["step"]) for l in train] == [(1, 1), (1, 2), (2, 1), (2, 2)] and [l["epoch"] for l in val] == [1, 2]
    losses = [l["train_loss"] for l in train] + [l["val_loss_mean_dice"] for l in val]
    assert all(math.isfinite(v) for v in losses + out["step_losses"] + out["epoch_losses"]), losses
    assert out["step_losses"] == [l["train_loss"] for l in train] and [v for _, v in out["val_losses"]] == [l["val_loss_mean_dice"] for l in val]
    assert abs(out["epoch_losses"][0] - sum(out["step_losses"][:2]) / 2) <= 1e-12
    assert 0.0 <= val[0]["val_loss_mean_dice"] <= 1.0
    printed = [float(v) for v in re.findall(r"^learning rate: (\S+)$", text, re.M)]
    cosine = [LR * (1 + math.cos(math.pi * e / 2)) / 2 for e in (0, 1)]
    print("printed learning rates", printed, "cosine", cosine)
    assert len(printed) == 2 and all(abs(a - b) <= 1e-7 * LR for a, b in zip(printed, cosine))
    assert "epoch 0002/0002" in text and "1/2, train_loss: " in text and "current epoch: 2 current mean dice: " in text
    assert "Training cache: 4 images 4 segs" in text and "Validation set: 1 images 1 segs" in text


def test_first_batch_against_the_restatement(run):
    from anatomix_amd.io.nifti import load_nifti
    from anatomix_amd.segmentation.augment import make_resident
    _, seen, _, _ = run
    epoch, step, inputs, labels, p = seen[0]
    assert (epoch, step) == (1, 1) and inputs.shape == labels.shape == (2, 1, 32, 32, 32)
    assert inputs.dtype == torch.float32 and labels.dtype == torch.uint8
    noise = torch.randn((2, 1, 32, 32, 32), generator=torch.Generator(dev()).manual_seed(p["noise_seed"]), device=dev()).cpu().numpy()
    print("switches of the first batch:", {k: v.tolist() for k, v in p["on"].items()})
    for b, path in enumerate(p["files"]):
        vol = make_resident(load_nifti(path)[0], dev()).cpu().numpy()
        lab = load_nifti(path.replace("imagesTr", "labelsTr"))[0]
        x64, y, src = AR.chain_sample(vol, lab, p, b, noise[b, 0], np.float64)
        x32, _, _ = AR.chain_sample(vol, lab, p, b, noise[b, 0], np.float32)
        e32 = float(np.abs(x32.astype(np.float64) - x64).max() / np.abs(x64).max())
        err, bound = float(np.abs(inputs[b, 0].double().numpy() - x64).max() / np.abs(x64).max()), 5e-6 + 10 * e32
        print(f"first batch sample {b}: max err / max|ref64| {err:.3e} bound {bound:.3e} (e32 {e32:.2e})")
        assert err <= bound
        sure = AR.half_integer_margin(src) >= 1e-4
        wrong = int((labels[b, 0].numpy()[sure] != y[sure]).sum())
        print(f"first batch sample {b}: {wrong} wrong labels, {100 * (1 - sure.mean()):.3f} % excluded, labels present {np.unique(y).tolist()}")
        assert 1 - sure.mean() <= 0.005 and wrong == 0


def test_two_runs_with_one_seed_hand_over_identical_batches(run, dataset, tmp_path):
    out, seen, _, _ = run
    out2, seen2, _ = _run(dataset, tmp_path)
    assert len(seen) == len(seen2) == 4
    for a, b in zip(seen, seen2):
        assert a[:2] == b[:2] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and a[4]["files"] == b[4]["files"]
    _, seen3, _ = _run(dataset, tmp_path / "other", seed=4)
    assert not all(torch.equal(a[2], b[2]) for a, b in zip(seen, seen3)), "the seed does not reach the batches"


def test_loss_falls_without_augmentation(tmp_path):
    from anatomix_amd.segmentation.train_segmentation import main
    from oracle import unet_ref as R
    root = tmp_path / "data"
    for sub in ("imagesTr", "labelsTr", "imagesVal", "labelsVal"):
        (root / sub).mkdir(parents=True)
    _write_pair(root, "Tr", "case1", (32, 32, 32), 60)
    ckpt = str(tmp_path / "unet6m.pth")
    torch.save(R.synthetic_state_dict(R.VARIANTS["anatomix"], 0), ckpt)
    seen = []
    out = main(["--dataset", str(root), "--pretrained_ckpt", ckpt, "--crop_size", "32", "--batch_size", "1", "--n_iters_per_epoch", "4",
                "--n_epochs", "3", "--val_interval", "10", "--train_amount", "1", "--n_classes", "3", "--lr", "2e-3", "--no_augment",
                "--out_dir", str(tmp_path / "out")], on_batch=lambda e, s, x, y, p: seen.append(x.clone()))
    print("epoch means without augmentation:", [f"{v:.5f}" for v in out["epoch_losses"]])
    assert len(out["step_losses"]) == 12 and all(torch.equal(seen[0], x) for x in seen), "without augmentation the batch is fixed"
    assert out["epoch_losses"][-1] < out["epoch_losses"][0]
    assert out["paths"]["checkpoints"] == [] and out["val_losses"] == []


def test_refusals(dataset, tmp_path):
    from anatomix_amd.segmentation.train_segmentation import main
    root, ckpt = dataset
    (tmp_path / "nothing").mkdir()
    with pytest.raises(AssertionError):
        main(["--dataset", str(tmp_path / "nothing"), "--pretrained_ckpt", ckpt, "--out_dir", str(tmp_path / "o1")])
    seen = []
    with pytest.raises(RuntimeError, match=r"divisible by 2\^num_downs"):
        main(["--dataset", str(root), "--pretrained_ckpt", ckpt, "--crop_size", "24", "--batch_size", "2", "--n_classes", "3",
              "--out_dir", str(tmp_path / "o2")], on_batch=lambda *a: seen.append(a))
    assert seen == [], "refused before the first step"
