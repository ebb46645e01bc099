"""GPU: the pretraining driver end to end (anatomix_amd/pretraining/pretrain_anatomix.py) -- the loop of the reference's
pretraining/trainers/train.py over the HIP step, with gradient clipping inside FusedAdamW, on injected loaders (two in-memory
subjects of 72 x 80 x 72 with 5 labels cropped to 64^3; one validation pair of 64 x 80 x 64) and the synthetic 6 M UNet."""
import json
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch

import _preaug_ref as PR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H5 = os.path.join(HERE, "golden", "two_view_train_data.hdf5")
MAX_NORM = 1e-3
LR = 2e-4


def dev():
    return torch.device("cuda:0")


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


@pytest.fixture(scope="module")
def world(tmp_path_factory, device):
    """The data root (the loader's dataset is replaced, but its constructor opens the files), the synthetic weights as a
    --pretrained_G_only_ckpt file, the in-memory subjects and the validation pair: built once."""
    from oracle import unet_ref as R
    root = tmp_path_factory.mktemp("pretrain")
    shutil.copy(H5, root / "train_data.hdf5")
    shutil.copy(H5, root / "val_data.hdf5")
    kw = R.VARIANTS["anatomix"]
    sd = R.synthetic_state_dict(kw, 3, gain=2 ** 0.5)
    torch.save(sd, root / "synthetic_G.pth")
    img, lab = PR.blob_volume((64, 80, 64), 77, n_labels=5)
    pair = {"A": torch.from_numpy(img[None, None]).float(), "B": torch.from_numpy(0.8 * img[None, None] + 0.05).float(),
            "A_seg": torch.from_numpy(lab[None, None]).float()}
    return Namespace(root=root, kw=kw, sd=sd, dataset=InMemory(2), val=[pair])


def run(world, name, *extra, on_step=None, sample_ids=None):
    from anatomix_amd.pretraining import AugmentedTwoViewLoader
    from anatomix_amd.pretraining.pretrain_anatomix import build_parser, options_from_args, pretrain
    argv = ["--ckpt_dir", str(world.root / "ckpt"), "--name", name, "--dataroot", str(world.root), "--crop_size", "64", "--batch_size", "1",
            "--num_patches", "64", "--n_epochs", "1", "--n_epochs_decay", "1", "--max_iters", "4", "--evaluation_freq", "2",
            "--save_latest_freq", "2", "--print_freq", "1", "--clip_grad", "True", "--max_norm_G", str(MAX_NORM), "--max_norm_F", str(MAX_NORM),
            "--pretrained_G_only_ckpt", str(world.root / "synthetic_G.pth")] + list(extra)
    opt = options_from_args(build_parser().parse_args(argv))
    loader = AugmentedTwoViewLoader(opt, device=dev(), seed=opt.loader_seed)
    loader.dataset = world.dataset
    out = pretrain(opt, train_loader=loader, val_loader=world.val, on_step=on_step, sample_ids=sample_ids)
    out["log"] = [json.loads(l) for l in open(os.path.join(out["save_dir"], "log.jsonl"))]
    return out


def steps_of(out):
    return {float(st["step"]) for o in out["optimizers"] for st in o.state.values()}


@pytest.fixture(scope="module")
def main_run(world):
    return run(world, "main")                                    # --graph auto: every batch has the captured shape


def test_files_log_and_optimizer_state(world, main_run):
    import anatomix_amd
    d = main_run["save_dir"]
    want = {f"{e}_net_{n}.pth" for e in (2, 4, "latest", "best_val") for n in "GF"} | {"best_val_loss.txt", "latest_train_state.pth", "log.jsonl"}
    assert set(os.listdir(d)) == want
    state = torch.load(os.path.join(d, "latest_train_state.pth"))
    assert set(state) == {"optimizers", "schedulers", "scaler", "total_iters", "epoch", "best_evaluation_loss", "last_eval_loss"}
    assert state["scaler"] is None and state["total_iters"] == 4 and len(state["optimizers"]) == 2
    fresh = anatomix_amd.Unet(**world.kw)
    fresh.load_state_dict(torch.load(os.path.join(d, "4_net_G.pth")), strict=True)
    assert float(open(os.path.join(d, "best_val_loss.txt")).read()) == main_run["best_evaluation_loss"]
    train = [l for l in main_run["log"] if l["kind"] == "train"]
    val = [l for l in main_run["log"] if l["kind"] == "val"]
    assert [l["total_iters"] for l in train] == [1, 2, 3, 4] and [l["total_iters"] for l in val] == [2, 4]
    assert all(np.isfinite(l["loss"]) and l["loss"] > 0 and all(np.isfinite(v) for v in l["per_layer"].values()) for l in train)
    assert all(np.isfinite(l["loss"]) and l["n"] == 1 for l in val)
    assert all(set(l) == {"kind", "total_iters", "epoch", "loss", "per_layer", "lr", "grad_norm_G", "grad_norm_F"} for l in train)
    # the logged norm is the one BEFORE clipping
    assert all(l["grad_norm_G"] > MAX_NORM and l["grad_norm_F"] > MAX_NORM for l in train)
    # const_linear with n_epochs 1, n_epochs_decay 1; two subjects per epoch
    assert [l["epoch"] for l in train] == [0, 0, 1, 1]
    assert [l["lr"] for l in train] == [LR * (1.0 - max(0, l["epoch"] - 1) / 2.0) for l in train]
    assert steps_of(main_run) == {4.0} and main_run["total_iters"] == 4 and main_run["start_iters"] == 0


def test_clipping_bites_and_the_graph_agrees_with_the_eager_step(world):
    """Three one-iteration runs with the same seeds, hence the same batch and (the first run's coordinates handed to the others)
    the same patches: clipped eager, unclipped eager, clipped through the graph."""
    ids = []

    def keep(info):
        if info["phase"] == "end":
            ids.extend(t.clone() for t in info["record"]["sample_ids"])

    clipped = run(world, "clip", "--max_iters", "1", "--graph", "off", on_step=keep)
    plain = run(world, "noclip", "--max_iters", "1", "--graph", "off", "--clip_grad", "False", sample_ids=ids)
    graphed = run(world, "graph", "--max_iters", "1", "--graph", "auto", sample_ids=ids)
    assert steps_of(clipped) == steps_of(plain) == steps_of(graphed) == {1.0}        # the capture's warm-up steps were undone
    l_clip, l_plain, l_graph = (r["log"][0]["loss"] for r in (clipped, plain, graphed))
    assert l_clip == l_plain                                  # same weights, batch and patches: the clip only acts in the step
    # the tolerance between an eager and a replayed step of tests/test_pretrain_gpu.py (the replay batches the heads and losses)
    print("first-step loss eager", l_clip, "graph", l_graph)
    assert abs(l_graph - l_clip) < 1e-5 * abs(l_clip)
    g_clip, g_graph = clipped["log"][0]["grad_norm_G"], graphed["log"][0]["grad_norm_G"]
    assert abs(g_graph - g_clip) < 1e-4 * g_clip

    def moved(r):
        sd = torch.load(os.path.join(r["save_dir"], "1_net_G.pth"))
        return sum(float((sd[k].double() - world.sd[k].double()).abs().sum()) for k in world.sd if k.endswith(".weight"))

    m_clip, m_plain, m_graph = moved(clipped), moved(plain), moved(graphed)
    print("first-step movement clipped", m_clip, "unclipped", m_plain, "clipped in the graph", m_graph)
    # Adam's first update is lr g / (|g| + eps): scaling g by coef < 1 shrinks every element's move
    assert 0 < m_clip < m_plain
    # (own bound: warm-up steps that were not undone would triple the movement; the two routes differ by 1e-5 in the gradients, which
    #  Adam's normalised update turns into +-lr only where a gradient is that close to zero)
    assert abs(m_graph - m_clip) < 0.05 * m_clip


def test_resume_continues_without_replaying(world):
    first = run(world, "resume", "--max_iters", "2", "--graph", "off")
    assert first["total_iters"] == 2 and steps_of(first) == {2.0}
    d = first["save_dir"]
    saved = torch.load(os.path.join(d, "latest_train_state.pth"))
    assert saved["total_iters"] == 2
    seen = []

    def look(info):
        if info["phase"] == "start" and not seen:
            want = torch.load(os.path.join(d, "2_net_G.pth"))
            got = info["netG"].state_dict()
            seen.append((info["total_iters"], all(torch.equal(got[k].cpu(), want[k]) for k in want) and set(got) == set(want),
                         [s.last_epoch for s in info["schedulers"]], {float(st["step"]) for o in info["optimizers"] for st in o.state.values()}))

    second = run(world, "resume", "--max_iters", "4", "--graph", "off", "--continue_train", "True", on_step=look)
    assert second["start_iters"] == 2
    total, same, last_epochs, steps = seen[0]
    assert total == 3 and same                                  # iteration 2 is not replayed; the weights are 2_net_G.pth bit for bit
    assert last_epochs == [s["last_epoch"] for s in saved["schedulers"]] and steps == {2.0}
    assert second["total_iters"] == 4 and steps_of(second) == {4.0}
    assert [l["total_iters"] for l in second["log"] if l["kind"] == "train"] == [1, 2, 3, 4]      # the log is appended to


def test_validation_loss(world, main_run):
    from anatomix_amd.pretraining import SupPatchNCELoss
    from anatomix_amd.pretraining.step import validation_loss
    netG, netF = main_run["netG"], main_run["netF"]
    layers = [27, 31, 38, 45, 52, 65]
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw")) for _ in layers]
    A, B, seg = (world.val[0][k].to(dev()) for k in ("A", "B", "A_seg"))
    netG.train(), netF.train()
    one = validation_loss(netG, netF, crits, A, B, seg, layers, num_patches=64)
    assert netG.training and netF.training and all(m.training for m in netF.modules())
    two = validation_loss(netG, netF, crits, A, B, seg, layers, num_patches=64, sample_ids=one["sample_ids"])
    three = validation_loss(netG, netF, crits, A, B, seg, layers, num_patches=64, sample_ids=one["sample_ids"])
    assert np.isfinite(one["loss"]) and one["loss"] > 0 and list(one["per_layer"]) == [str(l) for l in layers]
    assert one["loss"] == two["loss"] == three["loss"] and one["per_layer"] == two["per_layer"]
    assert abs(one["loss"] - sum(one["per_layer"].values()) / 6) < 1e-5 * one["loss"]
    netG.eval()
    validation_loss(netG, netF, crits, A, B, seg, layers, num_patches=64, sample_ids=one["sample_ids"])
    assert not netG.training and netF.training                  # whatever the modes were, they come back
    netG.train()
    big = torch.zeros(1, 1, 72, 80, 72, device=dev())
    with pytest.raises(ValueError, match="multiple"):
        validation_loss(netG, netF, crits, big, big, big, layers, num_patches=64)


def test_scaler_route_clips_after_unscale(world):
    """contrastive_step(scaler=...) with clipping optimizers: the norms are taken after ``unscale_`` -- those of the true gradients,
    not 1024 times them -- and ``scaler.step`` runs the clipping step.  A power-of-two scale leaves the gradients' bits alone, so the
    recorded norms equal those of the unscaled step up to the last bits of the fp32 unscale multiply."""
    import contextlib, copy, io
    import anatomix_amd
    from anatomix_amd.pretraining import FusedAdamW, PatchSampleF, SupPatchNCELoss, contrastive_step
    from oracle import pretrain_inputs as PI
    with contextlib.redirect_stdout(io.StringIO()):
        netG = anatomix_amd.Unet(**world.kw)
        netG.load_state_dict(world.sd)
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
        netF.create_mlp([torch.zeros(1, c, 1, 1, 1, device=dev()) for c in (128, 256, 128, 64, 32, 16)])
    netG.precision = "bf16"
    netG, netF = netG.to(dev()).train(), netF.to(dev()).train()
    netG2, netF2 = copy.deepcopy(netG), copy.deepcopy(netF)
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw")) for _ in PI.NCE_LAYERS]
    A, B, seg = [t.to(dev()) for t in PI.step_inputs(64)]
    okw = dict(lr=LR, weight_decay=1e-5, max_norm=MAX_NORM)
    plain = (FusedAdamW(netG.parameters(), **okw), FusedAdamW(netF.parameters(), **okw))
    scaled = (FusedAdamW(netG2.parameters(), **okw), FusedAdamW(netF2.parameters(), **okw))
    r1 = contrastive_step(netG, netF, crits, A, B, seg, PI.NCE_LAYERS, num_patches=64, optimizers=plain)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)
    r2 = contrastive_step(netG2, netF2, crits, A, B, seg, PI.NCE_LAYERS, num_patches=64, optimizers=scaled, sample_ids=r1["sample_ids"],
                          scaler=scaler)
    assert r1["loss"] == r2["loss"] and r1["grad_norm_G"] > MAX_NORM
    assert abs(r2["grad_norm_G"] - r1["grad_norm_G"]) < 1e-5 * r1["grad_norm_G"]
    assert abs(r2["grad_norm_F"] - r1["grad_norm_F"]) < 1e-5 * r1["grad_norm_F"]
    assert abs(float(scaled[0].total_norm) - r2["grad_norm_G"]) < 1e-6 * r2["grad_norm_G"]
    assert {float(st["step"]) for o in scaled for st in o.state.values()} == {1.0} and scaler.get_scale() == 1024.0
    assert all(p.grad is None for p in netG2.parameters())
