"""CPU: the host side of the pretraining driver (anatomix_amd/pretraining/pretrain_anatomix.py, schedulers.py, checkpoints.py)
against what the reference's launcher, options, schedulers and checkpoint files are (pretraining/scripts/pretrain_anatomix.py,
options/*.py, models/pretraining_networks.py:526-599, models/base_model.py:245-466; recorded in tests/golden/pretrain_cli.json by
tools/make_golden_pretrain_cli.py)."""
import json
import math
import os
from argparse import Namespace
from collections import OrderedDict

import pytest
import torch
import torch.nn as nn

import _segaug_ref as AR
from anatomix_amd.pretraining import checkpoints as CK
from anatomix_amd.pretraining.pretrain_anatomix import (EXTRA_FLAGS, TRAINER_DEFAULTS, build_parser, options_from_args, pretrain)
from anatomix_amd.pretraining.schedulers import POLICIES, get_scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "pretrain_cli.json")))


def test_parser_is_the_launchers_flag_for_flag():
    mine = AR.describe_parser(build_parser())
    n = len(GOLD["flags"])
    assert n == 66
    for a, b in zip(mine["flags"][:n], GOLD["flags"]):
        assert a == b, (a, b)
    assert mine["exclusive_groups"] == GOLD["exclusive_groups"]
    assert [f["dest"] for f in mine["flags"][n:]] == list(EXTRA_FLAGS) == ["precision", "graph", "loader_seed", "out_log"]


def test_trainer_side_defaults_are_the_trainers():
    want = GOLD["trainer_defaults"]
    for k, v in TRAINER_DEFAULTS.items():
        assert want[k] == v, k
    # every option of the trainer's parser is either passed by the launcher or carried as a default here
    assert set(want) == set(TRAINER_DEFAULTS) | set(GOLD["passed"])
    opt = options_from_args(build_parser().parse_args(["--ckpt_dir", "ckpts/x", "--clip_grad", "True", "--gpu_ids", "0", "--continue_train", "false"]))
    for k in want:
        assert hasattr(opt, k), k
    assert opt.checkpoints_dir == "ckpts/x" and not hasattr(opt, "ckpt_dir")
    assert opt.clip_grad is True and opt.continue_train is False and opt.weigh_rarity is False and opt.apply_same_inten_augment is False
    assert opt.gpu_ids == [0] and opt.pretrained_name is None and opt.pretrained_G_only_ckpt is None
    assert (opt.beta1, opt.beta2, opt.eps, opt.stop_epoch, opt.save_by_iter, opt.augment) == (0.9, 0.999, 1e-8, 99999999, False, True)
    assert opt.isTrain is True and opt.precision == "bf16" and opt.graph == "auto"


@pytest.mark.parametrize("argv,word", [(["--netG", "primus"], "primus"), (["--ndims", "2"], "ndims"), (["--gpu_ids", "-1"], "gpu_ids"),
                                       (["--pretrained_name", "other", "--continue_train", "True"], "exclusive")])
def test_refusals_come_before_any_work(argv, word, tmp_path):
    opt = options_from_args(build_parser().parse_args(["--ckpt_dir", str(tmp_path)] + argv))
    with pytest.raises(NotImplementedError, match=word):
        pretrain(opt)
    assert os.listdir(tmp_path) == []


LR, N_EPOCHS, N_DECAY, DECAY_ITERS = 2e-4, 3, 4, 2
CLOSED = {
    "const_linear": lambda e: LR * (1.0 - max(0, e - N_EPOCHS) / float(N_DECAY + 1)),
    "linear": lambda e: LR * (1.0 + (5e-2 - 1.0) * min(e, N_EPOCHS + N_DECAY) / (N_EPOCHS + N_DECAY)),
    "exponential": lambda e: LR * 0.99 ** e,
    "step": lambda e: LR * 0.5 ** (e // DECAY_ITERS),
    # a metric that never improves after the first evaluation: patience 5 -> the 7th step is the 6th bad one and halves the rate
    "plateau": lambda e: LR * (0.5 if e >= 7 else 1.0),
    "cosine": lambda e: LR * (1.0 + math.cos(math.pi * e / N_EPOCHS)) / 2.0,
}


@pytest.mark.parametrize("policy", POLICIES)
def test_eight_epochs_of_every_policy(policy):
    p = nn.Parameter(torch.zeros(3))
    optimizer = torch.optim.AdamW([p], lr=LR)
    opt = Namespace(lr_policy=policy, n_epochs=N_EPOCHS, n_epochs_decay=N_DECAY, lr_decay_iters=DECAY_ITERS, epoch_count=5)
    sched = get_scheduler(optimizer, opt)
    got = []
    for e in range(8):
        got.append(optimizer.param_groups[0]["lr"])
        p.grad = torch.ones(3)
        optimizer.step()
        sched.step(1.0) if policy == "plateau" else sched.step()
    assert got == pytest.approx([CLOSED[policy](e) for e in range(8)], rel=1e-9, abs=1e-18), policy


def test_unknown_policy_raises():
    assert set(CLOSED) == set(POLICIES)
    with pytest.raises(NotImplementedError, match="warmup"):
        get_scheduler(torch.optim.AdamW([nn.Parameter(torch.zeros(1))]), Namespace(lr_policy="warmup", n_epochs=1, n_epochs_decay=1))


class Tiny(nn.Module):
    """A network with the reference's layout: a ``model`` Sequential whose last parametrised child is the output head."""

    def __init__(self, out=2, mid=4):
        super().__init__()
        self.model = nn.Sequential(nn.Conv3d(1, mid, 3), nn.BatchNorm3d(mid), nn.ReLU(), nn.Conv3d(mid, out, 3))


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_network_files_round_trip(tmp_path):
    torch.manual_seed(0)
    g, f = Tiny(), nn.Sequential(nn.Linear(4, 4, bias=False), nn.BatchNorm1d(4))
    CK.save_networks(str(tmp_path), 4, {"G": g, "F": f})
    CK.save_networks(str(tmp_path), "latest", {"G": g})
    assert sorted(os.listdir(tmp_path)) == ["4_net_F.pth", "4_net_G.pth", "latest_net_G.pth"]
    raw = torch.load(tmp_path / "4_net_G.pth")
    assert list(raw) == list(g.state_dict()) and all(v.device.type == "cpu" for v in raw.values())      # plain keys
    g2, f2 = Tiny(), nn.Sequential(nn.Linear(4, 4, bias=False), nn.BatchNorm1d(4))
    CK.load_networks(str(tmp_path), 4, {"G": g2, "F": f2})
    assert _same(g.state_dict(), g2.state_dict()) and _same(f.state_dict(), f2.state_dict())
    # a file written after torch.compile + DataParallel: both prefixes go
    wrapped = OrderedDict(("_orig_mod.module." + k, v) for k, v in g.state_dict().items())
    torch.save(wrapped, tmp_path / "7_net_G.pth")
    g3 = Tiny()
    CK.load_networks(str(tmp_path), 7, {"G": g3})
    assert _same(g.state_dict(), g3.state_dict())
    g4 = Tiny()
    CK.load_G_only(str(tmp_path / "7_net_G.pth"), g4)
    assert _same(g.state_dict(), g4.state_dict())
    with pytest.raises(RuntimeError):
        CK.load_G_only(str(tmp_path / "4_net_F.pth"), Tiny())              # strict
    with pytest.raises(ValueError):
        CK.load_networks(str(tmp_path), 4, {})


def test_partial_load_allows_the_output_head_only(tmp_path):
    torch.manual_seed(1)
    src = Tiny(out=2)
    CK.save_networks(str(tmp_path), "latest", {"G": src})
    # another number of output channels: the head keeps its fresh initialisation, the rest is loaded
    dst = Tiny(out=5)
    head0 = dst.model[3].weight.detach().clone()
    left = CK.load_network(str(tmp_path / "latest_net_G.pth"), dst)
    assert left == ["model.3.bias", "model.3.weight"]
    assert torch.equal(dst.model[3].weight, head0)
    assert torch.equal(dst.model[0].weight, src.model[0].weight) and torch.equal(dst.model[1].running_var, src.model[1].running_var)
    assert CK.output_head_keys(dst, dst.state_dict().keys()) == {"model.3.weight", "model.3.bias"}
    # anything else that does not fit is refused, and nothing is loaded
    other = Tiny(out=2, mid=6)
    w0 = other.model[0].weight.detach().clone()
    with pytest.raises(RuntimeError, match="Refusing to partially load") as e:
        CK.load_network(str(tmp_path / "latest_net_G.pth"), other)
    assert "model.0.weight" in str(e.value) and torch.equal(other.model[0].weight, w0)


def test_training_state_round_trips(tmp_path):
    torch.manual_seed(2)
    opt = Namespace(lr_policy="const_linear", n_epochs=1, n_epochs_decay=2)

    def make():
        nets = [Tiny(), nn.Linear(3, 3)]
        optimizers = [torch.optim.AdamW(n.parameters(), lr=1e-3) for n in nets]
        return nets, optimizers, [get_scheduler(o, opt) for o in optimizers]

    nets, optimizers, schedulers = make()
    for _ in range(3):
        for n, o, s in zip(nets, optimizers, schedulers):
            for p in n.parameters():
                p.grad = torch.randn_like(p)
            o.step()
            s.step()
    extras = {"total_iters": 6, "epoch": 2, "best_evaluation_loss": 1.25, "last_eval_loss": 1.5}
    CK.save_training_state(str(tmp_path), optimizers, schedulers, None, extras)
    state = torch.load(tmp_path / "latest_train_state.pth")
    assert set(state) == {"optimizers", "schedulers", "scaler", "total_iters", "epoch", "best_evaluation_loss", "last_eval_loss"}
    assert state["scaler"] is None and len(state["optimizers"]) == len(state["schedulers"]) == 2
    assert CK.peek_training_state(str(tmp_path))["total_iters"] == 6
    nets2, optimizers2, schedulers2 = make()
    got = CK.load_training_state(str(tmp_path), optimizers2, schedulers2)
    assert got == extras
    for o, o2, s, s2 in zip(optimizers, optimizers2, schedulers, schedulers2):
        assert s2.last_epoch == s.last_epoch == 3 and o2.param_groups[0]["lr"] == o.param_groups[0]["lr"]
        for st, st2 in zip(o.state_dict()["state"].values(), o2.state_dict()["state"].values()):
            assert all(torch.equal(torch.as_tensor(st[k]), torch.as_tensor(st2[k])) for k in st)
    assert CK.load_training_state(str(tmp_path / "nothing"), optimizers2, schedulers2) is None
    assert CK.read_best_val(str(tmp_path)) is None
    CK.write_best_val(str(tmp_path), 0.4375)
    assert CK.read_best_val(str(tmp_path)) == 0.4375
