"""GPU: contrastive pretraining of the ViT -- ``PrimusV2.forward_train_sampled`` (the decoder on sampled rows), ``contrastive_step`` on
a PrimusV2 (sampled route against the dense modules), and ``pretrain`` with ``--netG primus --primus_version v2`` end to end.

The small network is PrimusV2 at 32^3 with width 132, depth 2, 8 output channels and TWO heads: the rotary embedding wants a head width
that is a multiple of 6 (PrimusV2.__init__), which 132 / 6 = 22 is not -- 132 / 2 = 66 is the head width of every PRIMUS_CONFIGS entry."""
import contextlib
import copy
import io
import json
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch

import _decode_rows_ref as R
import _preaug_ref as PR
from anatomix_amd.model.vit3d import PrimusV2

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H5 = os.path.join(HERE, "golden", "two_view_train_data.hdf5")
KW = dict(input_channels=1, num_classes=8, embed_dim=132, patch_embed_size=(8, 8, 8), eva_depth=2, eva_numheads=2, input_shape=(32, 32, 32),
          init_values=0.1, scale_attn_inner=True, qk_norm=True)


def _net(seed=5, **kw):
    torch.manual_seed(seed)
    m = PrimusV2(**{**KW, **kw})
    with torch.no_grad():                       # norm weights / biases and LayerScale away from their initial values
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return m


def _views(seed, n=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 1, 32, 32, 32, generator=g)


def test_forward_train_sampled_against_the_dense_forward_and_gather(device):
    """(g) rows and every parameter's gradient of rows.square().mean() by the ratio rule of tests/test_vit_decode_rows_gpu.py: the error
    of the sampled route against float64 CPU autograd is at most 4 x max(error of the fp32 dense route on the same device, 2^-22)."""
    coords = R.draw_distinct(96, (32, 32, 32), 31)
    x = _views(32)
    ref_net = _net().double()
    out = ref_net(x.double())
    rows = out[:, :, coords[:, 0], coords[:, 1], coords[:, 2]].permute(0, 2, 1)
    rows.square().mean().backward()
    ref = {"rows": rows.detach(), **{k: p.grad for k, p in ref_net.named_parameters()}}

    def run(sampled):
        net = _net().to(device)
        calls = []
        if sampled:
            def sampler(layer, shape):
                calls.append((layer, tuple(shape)))
                return coords.to(device)
            o, (r,), (c,), (dims,) = net.forward_train_sampled(x.to(device), [-1], sampler)
            assert o is None and dims == (32, 32, 32) and torch.equal(c.cpu(), coords) and calls == [(-1, (32, 32, 32))]
        else:
            o = net(x.to(device))
            r = o[:, :, coords[:, 0], coords[:, 1], coords[:, 2]].permute(0, 2, 1)
        r.square().mean().backward()
        return {"rows": r.detach(), **{k: p.grad for k, p in net.named_parameters()}}

    hip, stock = run(True), run(False)
    assert hip.keys() == stock.keys() == ref.keys() and all(v is not None for v in hip.values())
    worst = ("", 0.0)
    for k in ref:
        e_hip, e_stock = R.rel_l2(hip[k], ref[k]), R.rel_l2(stock[k], ref[k])
        ratio = e_hip / max(e_stock, R.FLOOR)
        worst = max(worst, (k, ratio), key=lambda t: t[1])
        print(k, "hip %.2e torch %.2e ratio %.2f" % (e_hip, e_stock, ratio))
        assert e_hip <= R.bar(e_stock), (k, e_hip, e_stock)
    print("worst ratio", worst)


def _step_setup(device, out_norm="none"):
    from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss
    netG = _net(out_norm=out_norm).to(device).train()
    with contextlib.redirect_stdout(io.StringIO()):
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=64, n_mlps=3)
        torch.manual_seed(9)
        netF.create_mlp([torch.zeros(1, 8, 1, 1, 1, device=device)])
    netF = netF.to(device).train()
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
    v = _views(40).to(device)
    seg = torch.from_numpy(PR.blob_volume((32, 32, 32), 41, n_labels=4)[1][None, None]).float().to(device)
    return netG, netF, crits, v[:1], v[1:], seg


def test_contrastive_step_sampled_route_against_the_dense_modules(device):
    """(h) the same network, weights, views and coordinates through the rows route and through ``allow_torch_path = True``: two fp32
    routes, held to the 1e-5 that tests/test_train_step_gpu.py asks of two fp32 routes of the UNet (its head / last-conv bound)."""
    from anatomix_amd.pretraining import contrastive_step
    ids = [R.draw_distinct(64, (32, 32, 32), 43).to(device)]
    recs = {}
    for route in ("rows", "dense"):
        netG, netF, crits, A, B, seg = _step_setup(device)
        netG.allow_torch_path = route == "dense"
        recs[route] = contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=64, sample_ids=ids)
        assert all(p.grad is not None for p in netG.parameters())
    rows, dense = recs["rows"], recs["dense"]
    assert rows["out"] is None and torch.is_tensor(dense["out"]) and dense["out"].shape == (2, 8, 32, 32, 32)
    assert list(rows["per_layer"]) == ["-1"] and np.isfinite(rows["loss"]) and rows["loss"] > 0
    print("loss", rows["loss"], dense["loss"], "gG", rows["grad_norm_G"], dense["grad_norm_G"], "gF", rows["grad_norm_F"], dense["grad_norm_F"])
    for k in ("loss", "grad_norm_G", "grad_norm_F"):
        assert abs(rows[k] - dense[k]) <= 1e-5 * abs(dense[k]), (k, rows[k], dense[k])
    # drawn coordinates: netF's sampler is consumed once, for the volume's shape
    netG, netF, crits, A, B, seg = _step_setup(device)
    drawn = contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=64)
    assert drawn["out"] is None and drawn["sample_ids"][0].shape == (64, 3) and int(drawn["sample_ids"][0].max()) < 32
    with pytest.raises(ValueError, match="outside the feature map"):
        contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=64, sample_ids=[ids[0] + 8])
    for bad in (ids[0][:, :2], ids[0].flatten(), ids[0].float()):
        with pytest.raises(ValueError, match="integer tensor"):
            contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=64, sample_ids=[bad])
    # more views x rows than the kernels take: said by the network, and the step takes the dense modules
    reals = torch.cat((A, B))
    assert netG.sampled_unsupported_reason(reals, 64) is None and "rows" in netG.sampled_unsupported_reason(reals, (1 << 19) + 1)
    from anatomix_amd.pretraining import step as S
    assert S._sampled_route(netG, netF, reals, [-1], 64) == {-1: 0}
    assert S._sampled_route(netG, netF, reals, [-1], 64, [torch.zeros((1 << 19) + 1, 3, dtype=torch.int64)]) is None


def test_validation_outside_the_engine_envelope_runs_the_torch_modules(device):
    """A 16^3 network has 8 tokens; amx_vit_forward wants a multiple of 64.  validation_loss says so once and evaluates on the torch
    composition -- the value of ``use_engine = False`` -- and leaves the switch as it was."""
    from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss
    from anatomix_amd.pretraining.step import validation_loss
    netG = _net(input_shape=(16, 16, 16)).to(device).train()
    with contextlib.redirect_stdout(io.StringIO()):
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=64, n_mlps=3)
        netF.create_mlp([torch.zeros(1, 8, 1, 1, 1, device=device)])
    netF = netF.to(device).train()
    crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
    g = torch.Generator().manual_seed(3)
    A, B = torch.randn(2, 1, 1, 16, 16, 16, generator=g).to(device).unbind(0)
    seg = torch.from_numpy(PR.blob_volume((16, 16, 16), 4, n_labels=3)[1][None, None]).float().to(device)
    with pytest.warns(UserWarning, match="torch modules"):
        one = validation_loss(netG, netF, crits, A, B, seg, [-1], num_patches=32)
    assert netG.use_engine and netG.training and np.isfinite(one["loss"])
    netG.use_engine = False
    two = validation_loss(netG, netF, crits, A, B, seg, [-1], num_patches=32, sample_ids=one["sample_ids"])
    assert two["loss"] == one["loss"]


def test_spatial_output_norm_falls_back_to_the_dense_route(device):
    from anatomix_amd.pretraining import FusedAdamW, contrastive_step
    netG, netF, crits, A, B, seg = _step_setup(device, out_norm="instance")
    assert "spatial" in netG.sampled_unsupported_reason(torch.cat((A, B)))
    before = [p.detach().clone() for p in netG.parameters()]
    opts = (FusedAdamW(netG.parameters(), lr=1e-3), FusedAdamW(netF.parameters(), lr=1e-3))
    rec = contrastive_step(netG, netF, crits, A, B, seg, [-1], num_patches=64, optimizers=opts)
    assert torch.is_tensor(rec["out"]) and np.isfinite(rec["loss"])
    assert any(not torch.equal(a, b) for a, b in zip(before, netG.parameters()))


class InMemory:
    dimension = 3

    def __init__(self, n):
        self.items = [PR.blob_volume((40, 36, 40), 500 + i, n_labels=4) for i in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        img, lab = self.items[i]
        seg = torch.from_numpy(lab[None]).float()
        return {"A": torch.from_numpy(img[None]).float(), "B": torch.from_numpy(0.8 * img[None] + 0.05).float(), "A_seg": seg,
                "B_seg": seg.clone(), "A_id": np.asarray([i]), "B_id": np.asarray([i]), "meta": "%06d" % i, "keys": ["A", "B", "A_seg", "B_seg"]}


@pytest.fixture(scope="module")
def world(tmp_path_factory, device):
    """The data root holds the stored two-view file (the loader's constructor opens it); its 12 x 10 x 8 volumes are smaller than the
    crop, so the subjects are in-memory blobs as in tests/test_pretrain_driver_gpu.py, and the validation pair has the network's shape."""
    root = tmp_path_factory.mktemp("primus")
    shutil.copy(H5, root / "train_data.hdf5")
    shutil.copy(H5, root / "val_data.hdf5")
    img, lab = PR.blob_volume((32, 32, 32), 78, n_labels=4)
    pair = {"A": torch.from_numpy(img[None, None]).float(), "B": torch.from_numpy(0.8 * img[None, None] + 0.05).float(),
            "A_seg": torch.from_numpy(lab[None, None]).float()}
    return Namespace(root=root, dataset=InMemory(2), val=[pair])


def _validation_of(world, device, run, iters, ids, netF):
    """``validation_loss`` of a FRESH PrimusV2 holding ``<iters>_net_G.pth`` of a run, with the given heads and coordinates."""
    from anatomix_amd.pretraining.pretrain_anatomix import build_networks
    from anatomix_amd.pretraining.step import validation_loss
    fresh, _, crits = build_networks(copy.copy(run["opt"]), device)
    fresh.load_state_dict(torch.load(os.path.join(run["save_dir"], f"{iters}_net_G.pth")), strict=True)
    A, B, seg = (world.val[0][k].to(device).float() for k in ("A", "B", "A_seg"))
    return validation_loss(fresh, netF, crits, A, B, seg, [-1], num_patches=64, sample_ids=ids)["loss"]


def _run(world, device, name, *extra, on_step=None, sample_ids=None):
    from anatomix_amd.pretraining import AugmentedTwoViewLoader
    from anatomix_amd.pretraining.pretrain_anatomix import build_parser, options_from_args, pretrain
    argv = ["--ckpt_dir", str(world.root / "ckpt"), "--name", name, "--dataroot", str(world.root), "--netG", "primus", "--primus_version", "v2",
            "--primus_config", "S", "--crop_size", "32", "--batch_size", "1", "--num_patches", "64", "--max_iters", "4", "--evaluation_freq", "2",
            "--n_epochs", "1", "--n_epochs_decay", "1", "--print_freq", "1"] + list(extra)
    opt = options_from_args(build_parser(primus_route=True).parse_args(argv))
    loader = AugmentedTwoViewLoader(opt, device=device, seed=opt.loader_seed)
    loader.dataset = world.dataset
    out = pretrain(opt, train_loader=loader, val_loader=world.val, on_step=on_step, sample_ids=sample_ids)
    out["log"] = [json.loads(l) for l in open(os.path.join(out["save_dir"], "log.jsonl"))]
    out["opt"] = opt
    return out


def test_driver_trains_checkpoints_and_resumes(world, device, monkeypatch):
    """(i) four iterations of PrimusV2-S at 32^3, then a resume of a two-iteration run."""
    from anatomix_amd.pretraining import step as S
    from anatomix_amd.pretraining.pretrain_anatomix import build_networks
    seen_val, orig = [], S.validation_loss

    def recording(*a, **k):
        seen_val.append(orig(*a, **k))
        return seen_val[-1]

    monkeypatch.setattr(S, "validation_loss", recording)
    run = _run(world, device, "main")
    monkeypatch.setattr(S, "validation_loss", orig)
    d = run["save_dir"]
    train = [l for l in run["log"] if l["kind"] == "train"]
    val = [l for l in run["log"] if l["kind"] == "val"]
    assert [l["total_iters"] for l in train] == [1, 2, 3, 4] and [l["total_iters"] for l in val] == [2, 4]
    assert all(list(l["per_layer"]) == ["-1"] and np.isfinite(l["per_layer"]["-1"]) and np.isfinite(l["loss"]) and l["loss"] > 0 for l in train)
    assert all(np.isfinite(l["loss"]) and l["n"] == 1 for l in val)
    assert all(l["grad_norm_G"] > 0 and l["grad_norm_F"] > 0 for l in train)
    assert "PrimusV2" in open(os.path.join(d, "netG.txt")).read()
    fresh = build_networks(copy.copy(run["opt"]), torch.device("cpu"))[0]
    assert isinstance(fresh, PrimusV2)
    fresh.load_state_dict(torch.load(os.path.join(d, "4_net_G.pth")), strict=True)
    assert {float(st["step"]) for o in run["optimizers"] for st in o.state.values()} == {4.0}
    # the evaluation at iteration 4 scored the weights of iteration 4 (FusedAdamW steps through raw pointers: an engine that kept the
    # parameters it packed at iteration 2 would score those): the logged loss is that of a fresh network holding 4_net_G.pth, with the
    # run's heads (unchanged since iteration 4) and the coordinates that evaluation drew -- not that of 2_net_G.pth
    assert len(seen_val) == 2 and seen_val[1]["loss"] == val[1]["loss"]
    ids4 = seen_val[1]["sample_ids"]
    now, stale = _validation_of(world, device, run, 4, ids4, run["netF"]), _validation_of(world, device, run, 2, ids4, run["netF"])
    print("validation at 4: logged", val[1]["loss"], "fresh 4_net_G", now, "fresh 2_net_G (stale)", stale)
    assert abs(now - val[1]["loss"]) <= 1e-6 * abs(now)
    assert abs(stale - val[1]["loss"]) > 1e-4 * abs(now)

    first = _run(world, device, "resume", "--max_iters", "2")
    assert first["total_iters"] == 2
    seen = []

    def look(info):
        if info["phase"] == "start" and not seen:
            want = torch.load(os.path.join(first["save_dir"], "2_net_G.pth"))
            got = info["netG"].state_dict()
            seen.append((info["total_iters"], set(got) == set(want) and all(torch.equal(got[k].cpu(), want[k]) for k in want)))

    second = _run(world, device, "resume", "--max_iters", "4", "--continue_train", "True", on_step=look)
    assert second["start_iters"] == 2 and seen[0] == (3, True) and second["total_iters"] == 4
    assert [l["total_iters"] for l in second["log"] if l["kind"] == "train"] == [1, 2, 3, 4]


def test_driver_train_routes_agree_on_the_first_loss(world, device):
    """``--primus_train_route torch`` against ``hip`` (f16 operands in the attention cores and the blocks' linears): the first
    iteration's loss, same seeds and coordinates, within the 1.6e-3 DESIGN 4.9 records between those routes."""
    ids = []

    def keep(info):
        if info["phase"] == "end":
            ids.extend(t.clone() for t in info["record"]["sample_ids"])

    hip = _run(world, device, "route_hip", "--max_iters", "1", on_step=keep)
    tor = _run(world, device, "route_torch", "--max_iters", "1", "--primus_train_route", "torch", sample_ids=ids)
    assert hip["netG"].train_linear == "hip" and tor["netG"].train_attention == "torch"
    l_hip, l_tor = hip["log"][0]["loss"], tor["log"][0]["loss"]
    print("first-iteration loss hip", l_hip, "torch", l_tor)
    assert abs(l_hip - l_tor) <= 1.6e-3 * abs(l_tor)
