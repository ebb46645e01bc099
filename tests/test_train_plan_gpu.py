"""GPU: what choosing the order and the route once, before any launch, repaired -- the ``on_start`` hook of the sampled training
forward (anatomix_amd/model/train.py) and the head route of the contrastive step (anatomix_amd/pretraining/step.py).  Smallest network the
path takes: num_downs=1, ngf=16 at 32^3 (conv ids 0, 3 | 7, 10 | 14, 17, output conv 20)."""
import contextlib
import copy
import io
from argparse import Namespace

import numpy as np
import pytest
import torch

import anatomix_amd
from anatomix_amd.model import train as TR
from anatomix_amd.pretraining import GraphedContrastiveStep, PatchSampleF, SupPatchNCELoss, contrastive_step
from oracle import pretrain_inputs as PI
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu
KW = dict(dimension=3, input_nc=1, output_nc=16, num_downs=1, ngf=16)
LAYERS = [0, 3, 20]                                   # module 0, the second block's conv, the output conv
P = 64


def _net(device):
    with contextlib.redirect_stdout(io.StringIO()):
        net = anatomix_amd.Unet(**KW)
    net.load_state_dict(R.synthetic_state_dict(KW, 3, gain=2 ** 0.5), strict=True)
    net.precision = "bf16"
    return net.to(device).train()


def _step_setup(device, temperatures):
    netG = _net(device)
    torch.manual_seed(7)
    with contextlib.redirect_stdout(io.StringIO()):
        netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=64, n_mlps=3)
        netF.create_mlp([torch.zeros(1, 16, 1, 1, 1, device=device) for _ in LAYERS])
    netF = netF.to(device).train()
    crits = [SupPatchNCELoss(Namespace(nce_T=t, weigh_rarity=False, balance_denominator=False, weighting_mode="raw")) for t in temperatures]
    return netG, netF, crits, [t.to(device) for t in PI.step_inputs(32)]


@pytest.mark.parametrize("layers", [[0, 20], [3, 20]])
def test_on_start_runs_once_and_before_the_first_draw(device, layers):
    """The hook of the sampled forward runs behind the first block's kernels, or right before the first draw when module 0 itself is
    tapped -- once either way."""
    net = _net(device)
    x = R.synthetic_input(11, 1, (32, 32, 32)).to(device)
    events = []
    g = torch.Generator().manual_seed(1)

    def sampler(i, shape):
        events.append(("tap", i))
        return torch.stack([torch.randint(0, s, (P,), generator=g) for s in shape], dim=1).to(device)

    out, rows, coords, dims = TR.forward_train_sampled(net, x, layers, sampler, on_start=lambda: events.append("start"))
    assert events == ["start"] + [("tap", l) for l in layers]
    assert [tuple(r.shape) for r in rows] == [(1, P, 16)] * 2 and dims == [(32, 32, 32)] * 2
    assert all(torch.isfinite(r).all() for r in rows) and torch.isfinite(out).all()


def test_graphed_step_with_a_sampled_tap_at_module_0(device):
    """A sampled tap at module 0 under capture: the up-front coordinate draw precedes the tap (``forward_train_sampled``'s on_start
    rule).  Before the training function took the hook as an argument it ran only behind the first block, so the cached-shapes sampler
    of the captured step was asked for module 0 before anything was drawn and raised KeyError."""
    netG, netF, crits, (A, B, seg) = _step_setup(device, [PI.NCE_T] * 3)
    step = GraphedContrastiveStep(netG, netF, crits, LAYERS, None, num_patches=P, warmup=2)
    recs, ids0 = [], []
    for _ in range(3):
        recs.append(step(A, B, seg))
        ids0.append(recs[-1]["sample_ids"][0].clone())
    assert step.graph is not None
    assert all(np.isfinite([r["loss"], r["grad_norm_G"], r["grad_norm_F"]] + list(r["per_layer"].values())).all() for r in recs)
    for c in ids0:
        assert tuple(c.shape) == (P, 3) and c.dtype == torch.int64
        assert int(c.min()) >= 0 and int(c.max()) < 32 and len({tuple(v) for v in c.tolist()}) == P
    assert not torch.equal(ids0[1], ids0[2])
    g0 = netG.model[0].weight.grad
    assert g0 is not None and torch.isfinite(g0).all() and float(g0.abs().max()) > 0


def test_heads_run_once_per_step_when_the_losses_cannot_be_batched(device):
    """Criteria of unequal settings are not eligible for the batched loss: the route is decided before any head runs, so every head's
    BatchNorm1d takes ONE momentum update per step (2 warm-up steps + 3 replays), and statistics and losses are those of the eager
    step on the same inputs and coordinates (tolerance of test_graphed_contrastive_step_matches_eager_on_the_same_coordinates)."""
    netG, netF, crits, (A, B, seg) = _step_setup(device, [PI.NCE_T, 0.2, PI.NCE_T])
    g = torch.Generator().manual_seed(3)
    ids = [torch.stack([torch.randperm(32 ** 3, generator=g)[:P] // 1024, torch.randperm(32 ** 3, generator=g)[:P] // 32 % 32,
                        torch.randperm(32 ** 3, generator=g)[:P] % 32], dim=1).to(device) for _ in LAYERS]
    netG2, netF2 = copy.deepcopy(netG), copy.deepcopy(netF)
    step = GraphedContrastiveStep(netG, netF, crits, LAYERS, None, num_patches=P, warmup=2, sample_ids=ids)
    recs = [step(A, B, seg) for _ in range(3)]
    ref = [contrastive_step(netG2, netF2, crits, A, B, seg, LAYERS, num_patches=P, optimizers=None, sample_ids=ids) for _ in range(5)]
    norms = [(k, m, dict(netF2.named_modules())[k]) for k, m in netF.named_modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(norms) == 9
    for k, m, m2 in norms:
        assert int(m.num_batches_tracked) == 5 == int(m2.num_batches_tracked), k
        for a, b in ((m.running_mean, m2.running_mean), (m.running_var, m2.running_var)):
            assert float((a - b).norm()) <= 1e-5 * float(b.norm()), k
    for r, e in zip(recs, ref[2:]):
        assert abs(r["loss"] - e["loss"]) < 1e-5 * abs(e["loss"])
        for l in r["per_layer"]:
            assert abs(r["per_layer"][l] - e["per_layer"][l]) < 1e-5 * abs(e["per_layer"][l])
