"""The backward walk on the device (tests/_backward_walk.py): every block of the training backward at ragged sizes, each stage
against float64 of the operands the backward itself held.  ``AMX_WALK_REPORT=<file>`` appends every case's full report to that file
(profiles/backward_walk_gpu.txt is one such run)."""
import os

import numpy as np
import pytest
import torch

import _backward_walk as BW
import anatomix_amd
from anatomix_amd.model import train as TR
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu

KW6M = R.VARIANTS["anatomix"]
COT_LAYERS = [27, 31, 38, 45, 52]

# The 6M network, the settings of test_train_step_gpu.py::test_backward_matches_the_rounding_point_emulation (synthetic weights seed 3,
# gain sqrt(2), cotangents at 27, 31, 38, 45, 52 plus 0.1 mean(out^2), loss scale 1024 in f16).
#   A  D, H, W all different.  Level 0 has W = 80: partial x tile of the direct route, wide-row weight gradient with a remainder.
#      Level 1 has W = 40: direct route with a partial tile.  Level 2 has W = 20: below the direct route and below
#      OVERLAP_WGRAD_MIN_W.  Bottom is 2 x 3 x 5.
#   B  batch 1, the widest legal W, H the short axis.
#   C  batch 3, the narrowest legal W; level 1 has W = 16, so its weight gradients run inline.
CASES_6M = {
    "A-f16": ("f16", 2, (32, 48, 80)),
    "A-bf16": ("bf16", 2, (32, 48, 80)),
    "B-f16": ("f16", 1, (48, 32, 128)),
    "C-bf16": ("bf16", 3, (32, 64, 32)),
}

# The shallow variants of test_train_step_gpu.py (configurations and taps), batch 2, (8, 12, 40), f16, loss scale 4096.
_POOL_UP = dict(dimension=3, input_nc=1, output_nc=16, num_downs=2, ngf=16, interp="nearest", pooling="Max")
CASES_SHALLOW = {
    "instance-avg-trilinear": (dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance", pooling="Avg",
                                    interp="trilinear", norm_eps=1e-2), [3, 13, 20, 27, 34], {}),
    "instance_affine-lrelu-dx": (dict(dimension=3, input_nc=1, output_nc=16, num_downs=1, ngf=16, norm="instance_affine", activation="lrelu"),
                                 [0, 3, 5, 10, 13, 17, 20], dict(x_grad=True)),
    "batch-frozen-lrelu": (dict(dimension=3, input_nc=1, output_nc=16, num_downs=2, ngf=16, activation="lrelu"), [3, 13, 20, 27, 34],
                           dict(freeze=True)),
    "max-nearest-pool-up-taps": (_POOL_UP, "pool+up", {}),
}

# conv module id -> (data-gradient route, weight gradient on the side stream), filled from one run and reviewed against the comments
# above: the side stream is taken exactly where W >= OVERLAP_WGRAD_MIN_W = 32, but for the stem, whose weight gradient runs inline.
ROUTE_TABLE = {
    'A-f16': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', True), 13: ('direct', True), 17: ('fold', False),
        20: ('fold', False), 24: ('fold', False), 27: ('fold', False), 31: ('fold', False), 34: ('fold', False),
        38: ('upcat', False), 41: ('fold', False), 45: ('upcat', False), 48: ('fold', False), 52: ('upcat', True),
        55: ('direct', True), 59: ('split48', True), 62: ('direct', True), 65: ('direct', True)},
    'A-bf16': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', True), 13: ('direct', True), 17: ('fold', False),
        20: ('fold', False), 24: ('fold', False), 27: ('fold', False), 31: ('fold', False), 34: ('fold', False),
        38: ('upcat', False), 41: ('fold', False), 45: ('upcat', False), 48: ('fold', False), 52: ('upcat', True),
        55: ('direct', True), 59: ('split48', True), 62: ('direct', True), 65: ('direct', True)},
    'B-f16': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', True), 13: ('direct', True), 17: ('fold', True),
        20: ('fold', True), 24: ('fold', False), 27: ('fold', False), 31: ('fold', False), 34: ('fold', False),
        38: ('upcat', False), 41: ('fold', False), 45: ('upcat', True), 48: ('fold', True), 52: ('upcat', True),
        55: ('direct', True), 59: ('split48', True), 62: ('direct', True), 65: ('direct', True)},
    'C-bf16': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', False), 13: ('fold', False), 17: ('fold', False),
        20: ('fold', False), 24: ('fold', False), 27: ('fold', False), 31: ('fold', False), 34: ('fold', False),
        38: ('upcat', False), 41: ('fold', False), 45: ('upcat', False), 48: ('fold', False), 52: ('upcat', False),
        55: ('fold', False), 59: ('split48', True), 62: ('direct', True), 65: ('direct', True)},
    'instance-avg-trilinear': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', False), 13: ('fold', False), 17: ('fold', False),
        20: ('fold', False), 24: ('fold', False), 27: ('fold', False), 31: ('fold', True), 34: ('direct', True),
        37: ('direct', True)},
    'instance_affine-lrelu-dx': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', False), 13: ('fold', False),
        17: ('split48', True), 20: ('direct', True), 23: ('direct', True)},
    'batch-frozen-lrelu': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', False), 13: ('fold', False), 17: ('fold', False),
        20: ('fold', False), 24: ('upcat', False), 27: ('fold', False), 31: ('split48', True), 34: ('direct', True),
        37: ('direct', True)},
    'max-nearest-pool-up-taps': {
        0: ('stem', False), 3: ('direct', True), 6: ('direct', True), 10: ('fold', False), 13: ('fold', False), 17: ('fold', False),
        20: ('fold', False), 24: ('upcat', False), 27: ('fold', False), 31: ('split48', True), 34: ('direct', True),
        37: ('direct', True)},
}


def _report(case, recs):
    path = os.environ.get("AMX_WALK_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"== {case}\n{BW.report(recs)}\nworst err/tol per stage: "
                    + ", ".join(f"{s} {v:.3f}" for s, v in sorted(BW.summary(recs).items())) + "\n\n")


def _net(kw, precision, device, seed=3, gain=2 ** 0.5):
    net = anatomix_amd.Unet(**kw)
    net.load_state_dict(R.synthetic_state_dict(kw, seed, gain=gain), strict=True)
    net.precision = precision
    return net.to(device).train()


def _loss_6m(net, x, scale):
    out, feats = net(x, COT_LAYERS)
    g = torch.Generator().manual_seed(5)
    loss = 0.1 * out.square().mean()
    for f in feats:
        loss = loss + (f * (torch.randn(f.shape, generator=g) / f[0].numel() ** 0.5).to(x.device)).sum()
    return loss * scale


def _check(case, net, rec, precision, recs):
    print(BW.report(recs))
    _report(case, recs)
    observed = {b.module: (b.route, b.side) for b in rec.blocks.values()}
    print("routes", case, observed)
    steps = TR.plan_network(net, [])
    want = {s.idx for s in steps if isinstance(s, (TR.ConvBlock, TR.Pool))}
    got = {r.module for r in recs if r.stage != "uptap" and r.what != "skipped"}
    assert got == want, (sorted(got), sorted(want))
    assert observed == ROUTE_TABLE[case], observed
    frames = [(k, v) for k, v in TR.T._CACHE.items() if k[0] == "frame"]
    assert frames
    for key, fr in frames:                                       # nobody writes the frame: every cached buffer, after the backward
        border = fr.clone()
        TR.T.interior(border).zero_()
        assert not border.any(), key
    assert all(r.ok for r in recs), BW.report([r for r in recs if not r.ok])          # (last: the structure above is held even where a figure misses)


@pytest.mark.parametrize("case", list(CASES_6M))
def test_6m_backward_walk(device, case):
    """Every block of the 6M network's backward, every stage, no element over its bound.

    What this walk found (case A-f16, the record before the fix):
        module  0 wgrad stem d weight err/tol 1.013 rel_l2 1.01e-05 worst tap 1.46e-05 cond 487 err 0.35 fp32 ulp of sum|terms| FAIL
    The stem's weight-gradient sum is the worst conditioned of the network: a non-negative image against a gradient whose channel sums
    are zero (the BatchNorm adjoint removes them), |sum of |terms|| / |dW| = 487.  Measured on the recorded operands of that block,
    ``amx_conv3d_wgrad`` called again: the chunk partials summed in double 1.013e-05 and one call per sample 1.016e-05 (neither the
    reduction nor the length of the MFMA chains); the same dY against the image minus 0.5 6.6e-07 at condition number 242 -- fifteen
    times less error for half the cancellation; error uncorrelated with dW (0.02).  By elimination (not shown directly) the loss sits
    in the 32-voxel dot product of one MFMA step when all its products share a sign.  The fix is in model/train.py
    (``_stem_weight_grad``): the kernel runs on the image with its mean taken out and c * sum dY is added back; the same record
    now reads rel_l2 6.93e-07 (A-bf16 2.2e-06, B 5.8e-07, C 2.2e-06), and the worst layer of any case stands at 4.7e-06."""
    precision, batch, size = CASES_6M[case]
    net = _net(KW6M, precision, device)
    x = torch.from_numpy(np.random.RandomState(3).rand(batch, 1, *size).astype(np.float32)).to(device)
    loss = _loss_6m(net, x, 1024.0 if precision == "f16" else 1.0)
    with BW.Recorder(TR) as rec:
        loss.backward()
    _check(case, net, rec, precision, BW.walk(rec, precision, BW.K_GPU))


@pytest.mark.parametrize("case", list(CASES_SHALLOW))
def test_shallow_variant_backward_walk(device, case):
    kw, layers, opt = CASES_SHALLOW[case]
    net = _net(kw, "f16", device, gain=1.0)
    if layers == "pool+up":
        kinds = [type(m).__name__ for m in net.model]
        layers = [i for i, k in enumerate(kinds) if k in ("MaxPool3d", "AvgPool3d", "Upsample")] + [len(kinds) - 1]
    if opt.get("freeze"):
        for i, m in enumerate(net.model):
            if isinstance(m, torch.nn.BatchNorm3d) and i % 2 == 0:
                m.eval()
    x = R.synthetic_input(11, 2, (8, 12, 40)).to(device).requires_grad_(bool(opt.get("x_grad")))
    out, feats = net(x, layers)
    g = torch.Generator().manual_seed(5)
    cots = [torch.randn(f.shape, generator=g).to(device) / f[0].numel() ** 0.5 for f in feats]
    loss = sum((f * c).sum() for f, c in zip(feats, cots)) + 0.1 * out.square().mean()
    with BW.Recorder(TR) as rec:
        (loss * 4096.0).backward()
    recs = BW.walk(rec, "f16", BW.K_GPU)
    if opt.get("x_grad"):
        assert any(r.route == "stem" and r.stage == "dgrad" for r in recs)          # the image gradient was walked
    _check(case, net, rec, "f16", recs)


def test_recorder_changes_no_bit_and_the_backward_repeats(device):
    """Case A in bf16: parameter gradients with the recorder active are bit-identical to those without it, and two backward passes
    give bit-identical gradients."""
    precision, batch, size = CASES_6M["A-bf16"]
    x = torch.from_numpy(np.random.RandomState(3).rand(batch, 1, *size).astype(np.float32)).to(device)
    grads = []
    for recorded in (False, False, True):
        net = _net(KW6M, precision, device)
        loss = _loss_6m(net, x, 1.0)
        if recorded:
            with BW.Recorder(TR):
                loss.backward()
        else:
            loss.backward()
        grads.append({k: p.grad.detach().clone() for k, p in net.named_parameters()})
    assert len(grads[0]) > 50
    for k in grads[0]:
        assert torch.isfinite(grads[0][k]).all(), k
        assert torch.equal(grads[0][k], grads[1][k]), ("two passes differ", k)
        assert torch.equal(grads[0][k], grads[2][k]), ("the recorder changed", k)
