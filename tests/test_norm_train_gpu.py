"""GPU: the token LayerNorms and the SwiGLU gate under autograd on the library's own kernels (``train_norm = "hip"``:
amx_layernorm_train_forward + amx_layernorm_backward, csrc/amx_layernorm_train.hip) against the float64 autograd reference of
tests/_norm_train_ref.py.

Bars.  y, dx, dgate, dw, db: 2e-5 rel-L2 against float64, the project's bar for its fp32 training routes (fp32 torch on a CPU is within
2e-6 on these inputs, so a plain fp32 implementation holds it with a 10x margin).  mean and rstd: 1e-6 relative -- for rstd per element;
for mean as rel-L2 and as the largest error over the largest |mean| of the case, because a row mean may lie arbitrarily close to zero (the
rows' means are uniform in [-2, 2]) while the rounding of a sum of C fp32 terms is relative to the terms, not to their sum: no fp32
summation holds 1e-6 of such an element.

Measured on an MI355X, worst over the 14 cases (rel-L2 against float64; bar 2e-5): y 1.10e-7, dx 9.20e-8, dgate 1.08e-7, dw 1.57e-7,
db 1.23e-7; mean 1.24e-7 and rstd 1.69e-7 (bar 1e-6); MEASURED below names the cases, and every run prints its own figures.  The constant
row of the degenerate test comes out as b exactly on both forms."""
import contextlib
import io
import itertools
import json
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn as nn

import _norm_train_ref as R
import _preaug_ref as PR
from _tokenizer_train_ref import NORMED_BIAS
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d import architectures as ARCH
from oracle import vit_ref as V

pytestmark = pytest.mark.gpu

# worst rel-L2 against float64 per tensor over the 14 cases, as measured on an MI355X (the case in brackets)
MEASURED = {"y": "1.10e-7 (257x1056 plain)", "dx": "9.20e-8 (1x132 gated)", "dgate": "1.08e-7 (1x132 gated)", "dw": "1.57e-7 (8200x352 plain)",
            "db": "1.23e-7 (8200x352 gated)", "mean": "1.24e-7 (5x396 plain)", "rstd (per element)": "1.69e-7 (8200x352)"}
BAR, STAT_BAR = 2e-5, 1e-6
HERE = os.path.dirname(os.path.abspath(__file__))
H5 = os.path.join(HERE, "golden", "two_view_train_data.hdf5")
BATCHED_CASES = [(2100, 132, False), (2100, 132, True)]


def entries(dev, x, gate, w, b, dy, eps, null=()):
    """The two C entries on plain device tensors [M, C]: a dict over R.TENSORS; outputs named in ``null`` are passed as null and come
    back as None.  Outputs start as NaN and the scratch as 0xA5 bytes: nothing an earlier call left is read."""
    lib = _lib.load()
    M, C = x.shape
    new = lambda like, name: None if name in null else torch.full_like(like, float("nan"))
    y, mean, rstd = new(x, "y"), torch.full((M,), float("nan"), device=dev), torch.full((M,), float("nan"), device=dev)
    out = dict(dx=new(x, "dx"), dgate=None if gate is None else new(x, "dgate"), dw=new(w, "dw"), db=new(w, "db"))
    with torch.cuda.device(dev):
        nb = lib.amx_layernorm_train_scratch_bytes(M, C)
        assert nb > 0
        sc = _lib.scratch(nb, dev)
        sc.fill_(0xA5)
        _lib.check(lib.amx_layernorm_train_forward(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(w), _lib.ptr(b), eps, M, C, _lib.ptr(y), _lib.ptr(mean),
                                                   _lib.ptr(rstd), _lib.stream(dev)))
        _lib.check(lib.amx_layernorm_backward(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(w), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(dy), M, C,
                                              _lib.ptr(out["dx"]), _lib.ptr(out["dgate"]), _lib.ptr(out["dw"]), _lib.ptr(out["db"]), _lib.ptr(sc), nb,
                                              _lib.stream(dev)))
    return dict(out, y=y, mean=mean, rstd=rstd)


def on_device(case, dev):
    return [None if t is None else t.to(dev) for t in R.inputs(case)]


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_entries_against_float64(case, device):
    """Item 1: every tensor of every case, nothing excluded from any norm."""
    ref = R.reference(case)
    got = entries(device, *on_device(case, device), R.eps_of(case))
    line = []
    for name in ("y", "dx", "dgate", "dw", "db"):
        if ref[name] is None:
            assert got[name] is None
            continue
        assert torch.isfinite(got[name]).all(), name
        e = R.rel_l2(got[name], ref[name])
        line.append(f"{name} {e:.2e}")
        assert e <= BAR, (name, e)
    mean, rstd = got["mean"].double().cpu(), got["rstd"].double().cpu()
    e_rstd = ((rstd - ref["rstd"]).abs() / ref["rstd"]).max().item()
    e_mean = max(R.rel_l2(mean, ref["mean"]), ((mean - ref["mean"]).abs().max() / ref["mean"].abs().max()).item())
    print(f"{R.case_id(case)}: " + ", ".join(line) + f", mean {e_mean:.2e}, rstd (per element) {e_rstd:.2e}")
    assert torch.isfinite(mean).all() and torch.isfinite(rstd).all()
    assert e_mean <= STAT_BAR and e_rstd <= STAT_BAR, (e_mean, e_rstd)


def _through_the_functions(dev, case, x=None, dy=None):
    """The autograd functions on the batched input of a case: y and the gradients."""
    x0, gate, w, b, dy0 = on_device(case, dev)
    lead = R.BATCHED[case[0]]
    x = x0.reshape(*lead, -1) if x is None else x
    dy = dy0.reshape(*lead, -1) if dy is None else dy
    leaves = [t.detach().requires_grad_(True) for t in (x, w.clone(), b.clone())]         # (x keeps its strides)
    if gate is None:
        y = ARCH._LayerNormFn.apply(leaves[0], leaves[1], leaves[2], R.eps_of(case))
        dx, dw, db = torch.autograd.grad(y, leaves, dy)
        dgate = None
    else:
        g = gate.reshape(*lead, -1).detach().requires_grad_(True)
        y = ARCH._GatedLayerNormFn.apply(g, leaves[0], leaves[1], leaves[2], R.eps_of(case))
        dgate, dx, dw, db = torch.autograd.grad(y, [g] + leaves, dy)
    assert y.shape == x.shape and dx.shape == x.shape and y.is_contiguous()
    return dict(y=y.detach(), dx=dx, dgate=dgate, dw=dw, db=db)


@pytest.mark.parametrize("case", BATCHED_CASES, ids=R.case_id)
def test_bit_equalities(case, device):
    """Item 2, on the [2, 1050, 132] input: the functions return the bits of the entries; every subset of null gradient outputs leaves
    the others bit-equal; two runs are bit-equal; a non-contiguous dy and a non-contiguous x give the bits of their contiguous copies."""
    args = on_device(case, device)
    eps = R.eps_of(case)
    full = entries(device, *args, eps)
    names = [n for n in ("dx", "dgate", "dw", "db") if full[n] is not None]
    same = lambda a, b, keys: all(torch.equal(a[k].reshape(-1), b[k].reshape(-1)) for k in keys)
    again = entries(device, *args, eps)
    assert same(full, again, names + ["y", "mean", "rstd"])
    for r in range(1, len(names) + 1):
        for null in itertools.combinations(names, r):
            got = entries(device, *args, eps, null=null)
            assert all(got[n] is None for n in null)
            assert same(full, got, [n for n in names if n not in null]), null
    fn = _through_the_functions(device, case)
    assert same(full, fn, names + ["y"])
    # non-contiguous views of the same values: every second column of a twice as wide tensor, and a transposed dy
    lead = R.BATCHED[case[0]]
    x, dy = args[0].reshape(*lead, -1), args[4].reshape(*lead, -1)
    wide = torch.zeros(*x.shape[:-1], 2 * x.shape[-1], device=device)
    wide[..., ::2] = x
    dyt = dy.transpose(0, 1).contiguous().transpose(0, 1)
    assert not wide[..., ::2].is_contiguous() and not dyt.is_contiguous() and torch.equal(dyt, dy)
    assert same(full, _through_the_functions(device, case, x=wide[..., ::2], dy=dyt), names + ["y"])


@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gated"])
def test_degenerate_rows(gated, device):
    """Item 3.  An all-zero row: y == b exactly, finite gradients.  A row of the constant v = 0.75: finite, and
    |y - b| <= 4 * 2^-24 * |v| / sqrt(eps) * |w| -- a last-place error of the mean is amplified by rstd = 1 / sqrt(eps); the property of
    the arithmetic, stated.  Gated: x is the degenerate row, so u is; the constant row gets the constant gate 1.25, u = silu(1.25) v is
    then no short binary fraction and the partial sums of the mean round: at C = 396 a lane adds at most 8 terms, the butterfly has 6
    steps and the division rounds once, each at most 2^-24 of a running sum that never exceeds the total (equal signs) -- 16 in place of
    the 4."""
    C, eps, v = 396, 1e-6, 0.75
    g = torch.Generator().manual_seed(77)
    x = torch.randn(6, C, generator=g)
    x[1], x[4] = 0.0, v
    gate = 2 * torch.randn(6, C, generator=g) if gated else None
    if gated:
        gate[4] = 1.25
    w, b, dy = 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g), torch.randn(6, C, generator=g)
    dev = lambda t: None if t is None else t.to(device)
    got = entries(device, dev(x), dev(gate), dev(w), dev(b), dev(dy), eps)
    for name, t in got.items():
        assert t is None or torch.isfinite(t).all(), name
    y = got["y"].cpu()
    assert torch.equal(y[1], b)
    u = v * (1.25 / (1 + np.exp(-1.25))) if gated else v
    bound = (16 if gated else 4) * 2.0 ** -24 * abs(u) / np.sqrt(eps) * w.abs()
    dev_c = (y[4] - b).abs()
    print(f"constant row: max |y - b| {dev_c.max().item():.3e}, smallest bound {bound.min().item():.3e}")
    assert (dev_c <= bound).all()
    assert got["mean"][1].item() == 0.0 and abs(got["rstd"][1].item() - 1e3) <= 1e-3
    # the other rows are ordinary rows of the same call
    ref = R.autograd(x, gate, w, b, dy, eps)
    keep = [0, 2, 3, 5]
    assert R.rel_l2(y[keep], ref["y"][keep]) <= BAR and R.rel_l2(got["dx"].cpu()[keep], ref["dx"][keep]) <= BAR


def test_envelope(device):
    """Item 4."""
    lib = _lib.load()
    for m, c in ((16, 6), (16, 398), (16, 4100), (0, 132)):
        assert lib.amx_layernorm_train_scratch_bytes(m, c) == 0, (m, c)
    x, _, w, b, dy = on_device((5, 396, False), device)
    st = _lib.stream(device)
    mean, rstd = torch.zeros(5, device=device), torch.ones(5, device=device)
    # a null y: refused before any launch
    rc = lib.amx_layernorm_train_forward(_lib.ptr(x), None, _lib.ptr(w), _lib.ptr(b), 1e-6, 5, 396, None, _lib.ptr(mean), _lib.ptr(rstd), st)
    assert rc == _lib.AMX_ERR_INVALID and "null" in lib.amx_last_error().decode()
    # a short scratch on backward
    nb = lib.amx_layernorm_train_scratch_bytes(5, 396)
    sc = _lib.scratch(nb, device)
    dx = torch.full_like(x, 7.0)
    rc = lib.amx_layernorm_backward(_lib.ptr(x), None, _lib.ptr(w), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(dy), 5, 396, _lib.ptr(dx), None, None, None,
                                    _lib.ptr(sc), nb - 1, st)
    assert rc == _lib.AMX_ERR_WORKSPACE and str(nb) in lib.amx_last_error().decode()
    torch.cuda.synchronize(device)
    assert (dx == 7.0).all() and (mean == 0).all()                    # nothing ran
    # C = 398: the function names the shape, the helper falls back to the module
    layer = nn.LayerNorm(398, eps=1e-6).to(device)
    xo = torch.randn(3, 7, 398, device=device, requires_grad=True)
    with pytest.raises(_lib.AmxError, match=r"\(21, 398\)"):
        ARCH._LayerNormFn.apply(xo, layer.weight, layer.bias, layer.eps)
    y = ARCH._layer_norm(layer, xo, "hip")
    assert torch.equal(y, layer(xo)) and "NativeLayerNorm" in type(y.grad_fn).__name__
    # inside the envelope the helper takes the function -- and not under no_grad, not on the "torch" route, not for an Identity
    layer = nn.LayerNorm(396, eps=1e-6).to(device)
    xi = torch.randn(3, 7, 396, device=device, requires_grad=True)
    assert "_LayerNormFn" in type(ARCH._layer_norm(layer, xi, "hip").grad_fn).__name__
    assert "NativeLayerNorm" in type(ARCH._layer_norm(layer, xi, "torch").grad_fn).__name__
    with torch.no_grad():
        assert ARCH._layer_norm(layer, xi, "hip").grad_fn is None
    assert ARCH._layer_norm(nn.Identity(), xi, "hip") is xi


KW = dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(32, 32, 32), eva_depth=2)


def _net(device):
    m = PrimusV2(**KW)
    m.load_state_dict(V.synthetic_state_dict(KW, 3), strict=True)
    return m.to(device).train()


# the seven conv biases of the tokenizer in front of an InstanceNorm and the last decoder bias in front of the "demean" output norm:
# the norm removes them, their gradient is mathematically zero (in float64 on a CPU: 1e-18 .. 1e-16; no other parameter of this network)
ZERO_GRAD = ["down_projection." + n for n in NORMED_BIAS] + ["up_projection.decode.2.bias"]


def _record_conv_output_gradients(m, store):
    """store[bias name] = sum over the voxels of |d raw| per channel for the convs of ZERO_GRAD: the terms whose sum the bias gradient is."""
    def hook(name):
        def fwd(mod, args, out):
            out.register_hook(lambda g: store.__setitem__(name, g.abs().sum((0, 2, 3, 4))))
        return fwd
    return [m.get_submodule(name[:-len(".bias")]).register_forward_hook(hook(name)) for name in ZERO_GRAD]


def test_wiring_through_primus(device):
    """Item 5: PrimusV2 (anatomix-dev-vit at 32^3, depth 2), two views, loss y.square().mean(): ``train_norm`` torch against hip with the
    other switches on torch, 1e-4 rel-L2 on y and every parameter gradient; then all four switches on hip.

    The eight gradients of ZERO_GRAD are mathematically zero: what either route holds there is the rounding of a sum whose terms cancel, and
    a rel-L2 between two such values says nothing (0.99 for stem.conv.bias, 1.18 for decode.2.bias on an MI355X).  They are held to the same 1e-4, of the sum of
    the magnitudes of their terms, on both routes -- zero to the precision of the sum.  Measured on an MI355X: y 4.39e-7, worst gradient
    2.74e-6 (down_projection.stem.conv.weight)."""
    x = V.synthetic_input(21, 2, (32, 32, 32)).to(device)
    out, calls = {}, []
    orig = (ARCH._LayerNormFn.forward, ARCH._GatedLayerNormFn.forward)
    ARCH._LayerNormFn.forward = staticmethod(lambda ctx, *a: (calls.append("plain"), orig[0](ctx, *a))[1])
    ARCH._GatedLayerNormFn.forward = staticmethod(lambda ctx, *a: (calls.append("gated"), orig[1](ctx, *a))[1])
    try:
        for route in ("torch", "hip"):
            m = _net(device)
            m.train_norm = route
            assert m.train_attention == "torch" and m.train_linear == "torch" and m.train_tokenizer == "torch"
            terms = {}
            hooks = _record_conv_output_gradients(m, terms)
            y = m(x)
            y.square().mean().backward()
            for h in hooks:
                h.remove()
            assert y.grad_fn is not None and torch.isfinite(y).all()
            out[route] = dict(y=y.detach(), grads={k: p.grad.clone() for k, p in m.named_parameters()}, terms=terms)
            if route == "torch":
                assert calls == []
        # per block norm1, attn.norm, norm2 and the gated mlp.norm; then the final norm
        assert calls == ["plain", "plain", "plain", "gated"] * 2 + ["plain"]
        hip, tor = out["hip"], out["torch"]
        e_y = R.rel_l2(hip["y"], tor["y"])
        worst = ("", 0.0)
        assert set(hip["grads"]) == set(tor["grads"])
        assert len(ZERO_GRAD) == 8 and all(k in tor["grads"] for k in ZERO_GRAD)
        for k in tor["grads"]:
            if k in ZERO_GRAD:
                assert all((o["grads"][k].abs() <= 1e-4 * o["terms"][k]).all() and o["terms"][k].min() > 0 for o in (hip, tor)), k
                continue
            e = R.rel_l2(hip["grads"][k], tor["grads"][k])
            worst = max(worst, (k, e), key=lambda t: t[1])
            assert e <= 1e-4, (k, e)
        for must in ("eva.blocks.0.norm1.weight", "eva.blocks.1.norm2.bias", "eva.blocks.0.attn.norm.weight", "eva.blocks.1.mlp.norm.bias",
                     "eva.blocks.1.mlp.norm.weight", "eva.norm.weight", "eva.norm.bias", "eva.blocks.0.gamma_1", "eva.blocks.1.gamma_2"):
            assert must in tor["grads"] and tor["grads"][must].abs().max() > 0, must
        print(f"wiring: y {e_y:.2e}; worst gradient rel-L2 between the routes {worst[0]} {worst[1]:.2e}")
        assert e_y <= 1e-4
        m = _net(device)
        m.train_norm = m.train_attention = m.train_linear = m.train_tokenizer = "hip"
        assert m.tokenizer_unsupported_reason(x) is None
        m(x).square().mean().backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
        # no_grad (the engine) and eval without the engine do not reach the functions
        n = len(calls)
        m.eval()
        with torch.no_grad():
            m(x)
            m.use_engine = False
            m(x)
        assert len(calls) == n
    finally:
        ARCH._LayerNormFn.forward, ARCH._GatedLayerNormFn.forward = staticmethod(orig[0]), staticmethod(orig[1])


def test_contrastive_step_on_both_routes(device):
    """Item 6: one ``contrastive_step`` at 32^3 with 64 patches, the other three switches on hip: the losses within 1e-5 relative."""
    from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss, contrastive_step
    g = torch.Generator().manual_seed(40)
    v = torch.randn(2, 1, 32, 32, 32, generator=g).to(device)
    seg = torch.from_numpy(PR.blob_volume((32, 32, 32), 41, n_labels=4)[1][None, None]).float().to(device)
    ids = [torch.randint(0, 32, (64, 3), generator=torch.Generator().manual_seed(43)).to(device)]
    loss = {}
    for route in ("torch", "hip"):
        netG = _net(device)
        netG.train_attention = netG.train_linear = netG.train_tokenizer = "hip"
        netG.train_norm = route
        with contextlib.redirect_stdout(io.StringIO()):
            netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=64, n_mlps=3)
            torch.manual_seed(9)
            netF.create_mlp([torch.zeros(1, KW["num_classes"], 1, 1, 1, device=device)])
        netF = netF.to(device).train()
        crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
        rec = contrastive_step(netG, netF, crits, v[:1], v[1:], seg, [-1], num_patches=64, sample_ids=ids)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in netG.parameters())
        loss[route] = rec["loss"]
    print("contrastive_step loss", loss)
    assert abs(loss["hip"] - loss["torch"]) <= 1e-5 * abs(loss["torch"])


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


def test_driver_with_the_norms_on_hip(tmp_path, device):
    """Item 7: two iterations of ``pretrain`` at --crop_size 32 with --primus_train_norm hip: log, checkpoints, finite losses."""
    from anatomix_amd.pretraining import AugmentedTwoViewLoader
    from anatomix_amd.pretraining.pretrain_anatomix import build_networks, build_parser, options_from_args, pretrain
    shutil.copy(H5, tmp_path / "train_data.hdf5")
    shutil.copy(H5, tmp_path / "val_data.hdf5")
    img, lab = PR.blob_volume((32, 32, 32), 78, n_labels=4)
    val = [{"A": torch.from_numpy(img[None, None]).float(), "B": torch.from_numpy(0.8 * img[None, None] + 0.05).float(),
            "A_seg": torch.from_numpy(lab[None, None]).float()}]
    argv = ["--ckpt_dir", str(tmp_path / "ckpt"), "--name", "norm", "--dataroot", str(tmp_path), "--netG", "primus", "--primus_version", "v2",
            "--primus_config", "S", "--crop_size", "32", "--batch_size", "1", "--num_patches", "64", "--max_iters", "2", "--evaluation_freq", "2",
            "--n_epochs", "1", "--n_epochs_decay", "1", "--print_freq", "1", "--primus_train_norm", "hip"]
    opt = options_from_args(build_parser(primus_route=True).parse_args(argv))
    loader = AugmentedTwoViewLoader(opt, device=device, seed=opt.loader_seed)
    loader.dataset = InMemory(2)
    calls = []
    orig = ARCH._GatedLayerNormFn.forward

    def counted(ctx, *a):
        calls.append(1)
        return orig(ctx, *a)

    ARCH._GatedLayerNormFn.forward = staticmethod(counted)
    try:
        out = pretrain(opt, train_loader=loader, val_loader=val)
    finally:
        ARCH._GatedLayerNormFn.forward = staticmethod(orig)
    assert out["netG"].train_norm == "hip" and out["netG"].train_tokenizer == "torch" and len(calls) >= 2 * 12
    log = [json.loads(l) for l in open(os.path.join(out["save_dir"], "log.jsonl"))]
    train = [l for l in log if l["kind"] == "train"]
    assert [l["total_iters"] for l in train] == [1, 2] and all(np.isfinite(l["loss"]) and l["loss"] > 0 for l in train)
    fresh = build_networks(opt, torch.device("cpu"))[0]
    fresh.load_state_dict(torch.load(os.path.join(out["save_dir"], "2_net_G.pth")), strict=True)
