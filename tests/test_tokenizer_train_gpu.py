"""GPU: the conv tokenizer under autograd on the library's own kernels (``train_tokenizer = "hip"``: amx_tokenizer_train_forward +
amx_tokenizer_backward, csrc/amx_tokenizer_bwd.hip) against the float64 restatement of tests/_tokenizer_train_ref.py.

Cases A, B, C are tests/_tokenizer_train_ref.py's; X (1 x 64 x 64 x 256) is the smallest input whose first stage has the 131072
output voxels at which tokconv takes its 64-voxel waves (its float64 reference takes a few seconds, and the fp32-on-CPU condition of
the backward test is not evaluated for it).  Measured on an MI355X (rel-L2 against float64; bar 2e-5): h3 A 1.94e-6, B 1.95e-6,
C 1.96e-6, X 2.07e-6, and 0 against the engine's tokenizer; worst gradient A 2.64e-6, B 2.71e-6, C 3.01e-6, X 8.04e-6; A with d_h3
x 1e-8 / x 1e+4: 0.84 .. 1.17 times the unscaled figures; differing mask elements per site: 0 in A, B, C, at most 2 in X."""
import contextlib
import ctypes
import io
import json
import os
import shutil
from argparse import Namespace

import numpy as np
import pytest
import torch

import _preaug_ref as PR
import _tokenizer_train_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d import architectures as ARCH

pytestmark = pytest.mark.gpu

BAR = 2e-5
HERE = os.path.dirname(os.path.abspath(__file__))
H5 = os.path.join(HERE, "golden", "two_view_train_data.hdf5")
# X: the smallest input whose first stage has 131072 output voxels, where tokconv takes its 64-voxels-per-wave instances
CASES = dict(R.CASES, X=(1, (64, 64, 256)))
SITE_SHAPE = lambda n, size, site: (n, (32, 32, 32, 64, 64, 128, 128)[site]) + tuple(s >> ((site + 1) // 2) for s in size)


class Route:
    """One shape on the device: the C entries with plain tensors."""

    def __init__(self, dev, n, size):
        self.dev, self.n, self.size, self.dims = dev, n, tuple(size), (n,) + tuple(size)
        self.lib = _lib.load()
        with torch.cuda.device(dev):
            self.sb = self.lib.amx_tokenizer_train_saved_bytes(*self.dims)
            self.nb = self.lib.amx_tokenizer_train_scratch_bytes(*self.dims)
        assert self.sb > 0 and self.nb > 0

    def forward(self, x, params):
        h3 = torch.full((self.n, 128) + tuple(s // 8 for s in self.size), float("nan"), dtype=torch.float32, device=self.dev)
        saved = torch.empty(self.sb, dtype=torch.uint8, device=self.dev)
        with torch.cuda.device(self.dev):
            sc = _lib.scratch(self.nb, self.dev)
            arr = (ctypes.c_void_p * 37)(*[p.data_ptr() for p in params])
            _lib.check(self.lib.amx_tokenizer_train_forward(_lib.ptr(x), arr, *self.dims, R.EPS, _lib.ptr(h3), _lib.ptr(saved), self.sb, _lib.ptr(sc),
                                                            self.nb, _lib.stream(self.dev)))
        return h3, saved

    def backward(self, d_h3, x, params, saved, null=()):
        grads = [None if i in null else torch.full_like(p, float("nan")) for i, p in enumerate(params)]
        with torch.cuda.device(self.dev):
            sc = _lib.scratch(self.nb, self.dev)
            sc.fill_(0xA5)                                  # nothing a forward or an earlier backward left in the scratch is read
            arr = (ctypes.c_void_p * 37)(*[p.data_ptr() for p in params])
            garr = (ctypes.c_void_p * 37)(*[None if g is None else g.data_ptr() for g in grads])
            _lib.check(self.lib.amx_tokenizer_backward(_lib.ptr(d_h3), _lib.ptr(x), arr, _lib.ptr(saved), *self.dims, R.EPS, garr, _lib.ptr(sc), self.nb,
                                                       _lib.stream(self.dev)))
        return grads

    def export(self, saved, site):
        out = torch.full(SITE_SHAPE(self.n, self.size, site), float("nan"), dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(self.lib.amx_tokenizer_train_export(_lib.ptr(saved), *self.dims, site, _lib.ptr(out)))
        return out

    def launches(self):
        buf = ctypes.create_string_buffer(1 << 14)
        _lib.check(self.lib.amx_tokenizer_train_route(*self.dims, buf, len(buf)))
        return buf.value.decode().split()


_cache = {}


def _case(name, device):
    """Everything one case needs, computed once: inputs, the free float64 reference, the route's forward, its masks, the float64
    reference forced to those masks, and the route's gradients."""
    if name in _cache:
        return _cache[name]
    n, size = CASES[name]
    p = R.parameters(0)
    x, d_h3 = R.inputs((n, size))
    c = Namespace(name=name, n=n, size=size, p=p, x=x, d_h3=d_h3, route=Route(device, n, size))
    c.free = R.reference(x, p, d_h3)
    c.xd, c.dd, c.pd = x.to(device), d_h3.to(device), [t.to(device) for t in p.values()]
    c.h3, c.saved = c.route.forward(c.xd, c.pd)
    c.act = [c.route.export(c.saved, s) for s in range(7)]
    c.masks = [a.cpu() > 0 for a in c.act]
    c.forced = R.reference(x, p, d_h3, masks=c.masks)
    c.grads = c.route.backward(c.dd, c.xd, c.pd, c.saved)
    _cache[name] = c
    return c


@pytest.fixture(scope="module", params=list(CASES))
def case(request, device):
    return _case(request.param, device)


def _check_grads(tag, grads, forced, bar=BAR):
    """Item 3: every gradient that is not mathematically zero to ``bar`` rel-L2; the seven normed conv biases to 1e-3 sum |d_raw|."""
    worst, fails = ("", 0.0), []
    for g, name in zip(grads, R.NAMES):
        assert g is not None and torch.isfinite(g).all(), (tag, name)
        ref = forced["grads"][name]
        if name in R.NORMED_BIAS:
            ratio = (g.double().cpu().abs() / (1e-3 * forced["draw_abs"][name]).clamp_min(1e-300)).max().item()
            print(f"{tag} {name}: |db| / (1e-3 sum |d_raw|) = {ratio:.2e}")
            if ratio > 1.0:
                fails.append((name, ratio))
            continue
        e = R.rel_l2(g.reshape(ref.shape), ref)
        worst = max(worst, (name, e), key=lambda t: t[1])
        print(f"{tag} {name}: rel-L2 {e:.2e} (ratio to the bar {e / bar:.2f})")
        if not e < bar:
            fails.append((name, e))
    print(f"{tag} worst gradient {worst[0]} {worst[1]:.2e}")
    assert not fails, (tag, fails)
    return worst[1]


def test_forward_matches_float64_and_the_engine(case, device):
    """Item 1."""
    e = R.rel_l2(case.h3, case.free["h3"])
    print(f"{case.name}: h3 rel-L2 vs float64 {e:.2e}")
    assert torch.isfinite(case.h3).all() and e < BAR
    assert torch.equal(case.act[6], case.h3)
    kw = dict(input_channels=1, num_classes=8, embed_dim=132, patch_embed_size=(8, 8, 8), eva_depth=1, eva_numheads=2, input_shape=case.size,
              init_values=0.1, scale_attn_inner=True, qk_norm=True, in_eps=R.EPS)
    torch.manual_seed(3)
    m = PrimusV2(**kw)
    m.down_projection.load_state_dict(dict(case.p, **{"proj.weight": m.down_projection.proj.weight, "proj.bias": m.down_projection.proj.bias}))
    m = m.to(device).eval()
    with torch.no_grad():
        _, taps = m.forward_hip(case.xd, taps=["s2.h"])
    (hi, lo), _ = taps["s2.h"]
    eng = (hi.float() + lo.float()).view(case.n, -1, 128).transpose(1, 2).reshape(case.h3.shape)
    e2 = R.rel_l2(case.h3, eng)
    print(f"{case.name}: h3 rel-L2 vs the engine's tokenizer {e2:.2e}")
    assert e2 < BAR


def test_masks_match_float64_outside_the_rounding_band(case):
    """Item 2."""
    for site, (act, pre) in enumerate(zip(case.act, case.free["pre"])):
        assert torch.isfinite(act).all()
        band = pre.abs() <= 2e-5 * pre.abs().max()
        differ = (act.cpu() > 0) != (pre > 0)
        print(f"{case.name} {R.SITES[site]}: {int(differ.sum())} differing, {int((differ & ~band).sum())} outside the band")
        assert not (differ & ~band).any() and int(differ.sum()) <= 16


def test_backward_matches_float64_with_the_routes_masks(case):
    """Item 3, with the condition on the inputs: fp32 torch on the CPU stays within 1e-5 of float64 on the same case."""
    if case.name != "X":
        f32 = R.reference(case.x, case.p, case.d_h3, masks=case.masks, dtype=torch.float32)
        cond = max(R.rel_l2(f32["grads"][k], case.forced["grads"][k]) for k in R.NAMES if k not in R.NORMED_BIAS)
        print(f"{case.name}: fp32 torch CPU worst rel-L2 vs float64 {cond:.2e}")
        assert cond < 1e-5
    _check_grads(case.name, case.grads, case.forced)


def test_launch_report_reaches_every_instance(device):
    """Every kernel instance the route can launch is launched by one of the cases."""
    seen = set()
    for name, (n, size) in CASES.items():
        seen |= set(Route(device, n, size).launches())
    conv = {f"tokconv<{t},{s},{mt},{nt},split>" for (t, s) in ((27, 2), (27, 1), (1, 1)) for mt in (2, 4) for nt in (2, 4)}
    print(sorted(seen))
    assert {"tokstem<0,split>", "tokstem<1,split>", "tokwgrad<27,2>", "tokwgrad<27,1>", "tokwgrad<1,1>", "tokdgrad2<2,2>", "tokstem_bwd<0>",
            "tokstem_bwd<1>", "tok_nadj_stats", "tok_nadj_apply", "tok_nadj_finalize", "tok_finalize_train", "tok_split", "tok_amax_fix"} <= seen
    # 64-voxel waves (mt 4) need 131072 output voxels: inside the envelope (2^22 input voxels) only the 32-channel first stage has them
    conv = {c for c in conv if not c.endswith(",4,4,split>")}
    assert {s for s in seen if s.startswith("tokconv")} == conv, sorted(conv ^ {s for s in seen if s.startswith("tokconv")})


def test_gradient_range(device):
    """Item 4: d_h3 scaled by 1e-8 and by 1e+4 gives the unscaled rel-L2 to within a factor of 2; everything is finite."""
    c = _case("A", device)
    base = {name: R.rel_l2(g.reshape(c.forced["grads"][name].shape), c.forced["grads"][name]) for g, name in zip(c.grads, R.NAMES) if name not in R.NORMED_BIAS}
    for scale in (1e-8, 1e4):
        grads = c.route.backward(c.dd * scale, c.xd, c.pd, c.saved)
        for g, name in zip(grads, R.NAMES):
            assert torch.isfinite(g).all(), (scale, name)
            if name in R.NORMED_BIAS:
                assert (g.double().cpu().abs() <= 1e-3 * scale * c.forced["draw_abs"][name]).all(), (scale, name)
                continue
            ref = c.forced["grads"][name] * scale
            e = R.rel_l2(g.reshape(ref.shape), ref)
            print(f"A x {scale:g} {name}: {e:.2e} (unscaled {base[name]:.2e})")
            assert e < BAR and base[name] / 2 <= e <= base[name] * 2, (scale, name, e, base[name])


def test_determinism_nulls_and_two_forwards(device):
    """Item 5."""
    c = _case("B", device)
    again = c.route.backward(c.dd, c.xd, c.pd, c.saved)
    assert all(torch.equal(a, b) for a, b in zip(again, c.grads))
    for i in range(37):
        part = c.route.backward(c.dd, c.xd, c.pd, c.saved, null=(i,))
        assert part[i] is None and all(torch.equal(a, b) for j, (a, b) in enumerate(zip(part, c.grads)) if j != i), R.NAMES[i]
    # a second forward (another input, its own saved state) between the first forward and its backward
    h3b, saved_b = c.route.forward(c.xd.flip(2) * 0.5, c.pd)
    assert not torch.equal(h3b, c.h3)
    assert all(torch.equal(a, b) for a, b in zip(c.route.backward(c.dd, c.xd, c.pd, c.saved), c.grads))


KW = dict(input_channels=1, num_classes=8, embed_dim=132, patch_embed_size=(8, 8, 8), eva_depth=2, eva_numheads=2, input_shape=(32, 32, 32),
          init_values=0.1, scale_attn_inner=True, qk_norm=True, num_register_tokens=8, in_eps=R.EPS)


def _net(device):
    torch.manual_seed(5)
    m = PrimusV2(**KW)
    tok = m.down_projection
    tok.load_state_dict(dict(R.parameters(1), **{"proj.weight": tok.proj.weight, "proj.bias": tok.proj.bias}))
    return m.to(device).train()


def test_wiring_through_primus(device):
    """Item 6: PrimusV2 at 32^3, depth 2, 8 register tokens, loss y.square().mean(), on both routes."""
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 1, 32, 32, 32, generator=g).to(device)
    out = {}
    for route in ("torch", "hip"):
        m = _net(device)
        m.train_tokenizer = route
        assert m.tokenizer_unsupported_reason(x) is None and m.train_attention == "torch" and m.train_linear == "torch"
        seen = {}
        def tap(mod, args, seen=seen):                      # h3 as proj receives it, and the gradient autograd delivers for it
            seen["h3"] = args[0].detach().clone()
            args[0].register_hook(lambda gr: seen.__setitem__("d_h3", gr.clone()))

        hook = m.down_projection.proj.register_forward_pre_hook(tap)
        y = m(x)
        y.square().mean().backward()
        hook.remove()
        out[route] = dict(y=y.detach(), grads={k: p.grad.clone() for k, p in m.named_parameters()}, **seen)
        assert (y.grad_fn is not None) and torch.isfinite(y).all()
    hip, tor = out["hip"], out["torch"]
    # _TokenizerFn returns the bits of the C entries
    p = R.parameters(1)
    pd = [t.to(device) for t in p.values()]
    r = Route(device, 2, (32, 32, 32))
    h3, saved = r.forward(x, pd)
    assert torch.equal(h3, hip["h3"])
    direct = r.backward(hip["d_h3"].contiguous(), x, pd, saved)
    for name, gd in zip(R.NAMES, direct):
        assert torch.equal(gd, hip["grads"]["down_projection." + name]), name
    # the tokenizer's gradients against the forced-mask float64 reference fed with the d_h3 autograd delivered
    masks = [r.export(saved, s).cpu() > 0 for s in range(7)]
    forced = R.reference(x.cpu(), p, hip["d_h3"].cpu(), masks=masks)
    _check_grads("wiring", direct, forced)
    worst = ("", 0.0)
    for k in tor["grads"]:
        if k.startswith("down_projection.") and not k.startswith("down_projection.proj"):
            continue
        e = R.rel_l2(hip["grads"][k], tor["grads"][k])
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < 1e-4, (k, e)
    print(f"wiring: worst rel-L2 between the routes outside the tokenizer {worst[0]} {worst[1]:.2e}; y {R.rel_l2(hip['y'], tor['y']):.2e}")
    # a reason present: the torch modules run whatever the switch says
    m = _net(device)
    m.train_tokenizer = "hip"
    xg = x.clone().requires_grad_(True)
    assert "gradient" in m.tokenizer_unsupported_reason(xg)
    m(xg).square().mean().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()


def test_contrastive_step_on_both_routes(device):
    from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss, contrastive_step
    g = torch.Generator().manual_seed(40)
    v = torch.randn(2, 1, 32, 32, 32, generator=g).to(device)
    seg = torch.from_numpy(PR.blob_volume((32, 32, 32), 41, n_labels=4)[1][None, None]).float().to(device)
    ids = [torch.randint(0, 32, (64, 3), generator=torch.Generator().manual_seed(43)).to(device)]
    loss = {}
    for route in ("torch", "hip"):
        netG = _net(device)
        netG.train_tokenizer = route
        with contextlib.redirect_stdout(io.StringIO()):
            netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=64, n_mlps=3)
            torch.manual_seed(9)
            netF.create_mlp([torch.zeros(1, 8, 1, 1, 1, device=device)])
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


def test_driver_with_the_tokenizer_on_hip(tmp_path, device):
    """Item 7: two iterations of ``pretrain`` at --crop_size 32 with --primus_train_tokenizer hip."""
    from anatomix_amd.pretraining import AugmentedTwoViewLoader
    from anatomix_amd.pretraining.pretrain_anatomix import build_networks, build_parser, options_from_args, pretrain
    shutil.copy(H5, tmp_path / "train_data.hdf5")
    shutil.copy(H5, tmp_path / "val_data.hdf5")
    img, lab = PR.blob_volume((32, 32, 32), 78, n_labels=4)
    val = [{"A": torch.from_numpy(img[None, None]).float(), "B": torch.from_numpy(0.8 * img[None, None] + 0.05).float(),
            "A_seg": torch.from_numpy(lab[None, None]).float()}]
    argv = ["--ckpt_dir", str(tmp_path / "ckpt"), "--name", "tok", "--dataroot", str(tmp_path), "--netG", "primus", "--primus_version", "v2",
            "--primus_config", "S", "--crop_size", "32", "--batch_size", "1", "--num_patches", "64", "--max_iters", "2", "--evaluation_freq", "2",
            "--n_epochs", "1", "--n_epochs_decay", "1", "--print_freq", "1", "--primus_train_tokenizer", "hip"]
    opt = options_from_args(build_parser(primus_route=True).parse_args(argv))
    loader = AugmentedTwoViewLoader(opt, device=device, seed=opt.loader_seed)
    loader.dataset = InMemory(2)
    calls = []
    orig = ARCH._TokenizerFn.forward

    def counted(ctx, *a):
        calls.append(1)
        return orig(ctx, *a)

    ARCH._TokenizerFn.forward = staticmethod(counted)
    try:
        out = pretrain(opt, train_loader=loader, val_loader=val)
    finally:
        ARCH._TokenizerFn.forward = staticmethod(orig)
    assert out["netG"].train_tokenizer == "hip" and len(calls) >= 2
    log = [json.loads(l) for l in open(os.path.join(out["save_dir"], "log.jsonl"))]
    train = [l for l in log if l["kind"] == "train"]
    assert [l["total_iters"] for l in train] == [1, 2] and all(np.isfinite(l["loss"]) and l["loss"] > 0 for l in train)
    fresh = build_networks(opt, torch.device("cpu"))[0]
    fresh.load_state_dict(torch.load(os.path.join(out["save_dir"], "2_net_G.pth")), strict=True)
