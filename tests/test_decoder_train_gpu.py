"""GPU: the ViT's dense patch decoder and the spatial output norms under autograd on the library's own kernels (``train_decoder = "hip"``:
amx_vit_decoder_train_forward + amx_vit_decoder_backward, csrc/amx_vit_decode_train.hip) against float64 CPU autograd through the real
modules (tests/_decoder_train_ref.py).

Bars.  The volume, d_tokens and every dW, db, dgamma, dbeta: 2e-5 rel-L2 against float64, the project's bar for its fp32-grade training
routes.  A gradient that is mathematically zero -- the last decoder bias in front of demean / instance -- is held to 1e-4 of the sum of the
magnitudes of its terms instead.  The ratio to fp32 torch's own error (the same modules in fp32 on the CPU) is printed, not asserted."""
import contextlib
import copy
import ctypes
import functools
import io
from argparse import Namespace

import pytest
import torch
import torch.nn as nn

import _decoder_train_ref as R
import _preaug_ref as PR
from _tokenizer_train_ref import NORMED_BIAS
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d import architectures as ARCH

pytestmark = pytest.mark.gpu
NAMES = ("out", "d_tokens", "w1", "b1", "g1", "be1", "w2", "b2", "g2", "be2", "w3", "b3")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 reference, fp32 torch's rel-L2 against it per tensor) of a case, computed once on the CPU and left unchanged."""
    dec, on, tokens, dy, grid, norm = R.case_inputs(name)
    ref = R.run_modules(dec, on, tokens, dy, grid)
    f32 = R.run_modules(copy.deepcopy(dec).float(), copy.deepcopy(on).float(), tokens.float(), dy.float(), grid)
    err = {k: R.rel_l2(f32[k], ref[k]) for k in NAMES}
    return ref, err


def hip_run(name, device, dy_scale=1.0, tokens_grad=True, params_grad=True):
    """{"out", "d_tokens", parameter names ...} of ``decode_dense`` on the case's inputs in fp32 on the device (None: not asked for)."""
    dec, on, tokens, dy, grid, norm = R.case_inputs(name)
    dec, on = copy.deepcopy(dec).float().to(device), copy.deepcopy(on).float().to(device)
    for p in dec.parameters():
        p.requires_grad_(params_grad)
    tok = tokens.float().to(device).requires_grad_(tokens_grad)
    out = ARCH.decode_dense(tok, dec, on, grid)
    assert "_DecoderFn" in type(out.grad_fn).__name__ and out.dtype == torch.float32 and out.is_contiguous()
    out.backward((dy * dy_scale).float().to(device))
    got = {"out": out.detach(), "d_tokens": tok.grad}
    got.update({k: v.grad for k, v in R.named_params(dec, None).items()})
    return got


def check(name, got, scale=1.0, label=""):
    ref, f32 = reference(name)
    norm = R.CASES[name][3]
    line = []
    for k in NAMES:
        assert got[k] is not None and torch.isfinite(got[k]).all(), (name, k)
        want = ref[k] if k == "out" else ref[k] * scale
        if k in R.ZERO_GRADS[norm]:
            rel = (got[k].double().cpu().abs() / (scale * ref["terms"])).max().item()
            line.append(f"{k} {rel:.1e} of its terms")
            assert rel <= R.ZERO_BAR, (name, k, rel)
            continue
        e = R.rel_l2(got[k], want)
        line.append(f"{k} {e:.2e} (x{e / max(f32[k], 1e-30):.2f} of fp32 torch)")
        assert e <= R.BAR, (name, k, e)
    print(f"case {name}{label}: " + ", ".join(line))


@pytest.mark.parametrize("name", list(R.CASES))
def test_cases_against_float64(name, device):
    check(name, hip_run(name, device))


@pytest.mark.parametrize("scale", [1e-8, 1e4])
def test_gradient_scaling(scale, device):
    """Case B with dy x 1e-8 and x 1e+4: the bars hold at either end (no gradient is rounded to a narrower format on the way)."""
    check("B", hip_run("B", device, dy_scale=scale), scale=scale, label=f" dy x {scale:g}")


def test_bit_identical_runs_and_skipped_outputs(device):
    full, again = hip_run("B", device), hip_run("B", device)
    assert all(torch.equal(full[k], again[k]) for k in NAMES)
    no_tok = hip_run("B", device, tokens_grad=False)
    assert no_tok["d_tokens"] is None and all(torch.equal(full[k], no_tok[k]) for k in NAMES if k != "d_tokens")
    frozen = hip_run("B", device, params_grad=False)
    assert all(frozen[k] is None for k in NAMES[2:]) and torch.equal(frozen["d_tokens"], full["d_tokens"]) and torch.equal(frozen["out"], full["out"])


KW = dict(input_channels=1, num_classes=8, embed_dim=132, patch_embed_size=(8, 8, 8), eva_depth=2, eva_numheads=2, input_shape=(32, 32, 32),
          init_values=0.1, scale_attn_inner=True, qk_norm=True, num_register_tokens=8)
LAST_BIAS = "up_projection.decode.2.bias"
# the tokenizer's conv biases in front of an InstanceNorm and the last decoder bias in front of a spatial output norm: mathematically zero
ZERO_GRAD = ["down_projection." + n for n in NORMED_BIAS] + [LAST_BIAS]


def _net(device, out_norm="demean"):
    torch.manual_seed(5)
    m = PrimusV2(out_norm=out_norm, **KW)
    with torch.no_grad():          # nothing at an initial value that would hide a missing term
        for name, p in m.up_projection.named_parameters():
            if p.dim() == 1:
                p.add_(0.2 * torch.randn(p.shape))
    return m.to(device).train()


@contextlib.contextmanager
def counted_calls():
    calls, orig = [], ARCH._DecoderFn.forward
    ARCH._DecoderFn.forward = staticmethod(lambda ctx, *a: (calls.append(a[3]), orig(ctx, *a))[1])          # a[3]: the norm mode
    try:
        yield calls
    finally:
        ARCH._DecoderFn.forward = staticmethod(orig)


def _grads_and_terms(body, model, run):
    """``run()`` -> scalar, backward; the parameter gradients of ``model`` and per ZERO_GRAD name the sum of the magnitudes of its terms
    (for the last decoder bias from the gradient of the body's output: d raw = dy - mean(dy) under demean, on either route)."""
    terms = {}

    def conv_hook(name):
        def fwd(mod, args, out):
            out.register_hook(lambda g: terms.__setitem__(name, g.abs().sum((0, 2, 3, 4))))
        return fwd

    def body_hook(mod, args, out):
        out.register_hook(lambda g: terms.__setitem__(LAST_BIAS, (g - g.mean((2, 3, 4), keepdim=True)).abs().sum((0, 2, 3, 4))))

    hooks = [body.get_submodule(n[:-len(".bias")]).register_forward_hook(conv_hook(n)) for n in ZERO_GRAD[:-1]]
    hooks.append(body.register_forward_hook(body_hook))
    value = run()
    value.backward()
    for h in hooks:
        h.remove()
    return value.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}, terms


def _compare_routes(hip, tor, prefix=""):
    worst = ("", 0.0)
    assert set(hip[1]) == set(tor[1])
    for k in tor[1]:
        if k[len(prefix):] in ZERO_GRAD:
            for val, grads, terms in (hip, tor):
                t = terms[k[len(prefix):]]
                assert t.min() > 0 and (grads[k].abs() <= 1e-4 * t).all(), k
            continue
        e = R.rel_l2(hip[1][k], tor[1][k])
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e <= 1e-4, (k, e)
    return worst


def test_wiring_through_primus(device):
    """PrimusV2 (width 132, 2 heads, depth 2, 32^3, demean), two views, loss y.square().mean(): ``train_decoder`` torch against hip with
    the other switches on torch, 1e-4 rel-L2 on y and every parameter gradient; then layernorm_affine: the decoder on HIP, the module behind."""
    g = torch.Generator().manual_seed(32)
    x = torch.randn(2, 1, 32, 32, 32, generator=g).to(device)
    probe = torch.randn(2, 8, 32, 32, 32, generator=g).to(device)
    for out_norm, mode in (("demean", 1), ("layernorm_affine", 0)):
        res = {}
        with counted_calls() as calls:
            for route in ("torch", "hip"):
                m = _net(device, out_norm)
                m.train_decoder = route
                assert (m.train_attention, m.train_linear, m.train_tokenizer, m.train_norm) == ("torch",) * 4
                assert m.decoder_unsupported_reason(x) is None
                ys = {}
                # behind a per-voxel LayerNorm y.square().mean() is all but constant (the norm fixes it up to eps), so its gradients are
                # rounding noise on either route (register_tokens: 2.8e-4 between the routes, measured); that variant takes a fixed
                # random functional of y instead
                loss_of = (lambda y: y.square().mean()) if out_norm == "demean" else (lambda y: (y * probe).mean())
                res[route] = _grads_and_terms(m, m, lambda: (ys.__setitem__("y", m(x)), loss_of(ys["y"]))[1])
                res[route + ".y"] = ys["y"].detach()
                assert calls == ([] if route == "torch" else [mode])
        e_y = R.rel_l2(res["hip.y"], res["torch.y"])
        if out_norm == "demean":
            worst = _compare_routes(res["hip"], res["torch"])
        else:          # the per-voxel norm keeps the last bias: an ordinary gradient
            worst = ("", 0.0)
            for k, gt in res["torch"][1].items():
                if k in ZERO_GRAD[:-1]:
                    continue
                e = R.rel_l2(res["hip"][1][k], gt)
                worst = max(worst, (k, e), key=lambda t: t[1])
                assert e <= 1e-4, (k, e)
            assert res["hip"][1]["out_norm.weight"].abs().max() > 0
        print(f"wiring {out_norm}: y {e_y:.2e}; worst gradient rel-L2 between the routes {worst[0]} {worst[1]:.2e}")
        assert e_y <= 1e-4
    # no_grad (the engine) does not reach the function; neither does forward_train_sampled's route
    m = _net(device)
    m.train_decoder = "hip"
    with counted_calls() as calls, torch.no_grad():
        m.eval()
        m(x)
        m.use_engine = False
        m(x)
        assert calls == []


def test_envelope_and_reasons(device):
    lib = _lib.load()
    x = torch.randn(1, 1, 32, 32, 32, device=device)
    # a two-stage decoder and a CPU tensor: a reason, and the torch modules run whatever the switch says
    m = _net(device)
    m.train_decoder = "hip"
    m.up_projection = ARCH.PatchDecode((4, 4, 4), 132, 8).to(device)
    assert "three stages" in m.decoder_unsupported_reason(x)
    with counted_calls() as calls:
        y = m(x)
        y.square().mean().backward()
        cpu = _net("cpu")
        cpu.train_decoder = "hip"
        assert "CPU" in cpu.decoder_unsupported_reason(x.cpu())
        cpu(x.cpu()).square().mean().backward()
        assert calls == [] and "_DecoderFn" not in type(y.grad_fn).__name__
    with pytest.raises(_lib.AmxEnvelopeError, match="three stages"):
        ARCH.decode_dense(torch.zeros(1, 64, 132, device=device), m.up_projection, None, (4, 4, 4))
    # the C entry names the shape: width 1060 is outside the envelope
    buf = torch.zeros(64, device=device)
    arr = (ctypes.c_void_p * 10)(*[buf.data_ptr()] * 10)
    assert lib.amx_vit_decoder_train_saved_bytes(1, 1, 1, 1, 1060, 328, 104, 16) == 0
    rc = lib.amx_vit_decoder_train_forward(_lib.ptr(buf), arr, 1, 1, 1, 1, 1060, 328, 104, 16, 1e-6, 0, 0.0, _lib.ptr(buf), _lib.ptr(buf), 256,
                                           _lib.ptr(buf), 256, _lib.stream(device))
    assert rc == _lib.AMX_ERR_SHAPE and "1060" in lib.amx_last_error().decode()
    rc = lib.amx_vit_decoder_backward(_lib.ptr(buf), None, _lib.ptr(buf), arr, _lib.ptr(buf), 256, 1, 1, 1, 1, 1060, 328, 104, 16, 1e-6, 0, 0.0,
                                      _lib.ptr(buf), arr, _lib.ptr(buf), 256, _lib.stream(device))
    assert rc == _lib.AMX_ERR_SHAPE and "1060" in lib.amx_last_error().decode()
    # a short saved buffer: refused before any launch
    sb = lib.amx_vit_decoder_train_saved_bytes(1, 1, 1, 1, 24, 16, 8, 4)
    nb = lib.amx_vit_decoder_train_scratch_bytes(1, 1, 1, 1, 24, 16, 8, 4)
    big, out = torch.zeros(max(sb, nb), dtype=torch.uint8, device=device), torch.full((4 * 512,), 7.0, device=device)
    rc = lib.amx_vit_decoder_train_forward(_lib.ptr(buf), arr, 1, 1, 1, 1, 24, 16, 8, 4, 1e-6, 0, 0.0, _lib.ptr(out), _lib.ptr(big), sb - 1, _lib.ptr(big),
                                           nb, _lib.stream(device))
    assert rc == _lib.AMX_ERR_WORKSPACE and str(sb) in lib.amx_last_error().decode()
    torch.cuda.synchronize(device)
    assert (out == 7.0).all()


def test_contrastive_step_on_both_routes(device):
    """One ``contrastive_step`` at 32^3 with 64 patches and out_norm = demean -- the rows route refuses the spatial norm, the step takes the
    dense route and ``out`` is the volume -- on both decoder routes: the losses within 1e-5 relative."""
    from anatomix_amd.pretraining import PatchSampleF, SupPatchNCELoss, contrastive_step
    g = torch.Generator().manual_seed(40)
    v = torch.randn(2, 1, 32, 32, 32, generator=g).to(device)
    seg = torch.from_numpy(PR.blob_volume((32, 32, 32), 41, n_labels=4)[1][None, None]).float().to(device)
    ids = [torch.randint(0, 32, (64, 3), generator=torch.Generator().manual_seed(43)).to(device)]
    loss = {}
    with counted_calls() as calls:
        for route in ("torch", "hip"):
            netG = _net(device)
            netG.train_decoder = route
            assert netG.sampled_unsupported_reason(v) is not None
            with contextlib.redirect_stdout(io.StringIO()):
                netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=64, n_mlps=3)
                torch.manual_seed(9)
                netF.create_mlp([torch.zeros(1, 8, 1, 1, 1, device=device)])
            netF = netF.to(device).train()
            crits = [SupPatchNCELoss(Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw"))]
            rec = contrastive_step(netG, netF, crits, v[:1], v[1:], seg, [-1], num_patches=64, sample_ids=ids)
            assert torch.is_tensor(rec["out"]) and tuple(rec["out"].shape) == (2, 8, 32, 32, 32)
            assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in netG.parameters())
            loss[route] = rec["loss"]
        assert len(calls) >= 1 and set(calls) == {1}          # the hip route alone reached the Function, with demean inside the call
    print("contrastive_step loss", loss)
    assert abs(loss["hip"] - loss["torch"]) <= 1e-5 * abs(loss["torch"])


def test_finetune_loss_on_a_vit(device):
    """``finetune_loss(Sequential(PrimusV2, Conv3d(C, 3, 1)), ...)`` with the decoder on HIP feeds the fused head + Dice/CE kernels (no
    logits); against ``loss(model(x), labels)`` on the torch route: the loss and every gradient within 1e-4."""
    from anatomix_amd.segmentation import DiceCELoss, finetune_loss
    from anatomix_amd.segmentation import losses as L
    g = torch.Generator().manual_seed(50)
    x = torch.randn(1, 1, 32, 32, 32, generator=g).to(device)
    labels = torch.from_numpy(PR.blob_volume((32, 32, 32), 51, n_labels=3)[1][None, None]).long().clamp_(0, 2).to(device)
    res = {}
    before = dict(L.CALLS)
    with counted_calls() as calls:
        for route in ("torch", "hip"):
            torch.manual_seed(6)
            head = nn.Conv3d(8, 3, 1).to(device)
            body = _net(device)
            body.train_decoder = route
            model = nn.Sequential(body, head)
            loss = DiceCELoss(softmax=True, to_onehot_y=True)
            run = (lambda: finetune_loss(model, x, labels, loss)) if route == "hip" else (lambda: loss(model(x), labels))
            res[route] = _grads_and_terms(body, model, run)
        # torch route: the loss on logits; hip route: the decoder's Function, and the head inside the loss
        assert calls == [1] and L.CALLS["logits"] == before["logits"] + 1 and L.CALLS["head"] == before["head"] + 1
    worst = _compare_routes(res["hip"], res["torch"], prefix="0.")
    rel = abs(res["hip"][0].item() - res["torch"][0].item()) / abs(res["torch"][0].item())
    print(f"finetune_loss: loss {res['hip'][0].item():.6f} / {res['torch'][0].item():.6f} ({rel:.2e}); worst gradient {worst[0]} {worst[1]:.2e}")
    assert rel <= 1e-4
