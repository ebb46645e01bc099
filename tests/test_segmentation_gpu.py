"""GPU: the segmentation head + Dice/CE loss, its backward and the arg-max (csrc/amx_segloss.hip) through
anatomix_amd.segmentation, against the float64 restatement on the CPU (tests/_seg_ref.py; parity with MONAI is unpinned).

Bounds.  Loss, Dice and CE: (5e-6 + 10 x e32) x |ref64|; each gradient tensor: (5e-6 + 10 x e32) x max|ref64|, where ref64 is
the float64 restatement and e32 the fp32 CPU restatement's own distance from float64 for that quantity, computed here.  No
bound comes from the code under test.  Every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest
import torch

import _seg_ref as SR

pytestmark = pytest.mark.gpu

# (B, F, C, D, H, W): V = 105 (odd vector tail, less than one workgroup, C = 2 with its only foreground class absent in sample 0);
# several workgroups with a ragged end at the reference's C; the envelope's C with the dev variant's F; F no multiple of 4 or 8;
# the envelope's F
SHAPES = [(1, 16, 2, 5, 3, 7), (3, 16, 5, 17, 16, 19), (2, 32, 32, 8, 8, 8), (2, 12, 3, 4, 4, 6), (2, 64, 2, 4, 4, 4)]
LABEL_DTYPES = [torch.float32, torch.int64, torch.uint8]
REF_KW = dict(softmax=True, to_onehot_y=True, include_background=False)


def dev():
    return torch.device("cuda:0")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b)) if float(b) != 0.0 else abs(float(a))


def _relmax(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@functools.lru_cache(maxsize=None)
def reference(shape, head, include_background=False, lambda_ce=1.0):
    """Inputs (numpy) and, from the restatement on the CPU, computed once and left unchanged: the float64 values and
    gradients, and the fp32 restatement's distance from them (e32) per quantity."""
    B, F, C = shape[:3]
    x, w, b, y, z = SR.make_inputs(B, F, C, shape[3:])
    kw = dict(include_background=include_background, lambda_ce=lambda_ce)
    out = {}
    for dt in (torch.float64, torch.float32):
        yt = torch.from_numpy(y)
        if head:
            leaves = [torch.from_numpy(a).to(dt).requires_grad_(True) for a in (x, w, b)]
            logits = SR.head_logits(*leaves)
        else:
            leaves = [torch.from_numpy(z).to(dt).requires_grad_(True)]
            logits = leaves[0]
        vals = SR.dice_ce(logits, yt, **kw)
        grads = torch.autograd.grad(vals[0], leaves)
        out[dt] = ([v.detach() for v in vals], list(grads), logits.detach())
    v64, g64, logits64 = out[torch.float64]
    v32, g32, _ = out[torch.float32]
    e_vals = [_rel(a, r) for a, r in zip(v32, v64)]
    e_grads = [_relmax(a, r) for a, r in zip(g32, g64)]
    return dict(x=x, w=w, b=b, y=y, z=z, vals=v64, grads=g64, e_vals=e_vals, e_grads=e_grads, logits=logits64)


def _loss(include_background=False, dice_only=False, **kw):
    from anatomix_amd.segmentation import DiceCELoss, DiceLoss
    args = dict(REF_KW, include_background=include_background, **kw)
    return DiceLoss(**args) if dice_only else DiceCELoss(**args)


def _head(F, C, w, b):
    from anatomix_amd.segmentation import UnetOutBlock
    head = UnetOutBlock(3, F, C).to(dev())
    with torch.no_grad():
        head.conv.conv.weight.copy_(cu(w).view(C, F, 1, 1, 1))
        head.conv.conv.bias.copy_(cu(b))
    return head


def _run(ref, shape, head, ldt, loss, upstream=1.0, x_dev=None):
    """One forward + backward on the GPU -> (values [total, dice, ce], gradients in the reference's order, bad label count)."""
    from anatomix_amd.segmentation import head_dice_ce
    B, F, C = shape[:3]
    lab = cu(ref["y"]).to(ldt)
    lab_keep = lab.clone()
    if head:
        x = (cu(ref["x"]) if x_dev is None else x_dev).requires_grad_(True)
        mod = _head(F, C, ref["w"], ref["b"])
        leaves = [x, mod.conv.conv.weight, mod.conv.conv.bias]
        keep = [t.detach().clone() for t in leaves]
        total = head_dice_ce(x, mod, lab, loss)
    else:
        x = (cu(ref["z"]) if x_dev is None else x_dev).requires_grad_(True)
        leaves = [x]
        keep = [x.detach().clone()]
        total = loss(x, lab)
    assert total.dim() == 0 and total.is_cuda and total.dtype == torch.float32
    (total * upstream).backward()
    for t, k in zip(leaves, keep):
        assert torch.equal(t.detach(), k), "an input was modified"
    assert torch.equal(lab, lab_keep)
    grads = [t.grad.reshape(g.shape) for t, g in zip(leaves, ref["grads"])]
    return [total.detach(), *loss.last_components], grads, loss.last_bad_labels


def _check(tag, ref, vals, grads, upstream=1.0, gnames=None):
    names = ["loss", "dice", "ce"]
    fails = []
    for nm, got, want, e32 in zip(names, vals, ref["vals"], ref["e_vals"]):
        err, bound = _rel(got, want), 5e-6 + 10 * e32
        print(f"{tag} {nm}: got {float(got):.9e} ref64 {float(want):.9e} rel err {err:.3e} bound {bound:.3e} (e32 {e32:.2e})")
        if not err <= bound:
            fails.append(nm)
    gnames = gnames or (["dx", "dW", "db"] if len(grads) == 3 else ["dz"])
    assert len(gnames) >= len(grads) and len(ref["grads"]) >= len(grads)
    for nm, got, want, e32 in zip(gnames, grads, ref["grads"], ref["e_grads"]):
        err, bound = _relmax(got, want * upstream), 5e-6 + 10 * e32
        print(f"{tag} {nm}: max err / max|ref64| {err:.3e} bound {bound:.3e} (e32 {e32:.2e})")
        if not err <= bound:
            fails.append(nm)
    assert not fails, fails


@pytest.mark.parametrize("ldt", LABEL_DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("head", [True, False], ids=["head", "logits"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradients_against_the_float64_restatement(shape, head, ldt):
    ref = reference(shape, head)
    loss = _loss()
    vals, grads, bad = _run(ref, shape, head, ldt, loss)
    _check(f"{shape} {'head' if head else 'logits'} {ldt}", ref, vals, grads)
    assert int(bad) == 0
    vals2, grads2, _ = _run(ref, shape, head, ldt, loss)
    assert all(torch.equal(a, b) for a, b in zip(vals + grads, vals2 + grads2)), "two calls differ"


@pytest.mark.parametrize("head", [True, False], ids=["head", "logits"])
def test_upstream_gradient_scales_all_gradients(head):
    shape = SHAPES[1]
    ref = reference(shape, head)
    vals, grads, _ = _run(ref, shape, head, torch.int64, _loss(), upstream=0.37)
    _check(f"{shape} upstream 0.37", ref, vals, grads, upstream=0.37)


@pytest.mark.parametrize("head", [True, False], ids=["head", "logits"])
@pytest.mark.parametrize("variant", ["include_background", "dice_only"])
def test_include_background_and_dice_loss(head, variant):
    shape = SHAPES[1]
    if variant == "include_background":
        ref, loss = reference(shape, head, include_background=True), _loss(include_background=True)
    else:
        ref, loss = reference(shape, head, lambda_ce=0.0), _loss(dice_only=True)
    vals, grads, _ = _run(ref, shape, head, torch.int64, loss)
    if variant == "dice_only":
        print(f"DiceLoss: ce component {float(vals[2])} (skipped)")
        assert float(vals[2]) == 0.0
        ref = dict(ref, vals=ref["vals"][:2], e_vals=ref["e_vals"][:2])
        vals = vals[:2]
    _check(f"{shape} {variant}", ref, vals, grads)


@pytest.mark.parametrize("head", [True, False], ids=["head", "logits"])
def test_unaligned_base_and_non_contiguous_input(head):
    """The input one element into a larger buffer (a contiguous tensor whose base is not 16-byte aligned), and the same values
    as a non-contiguous view, which the wrapper must make contiguous rather than misread."""
    shape = (2, 16, 5, 4, 4, 8)
    ref = reference(shape, head)
    src = cu(ref["x"] if head else ref["z"])
    buf = torch.empty(src.numel() + 1, dtype=torch.float32, device=dev())
    buf[1:].copy_(src.reshape(-1))
    off = buf[1:].view(src.shape)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    vals, grads, _ = _run(ref, shape, head, torch.int64, _loss(), x_dev=off.detach())
    _check(f"{shape} unaligned", ref, vals, grads)
    nc = src.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    assert not nc.is_contiguous()
    vals, grads, _ = _run(ref, shape, head, torch.int64, _loss(), x_dev=nc.detach())
    _check(f"{shape} non-contiguous", ref, vals, grads)


def test_saturated_logits_give_the_restatements_zero():
    B, C, sp = 2, 5, (6, 5, 7)
    y = torch.from_numpy(SR.make_inputs(B, 1, C, sp)[3])
    z = torch.full((B, C) + sp, -80.0).scatter_(1, y, 80.0)
    want = SR.dice_ce(z.double(), y)
    loss = _loss()
    zd = z.to(dev()).requires_grad_(True)
    total = loss(zd, y.to(dev()))
    total.backward()
    got = [total.detach(), *loss.last_components]
    print("saturated: got", [float(v) for v in got], "ref64", [float(v) for v in want])
    assert all(torch.isfinite(v) for v in got) and torch.isfinite(zd.grad).all()
    assert [float(v) for v in got] == [float(v) for v in want] == [0.0, 0.0, 0.0]


def test_bad_label_gives_nan_and_the_next_call_is_clean():
    shape = SHAPES[1]
    ref = reference(shape, True)
    B, F, C = shape[:3]
    from anatomix_amd.segmentation import head_dice_ce
    loss = _loss()
    x, head = cu(ref["x"]), _head(F, C, ref["w"], ref["b"])
    lab = cu(ref["y"])
    bad_lab = lab.clone()
    bad_lab[1, 0, 3, 2, 1] = C
    keep = x.clone()
    total = head_dice_ce(x, head, bad_lab, loss)
    print("bad label: loss", float(total.detach()), "components", [float(v) for v in loss.last_components], "count", int(loss.last_bad_labels))
    assert torch.isnan(total) and all(torch.isnan(v) for v in loss.last_components) and int(loss.last_bad_labels) == 1
    assert torch.equal(x, keep)
    total = head_dice_ce(x, head, lab, loss)
    _check("after a bad label", ref, [total.detach(), *loss.last_components], [])
    assert int(loss.last_bad_labels) == 0


@pytest.mark.parametrize("head", [True, False], ids=["head", "logits"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_predict_labels_is_the_argmax_of_the_logits(shape, head):
    from anatomix_amd.segmentation import predict_labels
    ref = reference(shape, head)
    B, F, C = shape[:3]
    z64 = ref["logits"]
    top2 = z64.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) >= 1e-4 * float(z64.abs().max())
    want = z64.argmax(1)
    src = cu(ref["x"] if head else ref["z"])
    keep = src.clone()
    got = predict_labels(src, _head(F, C, ref["w"], ref["b"])) if head else predict_labels(src)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 1) + tuple(shape[3:]) and torch.equal(src, keep)
    excluded = 1.0 - float(sure.double().mean())
    wrong = int((got[:, 0].cpu().long() != want)[sure].sum())
    print(f"predict_labels {shape} {'head' if head else 'logits'}: {wrong} wrong of {int(sure.sum())}, {100 * excluded:.3f} % excluded by the margin")
    assert excluded <= 0.005 and wrong == 0


def test_predict_labels_ties_pick_the_lowest_index():
    from anatomix_amd.segmentation import predict_labels
    z = torch.zeros(1, 5, 3, 5, 7)
    z[:, 2] = 1.0
    z[:, 4] = 1.0                      # classes 2 and 4 tie everywhere (105 voxels: the scalar path)
    assert bool((predict_labels(z.to(dev())) == 2).all())
    z = torch.zeros(2, 32, 4, 4, 8)    # every class ties (the 16-byte path)
    assert bool((predict_labels(z.to(dev())) == 0).all())
    from anatomix_amd.segmentation import UnetOutBlock
    head = UnetOutBlock(3, 4, 3).to(dev())
    with torch.no_grad():
        head.conv.conv.weight.zero_()
        head.conv.conv.bias.copy_(torch.tensor([0.5, 2.0, 2.0]))
    assert bool((predict_labels(torch.randn(1, 4, 2, 2, 4, device=dev()), head) == 1).all())


def test_outside_the_envelope_raises_before_any_launch():
    from anatomix_amd._lib import AmxEnvelopeError
    from anatomix_amd.segmentation import UnetOutBlock, head_dice_ce, predict_labels
    loss = _loss()
    y = torch.zeros(1, 1, 2, 2, 4, device=dev())
    for C in (33, 1):
        with pytest.raises(AmxEnvelopeError, match="classes"):
            loss(torch.zeros(1, C, 2, 2, 4, device=dev()), y)
        with pytest.raises(AmxEnvelopeError, match="classes"):
            predict_labels(torch.zeros(1, C, 2, 2, 4, device=dev()))
    with pytest.raises(AmxEnvelopeError, match="64"):
        head_dice_ce(torch.zeros(1, 65, 2, 2, 4, device=dev()), UnetOutBlock(3, 65, 3).to(dev()), y, loss)


def test_finetuning_end_to_end():
    """nn.Sequential(Unet, head) through finetune_loss against loss(model(x), labels) from identical parameters: the first
    step's loss and the head's gradients (the restatement applied to the UNet output captured by a forward hook), a gradient
    on every UNet parameter, six Adam steps that lower the loss, and the routing."""
    import copy
    import anatomix_amd
    from anatomix_amd.segmentation import UnetOutBlock, finetune_loss
    from anatomix_amd.segmentation import losses as L
    from oracle import unet_ref as R
    KW = R.VARIANTS["anatomix"]
    torch.manual_seed(0)
    net = anatomix_amd.Unet(**KW)
    net.load_state_dict(R.synthetic_state_dict(KW, 1, gain=2 ** 0.5), strict=True)
    net.precision = "bf16"
    model = torch.nn.Sequential(net, UnetOutBlock(3, 16, 4)).to(dev()).train()
    plain = copy.deepcopy(model)
    x = R.synthetic_input(3, 2, (32, 32, 64)).to(dev())
    labels = (x * 3.999).long().clamp(0, 3)                                # [2, 1, 32, 32, 64], derived from the input
    loss = _loss()
    captured = []
    hook = model[0].register_forward_hook(lambda m, i, o: captured.append(o.detach()))
    before = dict(L.CALLS)
    fused = finetune_loss(model, x, labels, loss)
    hook.remove()
    assert L.CALLS["head"] == before["head"] + 1 and L.CALLS["logits"] == before["logits"], "the fused Function did not run"
    fused.backward()
    hook = plain[0].register_forward_hook(lambda m, i, o: captured.append(o.detach()))
    unfused = loss(plain(x), labels)
    hook.remove()
    unfused.backward()
    assert L.CALLS["logits"] == before["logits"] + 1
    # the restatement on the captured UNet output
    feats = captured[0].double().cpu()
    out = {}
    for dt in (torch.float64, torch.float32):
        w = model[1].conv.conv.weight.detach().cpu().to(dt).view(4, 16).requires_grad_(True)
        b = model[1].conv.conv.bias.detach().cpu().to(dt).requires_grad_(True)
        val = SR.dice_ce(SR.head_logits(feats.to(dt), w, b), labels.cpu())[0]
        out[dt] = (val.detach(), *torch.autograd.grad(val, (w, b)))
    ref = dict(vals=[out[torch.float64][0]], e_vals=[_rel(out[torch.float32][0], out[torch.float64][0])],
               grads=list(out[torch.float64][1:]), e_grads=[_relmax(a, r) for a, r in zip(out[torch.float32][1:], out[torch.float64][1:])])
    conv = model[1].conv.conv
    _check("end to end, fused", ref, [fused.detach()], [conv.weight.grad.view(4, 16), conv.bias.grad], gnames=["dW", "db"])
    print(f"end to end: fused {float(fused):.9e} unfused {float(unfused):.9e}")
    pconv = plain[1].conv.conv
    want_plain = SR.dice_ce(SR.head_logits(captured[1].double().cpu(), pconv.weight.detach().double().cpu().view(4, 16),
                                           pconv.bias.detach().double().cpu()), labels.cpu())[0]
    print(f"end to end: unfused against the restatement on its own UNet output: rel err {_rel(unfused, want_plain):.3e}")
    assert _rel(unfused, want_plain) <= 5e-6 + 10 * ref["e_vals"][0]
    for nm, a, b, e32 in (("dW", conv.weight.grad, pconv.weight.grad, ref["e_grads"][0]), ("db", conv.bias.grad, pconv.bias.grad, ref["e_grads"][1])):
        print(f"end to end: fused against unfused {nm}: {_relmax(a, b):.3e}")
        assert _relmax(a, b) <= 2 * (5e-6 + 10 * e32)          # each side is within the bound of the restatement
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model[0].parameters())
    # training through the fused route
    opt = torch.optim.Adam(model.parameters(), lr=2e-4 * 10)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        v = finetune_loss(model, x, labels, loss)
        v.backward()
        opt.step()
        losses.append(v.detach())
    losses = [float(v) for v in losses]
    print("six Adam steps through finetune_loss:", [f"{v:.5f}" for v in losses])
    assert losses[-1] < losses[0]
    # a head with anything else in it takes the unfused route
    wrapped = torch.nn.Sequential(model[0], torch.nn.Sequential(model[1], torch.nn.ReLU()))
    before = dict(L.CALLS)
    finetune_loss(wrapped, x, labels, loss)
    assert L.CALLS["head"] == before["head"] and L.CALLS["logits"] == before["logits"] + 1
