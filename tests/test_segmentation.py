"""Host side of anatomix_amd.segmentation: the loss definition (tests/_seg_ref.py, an independent restatement of the documented
MONAI algorithm; parity with MONAI itself is unpinned) with hand-computed answers, the CPU path of DiceCELoss / DiceLoss
against it in float64, the closed-form gradient, the option surface, load_model and the C ABI listing."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import _seg_ref as SR
from anatomix_amd import _lib
from anatomix_amd.segmentation import DiceCELoss, DiceLoss, UnetOutBlock, finetune_loss, head_dice_ce, load_model, predict_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_KW = dict(softmax=True, to_onehot_y=True, include_background=False)          # train_segmentation.py:105-111


def _case(B=2, C=4, spatial=(3, 4, 5), seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((B, C) + spatial, generator=g, dtype=torch.float64) * 2
    y = torch.randint(0, C, (B, 1) + spatial, generator=g)
    return z, y


def test_uniform_logits_known_answer():
    """C = 3, all logits equal: p = 1/3 everywhere, ce = ln 3; a sample of V voxels with G_c labelled c has
    f_c = 1 - (2 G_c / 3 + nr) / (G_c + V / 3 + dr)."""
    y = torch.tensor([0, 1, 1, 2, 2, 2, 1, 0, 2, 1, 1, 0]).view(1, 1, 2, 2, 3)
    z = torch.full((1, 3, 2, 2, 3), 0.7, dtype=torch.float64)
    V, G = 12, {1: 5, 2: 4}
    want_dice = sum(1 - (2 * G[c] / 3 + 1e-5) / (G[c] + V / 3 + 1e-5) for c in (1, 2)) / 2
    for total, dice, ce in (SR.dice_ce(z, y), _module_values(DiceCELoss(**REF_KW), z, y)):
        assert abs(float(ce) - math.log(3)) < 1e-14
        assert abs(float(dice) - want_dice) < 1e-14
        assert abs(float(total) - (want_dice + math.log(3))) < 1e-14


def _module_values(mod, z, y):
    total = mod(z, y)
    return total, mod.last_components[0], mod.last_components[1]


def test_saturated_logits_stay_finite_and_give_zero():
    """Logits of +-80 that agree with the labels: p is exactly one-hot, 2 I = G + P, so every term is exactly 0."""
    _, y = _case()
    z = torch.full((2, 4, 3, 4, 5), -80.0, dtype=torch.float64).scatter_(1, y, 80.0)
    for vals in (SR.dice_ce(z, y), _module_values(DiceCELoss(**REF_KW), z, y)):
        assert [float(v) for v in vals] == [0.0, 0.0, 0.0]


def test_absent_class_known_answer():
    """A class with no voxel in a sample: I = G = 0, f = 1 - smooth_nr / (P + smooth_dr)."""
    z, y = _case(B=1, C=3)
    y[y == 2] = 1
    p2 = torch.softmax(z.reshape(1, 3, -1), 1)[0, 2].sum()
    p1 = torch.softmax(z.reshape(1, 3, -1), 1)[0, 1]
    t1 = (y.reshape(-1) == 1).double()
    f1 = 1 - (2 * (p1 * t1).sum() + 1e-5) / (t1.sum() + p1.sum() + 1e-5)
    want = (f1 + (1 - 1e-5 / (p2 + 1e-5))) / 2
    assert abs(float(SR.dice_ce(z, y)[1]) - float(want)) < 1e-14
    mod = DiceLoss(**REF_KW)
    assert abs(float(mod(z, y)) - float(want)) < 1e-14


@pytest.mark.parametrize("kw", [dict(), dict(include_background=True), dict(lambda_dice=0.3, lambda_ce=1.7),
                                dict(include_background=True, smooth_nr=1e-3, smooth_dr=2e-3, lambda_ce=0.5)])
@pytest.mark.parametrize("ldt", [torch.int64, torch.float32, torch.uint8, torch.int32, torch.float64])
def test_cpu_modules_agree_with_the_restatement(kw, ldt):
    z, y = _case()
    lab = (y.to(ldt) + 0.75) if ldt.is_floating_point else y.to(ldt)       # floating labels are truncated toward zero
    args = dict(REF_KW, **kw)
    mod = DiceCELoss(**args)
    zr = z.clone().requires_grad_(True)
    total = mod(zr, lab)
    total.backward()
    ref_kw = {k: v for k, v in args.items() if k not in ("softmax", "to_onehot_y")}
    want = SR.dice_ce(z, y, **ref_kw)
    for got, ref in zip((total, *mod.last_components), want):
        assert abs(float(got.detach()) - float(ref)) <= 1e-13 * abs(float(ref))
    assert int(mod.last_bad_labels) == 0 and total.dim() == 0
    g = SR.closed_form_grad(z, y, **ref_kw)
    assert float((zr.grad - g).abs().max()) <= 1e-13 * float(g.abs().max())
    dl = DiceLoss(**{k: v for k, v in args.items() if not k.startswith("lambda")})
    want_d = SR.dice_ce(z, y, **{k: v for k, v in ref_kw.items() if not k.startswith("lambda")})[1]
    assert abs(float(dl(z, lab)) - float(want_d)) <= 1e-13 * abs(float(want_d))


def test_cpu_bad_label_gives_nan_and_is_counted():
    z, y = _case()
    y[1, 0, 2, 3, 4] = 4
    mod = DiceCELoss(**REF_KW)
    assert math.isnan(float(mod(z, y))) and int(mod.last_bad_labels) == 1


def test_restatement_gradcheck_and_closed_form():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(1, 3, 2, 2, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randint(0, 3, (1, 1, 2, 2, 3), generator=g)
    for kw in (dict(), dict(include_background=True, lambda_dice=0.6, lambda_ce=1.3)):
        assert torch.autograd.gradcheck(lambda t: SR.dice_ce(t, y, **kw)[0], (z,), eps=1e-6, atol=1e-8)
        auto, = torch.autograd.grad(SR.dice_ce(z, y, **kw)[0], z)
        closed = SR.closed_form_grad(z.detach(), y, **kw)
        assert float((auto - closed).abs().max()) <= 1e-13 * float(auto.abs().max())


@pytest.mark.parametrize("cls", [DiceCELoss, DiceLoss])
@pytest.mark.parametrize("kw,name", [(dict(sigmoid=True), "sigmoid"), (dict(squared_pred=True), "squared_pred"),
                                     (dict(jaccard=True), "jaccard"), (dict(batch=True), "batch"),
                                     (dict(weight=torch.ones(4)), "weight"), (dict(reduction="sum"), "reduction"),
                                     (dict(reduction="none"), "reduction"), (dict(to_onehot_y=False), "to_onehot_y"),
                                     (dict(softmax=False), "softmax"), (dict(other_act=torch.tanh), "other_act")])
def test_unimplemented_monai_options_raise_and_name_the_argument(cls, kw, name):
    with pytest.raises(NotImplementedError, match=name):
        cls(**dict(REF_KW, **kw))


def test_monai_defaults_and_keyword_names():
    """MONAI's own defaults (to_onehot_y=False, softmax=False) select what is not implemented, so the reference's explicit call
    is the way to construct the losses; the keyword names are MONAI's."""
    with pytest.raises(NotImplementedError):
        DiceCELoss()
    p = inspect.signature(DiceCELoss.__init__).parameters
    assert [p[k].default for k in ("include_background", "to_onehot_y", "softmax", "reduction", "smooth_nr", "smooth_dr", "lambda_dice",
                                    "lambda_ce")] == [True, False, False, "mean", 1e-5, 1e-5, 1.0, 1.0]
    m = DiceCELoss(**REF_KW)
    assert (m.include_background, m.lambda_dice, m.lambda_ce, m.smooth_nr, m.smooth_dr) == (False, 1.0, 1.0, 1e-5, 1e-5)
    assert DiceLoss(**REF_KW).lambda_ce == 0.0


def test_load_model_signature_matches_the_reference():
    """segmentation_utils.py:36-48."""
    p = inspect.signature(load_model).parameters
    assert list(p) == ["n_classes", "device", "ckpt_path", "hf_variant", "num_downs", "ngf", "output_nc", "norm", "interp", "pooling"]
    assert [p[k].default for k in list(p)[2:]] == [None, None, 4, 16, 16, "batch", "nearest", "Max"]
    assert p["n_classes"].default is inspect.Parameter.empty and p["device"].default is inspect.Parameter.empty


def test_load_model_branches_head_and_checkpoint_keys(tmp_path):
    from anatomix_amd.registration.sliding_window import _pointwise_affine
    with pytest.raises(ValueError, match="exactly one"):
        load_model(4, "cpu")
    with pytest.raises(ValueError, match="exactly one"):
        load_model(4, "cpu", ckpt_path="a.pth", hf_variant="anatomix")
    with pytest.raises(FileNotFoundError):
        load_model(4, "cpu", ckpt_path=str(tmp_path / "missing.pth"))
    model = load_model(4, "cpu", ckpt_path="scratch", num_downs=2)
    assert isinstance(model, torch.nn.Sequential) and len(model) == 2
    import anatomix_amd
    assert isinstance(model[0], anatomix_amd.Unet) and isinstance(model[1], UnetOutBlock)
    conv = model[1].conv.conv
    assert isinstance(conv, torch.nn.Conv3d) and (conv.in_channels, conv.out_channels, conv.kernel_size) == (16, 5, (1, 1, 1))
    assert _pointwise_affine(model[1])
    keys = list(model.state_dict())
    assert all(k.startswith("0.model.") or k.startswith("1.") for k in keys)
    assert [k for k in keys if k.startswith("1.")] == ["1.conv.conv.weight", "1.conv.conv.bias"]
    # a checkpoint of the bare Unet goes through the ckpt_path branch, a finetuning checkpoint loads into the composition
    path = tmp_path / "unet.pth"
    torch.save({"_orig_mod." + k: v for k, v in model[0].state_dict().items()}, path)
    again = load_model(4, "cpu", ckpt_path=str(path), num_downs=2)
    assert torch.equal(again[0].model[0].weight, model[0].model[0].weight)
    again.load_state_dict(model.state_dict(), strict=True)


def test_structural_routing_on_the_host():
    """finetune_loss on a CPU model is the plain composition; head_dice_ce refuses what is not one 1x1x1 convolution."""
    from anatomix_amd.segmentation.losses import _single_conv_head
    head = UnetOutBlock(3, 16, 5)
    assert _single_conv_head(head) is head.conv.conv
    assert _single_conv_head(torch.nn.Conv3d(16, 5, 1)) is not None
    assert _single_conv_head(torch.nn.Sequential(head, torch.nn.ReLU())) is None
    assert _single_conv_head(torch.nn.Sequential(torch.nn.Conv3d(16, 8, 1), torch.nn.Conv3d(8, 5, 1))) is None
    assert _single_conv_head(torch.nn.Conv3d(16, 5, 3, padding=1)) is None
    loss = DiceCELoss(**REF_KW)
    with pytest.raises(ValueError, match="one 1x1x1"):
        head_dice_ce(torch.zeros(1, 16, 2, 2, 2), torch.nn.Sequential(head, torch.nn.ReLU()), torch.zeros(1, 1, 2, 2, 2), loss)
    model = torch.nn.Sequential(torch.nn.Conv3d(1, 16, 1), head).double()
    x, y = torch.randn(1, 1, 2, 3, 4, dtype=torch.float64), torch.randint(0, 5, (1, 1, 2, 3, 4))
    assert float(finetune_loss(model, x, y, loss).detach()) == float(loss(model(x), y).detach())


def test_predict_labels_on_the_host_first_maximum_wins():
    z, _ = _case()
    z[0, 1, 0, 0, 0] = z[0, 3, 0, 0, 0] = 50.0
    out = predict_labels(z)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 1, 3, 4, 5) and int(out[0, 0, 0, 0, 0]) == 1
    assert torch.equal(out.long(), z.argmax(1, keepdim=True))
    head = UnetOutBlock(3, 4, 3).double()
    assert torch.equal(predict_labels(z, head).long(), head(z).argmax(1, keepdim=True))


def test_header_and_symbols_list_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    for name in ("amx_seg_loss_scratch_bytes", "amx_seg_loss_forward", "amx_seg_loss_backward", "amx_seg_argmax"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SYMBOLS
    assert "train_segmentation.py:105-107" in hdr and "train_segmentation.py:84-86" in hdr
    lib = _lib.load()
    assert lib.amx_seg_loss_scratch_bytes(4, 128 ** 3, 5, 16) > 0
    assert lib.amx_seg_loss_scratch_bytes(4, 128 ** 3, 33, 16) == 0 and lib.amx_seg_loss_scratch_bytes(4, 128 ** 3, 5, 65) == 0
    # argument checks come before any launch: no device is needed to see them
    assert lib.amx_seg_argmax(None, 0, None, None, 1, 5, 8, None, None) == _lib.AMX_ERR_INVALID
    buf = (np.zeros(8, np.float32)).ctypes.data
    assert lib.amx_seg_argmax(buf, 0, None, None, 1, 33, 8, buf, None) == _lib.AMX_ERR_INVALID
    assert b"classes <= 32" in lib.amx_last_error()
    assert lib.amx_seg_argmax(buf, 65, buf, None, 1, 5, 8, buf, None) == _lib.AMX_ERR_INVALID
    assert b"feat <= 64" in lib.amx_last_error()
