"""CPU side of the ViT's dense patch decoder under autograd (``PrimusV2.train_decoder``, csrc/amx_vit_decode_train.hip): the nested-order
restatement of tests/_decoder_train_ref.py against the real modules in float64, the switch, its reasons, the C entries, the driver's
flag and ``finetune_loss`` on a ViT."""
import os
import re

import pytest
import torch
import torch.nn as nn

import _decoder_train_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d import architectures as ARCH
from anatomix_amd.pretraining.pretrain_anatomix import build_networks, build_parser, options_from_args, pretrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"amx_vit_decoder_train_saved_bytes": 8, "amx_vit_decoder_train_scratch_bytes": 8, "amx_vit_decoder_train_forward": 19,
           "amx_vit_decoder_backward": 22}
KW = dict(input_channels=1, num_classes=8, embed_dim=132, patch_embed_size=(8, 8, 8), eva_depth=1, eva_numheads=2, input_shape=(16, 16, 16))


@pytest.mark.parametrize("norm", ["none", "demean", "instance"])
def test_nested_restatement_is_the_modules(norm):
    """Values and every gradient in float64 on a NON-cubic grid (2, 3, 4) with two views: a swapped axis, a swapped stage bit or a wrong
    un-nest would show."""
    grid, n, widths = (2, 3, 4), 2, [24, 16, 8, 4]
    dec, on = R.build_modules(widths, norm, 31)
    assert R.widths_of(dec) == widths
    g = torch.Generator().manual_seed(32)
    tokens = torch.randn(n, 24, widths[0], generator=g, dtype=torch.float64)
    dy = torch.randn(n, widths[3], 16, 24, 32, generator=g, dtype=torch.float64)
    ref = R.run_modules(dec, on, tokens, dy, grid)
    params = R.named_params(dec, None)
    for p in params.values():
        p.grad = None
    tok = tokens.clone().requires_grad_(True)
    out = R.nested_restated(tok, params, grid, norm)
    out.backward(dy)
    got = {"out": out.detach(), "d_tokens": tok.grad, **{k: v.grad for k, v in params.items()}}
    assert len(got) == 12 and set(got) | {"terms"} == set(ref)
    for name, value in got.items():
        if name in R.ZERO_GRADS[norm]:
            assert (value.abs() <= 1e-12 * ref["terms"]).all() and (ref[name].abs() <= 1e-12 * ref["terms"]).all(), name
        else:
            assert R.rel_l2(value, ref[name]) <= 1e-12, name


def test_case_table_has_the_widths_the_issue_names():
    for name, (widths, n, grid, norm) in R.CASES.items():
        dec, on = R.build_modules(widths, norm, 0)
        assert R.widths_of(dec) == widths and ARCH._decoder_train_parts(dec, on)[2] == ARCH._DECODER_NORM_MODES[norm], name
    assert [R.CASES[k][0] for k in "ABD"] == [[24, 16, 8, 4], [396, 168, 72, 16], [1056, 328, 104, 16]]
    assert R.CASES["E"][0][3] == 12 and R.CASES["E"][1] == 3 and len(set(R.CASES["B"][2])) == 3


def test_switch_default_validation_and_independence():
    m = PrimusV2(**KW)
    assert m.train_decoder == "torch"
    m.train_decoder = "hip"
    assert m.train_decoder == "hip"
    assert (m.train_attention, m.train_linear, m.train_tokenizer, m.train_norm) == ("torch",) * 4
    m.train_attention = m.train_linear = m.train_tokenizer = m.train_norm = "hip"
    m.train_decoder = "torch"
    assert m.train_decoder == "torch" and m.train_norm == "hip"
    with pytest.raises(ValueError, match="train_decoder"):
        m.train_decoder = "f16"
    assert m.train_decoder == "torch"


def test_reasons_and_the_cpu_path():
    x = torch.rand(1, 1, 16, 16, 16)
    for norm in ("none", "demean", "instance", "layernorm", "layernorm_affine"):
        m = PrimusV2(out_norm=norm, **KW)
        assert "CPU" in m.decoder_unsupported_reason(x)
        # what decides apart from the device: no output norm is a reason, and the per-voxel ones stay modules behind the call
        tensors, ln_eps, mode, out_eps, tail = ARCH._decoder_train_parts(m.up_projection, m.out_norm)
        assert len(tensors) == 10 and ln_eps == 1e-6
        assert mode == {"demean": 1, "instance": 2}.get(norm, 0) and (tail is m.out_norm) == norm.startswith("layernorm")
    two = nn.Module()
    two.decode = nn.Sequential(nn.Sequential(nn.ConvTranspose3d(8, 8, 2, stride=2), ARCH.LayerNormNd(8), nn.GELU()), nn.ConvTranspose3d(8, 4, 2, stride=2))
    assert "three stages" in ARCH._decoder_train_parts(two, None)
    # on the CPU the switch changes nothing: the modules run, bit for bit
    m = PrimusV2(out_norm="demean", **KW)
    y0 = m(x)
    m.train_decoder = "hip"
    y1 = m(x)
    assert torch.equal(y0, y1) and "_DecoderFn" not in type(y1.grad_fn).__name__


def test_entries_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\(", header), name
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), name
    assert "amx_vit_decoder_train_forward" in integration and "amx_vit_decoder_backward" in integration
    assert "amx_vit_decode_train" in open(os.path.join(ROOT, "anatomix_amd", "csrc", "Makefile")).read()
    # the envelope, as the header states it
    for size in (lib.amx_vit_decoder_train_saved_bytes, lib.amx_vit_decoder_train_scratch_bytes):
        assert size(2, 16, 16, 16, 396, 168, 72, 16) > 0            # PrimusV2-S, two views of 128^3
        assert size(1, 1, 1, 1, 1056, 328, 104, 128) > 0 and size(3, 1, 5, 7, 24, 16, 8, 1) > 0
        for bad in ((2, 16, 16, 16, 1060, 168, 72, 16), (2, 16, 16, 16, 396, 332, 72, 16), (2, 16, 16, 16, 396, 168, 108, 16),
                    (2, 16, 16, 16, 396, 168, 72, 129), (2, 16, 16, 16, 396, 168, 72, 0), (2, 16, 16, 16, 398, 168, 72, 16),
                    (0, 16, 16, 16, 396, 168, 72, 16), (2, 0, 16, 16, 396, 168, 72, 16), (64, 64, 64, 64, 396, 168, 72, 16)):
            assert size(*bad) == 0, bad
    # the saved state is what the issue counts: a_1 and a_2 in fp32 plus two floats per row and per (n, c)
    r0 = 2 * 4096
    assert lib.amx_vit_decoder_train_saved_bytes(2, 16, 16, 16, 396, 168, 72, 16) == 4 * (8 * r0 * 168 + 64 * r0 * 72 + 2 * 72 * r0 + 2 * 32)


def _opt(tmp_path, *argv):
    base = ["--ckpt_dir", str(tmp_path), "--netG", "primus", "--primus_version", "v2", "--primus_config", "S", "--crop_size", "32"]
    return options_from_args(build_parser(primus_route=True).parse_args(base + list(argv)))


def test_driver_flag(tmp_path):
    assert _opt(tmp_path).primus_train_decoder == "torch"
    assert _opt(tmp_path, "--primus_train_decoder", "hip").primus_train_decoder == "hip"
    with pytest.raises(SystemExit):
        _opt(tmp_path, "--primus_train_decoder", "f16")
    assert "primus_train_decoder" not in {a.dest for a in build_parser()._actions}
    base = ["--ckpt_dir", str(tmp_path), "--netG", "primus", "--primus_version", "v2", "--crop_size", "32"]
    assert options_from_args(build_parser().parse_args(base)).primus_train_decoder == "torch"
    net = build_networks(_opt(tmp_path, "--primus_train_decoder", "hip", "--primus_out_norm", "demean"), torch.device("cpu"))[0]
    assert net.train_decoder == "hip" and net.train_tokenizer == "torch" and net.train_norm == "torch"
    assert build_networks(_opt(tmp_path), torch.device("cpu"))[0].train_decoder == "torch"
    bad = _opt(tmp_path)
    bad.primus_train_decoder = "f16"
    with pytest.raises(NotImplementedError, match="primus_train_decoder"):
        pretrain(bad)


def test_finetune_loss_on_the_cpu_is_the_plain_composition():
    from anatomix_amd.segmentation import DiceCELoss, finetune_loss
    torch.manual_seed(3)
    body = PrimusV2(out_norm="demean", **KW)
    body.train_decoder = "hip"
    model = nn.Sequential(body, nn.Conv3d(8, 3, 1))
    x = torch.rand(1, 1, 16, 16, 16)
    labels = torch.randint(0, 3, (1, 1, 16, 16, 16))
    loss = DiceCELoss(softmax=True, to_onehot_y=True)
    a = finetune_loss(model, x, labels, loss)
    assert float(a.detach()) == float(loss(model(x), labels).detach())
    a.backward()
    assert all(p.grad is not None for p in model.parameters())
