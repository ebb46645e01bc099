"""CPU side of the ViT's patch decoder on sampled rows (csrc/amx_vit_decode_rows.hip) and of ``--netG primus`` in the pretraining
driver: the float64 restatement of one row (tests/_decode_rows_ref.py) against the dense modules + gather, the three C entries, the
network the driver builds, and its refusals."""
import os
import re

import pytest
import torch

import _decode_rows_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d.architectures import _decode_rows_parts
from anatomix_amd.pretraining.pretrain_anatomix import build_networks, build_parser, options_from_args, pretrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"amx_vit_decode_rows_scratch_bytes": 6, "amx_vit_decode_rows_forward": 19, "amx_vit_decode_rows_backward": 21}


@pytest.mark.parametrize("out_norm", ["none", "layernorm", "layernorm_affine"])
def test_restated_row_is_the_dense_decoder_gathered(out_norm):
    """Values and every gradient (float64 autograd) on a NON-cubic grid (2, 3, 4): a swapped axis or a swapped stage bit would show."""
    grid, N, E, C = (2, 3, 4), 2, 24, 4
    dec, on = R.build_modules(E, C, out_norm, 21)
    assert R.widths_of(dec) == [24, 16, 8, 4]
    g = torch.Generator().manual_seed(22)
    tokens = torch.randn(N, 24, E, generator=g, dtype=torch.float64)
    coords = R.draw_distinct(300, (16, 24, 32), 23)
    # every (stage, offset) pair occurs, and every token
    for s in range(3):
        assert len({tuple(((c >> (2 - s)) & 1).tolist()) for c in coords}) == 8
    drows = torch.randn(N, 300, C, generator=g, dtype=torch.float64)
    dense = R.run_dense(dec, on, tokens, coords, drows, grid)
    params = R.named_params(dec, on)
    for p in params.values():
        p.grad = None
    tok = tokens.clone().requires_grad_(True)
    rows = R.rows_restated(tok, coords, params, grid, ln_eps=1e-6, out_norm=out_norm, out_eps=1e-5)
    rows.backward(drows)
    got = {"rows": rows.detach(), "d_tokens": tok.grad, **{k: v.grad for k, v in params.items()}}
    assert got.keys() == dense.keys() and len(got) == (14 if out_norm == "layernorm_affine" else 12)
    for name in dense:
        assert R.rel_l2(got[name], dense[name]) <= 1e-12, name


def test_case_table_has_the_widths_the_issue_names():
    for name, want in R.WIDTHS.items():
        E, C = R.CASES[name][:2]
        assert R.widths_of(R.build_modules(E, C, "none", 0)[0]) == want, name
    # (a): all 512 voxels of one patch + 40 elsewhere; (e): 64 coordinates twice; (f): one octant at every stage
    a = R.CASES["a_one_patch"][4]()
    assert a.shape == (552, 3) and len({tuple(c) for c in a.tolist()}) == 552
    assert ((a[:512] >> 3) == torch.tensor([1, 0, 1])).all() and not ((a[512:] >> 3) == torch.tensor([1, 0, 1])).all(1).any()
    e = R.CASES["e_repeats"][4]()
    assert e.shape == (512, 3) and len({tuple(c) for c in e.tolist()}) == 448
    f = R.CASES["f_one_octant"][4]()
    assert f.shape == (7, 3) and all(((f >> s) & 1 == torch.tensor([1, 0, 1])).all() for s in range(3))


def test_entries_are_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\(", header), name
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name), name
    # the envelope, as the header states it: patch 8, widths up to 1056, output channels up to 64
    assert lib.amx_vit_decode_rows_scratch_bytes(2, 512, 396, 168, 72, 16) > 0
    assert lib.amx_vit_decode_rows_scratch_bytes(1, 512, 1056, 328, 104, 64) > 0
    for bad in ((2, 512, 1057, 168, 72, 16), (2, 512, 396, 168, 72, 65), (0, 512, 396, 168, 72, 16), (2, 0, 396, 168, 72, 16),
                (2048, 1024, 396, 168, 72, 16)):
        assert lib.amx_vit_decode_rows_scratch_bytes(*bad) == 0, bad


def _opt(tmp_path, *argv):
    base = ["--ckpt_dir", str(tmp_path), "--netG", "primus", "--primus_version", "v2", "--primus_config", "S", "--crop_size", "32"]
    return options_from_args(build_parser(primus_route=True).parse_args(base + list(argv)))


def test_driver_builds_the_primus_of_define_G(tmp_path):
    opt = _opt(tmp_path, "--primus_out_norm", "layernorm", "--primus_num_register_tokens", "2")
    netG, netF, crits = build_networks(opt, torch.device("cpu"))
    assert isinstance(netG, PrimusV2) and netG.training
    assert len(netG.eva.blocks) == 12 and netG.eva.blocks[0].attn.num_heads == 6 and netG.eva.pos_embed.shape == (1, 64, 396)
    assert netG.up_projection.decode[-1].out_channels == 16 and netG.grid == (4, 4, 4)
    assert opt.nce_layers_list == [-1] and opt.nce_weights_list == [1.0] and len(crits) == 1
    assert netG.num_register_tokens == 2 and type(netG.out_norm).__name__ == "ChannelLayerNorm" and netG.out_norm.eps == opt.primus_v2_in_eps
    # LayerScale 0.1 and the inner attention norm (define_G); no init_weights pass: the conv biases are not zeroed
    assert torch.all(netG.eva.blocks[0].gamma_1 == 0.1) and isinstance(netG.eva.blocks[0].attn.norm, torch.nn.LayerNorm)
    assert netG.down_projection.stem.conv.bias.abs().sum() > 0
    assert netG.train_attention == "hip" and netG.train_linear == "hip"
    assert _opt(tmp_path).primus_train_route == "hip"
    torch_route = build_networks(_opt(tmp_path, "--primus_train_route", "torch"), torch.device("cpu"))[0]
    assert torch_route.train_attention == "torch" and torch_route.train_linear == "torch"
    # the stored description of the reference's flags does not see the new flag
    assert "primus_train_route" not in {a.dest for a in build_parser()._actions}


def test_sampled_route_states_why_not():
    opt_kw = dict(input_channels=1, num_classes=8, embed_dim=132, patch_embed_size=(8, 8, 8), eva_depth=1, eva_numheads=2, input_shape=(16, 16, 16))
    x = torch.zeros(1, 1, 16, 16, 16)
    assert "CPU" in PrimusV2(**opt_kw).sampled_unsupported_reason(x)
    # what decides apart from the device: the modules (the device check comes first in sampled_unsupported_reason)
    for mode, word in (("instance", "InstanceNorm3d"), ("demean", "ChannelDemean")):
        m = PrimusV2(out_norm=mode, **opt_kw)
        reason = _decode_rows_parts(m.up_projection, m.out_norm)
        assert isinstance(reason, str) and word in reason and "spatial" in reason
    wide = PrimusV2(**{**opt_kw, "num_classes": 72})
    assert "envelope" in _decode_rows_parts(wide.up_projection, wide.out_norm)
    for mode in ("none", "layernorm", "layernorm_affine"):
        m = PrimusV2(out_norm=mode, **opt_kw)
        tensors, ln_eps, code, out_eps = _decode_rows_parts(m.up_projection, m.out_norm)
        assert len(tensors) == 12 and ln_eps == 1e-6 and code == ("none", "layernorm", "layernorm_affine").index(mode)


@pytest.mark.parametrize("argv,graph,word", [(["--primus_version", "v1"], None, "v1"), (["--primus_patch_size", "16"], None, "primus_patch_size"),
                                             (["--crop_size", "36"], None, "crop_size"), (["--primus_drop_path_rate", "0.1"], None, "drop"),
                                             ([], "on", "graph")])
def test_primus_refusals_come_before_any_file(argv, graph, word, tmp_path):
    opt = _opt(tmp_path, *argv)
    if graph is not None:
        opt.graph = graph
    with pytest.raises(NotImplementedError, match=word):
        pretrain(opt)
    assert os.listdir(tmp_path) == []
