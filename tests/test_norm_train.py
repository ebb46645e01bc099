"""CPU side of the token LayerNorms under autograd (csrc/amx_layernorm_train.hip): the C entries and their envelope, the module
switch ``PrimusV2.train_norm``, the driver flag, and the closed forms of the float64 reference the GPU test uses."""
import os
import re

import pytest
import torch

import _norm_train_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from oracle import vit_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"amx_layernorm_train_scratch_bytes": 2, "amx_layernorm_train_forward": 11, "amx_layernorm_backward": 15}


def test_entries_are_exported_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\(", header), name
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name)
    assert "amx_layernorm_train" in open(os.path.join(ROOT, "anatomix_amd", "csrc", "Makefile")).read()


def test_byte_query_states_the_envelope():
    lib = _lib.load()
    q = lib.amx_layernorm_train_scratch_bytes
    for m, c in R.SHAPES + ((8192, 396), (8192, 1056), (1, 8), ((1 << 31) // 4096 - 1, 4096)):
        assert q(m, c) > 0, (m, c)
    for m, c in ((4, 6), (4, 398), (4, 4100), (0, 132), (4, 4), (-1, 132), ((1 << 31) // 4096, 4096)):
        assert q(m, c) == 0, (m, c)
    # the scratch is the per-workgroup partials of dw and db, a function of (M, C) alone, and does not grow with M without bound
    assert q(8192, 1056) == q(8192, 1056) and q(1 << 20, 396) <= 2 * q(8192, 396)
    # the entries refuse a shape outside the envelope before they look at anything else
    assert lib.amx_layernorm_train_forward(None, None, None, None, 1e-6, 4, 132, None, None, None, None) == _lib.AMX_ERR_INVALID
    assert "null" in lib.amx_last_error().decode()


def _small_vit():
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(16, 16, 16), eva_depth=2)
    return PrimusV2(**kw)


def test_train_norm_defaults_validates_and_leaves_the_other_switches():
    m = _small_vit()
    sites = lambda: [getattr(o, "train_norm") for blk in m.eva.blocks for o in (blk, blk.attn, blk.mlp)]
    assert m.train_norm == "torch" and sites() == ["torch"] * 6
    m.train_norm = "hip"
    assert m.train_norm == "hip" and sites() == ["hip"] * 6
    assert m.train_attention == "torch" and m.train_linear == "torch" and m.train_tokenizer == "torch"
    for bad in ("HIP", "fp32", None, 1):
        with pytest.raises(ValueError, match="train_norm"):
            m.train_norm = bad
    assert m.train_norm == "hip" and sites() == ["hip"] * 6
    m.train_attention = m.train_linear = m.train_tokenizer = "hip"
    assert m.train_norm == "hip"
    m.train_norm = "torch"
    assert sites() == ["torch"] * 6
    assert m.train_attention == "hip" and m.train_linear == "hip" and m.train_tokenizer == "hip"


def test_cpu_module_is_bit_equal_under_both_values():
    m = _small_vit()
    x = V.synthetic_input(12, 2, (16, 16, 16))
    out = {}
    for mode in ("torch", "hip"):
        m.train_norm = mode
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.square().mean().backward()
        out[mode] = (y.detach(), {n: p.grad.clone() for n, p in m.named_parameters()})
    assert torch.equal(out["torch"][0], out["hip"][0])
    assert all(torch.equal(g, out["hip"][1][n]) for n, g in out["torch"][1].items())
    assert any("norm" in n for n in out["hip"][1])


def test_state_dict_and_parameter_order_do_not_depend_on_the_switch():
    a, b = _small_vit(), _small_vit()
    b.train_norm = "hip"
    assert list(a.state_dict()) == list(b.state_dict())
    assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
    keys = list(b.state_dict())
    b.train_norm = "torch"
    assert list(b.state_dict()) == keys and not any("train_norm" in k for k in keys)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_closed_forms_equal_float64_autograd(case):
    ref = R.reference(case)
    got = R.closed_forms(*R.inputs(case), R.eps_of(case))
    for name in R.TENSORS:
        if ref[name] is None:
            assert got[name] is None and not case[2]
            continue
        assert got[name].shape == ref[name].shape, name
        assert R.rel_l2(got[name], ref[name]) <= 1e-12, (name, R.rel_l2(got[name], ref[name]))


def test_the_cases_have_no_degenerate_rows_and_one_plain_case_has_the_other_eps():
    assert len(R.CASES) == 14 and [R.eps_of(c) for c in R.CASES].count(1e-5) == 1 and R.eps_of((5, 396, False)) == 1e-5
    for case in R.CASES:
        x, gate = R.inputs(case)[:2]
        u = x.double() if gate is None else torch.nn.functional.silu(gate.double()) * x.double()
        assert u.std(-1).min() > 1e-2, case


def test_driver_flag_parses_and_defaults_to_torch(tmp_path):
    from anatomix_amd.pretraining.pretrain_anatomix import _refusals, build_networks, build_parser, options_from_args
    base = ["--ckpt_dir", str(tmp_path), "--name", "t", "--dataroot", str(tmp_path), "--netG", "primus", "--primus_version", "v2", "--primus_config", "S",
            "--crop_size", "16"]
    opt = lambda *argv: options_from_args(build_parser(primus_route=True).parse_args(base + list(argv)))
    assert opt().primus_train_norm == "torch" and opt().primus_train_route == "hip" and opt().primus_train_tokenizer == "torch"
    assert opt("--primus_train_norm", "hip").primus_train_norm == "hip"
    with pytest.raises(SystemExit):
        opt("--primus_train_norm", "f16")
    assert "primus_train_norm" not in {a.dest for a in build_parser()._actions}
    assert options_from_args(build_parser().parse_args(base)).primus_train_norm == "torch"
    net = build_networks(opt("--primus_train_norm", "hip"), torch.device("cpu"))[0]
    assert net.train_norm == "hip" and net.train_linear == "hip" and net.train_tokenizer == "torch"
    assert build_networks(opt(), torch.device("cpu"))[0].train_norm == "torch"
    bad = opt()
    bad.primus_train_norm = "f16"
    with pytest.raises(NotImplementedError, match="primus_train_norm"):      # the driver's refusal, as for the other two flags
        _refusals(bad)
    with pytest.raises(ValueError, match="train_norm"):
        build_networks(bad, torch.device("cpu"))
