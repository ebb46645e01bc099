"""CPU side of the conv tokenizer under autograd (csrc/amx_tokenizer_bwd.hip): the float64 restatement the GPU test uses, the C
entries and their envelope, the module switch, the driver flag, and the register budget of the new MFMA kernels."""
import os
import re
import sys

import pytest
import torch

import _tokenizer_train_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d.architectures import PatchEmbedDeeper
from oracle import vit_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"amx_tokenizer_train_saved_bytes": 4, "amx_tokenizer_train_scratch_bytes": 4, "amx_tokenizer_train_forward": 13,
           "amx_tokenizer_backward": 13, "amx_tokenizer_train_export": 7, "amx_tokenizer_train_route": 6}


def test_restatement_equals_float64_autograd_of_the_stock_modules():
    """Free masks, a non-cubic 16 x 32 x 48 input: h3 and all 37 gradients to 1e-12."""
    p = R.parameters(2)
    x, d_h3 = R.inputs((2, (16, 32, 48)), seed=2)
    ref = R.reference(x, p, d_h3)
    tok = PatchEmbedDeeper(1, 132, 32, (1, 1, 1), R.EPS)
    tok.load_state_dict(dict(p, **{"proj.weight": tok.proj.weight, "proj.bias": tok.proj.bias}))
    tok = tok.double()
    h3 = tok.stages(tok.stem(x.double()))
    h3.backward(d_h3.double())
    assert R.rel_l2(ref["h3"], h3) <= 1e-12
    got = dict(tok.named_parameters())
    assert len(R.NAMES) == 37 and [n for n in got if not n.startswith("proj")] == R.NAMES == [n for n in ref["grads"]]
    assert [id(t) for t in tok.tensors()] == [id(got[n]) for n in R.NAMES]
    for name in R.NAMES:
        g, want = ref["grads"][name], got[name].grad
        if name in R.NORMED_BIAS:                       # mathematically zero: both are rounding noise
            assert g.abs().max() <= 1e-12 * ref["draw_abs"][name].max()
            continue
        assert R.rel_l2(g, want) <= 1e-12, name
    # forcing the network's own masks changes nothing; the parameters have their awkward norm weights
    forced = R.reference(x, p, d_h3, masks=ref["masks"])
    assert all(torch.equal(forced["grads"][n], ref["grads"][n]) for n in R.NAMES)
    for name in R.NAMES:
        if "norm" in name and name.endswith("weight"):
            assert (p[name] == 0).sum() == 1 and (p[name] < 0).any()


def test_entries_are_exported_declared_and_listed():
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\(", header), name
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
        assert hasattr(lib, name)


def test_byte_queries_state_the_envelope():
    lib = _lib.load()
    both = lambda *a: (lib.amx_tokenizer_train_saved_bytes(*a), lib.amx_tokenizer_train_scratch_bytes(*a))
    for inside in ((2, 32, 32, 32), (1, 16, 32, 64), (3, 64, 32, 16), (2, 128, 128, 128)):
        s, b = both(*inside)
        assert s > 0 and b > 0, inside
    s, b = both(2, 128, 128, 128)
    print("2 x 128^3: saved %.1f MB, scratch %.1f MB" % (s / 1e6, b / 1e6))
    outside = {"W = 24": (2, 32, 32, 24), "odd D / 2": (2, 34, 32, 32), "odd D / 4": (2, 36, 32, 32), "60 tokens": (1, 24, 40, 32),
               "n = 0": (0, 32, 32, 32), "more than 2^22 voxels": (3, 128, 128, 128)}
    for why, dims in outside.items():
        assert both(*dims) == (0, 0), why
    # the entries refuse the same shapes before they look at a pointer
    assert lib.amx_tokenizer_train_forward(None, None, 2, 32, 32, 24, 1e-5, None, None, 0, None, 0, None) == _lib.AMX_ERR_SHAPE
    assert lib.amx_tokenizer_backward(None, None, None, None, 1, 24, 40, 32, 1e-5, None, None, 0, None) == _lib.AMX_ERR_SHAPE


def _small_vit():
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(16, 16, 16), eva_depth=2)
    return PrimusV2(**kw)


def test_train_tokenizer_defaults_validates_and_leaves_the_other_switches():
    m = _small_vit()
    assert m.train_tokenizer == "torch" and m.down_projection.train_route == "torch"
    m.train_tokenizer = "hip"
    assert m.train_tokenizer == "hip" and m.down_projection.train_route == "hip"
    assert m.train_attention == "torch" and m.train_linear == "torch"
    for bad in ("HIP", "strict", None, 1):
        with pytest.raises(ValueError, match="train_tokenizer"):
            m.train_tokenizer = bad
    assert m.train_tokenizer == "hip"
    m.train_attention = m.train_linear = "hip"
    assert m.train_tokenizer == "hip"
    m.train_tokenizer = "torch"
    assert m.train_attention == "hip" and m.train_linear == "hip"


def test_unsupported_reason_on_the_cpu_and_the_torch_modules_run():
    m = _small_vit()
    x = V.synthetic_input(11, 1, (16, 16, 16))
    assert "CPU" in m.tokenizer_unsupported_reason(x)
    assert "gradient" in m.tokenizer_unsupported_reason(x.clone().requires_grad_(True))
    out = {}
    for mode in ("torch", "hip"):
        m.train_tokenizer = mode
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.square().mean().backward()
        out[mode] = (y.detach(), {n: p.grad.clone() for n, p in m.named_parameters()})
    assert torch.equal(out["torch"][0], out["hip"][0])
    assert all(torch.equal(g, out["hip"][1][n]) for n, g in out["torch"][1].items())


def test_driver_flag_parses_and_defaults_to_torch(tmp_path):
    from anatomix_amd.pretraining.pretrain_anatomix import build_networks, build_parser, options_from_args
    base = ["--ckpt_dir", str(tmp_path), "--name", "t", "--dataroot", str(tmp_path), "--netG", "primus", "--primus_version", "v2", "--primus_config", "S",
            "--crop_size", "16"]
    opt = lambda *argv: options_from_args(build_parser(primus_route=True).parse_args(base + list(argv)))
    assert opt().primus_train_tokenizer == "torch" and opt().primus_train_route == "hip"
    assert opt("--primus_train_tokenizer", "hip").primus_train_tokenizer == "hip"
    with pytest.raises(SystemExit):
        opt("--primus_train_tokenizer", "f16")
    assert "primus_train_tokenizer" not in {a.dest for a in build_parser()._actions}
    assert options_from_args(build_parser().parse_args(base)).primus_train_tokenizer == "torch"
    net = build_networks(opt("--primus_train_tokenizer", "hip"), torch.device("cpu"))[0]
    assert net.train_tokenizer == "hip" and net.train_linear == "hip"
    assert build_networks(opt(), torch.device("cpu"))[0].train_tokenizer == "torch"


def test_new_mfma_kernels_neither_spill_nor_use_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_budget
    finally:
        sys.path.pop(0)
    rows = isa_budget.budget(os.path.join(ROOT, "anatomix_amd", "csrc", "amx_tokenizer_bwd.hip"))
    kernels = {r["kernel"] for r in rows}
    assert {"tokwgrad_kernel<27,2>", "tokwgrad_kernel<27,1>", "tokwgrad_kernel<1,1>", "tokdgrad2_kernel<2,2>"} <= kernels, kernels
    for r in rows:
        assert r["mfma"] > 0 and r["spill"] == 0 and r["scratch_bytes"] == 0, r
