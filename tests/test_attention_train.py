"""CPU side of the attention core under autograd: the float64 emulation of the kernel's rounding points stays inside the bounds the
GPU test holds the kernel to (this pins tests/_attn_bwd_ref.py), the three C-ABI entries are declared, and the module switch."""
import os
import re

import pytest
import torch

import _attn_bwd_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d.architectures import EvaAttention
from oracle import vit_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("amx_attention_train_scratch_bytes", "amx_attention_qknorm_rope_train", "amx_attention_backward")


@pytest.mark.parametrize("shape", R.SHAPES, ids=str)
def test_emulation_of_the_rounding_points_is_inside_the_bounds(shape):
    """f16 operands alone cost about 5e-4 rel-L2: inside rel-L2 < 1e-3 / max-norm < 4e-3 on dq, dk, dv by about 2x and 4x; the norm
    vectors up to 1.0e-3 (held to 2e-3 here); k_norm.bias on its absolute scale."""
    att, q, k, v, dout, table = R.make_case(shape)
    exact = R.exact_grads(att, q, k, v, dout, table, shape[4])
    emul = R.emulated_grads(att, q, k, v, dout, table, shape[4])
    for name in R.NAMES:
        if exact[name] is None:
            assert emul[name] is None and not shape[5]
            continue
        assert emul[name].shape == exact[name].shape
        if name == "k_norm.bias":
            assert ((emul[name] - exact[name]).abs() <= 2.0 ** -9 * exact["k_bias_scale"]).all()
            if table is None:            # a shift common to all keys leaves the softmax unchanged
                assert exact[name].abs().max() <= 1e-12 * exact["k_bias_scale"].max()
            continue
        e, m = R.errors(emul[name], exact[name])
        if name in ("dq", "dk", "dv"):
            assert 1e-4 < e < 1e-3 and m < 4e-3, (name, e, m)
        else:
            assert e < 2e-3 and m < 2e-3, (name, e, m)


def test_entries_are_declared_in_the_table_and_the_header():
    header = open(os.path.join(ROOT, "include", "anatomix_amd.h")).read()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b" + name + r"\(", header), name
    # the backward takes the forward's arguments, the saved tensors, seven gradient outputs, the scratch and the stream
    assert len(_lib.SYMBOLS["amx_attention_backward"][1]) == 27
    assert len(_lib.SYMBOLS["amx_attention_qknorm_rope_train"][1]) == len(_lib.SYMBOLS["amx_attention_qknorm_rope"][1]) + 1


def _small_vit():
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(16, 16, 16), eva_depth=1)
    m = PrimusV2(**kw)
    m.load_state_dict(V.synthetic_state_dict(kw, 3), strict=True)
    return m


def test_train_attention_validates_its_value_and_reaches_every_block():
    m = _small_vit()
    assert m.train_attention == "torch" and all(b.attn.train_core == "torch" for b in m.eva.blocks)
    m.train_attention = "hip"
    assert m.train_attention == "hip" and all(b.attn.train_core == "hip" for b in m.eva.blocks)
    for bad in ("HIP", "flash", None, 1):
        with pytest.raises(ValueError, match="train_attention"):
            m.train_attention = bad
    assert m.train_attention == "hip"
    assert EvaAttention(132, 2, True, False).train_core == "torch"


def test_cpu_module_takes_the_torch_core_whatever_the_switch_says():
    m = _small_vit()
    x = V.synthetic_input(11, 1, (16, 16, 16))
    grads = {}
    for mode in ("torch", "hip"):
        m.train_attention = mode
        m.zero_grad(set_to_none=True)
        m(x).square().mean().backward()
        grads[mode] = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert grads["torch"].keys() == grads["hip"].keys() and grads["hip"]
    for name, g in grads["torch"].items():
        assert torch.equal(g, grads["hip"][name]), name
