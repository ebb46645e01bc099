"""CPU references for the backward of the attention core (csrc/amx_attention_bwd.hip):

* ``exact_grads``     float64 gradients of ``EvaAttention.double().core_torch`` through ``torch.autograd.grad``;
* ``emulated_grads``  the same mathematics in float64 with the KERNEL'S ROUNDING POINTS: q-hat (carrying log2(e) / sqrt(hd)), k-hat,
  v-hat, P, dS and the scaled dO-hat are rounded to f16; D comes from the unrounded dO; the adjoint of the preparation
  (rotation, per-head LayerNorm) is exact.  Its distance from ``exact_grads`` is what f16 operands cost, whatever the kernel does
  with its fp32 sums -- the yardstick of tests/test_attention_train_gpu.py.
"""
import math

import numpy as np
import torch

from anatomix_amd.model.vit3d.architectures import EvaAttention, _rope, build_rope_table

NAMES = ("dq", "dk", "dv", "q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias")
GRAD_EXP = 3           # the kernel's normalisation: max |dO-hat| of a (batch, head) lies in [2^3, 2^4)

# (B, N, heads, hd, n_prefix, qk_norm, rope)
SHAPES = [
    (1, 72, 2, 66, 8, True, True),          # 4^3 grid + 8 register tokens: a second, partial key block; partial query workgroup
    (1, 100, 2, 64, 0, False, False),       # plain attention
    (2, 200, 3, 18, 4, True, False),        # both operand widths padded; batch and head strides
    (1, 129, 1, 80, 1, False, False),       # the no-ONES instantiation; one query past a workgroup
    (2, 520, 6, 66, 8, True, True),         # the model's head layout over nine key blocks
]


def make_case(shape):
    """Seeded module (CPU, fp32; norm weights and biases randomised), q, k, v, dO [B, N, E] and the rotary table (or None)."""
    B, N, heads, hd, nreg, qk_norm, rope = shape
    rs = np.random.RandomState(B * 1000 + N)
    E = heads * hd
    att = EvaAttention(E, heads, qk_norm, False)
    if qk_norm:
        for ln in (att.q_norm, att.k_norm):
            ln.weight.data = torch.from_numpy(rs.uniform(0.5, 1.5, hd).astype(np.float32))
            ln.bias.data = torch.from_numpy((rs.randn(hd) * 0.1).astype(np.float32))
    q, k, v, dout = [torch.from_numpy(rs.randn(B, N, E).astype(np.float32)) for _ in range(4)]
    table = None
    if rope:
        side = round((N - nreg) ** (1 / 3))
        assert side ** 3 == N - nreg
        table = build_rope_table((side,) * 3, hd)
    return att, q, k, v, dout, table


def _f16(t):
    return t.to(torch.float16).to(torch.float64)


def _norm_params(att):
    if att.q_norm is None:
        return []
    return [att.q_norm.weight, att.q_norm.bias, att.k_norm.weight, att.k_norm.bias]


def _as_dict(grads, has_norm):
    out = dict(zip(NAMES[:3], grads[:3]))
    for i, name in enumerate(NAMES[3:]):
        out[name] = grads[3 + i] if has_norm else None
    return out


def exact_grads(att, q, k, v, dout, table, n_prefix):
    """{name: float64 gradient} of sum(core_torch(q, k, v) * dout), plus ``"k_bias_scale"``: per channel the sum over rows
    (batch, head, token) of |gradient reaching k_norm's output| -- the absolute scale of ``k_norm.bias``'s gradient, whose true value
    is a small remainder of cancelling terms (exactly zero without rotation).  None where the module has no QK norm."""
    att64 = EvaAttention(att.num_heads * att.head_dim, att.num_heads, att.q_norm is not None, False).double()
    att64.load_state_dict({n: p.double() for n, p in att.state_dict().items()})
    q64, k64, v64 = [t.double().requires_grad_(True) for t in (q, k, v)]
    kept = []
    hook = att64.k_norm.register_forward_hook(lambda m, i, o: kept.append(o)) if att64.k_norm is not None else None
    y = att64.core_torch(q64, k64, v64, None if table is None else table.double(), n_prefix)
    if hook is not None:
        hook.remove()
    grads = torch.autograd.grad(y, [q64, k64, v64] + _norm_params(att64) + kept, dout.double())
    out = _as_dict([g.detach() for g in grads], att64.q_norm is not None)
    out["k_bias_scale"] = grads[-1].detach().abs().sum(dim=(0, 1, 2)) if kept else None      # k_norm output: [B, heads, N, hd]
    return out


def emulated_grads(att, q, k, v, dout, table, n_prefix):
    """{name: float64 gradient} with the kernel's f16 rounding points (module docstring)."""
    B, N, E = q.shape
    heads, hd = att.num_heads, att.head_dim
    has_norm = att.q_norm is not None
    att64 = EvaAttention(E, heads, has_norm, False).double()
    att64.load_state_dict({n: p.double() for n, p in att.state_dict().items()})
    sh = lambda t: t.reshape(B, N, heads, hd).transpose(1, 2)                    # [B, heads, N, hd]
    q64, k64, v64 = [t.double().requires_grad_(True) for t in (q, k, v)]
    # the preparation, exact, as a differentiable function (its adjoint is taken by autograd below)
    qt, kt = sh(q64), sh(k64)
    if has_norm:
        qt, kt = att64.q_norm(qt), att64.k_norm(kt)
    if table is not None:
        t64 = table.double()
        qt = torch.cat((qt[:, :, :n_prefix], _rope(qt[:, :, n_prefix:], t64)), 2)
        kt = torch.cat((kt[:, :, :n_prefix], _rope(kt[:, :, n_prefix:], t64)), 2)
    qt = qt * (math.log2(math.e) / math.sqrt(hd))
    qh, kh, vh = _f16(qt.detach()), _f16(kt.detach()), _f16(sh(v64).detach())      # rounding points 1-3
    s = qh @ kh.transpose(-1, -2)                                                 # exp2 domain
    lse = torch.logsumexp(s * math.log(2.0), -1, keepdim=True) / math.log(2.0)
    p = torch.exp2(s - lse)
    o = p @ vh
    do = sh(dout.double())
    d = (do * o).sum(-1, keepdim=True)                                            # from the unrounded dO
    amax = do.abs().amax(dim=(-1, -2), keepdim=True)                              # one power of two per (batch, head)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.clamp_min(1e-300))) - GRAD_EXP, torch.zeros_like(amax))
    doh = _f16(do * torch.exp2(-e))                                               # rounding point 4
    dp = doh @ vh.transpose(-1, -2)
    ds = _f16(p * (dp - d * torch.exp2(-e)))                                      # rounding point 6
    p16 = _f16(p)                                                                 # rounding point 5
    dvh = (p16.transpose(-1, -2) @ doh) * torch.exp2(e)
    dqh = math.log(2.0) * (ds @ kh) * torch.exp2(e)
    dkh = math.log(2.0) * (ds.transpose(-1, -2) @ qh) * torch.exp2(e)
    grads = torch.autograd.grad([qt, kt], [q64, k64] + _norm_params(att64), [dqh, dkh])
    dv = dvh.transpose(1, 2).reshape(B, N, E)
    return _as_dict([grads[0].detach(), grads[1].detach(), dv] + [g.detach() for g in grads[2:]], has_norm)


def errors(got, ref):
    """(rel-L2, max-norm error) of one tensor against its float64 reference."""
    got, ref = got.double().cpu(), ref.double()
    return (((got - ref).norm() / ref.norm().clamp_min(1e-300)).item(),
            ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item())
