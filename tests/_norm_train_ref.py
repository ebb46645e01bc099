"""Reference of the token LayerNorms under autograd (csrc/amx_layernorm_train.hip; not a test module): float64 ``F.layer_norm`` --
with ``F.silu(g) * x`` in front of it for the gated cases -- under CPU autograd, and the closed forms the kernels implement, in float64.

Cases are ``(M, C)``, each run plain and gated.  Inputs: a row is ``mean + std * randn`` with the row mean uniform in [-2, 2] and the
row standard deviation log-uniform in [0.25, 4]; the gate is ``2 * randn``; ``w = 1 + 0.3 randn``, ``b = 0.2 randn``, ``dy = randn``;
seeds are fixed per case.  There are no degenerate rows here (tests/test_norm_train_gpu.py has them in a test of their own).  eps is
1e-6, and 1e-5 in the plain (5, 396) case.  (2100, 132) is handed to the autograd functions as [2, 1050, 132]."""
import functools
import math

import torch
import torch.nn.functional as F

SHAPES = ((1, 132), (5, 396), (2100, 132), (257, 1056), (130, 2816), (64, 4096), (8200, 352))
CASES = tuple((m, c, gated) for m, c in SHAPES for gated in (False, True))
BATCHED = {2100: (2, 1050)}          # the leading axes a case is fed to the functions with
TENSORS = ("y", "mean", "rstd", "dx", "dgate", "dw", "db")


def case_id(case):
    return "%dx%d-%s" % (case[0], case[1], "gated" if case[2] else "plain")


def eps_of(case):
    return 1e-5 if case == (5, 396, False) else 1e-6


def rel_l2(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def inputs(case):
    """fp32 CPU tensors ``x, gate (or None), w, b, dy`` of a case."""
    m, c, gated = case
    g = torch.Generator().manual_seed(1000 * SHAPES.index((m, c)) + 17 + int(gated))
    mean = 4 * torch.rand(m, 1, generator=g, dtype=torch.float64) - 2
    std = torch.exp(math.log(0.25) + math.log(16.0) * torch.rand(m, 1, generator=g, dtype=torch.float64))
    x = (mean + std * torch.randn(m, c, generator=g, dtype=torch.float64)).float()
    gate = (2 * torch.randn(m, c, generator=g, dtype=torch.float64)).float() if gated else None
    w = (1 + 0.3 * torch.randn(c, generator=g, dtype=torch.float64)).float()
    b = (0.2 * torch.randn(c, generator=g, dtype=torch.float64)).float()
    dy = torch.randn(m, c, generator=g, dtype=torch.float64).float()
    return x, gate, w, b, dy


def autograd(x, gate, w, b, dy, eps, dtype=torch.float64):
    """``F.layer_norm`` (after ``F.silu(gate) * x``) and its gradients under CPU autograd in ``dtype``; a dict over TENSORS (dgate is
    None without a gate)."""
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    x, gate, w, b = leaf(x), leaf(gate), leaf(w), leaf(b)
    u = x if gate is None else F.silu(gate) * x
    y = F.layer_norm(u, (x.shape[-1],), w, b, eps)
    y.backward(dy.to(dtype))
    ud = u.detach()
    mean = ud.mean(-1)
    rstd = (ud.var(-1, unbiased=False) + eps).rsqrt()
    return dict(y=y.detach(), mean=mean, rstd=rstd, dx=x.grad, dgate=None if gate is None else gate.grad, dw=w.grad, db=b.grad)


def closed_forms(x, gate, w, b, dy, eps):
    """The formulas of include/anatomix_amd.h, in float64, without autograd."""
    x, w, b, dy = x.double(), w.double(), b.double(), dy.double()
    u = x
    if gate is not None:
        gate = gate.double()
        s = torch.sigmoid(gate)
        u = gate * s * x
    mean = u.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((u - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (u - mean) * rstd
    t = dy * w
    du = rstd * (t - t.mean(-1, keepdim=True) - xh * (t * xh).mean(-1, keepdim=True))
    flat = lambda v: v.reshape(-1, v.shape[-1])
    out = dict(y=xh * w + b, mean=mean.squeeze(-1), rstd=rstd.squeeze(-1), dw=flat(dy * xh).sum(0), db=flat(dy).sum(0))
    if gate is None:
        out.update(dx=du, dgate=None)
    else:
        out.update(dx=du * gate * s, dgate=du * x * s * (1 + gate * (1 - s)))
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    """The float64 autograd result of a case, computed once and shared; do not modify it."""
    return autograd(*inputs(case), eps_of(case))
