"""CPU float64 references of the linear layers under autograd (csrc/amx_linear_bwd.hip): ``exact`` is float64 autograd of F.linear,
``emulated`` the same products with the kernel's three rounding points -- x^ = f16(x), W^ = f16(W), dy^ = f16(dy 2^-e) with one
exponent per call, 2^e <= max |dy| / 8 < 2^(e+1) (an all-zero dy: e = 0) -- and exact sums.  Both return the ``S`` matrices that
scale an accumulation bound: the same sums over absolute values."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64

# (M, K, N, bias): the smallest shapes at which each part can go wrong
SHAPES = (
    (72, 396, 396, True),       # the model's width: K padded 396 -> 416, a 12-feature last tile, a partial row tile
    (200, 1056, 396, True),     # fc2: 33 K steps
    (200, 396, 1056, True),     # fc1: the 66-tile side
    (129, 64, 20, False),       # no bias (k_proj), N below two tiles, one row past a tile
    (33, 8, 4, True),           # the envelope's floor
    # wgrad chunking: 2100 tokens = 66 steps of 32; 2 x 3 workgroups per chunk ask for the 16-step minimum -> 5 token chunks, the last
    # one of 2 steps whose second ends at token 2100 of 2112.  x is handed over as [2, 1050, 132].
    (2100, 132, 264, True),
)
M5_LEADING = (2, 1050)


def make_case(shape):
    """fp32 x ~ N(0, 1), W ~ N(0, 1 / K), b ~ N(0, 1) / 2, dy ~ N(0, 1) x a per-row factor from U(0.01, 3); RandomState(7 M + K)."""
    M, K, N, bias = shape
    rs = np.random.RandomState(7 * M + K)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    x = t(rs.randn(M, K))
    w = t(rs.randn(N, K) / math.sqrt(K))
    b = t(rs.randn(N) * 0.5) if bias else None
    dy = t(rs.randn(M, N) * rs.uniform(0.01, 3.0, size=(M, 1)))
    return x, w, b, dy


def exponent(dy):
    """The call's exponent: floor(log2(max |dy|)) - 3 within [-126, 126]; 0 for an all-zero (or non-finite) dy."""
    am = float(dy.abs().max())
    if not (am > 0.0 and math.isfinite(am)):
        return 0
    return max(-126, min(126, math.frexp(am)[1] - 1 - 3))


def exact(x, w, b, dy):
    """float64 autograd of F.linear -> dict(y, dx, dw, db) (db None without a bias)."""
    xd, wd = x.to(F64).requires_grad_(True), w.to(F64).requires_grad_(True)
    bd = None if b is None else b.to(F64).requires_grad_(True)
    y = F.linear(xd, wd, bd)
    grads = torch.autograd.grad(y, [xd, wd] + ([] if bd is None else [bd]), dy.to(F64))
    return dict(y=y.detach(), dx=grads[0], dw=grads[1], db=None if bd is None else grads[2])


def emulated(x, w, b, dy, rounding=True):
    """The kernel's arithmetic with exact sums -> (dict(y, dx, dw, db), dict of the S matrices under the same names).  The inputs are
    fp32, so each ``.to(float16)`` below is the single rounding the kernel makes (the scaling by 2^-e is exact in fp32)."""
    e = exponent(dy) if rounding else 0
    r16 = (lambda t: t.to(torch.float16).to(F64)) if rounding else (lambda t: t.to(F64))
    xh, wh = r16(x), r16(w)
    dyh = r16(dy * 2.0 ** -e)
    up = 2.0 ** e
    bd = None if b is None else b.to(F64)
    y = xh @ wh.T + (0 if bd is None else bd)
    out = dict(y=y, dx=(dyh @ wh) * up, dw=(dyh.T @ xh) * up, db=None if b is None else dy.to(F64).sum(0))
    S = dict(y=xh.abs() @ wh.abs().T + (0 if bd is None else bd.abs()), dx=(dyh.abs() @ wh.abs()) * up, dw=(dyh.abs().T @ xh.abs()) * up,
             db=dy.to(F64).abs().sum(0))
    return out, S


@functools.lru_cache(maxsize=None)
def case(idx):
    """(inputs, exact, emulated, S) of shape ``idx``, computed once and shared (never modified)."""
    inputs = make_case(SHAPES[idx])
    emu, S = emulated(*inputs)
    return inputs, exact(*inputs), emu, S


def errors(got, ref):
    """(rel-L2, max-norm error) of one tensor against its float64 reference."""
    got, ref = got.double().cpu(), ref.double()
    return (((got - ref).norm() / ref.norm().clamp_min(1e-300)).item(),
            ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item())
