"""Float64 side of the ViT's dense patch decoder under autograd (csrc/amx_vit_decode_train.hip, include/anatomix_amd.h): the cases the
CPU and GPU tests share, the reference -- float64 CPU autograd through the real modules, ``PatchDecode`` + ``build_out_norm`` -- and
the restatement of the decoder in NESTED ROW ORDER, which is what the kernels compute: a stage is a row product
[R, Cin] x [Cin, 8 Cout] whose output read as [8 R, Cout] is the next stage's input without moving data (row = token, then the child
offset (kz, ky, kx) of stage 1, then of stage 2), LayerNorm + erf-GELU are row operators, and only the last stage un-nests to planar."""
import math

import torch
import torch.nn as nn

from _decode_rows_ref import named_params, rel_l2, widths_of          # noqa: F401  (re-exported for the tests)
from anatomix_amd.model.vit3d.architectures import LayerNormNd, PatchDecode, build_out_norm

BAR = 2e-5           # rel-L2 against float64 for every output and gradient: the bar of the project's fp32-grade training routes
ZERO_BAR = 1e-4      # a mathematically zero gradient, relative to the sum of the magnitudes of its terms
LN_EPS, OUT_EPS = 1e-6, 1e-5

# name -> (widths E / c1 / c2 / C, views, token grid, output norm)
CASES = {
    "A": ([24, 16, 8, 4], 1, (1, 1, 3), "none"),
    "B": ([396, 168, 72, 16], 2, (2, 3, 4), "demean"),
    "C": ([396, 168, 72, 16], 2, (2, 3, 4), "instance"),
    "D": ([1056, 328, 104, 16], 1, (1, 2, 2), "none"),
    "E": ([132, 64, 32, 12], 3, (2, 2, 2), "demean"),
}
ZERO_GRADS = {"none": (), "demean": ("b3",), "instance": ("b3",)}      # the spatial norms remove the last bias


def build_modules(widths, out_norm, seed, dtype=torch.float64):
    """A three-stage PatchDecode of exactly ``widths`` and its output norm module, every parameter drawn (norm weights around 1)."""
    g = torch.Generator().manual_seed(seed)
    dec = PatchDecode((8, 8, 8), widths[0], widths[3])
    if widths_of(dec) != list(widths):          # widths PatchDecode's rule does not produce: the same modules at the stated widths
        ch = list(widths)
        stages = [nn.Sequential(nn.ConvTranspose3d(ch[k], ch[k + 1], 2, stride=2), LayerNormNd(ch[k + 1]), nn.GELU()) for k in range(2)]
        dec.decode = nn.Sequential(*stages, nn.ConvTranspose3d(ch[2], ch[3], 2, stride=2))
    on = build_out_norm(out_norm, widths[3], OUT_EPS)
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if p.dim() == 5:
                p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(p.shape[0]))
            elif name.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    return dec.to(dtype), on.to(dtype)


def case_inputs(name):
    """(decoder, out norm module, tokens [N, T, E], dy [N, C, D, H, W], grid, norm name), float64 on the CPU, seeded by the name."""
    widths, n, grid, norm = CASES[name]
    seed = 100 + ord(name[0])
    dec, on = build_modules(widths, norm, seed)
    g = torch.Generator().manual_seed(seed + 1)
    tokens = torch.randn(n, grid[0] * grid[1] * grid[2], widths[0], generator=g, dtype=torch.float64)
    dy = torch.randn(n, widths[3], *(8 * s for s in grid), generator=g, dtype=torch.float64)
    return dec, on, tokens, dy, grid, norm


def run_modules(dec, on, tokens, dy, grid):
    """{"out", "d_tokens", parameter names ..., "terms"} of ``on(dec(tokens as a volume))`` at the modules' dtype and device;
    ``terms``: per output channel the sum over views and voxels of |d raw output| -- the magnitudes whose signed sum is d b3."""
    for p in dec.parameters():
        p.grad = None
    tok = tokens.detach().clone().requires_grad_(True)
    n, _, e = tok.shape
    raw = dec(tok.transpose(1, 2).reshape(n, e, *grid))
    seen = {}
    raw.register_hook(lambda g: seen.__setitem__("terms", g.abs().sum((0, 2, 3, 4))))
    out = on(raw)
    out.backward(dy)
    res = {"out": out.detach(), "d_tokens": tok.grad, "terms": seen["terms"]}
    res.update({k: v.grad for k, v in named_params(dec, None).items()})
    return res


def _gelu_erf(y):
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))


def nested_restated(tokens, params, grid, norm, ln_eps=LN_EPS, out_eps=OUT_EPS):
    """The volume [N, C, 8 gd, 8 gh, 8 gw] from tokens [N, T, E] and ``params`` = dict(w1, b1, g1, be1, w2, b2, g2, be2, w3, b3) with the
    conv weights as torch stores them, [cin, cout, 2, 2, 2]: stage GEMMs on nested rows, row LN + GELU, the un-nest.  Differentiable."""
    n, t, e = tokens.shape
    gd, gh, gw = grid
    rows = tokens.reshape(n * t, e)
    for s in (1, 2, 3):
        w, b = params[f"w{s}"], params[f"b{s}"]
        cin, cout = w.shape[:2]
        bp = w.reshape(cin, cout, 8).permute(0, 2, 1).reshape(cin, 8 * cout)          # column k cout + co, k = 4 kz + 2 ky + kx
        a = (rows @ bp + b.repeat(8)).reshape(-1, cout)                                # [R, 8 cout] read as [8 R, cout]
        if s < 3:
            mean = a.mean(-1, keepdim=True)
            var = ((a - mean) ** 2).mean(-1, keepdim=True)
            a = _gelu_erf((a - mean) / torch.sqrt(var + ln_eps) * params[f"g{s}"] + params[f"be{s}"])
        rows = a
    c = rows.shape[1]
    # row index ((((n T + t) 8 + k1) 8 + k2) 8 + k3: (n, tz, ty, tx, z1, y1, x1, z2, y2, x2, z3, y3, x3, c) -> (n, c, z, y, x)
    v = rows.reshape(n, gd, gh, gw, 2, 2, 2, 2, 2, 2, 2, 2, 2, c).permute(0, 13, 1, 4, 7, 10, 2, 5, 8, 11, 3, 6, 9, 12)
    v = v.reshape(n, c, 8 * gd, 8 * gh, 8 * gw)
    if norm == "demean":
        return v - v.mean((2, 3, 4), keepdim=True)
    if norm == "instance":
        mean = v.mean((2, 3, 4), keepdim=True)
        var = ((v - mean) ** 2).mean((2, 3, 4), keepdim=True)
        return (v - mean) / torch.sqrt(var + out_eps)
    if norm != "none":
        raise ValueError(norm)
    return v
