"""CPU float64 reference of the conv tokenizer under autograd (csrc/amx_tokenizer_bwd.hip): stem + the three residual stages of
``PatchEmbedDeeper`` restated so that every LeakyReLU takes its sign mask as an argument (``x * where(mask, 1, 0.01)``).  With the
masks left free (``pre > 0``) it is the network itself; with the masks a kernel route took it is the function that route
differentiates, which is what the route's gradients are held to: a single free-running flip moves a gradient by 4e-3.

Parameters: ``oracle.vit_ref.synthetic_state_dict`` with every norm weight redrawn as 1 + 0.3 randn, every norm bias and conv bias as
0.2 randn, and in every norm one weight exactly 0 and one negative (the backward must never divide by gamma)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import vit_ref as V

SLOPE = 0.01
EPS = 1e-2
STAGE = ("conv1.weight", "conv1.bias", "norm1.weight", "norm1.bias", "conv2.weight", "conv2.bias", "norm2.weight", "norm2.bias",
         "skip.weight", "skip_norm.weight", "skip_norm.bias")
NAMES = ["stem.conv.weight", "stem.conv.bias", "stem.norm.weight", "stem.norm.bias"] + [f"stages.{k}.{s}" for k in range(3) for s in STAGE]
# the seven conv biases in front of an InstanceNorm (exactly zero gradient) -> the raw conv output they belong to
NORMED_BIAS = {"stem.conv.bias": "stem"} | {f"stages.{k}.conv{i}.bias": f"s{k}.raw{i}" for k in range(3) for i in (1, 2)}
SITES = ("h0", "a1_0", "h1", "a1_1", "h2", "a1_2", "h3")          # the seven LeakyReLUs, in amx_tokenizer_train_export's order

# name: (N, (D, H, W)).  A: the minimum (deepest level 4^3).  B: two z-planes at the deepest level, both borders in one tile.
# C: rows of 2 voxels at the deepest level (a 16-voxel tile wraps 8 rows), stem W = 16.
CASES = OrderedDict(A=(2, (32, 32, 32)), B=(1, (16, 32, 64)), C=(3, (64, 32, 16)))


def parameters(seed):
    """{name: float32 tensor} in the order of NAMES."""
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(16, 16, 16), eva_depth=1)
    sd = V.synthetic_state_dict(kw, seed)
    g = torch.Generator().manual_seed(7000 + seed)
    out = OrderedDict()
    for name in NAMES:
        t = sd["down_projection." + name].clone()
        if "norm" in name and name.endswith("weight"):
            t = 1 + 0.3 * torch.randn(t.shape, generator=g)
            t[3] = 0.0
            t[5] = -t[5].abs() - 0.05
        elif name.endswith("bias"):
            t = 0.2 * torch.randn(t.shape, generator=g)
        out[name] = t.float().contiguous()
    return out


def inputs(case, seed=0):
    n, size = CASES[case] if isinstance(case, str) else case
    x = V.synthetic_input(100 + seed, n, size)
    g = torch.Generator().manual_seed(9000 + seed)
    d_h3 = torch.randn(n, 128, size[0] // 8, size[1] // 8, size[2] // 8, generator=g)
    return x, d_h3


def _inorm(x, w, b, eps):
    mean = x.mean((2, 3, 4), keepdim=True)
    var = x.var((2, 3, 4), unbiased=False, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w.view(1, -1, 1, 1, 1) + b.view(1, -1, 1, 1, 1)


def forward(x, p, masks=None, eps=EPS, keep=None):
    """h3 and the seven pre-activations; ``masks``: seven bool tensors, or None for the free network.  ``keep``: a dict that receives
    the raw conv outputs (with ``retain_grad``) by the names of NORMED_BIAS."""
    pre = []

    def act(v):
        m = v.detach() > 0 if masks is None else masks[len(pre)]
        pre.append(v)
        return v * torch.where(m, torch.ones((), dtype=v.dtype), torch.full((), SLOPE, dtype=v.dtype))

    def raw(name, v):
        if keep is not None:
            v.retain_grad()
            keep[name] = v
        return v

    h = act(_inorm(raw("stem", F.conv3d(x, p["stem.conv.weight"], p["stem.conv.bias"], padding=1)), p["stem.norm.weight"], p["stem.norm.bias"], eps))
    for k in range(3):
        q = lambda s: p[f"stages.{k}.{s}"]
        a1 = act(_inorm(raw(f"s{k}.raw1", F.conv3d(h, q("conv1.weight"), q("conv1.bias"), stride=2, padding=1)), q("norm1.weight"), q("norm1.bias"), eps))
        y = _inorm(raw(f"s{k}.raw2", F.conv3d(a1, q("conv2.weight"), q("conv2.bias"), padding=1)), q("norm2.weight"), q("norm2.bias"), eps)
        s = _inorm(F.conv3d(F.avg_pool3d(h, 2), q("skip.weight")), q("skip_norm.weight"), q("skip_norm.bias"), eps)
        h = act(y + s)
    return h, pre


def reference(x, p, d_h3, masks=None, eps=EPS, dtype=torch.float64):
    """dict(h3, pre (list of 7), masks (list of 7 bool), grads {name: tensor}, draw_abs {bias name: per-channel sum |d_raw|}) in
    ``dtype`` on the CPU."""
    pp = OrderedDict((k, v.detach().to(dtype).cpu().requires_grad_(True)) for k, v in p.items())
    keep = {}
    h3, pre = forward(x.detach().to(dtype).cpu(), pp, None if masks is None else [m.cpu() for m in masks], eps, keep)
    h3.backward(d_h3.detach().to(dtype).cpu())
    return dict(h3=h3.detach(), pre=[v.detach() for v in pre], masks=[v.detach() > 0 for v in pre] if masks is None else masks,
                grads=OrderedDict((k, v.grad) for k, v in pp.items()),
                draw_abs={b: keep[r].grad.abs().sum((0, 2, 3, 4)) for b, r in NORMED_BIAS.items()})


def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()
