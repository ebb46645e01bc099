"""``anatomix-dev-vit``: the PrimusV2 3D ViT with the call surface of ``anatomix.model.vit3d.PrimusV2``
(reference: anatomix/model/vit3d/architectures.py:231-260 + ``_PrimusExtensions`` :89-165, tokenizer deep_tokenizer.py:12-149,
registry entry load_from_hf.py:25-35).

The reference class is a thin subclass of ``dynamic_network_architectures.architectures.primus.PrimusV2`` (PyPI package
``dynamic-network-architectures==0.4.4``, requirements.txt:17; its EVA blocks come from ``timm``).  That package is neither in
the reference tree nor in this image, so the network body is RESTATED here from the published architecture (see
oracle/vit_ref.py for every assumption) -- **parity with the upstream package is unpinned**: constructor keywords, the
``forward(x, layers, encode_only)`` contract, the wrapper's extensions (per-head QK LayerNorm, register-token init,
``ChannelDemean`` output norm, tokenizer ``in_eps``) and the arithmetic of the published blocks are reproduced; upstream
state_dict key names and a few hyper-parameters of the tokenizer / decoder could not be checked.

What runs where: for CUDA inputs under ``torch.no_grad()`` the WHOLE forward -- conv tokenizer, position embedding / register
tokens, every EVA block (LayerNorms, q / k / v, QK-LayerNorm + rotary embedding + softmax attention, output projection,
LayerScale residuals, SwiGLU MLP), final norm, transposed-conv decoder, ChannelDemean -- is ONE call into libanatomix_amd.so
(``amx_vit_forward``, csrc/amx_vit.hip: own MFMA kernels for the convolutions, the token-matrix products and the attention;
no vendor GEMM / conv library).  Output norms other than none / demean are applied on the engine's output by their torch module.
Under autograd or on the CPU the torch modules below compute the same network; ``PrimusV2.use_engine = False`` forces that
composition on the GPU too (its attention core then still runs through ``amx_attention_qknorm_rope``).  Of training, three parts
are on the accelerated path, each behind its own switch with the default ``"torch"``: ``PrimusV2.train_attention = "hip"`` runs
the attention core forward and backward on the library's kernels (``_AttentionCoreFn``: amx_attention_qknorm_rope_train /
amx_attention_backward) instead of F.scaled_dot_product_attention, and ``PrimusV2.train_linear = "hip"`` runs the blocks' seven
nn.Linear the same way (``_LinearFn``: amx_linear_forward / amx_linear_backward, f16 operands and fp32 sums).  Another part has no
switch: ``PrimusV2.forward_train_sampled`` (what the contrastive step calls) computes the decoder and a per-voxel output norm only at
the sampled voxels (``_DecodeRowsFn``: amx_vit_decode_rows_forward / _backward, fp32).  ``PrimusV2.train_tokenizer = "hip"`` runs the
conv tokenizer's stem and stages (``_TokenizerFn``: amx_tokenizer_train_forward / amx_tokenizer_backward, strict hi + lo f16 operands;
``proj`` stays torch).  ``PrimusV2.train_norm = "hip"`` runs the blocks' four token LayerNorms, the SwiGLU product in front of
``mlp.norm`` and the final norm (``_LayerNormFn`` / ``_GatedLayerNormFn``: amx_layernorm_train_forward / amx_layernorm_backward, fp32).
``PrimusV2.train_decoder = "hip"`` runs the dense decoder of ``forward`` and a spatial output norm (none / demean / instance)
(``_DecoderFn``: amx_vit_decoder_train_forward / amx_vit_decoder_backward, fp32 on the f32-input MFMA) -- the path of a contrastive step
whose output norm needs the whole volume, and of dense supervision.  LayerScale is torch autograd either way.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _lib

# architectures.py:20-25
PRIMUS_CONFIGS = {
    "S": {"eva_depth": 12, "eva_numheads": 6, "embed_dim": 396},
    "B": {"eva_depth": 12, "eva_numheads": 12, "embed_dim": 792},
    "M": {"eva_depth": 16, "eva_numheads": 12, "embed_dim": 864},
    "L": {"eva_depth": 24, "eva_numheads": 16, "embed_dim": 1056},
}


class ChannelDemean(nn.Module):
    """architectures.py:28-33: subtract each channel's spatial mean."""

    def forward(self, x):
        return x - x.mean(dim=(2, 3, 4), keepdim=True)


class ChannelLayerNorm(nn.Module):
    """architectures.py:36-52: standardise over the channel axis, no affine."""

    def __init__(self, eps=1e-5):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        mean = x.mean(dim=1, keepdim=True)
        var = x.var(dim=1, unbiased=False, keepdim=True)
        return (x - mean) / torch.sqrt(var + self.eps)


class LayerNormNd(nn.Module):
    """Channel-wise LayerNorm with affine parameters on [B, C, ...] tensors (the upstream decoder's norm)."""

    def __init__(self, c, eps=1e-6):
        super().__init__()
        self.weight, self.bias, self.eps = nn.Parameter(torch.ones(c)), nn.Parameter(torch.zeros(c)), eps

    def forward(self, x):
        # (x - mean) / sqrt(var + eps) * w + b over the channel axis, in four passes over the tensor instead of nine
        s, u = torch.var_mean(x, dim=1, keepdim=True, unbiased=False)
        shape = (1, -1) + (1,) * (x.dim() - 2)
        return torch.addcmul(self.bias.view(shape), (x - u) * torch.rsqrt(s + self.eps), self.weight.view(shape))


# spelling -> canonical name of the output normalisation (the strings are the reference's interface, architectures.py:55-86)
_OUT_NORM_ALIASES = {
    **dict.fromkeys(("none", "identity", "off"), "none"),
    **dict.fromkeys(("instance", "instancenorm", "in"), "instance"),
    **dict.fromkeys(("demean", "center"), "demean"),
    **dict.fromkeys(("layernorm", "layer", "ln"), "layernorm"),
    **dict.fromkeys(("layernorm_affine", "layernorm-affine", "ln_affine"), "layernorm_affine"),
}
_OUT_NORM_FACTORY = {
    "none": lambda c, eps: nn.Identity(),
    "instance": lambda c, eps: nn.InstanceNorm3d(c, eps=eps, affine=False),
    "demean": lambda c, eps: ChannelDemean(),
    "layernorm": lambda c, eps: ChannelLayerNorm(eps=eps),
    "layernorm_affine": lambda c, eps: LayerNormNd(c, eps=eps),
}


def build_out_norm(mode, num_classes, eps):
    """Output normalisation selected by name; a bool means instance norm on / off, ``None`` means none (architectures.py:55-86)."""
    if isinstance(mode, bool):
        key = "instance" if mode else "none"
    else:
        key = str(mode).lower() if mode else "none"          # None / "" select no normalisation
    try:
        return _OUT_NORM_FACTORY[_OUT_NORM_ALIASES[key]](num_classes, eps)
    except KeyError:
        raise ValueError(f"unsupported output normalization: {mode!r}") from None


class _ConvNormAct(nn.Module):
    def __init__(self, cin, cout, eps):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 3, padding=1)
        self.norm = nn.InstanceNorm3d(cout, eps=eps, affine=True)

    def forward(self, x):
        return F.leaky_relu(self.norm(self.conv(x)), 0.01)


class _ResidualDown(nn.Module):
    """BasicBlockD with stride 2: conv-IN-LeakyReLU-conv-IN + [AvgPool(2) -> 1x1 conv -> IN], LeakyReLU."""

    def __init__(self, cin, cout, eps):
        super().__init__()
        self.conv1 = nn.Conv3d(cin, cout, 3, stride=2, padding=1)
        self.norm1 = nn.InstanceNorm3d(cout, eps=eps, affine=True)
        self.conv2 = nn.Conv3d(cout, cout, 3, padding=1)
        self.norm2 = nn.InstanceNorm3d(cout, eps=eps, affine=True)
        self.skip = nn.Conv3d(cin, cout, 1, bias=False)
        self.skip_norm = nn.InstanceNorm3d(cout, eps=eps, affine=True)

    def forward(self, x):
        y = self.norm2(self.conv2(F.leaky_relu(self.norm1(self.conv1(x)), 0.01)))
        return F.leaky_relu(y + self.skip_norm(self.skip(F.avg_pool3d(x, 2))), 0.01)


class PatchEmbedDeeper(nn.Module):
    """deep_tokenizer.py:12-68: stem + three stride-2 residual stages + 1x1x1 projection, InstanceNorm eps = ``in_eps``."""

    def __init__(self, input_channels=3, embed_dim=864, base_features=32, depth_per_level=(1, 1, 1), in_eps=1e-5):
        super().__init__()
        if tuple(depth_per_level) != (1, 1, 1):
            raise NotImplementedError("PatchEmbedDeeper: one block per level (the PrimusV2 default) is implemented")
        self.stem = _ConvNormAct(input_channels, base_features, in_eps)
        widths, cin, stages = [base_features * 2 ** k for k in range(3)], base_features, []
        for c in widths:
            stages.append(_ResidualDown(cin, c, in_eps))
            cin = c
        self.stages = nn.Sequential(*stages)
        self.proj = nn.Conv3d(cin, embed_dim, 1)
        self.in_eps = float(in_eps)
        self.train_route = "torch"           # "hip": stem + stages through ``_TokenizerFn`` under autograd (``PrimusV2.train_tokenizer``)

    def tensors(self):
        """The 37 parameters of stem + stages in the order of ``amx_tokenizer_train_forward``'s ``params``."""
        out = [self.stem.conv.weight, self.stem.conv.bias, self.stem.norm.weight, self.stem.norm.bias]
        for st in self.stages:
            out += [st.conv1.weight, st.conv1.bias, st.norm1.weight, st.norm1.bias, st.conv2.weight, st.conv2.bias, st.norm2.weight,
                    st.norm2.bias, st.skip.weight, st.skip_norm.weight, st.skip_norm.bias]
        return out

    def unsupported_reason(self, x):
        """None when ``_TokenizerFn`` covers this module and input, else why not."""
        if x.requires_grad:
            return "the input requires a gradient: amx_tokenizer_backward computes none for it"
        if not x.is_cuda:
            return "the input is a CPU tensor: the tokenizer kernels have no host path"
        if self.stem.conv.in_channels != 1 or self.stem.conv.out_channels != 32 or len(self.stages) != 3:
            return "depth_per_level (1, 1, 1), one input channel and base width 32 are what the kernels cover"
        if x.dim() != 5 or x.shape[1] != 1:
            return f"the input {tuple(x.shape)} is not [N, 1, D, H, W]"
        n, _, D, H, W = x.shape
        with torch.cuda.device(x.device):
            if _lib.load().amx_tokenizer_train_saved_bytes(n, D, H, W) == 0:
                return (f"n = {n}, {D} x {H} x {W} is outside the envelope (W a multiple of 16, D and H of 8, a multiple of 64 tokens, "
                        "at most 2^22 voxels in all)")
        return None

    def forward(self, x):
        if self.train_route == "hip" and torch.is_grad_enabled() and self.unsupported_reason(x) is None:
            return self.proj(_TokenizerFn.apply(x, self.in_eps, *self.tensors()))
        return self.proj(self.stages(self.stem(x)))


class PatchDecode(nn.Module):
    def __init__(self, patch_size, embed_dim, out_channels):
        super().__init__()
        nst = int(round(math.log2(max(patch_size))))
        red = (embed_dim / (2 * out_channels)) ** (1.0 / nst)
        r8 = lambda v: int(max(8, round((v + 1e-6) / 8) * 8))
        ch = [embed_dim] + [r8(embed_dim / red ** (k + 1)) for k in range(nst)]
        ch[-1] = out_channels
        stages = [nn.Sequential(nn.ConvTranspose3d(ch[k], ch[k + 1], 2, stride=2), LayerNormNd(ch[k + 1]), nn.GELU())
                  for k in range(nst - 1)]
        stages.append(nn.ConvTranspose3d(ch[-2], ch[-1], 2, stride=2))
        self.decode = nn.Sequential(*stages)

    def forward(self, x):
        return self.decode(x)


def build_rope_table(grid, head_dim, temperature=10000.0):
    """[N, 2 * head_dim] fp32: per token [sin | cos], each band repeated for its (even, odd) channel pair."""
    nb = head_dim // (2 * len(grid))
    bands = 1.0 / (temperature ** (torch.arange(nb, dtype=torch.float64) / nb))
    axes = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in grid], indexing="ij")
    ang = (torch.stack(axes, dim=-1).reshape(-1, len(grid), 1) * bands).reshape(-1, len(grid) * nb)
    return torch.cat((ang.sin().repeat_interleave(2, -1), ang.cos().repeat_interleave(2, -1)), -1).float()


def _rope(x, table):
    hd = x.shape[-1]
    rot = torch.stack((-x[..., 1::2], x[..., ::2]), -1).reshape(x.shape)
    return x * table[:, hd:] + rot * table[:, :hd]


TRAIN_CORES = ("torch", "hip")
_train_scratch_cache = {}


def _train_scratch(nb, dev):
    """One scratch buffer per device for every block's training calls: a call leaves nothing in it that a later call reads (the
    backward re-runs the preparation), and the calls of one autograd pass are ordered on the stream."""
    buf = _train_scratch_cache.get(dev)
    if buf is None or buf.numel() < nb:
        buf = _train_scratch_cache[dev] = torch.empty(nb, dtype=torch.uint8, device=dev)
    return buf


class _AttentionCoreFn(torch.autograd.Function):
    """The attention core under autograd on the library's own kernels: ``amx_attention_qknorm_rope_train`` forward (the no-grad
    core's output bit for bit, plus the log-sum-exp), ``amx_attention_backward`` backward (csrc/amx_attention_bwd.hip).  Saved:
    q, k, v, the output, the log-sum-exp [B, heads, N], the norm parameters and the rotary table -- no N x N tensor."""

    @staticmethod
    def forward(ctx, q, k, v, qn_w, qn_b, kn_w, kn_b, table, n_prefix, heads, eps):
        lib = _lib.load()
        B, N, E = q.shape
        hd, dev = E // heads, q.device
        out = torch.empty_like(q)
        lse = torch.empty(B, heads, N, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            nb = lib.amx_attention_train_scratch_bytes(B, heads, N, hd)
            if nb == 0:
                raise _lib.AmxError(f"attention: unsupported shape (heads {heads}, head_dim {hd})")
            scratch = _train_scratch(nb, dev)
            _lib.check(lib.amx_attention_qknorm_rope_train(
                _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(qn_w), _lib.ptr(qn_b), _lib.ptr(kn_w), _lib.ptr(kn_b), float(eps),
                _lib.ptr(table), int(n_prefix), B, N, heads, hd, _lib.ptr(out), _lib.ptr(lse), _lib.ptr(scratch), nb,
                _lib.stream(dev)))
        ctx.save_for_backward(q, k, v, out, lse, qn_w, qn_b, kn_w, kn_b, table)
        ctx.cfg = (int(n_prefix), int(heads), float(eps))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, qn_w, qn_b, kn_w, kn_b, table = ctx.saved_tensors
        n_prefix, heads, eps = ctx.cfg
        lib = _lib.load()
        B, N, E = q.shape
        hd, dev = E // heads, q.device
        dout = _lib.f32c(dout)
        need = ctx.needs_input_grad
        new = lambda like, on: torch.empty_like(like) if on else None
        dq, dk, dv = new(q, need[0]), new(k, need[1]), new(v, need[2])
        dnorm = [new(p, p is not None and need[3 + i]) for i, p in enumerate((qn_w, qn_b, kn_w, kn_b))]
        with torch.cuda.device(dev):
            nb = lib.amx_attention_train_scratch_bytes(B, heads, N, hd)
            scratch = _train_scratch(nb, dev)
            _lib.check(lib.amx_attention_backward(
                _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(qn_w), _lib.ptr(qn_b), _lib.ptr(kn_w), _lib.ptr(kn_b), eps,
                _lib.ptr(table), n_prefix, B, N, heads, hd, _lib.ptr(out), _lib.ptr(lse), _lib.ptr(dout), _lib.ptr(dq), _lib.ptr(dk),
                _lib.ptr(dv), *[_lib.ptr(t) for t in dnorm], _lib.ptr(scratch), nb, _lib.stream(dev)))
        return (dq, dk, dv, *dnorm, None, None, None, None)


class _LinearFn(torch.autograd.Function):
    """``F.linear(x, weight, bias)`` under autograd on the library's own kernels (csrc/amx_linear_bwd.hip): ``amx_linear_forward``
    forward, ``amx_linear_backward`` backward (dx, dW and db in one call; gradients nobody needs are passed as null).  Every
    operand is rounded once to f16, every sum is fp32.  Saved: the fp32 ``x`` and ``weight`` -- no f16 copy is kept."""

    @staticmethod
    def _scratch(lib, M, K, N, dev):
        nb = lib.amx_linear_train_scratch_bytes(M, K, N)
        if nb == 0:
            raise _lib.AmxError(f"linear: (M, K, N) = ({M}, {K}, {N}) is outside the envelope of amx_linear_forward "
                                "(K and N multiples of 4, M * max(K, N) < 2^31)")
        return _train_scratch(nb, dev), nb

    @staticmethod
    def forward(ctx, x, weight, bias):
        lib = _lib.load()
        N, K = weight.shape
        dev = x.device
        xc, w, b = _lib.f32c(x), _lib.f32c(weight), None if bias is None else _lib.f32c(bias)
        M = xc.numel() // K
        y = torch.empty(*x.shape[:-1], N, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            scratch, nb = _LinearFn._scratch(lib, M, K, N, dev)
            _lib.check(lib.amx_linear_forward(_lib.ptr(xc), _lib.ptr(w), _lib.ptr(b), M, K, N, _lib.ptr(y), _lib.ptr(scratch), nb,
                                              _lib.stream(dev)))
        ctx.save_for_backward(xc, w)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        lib = _lib.load()
        N, K = w.shape
        M, dev = x.numel() // K, x.device
        dy = _lib.f32c(dy)
        need = ctx.needs_input_grad
        dx = torch.empty_like(x) if need[0] else None
        dw = torch.empty_like(w) if need[1] else None
        db = torch.empty(N, dtype=torch.float32, device=dev) if ctx.has_bias and need[2] else None
        with torch.cuda.device(dev):
            scratch, nb = _LinearFn._scratch(lib, M, K, N, dev)
            _lib.check(lib.amx_linear_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(dy), M, K, N, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                               _lib.ptr(scratch), nb, _lib.stream(dev)))
        return dx, dw, db


class _LayerNormFn(torch.autograd.Function):
    """``F.layer_norm(x, (C,), w, b, eps)`` over the last axis under autograd on the library's own kernels
    (csrc/amx_layernorm_train.hip): ``amx_layernorm_train_forward`` forward, ``amx_layernorm_backward`` backward (dx, dw and db in one
    call; gradients nobody needs are passed as null).  fp32 throughout.  Saved: ``x``, ``w`` and the rows' mean and rstd [M] -- nothing
    else of width C; the backward recomputes the normalised rows."""

    @staticmethod
    def _scratch(lib, M, C, dev):
        nb = lib.amx_layernorm_train_scratch_bytes(M, C)
        if nb == 0:
            raise _lib.AmxError(f"layernorm: (M, C) = ({M}, {C}) is outside the envelope of amx_layernorm_train_forward "
                                "(C a multiple of 4, 8 <= C <= 4096, M * C < 2^31)")
        return _train_scratch(nb, dev), nb

    @staticmethod
    def _forward(ctx, gate, x, w, b, eps):
        lib = _lib.load()
        C, dev = x.shape[-1], x.device
        xc, wc, bc = _lib.f32c(x), _lib.f32c(w), _lib.f32c(b)
        gc = None if gate is None else _lib.f32c(gate)
        M = xc.numel() // C
        _LayerNormFn._scratch(lib, M, C, dev)          # the envelope, before anything is allocated
        y = torch.empty_like(xc)
        mean, rstd = torch.empty(M, dtype=torch.float32, device=dev), torch.empty(M, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.amx_layernorm_train_forward(_lib.ptr(xc), _lib.ptr(gc), _lib.ptr(wc), _lib.ptr(bc), float(eps), M, C, _lib.ptr(y),
                                                       _lib.ptr(mean), _lib.ptr(rstd), _lib.stream(dev)))
        if gate is None:
            ctx.save_for_backward(xc, wc, mean, rstd)
        else:
            ctx.save_for_backward(xc, wc, mean, rstd, gc)
        return y

    @staticmethod
    def _backward(ctx, dy, need_gate, need_x, need_w, need_b):
        x, w, mean, rstd, *rest = ctx.saved_tensors
        gate = rest[0] if rest else None
        lib = _lib.load()
        C, dev = x.shape[-1], x.device
        M = x.numel() // C
        dy = _lib.f32c(dy)
        dx = torch.empty_like(x) if need_x else None
        dgate = torch.empty_like(gate) if need_gate else None
        dw = torch.empty_like(w) if need_w else None
        db = torch.empty_like(w) if need_b else None
        with torch.cuda.device(dev):
            scratch, nb = _LayerNormFn._scratch(lib, M, C, dev)
            _lib.check(lib.amx_layernorm_backward(_lib.ptr(x), _lib.ptr(gate), _lib.ptr(w), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(dy), M, C,
                                                  _lib.ptr(dx), _lib.ptr(dgate), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(scratch), nb,
                                                  _lib.stream(dev)))
        return dgate, dx, dw, db

    @staticmethod
    def forward(ctx, x, w, b, eps):
        return _LayerNormFn._forward(ctx, None, x, w, b, eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        need = ctx.needs_input_grad
        return (*_LayerNormFn._backward(ctx, dy, False, need[0], need[1], need[2])[1:], None)


class _GatedLayerNormFn(torch.autograd.Function):
    """``F.layer_norm(F.silu(gate) * x, (C,), w, b, eps)`` -- the SwiGLU product and ``mlp.norm`` -- through the same two entries with
    their gate argument: the product is formed in registers and never stored.  Saved: ``gate``, ``x``, ``w``, mean and rstd."""

    @staticmethod
    def forward(ctx, gate, x, w, b, eps):
        if gate.shape != x.shape:
            raise ValueError(f"gated layernorm: gate {tuple(gate.shape)} and x {tuple(x.shape)} differ")
        return _LayerNormFn._forward(ctx, gate, x, w, b, eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        need = ctx.needs_input_grad
        return (*_LayerNormFn._backward(ctx, dy, need[0], need[1], need[2], need[3]), None)


class _TokenizerFn(torch.autograd.Function):
    """Stem + the three residual stages of ``PatchEmbedDeeper`` under autograd on the library's own kernels
    (csrc/amx_tokenizer_bwd.hip): ``amx_tokenizer_train_forward`` returns h3, the input of ``proj``, and fills ``saved`` -- a tensor
    this node owns, not scratch -- with the raw conv outputs, the norm statistics and the hi + lo activation planes;
    ``amx_tokenizer_backward`` writes the 37 parameter gradients (those nobody needs are passed as null).  No gradient for ``x``."""

    @staticmethod
    def _sizes(lib, shape):
        n, _, D, H, W = shape
        sb, nb = lib.amx_tokenizer_train_saved_bytes(n, D, H, W), lib.amx_tokenizer_train_scratch_bytes(n, D, H, W)
        if sb == 0:
            raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"tokenizer: input {tuple(shape)} is outside the envelope of amx_tokenizer_train_forward")
        return (n, D, H, W), sb, nb

    @staticmethod
    def forward(ctx, x, eps, *params):
        lib = _lib.load()
        dev = x.device
        xc, held = _lib.f32c(x.detach()), [_lib.f32c(p.detach()) for p in params]
        with torch.cuda.device(dev):
            dims, sb, nb = _TokenizerFn._sizes(lib, xc.shape)
            n, D, H, W = dims
            h3 = torch.empty(n, 128, D // 8, H // 8, W // 8, dtype=torch.float32, device=dev)
            saved = torch.empty(sb, dtype=torch.uint8, device=dev)
            scratch = _train_scratch(nb, dev)
            arr = (ctypes.c_void_p * len(held))(*[t.data_ptr() for t in held])
            _lib.check(lib.amx_tokenizer_train_forward(_lib.ptr(xc), arr, *dims, float(eps), _lib.ptr(h3), _lib.ptr(saved), sb, _lib.ptr(scratch), nb,
                                                       _lib.stream(dev)))
        ctx.save_for_backward(xc, saved, *held)
        ctx.eps = float(eps)
        return h3

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dh3):
        xc, saved, *held = ctx.saved_tensors
        lib = _lib.load()
        dev = xc.device
        need = ctx.needs_input_grad
        grads = [torch.empty_like(t) if need[2 + i] else None for i, t in enumerate(held)]
        with torch.cuda.device(dev):
            dims, sb, nb = _TokenizerFn._sizes(lib, xc.shape)
            scratch = _train_scratch(nb, dev)
            arr = (ctypes.c_void_p * len(held))(*[t.data_ptr() for t in held])
            garr = (ctypes.c_void_p * len(held))(*[None if g is None else g.data_ptr() for g in grads])
            _lib.check(lib.amx_tokenizer_backward(_lib.ptr(_lib.f32c(dh3)), _lib.ptr(xc), arr, _lib.ptr(saved), *dims, ctx.eps, garr, _lib.ptr(scratch), nb,
                                                  _lib.stream(dev)))
        return (None, None, *grads)


_DECODE_ROWS_MAX_WIDTH, _DECODE_ROWS_MAX_OUT, _DECODE_ROWS_MAX_ROWS = 1056, 64, 1 << 20          # the envelope of amx_vit_decode_rows_* (include/anatomix_amd.h)


def _decoder_stages(decoder):
    """``(convs, norms)`` of a three-stage PatchDecode -- what both decoder routes of the library restate -- or a string: why these
    modules are something else."""
    mods = list(decoder.decode)
    if len(mods) != 3 or not all(isinstance(m, nn.Sequential) and len(m) == 3 for m in mods[:2]):
        return "the decoder is not three stages (patch size 8)"
    convs, norms = [mods[0][0], mods[1][0], mods[2]], [mods[0][1], mods[1][1]]
    if not all(isinstance(c, nn.ConvTranspose3d) and c.kernel_size == (2, 2, 2) and c.stride == (2, 2, 2) for c in convs):
        return "the decoder's stages are not ConvTranspose3d(kernel 2, stride 2)"
    if not all(isinstance(n, LayerNormNd) for n in norms) or norms[0].eps != norms[1].eps:
        return "the decoder's norms are not LayerNormNd with one eps"
    if not all(isinstance(m[2], nn.GELU) and m[2].approximate == "none" for m in mods[:2]):
        return "the decoder's activations are not the erf GELU"
    return convs, norms


def _decode_rows_parts(decoder, out_norm):
    """``(tensors, ln_eps, mode, out_eps)`` of a PatchDecode + output norm as ``amx_vit_decode_rows_*`` takes them -- the twelve
    parameter tensors {W1, b1, ln1.w, ln1.b, W2, b2, ln2.w, ln2.b, W3, b3, out.w, out.b} (None where absent) -- or a string: why the
    rows route does not cover these modules."""
    stages = _decoder_stages(decoder)
    if isinstance(stages, str):
        return stages
    convs, norms = stages
    if isinstance(out_norm, LayerNormNd):
        mode, tail, out_eps = 2, [out_norm.weight, out_norm.bias], out_norm.eps
    elif isinstance(out_norm, ChannelLayerNorm):
        mode, tail, out_eps = 1, [None, None], out_norm.eps
    elif out_norm is None or isinstance(out_norm, nn.Identity):
        mode, tail, out_eps = 0, [None, None], 0.0
    else:
        return f"the output norm {type(out_norm).__name__} needs spatial statistics of the dense volume"
    widths = [convs[0].in_channels] + [c.out_channels for c in convs]
    if max(widths[:3]) > _DECODE_ROWS_MAX_WIDTH or widths[3] > _DECODE_ROWS_MAX_OUT:
        return (f"decoder widths {widths} are outside the envelope (up to {_DECODE_ROWS_MAX_WIDTH}, output channels up to "
                f"{_DECODE_ROWS_MAX_OUT})")
    tensors = [convs[0].weight, convs[0].bias, norms[0].weight, norms[0].bias, convs[1].weight, convs[1].bias, norms[1].weight,
               norms[1].bias, convs[2].weight, convs[2].bias] + tail
    return tensors, float(norms[0].eps), mode, float(out_eps)


class _DecodeRowsFn(torch.autograd.Function):
    """The patch decoder (+ a per-voxel output norm) at sampled voxels under autograd on the library's own kernels
    (csrc/amx_vit_decode_rows.hip): rows [N, P, C] from tokens [N, T, E] and coordinates [P, 3], all fp32.  Saved: the tokens, the
    coordinates and the parameters -- the backward call re-runs the forward passes into the shared training scratch (a call leaves
    nothing there that a later call reads)."""

    @staticmethod
    def _call(lib, entry, tokens, coords, grid, params, widths, ln_eps, mode, out_eps, extra):
        dev = tokens.device
        N, P = tokens.shape[0], coords.shape[0]
        with torch.cuda.device(dev):
            nb = lib.amx_vit_decode_rows_scratch_bytes(N, P, *widths)
            if nb == 0:
                raise _lib.AmxError(_lib.AMX_ERR_SHAPE, f"decode rows: views {N}, rows {P}, widths {tuple(widths)} are outside the envelope of "
                                    f"amx_vit_decode_rows_forward (widths up to {_DECODE_ROWS_MAX_WIDTH}, output channels up to "
                                    f"{_DECODE_ROWS_MAX_OUT}, views x rows up to 2^20)")
            scratch = _train_scratch(nb, dev)
            arr = (ctypes.c_void_p * 12)(*[None if t is None else t.data_ptr() for t in params])
            _lib.check(entry(_lib.ptr(tokens), _lib.ptr(coords), arr, N, P, *grid, *widths, ln_eps, mode, out_eps, *extra, _lib.ptr(scratch), nb,
                             _lib.stream(dev)))

    @staticmethod
    def forward(ctx, tokens, coords, grid, ln_eps, mode, out_eps, *params):
        lib = _lib.load()
        tok = _lib.f32c(tokens)
        held = [None if t is None else _lib.f32c(t) for t in params]
        widths = (held[0].shape[0], held[0].shape[1], held[4].shape[1], held[8].shape[1])
        rows = torch.empty(tok.shape[0], coords.shape[0], widths[3], dtype=torch.float32, device=tok.device)
        _DecodeRowsFn._call(lib, lib.amx_vit_decode_rows_forward, tok, coords, grid, held, widths, ln_eps, mode, out_eps, (_lib.ptr(rows),))
        ctx.save_for_backward(tok, coords, *[t for t in held if t is not None])
        ctx.present = [t is not None for t in held]
        ctx.cfg = (tuple(grid), widths, ln_eps, mode, out_eps)
        return rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, drows):
        tok, coords, *rest = ctx.saved_tensors
        it = iter(rest)
        held = [next(it) if on else None for on in ctx.present]
        grid, widths, ln_eps, mode, out_eps = ctx.cfg
        need = ctx.needs_input_grad
        dtok = torch.empty_like(tok) if need[0] else None
        grads = [torch.empty_like(t) if t is not None and need[6 + i] else None for i, t in enumerate(held)]
        garr = (ctypes.c_void_p * 12)(*[None if g is None else g.data_ptr() for g in grads])
        lib = _lib.load()
        _DecodeRowsFn._call(lib, lib.amx_vit_decode_rows_backward, tok, coords, grid, held, widths, ln_eps, mode, out_eps,
                            (_lib.ptr(_lib.f32c(drows)), _lib.ptr(dtok), garr))
        return (dtok, None, None, None, None, None, *grads)


def decode_rows(tokens, coords, decoder, out_norm=None, grid=None, check_coords=True):
    """``out_norm(decoder(tokens as a volume))[:, :, z, y, x]`` as rows [N, P, C] for the voxels ``coords`` (int64 [P, 3] as (z, y, x),
    shared by the N views) without the volume: ``tokens`` fp32 [N, T, E] on a GPU, T = prod(grid) in C order, ``decoder`` a
    ``PatchDecode`` of patch size 8, ``out_norm`` None / Identity / ``ChannelLayerNorm`` / ``LayerNormNd``.  Differentiable in the
    tokens and every parameter.  ``check_coords``: refuse coordinates outside the volume here (one host read; the kernels clamp
    whatever they are given) -- for coordinates a caller supplies."""
    parts = _decode_rows_parts(decoder, out_norm)
    if isinstance(parts, str):
        raise _lib.AmxError(_lib.AMX_ERR_SHAPE, f"decode rows: {parts}")
    tensors, ln_eps, mode, out_eps = parts
    grid = tuple(int(g) for g in grid)
    if not tokens.is_cuda:
        raise RuntimeError("decode rows: the rows route runs on the GPU and has no host path")
    if tokens.dim() != 3 or tokens.shape[1] != grid[0] * grid[1] * grid[2] or tokens.shape[2] != tensors[0].shape[0]:
        raise ValueError(f"decode rows: tokens {tuple(tokens.shape)} do not match the grid {grid} and the width {tensors[0].shape[0]}")
    if coords.dim() != 2 or coords.shape[1] != 3 or coords.dtype != torch.int64 or coords.shape[0] < 1:
        raise ValueError(f"decode rows: coordinates are int64 [P, 3] (got {coords.dtype} {tuple(coords.shape)})")
    if check_coords:
        lo, hi = coords.amin(0).tolist(), coords.amax(0).tolist()
        if min(lo) < 0 or any(h >= 8 * g for h, g in zip(hi, grid)):
            raise ValueError(f"decode rows: coordinates span {lo} .. {hi}, outside the volume {tuple(8 * g for g in grid)}")
    coords = coords.to(tokens.device).contiguous()
    return _DecodeRowsFn.apply(tokens, coords, grid, ln_eps, mode, out_eps, *tensors)


_DECODER_NORM_MODES = {"none": 0, "demean": 1, "instance": 2}          # out_norm of amx_vit_decoder_train_forward (include/anatomix_amd.h)


def _decoder_train_parts(decoder, out_norm):
    """``(tensors, ln_eps, mode, out_eps, tail)`` of a PatchDecode + output norm as ``amx_vit_decoder_train_forward`` takes them -- the
    ten parameter tensors {W1, b1, ln1.w, ln1.b, W2, b2, ln2.w, ln2.b, W3, b3}, the output norm the call applies itself (none /
    demean / instance) and ``tail``, the torch module that runs on the call's output (a per-voxel norm; None otherwise) -- or a
    string: why the dense route does not cover the decoder.  No output norm is a reason."""
    stages = _decoder_stages(decoder)
    if isinstance(stages, str):
        return stages
    convs, norms = stages
    mode, out_eps, tail = 0, 0.0, None
    if isinstance(out_norm, ChannelDemean):
        mode = _DECODER_NORM_MODES["demean"]
    elif isinstance(out_norm, nn.InstanceNorm3d) and not out_norm.affine and not out_norm.track_running_stats:
        mode, out_eps = _DECODER_NORM_MODES["instance"], out_norm.eps
    elif out_norm is not None and not isinstance(out_norm, nn.Identity):
        tail = out_norm
    tensors = [convs[0].weight, convs[0].bias, norms[0].weight, norms[0].bias, convs[1].weight, convs[1].bias, norms[1].weight,
               norms[1].bias, convs[2].weight, convs[2].bias]
    return tensors, float(norms[0].eps), mode, float(out_eps), tail


class _DecoderFn(torch.autograd.Function):
    """The dense patch decoder and a spatial output norm under autograd on the library's own kernels (csrc/amx_vit_decode_train.hip):
    tokens [N, T, E] -> the planar fp32 volume [N, C, 8 gd, 8 gh, 8 gw] of ``out_norm(decoder(tokens as a volume))`` for the modes
    none / demean / instance, all fp32 (products on the f32-input MFMA).  ``amx_vit_decoder_train_forward`` fills ``saved`` -- a
    tensor this node owns, not scratch -- with the raw stage outputs and the norm statistics; ``amx_vit_decoder_backward`` writes
    ``d_tokens`` and the ten parameter gradients (those nobody needs are passed as null).  Saved besides: the tokens, the parameters
    and, for the instance norm, the output."""

    @staticmethod
    def _sizes(lib, n, grid, widths):
        sb, nb = lib.amx_vit_decoder_train_saved_bytes(n, *grid, *widths), lib.amx_vit_decoder_train_scratch_bytes(n, *grid, *widths)
        if sb == 0:
            raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"decoder: views {n}, token grid {tuple(grid)}, widths {tuple(widths)} are outside "
                                        "the envelope of amx_vit_decoder_train_forward")
        return sb, nb

    @staticmethod
    def forward(ctx, tokens, grid, ln_eps, mode, out_eps, *params):
        lib = _lib.load()
        dev = tokens.device
        tok = _lib.f32c(tokens.detach())
        held = [None if t is None else _lib.f32c(t.detach()) for t in params]
        widths = (held[0].shape[0], held[0].shape[1], held[4].shape[1], held[8].shape[1])
        grid = tuple(int(g) for g in grid)
        n = tok.shape[0]
        if tok.dim() != 3 or tok.shape[1] != grid[0] * grid[1] * grid[2] or tok.shape[2] != widths[0]:
            raise ValueError(f"decoder: tokens {tuple(tok.shape)} do not match the grid {grid} and the width {widths[0]}")
        with torch.cuda.device(dev):
            sb, nb = _DecoderFn._sizes(lib, n, grid, widths)
            out = torch.empty(n, widths[3], *(8 * g for g in grid), dtype=torch.float32, device=dev)
            saved = torch.empty(sb, dtype=torch.uint8, device=dev)
            scratch = _train_scratch(nb, dev)
            arr = (ctypes.c_void_p * 10)(*[None if t is None else t.data_ptr() for t in held])
            _lib.check(lib.amx_vit_decoder_train_forward(_lib.ptr(tok), arr, n, *grid, *widths, float(ln_eps), int(mode), float(out_eps),
                                                         _lib.ptr(out), _lib.ptr(saved), sb, _lib.ptr(scratch), nb, _lib.stream(dev)))
        ctx.save_for_backward(tok, saved, *([out] if mode == _DECODER_NORM_MODES["instance"] else []), *[t for t in held if t is not None])
        ctx.present = [t is not None for t in held]
        ctx.cfg = (grid, widths, float(ln_eps), int(mode), float(out_eps))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        grid, widths, ln_eps, mode, out_eps = ctx.cfg
        tok, saved, *rest = ctx.saved_tensors
        out = rest.pop(0) if mode == _DECODER_NORM_MODES["instance"] else None
        it = iter(rest)
        held = [next(it) if on else None for on in ctx.present]
        lib = _lib.load()
        dev = tok.device
        need = ctx.needs_input_grad
        dtok = torch.empty_like(tok) if need[0] else None
        grads = [torch.empty_like(t) if t is not None and need[5 + i] else None for i, t in enumerate(held)]
        with torch.cuda.device(dev):
            sb, nb = _DecoderFn._sizes(lib, tok.shape[0], grid, widths)
            scratch = _train_scratch(nb, dev)
            arr = (ctypes.c_void_p * 10)(*[None if t is None else t.data_ptr() for t in held])
            garr = (ctypes.c_void_p * 10)(*[None if g is None else g.data_ptr() for g in grads])
            _lib.check(lib.amx_vit_decoder_backward(_lib.ptr(_lib.f32c(dout)), _lib.ptr(out), _lib.ptr(tok), arr, _lib.ptr(saved), sb, tok.shape[0],
                                                    *grid, *widths, ln_eps, mode, out_eps, _lib.ptr(dtok), garr, _lib.ptr(scratch), nb,
                                                    _lib.stream(dev)))
        return (dtok, None, None, None, None, *grads)


def decode_dense(tokens, decoder, out_norm=None, grid=None):
    """``out_norm(decoder(tokens as a volume))`` [N, C, 8 gd, 8 gh, 8 gw] through ``_DecoderFn``: ``tokens`` fp32 [N, T, E] on a GPU,
    T = prod(grid) in C order, ``decoder`` a ``PatchDecode`` of patch size 8.  none / demean / instance run inside the call; any
    other output norm module runs on the call's output.  Differentiable in the tokens and every parameter."""
    parts = _decoder_train_parts(decoder, out_norm)
    if isinstance(parts, str):
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"decoder: {parts}")
    if not tokens.is_cuda:
        raise RuntimeError("decoder: the dense route runs on the GPU and has no host path")
    tensors, ln_eps, mode, out_eps, tail = parts
    vol = _DecoderFn.apply(tokens, tuple(int(g) for g in grid), ln_eps, mode, out_eps, *tensors)
    return vol if tail is None else tail(vol)


def _linear(layer, x, route):
    """``layer(x)`` for an nn.Linear: through ``_LinearFn`` when the route is "hip", the input is on a GPU and autograd is on."""
    if route == "hip" and x.is_cuda and torch.is_grad_enabled():
        return _LinearFn.apply(x, layer.weight, layer.bias)
    return layer(x)


def _norm_on_hip(layer, x, route):
    """Whether a token LayerNorm of ``x`` takes the library's kernels: the route is "hip", the input is on a GPU, autograd is on, the
    layer is an affine nn.LayerNorm over the last axis and the rows are inside the envelope of ``amx_layernorm_train_forward``."""
    if not (route == "hip" and x.is_cuda and torch.is_grad_enabled() and isinstance(layer, nn.LayerNorm)):
        return False
    if layer.weight is None or layer.bias is None or tuple(layer.normalized_shape) != (x.shape[-1],) or x.numel() == 0:
        return False
    return _lib.load().amx_layernorm_train_scratch_bytes(x.numel() // x.shape[-1], x.shape[-1]) != 0


def _layer_norm(layer, x, route):
    """``layer(x)`` for an nn.LayerNorm over the tokens' last axis: through ``_LayerNormFn`` where ``_norm_on_hip`` says so, else the
    module itself (CPU tensors, ``torch.no_grad()``, widths outside the envelope, an nn.Identity in its place)."""
    if _norm_on_hip(layer, x, route):
        return _LayerNormFn.apply(x, layer.weight, layer.bias, layer.eps)
    return layer(x)


class EvaAttention(nn.Module):
    def __init__(self, dim, num_heads, qk_norm, scale_attn_inner):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(dim, dim), nn.Linear(dim, dim, bias=False), nn.Linear(dim, dim)
        self.q_norm = nn.LayerNorm(self.head_dim) if qk_norm else None        # architectures.py:108-115
        self.k_norm = nn.LayerNorm(self.head_dim) if qk_norm else None
        self.norm = nn.LayerNorm(dim) if scale_attn_inner else nn.Identity()
        self.proj = nn.Linear(dim, dim)
        self._scratch = None
        # the core under autograd on a GPU: "torch" (F.scaled_dot_product_attention and torch's autograd) or "hip" (_AttentionCoreFn)
        self.train_core = "torch"
        # the four linears under autograd on a GPU: "torch" (nn.Linear) or "hip" (_LinearFn)
        self.train_linear = "torch"
        # ``norm`` (the scale_attn_inner LayerNorm) under autograd on a GPU: "torch" (the module) or "hip" (_LayerNormFn)
        self.train_norm = "torch"

    def core_hip_train(self, q, k, v, table, n_prefix):
        """``core_hip`` as a differentiable function of q, k, v and the norm parameters (fp32 contiguous CUDA tensors)."""
        qn, kn = self.q_norm, self.k_norm
        return _AttentionCoreFn.apply(q, k, v, qn.weight if qn else None, qn.bias if qn else None, kn.weight if qn else None,
                                      kn.bias if qn else None, table, n_prefix, self.num_heads, qn.eps if qn else 1e-5)

    def core_hip(self, q, k, v, table, n_prefix):
        """q, k, v fp32 [B, N, E] -> attention output [B, N, E]: one C-ABI call."""
        lib = _lib.load()
        B, N, E = q.shape
        dev = q.device
        out = torch.empty_like(q)
        with torch.cuda.device(dev):
            nb = lib.amx_attention_scratch_bytes(B, self.num_heads, N, self.head_dim)
            if nb == 0:
                raise _lib.AmxError(f"attention: unsupported shape (heads {self.num_heads}, head_dim {self.head_dim})")
            if self._scratch is None or self._scratch.numel() < nb or self._scratch.device != dev:
                self._scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
            qn = self.q_norm
            st = _lib.stream(dev)
            _lib.check(lib.amx_attention_qknorm_rope(
                _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), _lib.ptr(qn.weight if qn else None), _lib.ptr(qn.bias if qn else None),
                _lib.ptr(self.k_norm.weight if qn else None), _lib.ptr(self.k_norm.bias if qn else None),
                float(qn.eps if qn else 1e-5), _lib.ptr(table), int(n_prefix), B, N, self.num_heads, self.head_dim, _lib.ptr(out),
                _lib.ptr(self._scratch), nb, st))
        return out

    def core_torch(self, q, k, v, table, n_prefix):
        B, N, E = q.shape
        sh = lambda t: t.reshape(B, N, self.num_heads, self.head_dim).transpose(1, 2)
        q, k, v = sh(q), sh(k), sh(v)
        if self.q_norm is not None:
            q, k = self.q_norm(q), self.k_norm(k)
        if table is not None:
            q = torch.cat((q[:, :, :n_prefix], _rope(q[:, :, n_prefix:], table)), 2)
            k = torch.cat((k[:, :, :n_prefix], _rope(k[:, :, n_prefix:], table)), 2)
        return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, E)

    def forward(self, x, table, n_prefix):
        lin = self.train_linear
        q, k, v = _linear(self.q_proj, x, lin), _linear(self.k_proj, x, lin), _linear(self.v_proj, x, lin)
        if x.is_cuda and not torch.is_grad_enabled():          # the kernel takes fp32 (under the f16 mode the linears hand over halves)
            y = self.core_hip(q.float().contiguous(), k.float().contiguous(), v.float().contiguous(), table, n_prefix)
        elif x.is_cuda and self.train_core == "hip":
            y = self.core_hip_train(q.float().contiguous(), k.float().contiguous(), v.float().contiguous(), table, n_prefix)
        else:
            y = self.core_torch(q, k, v, table, n_prefix)
        return _linear(self.proj, _layer_norm(self.norm, y, self.train_norm), lin)


class SwiGLU(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1_g, self.fc1_x = nn.Linear(dim, hidden), nn.Linear(dim, hidden)
        self.norm = nn.LayerNorm(hidden, eps=1e-6)
        self.fc2 = nn.Linear(hidden, dim)
        self.train_linear = "torch"          # as EvaAttention.train_linear
        self.train_norm = "torch"            # "hip": the gate product and ``norm`` through ``_GatedLayerNormFn``

    def forward(self, x):
        lin = self.train_linear
        g, h = _linear(self.fc1_g, x, lin), _linear(self.fc1_x, x, lin)
        if _norm_on_hip(self.norm, h, self.train_norm):
            h = _GatedLayerNormFn.apply(g, h, self.norm.weight, self.norm.bias, self.norm.eps)
        else:
            h = self.norm(F.silu(g) * h)
        return _linear(self.fc2, h, lin)


class EvaBlock(nn.Module):
    def __init__(self, dim, num_heads, hidden, init_values, qk_norm, scale_attn_inner):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = EvaAttention(dim, num_heads, qk_norm, scale_attn_inner)
        self.gamma_1 = nn.Parameter(init_values * torch.ones(dim)) if init_values is not None else None
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = SwiGLU(dim, hidden)
        self.gamma_2 = nn.Parameter(init_values * torch.ones(dim)) if init_values is not None else None
        self.train_norm = "torch"            # norm1 / norm2 under autograd on a GPU: "torch" (the modules) or "hip" (_LayerNormFn)

    def forward(self, x, table, n_prefix):
        a = self.attn(_layer_norm(self.norm1, x, self.train_norm), table, n_prefix)
        x = x + (a if self.gamma_1 is None else self.gamma_1 * a)
        m = self.mlp(_layer_norm(self.norm2, x, self.train_norm))
        return x + (m if self.gamma_2 is None else self.gamma_2 * m)


class Eva(nn.Module):
    def __init__(self, dim, depth, num_heads, grid, hidden, init_values, qk_norm, scale_attn_inner):
        super().__init__()
        self.pos_embed = nn.Parameter(torch.zeros(1, int(torch.tensor(grid).prod()), dim))
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        self.blocks = nn.ModuleList(EvaBlock(dim, num_heads, hidden, init_values, qk_norm, scale_attn_inner) for _ in range(depth))
        self.norm = nn.LayerNorm(dim, eps=1e-6)


class PrimusV2(nn.Module):
    """Constructor keywords of the reference wrapper (architectures.py:168-260).  Dropout / drop-path / patch-drop rates are
    accepted and must be zero (inference path)."""

    def __init__(self, input_channels, num_classes, embed_dim, patch_embed_size, eva_depth=24, eva_numheads=16, input_shape=None,
                 num_register_tokens=0, init_values=None, scale_attn_inner=False, qk_norm=False, out_norm="none", out_norm_eps=1e-5,
                 register_init_std=1e-6, in_eps=1e-5, drop_path_rate=0.0, patch_drop_rate=0.0, proj_drop_rate=0.0,
                 attn_drop_rate=0.0, mlp_ratio=4 * 2 / 3):
        super().__init__()
        if tuple(patch_embed_size) != (8, 8, 8):
            raise ValueError("PrimusV2's deeper patch embed is hardwired to an 8x stride")          # pretraining_networks.py:116-118
        if any(r != 0 for r in (drop_path_rate, patch_drop_rate, proj_drop_rate, attn_drop_rate)):
            raise NotImplementedError("PrimusV2 (anatomix_amd): dropout / drop-path / patch-drop are not implemented")
        if input_shape is None or embed_dim % eva_numheads:
            raise ValueError("input_shape is required and embed_dim must be divisible by eva_numheads")
        if (embed_dim // eva_numheads) % (2 * len(input_shape)):
            # the rotary table holds head_dim // (2 * axes) frequency bands per axis, each for one (even, odd) channel pair: a head
            # width that is not a multiple of 2 * axes leaves channels without a band (every PRIMUS_CONFIGS entry is: 66, 66, 72, 66)
            raise ValueError(f"head_dim {embed_dim // eva_numheads} must be a multiple of {2 * len(input_shape)} "
                             "(rotation pairs x spatial axes of the rotary embedding)")
        self.grid = tuple(int(s) // 8 for s in input_shape)
        self.num_register_tokens = int(num_register_tokens)
        self.down_projection = PatchEmbedDeeper(input_channels, embed_dim, 32, (1, 1, 1), in_eps)
        self.eva = Eva(embed_dim, eva_depth, eva_numheads, self.grid, int(embed_dim * mlp_ratio), init_values, qk_norm, scale_attn_inner)
        self.up_projection = PatchDecode(patch_embed_size, embed_dim, num_classes)
        self.register_tokens = None
        if self.num_register_tokens > 0:
            self.register_tokens = nn.Parameter(torch.randn(1, self.num_register_tokens, embed_dim) * register_init_std)
        self.out_norm = build_out_norm(out_norm, num_classes, out_norm_eps)
        # The vendor-library parts (linears, tokenizer / decoder convolutions) run in fp32, as the reference runs them.
        # (Measured: torch.autocast(float16) around them costs 2.6e-3 rel-L2 against the fp32 result -- beyond the 1e-3 target --
        # for 10 % at batch 2, so no such mode is offered.)
        self.register_buffer("rope_table", build_rope_table(self.grid, embed_dim // eva_numheads), persistent=False)
        self._vit_cfg = dict(input_channels=int(input_channels), num_classes=int(num_classes), embed_dim=int(embed_dim), depth=int(eva_depth),
                             heads=int(eva_numheads), num_register_tokens=self.num_register_tokens, grid_d=self.grid[0], grid_h=self.grid[1],
                             grid_w=self.grid[2], hidden=int(embed_dim * mlp_ratio), dec1=0, dec2=0, qk_norm=int(bool(qk_norm)),
                             scale_attn_inner=int(bool(scale_attn_inner)), layer_scale=int(init_values is not None), in_eps=float(in_eps),
                             out_norm=int(isinstance(self.out_norm, ChannelDemean)),
                             decoder_split=1, stem_split=1)
        dec = [m for m in self.up_projection.decode.modules() if isinstance(m, nn.ConvTranspose3d)]
        self._vit_cfg["dec1"], self._vit_cfg["dec2"] = (dec[0].out_channels, dec[1].out_channels) if len(dec) == 3 else (0, 0)
        self.use_engine = True
        self._train_attention = "torch"
        self._train_linear = "torch"
        self._train_tokenizer = "torch"
        self._train_norm = "torch"
        self._train_decoder = "torch"
        self._handle = None
        self._engine_sig = None
        self._engine_ws = None

    @property
    def train_attention(self):
        """Who runs the attention core when autograd is on and the input is on a GPU: ``"torch"`` (the default:
        F.scaled_dot_product_attention) or ``"hip"`` (the library's flash forward + backward, ``_AttentionCoreFn``).  LayerScale
        is torch autograd either way; the linears, the tokenizer, the token LayerNorms and the dense decoder have their own
        switches, ``train_linear``, ``train_tokenizer``, ``train_norm`` and ``train_decoder``."""
        return self._train_attention

    @train_attention.setter
    def train_attention(self, value):
        if value not in TRAIN_CORES:
            raise ValueError(f"train_attention must be one of {TRAIN_CORES}, got {value!r}")
        self._train_attention = value
        for blk in self.eva.blocks:
            blk.attn.train_core = value

    @property
    def train_linear(self):
        """Who runs the seven nn.Linear of every EVA block when autograd is on and the input is on a GPU: ``"torch"`` (the default:
        fp32 vendor GEMMs under torch autograd) or ``"hip"`` (``_LinearFn``: f16 operands, fp32 sums, forward and both gradients on
        the library's kernels).  CPU tensors and ``torch.no_grad()`` keep their paths either way."""
        return self._train_linear

    @train_linear.setter
    def train_linear(self, value):
        if value not in TRAIN_CORES:
            raise ValueError(f"train_linear must be one of {TRAIN_CORES}, got {value!r}")
        self._train_linear = value
        for blk in self.eva.blocks:
            blk.attn.train_linear = blk.mlp.train_linear = value

    @property
    def train_tokenizer(self):
        """Who runs the conv tokenizer (stem + three residual stages; ``proj`` stays a torch module) when autograd is on and the input
        is on a GPU: ``"torch"`` (the default: vendor convolutions under torch autograd) or ``"hip"`` (``_TokenizerFn``: the engine's
        strict forward kernels plus the library's backward).  Independent of ``train_attention`` / ``train_linear``.  Where
        ``tokenizer_unsupported_reason`` names a reason, the torch modules run whatever the switch says."""
        return self._train_tokenizer

    @train_tokenizer.setter
    def train_tokenizer(self, value):
        if value not in TRAIN_CORES:
            raise ValueError(f"train_tokenizer must be one of {TRAIN_CORES}, got {value!r}")
        self._train_tokenizer = value
        self.down_projection.train_route = value

    @property
    def train_norm(self):
        """Who runs the token LayerNorms of every EVA block (``norm1``, ``attn.norm``, ``norm2``, ``mlp.norm`` with the SwiGLU product
        ``silu(g) * x`` in front of it) and the final ``eva.norm`` when autograd is on and the input is on a GPU: ``"torch"`` (the
        default: the modules under torch autograd) or ``"hip"`` (``_LayerNormFn`` / ``_GatedLayerNormFn``, fp32).  Independent of the
        other three switches.  The per-head q / k norms belong to the attention core; LayerScale stays torch.  CPU tensors,
        ``torch.no_grad()`` and widths outside the kernels' envelope keep the modules either way."""
        return self._train_norm

    @train_norm.setter
    def train_norm(self, value):
        if value not in TRAIN_CORES:
            raise ValueError(f"train_norm must be one of {TRAIN_CORES}, got {value!r}")
        self._train_norm = value
        for blk in self.eva.blocks:
            blk.train_norm = blk.attn.train_norm = blk.mlp.train_norm = value

    @property
    def train_decoder(self):
        """Who runs the dense patch decoder and a spatial output norm in ``forward`` when autograd is on and the input is on a GPU:
        ``"torch"`` (the default: vendor transposed convolutions under torch autograd) or ``"hip"`` (``_DecoderFn``: fp32 products on
        the f32-input MFMA, forward and every gradient on the library's kernels).  none / demean / instance run inside the call; a
        per-voxel output norm (layernorm, layernorm_affine) keeps its torch module behind it.  Independent of the other four
        switches; ``forward_train_sampled`` and the no-grad engine path do not look at it.  Where ``decoder_unsupported_reason``
        names a reason, the torch modules run whatever the switch says."""
        return self._train_decoder

    @train_decoder.setter
    def train_decoder(self, value):
        if value not in TRAIN_CORES:
            raise ValueError(f"train_decoder must be one of {TRAIN_CORES}, got {value!r}")
        self._train_decoder = value

    def decoder_unsupported_reason(self, x):
        """None when ``train_decoder = "hip"`` covers this network and input, else why not: a CPU tensor, a decoder that is not the
        three-stage ``PatchDecode``, or views / widths outside the envelope of ``amx_vit_decoder_train_forward``."""
        if not x.is_cuda:
            return "the input is a CPU tensor: the decoder kernels have no host path"
        parts = _decoder_train_parts(self.up_projection, self.out_norm)
        if isinstance(parts, str):
            return parts
        w = parts[0]
        widths = (w[0].shape[0], w[0].shape[1], w[4].shape[1], w[8].shape[1])
        with torch.cuda.device(x.device):
            if _lib.load().amx_vit_decoder_train_saved_bytes(int(x.shape[0]), *self.grid, *widths) == 0:
                return (f"{x.shape[0]} views, token grid {self.grid}, decoder widths {widths} are outside the envelope (multiples of 4 up "
                        "to 1056 / 328 / 104, 1 .. 128 output channels, every tensor below 2^31 elements)")
        return None

    def tokenizer_unsupported_reason(self, x):
        """None when ``train_tokenizer = "hip"`` covers this network and input, else why not: a CPU tensor, a shape outside the
        envelope of ``amx_tokenizer_train_forward``, an input that requires a gradient, or a tokenizer other than one input channel,
        base width 32 and ``depth_per_level`` (1, 1, 1)."""
        return self.down_projection.unsupported_reason(x)

    # ------------------------------------------------------------------------------------------------------------------
    # HIP engine (one C-ABI call per forward)
    def _engine_tensors(self, lib):
        sd = dict(self.named_parameters())
        n = lib.amx_vit_num_params(self._handle)
        return [sd[lib.amx_vit_param_name(self._handle, i).decode()] for i in range(n)]

    def _engine(self, dev):
        """The loaded engine on ``dev``: creates the handle at first use, uploads the parameters when they changed, and refuses
        parameters that live elsewhere.  Returns ``(lib, stream)``; call it inside ``torch.cuda.device(dev)``.  The forward and the
        sliding-window routes (registration/sliding_window.py) both start here."""
        lib = _lib.load()
        stream = _lib.stream(dev)
        if self._handle is None:
            cfg = _lib.VitCfg(**self._vit_cfg)
            hnd = ctypes.c_void_p()
            _lib.check(lib.amx_vit_create(ctypes.byref(hnd), ctypes.byref(cfg)))
            self._handle = hnd
        tensors = self._engine_tensors(lib)
        # the engine is handed raw device pointers: a parameter still on the host (module never moved, or moved after the input)
        # would fault the GPU instead of raising torch's device-mismatch error
        stray = [tuple(t.shape) for t in list(tensors) + [self.rope_table] if t.device != dev]
        if stray:
            raise RuntimeError(f"PrimusV2.forward_hip: input on {dev} but {len(stray)} parameter / buffer tensors are elsewhere "
                               f"(first shape {stray[0]}): move the module with .to({str(dev)!r}) first")
        sig = tuple((t.data_ptr(), t._version) for t in tensors) + (str(dev),)
        if sig != self._engine_sig:
            held = [t.detach().float().contiguous() for t in tensors]
            arr = (ctypes.c_void_p * len(held))(*[t.data_ptr() for t in held])
            rope = self.rope_table.detach().float().contiguous()
            _lib.check(lib.amx_vit_load(self._handle, arr, len(held), _lib.ptr(rope), stream))
            torch.cuda.current_stream(dev).synchronize()          # the staging copies in `held` may be temporaries
            self._engine_sig = sig
        return lib, stream

    def _engine_workspace(self, need, dev):
        """The engine's one device workspace, grown to ``need`` bytes (the forward and the window routes share it: they never overlap
        on a stream)."""
        ws = self._engine_ws
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self._engine_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def forward_hip(self, x, n_blocks=-1, taps=None):
        """[N, 1, D, H, W] fp32 on the GPU -> [N, num_classes, D, H, W]: ``amx_vit_forward`` + (for output norms other than none /
        demean) the torch output norm.  Raises when the configuration is outside the engine's envelope -- there is no fallback.

        ``taps`` (test aid): names of intermediates (``amx_vit_forward_taps``, include/anatomix_amd.h lists them), or a dict
        name -> bool (False: only the route, nothing is copied).  Returns ``(y, {name: (data, route)})``: ``data`` is the flat byte
        buffer viewed as the tap's type -- one tensor, a ``(first, second)`` pair for the two-range taps (hi | lo planes, scale |
        shift), or None -- and ``route`` the instance name of the launch that produced it.  ``y`` has the bits of a plain forward."""
        dev = x.device
        if tuple(x.shape[2:]) != tuple(8 * g for g in self.grid) or x.shape[1] != self._vit_cfg["input_channels"]:
            raise ValueError(f"PrimusV2 was built for inputs of {tuple(8 * g for g in self.grid)} (got {tuple(x.shape[1:])})")
        with torch.cuda.device(dev):
            lib, stream = self._engine(dev)
            n = x.shape[0]
            need = lib.amx_vit_workspace_bytes(self._handle, n)
            ws = self._engine_workspace(need, dev)
            xin = x.detach().float().contiguous()
            y = torch.empty((n, self._vit_cfg["num_classes"]) + tuple(x.shape[2:]), dtype=torch.float32, device=dev)
            if taps is None:
                _lib.check(lib.amx_vit_forward(self._handle, _lib.ptr(xin), _lib.ptr(y), n, _lib.ptr(ws), need, int(n_blocks), stream))
            else:
                want = dict(taps) if isinstance(taps, dict) else {name: True for name in taps}
                req = (_lib.VitTap * max(1, len(want)))()
                bufs = {}
                for r, (name, copy) in zip(req, want.items()):
                    r.name = name.encode()
                    if copy:
                        nbytes = lib.amx_vit_tap_bytes(self._handle, n, r.name)
                        bufs[name] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                        r.d_dst, r.bytes = bufs[name].data_ptr(), nbytes
                _lib.check(lib.amx_vit_forward_taps(self._handle, _lib.ptr(xin), _lib.ptr(y), n, _lib.ptr(ws), need, int(n_blocks), req,
                                                    len(want), stream))
                got = {name: (self._tap_view(name, bufs.get(name)), r.route.decode()) for r, name in zip(req, want)}
        if not isinstance(self.out_norm, (ChannelDemean, nn.Identity)):
            y = self.out_norm(y)
        return y if taps is None else (y, got)

    def _tap_view(self, name, buf):
        """A tap's bytes as tensors of its type: fp32 for the raw conv outputs, (scale, shift), the token stream, the attention
        output, the demean constants and the output; f16 for the operand rows; a pair for the two-range taps."""
        if buf is None:
            return None
        leaf = name.split(".")[-1]
        if leaf in ("ss1", "ss2", "sss"):
            return tuple(buf.view(torch.float32).chunk(2))
        if leaf in ("raw1", "raw2", "raws", "tokens", "attn", "tok1", "tok2", "raw", "mean", "y"):
            return buf.view(torch.float32)
        split = self._vit_cfg["stem_split"] if name == "h0" else (self._vit_cfg["decoder_split"] if name[0] == "d" else 1)
        if leaf in ("h0", "p0", "a1", "h", "p", "in") or name == "d.ln":
            return tuple(buf.view(torch.float16).chunk(2)) if split else (buf.view(torch.float16), None)
        return buf.view(torch.float16)

    def train(self, mode=True):
        """A switch of mode marks the engine's packed parameters stale: optimizers that update the parameters through raw device
        pointers (``FusedAdamW``) do not move the tensors' version counters, which is all ``_engine`` compares (``Unet.train`` does the
        same for its handle)."""
        self._engine_sig = None
        return super().train(mode)

    def _drop_engine(self):
        """The engine's packed parameters live on the device it was created on: a move / copy / replica starts over."""
        hnd, self._handle = self.__dict__.get("_handle"), None
        self._engine_sig = None
        self._engine_ws = None
        if hnd is not None:
            try:
                _lib.load().amx_vit_destroy(hnd)
            except Exception:
                pass

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._drop_engine()
        return out

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = None if k in ("_handle", "_engine_sig", "_engine_ws") else copy.deepcopy(v, memo)
        return new

    def __getstate__(self):
        state = dict(self.__dict__)
        for k in ("_handle", "_engine_sig", "_engine_ws"):
            state[k] = None
        return state

    def __copy__(self):
        new = self.__class__.__new__(self.__class__)
        new.__dict__.update(self.__getstate__())
        return new

    def _replicate_for_data_parallel(self):
        replica = super()._replicate_for_data_parallel()
        for k in ("_handle", "_engine_sig", "_engine_ws"):
            replica.__dict__[k] = None
        return replica

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                _lib.load().amx_vit_destroy(self._handle)
        except Exception:
            pass

    def _tokens(self, x):
        """[N, T, E]: the tokens after the final norm, register tokens dropped."""
        feat = self.down_projection(x)
        B, E = feat.shape[:2]
        if tuple(feat.shape[2:]) != self.grid:
            raise ValueError(f"PrimusV2 was built for inputs of {tuple(8 * g for g in self.grid)} (got {tuple(x.shape[2:])})")
        tok = feat.flatten(2).transpose(1, 2) + self.eva.pos_embed
        nreg = self.num_register_tokens
        if nreg:
            tok = torch.cat((self.register_tokens.expand(B, -1, -1), tok), 1)
        for blk in self.eva.blocks:
            tok = blk(tok, self.rope_table, nreg)
        return _layer_norm(self.eva.norm, tok, self._train_norm)[:, nreg:]

    def _body(self, x):
        tok = self._tokens(x)
        return self.up_projection(tok.transpose(1, 2).reshape(tok.shape[0], tok.shape[2], *self.grid))

    def sampled_unsupported_reason(self, x, rows=None):
        """None when ``forward_train_sampled`` covers this network and input, else why not: an output norm with spatial statistics
        (instance, demean), a CPU tensor, a decoder or widths outside the envelope of ``amx_vit_decode_rows_*`` -- or, when the caller
        says how many ``rows`` per view it will sample, more views x rows than the kernels take."""
        if not x.is_cuda:
            return "the input is a CPU tensor: the rows kernels have no host path"
        if x.dim() != 5 or tuple(x.shape[2:]) != tuple(8 * g for g in self.grid):
            return f"the input {tuple(x.shape)} is not [N, C, {', '.join(str(8 * g) for g in self.grid)}]"
        parts = _decode_rows_parts(self.up_projection, self.out_norm)
        if isinstance(parts, str):
            return parts
        if x.shape[0] < 1 or x.shape[0] > 65535:
            return f"{x.shape[0]} views are outside the envelope"
        if rows is not None and (rows < 1 or x.shape[0] * int(rows) > _DECODE_ROWS_MAX_ROWS):
            return f"{x.shape[0]} views x {rows} rows are outside the envelope (1 .. 2^20)"
        return None

    def forward_train_sampled(self, x, layers, sampler, on_start=None):
        """The differentiable forward with the final volume SAMPLED, the contract of ``model.train.forward_train_sampled``: returns
        ``(None, [rows], [coords], [(D, H, W)])`` -- the fp32 rows [N, P, C] of ``out_norm(decoder(tokens))`` at the coordinates
        ``sampler(layer id, (D, H, W))`` drew when the forward reached the decoder (called exactly once; ``on_start()`` runs right before
        it).  The dense volume is never formed: the first result is None.  The body up to the final norm is ``forward``'s, with
        ``train_attention`` / ``train_linear`` honoured; the decoder and a per-voxel output norm run on ``amx_vit_decode_rows_*``."""
        layers = [int(l) for l in layers]
        if len(layers) != 1:
            raise ValueError(f"PrimusV2.forward_train_sampled: the ViT has one tap, the final volume (got layers {layers})")
        reason = self.sampled_unsupported_reason(x)
        if reason is not None:
            raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"PrimusV2.forward_train_sampled: {reason}")
        tok = self._tokens(x)
        dims = tuple(8 * g for g in self.grid)
        if on_start is not None:
            on_start()
        coords = sampler(layers[0], dims)
        rows = decode_rows(tok, coords, self.up_projection, self.out_norm, self.grid, check_coords=False)
        return None, [rows], [coords], [dims]

    def forward(self, x, layers=None, encode_only=False, verbose=False, ret_mask=False):
        """architectures.py:122-165: a nonempty ``layers`` asks for the final volume as the sole feature; a boolean ``layers`` is
        the upstream positional ``ret_mask`` (no patch dropout here: the mask is all ones)."""
        if isinstance(layers, bool):
            ret_mask, layers = layers, None
        if x.is_cuda and not torch.is_grad_enabled() and self.use_engine:
            try:
                output = self.forward_hip(x)
            except _lib.AmxError as e:
                # configurations outside the engine's envelope (amx_vit_create refuses them with AMX_ERR_INVALID / AMX_ERR_SHAPE:
                # input_channels != 1, token grids that are not multiples of 64 or have an odd width, widths beyond its tiles, other
                # decoders) ran on the torch modules before the engine existed: name the switch.  Every other failure (HIP runtime
                # errors, out of memory, the overflow guard) keeps its own type and message.
                if getattr(e, "code", None) not in (_lib.AMX_ERR_INVALID, _lib.AMX_ERR_SHAPE):
                    raise
                raise _lib.AmxEnvelopeError(e.code, f"PrimusV2: the HIP engine does not cover this configuration ({e}); set "
                                            "`model.use_engine = False` to run the stock torch composition of the same modules") from e
        elif self._train_decoder == "hip" and torch.is_grad_enabled() and self.decoder_unsupported_reason(x) is None:
            output = decode_dense(self._tokens(x), self.up_projection, self.out_norm, self.grid)
        else:
            output = self.out_norm(self._body(x))
        if ret_mask:
            return output, torch.ones((x.shape[0], 1) + self.grid, dtype=torch.bool, device=x.device)
        if layers:
            return [output] if encode_only else (output, [output])
        return output
