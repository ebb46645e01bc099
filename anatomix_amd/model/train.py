"""Differentiable train-mode forward of ``Unet`` on the HIP kernels (the UNet inside the reference's contrastive
step, pretraining/models/supcl_model.py:603-661, 735-742: ``netG(reals, nce_layers, False)`` with BatchNorm in train
mode, then ``loss.backward()``).

One ``torch.autograd.Function`` covers the whole network: the forward runs conv -> train-mode BatchNorm -> activation
blocks, max-pools and the upsample + concat convs through the library's single-operator entry points
(``anatomix_amd.model.train_ops``), keeps what the adjoint needs (raw conv outputs, activations, batch statistics) in
16-bit channels-last tensors, and the backward walks the blocks in reverse: activation/BatchNorm adjoint -> weight
gradient (MFMA kernel) -> data gradient (forward kernel on the zero-framed gradient with flipped weights + reflect fold)
-> max-pool / upsample / concat adjoints.  Storage precision is ``model.train_precision`` (``model.precision`` when set explicitly, else "bf16": "bf16" mirrors the reference's
bf16 autocast); parameter gradients and BatchNorm statistics are fp32.

Supported configuration: norm 'batch' (batch statistics + running-stat update; layers in eval mode use their frozen
running statistics, folded into the conv), 'instance' / 'instance_affine' (the same kernels, one sample at a time), conv bias, activation relu/lrelu, pooling 'Max' / 'Avg', interp 'nearest' (fused
into the concat convs) / 'trilinear' (materialised + its adjoint kernel), doubleconv either; feature taps at conv /
norm / activation / pool / upsample ids and at the output conv.  Everything else raises (the caller can still opt into the stock-module
path).

Layout: ``plan_network`` turns ``model.model`` into typed steps on the host and raises everything that is not covered BEFORE the first
launch; ``_UnetTrainFn.forward`` / ``.backward`` are drivers over those steps, one function per step.
"""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import train_ops as T

_DT = {"f16": torch.float16, "fp16": torch.float16, "float16": torch.float16, "bf16": torch.bfloat16, "bfloat16": torch.bfloat16}


# weight gradients go to a side stream, beside the data gradient of the same block, for blocks at least this wide (narrower: the two
# joins cost what the overlap returns; 6.41 -> 6.37 ms per step)
OVERLAP_WGRAD_MIN_W = 32
_SIDE = {}


def _side_stream(device):
    key = (device.type, device.index)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device)
    return _SIDE[key]


# ---- the plan: model.model as typed steps, host only -------------------------------------------------------------------------

class TapNotImplemented(NotImplementedError):
    """A feature tap the HIP training path does not serve (``unsupported_reason`` returns these messages)."""


_TAPS_AT = "feature taps are implemented at conv / norm / activation / pool / upsample ids"
_UP_TAP_NO_SKIP = "a tap at an upsample id without skip connections is not implemented in the HIP training path"
_SAMPLED_AT = "sampled taps are implemented at conv ids (pre-norm outputs) and the output conv"
_SAMPLED_FROZEN = "sampled taps at a frozen-statistics block"


class ConvBlock(NamedTuple):
    """conv [-> norm [-> activation]] at module ids ``idx`` / ``alias_ids``; its output tensor is ``name``."""
    idx: int
    conv: nn.Module
    norm: Optional[nn.Module]
    act: str                    # 'relu' / 'lrelu' / 'none'
    alias_ids: tuple            # norm and activation ids: taps there read the activated output (the activation is in place)
    kind: str                   # 'frozen' (eval-mode BatchNorm folded into the conv) / 'norm' / 'output' (the bare last conv)
    src: str                    # the input tensor; behind an upsample: the skip
    low: Optional[str]          # behind an upsample: the low-resolution tensor
    cat: Optional[str]          # behind an upsample: 'fused' (nearest, inside the conv) / 'materialised' (trilinear: tensor cat<idx>)
    push_skip: bool             # the output is kept for a decoder concat
    taps: tuple                 # (tap id, 'pre' | 'act' | 'sampled' | 'output'): pre-norm export, activated alias, sampled rows, the network output

    @property
    def name(self):
        return f"y{self.idx}"

    @property
    def last_id(self):
        return self.alias_ids[-1] if self.alias_ids else self.idx

    @property
    def inputs(self):
        """The tensor names the convolution reads: (x0, nearest-upsampled x1 or None)."""
        return (f"cat{self.idx}", None) if self.cat == "materialised" else (self.src, self.low)

    @property
    def tap_ids(self):
        return tuple(t for t, _ in self.taps)


class Pool(NamedTuple):
    idx: int
    src: str
    dst: str
    avg: bool
    tap: bool

    @property
    def tap_ids(self):
        return (self.idx,) if self.tap else ()


class Up(NamedTuple):
    """An upsample id: the next ConvBlock reads ``skip`` and ``low``; a tap here is the concat of the two (network.py:500-502)."""
    idx: int
    skip: Optional[str]
    low: str
    tap: bool

    @property
    def tap_ids(self):
        return (self.idx,) if self.tap else ()


def _module_kinds(model):
    kinds = []
    for mod in model.model:
        if isinstance(mod, nn.Conv3d):
            kinds.append("conv")
        elif isinstance(mod, (nn.BatchNorm3d, nn.InstanceNorm3d)):
            kinds.append("norm")
        elif isinstance(mod, (nn.ReLU, nn.LeakyReLU)):
            kinds.append("act")
        elif isinstance(mod, (nn.MaxPool3d, nn.AvgPool3d)):
            kinds.append("pool")
        elif isinstance(mod, nn.Upsample):
            kinds.append("up")
        else:
            kinds.append("other")
    return kinds


def plan_network(model, layers=(), sampled=False):
    """``model.model`` as a list of ConvBlock / Pool / Up steps with the taps ``layers`` assigned to them (``sampled``: as gathered rows).
    Host only: no tensors, no launches.  What the path does not cover raises here -- taps as TapNotImplemented, structure as
    NotImplementedError.  Built per call: whether a block is frozen follows ``norm.training``."""
    mods, kinds = list(model.model), _module_kinds(model)
    skip_ok, trilinear, act = model.use_skip_connection, model._cfg["interp"] == "trilinear", model._cfg["activation"]
    for l in layers:
        if not (0 <= l < len(kinds)) or kinds[l] not in ("conv", "norm", "act", "pool", "up"):
            raise TapNotImplemented(_TAPS_AT)
        if kinds[l] == "up" and not skip_ok:
            raise TapNotImplemented(_UP_TAP_NO_SKIP)
    layers = set(layers)
    steps, skips, cur, pending_low = [], [], "x", None
    i = 0
    while i < len(mods):
        k = kinds[i]
        if sampled and i in layers and k in ("pool", "up"):
            raise TapNotImplemented(_SAMPLED_AT)
        if k == "conv":
            has_bn = i + 1 < len(mods) and kinds[i + 1] == "norm"
            has_act = i + 1 + int(has_bn) < len(mods) and kinds[i + 1 + int(has_bn)] == "act"
            if pending_low is not None and not skip_ok:
                raise NotImplementedError("upsample without skip connection in the HIP training path")
            src, low = (skips.pop(), pending_low) if pending_low is not None else (cur, None)
            pending_low = None
            norm = mods[i + 1] if has_bn else None
            # BatchNorm with frozen statistics: the reference freezes single layers (pretraining/models/base_model.py:175-184); also a
            # whole network in eval mode under autograd
            kind = "output" if not has_bn else "frozen" if isinstance(norm, nn.BatchNorm3d) and not norm.training else "norm"
            alias = tuple(i + 1 + a for a in range(int(has_bn) + int(has_act))) if has_bn else ()
            tapped = [t for t in (i,) + alias if t in layers] if layers else ()
            if sampled and tapped:
                if kind == "frozen":
                    raise TapNotImplemented(_SAMPLED_FROZEN)
                if tapped != [i]:
                    raise TapNotImplemented(_SAMPLED_AT)
            taps = tuple((t, "sampled" if sampled else "output" if kind == "output" else "pre" if t == i else "act") for t in tapped)
            blk = ConvBlock(i, mods[i], norm, act if (has_bn and has_act) else "none", alias, kind, src, low,
                            None if low is None else "materialised" if trilinear else "fused",
                            skip_ok and (alias[-1] if alias else i) in model.encoder_idx, taps)
            steps.append(blk)
            cur, i = blk.name, blk.last_id
            if blk.push_skip:
                skips.append(cur)
        elif k == "pool":
            steps.append(Pool(i, cur, f"p{i}", isinstance(mods[i], nn.AvgPool3d), i in layers))
            cur = f"p{i}"
        elif k == "up":
            pending_low = cur
            steps.append(Up(i, skips[-1] if skips else None, cur, i in layers))
        else:
            raise NotImplementedError(f"module {i} ({type(mods[i]).__name__}) in the HIP training path")
        i += 1
    return steps


def _tap_reason(model, layers, sampled):
    """The plan's refusal of these taps, or None.  (Structure the plan refuses is raised by the forward itself.)"""
    try:
        plan_network(model, layers, sampled)
    except TapNotImplemented as e:
        return str(e)
    except NotImplementedError:
        pass
    return None


def unsupported_reason(model, x, layers):
    r = _config_reason(model, x)
    return r if r is not None else _tap_reason(model, layers, False)


def _config_reason(model, x):
    c = model._cfg
    if model.train_precision not in _DT:
        return (f"the HIP training path stores activations in f16 / bf16 (the reference trains under bf16 autocast); "
                f"precision '{model.train_precision}' is an inference mode")
    if c["dimension"] != 3 or c["pad_type"] != "reflect" or c["residual_connection"]:
        return "only dimension=3, pad_type='reflect', residual_connection=False are implemented"
    if c["norm"] not in ("batch", "instance", "instance_affine") or c["activation"] not in ("relu", "lrelu") or c["final_act"] != "none":
        return "the HIP training path covers norm batch / instance / instance_affine, activation relu/lrelu, final_act='none'"
    if c["pooling"] not in ("Max", "Avg") or c["interp"] not in ("nearest", "trilinear"):
        return "the HIP training path covers pooling Max / Avg, interp nearest / trilinear"
    if c["input_nc"] != 1 or c["ngf"] % 16 or c["output_nc"] % 16 or c["output_nc"] > 32:
        return "the HIP training path needs input_nc == 1, ngf a multiple of 16, output_nc in {16, 32}"
    if x.dim() != 5 or x.shape[1] != 1 or not x.is_cuda:
        return "expected a CUDA input of shape [N, 1, D, H, W]"
    m = 1 << c["num_downs"]
    if any(s % m or (s >> c["num_downs"]) < 2 for s in x.shape[2:]) or x.shape[4] < 32 or x.shape[4] > 128:
        return "spatial dims must be divisible by 2^num_downs, >= 2 at the bottleneck, 32 <= W <= 128"
    return None


def sampled_unsupported_reason(model, x, layers):
    """None when ``forward_train_sampled`` covers the request: the HIP training path itself, and every tap at a convolution that is
    followed by a norm in train mode (the pre-norm output) or at the output conv -- the ids the reference's launcher uses
    (pretraining/scripts/pretrain_anatomix.py:385: 27, 31, 38, 45, 52, 65)."""
    r = _config_reason(model, x)       # (the plan for sampled taps refuses everything the plan for dense taps does: one plan)
    return r if r is not None else _tap_reason(model, list(layers), True)


# ---- packed weights: record once per input shape, replay in one launch ---------------------------------------------------------

class PackPlan:
    """Packed weights of every plain conv in ONE launch per pass (T.pack_batch) instead of one small launch inside each conv call.
    Which convs, with how many stored input channels and at which width, is recorded by the first forward (mode 0) / backward (mode 1) of
    a given (input shape, dtype) -- which pack per call -- stored on the module and replayed afterwards; a conv whose recorded shape does
    not match packs itself as before."""
    _ATTR = ("_pack_plan", "_pack_plan_bwd")

    def __init__(self, model, key, mode):
        self.model, self.key, self.mode = model, key, mode
        self.plan = getattr(model, self._ATTR[mode], {}).get(key)
        self.rec, self.packs = {}, {}

    def views(self, dt, dev, record_to=None):
        """The batched launch of the recorded plan on the current stream (``record_to``: the stream that will read the views)."""
        ids = sorted(self.plan)
        views = T.pack_batch([(T._as_weight(self.model.model[j].weight), self.mode, self.plan[j][0], self.plan[j][1]) for j in ids], dt, dev)
        if record_to is not None:
            for v in views:
                v.record_stream(record_to)
        self.packs = dict(zip(ids, views))

    def take(self, j, cin_pad, width):
        """The packed weights of conv ``j`` for this call, or None (the conv then packs itself); records the request."""
        self.rec[j] = (cin_pad, width)
        return self.packs.get(j) if self.plan and self.plan.get(j) == (cin_pad, width) else None

    def save(self):
        if not self.plan:
            self.model.__dict__.setdefault(self._ATTR[self.mode], {})[self.key] = self.rec


def _import_and_pack(model, x, dt):
    """The 16-bit input and the pack plans of both passes.  While a HIP graph is being captured both pack launches go to a side stream,
    beside the input import -- the backward's packing (the weights do not change in between) is then off the main stream altogether."""
    dev = x.device
    key = (tuple(x.shape), dt)
    fwd, bwd = PackPlan(model, key, 0), PackPlan(model, key, 1)
    side = None
    if fwd.plan and x.is_cuda and torch.cuda.is_current_stream_capturing():
        side, main = _side_stream(dev), torch.cuda.current_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            # (the requests are formed ON the side stream: a parameter that is not fp32-contiguous gets a temporary copy there,
            #  which the allocator then only recycles behind the side stream's pack kernel)
            fwd.views(dt, dev, main)
            if bwd.plan:
                bwd.views(dt, dev, main)
    elif fwd.plan:
        fwd.views(dt, dev)
    # the single input channel, padded to one MFMA chunk: one pass (zero fill + cast + strided copy were three, 56 us at 128^3 x 2)
    xin = T.import_input(x[:, :1], dt) if x.is_cuda else None
    if side is not None:
        torch.cuda.current_stream(dev).wait_stream(side)
    if xin is None:
        xin = torch.zeros((x.shape[0],) + tuple(x.shape[2:]) + (16,), dtype=dt, device=dev)
        xin[..., 0] = x.detach()[:, 0].to(dt)
    return xin, fwd, bwd


# ---- forward steps ---------------------------------------------------------------------------------------------------------

def _bn_momentum(bn):
    """torch: momentum=None means a cumulative moving average, factor 1 / num_batches_tracked (counted including this batch)."""
    if bn.momentum is not None:
        return bn.momentum
    if torch.cuda.is_current_stream_capturing():
        # the factor 1 / (n + 1) is read back from the device (a host synchronisation, illegal during capture) and would be frozen
        # into the graph for every replay; the reference never builds its norms this way (network.py:148-152: default momentum)
        raise NotImplementedError("BatchNorm3d(momentum=None) (cumulative moving average) cannot be captured in a HIP graph: "
                                  "run the step eagerly or give the layer a momentum")
    if bn.num_batches_tracked is None:
        raise NotImplementedError("BatchNorm3d(momentum=None) without num_batches_tracked in the HIP training path")
    return 1.0 / (int(bn.num_batches_tracked.item()) + 1)


def _to_cl(t, dt):            # fp32 NCDHW -> 16-bit NDHWC
    return t.permute(0, 2, 3, 4, 1).to(dt).contiguous()


def _to_ncdhw(t):             # 16-bit NDHWC -> fp32 NCDHW
    return T.export_ncdhw(t) if t.shape[-1] % 8 == 0 else t.permute(0, 4, 1, 2, 3).float().contiguous()


def _nearest_up2(t):
    """Nearest x2 upsample of a channels-last tensor: every voxel to its 8 children."""
    n, d, h, w, c = t.shape
    return t[:, :, None, :, None, :, None, :].expand(n, d, 2, h, 2, w, 2, c).reshape(n, 2 * d, 2 * h, 2 * w, c)


def _sum_children(t, dt):
    """Adjoint of ``_nearest_up2``: the fp32 sum over the 8 children of every low-resolution voxel, stored as ``dt``."""
    n, d, h, w, c = t.shape
    return t.reshape(n, d // 2, 2, h // 2, 2, w // 2, 2, c).float().sum((2, 4, 6)).to(dt)


class _Saved(NamedTuple):
    """What a block's adjoint reads: raw conv output, activated output, statistics (norm blocks); folded scale (frozen blocks)."""
    Y: torch.Tensor
    X: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None
    rstd: Optional[torch.Tensor] = None
    a: Optional[torch.Tensor] = None


def _inputs(tensors, blk):
    in0, in1 = blk.inputs
    return tensors[in0], None if in1 is None else tensors[in1]


class _Run:
    """State of one forward: tensors by name, taps by id, what the backward keeps."""

    def __init__(self, xin, packs, sampler, on_start):
        self.tensors, self.taps, self.coords_of, self.saved = {"x": xin}, {}, {}, {}
        self.tracked = []                                                # num_batches_tracked of every BatchNorm: one foreach add
        self.packs, self.sampler, self.on_start = packs, sampler, on_start

    def start(self):
        """on_start(), once: after the first block's kernels are enqueued or right before the first draw, whichever comes first --
        work that does not depend on the forward (the coordinate draws) is enqueued behind them instead of in front of the whole forward."""
        hook, self.on_start = self.on_start, None
        if hook is not None:
            hook()

    def packed(self, blk, x0, x1):
        cin_pad, cout = x0.shape[-1] + (0 if x1 is None else x1.shape[-1]), (blk.conv.out_channels + 15) // 16 * 16
        if (cin_pad, cout) == (48, 16):                                  # the 16 + up32 -> 16 merged-tap layer packs its own format
            return None
        return self.packs.take(blk.idx, cin_pad, x0.shape[3])

    def tap(self, tid, t, how, cout=None):
        """The one way a tap leaves: a dense fp32 NCDHW export, or (``how == 'sampled'``) the P rows [N, P, C] fp32 at the coordinates
        the sampler draws now, gathered in place from channels-last 16-bit storage or from the fp32 NCDHW output of the output conv."""
        if how != "sampled":
            self.taps[tid] = _to_ncdhw(t)
            return
        cl = cout is not None
        self.start()
        c = self.coords_of[tid] = self.sampler(tid, tuple(t.shape[1:4] if cl else t.shape[2:]))
        self.taps[tid] = T.gather_rows(t, c)[..., :cout] if cl else T.gather_rows(t, c, channels_last=False)


def _bias(conv):
    return None if conv.bias is None else conv.bias.detach().float().contiguous()


def _run_frozen_block(run, blk):
    # y = act(a * conv(x) + b) with a, b from the running statistics -- folded into the conv's weights and shift, no norm kernels at all
    conv, bn, (x0, x1), bias = blk.conv, blk.norm, _inputs(run.tensors, blk), _bias(blk.conv)
    gam = None if bn.weight is None else bn.weight.detach().float()
    bet = None if bn.bias is None else bn.bias.detach().float()
    a = (bn.running_var.float() + bn.eps).rsqrt()
    if gam is not None:
        a = a * gam
    b = -bn.running_mean.float() * a
    if bet is not None:
        b = b + bet
    if bias is not None:
        b = b + bias * a
    Y = T.conv_forward(x0, x1, conv.weight.detach().float() * a.view(-1, 1, 1, 1, 1), blk.act, 0.3, shift=b.contiguous())
    run.saved[blk.idx] = _Saved(Y=Y, a=a)
    run.tensors[blk.name] = Y
    for tid, how in blk.taps:
        # pre-norm tap: the raw convolution, computed only when asked for
        run.tap(tid, T.conv_forward(x0, x1, conv.weight, shift=bias) if how == "pre" else Y, how)


def _run_norm_block(run, blk):
    conv, bn, (x0, x1) = blk.conv, blk.norm, _inputs(run.tensors, blk)
    X = T.conv_forward(x0, x1, conv.weight, shift=_bias(conv), wpk=run.packed(blk, x0, x1))
    gam = None if bn.weight is None else bn.weight.detach()
    bet = None if bn.bias is None else bn.bias.detach()
    if isinstance(bn, nn.BatchNorm3d):
        Y, mean, rstd = T.bn_train_forward(X, gam, bet, bn.eps, blk.act, 0.3, bn.running_mean, bn.running_var, _bn_momentum(bn))
        if bn.num_batches_tracked is not None:
            run.tracked.append(bn.num_batches_tracked)
    else:
        # InstanceNorm3d: the same statistics kernels over one sample at a time, no running statistics
        Y = torch.empty_like(X)
        stats = [T.bn_train_forward(X[s:s + 1], gam, bet, bn.eps, blk.act, 0.3, out=Y[s:s + 1])[1:] for s in range(X.shape[0])]
        mean = torch.stack([m for m, _ in stats])
        rstd = torch.stack([r for _, r in stats])
    run.saved[blk.idx] = _Saved(Y=Y, X=X, mean=mean, rstd=rstd)
    run.tensors[blk.name] = Y
    for tid, how in blk.taps:                                            # conv id: the pre-norm output; the in-place activation aliases the norm output
        run.tap(tid, Y if how == "act" else X, how, conv.out_channels)


def _run_output_conv(run, blk):
    x0, _ = _inputs(run.tensors, blk)
    out = T.conv_forward(x0, None, blk.conv.weight, out32=True, shift=_bias(blk.conv), wpk=run.packed(blk, x0, None))
    run.tensors[blk.name] = out
    for tid, how in blk.taps:
        if how == "sampled":                                             # (a dense tap here is the network output itself)
            run.tap(tid, out, how)


def _run_pool(run, st):
    run.tensors[st.dst] = T.pool2(run.tensors[st.src], 1 if st.avg else 0)
    if st.tap:
        run.tap(st.idx, run.tensors[st.dst], "act")


def _run_up_tap(run, st, trilinear):
    # the reference takes this tap AFTER torch.cat((skip, upsampled), 1) (network.py:500-502): materialised
    # only when asked for -- the convolution that follows still reads skip and low-resolution tensor directly
    low = run.tensors[st.low]
    up = T.upsample2_trilinear(low) if trilinear else _nearest_up2(low)
    run.tap(st.idx, torch.cat([run.tensors[st.skip], up], dim=-1), "act")


_RUN_BLOCK = {"frozen": _run_frozen_block, "norm": _run_norm_block, "output": _run_output_conv}


# ---- backward steps --------------------------------------------------------------------------------------------------------

class _Adjoint:
    """State of one backward: gradients by tensor name, parameter gradients by id, tap cotangents by id."""

    def __init__(self, ctx, dtaps):
        self.ctx, self.tensors, self.saved, self.dt = ctx, ctx.tensors, ctx.saved, ctx.dt
        self.dev = ctx.tensors["x"].device
        self.dtap = {l: g for l, g in zip(ctx.layers, dtaps) if g is not None}
        self.grads, self.pgrads, self.frames = {}, {}, {}
        self.dx_in, self.wgrad_pending, self.packs = None, None, None

    def add_grad(self, name, g):
        self.grads[name] = g if name not in self.grads else self.grads[name] + g

    def frame(self, shape, c):
        key = (tuple(shape), c)
        if key not in self.frames:
            self.frames[key] = T.shared_framed(shape[0], shape[1], shape[2], shape[3], c, self.dt, self.dev)
        return self.frames[key]

    def join(self):
        if self.wgrad_pending is not None:                               # the frames and the scratch are shared: one in flight
            torch.cuda.current_stream(self.dev).wait_stream(self.wgrad_pending)
            self.wgrad_pending = None

def _up_tap_grads(bw, steps, trilinear):
    """Gradients of taps taken at upsample ids: split the concatenated gradient, skip part as is, upsampled part through the
    adjoint of the interpolation."""
    for st in steps:
        if not (isinstance(st, Up) and st.tap and st.idx in bw.dtap):
            continue
        g = bw.dtap.pop(st.idx)
        skip, low = bw.tensors[st.skip], bw.tensors[st.low]
        cs = skip.shape[-1]
        bw.add_grad(st.skip, T.import_ncdhw(g[:, :cs], torch.empty_like(skip)))
        gu = torch.empty((low.shape[0], 2 * low.shape[1], 2 * low.shape[2], 2 * low.shape[3], low.shape[4]), dtype=bw.dt, device=low.device)
        T.import_ncdhw(g[:, cs:], gu)
        bw.add_grad(st.low, T.upsample2_trilinear_backward(gu) if trilinear else _sum_children(gu, bw.dt))


def _backward_packs(bw, pre):
    """Data-gradient packings of the plain blocks in one launch (same record-and-replay as the forward)."""
    packs = PackPlan(bw.ctx.model, bw.ctx.pkey, 1)
    if packs.plan and pre is not None and pre.plan == packs.plan:        # packed beside the forward's input import (same weights)
        packs.packs = pre.packs
    elif packs.plan:
        packs.views(bw.dt, bw.dev)
    return packs


def _pool_adjoint(bw, st):
    grads, dtap = bw.grads, bw.dtap
    if st.idx in dtap:                                                   # tap at the pool id: gradient of the pooled tensor
        if st.dst in grads:
            T.import_ncdhw(dtap.pop(st.idx), grads[st.dst], accumulate=True)
        else:
            grads[st.dst] = T.import_ncdhw(dtap.pop(st.idx), torch.empty_like(bw.tensors[st.dst]))
    if st.dst not in grads:
        return
    dp = grads.pop(st.dst)
    if st.avg:                                                           # adjoint of AvgPool3d(2): every child gets dp / 8
        bw.add_grad(st.src, _nearest_up2(dp * 0.125))
    elif st.src in grads:
        T.pool2_max_backward(dp, bw.tensors[st.src], accumulate_into=grads[st.src])
    else:
        grads[st.src] = T.pool2_max_backward(dp, bw.tensors[st.src])


def _output_adjoint(bw, blk, dout):
    """The framed gradient of the output conv's result (None: nothing to do, or everything done from the sampled rows)."""
    conv, idx, (x0, x1) = blk.conv, blk.idx, _inputs(bw.tensors, blk)
    coords = bw.ctx.coords_of.get(idx)
    rows = bw.dtap.pop(idx, None) if coords is not None else None
    if dout is None and rows is None:
        return None
    if (dout is None and x1 is None and x0.is_cuda and conv.out_channels <= 16 and conv.in_channels <= 16 and rows.shape[1] <= 1024):
        # the only cotangent of the output conv is 2 x 512 sampled rows: its weight and data gradient from those rows
        # directly (amx_conv3d_backward_sampled) instead of a dense pass over a gradient volume of zeros
        need_din = blk.inputs[0] != "x"
        dw, din = T.conv_backward_sampled(rows, coords, x0, conv.weight, conv.in_channels, need_din)
        bw.pgrads[id(conv.weight)] = dw
        if conv.bias is not None:
            bw.pgrads[id(conv.bias)] = rows.to(bw.dt).float().sum((0, 1))
        if need_din:
            bw.add_grad(blk.inputs[0], din)
        elif bw.ctx.needs_input_grad[1]:
            raise NotImplementedError("input gradient through a sampled tap at a one-conv network")
        return None
    fr = bw.frame(x0.shape[:4], conv.out_channels)
    if dout is not None:
        T.import_ncdhw(dout, T.interior(fr))
    else:
        fr.zero_()                                                       # (the whole buffer: a contiguous fill is 3x faster than the strided interior)
    if rows is not None:                                                 # sampled tap at the output conv: 2 x 512 rows of gradient
        T.scatter_rows(rows, coords, T.interior(fr), accumulate=True)
    return fr


def _norm_adjoint(bw, blk):
    """Activation + norm adjoint of a frozen / BatchNorm / InstanceNorm block into the framed gradient of its raw conv output, norm
    parameter gradients included; no gradient of the activated output: the zeroed frame.  None: nothing downstream was used."""
    idx, bn, cout, sv, dtap, pgrads = blk.idx, blk.norm, blk.conv.out_channels, bw.saved[blk.idx], bw.dtap, bw.pgrads
    dy = bw.grads.pop(blk.name, None)
    for j in blk.alias_ids:                                              # taps that alias the activated output
        if j in dtap:
            if dy is None:
                dy = torch.empty_like(sv.Y)
                T.import_ncdhw(dtap.pop(j), dy)
            else:
                dy = T.import_ncdhw(dtap.pop(j), dy, accumulate=True)    # dy is owned by this backward: in place
    if dy is None and idx not in dtap:
        return None
    n = sv.Y.shape[0]
    fr = bw.frame(sv.Y.shape[:4], cout)
    gam = None if bn.weight is None else bn.weight.detach()
    bet = None if bn.bias is None else bn.bias.detach()
    if dy is not None and blk.kind == "frozen":
        # du = dy * act'(y) (bare activation adjoint); d gamma / d beta from the recovered pre-activation u; then the
        # gradient of the raw convolution output is a * du and everything downstream is the ordinary conv adjoint
        T.bn_act_backward(dy, sv.Y, None, None, None, None, blk.act, 0.3, framed=fr)
        du = T.interior(fr)[..., :cout]
        if bn.weight is not None:
            duf, yf = du.float(), sv.Y[..., :cout].float()
            u = yf if blk.act != "lrelu" else torch.where(yf > 0, yf, yf / 0.3)
            s1 = duf.sum((0, 1, 2, 3))
            pgrads[id(bn.bias)] = s1
            pgrads[id(bn.weight)] = ((duf * u).sum((0, 1, 2, 3)) - bn.bias.detach().float() * s1) / bn.weight.detach().float()
        du.mul_(sv.a.to(bw.dt))
    elif dy is not None and isinstance(bn, nn.BatchNorm3d):
        _, dgamma, dbeta = T.bn_act_backward(dy, sv.Y, sv.X, sv.mean, sv.rstd, gam, blk.act, 0.3, framed=fr, beta=bet, recompute=True)
        pgrads[id(bn.weight)], pgrads[id(bn.bias)] = dgamma, dbeta
    elif dy is not None:                                                 # InstanceNorm3d: per sample
        dgs, dbs = [], []
        for s_ in range(n):
            _, dg_, db_ = T.bn_act_backward(dy[s_:s_ + 1], sv.Y[s_:s_ + 1], sv.X[s_:s_ + 1], sv.mean[s_], sv.rstd[s_], gam, blk.act, 0.3,
                                            framed=fr[s_:s_ + 1], beta=bet, recompute=True)
            dgs.append(dg_)
            dbs.append(db_)
        if bn.weight is not None:
            pgrads[id(bn.weight)], pgrads[id(bn.bias)] = torch.stack(dgs).sum(0), torch.stack(dbs).sum(0)
    else:
        fr.zero_()                                                       # (the whole buffer: a contiguous fill is 3x faster than the strided interior)
    if idx in dtap:                                                      # tap at the conv id: gradient of the PRE-norm output
        if idx in bw.ctx.coords_of:
            T.scatter_rows(dtap.pop(idx), bw.ctx.coords_of[idx], T.interior(fr), accumulate=True)
        else:
            T.import_ncdhw(dtap.pop(idx), T.interior(fr), accumulate=True)
    return fr


def _stem_weight_grad(fr, x0, cout):
    """The stem's weight gradient, on the image with its mean taken out.  An image is one-signed and the gradient of the stem's raw
    output has zero channel sums (the norm adjoint removes them), so sum dY x cancels to 1/500 of its terms while the 32 products
    of every MFMA step share a sign: at 2 x (32, 48, 80) in f16 the kernel on x itself stood at rel-L2 1.01e-5 of float64, and at
    6.6e-7 on x - 0.5 (tests/test_backward_walk_gpu.py).  So: dW = sum dY (x - c) + c sum dY with c the image's mean; x - c goes
    into two of the sixteen stored channels the kernel reads anyway (its 16-bit rounding and what that leaves), the sum of dY is
    taken in double.  Inline: the stem is the last block and normally has no data gradient to run beside."""
    d = x0[..., 0].float()
    c = d.mean()
    d = d - c
    hi = d.to(x0.dtype)
    xs = torch.zeros_like(x0)
    xs[..., 0] = hi
    xs[..., 1] = (d - hi.float()).to(x0.dtype)
    dw = T.conv_wgrad(fr, xs, None, 2, cout)
    total = T.interior(fr)[..., :cout].sum((0, 1, 2, 3), dtype=torch.float64)
    return dw[:, :1] + dw[:, 1:] + (c.double() * total).float().view(-1, 1, 1, 1, 1)


def _weight_grad(bw, blk, fr, x0, x1):
    # The weight gradient and the data gradient of a block both read `fr` and nothing else of each other: the weight
    # gradient goes to a side stream (result and scratch preallocated / cached on this one) and is joined before the next
    # block touches a framed buffer (they are shared per shape).  Letting it also run beside the next block's BatchNorm
    # adjoint (second frame per shape + events) measured slower: 11.4 vs 10.7 ms per step in round 2, and again 9.04 vs 8.71 ms in
    # round 3 with the one-round weight-gradient launches (the two MFMA kernels contend; the adjoint passes lose more than the join costs).
    conv, cin, cout = blk.conv, blk.conv.in_channels, blk.conv.out_channels
    if blk.inputs[0] == "x" and cin == 1 and x1 is None:
        bw.pgrads[id(conv.weight)] = _stem_weight_grad(fr, x0, cout)
    elif x0.is_cuda and x0.shape[3] >= OVERLAP_WGRAD_MIN_W:
        dw = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float32, device=x0.device)
        T.wgrad_scratch(x0, x1, cout)                                    # make sure the cached scratch exists (allocated here)
        side = _side_stream(x0.device)
        side.wait_stream(torch.cuda.current_stream(x0.device))
        with torch.cuda.stream(side):
            T.conv_wgrad(fr, x0, x1, cin, cout, out=dw)
        bw.pgrads[id(conv.weight)] = dw
        bw.wgrad_pending = side
    else:
        bw.pgrads[id(conv.weight)] = T.conv_wgrad(fr, x0, x1, cin, cout)
    if conv.bias is not None:                                            # d bias = sum of the pre-norm gradient over the voxels
        bw.pgrads[id(conv.bias)] = T.interior(fr).float().sum((0, 1, 2, 3))[:cout]


def _dgrad_route(blk, fr, x0, x1):
    """Which data-gradient route a block takes: 'stem' / 'split48' / 'direct' / 'upcat' / 'fold' (the reasons sit with each route)."""
    conv, c0, c1 = blk.conv, x0.shape[-1], 0 if x1 is None else x1.shape[-1]
    if blk.inputs[0] == "x":
        return "stem"
    if x1 is not None and conv.out_channels == 16 and c0 == 16 and c1 == 32 and tuple(conv.weight.shape[:2]) == (16, 48):
        return "split48"
    if x1 is None and blk.cat is None and T.dgrad_direct_supported(fr, conv.weight):
        return "direct"
    # (the framed data gradient comes back with the conv's input channels padded to a multiple of 16)
    if x1 is not None and (conv.in_channels + 15) // 16 * 16 == c0 + c1 and c0 % 8 == 0 and c1 % 8 == 0:
        return "upcat"
    return "fold"


def _dgrad_stem(bw, blk, fr, x0, x1):
    if bw.ctx.needs_input_grad[1]:                                       # d loss / d image: the stem's data gradient (channel 0 of
        bw.dx_in = T.conv_dgrad(fr, blk.conv.weight)[..., 0].float().unsqueeze(1)   # the 16-channel padded result)


def _dgrad_split48(bw, blk, fr, x0, x1):
    # the level-0 concat layer (48 -> 16): its data gradient is a 16 -> 48 convolution on the framed domain, which only the
    # generic kernel takes as one launch (415 us at 128^3 x 2 views); as a 16 -> 16 (skip channels) and a 16 -> 32
    # (upsampled channels) launch both halves run on the z-marching kernels, and the halves feed different consumers anyway
    (in0, in1), c0 = blk.inputs, x0.shape[-1]
    w = blk.conv.weight.detach()
    w_skip = w[:, :c0].contiguous()
    g_up = T.conv_dgrad_framed(fr, w[:, c0:].contiguous())
    if T.dgrad_direct_supported(fr, w_skip):
        bw.add_grad(in0, T.conv_dgrad_direct(fr, w_skip))
    else:
        bw.grads[in0] = T.pad_fold(T.conv_dgrad_framed(fr, w_skip), bw.grads.get(in0))
    bw.add_grad(in1, T.upcat_split_backward_framed(g_up, 0, x1.shape[-1])[1])


def _dgrad_direct(bw, blk, fr, x0, x1):
    # the forward kernel on the interior of the framed gradient + the folded shell terms: no (n + 4)^3 domain, no fold pass
    g = T.conv_dgrad_direct(fr, blk.conv.weight, wpk=bw.packs.take(blk.idx, fr.shape[-1], fr.shape[3] - 4))
    bw.add_grad(blk.inputs[0], g[..., : x0.shape[-1]] if g.shape[-1] != x0.shape[-1] else g)


def _dgrad_upcat(bw, blk, fr, x0, x1):
    # reflect-padding adjoint, channel split and the sum over the 8 children of every low-resolution voxel (adjoint of
    # the nearest x2 upsample) in ONE pass over the framed result; the skip part accumulates in place when the skip
    # already has a gradient
    in0, in1 = blk.inputs
    g_fr = T.conv_dgrad_framed(fr, blk.conv.weight, wpk=bw.packs.take(blk.idx, fr.shape[-1], fr.shape[3]))
    dskip, dlow = T.upcat_split_backward_framed(g_fr, x0.shape[-1], x1.shape[-1], skip_into=bw.grads.get(in0))
    bw.grads[in0] = dskip
    bw.add_grad(in1, dlow)


def _dgrad_fold(bw, blk, fr, x0, x1):
    """The framed data gradient, the reflect fold, then one of three tails: trilinear concat / plain input / nearest concat."""
    in0, in1 = blk.inputs
    dcat = T.pad_fold(T.conv_dgrad_framed(fr, blk.conv.weight, wpk=bw.packs.take(blk.idx, fr.shape[-1], fr.shape[3])))
    c0 = x0.shape[-1]
    if blk.cat == "materialised":                                        # materialised trilinear concat: split, then the adjoint
        cs = bw.tensors[blk.src].shape[-1]
        bw.add_grad(blk.src, dcat[..., :cs].contiguous())
        bw.add_grad(blk.low, T.upsample2_trilinear_backward(dcat[..., cs: cs + bw.tensors[blk.low].shape[-1]]))
    elif x1 is None:
        bw.add_grad(in0, dcat[..., :c0] if dcat.shape[-1] != c0 else dcat)
    else:
        bw.add_grad(in0, dcat[..., :c0].contiguous())
        bw.add_grad(in1, _sum_children(dcat[..., c0: c0 + x1.shape[-1]], bw.dt))


_DGRAD = {"stem": _dgrad_stem, "split48": _dgrad_split48, "direct": _dgrad_direct, "upcat": _dgrad_upcat, "fold": _dgrad_fold}


def _data_grad(bw, blk, fr, x0, x1):
    _DGRAD[_dgrad_route(blk, fr, x0, x1)](bw, blk, fr, x0, x1)


# ---- the autograd function: two drivers over the plan ---------------------------------------------------------------------------

class _UnetTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, x, layers, sampler, on_start, *params):
        # sampler (None: dense taps): callable (module id, (d, h, w)) -> int64 coords [P, 3]; the taps then come back as the P sampled
        # rows [N, P, C] fp32 of each tapped tensor (gathered in place from the 16-bit channels-last storage) instead of dense fp32
        # NCDHW copies, and the backward scatters the row gradients straight into the framed gradient buffers
        steps = plan_network(model, layers, sampler is not None)
        dt = _DT[model.train_precision]
        trilinear = model._cfg["interp"] == "trilinear"
        # an output nobody differentiates (the network output next to sampled taps: 268 MB at 128^3) arrives as None in backward, not as a
        # dense zero tensor that would then be imported
        ctx.set_materialize_grads(False)
        xin, packs, bwd_packs = _import_and_pack(model, x, dt)
        run = _Run(xin, packs, sampler, on_start)
        for st in steps:
            if isinstance(st, Pool):
                _run_pool(run, st)
            elif isinstance(st, Up):
                if st.tap:
                    _run_up_tap(run, st, trilinear)
            else:
                if st.cat == "materialised":
                    # trilinear: the upsampled tensor is materialised and concatenated (the nearest case is fused into the conv)
                    run.tensors[st.inputs[0]] = torch.cat([run.tensors[st.src], T.upsample2_trilinear(run.tensors[st.low])], dim=-1)
                _RUN_BLOCK[st.kind](run, st)
                run.start()
        packs.save()
        if run.tracked:
            torch._foreach_add_(run.tracked, 1)
        ctx.model, ctx.steps, ctx.tensors, ctx.saved, ctx.dt, ctx.trilinear = model, steps, run.tensors, run.saved, dt, trilinear
        ctx.coords_of, ctx.layers, ctx.pkey = run.coords_of, sorted(run.taps), packs.key
        ctx.bpacks_pre = bwd_packs if bwd_packs.packs else None
        ctx.param_ids = [id(p) for p in model.parameters()]
        # popped, not read: the backward never needs the network's output, and an OUTPUT kept in ctx is a reference cycle (output ->
        # grad_fn -> ctx -> output) that only the garbage collector frees -- until then the parameters' AccumulateGrad nodes stay bound
        # to the stream of this call, and a HIP-graph capture of the same modules would run them there (outside the capture)
        out = run.tensors.pop([st for st in steps if isinstance(st, ConvBlock)][-1].name)
        return (out,) + tuple(run.taps[l] for l in ctx.layers)

    @staticmethod
    def backward(ctx, dout, *dtaps):
        bw = _Adjoint(ctx, dtaps)
        _up_tap_grads(bw, ctx.steps, ctx.trilinear)
        bw.packs = _backward_packs(bw, ctx.bpacks_pre)
        for st in reversed(ctx.steps):
            if isinstance(st, Up):
                continue
            bw.join()
            if isinstance(st, Pool):
                _pool_adjoint(bw, st)
                continue
            fr = _output_adjoint(bw, st, dout) if st.kind == "output" else _norm_adjoint(bw, st)
            if fr is not None:
                x0, x1 = _inputs(bw.tensors, st)
                _weight_grad(bw, st, fr, x0, x1)
                _data_grad(bw, st, fr, x0, x1)
        bw.join()
        bw.packs.save()
        return (None, bw.dx_in, None, None, None) + tuple(bw.pgrads.get(pid) for pid in ctx.param_ids)


def forward_train(model, x, layers):
    """(out, feats) like Unet.forward(input, layers) -- or out alone when ``layers`` is empty -- differentiable."""
    layers = [int(l) for l in layers]
    final_idx = max(i for i, m in enumerate(model.model) if isinstance(m, nn.Conv3d))
    want = sorted({l for l in layers if l != final_idx})
    res = _UnetTrainFn.apply(model, x, tuple(want), None, None, *list(model.parameters()))
    out, taps = res[0], dict(zip(want, res[1:]))
    if not layers:
        return out
    feats = [out if l == final_idx else taps[l] for l in sorted(set(layers))]
    return out, feats


def forward_train_sampled(model, x, layers, sampler, on_start=None):
    """The differentiable train-mode forward with SAMPLED taps: returns ``(out, rows, coords, dims)`` -- per tapped module id (ascending) the
    fp32 rows [N, P, C] at the coordinates ``sampler(module id, (d, h, w))`` drew when the forward reached that tensor, those
    coordinates, and the tensor's spatial size.  Same values as gathering from ``forward_train``'s dense taps; the dense fp32 copies, their
    zero-filled gradients and the import passes are never made.  ``on_start()`` runs exactly once: right after the first block's kernels
    are enqueued, or immediately before the first ``sampler`` call, whichever comes first."""
    layers = sorted({int(l) for l in layers})
    dims, coords = {}, {}

    def recording(i, shape):
        dims[i] = tuple(shape)
        coords[i] = sampler(i, shape)
        return coords[i]

    res = _UnetTrainFn.apply(model, x, tuple(layers), recording, on_start, *list(model.parameters()))
    return res[0], list(res[1:]), [coords[l] for l in layers], [dims[l] for l in layers]
