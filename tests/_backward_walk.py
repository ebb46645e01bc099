"""The backward walk: every block of the training backward (anatomix_amd/model/train.py, ``_UnetTrainFn.backward``) checked on its
own, teacher-forced with the tensors the backward itself held.

``Recorder(TR)`` wraps the six module-level functions the backward looks up by name (``_norm_adjoint``, ``_output_adjoint``,
``_weight_grad``, ``_data_grad``, ``_pool_adjoint``, ``_up_tap_grads``) and copies, per block, what went in and what came out to the
host: the incoming 16-bit ``dy``, the tap cotangents, the stored ``X`` / ``Y`` / statistics, the whole framed buffer, the parameter
gradients the block wrote, and every input tensor's gradient before and after ``_data_grad``.  It adds no launch but those copies and
joins the side stream (``bw.join()``) before it copies, at the point where the backward's own next ``bw.join()`` stands.

``walk(rec, precision, k)`` then judges every stage against float64 arithmetic on exactly those operands (conv weights rounded to
storage, as tests/test_train_ops_gpu.py::test_conv_dgrad_and_wgrad does), so a wrong row of a partial tile is a failure of that
block's data gradient at that voxel and not 1e-4 of some parameter's rel-L2 downstream.

Stages and bounds
  norm    activation + norm adjoint into the framed buffer (train BatchNorm, InstanceNorm per sample, frozen block, no ``dy``), then
          the tap at the conv id added in 16 bit.  The activation's sign comes from ``a X + b``; voxels where the float64 value is
          within 2^-20 (|a X| + |b|) of zero are left out (the fp32 sign is not determined there), at most EXCLUDE_CAP of a block.
          The output conv's block is this stage too: the imported cotangent.
  vec     d gamma, d beta, conv bias gradient against float64 sums: rtol 2e-3, atol 2e-3 x the vector's max
          (test_bn_train_forward_and_backward).
  wgrad   rel-L2 < 1e-5 per layer (test_conv_dgrad_and_wgrad); the worst of the 27 taps is reported beside it, and so are the
          layer's condition number |sum of |terms|| / |dW| and the error in fp32 ulps of that sum of |terms|.
  dgrad   per input tensor the stored result r16(previous gradient + contribution), per element.
  pool    max: ``torch.equal`` with float64 autograd (first-max tie rule) when nothing is accumulated and no tap is added; otherwise, and
          for the average pool, per element.
  uptap   the split of a tap at an upsample id: skip part, child sum / trilinear adjoint of the rest, per element.
  frame   the frame of the returned framed buffer is all zero; everything is finite.

Per-element bound ``tol = R + A``.  ``R = u (1 + u)^p x sum |value at each of the p rounding points| + p x 2^-25 (f16)``, u = 2^-11 (f16),
2^-8 (bf16), from the float64 intermediates; the factor (1 + u)^p is the second order (a later point rounds an already rounded value),
not an allowance.  ``A = k 2^-24 S``, S the float64 sum of |terms| of the fp32 sums that feed the element.

Rounding points as the code has them (train.py, train_ops.py, amx_train.hip):
  direct   the interior launch stores its result; the shell launch (``dgrad_shell_kernel``) then reads that stored value back, adds the
           folded shell terms in fp32 and stores again -- so the near-face voxels (a coordinate equal to 1 or L - 2) have TWO rounding
           points, one more than "one rounding of the contribution"; every other voxel has one.
  fold     the padded-domain values (up to eight fold into one voxel), then the folded result.
  upcat    the padded domain, then one rounding of the skip part (previous gradient included) and one of the child sum.
  split48  the upsampled half: padded domain, then the child sum; the skip half: the direct route, or padded domain + accumulating fold.
  nearest concat via fold: the fold, then ``_sum_children``;  materialised trilinear: the fold, then the adjoint's store.
  frozen   du = dy act'(y) is stored, then multiplied IN 16 BIT by the folded scale rounded to storage (``du.mul_(a.to(dt))``): the
           reference multiplies by that rounded scale; two rounding points.
  norm     one store; a tap at the conv id one more.  add_grad / accumulate_into of an existing gradient: one more.
  avg pool ``dp * 0.125`` in 16 bit (exact but for f16 subnormals), then the add.

k, measured: the k at which the worst element of the torch fp32 emulation of the staged backward (tests/test_backward_walk.py, the
real train.py backward on emulated operators) just passes against the float64 reference on the same operands.  k is an extreme over
the elements of a block and grows with their number and with the length of the fp32 sums, so it is taken at the small networks the host
test runs AND at the shapes the device is judged at (``PYTHONPATH=. python tests/test_backward_walk.py`` prints the second row, about a minute):
    K_SMALL   batch-norm / max / nearest and instance / avg / trilinear at (8, 12, 40), f16 and bf16:  norm 0.2345  dgrad 1.5597  pool 0  uptap 0
    K_WALKED  the 6M network at cases A (f16, bf16), B, C of test_backward_walk_gpu.py:             norm 0.9353  dgrad 4.1756  pool 0
              (norm: module 62 of case C, 3 x 32 x 64 x 32 voxels per channel; dgrad: module 6 of case B, direct route)
(pool and uptap are zero because their fp32 sums -- one add, or eight children / 27 trilinear weights of 16-bit values -- are exact
or far inside R; err / R of the emulation peaks at 0.999 there, the store's own half ulp.)  K_EMUL is the larger of the two rows,
rounded up in the third digit, and the GPU limit is K_GPU = 4 x K_EMUL: the kernels' summation order and torch's differ, and neither
is privileged.  (With K_SMALL alone the device missed at one place: case C, module 62, norm, 2 voxels at err / tol 1.134, where the
emulation itself needs k = 0.935 of the 0.94 allowed.)

Worst measured err / tol on the MI355X per stage kind and precision (profiles/backward_walk_gpu.txt, every block of every case;
WORST_GPU below repeats them).  The per-element stages sit just under 1 because R is reached by the store's own half ulp:
    f16    norm 0.999   dgrad 0.994   pool 0.999   uptap 0.999   vec 0.226   wgrad 0.474 (case A, module 10)
    bf16   norm 0.992   dgrad 0.988   pool 0.992   (no uptap case)  vec 0.002   wgrad 0.223
Before ``_stem_weight_grad`` of model/train.py the stem's weight gradient of case A in f16 stood at 1.013 (rel-L2 1.01e-05 against
1e-5): see test_backward_walk_gpu.py::test_6m_backward_walk.
"""
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
EXCLUDE_CAP = 1e-4
SIGN_BAND = 2.0 ** -20
VEC_RTOL = VEC_ATOL = 2e-3               # test_bn_train_forward_and_backward
WGRAD_REL_L2 = 1e-5                      # test_conv_dgrad_and_wgrad
K_SMALL = {"norm": 0.235, "dgrad": 1.56, "pool": 0.0, "uptap": 0.0}
K_WALKED = {"norm": 0.936, "dgrad": 4.18, "pool": 0.0, "uptap": 0.0}
K_EMUL = {s: max(K_SMALL[s], K_WALKED[s]) for s in K_SMALL}
K_GPU = {s: 4.0 * v for s, v in K_EMUL.items()}
# worst err / tol of one MI355X run (profiles/backward_walk_gpu.txt), stage kind -> precision -> ratio
WORST_GPU = {"norm": {"f16": 0.999, "bf16": 0.992}, "dgrad": {"f16": 0.994, "bf16": 0.988}, "pool": {"f16": 0.999, "bf16": 0.992},
             "uptap": {"f16": 0.999}, "vec": {"f16": 0.226, "bf16": 0.002}, "wgrad": {"f16": 0.474, "bf16": 0.223}}
SLOPE = 0.3


# ---- the recorder ------------------------------------------------------------------------------------------------------------

def _cpu(t):
    return None if t is None else t.detach().to("cpu", copy=True)


class Recorder:
    """Context manager over ``anatomix_amd.model.train`` (``TR``).  After a backward: ``blocks`` (conv module id -> record), ``pools``
    (pool id -> record), ``uptaps`` (upsample id -> record), ``order`` (ids as the backward visited them).  ``on_block(idx)`` is
    called before each block / pool (the host emulation plants its defects by it)."""
    NAMES = ("_norm_adjoint", "_output_adjoint", "_weight_grad", "_data_grad", "_pool_adjoint", "_up_tap_grads")

    def __init__(self, TR, on_block=None):
        self.TR, self.on_block = TR, on_block or (lambda idx: None)
        self.blocks, self.pools, self.uptaps, self.order, self.frames = {}, {}, {}, [], []

    def __enter__(self):
        self._orig = {n: getattr(self.TR, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(self.TR, n, getattr(self, "_w" + n)(self._orig[n]))
        return self

    def __exit__(self, *exc):
        for n, f in self._orig.items():
            setattr(self.TR, n, f)

    # -- one wrapper per function
    def _w_up_tap_grads(self, orig):
        def f(bw, steps, trilinear):
            ups = [st for st in steps if isinstance(st, self.TR.Up) and st.tap and st.idx in bw.dtap]
            pre = {st.idx: SimpleNamespace(module=st.idx, trilinear=trilinear, g=_cpu(bw.dtap[st.idx]), skip=st.skip, low=st.low,
                                           cs=bw.tensors[st.skip].shape[-1],
                                           before={n: _cpu(bw.grads.get(n)) for n in (st.skip, st.low)}) for st in ups}
            orig(bw, steps, trilinear)
            for st in ups:
                pre[st.idx].after = {n: _cpu(bw.grads.get(n)) for n in (st.skip, st.low)}
                self.uptaps[st.idx] = pre[st.idx]
                self.order.append(st.idx)
        return f

    def _w_pool_adjoint(self, orig):
        def f(bw, st):
            self.on_block(st.idx)
            r = SimpleNamespace(module=st.idx, avg=st.avg, tap=_cpu(bw.dtap.get(st.idx)), dp=_cpu(bw.grads.get(st.dst)),
                                src=_cpu(bw.tensors[st.src]), before=_cpu(bw.grads.get(st.src)))
            orig(bw, st)
            r.after = _cpu(bw.grads.get(st.src))
            self.pools[st.idx] = r
            self.order.append(st.idx)
        return f

    def _begin(self, bw, blk):
        self.on_block(blk.idx)
        conv, bn = blk.conv, blk.norm
        sv = bw.saved.get(blk.idx)
        p = lambda t: None if t is None else _cpu(t).float()
        r = SimpleNamespace(module=blk.idx, kind=blk.kind, act=blk.act, cat=blk.cat, src=blk.src, low=blk.low, inputs=blk.inputs,
                            cin=conv.in_channels, cout=conv.out_channels, w=p(conv.weight), bias=p(conv.bias),
                            norm=None if bn is None else "batch" if isinstance(bn, nn.BatchNorm3d) else "instance",
                            gamma=None if bn is None else p(bn.weight), beta=None if bn is None else p(bn.bias),
                            eps=None if bn is None else bn.eps, dy=_cpu(bw.grads.get(blk.name)),
                            alias_taps=[_cpu(bw.dtap[j]) for j in blk.alias_ids if j in bw.dtap],
                            conv_tap=_cpu(bw.dtap.get(blk.idx)), coords=_cpu(bw.ctx.coords_of.get(blk.idx)), dout=None,
                            X=None if sv is None else _cpu(sv.X), Y=None if sv is None else _cpu(sv.Y),
                            mean=None if sv is None else _cpu(sv.mean), rstd=None if sv is None else _cpu(sv.rstd),
                            a=None if sv is None else _cpu(sv.a), fr=None, pg={}, route=None, side=False, grads=[], dx_in=None)
        self.blocks[blk.idx] = r
        self.order.append(blk.idx)
        return r

    def _w_norm_adjoint(self, orig):
        def f(bw, blk):
            r = self._begin(bw, blk)
            fr = orig(bw, blk)
            r.fr = _cpu(fr)
            if blk.norm is not None and blk.norm.weight is not None:
                r.pg["gamma"], r.pg["beta"] = _cpu(bw.pgrads.get(id(blk.norm.weight))), _cpu(bw.pgrads.get(id(blk.norm.bias)))
            if fr is not None:
                self.frames.append(fr)
            return fr
        return f

    def _w_output_adjoint(self, orig):
        def f(bw, blk, dout):
            r = self._begin(bw, blk)
            r.dout = _cpu(dout)
            fr = orig(bw, blk, dout)
            r.fr = _cpu(fr)
            if fr is not None:
                self.frames.append(fr)
            return fr
        return f

    def _w_weight_grad(self, orig):
        def f(bw, blk, fr, x0, x1):
            orig(bw, blk, fr, x0, x1)
            self.blocks[blk.idx].side = bw.wgrad_pending is not None       # (its result is copied after the join in _data_grad)
        return f

    def _w_data_grad(self, orig):
        def f(bw, blk, fr, x0, x1):
            r = self.blocks[blk.idx]
            r.route = self.TR._dgrad_route(blk, fr, x0, x1)
            r.x0, r.x1 = _cpu(x0), _cpu(x1)
            if r.route == "split48":                                       # (a host question, as _dgrad_split48 asks it)
                r.skip_direct = bool(self.TR.T.dgrad_direct_supported(fr, blk.conv.weight.detach()[:, :x0.shape[-1]].contiguous()))
            names = [blk.src, blk.low] if blk.cat == "materialised" else [n for n in blk.inputs if n is not None]
            r.chans = [bw.tensors[n].shape[-1] for n in names]
            before = [_cpu(bw.grads.get(n)) for n in names]
            orig(bw, blk, fr, x0, x1)
            bw.join()                                                      # where the backward's own next join stands
            r.grads = [(n, b, _cpu(bw.grads.get(n))) for n, b in zip(names, before)]
            r.dx_in = _cpu(bw.dx_in) if r.route == "stem" else None
            r.pg["weight"] = _cpu(bw.pgrads.get(id(blk.conv.weight)))
            if blk.conv.bias is not None:
                r.pg["bias"] = _cpu(bw.pgrads.get(id(blk.conv.bias)))
        return f


# ---- records -------------------------------------------------------------------------------------------------------------------

@dataclass
class Rec:
    module: int
    stage: str               # norm | vec | wgrad | dgrad | pool | uptap | frame
    route: str = ""
    what: str = ""           # which tensor / vector of the stage
    ratio: float = 0.0       # worst err / tol
    over: int = 0
    worst: tuple = ()
    got_at: float = 0.0
    ref_at: float = 0.0
    excluded: float = 0.0    # norm: share of voxels left out (sign of a X + b undetermined in fp32)
    r_ratio: float = 0.0     # worst err / R (what the rounding points alone explain)
    k_needed: float = 0.0    # the k that would just pass
    rel_l2: float = 0.0
    worst_tap: float = 0.0   # wgrad: the worst of the 27 taps' own rel-L2
    cond: float = 0.0        # wgrad: |sum of |terms|| / |dW| (L2 over the layer): how much of the fp32 sums cancels
    ulps_of_sum: float = 0.0  # wgrad: |error| / (2^-24 |sum of |terms||), L2
    side: bool = False
    ok: bool = True
    note: str = field(default="")

    def __str__(self):
        s = f"module {self.module:2d} {self.stage:5s} {self.route:8s} {self.what:14s} err/tol {self.ratio:6.3f} err/R {self.r_ratio:6.3f} over {self.over}"
        if self.worst != ():
            s += f" worst {self.worst} (got {self.got_at:.6g} ref {self.ref_at:.6g})"
        if self.stage == "norm":
            s += f" excluded {self.excluded:.1e}"
        if self.stage == "wgrad":
            s += (f" rel_l2 {self.rel_l2:.2e} worst tap {self.worst_tap:.2e} cond {self.cond:.0f} err {self.ulps_of_sum:.2f} fp32 ulp of sum|terms|"
                  f" {'side stream' if self.side else 'inline'}")
        return s + (f" [{self.note}]" if self.note else "") + f" {'ok' if self.ok else 'FAIL'}"


def report(recs):
    return "\n".join(str(r) for r in recs)


def summary(recs):
    """stage kind -> worst err / tol over the records."""
    out = {}
    for r in recs:
        out[r.stage] = max(out.get(r.stage, 0.0), r.ratio)
    return out


# ---- float64 helpers ---------------------------------------------------------------------------------------------------------------

def _nc(t):                         # NDHWC (any float type) -> NCDHW float64
    return t.double().permute(0, 4, 1, 2, 3).contiguous()


def _q(t, precision):               # round to storage, back to float64
    return t.to(DT[precision]).double()


def fold64(P):
    """Adjoint of reflect padding by one voxel on [N, C, D+2, H+2, W+2]: voxel 1 collects padded coordinate -1, voxel L - 2 collects L."""
    out = P
    for ax in (2, 3, 4):
        L = out.shape[ax] - 2
        core = out.narrow(ax, 1, L).clone()
        core.narrow(ax, 1, 1).add_(out.narrow(ax, 0, 1))
        core.narrow(ax, L - 2, 1).add_(out.narrow(ax, L + 1, 1))
        out = core
    return out


def children64(t):
    n, c, d, h, w = t.shape
    return t.reshape(n, c, d // 2, 2, h // 2, 2, w // 2, 2).sum((3, 5, 7))


def up_nearest64(t):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)


def tri_adjoint64(g):
    n, c, d, h, w = g.shape
    z = torch.zeros(n, c, d // 2, h // 2, w // 2, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.interpolate(z, scale_factor=2, mode="trilinear"), z, g)[0]


def _near_face(shape):
    m = torch.zeros(shape[2:], dtype=torch.bool)
    for a, s in enumerate(shape[2:]):
        idx = [slice(None)] * 3
        for v in (1, s - 2):
            idx[a] = v
            m[tuple(idx)] = True
    return m[None, None]


def _elementwise(module, stage, route, what, got, ref, rsum, points, S, precision, k, keep=None):
    """One per-element record: tol = u (1 + u)^p rsum + p 2^-25 (f16) + k 2^-24 S; ``keep``: voxels that are judged."""
    u = U[precision]
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (module, stage, what, got.shape, ref.shape)
    R = u * (1 + u) ** points * rsum + (points * 2.0 ** -25 if precision == "f16" else 0.0)
    A = 2.0 ** -24 * S
    tol = R + k * A
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    if keep is not None:
        err = torch.where(keep, err, torch.zeros_like(err))
    tiny = 1e-300
    ratio = err / (tol + tiny)
    rec = Rec(module, stage, route, what, ratio=float(ratio.max()), over=int((err > tol).sum()),
              r_ratio=float((err / (R + tiny)).max()), k_needed=float(((err - R).clamp_min(0) / (A + tiny)).max()))
    rec.worst = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), err.shape))
    rec.got_at, rec.ref_at = float(got[rec.worst]), float(ref[rec.worst])
    rec.ok = rec.over == 0 and bool(torch.isfinite(got).all())
    return rec


def _vector(module, what, got, ref):
    got, ref = got.double(), ref.double()
    tol = VEC_ATOL * float(ref.abs().max()) + VEC_RTOL * ref.abs()
    err = (got - ref).abs()
    ratio = err / (tol + 1e-300)
    i = int(ratio.argmax())
    return Rec(module, "vec", "", what, ratio=float(ratio.max()), over=int((err > tol).sum()), worst=(i,), got_at=float(got[i]),
               ref_at=float(ref[i]), ok=bool((err <= tol).all()) and bool(torch.isfinite(got).all()))


# ---- stage references ----------------------------------------------------------------------------------------------------------------

def _act_grad(u, act):
    one = torch.ones_like(u)
    return torch.where(u > 0, one, SLOPE * one) if act == "lrelu" else (u > 0).double() if act == "relu" else one


def check_norm(b, precision, k):
    """The framed buffer's interior after the norm / output adjoint, the norm's parameter gradients, and the frame."""
    recs = []
    fr = b.fr
    got = _nc(fr[:, 2:-2, 2:-2, 2:-2, :b.cout])
    border = fr.clone()
    border[:, 2:-2, 2:-2, 2:-2, :].zero_()
    nz = int((border != 0).sum())
    recs.append(Rec(b.module, "frame", "", "border", ratio=float("inf") if nz else 0.0, over=nz,
                    worst=tuple(int(v) for v in border.nonzero()[0]) if nz else (), ok=nz == 0 and bool(torch.isfinite(fr.float()).all())))
    zero = torch.zeros_like(got)
    keep, excluded, what = None, 0.0, b.kind
    if b.kind == "output":
        ref = zero if b.dout is None else b.dout.double()
        rsum, points, S = ref.abs(), 1, zero
    else:
        dy = None if b.dy is None else _nc(b.dy[..., :b.cout])
        for t in b.alias_taps:                                             # imported in 16 bit: r16(dy + tap)
            dy = _q(t.double() if dy is None else dy + t.double(), precision)
        c = b.cout
        v = lambda t, d: torch.full((c,), d, dtype=torch.float64) if t is None else t.double()[:c]
        gamma, beta = v(b.gamma, 1.0), v(b.beta, 0.0)
        if dy is None:
            ref, rsum, points, S, what = zero, zero, 0, zero, "no dy"
        elif b.kind == "frozen":
            a16 = _q(b.a[:c], precision).view(1, -1, 1, 1, 1)
            Y = _nc(b.Y[..., :c])
            du = dy * _act_grad(Y, b.act)
            ref = du * a16
            rsum, points, S = 2 * ref.abs(), 2, ref.abs()
            if b.gamma is not None:
                uu = Y if b.act != "lrelu" else torch.where(Y > 0, Y, Y / SLOPE)
                s1 = du.sum((0, 2, 3, 4))
                recs.append(_vector(b.module, "d beta", b.pg["beta"], s1))
                recs.append(_vector(b.module, "d gamma", b.pg["gamma"], ((du * uu).sum((0, 2, 3, 4)) - beta * s1) / gamma))
        else:
            X = _nc(b.X[..., :c])
            per_sample = b.norm == "instance"
            mean, rstd = b.mean.double()[..., :c], b.rstd.double()[..., :c]
            shp = (-1, c, 1, 1, 1) if per_sample else (1, c, 1, 1, 1)
            dims = (2, 3, 4) if per_sample else (0, 2, 3, 4)
            a = (gamma * rstd).view(shp)
            bb = beta.view(1, c, 1, 1, 1) - mean.view(shp) * a
            uu = a * X + bb
            keep = uu.abs() > SIGN_BAND * ((a * X).abs() + bb.abs())
            excluded = 1.0 - float(keep.double().mean())
            g = dy * _act_grad(uu, b.act)
            xh = (X - mean.view(shp)) * rstd.view(shp)
            M = X[0, 0].numel() * (1 if per_sample else X.shape[0])
            s1, s2 = g.sum(dims, keepdim=True), (g * xh).sum(dims, keepdim=True)
            ref = a * (g - s1 / M - xh * s2 / M)
            a1, a2 = g.abs().sum(dims, keepdim=True), (g * xh).abs().sum(dims, keepdim=True)
            S = a.abs() * (g.abs() + a1 / M + xh.abs() * a2 / M)
            rsum, points = ref.abs(), 1
            if b.gamma is not None:
                recs.append(_vector(b.module, "d beta", b.pg["beta"], s1.sum(0).flatten()))
                recs.append(_vector(b.module, "d gamma", b.pg["gamma"], s2.sum(0).flatten()))
            what = b.norm
    if b.conv_tap is not None:                                             # tap at the conv id: added to the stored value in 16 bit
        assert b.coords is None, "sampled taps are not walked"
        ref = ref + b.conv_tap.double()
        rsum, points, S = rsum + ref.abs(), points + 1, S + ref.abs()
        what += " + tap"
    rec = _elementwise(b.module, "norm", "", what, got, ref, rsum, points, S, precision, k["norm"], keep)
    rec.excluded = excluded
    rec.ok = rec.ok and excluded <= EXCLUDE_CAP
    recs.append(rec)
    return recs


def _dgrad_parts(b, P, Pabs, prevs, precision):
    """Per input tensor of the block: (name, reference, sum of |values| at the rounding points, points, S) of the CONTRIBUTION and its
    accumulation into the previous gradient.  P / Pabs: the padded-domain gradient and its sum of |terms|, [N, Cin, D+2, H+2, W+2]."""
    folded, fabs, fS = fold64(P), fold64(P.abs()), fold64(Pabs)
    c0 = b.chans[0]
    out = []

    def add(name, c, rsum, points, S, prev, fused=False):
        """``fused``: the previous gradient enters the contribution's last store (skip_into / accumulate_into); else add_grad."""
        if prev is None:
            out.append((name, c, rsum + c.abs(), points + 1, S))
        elif fused:
            out.append((name, prev + c, rsum + (prev + c).abs(), points + 1, S))
        else:
            out.append((name, prev + c, rsum + c.abs() + (prev + c).abs(), points + 2, S))

    def direct(name, ch, prev):
        interior = P[:, ch, 1:-1, 1:-1, 1:-1]
        c = folded[:, ch]
        nf = _near_face(c.shape).double()
        # interior store everywhere; on the near-face voxels the stored value is read back and stored again with the shell terms
        rs = interior.abs() + nf * c.abs()
        if prev is None:
            out.append((name, c, rs, 2, fS[:, ch]))
        else:
            out.append((name, prev + c, rs + (prev + c).abs(), 3, fS[:, ch]))

    names = [n for n, _, _ in b.grads]
    s0, s1 = slice(0, c0), (slice(c0, c0 + b.chans[1]) if len(names) > 1 else None)
    route = b.route
    if route == "direct":
        direct(names[0], slice(0, b.cin), prevs[0])
    elif route == "upcat":
        add(names[0], folded[:, s0], fabs[:, s0], 8, fS[:, s0], prevs[0], fused=True)
        add(names[1], children64(folded[:, s1]), children64(fabs[:, s1]), 64, children64(fS[:, s1]), prevs[1])
    elif route == "split48":
        if b.skip_direct:
            direct(names[0], s0, prevs[0])
        else:
            add(names[0], folded[:, s0], fabs[:, s0], 8, fS[:, s0], prevs[0], fused=True)
        add(names[1], children64(folded[:, s1]), children64(fabs[:, s1]), 64, children64(fS[:, s1]), prevs[1])
    elif route == "fold" and len(names) == 1:
        add(names[0], folded[:, :b.cin], fabs[:, :b.cin], 8, fS[:, :b.cin], prevs[0])
    elif route == "fold":
        add(names[0], folded[:, s0], fabs[:, s0], 8, fS[:, s0], prevs[0])
        adj = tri_adjoint64 if b.cat == "materialised" else children64
        add(names[1], adj(folded[:, s1]), adj(fabs[:, s1] + folded[:, s1].abs()), 72, adj(fS[:, s1]), prevs[1])
    return out


def check_conv(b, precision, k):
    """Weight gradient, conv bias gradient and the data gradient of one block, from the recorded framed buffer and stored inputs."""
    recs = []
    G = _nc(b.fr[:, 2:-2, 2:-2, 2:-2, :b.cout])
    wq = _q(b.w, precision)
    xin = _nc(b.x0) if b.x1 is None else torch.cat((_nc(b.x0), up_nearest64(_nc(b.x1))), 1)
    xp = F.pad(xin[:, :b.cin], (1,) * 6, mode="reflect")
    dw = torch.nn.grad.conv3d_weight(xp, wq.shape, G)
    got = b.pg["weight"].double()
    num, den = (got - dw).flatten(2), dw.flatten(2)
    taps = num.norm(dim=(0, 1)) / den.norm(dim=(0, 1)).clamp_min(1e-300)
    r = Rec(b.module, "wgrad", b.route, "d weight", rel_l2=float(num.norm() / den.norm().clamp_min(1e-300)), worst_tap=float(taps.max()),
            worst=tuple(int(v) for v in np.unravel_index(int(taps.argmax()), (3, 3, 3))), side=b.side)
    S = torch.nn.grad.conv3d_weight(xp.abs(), wq.shape, G.abs())
    r.cond = float(S.norm() / dw.norm().clamp_min(1e-300))
    r.ulps_of_sum = float(num.norm() / (2.0 ** -24 * S.norm()).clamp_min(1e-300))
    r.ratio = r.rel_l2 / WGRAD_REL_L2
    r.over = int(r.rel_l2 >= WGRAD_REL_L2)
    r.ok = r.rel_l2 < WGRAD_REL_L2 and bool(torch.isfinite(got).all())
    recs.append(r)
    if "bias" in b.pg:
        recs.append(_vector(b.module, "d bias", b.pg["bias"], G.sum((0, 2, 3, 4))))
    if b.route == "stem":
        if b.dx_in is None:
            return recs
        P = F.conv_transpose3d(G, wq)
        Pabs = F.conv_transpose3d(G.abs(), wq.abs())
        c = fold64(P)
        recs.append(_elementwise(b.module, "dgrad", "stem", "d image", b.dx_in, c, fold64(P.abs()) + c.abs(), 9, fold64(Pabs), precision, k["dgrad"]))
        return recs
    P = F.conv_transpose3d(G, wq)
    Pabs = F.conv_transpose3d(G.abs(), wq.abs())
    prevs = [None if p is None else _nc(p) for _, p, _ in b.grads]
    parts = _dgrad_parts(b, P, Pabs, prevs, precision)
    assert len(parts) == len(b.grads), (b.module, b.route)
    for (name, ref, rsum, points, S), (_, _, after), ch in zip(parts, b.grads, b.chans):
        recs.append(_elementwise(b.module, "dgrad", b.route, f"d {name}", _nc(after[..., :ref.shape[1]]), ref, rsum, points, S, precision, k["dgrad"]))
    return recs


def check_pool(p, precision, k):
    src = _nc(p.src)
    dp = None if p.dp is None else _nc(p.dp)
    rs_dp, pts = 0.0, 0
    if p.tap is not None:                                                  # r16(dp + tap), or the imported tap alone
        dp = p.tap.double() if dp is None else dp + p.tap.double()
        rs_dp, pts = dp.abs(), 1
    zero_dp = 0 * dp
    if p.avg:                                                              # dp * 0.125 is a 16-bit product: exact but for f16 subnormals
        routed = up_nearest64(dp * 0.125)
        rs, pts = up_nearest64((rs_dp if pts else zero_dp) * 0.125), pts + 1
    else:
        s = src.clone().requires_grad_(True)
        routed = torch.autograd.grad(F.max_pool3d(s, 2), s, dp)[0]
        mask = torch.autograd.grad(F.max_pool3d(s, 2), s, torch.ones_like(dp))[0]
        rs = mask * up_nearest64(rs_dp if pts else zero_dp)
    prev = None if p.before is None else _nc(p.before)
    got = _nc(p.after)
    if prev is None and pts == 0:
        bad = got != routed
        n_bad = int(bad.sum())
        return [Rec(p.module, "pool", "max", "d src (equal)", ratio=float("inf") if n_bad else 0.0, over=n_bad,
                    worst=tuple(int(v) for v in bad.nonzero()[0]) if n_bad else (), ok=n_bad == 0 and bool(torch.isfinite(got).all()))]
    ref = routed
    if prev is not None:                                                   # the accumulating store / add_grad
        ref = prev + routed
        rs, pts = rs + ref.abs(), pts + 1
    return [_elementwise(p.module, "pool", "avg" if p.avg else "max", "d src", got, ref, rs, pts, ref.abs(), precision, k["pool"])]


def check_uptap(t, precision, k):
    g = t.g.double()
    gs, gu = g[:, :t.cs], g[:, t.cs:]
    adj = tri_adjoint64 if t.trilinear else children64
    recs = []
    for name, ref, rsum, points in ((t.skip, gs, gs.abs(), 1), (t.low, adj(gu), adj(gu.abs()) + adj(gu).abs(), 9)):
        prev = t.before[name]
        if prev is not None:
            ref = _nc(prev) + ref
            rsum, points = rsum + ref.abs(), points + 1
        recs.append(_elementwise(t.module, "uptap", "trilinear" if t.trilinear else "nearest", f"d {name}", _nc(t.after[name]), ref, rsum,
                                 points, adj(gu.abs()) if name == t.low else 0 * ref, precision, k["uptap"]))
    return recs


def walk(rec, precision, k=K_GPU, only=None):
    """One list of Rec over everything the recorder holds, in the backward's order.  ``only``: restrict to these module ids."""
    out = []
    for idx in rec.order:
        if only is not None and idx not in only:
            continue
        if idx in rec.uptaps:
            out += check_uptap(rec.uptaps[idx], precision, k)
        elif idx in rec.pools:
            out += check_pool(rec.pools[idx], precision, k)
        else:
            b = rec.blocks[idx]
            if b.fr is None:
                out.append(Rec(idx, "norm", "", "skipped", note="no gradient reached the block"))
                continue
            out += check_norm(b, precision, k)
            out += check_conv(b, precision, k)
    return out
