"""The layer walk: every layer of a U-Net forward checked on its own, teacher-forced with the tensors the forward itself stored.

``walk(kw, sd, x, taps, precision, routes)`` goes through ``oracle.unet_ref.build_plan`` group by group.  The input of each layer
is the tap in front of it (what the production kernel stored, exactly representable in the storage type), the reference is a
float64 convolution of those values with the weights folded as the pack step folds them (in fp32) and rounded to storage, and the
bound is what ONE rounding of the result can cost.  A wrong row of a ragged tile at a deep level is then a failure of that layer at that voxel, not 1e-4 of an
end-of-network rel-L2.

Which taps keep the production schedule (amx_unet.hip, ``Forward::plan_conv`` and what it calls, ``plan_norm``, ``pool``).  On a batch-norm /
nearest / max-pool network a feature tap at an ACTIVATION id or at a POOL id is a plain export of the tensor the production kernel
stored: it changes no launch.  Exactly three things reroute a forward:

  1. a tap at a conv id that a BatchNorm follows (``ConvPlan::raw_bn``, set in ``plan_terms``: the conv runs on its unfolded weights,
     the norm in a pass of its own);
  2. a tap before module ``g1 - 1`` in ``plan_stem_pair`` (the stem's tensor has to reach memory: two launches instead of the pair);
  3. on the ``f16x2mx`` networks, any tap at all (``taps`` in the first line of ``plan_norm``, and ``conv_only``).

So the walk of the plain forward taps the activation ids from the one behind the stem pair on, the pool ids and the output conv;
a second run adds the stem's activation id and must agree with the first bit for bit behind the pair.  Because of 3. the
``anatomix-dev`` / ``f16x2mx`` network is NOT walked: a walk there would check a schedule the plain forward does not run.

Reference per route (``routes``: conv module id -> the kernel name ``profile_forward`` reports for it):

  * one input, or a decoder concat conv on the generic kernel .. ``_util.ref_conv`` (float64 sums) on the taps;
  * ``conv3d_upcat16`` ........................................ ``_util.ref_conv_upcat_merged`` (merged taps, rounded once);
  * ``... + upmerge<...>`` .................................... ``_util.ref_conv_upcat_merged(round_partial=True)``: the skip conv's
    partial sums are stored in 16 bits, so a partial sum may round the other way after fp32 accumulation.  Three conditions, those
    of test_conv_kernel_gpu.py::test_merged_concat_conv_matches_cpu: every voxel within ``ulp * (|ref| + 4) + 2e-5``, a share of
    voxels over the one-rounding bound below 2e-3, and the rel-L2 limit.  The record also carries the share that a CPU emulation of
    the two launches (fp32 accumulation, partial sums rounded to storage) shows on the same inputs: the cap has to hold for it too;
  * pool id ................................................... ``torch.equal`` with ``max_pool3d`` of the tap in front;
  * output conv (fp32 planar) ................................. ``max_rel < 2e-5``;
  * strict (bf16x2) ........................................... operands through ``q_storage(., "bf16x2")``, ``rel_l2 < 2e-5`` and
    ``max_rel < 8e-5`` per layer.

One-rounding bound per voxel: ``ulp * |ref| + 1e-3 * ulp + 2e-5`` with ``ulp = 2^-10`` (f16) or ``2^-7`` (bf16), the bound of
test_conv_kernel_gpu.py::test_conv_matches_cpu.  No share of voxels is excluded from it.
"""
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from _util import SPLIT, max_rel, q_storage, ref_conv, ref_conv_upcat_merged, rel_l2
from oracle import unet_ref as R

ULP = {"f16": 2.0 ** -10, "bf16": 2.0 ** -7}
STRICT_REL_L2, STRICT_MAX_REL = 2e-5, 8e-5        # test_conv_kernel_gpu.py::test_conv_strict_precision_matches_fp64 (bf16x2)
PLANAR_MAX_REL = 2e-5                             # test_conv_kernel_gpu.py::test_conv_planar_fp32_output
MERGED_SHARE = 2e-3                               # test_conv_kernel_gpu.py::test_merged_concat_conv_matches_cpu
MERGED_REL_L2 = {"f16": 4e-4, "bf16": 3.2e-3}     # ... the result's own rounding: 2^-11 / sqrt(3), 2^-8 / sqrt(3)
ACT = {"none": 0, "relu": 1, "lrelu": 2}
DEFAULTS = dict(ngf=24, norm="batch", final_act="none", activation="relu", pooling="Max", interp="nearest",
                use_skip_connection=True, norm_eps=1e-5, doubleconv=True)


@dataclass
class Rec:
    module: int            # conv or pool module id
    out_id: int            # id of the tap that holds the layer's stored result
    kind: str              # "conv" | "upcat16" | "upmerge" | "planar" | "strict" | "pool"
    route: str
    ratio: float           # worst err / tol over the voxels (pool: 0 or inf)
    over: int              # voxels over the bound
    worst: tuple           # (n, c, z, y, x) of the worst voxel
    ref_absmax: float
    got_at: float = 0.0    # stored / reference value at the worst voxel
    ref_at: float = 0.0
    rel_l2: float = 0.0
    max_rel: float = 0.0
    share: float = 0.0         # upmerge: share of voxels over the ONE-rounding bound
    emul_share: float = 0.0    # upmerge: the same share for the CPU emulation of the two launches
    ok: bool = True

    def __str__(self):
        s = f"module {self.module:2d} {self.kind:8s} err/tol {self.ratio:6.3f} over {self.over} worst {self.worst} (got {self.got_at:.6g} ref {self.ref_at:.6g}) |ref|max {self.ref_absmax:.3f}"
        if self.kind == "upmerge":
            s += f" flip share {self.share:.2e} (emulation {self.emul_share:.2e})"
        if self.kind in ("strict", "planar", "upmerge"):
            s += f" rel_l2 {self.rel_l2:.2e} max_rel {self.max_rel:.2e}"
        return s + f" {'ok' if self.ok else 'FAIL'}  {self.route}"


def family(name):
    """Kernel family of a profile record: the name up to '<', plus the merged-tap launch when one is attached."""
    return name.split("<")[0].strip() + (" + upmerge" if "+ upmerge" in name else "")


def routes_of(records):
    """conv / pool module id -> kernel name, from ``profile_forward``'s records.  The stem pair is one record at the stem's id."""
    return {r["module_idx"]: r["kernel"] for r in records}


def _kind(route, precision, final):
    if precision in SPLIT:
        return "strict"
    if final:
        return "planar"
    if "+ upmerge" in route:
        return "upmerge"
    return "upcat16" if route.startswith("conv3d_upcat16") else "conv"


def groups(kw):
    """The layers of the plan as the forward runs them: dicts with ``op`` in conv / pool, the module id, the id of the stored result
    (``out``) and the ids of the tensors read (``src``: None = the network input; ``skip``: the concat's first segment)."""
    full = {**DEFAULTS, **kw}
    assert full["norm"] in ("batch", "none") and full["pooling"] == "Max" and full["interp"] == "nearest", \
        "the walk covers the batch-norm / nearest / max-pool networks (see the module docstring)"
    p = R.build_plan(**{k: v for k, v in full.items() if k != "dimension"})
    out, cur, skips, skip, i, n = [], None, [], None, 0, len(p.kinds)
    last_conv = max(p.conv_io)
    while i < n:
        kind = p.kinds[i]
        if kind == "conv":
            j = i + 1
            while j < n and p.kinds[j] in ("norm", "act", "final_act"):
                j += 1
            has_act = "act" in p.kinds[i + 1:j]
            final = i == last_conv
            out.append(dict(op="conv", module=i, out=i if final else j - 1, src=cur, skip=skip, final=final,
                            act=ACT[full["final_act"] if final else (full["activation"] if has_act else "none")]))
            cur, skip, last = out[-1]["out"], None, j - 1
            i = j
        elif kind == "pool":
            out.append(dict(op="pool", module=i, out=i, src=cur))
            cur, last = i, i
            i += 1
        else:                     # "up": the next conv reads cat(skip, nearest_up2(cur))
            if full["use_skip_connection"]:
                skip = skips.pop()
            last = -1
            i += 1
        if full["use_skip_connection"] and last in p.encoder_idx:
            skips.append(cur)
    return out, p, full


def conv_params(sd, full, g, plan):
    """(weight, gain, shift) of a conv group as the forward's pack step sees them: the eval-mode BatchNorm is folded in FLOAT32
    (fold_norm_kernel: s = gamma / sqrtf(var + eps), t = beta - mean * s), and the references multiply weight and gain in fp32 as
    the pack kernels do.  A float64 fold is not the same operand: 1 to 88 of a layer's f16 weights then round the other way (10
    in module 24), each worth up to a whole ulp of an output (module 24, channel 19 then stood at 0.87 to 1.03 of the bound on
    every route).  The gain comes out of ``fold_conv_params`` on a weight of ones.  What is left: the device's gain can still be one
    fp32 ulp from this chain (its divide and square root are not this host's), which moved one weight each of modules 17 (channel
    22) and 62 (channel 7) of the seed-0 network; those channels reach 0.51 and 0.58 of the bound where every other layer stays at
    0.5, the cost of the store rounding."""
    i = g["module"]
    w = sd[f"model.{i}.weight"].float()
    ones = {**sd, f"model.{i}.weight": torch.ones(w.shape[0], 1, 1, 1, 1)}
    s, t = R.fold_conv_params(ones, full, i, plan, dtype=torch.float32)
    return w, s.reshape(-1), t


def _split_concat(g, taps):
    """(x0, x1) of a conv group: x1 is the half-resolution tensor of a decoder concat conv, else None."""
    if g["skip"] is not None:
        return taps[g["skip"]], taps[g["src"]]
    return taps[g["src"]], None


def emulate_upmerge(x0, x1, w, scale, shift, act, precision):
    """The two launches of the merged route on the CPU: skip conv accumulated in fp32 and rounded to storage, then the merged-tap
    part (``ref_conv_upcat_merged`` on a zero skip tensor: its float64 sums, taken as fp32), shift and activation in fp32, one store."""
    c0 = x0.shape[1]
    ws = w[:, :c0] * scale[:, None, None, None, None]
    part = q_storage(R.conv3_reflect(q_storage(x0, precision), q_storage(ws, precision)), precision)
    up = ref_conv_upcat_merged(torch.zeros_like(x0), x1, w, scale, None, 0, precision, round_partial=True)
    y = part + up + shift.float()[None, :, None, None, None]
    y = F.relu(y) if act == 1 else (F.leaky_relu(y, 0.3) if act == 2 else y)
    return q_storage(y, precision)


def _reference(g, kind, x, taps, w, s, t, precision):
    prec = "bf16x2" if precision in SPLIT else precision
    if g["src"] is None:
        return ref_conv(x, None, w, s, t, g["act"], prec)            # (ref_conv rounds the input as the stem kernel does)
    x0, x1 = _split_concat(g, taps)
    if kind == "upmerge":
        return ref_conv_upcat_merged(x0, x1, w, s, t, g["act"], prec, round_partial=True)
    if kind == "upcat16" or (kind == "planar" and x1 is not None):
        return ref_conv_upcat_merged(x0, x1, w, s, t, g["act"], prec)
    return ref_conv(x0, x1, w, s, t, g["act"], prec)


def walk(kw, sd, x, taps, precision, routes, only=None):
    """Checks every layer whose input and output are both in ``taps`` (module id -> fp32 NCDHW CPU tensor; the network output
    belongs at the output conv's id).  ``routes``: conv module id -> kernel name (missing: the generic kernel).  Returns one Rec
    per checked layer; the caller asserts on ``ok`` and on WHICH modules were checked.  ``only``: restrict to these module ids."""
    gs, plan, full = groups(kw)
    recs = []
    for g in gs:
        need = [g["out"]] + [s for s in (g["src"], g.get("skip")) if s is not None]
        if any(s not in taps for s in need) or (only is not None and g["module"] not in only):
            continue
        got = taps[g["out"]].double()
        route = routes.get(g["module"], "")
        if g["op"] == "pool":
            ref = F.max_pool3d(taps[g["src"]], 2).double()
            bad = got != ref
            n_bad = int(bad.sum()) if got.shape == ref.shape else got.numel()
            worst = tuple(int(v) for v in bad.nonzero()[0]) if n_bad and got.shape == ref.shape else ()
            recs.append(Rec(g["module"], g["out"], "pool", route or "(fused into the conv in front)", ratio=float("inf") if n_bad else 0.0,
                            over=n_bad, worst=worst, ref_absmax=float(ref.abs().max()), ok=n_bad == 0))
            continue
        kind = _kind(route, precision, g["final"])
        w, s, t = conv_params(sd, full, g, plan)
        ref = _reference(g, kind, x, taps, w, s, t, precision).double()
        assert got.shape == ref.shape, (g["module"], got.shape, ref.shape)
        err = (got - ref).abs()
        rec = Rec(g["module"], g["out"], kind, route, ratio=0.0, over=0, worst=(), ref_absmax=float(ref.abs().max()),
                  rel_l2=rel_l2(got, ref), max_rel=max_rel(got, ref))
        if kind == "strict":
            # rel-L2 and max-rel measures: the ratio is the worse of the two against its limit, the worst voxel the largest error
            tol = torch.full_like(err, STRICT_MAX_REL * rec.ref_absmax)
            rec.ok = rec.rel_l2 < STRICT_REL_L2 and rec.max_rel < STRICT_MAX_REL
            rec.ratio = max(rec.rel_l2 / STRICT_REL_L2, rec.max_rel / STRICT_MAX_REL)
        elif kind == "planar":
            tol = torch.full_like(err, PLANAR_MAX_REL * rec.ref_absmax)
            rec.ok = rec.max_rel < PLANAR_MAX_REL
            rec.ratio = rec.max_rel / PLANAR_MAX_REL
        else:
            ulp = ULP[precision]
            one = ulp * ref.abs() + 1e-3 * ulp + 2e-5
            tol = one
            if kind == "upmerge":
                tol = ulp * (ref.abs() + 4.0) + 2e-5
                rec.share = float((err > one).double().mean())
                x0, x1 = _split_concat(g, taps)
                emu = emulate_upmerge(x0, x1, w, s, t, g["act"], precision).double()
                rec.emul_share = float(((emu - ref).abs() > one).double().mean())
                rec.ok = rec.share < MERGED_SHARE and rec.emul_share < MERGED_SHARE and rec.rel_l2 < MERGED_REL_L2[precision]
            rec.ratio = float((err / tol).max())
            rec.ok = rec.ok and bool((err <= tol).all())
        rec.over = int((err > tol).sum())
        rec.worst = tuple(int(v) for v in np.unravel_index(int((err / tol).argmax()), err.shape))
        rec.got_at, rec.ref_at = float(got[rec.worst]), float(ref[rec.worst])
        rec.ok = rec.ok and bool(torch.isfinite(got).all())
        recs.append(rec)
    return recs


def emulate(kw, sd, x, precision, routes):
    """Taps of a CPU emulation of the 16-bit forward, one per activation / pool id and the output conv: ``forward_lowp``'s arithmetic
    (operands rounded to storage, fp32 accumulation, shift and activation in fp32, one store rounding; the output conv stays fp32),
    collected per module.  The concat convs follow ``routes``: the merged routes use the merged weights, as their kernels do."""
    gs, plan, full = groups(kw)
    q = lambda v: q_storage(v, precision)
    taps = {}
    for g in gs:
        if g["op"] == "pool":
            taps[g["out"]] = F.max_pool3d(taps[g["src"]], 2)
            continue
        w, s, t = conv_params(sd, full, g, plan)
        wq = q(w * s[:, None, None, None, None])
        kind = _kind(routes.get(g["module"], ""), precision, g["final"])
        if g["src"] is None:
            y = R.conv3_reflect(q(x.float()), wq, t)
        elif g["skip"] is None:
            y = R.conv3_reflect(taps[g["src"]], wq, t)
        elif kind == "upmerge":
            taps[g["out"]] = emulate_upmerge(taps[g["skip"]], taps[g["src"]], w, s, t, g["act"], precision)
            continue
        elif kind == "upcat16":
            y = ref_conv_upcat_merged(taps[g["skip"]], taps[g["src"]], w, s, t, 0, precision)
        else:
            y = R.conv3_reflect(torch.cat((taps[g["skip"]], F.interpolate(taps[g["src"]], scale_factor=2, mode="nearest")), 1), wq, t)
        y = F.relu(y) if g["act"] == 1 else (F.leaky_relu(y, 0.3) if g["act"] == 2 else y)
        taps[g["out"]] = y if g["final"] else q(y)
    return taps


def report(recs):
    return "\n".join(str(r) for r in recs)
