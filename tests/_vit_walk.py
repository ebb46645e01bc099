"""The ViT stage walk: every stage of the engine forward (amx_vit.hip ``VitForward``) checked on its own, teacher-forced with the tensors
the forward itself stored (``PrimusV2.forward_hip(x, taps=...)``, names in include/anatomix_amd.h).

``walk(sd, kw, x, taps, only=None, samples=None, routes=None) -> [Rec]``: one record per stage.  The input of a stage is the tap in
front of it exactly as stored (hi + lo planes summed in float64, f16 operands as they are), the weights are rounded as the pack kernels
round them (``hi = w.half()``, ``lo = (w - hi).half()``, f16 alone in the blocks), the arithmetic is float64, and the bound is per
element -- no share of elements is excluded anywhere.  ``emulate(sd, kw, x)`` produces the same tap dictionary on the CPU with the
engine's arithmetic (fp32 compute, the storage roundings, attention in key blocks of 64 with f16 probabilities relative to the lazy
reference point, fp32 partial statistics, fp32 column-sum chunks): the walk must pass on it with room to spare, and the constants that
are not a single rounding come from it, never from GPU output.

Unit roundoffs: ``U32 = 2^-24``, ``U16 = 2^-11``.  Bound forms (``S = |a| @ |w|^T + |bias|`` in float64):

  * split product, fp32 result (tokenizer convs, ``tokens``, ``d*.raw``, ``y``) .. ``c_split(K) * S``, see ``c_split``;
  * f16-operand product into the fp32 residual stream (``tok1``, ``tok2``) ....... ``c_f16(K) * (|cur| + |gamma| S)``, see ``c_f16``;
  * results stored as f16 (``ln1``, ``ln_attn``, ``ln2``, ``ln_mlp``, ``hd``) ........ ``ULP16 |ref| + (fp32 arithmetic term) + 2^-24``, ULP16 = 2^-10:
    one rounding costs half of that, the other half and the small term are what the fp32 arithmetic in front of the rounding may move;
  * results stored as hi + lo (``h0``, ``a1``, ``h``, ``p``, ``d.ln``, ``d*.in``) ....... fp32-grade: ``HILO (sum of |terms|) + 2^-23``, HILO = 3 * 2^-22 (the
    2x2x2 averages: 2^-20 mean|h|, the stored h carries 2^-22 itself and seven more additions); GELU stages add ``erf_fast``'s stated
    error 1.5e-7 (amx_gemm.hip) times ``|z| / 2``;
  * InstanceNorm ``(scale, shift)`` against float64 statistics of the stored raw tensor, ``d.mean`` against the float64 channel mean of
    the reference output: ``C_SS`` / ``C_MEAN`` below;
  * the attention group ``ln1 -> attn``: q (after norm, rotary embedding and the log2(e) / sqrt(hd) scale), k and v rounded to f16 as the
    EPI_QK / EPI_VT epilogues round them, float64 softmax: ``C_ATT (P @ |V|) + C_ATT_SUM |ref|``;
  * every operand tap is exactly zero in its padding columns ``C .. ld - 1`` (counted into ``over`` of the stage that wrote it).

Constants that are not a single rounding -- worst value of the CPU emulation (cases A and B of tests/test_vit_walk.py, in units of
the bound's own form) and the constant used (at least 2x over it):

  ======================  ===========================================================  =================  ==========
  constant                form                                                         emulation's worst  used
  ======================  ===========================================================  =================  ==========
  ``C_SS``                ``C_SS U32`` relative error of E|r| and E[r^2] (slot sums)   1.8                8
  ``C_MEAN``              ``C_MEAN U32 (mean|x| @ |W| / 8 + |bias|)``                  0.28               2
  ``C_ATT = C_ATT_SUM``   ``C_ATT (P @ |V|) + C_ATT_SUM |ref|``                        1.9e-4             2^-11
  ======================  ===========================================================  =================  ==========

Worst err / tol per stage kind, clean emulation of cases A and B (tests/test_vit_walk.py asserts the limits in brackets): split 0.068
[0.15], resid 0.031 [0.08], f16 0.4993 [0.51: half of ULP16 is the rounding itself], hilo 0.36 [0.6], stats 0.22 [0.45], attn 0.38 [0.6].
One run of cases A - D on an MI355X (profiles/vit_walk_gpu.txt): split 0.052, resid 0.013, f16 0.4993, hilo 0.40, stats 0.22, attn 0.36.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

U32, U16, ULP16 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -10
ERF_FAST = 1.5e-7              # amx_gemm.hip, erf_fast: |error| of the Abramowitz-Stegun 7.1.26 polynomial
LAMBDA = 8.0                   # see c_split
STAGE_C = (32, 32, 64, 128)
F64 = torch.float64

# Worst observed value of the CPU emulation for each constant (tests/test_vit_walk.py::test_constants_have_their_margin re-measures
# them and asserts used >= 2 x worst), in the unit of the "form" column above.
_EMU_WORST = {"C_SS": 1.8, "C_MEAN": 0.28, "C_ATT": 1.9e-4}
C_SS = 8.0                     # a slot sum of 32 / 64 fp32 values: worst case 63 U32 in any order; the emulation shows 1.8 U32
C_MEAN = 2.0                   # column sums in fp32 chunks, combined in double; the emulation shows 0.28 U32
C_ATT = 2.0 ** -11             # f16 probabilities and f16 flips of q / k / v: 4.9e-4 = 2.6 x the emulation's 1.9e-4
C_ATT_SUM = 2.0 ** -11         # the row sum is a sum of the same f16 probabilities (measured together with C_ATT)
HILO = 3 * 2.0 ** -22          # hi + lo storage 2^-22 and up to five fp32 roundings of the elementwise arithmetic in front (5 U32)
FLOOR = 2.0 ** -23             # hi + lo stages: a lo plane below 2^-14 is subnormal, 2^-25 per stored value on the way in and out, x 4


def c_split(K):
    """Split (hi + lo) product with fp32 accumulation, K terms: ``acc = wh xh + wh xl + wl xh``.  Against the float64 product of
    ``(wh + wl)`` and ``(xh + xl)`` the dropped term is ``|wl xl| <= U16^2 |w||x|``.  The 3 K products are exact in fp32 (11 x 11 bits),
    their accumulation rounds: worst case ``(3 K + 2) U32 S``, which at K = 27 * 128 would hide a missing ``wl xh`` term (4.9e-4 S), so the
    bound is the probabilistic one for rounding errors of mean zero (Higham & Mary 2019, thm 2.4): ``LAMBDA sqrt(3 K + 4) U32`` fails with
    probability ``2 exp(-LAMBDA^2 / 2) = 2.5e-14`` per element at LAMBDA = 8 (the + 4: bias, position embedding / demean constant)."""
    return U16 * U16 + LAMBDA * math.sqrt(3 * K + 4) * U32


def c_f16(K):
    """f16 operands (exact in the reference) and fp32 accumulation over K terms, then ``cur + gamma * (acc + bias)`` in fp32: the
    probabilistic accumulation bound of ``c_split`` with K + 4 roundings."""
    return LAMBDA * math.sqrt(K + 4) * U32


@dataclass
class Rec:
    stage: str             # tap name of the stored result
    kind: str              # "split" | "resid" | "f16" | "hilo" | "stats" | "attn" | "exact"
    route: str
    ratio: float           # worst err / tol
    over: int              # elements over the bound + nonzero padding elements
    worst: tuple           # index of the worst element (in the stage's own layout)
    got_at: float
    ref_at: float
    ref_absmax: float
    pad_bad: int = 0
    ok: bool = True

    def __str__(self):
        return (f"{self.stage:10s} {self.kind:6s} err/tol {self.ratio:7.4f} over {self.over} worst {self.worst} (got {self.got_at:.7g} ref {self.ref_at:.7g}) "
                f"|ref|max {self.ref_absmax:.4g}{' PAD ' + str(self.pad_bad) if self.pad_bad else ''} {'ok' if self.ok else 'FAIL'}  {self.route}")


def report(recs):
    return "\n".join(str(r) for r in recs)


def up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------------ configuration
class Cfg:
    def __init__(self, sd, kw, x_shape):
        self.n = int(x_shape[0])
        self.vol = tuple(int(v) for v in x_shape[2:])
        self.grid = tuple(v // 8 for v in self.vol)
        self.E = int(sd["down_projection.proj.weight"].shape[0])
        self.Ep = up(self.E, 32)
        self.heads = int(kw["eva_numheads"])
        self.hd = self.E // self.heads
        self.V = int(np.prod(self.grid))
        self.nreg = int(kw.get("num_register_tokens", 0))
        self.T = self.V + self.nreg
        self.M = self.n * self.T
        self.depth = int(kw["eva_depth"])
        self.hid = int(sd["eva.blocks.0.mlp.fc1_g.weight"].shape[0])
        self.dec = [self.E, int(sd["up_projection.decode.0.0.weight"].shape[1]), int(sd["up_projection.decode.1.0.weight"].shape[1]),
                    int(sd["up_projection.decode.2.weight"].shape[1])]
        self.qk_norm = bool(kw.get("qk_norm", False))
        self.inner = bool(kw.get("scale_attn_inner", False))
        self.layer_scale = kw.get("init_values", None) is not None
        self.demean = str(kw.get("out_norm", "none")).lower() in ("demean", "center")
        self.in_eps = float(kw.get("in_eps", 1e-5))

    def fused(self, k):
        """decoder stage k runs LayerNorm + GELU inside the product (amx_vit.hip ``dec_fused``)."""
        return up(self.dec[k + 1], 16) == 128 and up(self.dec[k + 1], 32) <= 128


def tap_names(cfg, n_blocks=-1):
    nb = cfg.depth if n_blocks < 0 or n_blocks > cfg.depth else n_blocks
    names = ["h0", "p0"]
    for k in range(3):
        names += [f"s{k}.{s}" for s in ("raw1", "ss1", "a1", "raw2", "ss2", "raws", "sss", "h")] + ([f"s{k}.p"] if k < 2 else [])
    names.append("tokens")
    for b in range(nb):
        names += [f"b{b}.{s}" for s in ("ln1", "attn", "ln_attn", "tok1", "ln2", "hd", "ln_mlp", "tok2")]
    names.append("d.ln")
    for k in range(2):
        if not cfg.fused(k):
            names.append(f"d{k}.raw")
        names.append(f"d{k + 1}.in")
    if cfg.demean:
        names.append("d.mean")
    return names + ["y"]


def split_taps(got):
    """``forward_hip(..., taps=)``'s ``{name: (data, route)}`` -> (CPU data dict, route dict)."""
    cpu = lambda d: None if d is None else (tuple(cpu(e) for e in d) if isinstance(d, tuple) else d.cpu())
    return {k: cpu(v[0]) for k, v in got.items()}, {k: v[1] for k, v in got.items()}


# ------------------------------------------------------------------------------------------------------------------ roundings
def split16(v):
    """fp32 -> (hi, lo) f16 as split8 / split4 and the pack kernels do: hi = f16(v), lo = f16(v - hi)."""
    v = v.float()
    hi = v.half()
    return hi, (v - hi.float()).half()


def w_split(w):
    hi, lo = split16(w)
    return hi.double() + lo.double()


def w_f16(w):
    return w.float().half().double()


def hl(t):
    """A two-plane tap as float64 (lo may be None: single f16)."""
    if isinstance(t, tuple):
        return t[0].double() + (t[1].double() if t[1] is not None else 0.0)
    return t.double()


def lrelu(v):
    return torch.where(v > 0, v, v * 0.01)


def gelu64(z):
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865476))


def gelu_fast32(y):
    """gelu_exact of amx_gemm.hip in fp32 (erf_fast: Abramowitz-Stegun 7.1.26)."""
    x = y * np.float32(0.70710678118654752)
    ax = x.abs()
    t = 1.0 / (1.0 + np.float32(0.3275911) * ax)
    poly = ((((np.float32(1.061405429) * t - np.float32(1.453152027)) * t + np.float32(1.421413741)) * t - np.float32(0.284496736)) * t
            + np.float32(0.254829592)) * t
    r = 1.0 - poly * torch.exp(-ax * ax)
    return 0.5 * y * (1.0 + torch.copysign(r, x))


def conv_cl(x_cl, w, bias, stride, pad):
    """channels-last [n, D, H, W, C] conv3d with weight [Co, Ci, k, k, k] in the tensors' own dtype -> channels-last."""
    y = F.conv3d(x_cl.permute(0, 4, 1, 2, 3), w, bias, stride=stride, padding=pad)
    return y.permute(0, 2, 3, 4, 1).contiguous()


def pool_cl(x_cl):
    return F.avg_pool3d(x_cl.permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1).contiguous()


def rope_pairs(table, hd):
    """[V, 2 hd] = [sin | cos] (fp32, as handed to amx_vit_load) -> sin, cos [V, hd]."""
    return table[:, :hd], table[:, hd:]


def apply_rope(x, sin, cos):
    rot = torch.stack((-x[..., 1::2], x[..., ::2]), -1).reshape(x.shape)
    return x * cos + rot * sin


def rope_table(grid, hd):
    from oracle import vit_ref as V
    return V.rope_table(grid, hd, dtype=torch.float64).float()         # the product module's buffer: float64 angles, stored in fp32


# ------------------------------------------------------------------------------------------------------------------ statistics
def in_stats64(raw, gamma, beta, eps):
    """float64 InstanceNorm constants of a channels-last raw tensor [n, ..., C]: (scale, shift, tol_scale, tol_shift), [n, C] each.
    The engine adds fp32 slot sums of r and r^2 (32 / 64 values each) in double: relative error ``C_SS U32`` of E|r| and E[r^2]."""
    n, C = raw.shape[0], raw.shape[-1]
    r = raw.reshape(n, -1, C)
    mean, m2, ma = r.mean(1), (r * r).mean(1), r.abs().mean(1)
    var = (m2 - mean * mean).clamp_min(0.0)
    k = gamma.double() / torch.sqrt(var + eps)
    shift = beta.double() - mean * k
    e1, e2 = C_SS * U32 * ma, C_SS * U32 * m2
    dvar = e2 + 2 * mean.abs() * e1
    dk = k.abs() * dvar / (2 * (var + eps)) + 2 * U32 * k.abs()
    dshift = mean.abs() * dk + k.abs() * e1 + 2 * U32 * (beta.double().abs() + (mean * k).abs())
    return k, shift, dk, dshift


def slot_stats32(raw32, slot):
    """The engine's statistics: fp32 sums of r and r^2 over ``slot`` consecutive voxels, the slots added in double."""
    n, C = raw32.shape[0], raw32.shape[-1]
    r = raw32.reshape(n, -1, slot, C)
    return r.sum(2).double().sum(1), (r * r).sum(2).double().sum(1), r.shape[1] * slot


def finalize32(s, q, count, gamma, beta, eps):
    mean = s / count
    var = (q / count - mean * mean).clamp_min(0.0)
    k = gamma.double() / torch.sqrt(var + float(np.float32(eps)))
    return k.float(), (beta.double() - mean * k).float()


# ------------------------------------------------------------------------------------------------------------------ the walk
def _params(sd):
    """A module or its state dict -> fp32 CPU tensors."""
    sd = sd.state_dict() if hasattr(sd, "state_dict") else sd
    return {k: v.detach().cpu().float() for k, v in sd.items()}


class _Walk:
    def __init__(self, sd, kw, x, taps, only, samples, routes):
        self.sd = _params(sd)
        self.c = Cfg(self.sd, kw, x.shape)
        self.x = x.detach().cpu().float()
        self.taps, self.only, self.routes = taps, only, routes or {}
        self.samples = list(range(self.c.n)) if samples is None else list(samples)
        self.recs = []
        self.table = rope_table(self.c.grid, self.c.hd)

    def want(self, name, reads):
        if self.only is not None and name not in self.only:
            return False
        return name in self.taps and all(r in self.taps for r in reads)

    def rec(self, name, kind, got, ref, tol, pad=None):
        got, ref, tol = got.double(), ref.double(), tol.double()
        assert got.shape == ref.shape == tol.shape, (name, got.shape, ref.shape, tol.shape)
        err = (got - ref).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        ratio = torch.where(err == 0, torch.zeros_like(err), err / tol.clamp_min(1e-300))
        i = int(ratio.argmax())
        worst = tuple(int(v) for v in np.unravel_index(i, ratio.shape))
        over = int((err > tol).sum())
        pad_bad = 0 if pad is None else int((pad != 0).sum())
        self.recs.append(Rec(name, kind, self.routes.get(name, ""), float(ratio.reshape(-1)[i]), over + pad_bad, worst, float(got.reshape(-1)[i]),
                             float(ref.reshape(-1)[i]), float(ref.abs().max()), pad_bad, ok=over == 0 and pad_bad == 0))

    # ---- tap decoding
    def cl(self, name, C, div, samples=None):
        """channels-last volume tap at 1 / div of the input resolution as float64 [n, D, H, W, C] (``samples``: of these samples only)."""
        d, h, w = (v // div for v in self.c.vol)
        t = self.taps[name]
        pick = lambda p: None if p is None else (p.reshape(self.c.n, d, h, w, C) if samples is None else p.reshape(self.c.n, d, h, w, C)[samples])
        return hl(tuple(pick(p) for p in t) if isinstance(t, tuple) else pick(t))

    def rows(self, name, ld):
        t = self.taps[name]
        if isinstance(t, tuple):
            return hl(t).reshape(-1, ld), torch.cat([p.reshape(-1, ld) for p in t if p is not None])
        return t.double().reshape(-1, ld), t.reshape(-1, ld)

    def ss(self, name, C):
        sc, sh = self.taps[name]
        return sc.double().reshape(self.c.n, C), sh.double().reshape(self.c.n, C)

    # ---- stage helpers
    def norm_act(self, name, kind, raw_terms, C, div, pooled=None):
        """hi + lo stage ``lrelu(sum raw_i * scale_i + shift_i)`` and (``pooled``) its 2x2x2 average, teacher-forced."""
        c = self.c
        z, mag = 0.0, 0.0
        for raw_name, ss_name in raw_terms:
            raw = self.cl(raw_name, C, div)
            sc, sh = self.ss(ss_name, C)
            sc, sh = sc.reshape(c.n, 1, 1, 1, C), sh.reshape(c.n, 1, 1, 1, C)
            z = z + raw * sc + sh
            mag = mag + (raw * sc).abs() + sh.abs()
        self.rec(name, kind, self.cl(name, C, div), lrelu(z), HILO * mag + FLOOR)

    def pool(self, name, src, C, div):
        h = self.cl(src, C, div, self.samples)
        self.rec(name, "hilo", self.cl(name, C, 2 * div, self.samples), pool_cl(h), 2.0 ** -20 * pool_cl(h.abs()) + FLOOR)

    def conv(self, name, src, w, bias, stride, Cin, Cout, div_in):
        """split conv, fp32 channels-last result, on the samples of ``self.samples``."""
        s = self.samples
        a = self.cl(src, Cin, div_in, s)
        W = w_split(w)
        k = W.shape[-1]
        b = None if bias is None else bias.double()
        ref = conv_cl(a, W, b, stride, k // 2)
        S = conv_cl(a.abs(), W.abs(), None if b is None else b.abs(), stride, k // 2)
        got = self.cl(name, Cout, div_in * stride, s)
        self.rec(name, "split", got, ref, c_split(Cin * k ** 3) * S)

    def stats(self, name, raw_name, C, div, gamma, beta):
        raw = self.cl(raw_name, C, div)
        k, sh, dk, dsh = in_stats64(raw, gamma, beta, float(np.float32(self.c.in_eps)))      # the engine's eps is a float
        sc_got, sh_got = self.ss(name, C)
        self.rec(name, "stats", torch.stack((sc_got, sh_got)), torch.stack((k, sh)), torch.stack((dk, dsh)))

    def ln_rows(self, x, w, b, eps):
        """float64 LayerNorm rows + the fp32 arithmetic term of its bound."""
        mean = x.mean(-1, keepdim=True)
        d = x - mean
        rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
        if w is None:                                                          # plain conversion: (x - mean) + mean in fp32
            return x, 4 * U32 * (x.abs() + mean.abs()), rstd, d
        y = d * rstd * w.double() + b.double()
        arith = 2.0 ** -20 * ((x.abs() + mean.abs()) * rstd * w.double().abs() + b.double().abs())
        return y, arith, rstd, d

    def f16_rows(self, name, x, w, b, eps, C, ld):
        got, stored = self.rows(name, ld)
        y, arith, _, _ = self.ln_rows(x, w, b, eps)
        self.rec(name, "f16", got[:, :C], y, ULP16 * y.abs() + arith + 2.0 ** -24, pad=stored[:, C:])

    def product(self, a, W, bias):
        """float64 product of operand rows [M, K] with W [N, K] (+ bias) and its S."""
        ref = a @ W.t()
        S = a.abs() @ W.abs().t()
        if bias is not None:
            ref, S = ref + bias.double(), S + bias.double().abs()
        return ref, S

    # ---- the stages in launch order
    def run(self):
        c, sd, P = self.c, self.sd, "down_projection."
        # ---------------------------------------------------------------- tokenizer
        if self.want("h0", []):
            s = self.samples
            xs = self.x[s].permute(0, 2, 3, 4, 1)                               # [n, D, H, W, 1]
            xh, xl = split16(xs)                                               # the stem splits the fp32 input on the fly
            a = xh.double() + xl.double()
            W, b = w_split(sd[P + "stem.conv.weight"]), sd[P + "stem.conv.bias"].double()
            r = conv_cl(a, W, b, 1, 1)
            S = conv_cl(a.abs(), W.abs(), b.abs(), 1, 1)
            k, sh, dk, dsh = in_stats64(r, sd[P + "stem.norm.weight"], sd[P + "stem.norm.bias"], c.in_eps)
            v = lambda t: t.reshape(len(s), 1, 1, 1, 32)
            # the stem's statistics are not tapped (its raw output never exists): they are this reference's own, with their tolerance
            dr = c_split(32) * S + 2.0 ** -24                                 # (+ the input's lo plane is subnormal below 2^-14: 2^-25 per tap)
            tol = v(k).abs() * dr + r.abs() * v(dk) + v(dsh) + HILO * ((r * v(k)).abs() + v(sh).abs()) + FLOOR
            self.rec("h0", "hilo", self.cl("h0", 32, 1, s), lrelu(r * v(k) + v(sh)), tol)
        if self.want("p0", ["h0"]):
            self.pool("p0", "h0", 32, 1)
        src, psrc, div = "h0", "p0", 1
        for k in range(3):
            p, sk = f"{P}stages.{k}.", f"s{k}"
            Cin, C = STAGE_C[k], STAGE_C[k + 1]
            if self.want(sk + ".raw1", [src]):
                self.conv(sk + ".raw1", src, sd[p + "conv1.weight"], sd[p + "conv1.bias"], 2, Cin, C, div)
            if self.want(sk + ".ss1", [sk + ".raw1"]):
                self.stats(sk + ".ss1", sk + ".raw1", C, 2 * div, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
            if self.want(sk + ".a1", [sk + ".raw1", sk + ".ss1"]):
                self.norm_act(sk + ".a1", "hilo", [(sk + ".raw1", sk + ".ss1")], C, 2 * div)
            if self.want(sk + ".raw2", [sk + ".a1"]):
                self.conv(sk + ".raw2", sk + ".a1", sd[p + "conv2.weight"], sd[p + "conv2.bias"], 1, C, C, 2 * div)
            if self.want(sk + ".ss2", [sk + ".raw2"]):
                self.stats(sk + ".ss2", sk + ".raw2", C, 2 * div, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
            if self.want(sk + ".raws", [psrc]):
                self.conv(sk + ".raws", psrc, sd[p + "skip.weight"], None, 1, Cin, C, 2 * div)
            if self.want(sk + ".sss", [sk + ".raws"]):
                self.stats(sk + ".sss", sk + ".raws", C, 2 * div, sd[p + "skip_norm.weight"], sd[p + "skip_norm.bias"])
            if self.want(sk + ".h", [sk + ".raw2", sk + ".ss2", sk + ".raws", sk + ".sss"]):
                self.norm_act(sk + ".h", "hilo", [(sk + ".raw2", sk + ".ss2"), (sk + ".raws", sk + ".sss")], C, 2 * div)
            if k < 2 and self.want(sk + ".p", [sk + ".h"]):
                self.pool(sk + ".p", sk + ".h", C, 2 * div)
            src, psrc, div = sk + ".h", sk + ".p", 2 * div
        if self.want("tokens", ["s2.h"]):
            a = self.cl("s2.h", 128, 8).reshape(c.n * c.V, 128)
            ref, S = self.product(a, w_split(sd[P + "proj.weight"].reshape(c.E, 128)), sd[P + "proj.bias"])
            pos = sd["eva.pos_embed"].double().reshape(c.V, c.E)
            ref = ref.reshape(c.n, c.V, c.E) + pos
            tol = c_split(128) * (S.reshape(c.n, c.V, c.E) + pos.abs())
            if c.nreg:                                                         # the register rows are copies: exact
                regs = sd["register_tokens"].double().reshape(1, c.nreg, c.E).expand(c.n, -1, -1)
                ref, tol = torch.cat((regs, ref), 1), torch.cat((torch.zeros_like(regs), tol), 1)
            self.rec("tokens", "split", self.taps["tokens"].double().reshape(c.n, c.T, c.E), ref, tol)
        # ---------------------------------------------------------------- blocks
        stream = "tokens"
        nb = sum(1 for b in range(c.depth) if f"b{b}.tok2" in self.taps or f"b{b}.ln1" in self.taps)
        for bi in range(nb):
            p, bk = f"eva.blocks.{bi}.", f"b{bi}"
            tok = lambda nm: self.taps[nm].double().reshape(c.M, c.E)
            if self.want(bk + ".ln1", [stream]):
                self.f16_rows(bk + ".ln1", tok(stream), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6, c.E, c.Ep)
            if self.want(bk + ".attn", [bk + ".ln1"]):
                self.attn(bk, p)
            if self.want(bk + ".ln_attn", [bk + ".attn"]):
                w, b = (sd[p + "attn.norm.weight"], sd[p + "attn.norm.bias"]) if c.inner else (None, None)
                self.f16_rows(bk + ".ln_attn", tok(bk + ".attn"), w, b, 1e-5, c.E, c.Ep)
            if self.want(bk + ".tok1", [bk + ".ln_attn", stream]):
                self.resid(bk + ".tok1", stream, bk + ".ln_attn", c.Ep, c.E, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"],
                           sd[p + "gamma_1"] if c.layer_scale else None)
            if self.want(bk + ".ln2", [bk + ".tok1"]):
                self.f16_rows(bk + ".ln2", tok(bk + ".tok1"), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6, c.E, c.Ep)
            h16, h32 = up(c.hid, 16), up(c.hid, 32)
            if self.want(bk + ".hd", [bk + ".ln2"]):
                a = self.rows(bk + ".ln2", c.Ep)[0][:, :c.E]
                g, Sg = self.product(a, w_f16(sd[p + "mlp.fc1_g.weight"]), sd[p + "mlp.fc1_g.bias"])
                v, Sv = self.product(a, w_f16(sd[p + "mlp.fc1_x.weight"]), sd[p + "mlp.fc1_x.bias"])
                silu = g * torch.sigmoid(g)
                ref = silu * v
                # d silu / dg is within [-0.1, 1.1]; __expf's few fp32 ulps sit inside the second half of ULP16
                tol = ULP16 * ref.abs() + c_f16(c.E) * (1.1 * v.abs() * Sg + silu.abs() * Sv) + 2.0 ** -24
                got, stored = self.rows(bk + ".hd", h16)
                self.rec(bk + ".hd", "f16", got[:, :c.hid], ref, tol, pad=stored[:, c.hid:])
            if self.want(bk + ".ln_mlp", [bk + ".hd"]):
                x = self.rows(bk + ".hd", h16)[0][:, :c.hid]
                self.f16_rows(bk + ".ln_mlp", x, sd[p + "mlp.norm.weight"], sd[p + "mlp.norm.bias"], 1e-6, c.hid, h32)
            if self.want(bk + ".tok2", [bk + ".ln_mlp", bk + ".tok1"]):
                self.resid(bk + ".tok2", bk + ".tok1", bk + ".ln_mlp", h32, c.hid, sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"],
                           sd[p + "gamma_2"] if c.layer_scale else None)
            stream = bk + ".tok2"
        # ---------------------------------------------------------------- final norm + decoder
        if self.want("d.ln", [stream]):
            x = self.taps[stream].double().reshape(c.n, c.T, c.E)[:, c.nreg:].reshape(c.n * c.V, c.E)
            y, arith, _, _ = self.ln_rows(x, sd["eva.norm.weight"], sd["eva.norm.bias"], 1e-6)
            got, stored = self.rows("d.ln", c.Ep)
            self.rec("d.ln", "hilo", got[:, :c.E], y, arith + HILO * y.abs() + FLOOR, pad=stored[:, c.E:])
        g = c.grid
        src = "d.ln"
        for k in range(2):
            p = f"up_projection.decode.{k}."
            Cin, Co = c.dec[k], c.dec[k + 1]
            ldi, ldo = up(Cin, 32), up(Co, 32)
            raw, nxt = f"d{k}.raw", f"d{k + 1}.in"
            lnw, lnb = sd[p + "1.weight"], sd[p + "1.bias"]
            if c.fused(k):
                if self.want(nxt, [src]):
                    r, S = self.tconv(src, ldi, Cin, sd[p + "0.weight"], sd[p + "0.bias"], g)
                    self.gelu_rows(nxt, r, c_split(Cin) * S, lnw, lnb, Co, ldo)
            else:
                if self.want(raw, [src]):
                    r, S = self.tconv(src, ldi, Cin, sd[p + "0.weight"], sd[p + "0.bias"], g)
                    self.rec(raw, "split", self.taps[raw].double().reshape(-1, Co), r, c_split(Cin) * S)
                if self.want(nxt, [raw]):
                    self.gelu_rows(nxt, self.taps[raw].double().reshape(-1, Co), None, lnw, lnb, Co, ldo)
            src, g = nxt, tuple(2 * v for v in g)
        if self.want("y", ["d2.in"] + (["d.mean"] if c.demean else [])) or self.want("d.mean", ["d2.in"]):
            Cin, Co = c.dec[2], c.dec[3]
            w, b = sd["up_projection.decode.2.weight"], sd["up_projection.decode.2.bias"]
            r, S = self.tconv("d2.in", up(Cin, 32), Cin, w, b, g)               # rows of the full-resolution grid, [n vox, Co]
            vox = r.shape[0] // c.n
            r, S = r.reshape(c.n, vox, Co), S.reshape(c.n, vox, Co)
            if c.demean and self.want("d.mean", ["d2.in"]):
                # the engine: fp32 column sums of d2.in in chunks, double from there on, the weight summed over its 8 parities in fp32
                a = self.rows("d2.in", up(Cin, 32))[0][:, :Cin].reshape(c.n, -1, Cin)
                wsum = w.double().abs().sum((2, 3, 4)) / 8                   # [Cin, Co]
                # (+ U16^2: the engine multiplies by the fp32 weight itself, this reference by its hi + lo planes)
                tol = (C_MEAN * U32 + U16 * U16) * (a.abs().mean(1) @ wsum + b.double().abs()) + 2.0 ** -24
                self.rec("d.mean", "stats", self.taps["d.mean"].double().reshape(c.n, Co), r.mean(1), tol)
            if self.want("y", ["d2.in"] + (["d.mean"] if c.demean else [])):
                sub = self.taps["d.mean"].double().reshape(c.n, 1, Co) if c.demean else torch.zeros(c.n, 1, Co, dtype=F64)
                D, H, Wd = c.vol
                cl2planar = lambda t: t.reshape(c.n, D, H, Wd, Co).permute(0, 4, 1, 2, 3)
                self.rec("y", "split", self.taps["y"].double().reshape(c.n, Co, D, H, Wd), cl2planar(r - sub),
                         cl2planar(c_split(Cin) * (S + sub.abs()) + 2 * U32 * (r - sub).abs()))
        return self.recs

    def resid(self, name, cur_name, a_name, ld, K, w, bias, gamma):
        c = self.c
        a = self.rows(a_name, ld)[0][:, :K]
        cur = self.taps[cur_name].double().reshape(c.M, c.E)
        lin, S = self.product(a, w_f16(w), bias)
        g = gamma.double() if gamma is not None else torch.ones(c.E, dtype=F64)
        self.rec(name, "resid", self.taps[name].double().reshape(c.M, c.E), cur + g * lin, c_f16(K) * (cur.abs() + g.abs() * S))

    def tconv(self, src, ld, Cin, w, bias, grid):
        """ConvTranspose3d(k = 2, s = 2) of operand rows [n gd gh gw, ld] as a product: rows of the doubled grid in raster order,
        [rows * 8, Co], and S."""
        c = self.c
        a = self.rows(src, ld)[0][:, :Cin]
        Co = w.shape[1]
        W = w_split(w).reshape(Cin, Co * 8)                                   # column = co * 8 + (dz, dy, dx)
        r, S = a @ W, a.abs() @ W.abs()
        gd, gh, gw = grid
        def scatter(t, b):
            t = t.reshape(c.n, gd, gh, gw, Co, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4)   # n, z, dz, y, dy, x, dx, co
            return t.reshape(-1, Co) + b
        return scatter(r, bias.double()), scatter(S, bias.double().abs())

    def gelu_rows(self, name, raw, draw, lnw, lnb, C, ld):
        """hi + lo rows ``gelu(LayerNorm(raw))``; ``draw``: per-element uncertainty of ``raw`` when it is this reference's own product
        (fused stage), propagated through the norm: ``rstd |w| (d_i + mean(d) + |x_i - mean| rstd rms(d))``."""
        z, arith, rstd, d = self.ln_rows(raw, lnw, lnb, 1e-6)
        dz = arith
        if draw is not None:
            dz = dz + rstd * lnw.double().abs() * (draw + draw.mean(-1, keepdim=True) + d.abs() * rstd * torch.sqrt((draw * draw).mean(-1, keepdim=True)))
        y = gelu64(z)
        got, stored = self.rows(name, ld)
        self.rec(name, "hilo", got[:, :C], y, 1.13 * dz + ERF_FAST * z.abs() / 2 + HILO * y.abs() + FLOOR, pad=stored[:, C:])

    def qkv64(self, bk, p, arith, rope_prefix=False):
        """q (scaled), k, v of a block from the ``ln1`` tap: [n, heads, T, hd] each, rounded to f16 (``arith``: torch dtype of the
        arithmetic in front of the rounding: float64 for the reference, float32 for the emulation)."""
        c, sd = self.c, self.sd
        a = self.rows(bk + ".ln1", c.Ep)[0][:, :c.E].to(arith)
        sh = lambda t: t.reshape(c.n, c.T, c.heads, c.hd).transpose(1, 2)
        lin = lambda w, b: a @ w_f16(sd[p + w]).to(arith).t() + (sd[p + b].to(arith) if b else 0)
        q, k, v = sh(lin("attn.q_proj.weight", "attn.q_proj.bias")), sh(lin("attn.k_proj.weight", None)), sh(lin("attn.v_proj.weight", "attn.v_proj.bias"))
        if c.qk_norm:
            q = F.layer_norm(q, (c.hd,), sd[p + "attn.q_norm.weight"].to(arith), sd[p + "attn.q_norm.bias"].to(arith), 1e-5)
            k = F.layer_norm(k, (c.hd,), sd[p + "attn.k_norm.weight"].to(arith), sd[p + "attn.k_norm.bias"].to(arith), 1e-5)
        sin, cos = rope_pairs(self.table.to(arith), c.hd)
        # (rope_prefix: a planted defect of tests/test_vit_walk.py -- the register rows rotated as well, with table rows 1 .. nreg)
        pre = (lambda t: apply_rope(t, sin[1:c.nreg + 1], cos[1:c.nreg + 1])) if rope_prefix else (lambda t: t)
        rp = lambda t: torch.cat((pre(t[:, :, :c.nreg]), apply_rope(t[:, :, c.nreg:], sin, cos)), 2)
        q, k = rp(q), rp(k)
        qs = float(np.float32(1.4426950408889634) / np.sqrt(np.float32(c.hd)))
        return (q * qs).half(), k.half(), v.half()

    def attn(self, bk, p):
        c = self.c
        q, k, v = (t.double() for t in self.qkv64(bk, p, F64))
        s = q @ k.transpose(-1, -2)                                            # log2 domain
        P = torch.softmax(s * math.log(2.0), -1)
        ref = (P @ v).transpose(1, 2).reshape(c.M, c.E)
        tol = (C_ATT * (P @ v.abs()) + C_ATT_SUM * (P @ v).abs()).transpose(1, 2).reshape(c.M, c.E) + 2.0 ** -24
        self.rec(bk + ".attn", "attn", self.taps[bk + ".attn"].double().reshape(c.M, c.E), ref, tol)


def walk(sd, kw, x, taps, only=None, samples=None, routes=None):
    """``sd``: a PrimusV2 module or its state dict; ``kw``: its constructor keywords.  One Rec per stage whose result and inputs are in ``taps`` (``split_taps`` of ``forward_hip(x, taps=...)``, or ``emulate``).
    ``only``: restrict to these stage names.  ``samples``: the float64 convolutions of the tokenizer run on these samples only (their
    inputs are stored taps: a subset needs nothing from the others); the statistics stages always cover every sample."""
    return _Walk(sd, kw, x, taps, only, samples, routes).run()


def readers(name, cfg):
    """Names of the stages that read tap ``name`` (the stages a defect planted in ``name`` may also fail)."""
    out = []
    probe = {n: None for n in tap_names(cfg)}

    class _Probe(_Walk):
        def __init__(self):
            self.c, self.taps, self.only = cfg, probe, None
            self.hits = []

        def want(self, stage, reads):
            if name in reads:
                out.append(stage)
            return False
    import collections
    pr = _Probe()
    pr.sd, pr.samples, pr.recs = collections.defaultdict(lambda: None), [], []
    pr.run()
    return out


# ------------------------------------------------------------------------------------------------------------------ the emulation
def _prod32(a_hi, a_lo, w, bias):
    """The split product in fp32: wh xh + wh xl + wl xh (the lo x lo term is dropped), fp32 accumulation."""
    wh, wl = split16(w)
    y = a_hi.float() @ wh.float().t() + a_lo.float() @ wh.float().t() + a_hi.float() @ wl.float().t()
    return y if bias is None else y + bias.float()


def _conv32(x_hi, x_lo, w, bias, stride):
    wh, wl = (t.float() for t in split16(w))
    k = w.shape[-1]
    y = conv_cl(x_hi.float(), wh, None, stride, k // 2) + conv_cl(x_lo.float(), wh, None, stride, k // 2) + conv_cl(x_hi.float(), wl, None, stride, k // 2)
    return y if bias is None else y + bias.float()


def _ln32(x, w, b, eps, gelu=False):
    x = x.float()
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + np.float32(eps))
    y = d * rstd * w.float() + b.float() if w is not None else d + mean
    return gelu_fast32(y) if gelu else y


def _padded(t, ld):
    return F.pad(t, (0, ld - t.shape[-1]))


def _attn32(q, k, v, T):
    """attn_fwd_kernel on f16 operands [n, heads, T, hd]: key blocks of 64, the lazy reference point (it moves in block 0 and when a
    shifted score exceeds kLag = 8), probabilities rounded to f16, row sum through the same f16 probabilities, fp32 accumulators."""
    q, k, v = q.float(), k.float(), v.float()
    m_ref = torch.zeros(q.shape[:-1] + (1,))
    acc = torch.zeros_like(q)
    l = torch.zeros_like(m_ref)
    for blk, k0 in enumerate(range(0, T, 64)):
        s = q @ k[:, :, k0:k0 + 64].transpose(-1, -2) - m_ref
        mq = s.max(-1, keepdim=True).values
        delta = mq if blk == 0 else torch.where(mq > 8.0, mq, torch.zeros_like(mq))
        alpha = torch.exp2(-delta)
        m_ref, s, acc, l = m_ref + delta, s - delta, acc * alpha, l * alpha
        pr = torch.exp2(s).half().float()
        acc = acc + pr @ v[:, :, k0:k0 + 64]
        l = l + pr.sum(-1, keepdim=True)
    return acc * (1.0 / l)


def emulate(sd, kw, x, n_blocks=-1):
    """The full tap dictionary of a forward on the CPU with the engine's arithmetic, in the layout ``forward_hip(x, taps=...)`` returns
    (flat tensors; pairs for the two-range taps)."""
    sd = _params(sd)
    c = Cfg(sd, kw, x.shape)
    P = "down_projection."
    t = {}
    flat = lambda pair: tuple(p.reshape(-1) for p in pair)
    eps = c.in_eps

    def norm32(raw, slot, gamma, beta):
        s, q, count = slot_stats32(raw, slot)
        return finalize32(s, q, count, gamma, beta, eps)

    bc = lambda v, C: v.reshape(c.n, 1, 1, 1, C)
    # stem: a wave owns 2 x 2 rows of the volume: its slot is 4 W voxels (not consecutive in raster order; any order serves the emulation)
    xs = x.detach().cpu().float().permute(0, 2, 3, 4, 1)
    xh, xl = split16(xs)
    r = _conv32(xh, xl, sd[P + "stem.conv.weight"], sd[P + "stem.conv.bias"], 1)
    sc, sh = norm32(r, 4 * c.vol[2], sd[P + "stem.norm.weight"], sd[P + "stem.norm.bias"])
    h = lrelu(r * bc(sc, 32) + bc(sh, 32))
    pool = pool_cl(h)
    t["h0"], t["p0"] = flat(split16(h)), flat(split16(pool))
    hcur, pcur = split16(h), split16(pool)
    vox = int(np.prod(c.vol))
    for k in range(3):
        p, sk = f"{P}stages.{k}.", f"s{k}"
        C = STAGE_C[k + 1]
        vox //= 8
        slot = 64 if c.n * vox // 64 >= 2048 else 32                          # tokconv_mt
        raw1 = _conv32(hcur[0], hcur[1], sd[p + "conv1.weight"], sd[p + "conv1.bias"], 2)
        sc1, sh1 = norm32(raw1, slot, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
        a1 = split16(lrelu(raw1 * bc(sc1, C) + bc(sh1, C)))
        raw2 = _conv32(a1[0], a1[1], sd[p + "conv2.weight"], sd[p + "conv2.bias"], 1)
        sc2, sh2 = norm32(raw2, slot, sd[p + "norm2.weight"], sd[p + "norm2.bias"])
        raws = _conv32(pcur[0], pcur[1], sd[p + "skip.weight"], None, 1)
        scs, shs = norm32(raws, slot, sd[p + "skip_norm.weight"], sd[p + "skip_norm.bias"])
        h = lrelu((raw2 * bc(sc2, C) + bc(sh2, C)) + (raws * bc(scs, C) + bc(shs, C)))
        hcur = split16(h)
        t[sk + ".raw1"], t[sk + ".ss1"], t[sk + ".a1"] = raw1.reshape(-1), (sc1.reshape(-1), sh1.reshape(-1)), flat(a1)
        t[sk + ".raw2"], t[sk + ".ss2"] = raw2.reshape(-1), (sc2.reshape(-1), sh2.reshape(-1))
        t[sk + ".raws"], t[sk + ".sss"], t[sk + ".h"] = raws.reshape(-1), (scs.reshape(-1), shs.reshape(-1)), flat(hcur)
        if k < 2:
            pcur = split16(pool_cl(h))
            t[sk + ".p"] = flat(pcur)
    a_hi, a_lo = (v.reshape(c.n * c.V, 128) for v in hcur)
    tok = _prod32(a_hi, a_lo, sd[P + "proj.weight"].reshape(c.E, 128), sd[P + "proj.bias"]).reshape(c.n, c.V, c.E) + sd["eva.pos_embed"].reshape(c.V, c.E)
    if c.nreg:
        tok = torch.cat((sd["register_tokens"].reshape(1, c.nreg, c.E).expand(c.n, -1, -1), tok), 1)
    tok = tok.reshape(c.M, c.E).contiguous()
    t["tokens"] = tok.reshape(-1).clone()
    nb = c.depth if n_blocks < 0 or n_blocks > c.depth else n_blocks
    h16, h32 = up(c.hid, 16), up(c.hid, 32)
    helper = _Walk(sd, kw, x, t, None, None, None)
    for bi in range(nb):
        p, bk = f"eva.blocks.{bi}.", f"b{bi}"
        ln1 = _ln32(tok, sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6).half()
        t[bk + ".ln1"] = _padded(ln1, c.Ep).reshape(-1)
        q, k_, v = helper.qkv64(bk, p, torch.float32)
        att = _attn32(q, k_, v, c.T).transpose(1, 2).reshape(c.M, c.E).contiguous()
        t[bk + ".attn"] = att.reshape(-1)
        la = _ln32(att, sd[p + "attn.norm.weight"] if c.inner else None, sd.get(p + "attn.norm.bias"), 1e-5).half()
        t[bk + ".ln_attn"] = _padded(la, c.Ep).reshape(-1)
        g1 = sd[p + "gamma_1"] if c.layer_scale else torch.ones(c.E)
        tok = tok + g1 * (la.float() @ sd[p + "attn.proj.weight"].half().float().t() + sd[p + "attn.proj.bias"])
        t[bk + ".tok1"] = tok.reshape(-1).clone()
        ln2 = _ln32(tok, sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6).half()
        t[bk + ".ln2"] = _padded(ln2, c.Ep).reshape(-1)
        g = ln2.float() @ sd[p + "mlp.fc1_g.weight"].half().float().t() + sd[p + "mlp.fc1_g.bias"]
        xv = ln2.float() @ sd[p + "mlp.fc1_x.weight"].half().float().t() + sd[p + "mlp.fc1_x.bias"]
        hdn = (g / (1.0 + torch.exp(-g)) * xv).half()
        t[bk + ".hd"] = _padded(hdn, h16).reshape(-1)
        lm = _ln32(hdn, sd[p + "mlp.norm.weight"], sd[p + "mlp.norm.bias"], 1e-6).half()
        t[bk + ".ln_mlp"] = _padded(lm, h32).reshape(-1)
        g2 = sd[p + "gamma_2"] if c.layer_scale else torch.ones(c.E)
        tok = tok + g2 * (lm.float() @ sd[p + "mlp.fc2.weight"].half().float().t() + sd[p + "mlp.fc2.bias"])
        t[bk + ".tok2"] = tok.reshape(-1).clone()
    xv = tok.reshape(c.n, c.T, c.E)[:, c.nreg:].reshape(c.n * c.V, c.E)
    rows = split16(_ln32(xv, sd["eva.norm.weight"], sd["eva.norm.bias"], 1e-6))
    t["d.ln"] = tuple(_padded(r_, c.Ep).reshape(-1) for r_ in rows)
    g = c.grid
    for k in range(3):
        p = f"up_projection.decode.{k}." + ("0." if k < 2 else "")
        w, b = sd[p + "weight"], sd[p + "bias"]
        Cin, Co = c.dec[k], c.dec[k + 1]
        raw = _prod32(rows[0], rows[1], w.reshape(Cin, Co * 8).t(), None)
        raw = raw.reshape(c.n, *g, Co, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(-1, Co) + b
        g = tuple(2 * v for v in g)
        if k < 2:
            if not c.fused(k):
                t[f"d{k}.raw"] = raw.reshape(-1)
            lp = f"up_projection.decode.{k}.1."
            rows = split16(_ln32(raw, sd[lp + "weight"], sd[lp + "bias"], 1e-6, gelu=True))
            t[f"d{k + 1}.in"] = tuple(_padded(r_, up(Co, 32)).reshape(-1) for r_ in rows)
        else:
            y = raw.reshape(c.n, -1, Co)
            if c.demean:      # column sums of hi and lo in 128 fp32 chunks per sample, double from there on
                a = (rows[0].float().reshape(c.n, 128, -1, Cin).sum(2) + rows[1].float().reshape(c.n, 128, -1, Cin).sum(2)).double().sum(1)
                xbar = a / (rows[0].shape[0] // c.n)
                mean = (xbar @ (w.sum((2, 3, 4)).double() * 0.125) + b.double()).float()
                t["d.mean"] = mean.reshape(-1)
                y = (raw.reshape(c.n, -1, Co) - b) + (b - mean).reshape(c.n, 1, Co)
            t["y"] = y.reshape(c.n, *c.vol, Co).permute(0, 4, 1, 2, 3).contiguous().reshape(-1)
    return t


# ------------------------------------------------------------------------------------------------------------------ composition
def chain64(sd, kw, x):
    """The stage references chained WITHOUT teacher forcing and without any storage rounding, in float64: must reproduce
    ``oracle.vit_ref.forward(..., dtype=float64)`` (tests/test_vit_walk.py) -- it pins the references above to the suite's oracle.
    Implemented as the walk's own arithmetic on exact taps: every stage's reference becomes the next stage's input."""
    sd64 = {k: v.double() for k, v in _params(sd).items()}
    c = Cfg(sd64, kw, x.shape)
    w = _Walk(sd, kw, x, {}, None, None, None)
    P = "down_projection."
    eps = c.in_eps

    def inorm(r, gamma, beta):
        k, sh, _, _ = in_stats64(r, gamma, beta, eps)
        C = r.shape[-1]
        return r * k.reshape(c.n, 1, 1, 1, C) + sh.reshape(c.n, 1, 1, 1, C)

    h = lrelu(inorm(conv_cl(x.detach().cpu().double().permute(0, 2, 3, 4, 1), sd64[P + "stem.conv.weight"], sd64[P + "stem.conv.bias"], 1, 1),
                    sd64[P + "stem.norm.weight"], sd64[P + "stem.norm.bias"]))
    for k in range(3):
        p = f"{P}stages.{k}."
        a1 = lrelu(inorm(conv_cl(h, sd64[p + "conv1.weight"], sd64[p + "conv1.bias"], 2, 1), sd64[p + "norm1.weight"], sd64[p + "norm1.bias"]))
        y2 = inorm(conv_cl(a1, sd64[p + "conv2.weight"], sd64[p + "conv2.bias"], 1, 1), sd64[p + "norm2.weight"], sd64[p + "norm2.bias"])
        ys = inorm(conv_cl(pool_cl(h), sd64[p + "skip.weight"], None, 1, 0), sd64[p + "skip_norm.weight"], sd64[p + "skip_norm.bias"])
        h = lrelu(y2 + ys)
    tok = h.reshape(c.n, c.V, 128) @ sd64[P + "proj.weight"].reshape(c.E, 128).t() + sd64[P + "proj.bias"] + sd64["eva.pos_embed"].reshape(c.V, c.E)
    if c.nreg:
        tok = torch.cat((sd64["register_tokens"].reshape(1, c.nreg, c.E).expand(c.n, -1, -1), tok), 1)
    tok = tok.reshape(c.M, c.E)
    from oracle import vit_ref as V
    sin, cos = rope_pairs(V.rope_table(c.grid, c.hd, dtype=F64), c.hd)
    for bi in range(c.depth):
        p = f"eva.blocks.{bi}."
        a = w.ln_rows(tok, sd64[p + "norm1.weight"], sd64[p + "norm1.bias"], 1e-6)[0]
        shp = lambda t_: t_.reshape(c.n, c.T, c.heads, c.hd).transpose(1, 2)
        q = shp(a @ sd64[p + "attn.q_proj.weight"].t() + sd64[p + "attn.q_proj.bias"])
        k_ = shp(a @ sd64[p + "attn.k_proj.weight"].t())
        v = shp(a @ sd64[p + "attn.v_proj.weight"].t() + sd64[p + "attn.v_proj.bias"])
        if c.qk_norm:
            q = F.layer_norm(q, (c.hd,), sd64[p + "attn.q_norm.weight"], sd64[p + "attn.q_norm.bias"], 1e-5)
            k_ = F.layer_norm(k_, (c.hd,), sd64[p + "attn.k_norm.weight"], sd64[p + "attn.k_norm.bias"], 1e-5)
        rp = lambda t_: torch.cat((t_[:, :, :c.nreg], apply_rope(t_[:, :, c.nreg:], sin, cos)), 2)
        s = (rp(q) * (math.log2(math.e) / math.sqrt(c.hd))) @ rp(k_).transpose(-1, -2)
        att = (torch.softmax(s * math.log(2.0), -1) @ v).transpose(1, 2).reshape(c.M, c.E)
        if c.inner:
            att = w.ln_rows(att, sd64[p + "attn.norm.weight"], sd64[p + "attn.norm.bias"], 1e-5)[0]
        lin = att @ sd64[p + "attn.proj.weight"].t() + sd64[p + "attn.proj.bias"]
        tok = tok + (sd64[p + "gamma_1"] * lin if c.layer_scale else lin)
        a = w.ln_rows(tok, sd64[p + "norm2.weight"], sd64[p + "norm2.bias"], 1e-6)[0]
        g = a @ sd64[p + "mlp.fc1_g.weight"].t() + sd64[p + "mlp.fc1_g.bias"]
        hdn = g * torch.sigmoid(g) * (a @ sd64[p + "mlp.fc1_x.weight"].t() + sd64[p + "mlp.fc1_x.bias"])
        lm = w.ln_rows(hdn, sd64[p + "mlp.norm.weight"], sd64[p + "mlp.norm.bias"], 1e-6)[0]
        lin = lm @ sd64[p + "mlp.fc2.weight"].t() + sd64[p + "mlp.fc2.bias"]
        tok = tok + (sd64[p + "gamma_2"] * lin if c.layer_scale else lin)
    rows = w.ln_rows(tok.reshape(c.n, c.T, c.E)[:, c.nreg:].reshape(c.n * c.V, c.E), sd64["eva.norm.weight"], sd64["eva.norm.bias"], 1e-6)[0]
    g = c.grid
    for k in range(3):
        p = f"up_projection.decode.{k}." + ("0." if k < 2 else "")
        Co = c.dec[k + 1]
        raw = rows @ sd64[p + "weight"].reshape(c.dec[k], Co * 8)
        raw = raw.reshape(c.n, *g, Co, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(-1, Co) + sd64[p + "bias"]
        g = tuple(2 * v for v in g)
        if k < 2:
            lp = f"up_projection.decode.{k}.1."
            rows = gelu64(w.ln_rows(raw, sd64[lp + "weight"], sd64[lp + "bias"], 1e-6)[0])
    y = raw.reshape(c.n, -1, c.dec[3])
    if c.demean:
        y = y - y.mean(1, keepdim=True)
    return y.reshape(c.n, *c.vol, c.dec[3]).permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------------------------------------------------------ the cases
_FLAGSHIP = dict(input_channels=1, num_classes=32, embed_dim=396, eva_numheads=6, patch_embed_size=(8, 8, 8), num_register_tokens=8,
                 init_values=0.1, scale_attn_inner=True, qk_norm=True, out_norm="demean", out_norm_eps=1e-2, register_init_std=0.02, in_eps=1e-2)
CASES = {
    # flagship widths: T = 72 (one full key block and one of 8 keys), M = 144
    "A": dict(kw=dict(_FLAGSHIP, input_shape=(32, 32, 32), eva_depth=2), batch=2, n_blocks=-1, samples=None),
    # ragged shapes, every flag off: T = 67 (T % 4 != 0), M = 201 (partial row tile, tiles across two samples), Ep = 256 > E = 240,
    # hidden = int(240 * 2.53) = 607 (a multiple of neither 16 nor 4), 36 classes (cp = 48), decoder 160 / 104
    "B": dict(kw=dict(input_channels=1, num_classes=36, embed_dim=240, eva_numheads=4, patch_embed_size=(8, 8, 8), num_register_tokens=3,
                      init_values=None, scale_attn_inner=False, qk_norm=False, out_norm="none", register_init_std=0.02, in_eps=1e-2,
                      input_shape=(16, 64, 32), eva_depth=1, mlp_ratio=2.53), batch=3, n_blocks=-1, samples=None),
    # PrimusV2-L widths on the minimum grid width
    "C": dict(kw=dict(_FLAGSHIP, embed_dim=1056, eva_numheads=16, input_shape=(64, 32, 16), eva_depth=1), batch=1, n_blocks=-1, samples=None),
    # tokenizer only: 32 x 32^3 and 32 x 16^3 = 131072 output voxels select tokconv<..,4,2,..> and <..,4,4,..>
    "D": dict(kw=dict(_FLAGSHIP, input_shape=(64, 64, 64), eva_depth=1), batch=32, n_blocks=0, samples=[0, 17, 31]),
}
D_STAGES = ["h0", "p0"] + [f"s{k}.{s}" for k in range(2) for s in ("raw1", "ss1", "a1", "raw2", "ss2", "raws", "sss", "h", "p")]


def case(name, seed=None):
    """(kw, state dict, input, entry of CASES).  Parameters: ``oracle.vit_ref.synthetic_state_dict`` where it applies (A, C, D); case B's
    hidden width and absent flags are outside it: a seeded module with its 1-D parameters moved off their defaults."""
    from oracle import vit_ref as V
    cs = CASES[name]
    kw = cs["kw"]
    seed = {"A": 21, "B": 22, "C": 23, "D": 24}[name] if seed is None else seed
    if name == "B":
        from anatomix_amd.model.vit3d import PrimusV2
        gen = torch.Generator().manual_seed(seed)
        torch.manual_seed(seed)
        m = PrimusV2(**kw)
        with torch.no_grad():
            for prm in m.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn(prm.shape, generator=gen))
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    else:
        sd = V.synthetic_state_dict(kw, seed)
    x = V.synthetic_input(100 + seed, cs["batch"], kw["input_shape"])
    return kw, sd, x, cs
