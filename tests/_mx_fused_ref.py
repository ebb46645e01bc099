"""float64 restatements of the fused launches of the f16x2mx schedule, the comparisons the GPU tests make with them, and a host
emulation of each launch with planted defects (tests/test_mx_fused.py proves on the host that every comparison names its launch).

The launches (amx_conv3d_zx.hip, amx_norm.hip), each reached alone through a probe entry of include/anatomix_amd.h:

  zx         conv3d_k3_zx<...>: 32 -> 32 reflect conv whose converter waves read the stored pair x = hi + lo, form v = act(a x + b)
             in fp32 and split v into the f16 operand and two e4m3 copies (mx_split8_direct: the lo copy is e4m3 of the fp32 residual
             2^11 (v - hi), not of an f16 lo); the epilogue stores the raw pair (or fp32 planar) and the InstanceNorm partial sums
  finalize   launch_instnorm from slots: (a, b) per (n, c) from partial sums about a shift K
  apply      the apply pass with a real row length
  apply+pool in_apply_pool_kernel
  upsample   upsample2_trilinear_kernel with a pending norm

a x + b is ONE fused multiply-add in all of them (v_pk_fma_f32 in the gfx950 code of the converter waves, of in_apply_fast_kernel,
in_apply_pool_kernel and upsample2_trilinear_kernel).  torch has no fp32 fma on the host; `pending_f32` forms the product in float64,
where it is exact (24 + 24 bits), adds b there and rounds the sum to fp32.  That differs from the fma only when the float64 sum
rounds onto an exact fp32 tie that the unrounded sum was not: once in about 2^29 values, by one fp32 ulp of v (2^-24 relative), four
hundred times below the tightest bound that reads v (2e-6 rel-L2 over 864 terms), and inside every per-element bound below, which all
grant at least one fp32 rounding of the affine.  The activation, (v > 0 ? v : v k) + 0 with k = 0 / slope / 1, is exact to restate.
"""
import torch
import torch.nn.functional as F

from _util import check_copies, from_ndhwc_mx, max_rel, ref_conv_fp64, ref_conv_mx, rel_l2, split_pair, to_ndhwc_mx

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
C = 32                      # channels of the zx kernel
POISON = 0x7F
WORST = {}                  # launch kind -> (worst error / tolerance seen, error, tolerance): the figures of the module docstring


def note(kind, err, tol):
    r = float(err) / float(tol) if tol > 0 else (0.0 if err == 0 else float("inf"))
    if kind not in WORST or r > WORST[kind][0]:
        WORST[kind] = (r, float(err), float(tol))


# ------------------------------------------------------------------------------------------------ layouts
def zx_tile(h, w):
    """(TY, TX) of launch_conv_zx: 4x16 tiles wherever they fit, 2x32 otherwise."""
    return (4, 16) if (w % 16 == 0 and h % 4 == 0) else (2, 32)


def zx_eligible(d, h, w):
    return d % 2 == 0 and d >= 4 and ((w % 32 == 0 and h % 2 == 0) or (w % 16 == 0 and h % 4 == 0))


def zx_name(h, w, norm_in, planar):
    ty, tx = zx_tile(h, w)
    return "conv3d_k3_zx<f16x2mx,32->32,2x%dx%d,m4+x4+cv4,r6%s%s>" % (ty, tx, ",norm-in" if norm_in else "", ",o1" if planar else "")


def slot_map(h, w):
    """slot[y, x] of the statistics a main wave writes (amx_conv3d_zx.hip, the epilogue behind the march): slot = (tile y * nbx + tile
    x) * 2 + half, where a wave's half is the lower / upper row pair of a 4x16 tile and the left / right 16 columns of a 2x32 tile.
    A slot covers its 2 x 16 voxels of every plane and all 32 channels (the two cout tiles of an x half fill one slot)."""
    ty, tx = zx_tile(h, w)
    y = torch.arange(h)[:, None].expand(h, w)
    x = torch.arange(w)[None, :].expand(h, w)
    half = (y % ty) // 2 if tx == 16 else (x % tx) // 16
    return ((y // ty) * (w // tx) + x // tx) * 2 + half


def slot_where(h, w, s):
    ty, tx = zx_tile(h, w)
    return "tile (y %d, x %d) half %d of %dx%d tiles" % (s // 2 // (w // tx), s // 2 % (w // tx), s % 2, ty, tx)


def poisoned_raw(n, d, h, w, c):
    return torch.full((n, d, h, 3 * c // 16, w, 32), POISON, dtype=torch.uint8)


def raw_of(val, copies=True):
    """NCDHW fp32 -> row-planar storage; copies False: what a conv epilogue leaves (the pair, the caller's poison in the copy section)."""
    raw = to_ndhwc_mx(val)
    if not copies:
        raw[:, :, :, 2 * (val.shape[1] // 16):] = POISON
    return raw


def stored(val):
    hi, lo = split_pair(val.float(), torch.float16)
    return hi.float() + lo.float()


# ------------------------------------------------------------------------------------------------ references
def act_k(act, slope):
    return torch.tensor(0.0 if act == ACT_RELU else (slope if act == ACT_LRELU else 1.0), dtype=torch.float32)


def bcast(ab, i):
    return ab[:, :, i][:, :, None, None, None]


def pending_f32(x, ab, act, slope):
    """v = act(a x + b) as fp32, the value every consumer of a pending norm forms from the stored x (NCDHW fp32); ab [N, C, 2] or None."""
    x = x.float()
    if ab is None:
        return x + 0.0
    v = (x.double() * bcast(ab, 0).double() + bcast(ab, 1).double()).float()
    return torch.where(v > 0, v, v * act_k(act, slope)) + 0.0


def pending_f64(x, ab, act, slope):
    v = x.double() * bcast(ab, 0).double() + bcast(ab, 1).double()
    return torch.where(v > 0, v, v * act_k(act, slope).double())


def zx_refs(x, wgt, scale, bias, ab, act, slope):
    """(restated arithmetic, float64 convolution of the unrounded operands) of one zx layer on the stored input x."""
    v = pending_f32(x, ab, act, slope)
    return ref_conv_mx(v, None, wgt, scale, bias, 0, direct_lo=True), ref_conv_fp64(v, None, wgt, scale, bias, 0)


def slot_sums(val, bias, dtype=torch.float64):
    """[N, slots, C, 2] sums of d = val - bias and d^2 over each slot's voxels, and the same of |d| and d^2 (the bounds' scale)."""
    n, c, d, h, w = val.shape
    sm = slot_map(h, w).reshape(-1)
    dv = val.to(dtype) - (0 if bias is None else bias.to(dtype)[None, :, None, None, None])
    out = []
    for t in (dv, dv * dv, dv.abs()):
        per = t.sum(2).permute(0, 2, 3, 1).reshape(n, h * w, c)                 # [N, H W, C]
        out.append(torch.zeros(n, h * w // 32, c, dtype=dtype).index_add_(1, sm, per))
    return torch.stack((out[0], out[1]), -1), torch.stack((out[2], out[1]), -1)


def finalize_f64(part, kshift, vox, eps, gamma=None, beta=None):
    """(a, b) [N, C, 2] in float64 from partial sums [N, S, C, 2] about the shift kshift [C] (or None), biased variance; and the size
    of what the roundings of b act on, (|K| + |m1|) |a| + |beta| (b = beta - (K + m1) a may cancel to nothing)."""
    s = part.double().sum(1)
    m1 = s[..., 0] / vox
    var = (s[..., 1] / vox - m1 * m1).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mean = m1 + (0.0 if kshift is None else kshift.double()[None])
    g = 1.0 if gamma is None else gamma.double()[None]
    b = (0.0 if beta is None else beta.double()[None]) - mean * rstd * g
    size = (m1.abs() + (0.0 if kshift is None else kshift.double()[None].abs())) * (rstd * g).abs() + (0.0 if beta is None else beta.double()[None].abs())
    return torch.stack((rstd * g + 0 * b, b), -1), size


def finalize_f32(part, kshift, vox, eps, gamma=None, beta=None):
    """The same entirely in fp32, the slots added in in_finalize_kernel's order (lane l takes slots l, l + 32, ...; then the 32 lanes
    in order): the emulation whose deviation from float64 sizes the tolerance of the device's (a, b)."""
    p = part.float()
    lanes = [torch.zeros_like(p[:, 0]) for _ in range(32)]
    for b in range(p.shape[1]):
        lanes[b % 32] = lanes[b % 32] + p[:, b]
    s = torch.zeros_like(p[:, 0])
    for k in range(32):
        s = s + lanes[k]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    m1 = s[..., 0] / f(float(vox))
    var = (s[..., 1] / f(float(vox)) - m1 * m1).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + f(eps))
    mean = m1 + (0.0 if kshift is None else kshift.float()[None])
    g = 1.0 if gamma is None else gamma.float()[None]
    b = (0.0 if beta is None else beta.float()[None]) - mean * rstd * g
    return torch.stack((rstd * g + 0 * b, b), -1)


def ab_deviation(ab, ref, bscale):
    """Worst relative deviation of pairs [N, C, 2] from the float64 ones: a against |a|, b against the size finalize_f64
    returns with them."""
    da = ((ab[..., 0].double() - ref[..., 0]).abs() / ref[..., 0].abs().clamp_min(1e-300)).max().item()
    db = ((ab[..., 1].double() - ref[..., 1]).abs() / bscale.clamp_min(1e-300)).max().item()
    return max(da, db)


def pool_windows(t):
    """[N, C, D, H, W] -> [8, N, C, D/2, H/2, W/2]: the eight voxels of every 2x2x2 window."""
    return torch.stack([t[:, :, dz::2, dy::2, dx::2] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)])


def upsample_ref(v):
    return F.interpolate(v.double(), scale_factor=2, mode="trilinear", align_corners=False)


# ------------------------------------------------------------------------------------------------ comparisons (GPU tests and host proof)
def fail(what, msg):
    raise AssertionError("%s: %s" % (what, msg))


def check_pair(raw, c, what, copies_poisoned):
    """The stored pair is a proper split; a conv epilogue leaves the copy section alone."""
    val, x8, hi, lo = from_ndhwc_mx(raw, c, parts=True)
    if not torch.isfinite(val).all():
        fail(what, "non-finite stored values")
    if not (lo.float().abs() <= hi.float().abs() * 2.0 ** -11 + 2.0 ** -25).all():
        fail(what, "the stored pair is not a split: |lo| > 2^-11 |hi| + 2^-25")
    if copies_poisoned and not (x8 == POISON).all():
        fail(what, "%d bytes of the copy section were written" % (x8 != POISON).sum().item())
    return val, hi, lo


def check_slots(stats, val, bias, what):
    """stats [N, slots, 32, 2] against the float64 sums of the STORED output val: |error| <= (n 2^-24 + 2^-22) sum|d| for s1 and the
    same with d^2 for s2 -- n = 32 D fp32 additions in some order, 2^-22 for the pair that replaced the fp32 value."""
    n, c, d, h, w = val.shape
    ref, scale = slot_sums(val, bias)
    tol = (32 * d * 2.0 ** -24 + 2.0 ** -22) * scale
    err = (stats.double() - ref).abs()
    bad = err > tol
    worst = (err / tol.clamp_min(1e-300)).max().item()
    note("zx statistics slots", worst, 1.0)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        fail(what, "statistics slot %d (%s) of sample %d, channel %d, s%d: %.9g, float64 sum of the stored output %.9g, bound %.3g"
             % (i[1], slot_where(h, w, i[1]), i[0], i[2], i[3] + 1, stats[tuple(i)].item(), ref[tuple(i)].item(), tol[tuple(i)].item()))


def check_zx(res, x, wgt, scale, bias, ab, act, slope, planar, refs=None, flag=0):
    """One zx launch: res = dict(kernel, out (raw uint8) or out32, stats or None, flag)."""
    n, _, d, h, w = x.shape
    what = zx_name(h, w, ab is not None, planar)
    if res["kernel"] != what:
        fail(what, "the launch ran %r" % res["kernel"])
    ref, full = refs if refs is not None else zx_refs(x, wgt, scale, bias, ab, act, slope)
    if planar:
        got = res["out32"]
        if not torch.isfinite(got).all():
            fail(what, "non-finite output")
    else:
        got = check_pair(res["out"], C, what, copies_poisoned=True)[0]
    e, m, f = rel_l2(got, ref), max_rel(got, ref), rel_l2(got, full)
    note("zx conv rel-L2 vs restated arithmetic", e, 2e-6)
    note("zx conv max-rel vs restated arithmetic", m, 1e-5)
    note("zx conv rel-L2 vs float64 of unrounded operands", f, 4e-5)
    if not (e < 2e-6 and m < 1e-5):
        i = (got.double() - ref.double()).abs().flatten().argmax().item()
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), got.shape)]
        fail(what, "rel-L2 %.3g (< 2e-6) max-rel %.3g (< 1e-5) against the restated arithmetic, worst at (n, c, z, y, x) = %s" % (e, m, idx))
    if not f < 4e-5:
        fail(what, "rel-L2 %.3g (< 4e-5) against the float64 convolution of the unrounded operands" % f)
    if res.get("stats") is not None:
        check_slots(res["stats"], got, bias, what)
    if res["flag"] != flag:
        fail(what, "range flag %d, expected %d" % (res["flag"], flag))
    return got


def check_stored_value(got, ref, t, what, kind, label):
    """got, the value of a stored pair, against the float64 ref of the fp32 value v behind it, |v - ref| <= t.  The issue's bound for
    this is t + 2^-22 |ref|, whose second term is the pair's error where lo is a normal f16 (2^-11 of a residual of 2^-11 |v|).  A lo
    below 2^-14 is a subnormal f16 with a spacing of 2^-24, so that term holds for every pair only from |ref| >= 2^-3 on (2^-25 <=
    2^-22 |ref|); the host emulation, which is torch arithmetic alone, misses it below (0.0639473 stored 2.5e-8 off, bound 2.3e-8).
    So: the stated bound wherever it can hold, and everywhere the exact statement it abbreviates -- the split is monotone, hence
    stored(ref - t) <= got <= stored(ref + t), which is the tighter of the two wherever both apply."""
    def outward(v, up):
        f = v.float()
        over = (f.double() < v) if up else (f.double() > v)
        return torch.where(over, torch.nextafter(f, torch.full_like(f, float("inf") if up else float("-inf"))), f)
    lo_b, hi_b = stored(outward(ref - t, False)), stored(outward(ref + t, True))
    err = (got.double() - ref).abs()
    tol = t + 2.0 ** -22 * ref.abs()
    big = ref.abs() >= 2.0 ** -3
    bad = (got < lo_b) | (got > hi_b) | (big & (err > tol))
    if big.any():
        note(kind, (err / tol.clamp_min(1e-300))[big].max().item(), 1.0)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        fail(what, "%s at (n, c, z, y, x) = %s: %.9g, float64 %.9g, bound %.3g (stored interval [%.9g, %.9g])"
             % (label, i, got[tuple(i)].item(), ref[tuple(i)].item(), tol[tuple(i)].item(), lo_b[tuple(i)].item(), hi_b[tuple(i)].item()))


def check_apply(raw, x, ab, act, slope, what, kind="norm apply"):
    """The in-place tensor equals act(a x + b) of the stored input x: per element one fp32 rounding of the affine plus the pair,
    2^-23 (|a x| + |b|) + 2^-22 |y| (check_stored_value); copies as check_copies holds them."""
    got = check_copies(raw, x.shape[1], what)
    ref = pending_f64(x, ab, act, slope)
    t = 2.0 ** -23 * ((x.double() * bcast(ab, 0).double()).abs() + bcast(ab, 1).double().abs())
    check_stored_value(got, ref, t, what, kind + " per-element", "in-place value")
    return got


def check_max_pool(pooled_raw, inplace_raw, c, what):
    """hi and lo of the pooled tensor are bit-equal to one of the eight in-place stored pairs of its window, one that holds the
    window's maximum by value (the split is monotone, so the pair of the maximum is the maximum of the pairs)."""
    check_copies(pooled_raw, c, what + " (pooled)")
    _, _, ph, pl = from_ndhwc_mx(pooled_raw, c, parts=True)
    _, _, ih, il = from_ndhwc_mx(inplace_raw, c, parts=True)
    cf = lambda t: t.permute(0, 4, 1, 2, 3)
    h8, l8 = pool_windows(cf(ih)), pool_windows(cf(il))
    v8 = h8.float() + l8.float()
    ok = ((h8 == cf(ph)[None]) & (l8 == cf(pl)[None]) & (v8 == v8.max(0).values[None])).any(0)
    note("apply+pool max, pairs off", (~ok).sum().item(), 0.5)
    if not ok.all():
        i = (~ok).nonzero()[0].tolist()
        fail(what, "max-pooled pair at (n, c, z, y, x) = %s is %.9g, the window's maximum is %.9g; %d of %d pairs differ"
             % (i, (cf(ph).float() + cf(pl).float())[tuple(i)].item(), v8.max(0).values[tuple(i)].item(), (~ok).sum().item(), ok.numel()))


def check_avg_pool(pooled_raw, x, ab, act, slope, what):
    """Within 8 2^-24 mean|v| + 2^-22 |y| of the float64 mean of the eight fp32 values v = act(a x + b) (check_stored_value)."""
    got = check_copies(pooled_raw, x.shape[1], what + " (pooled)")
    v8 = pool_windows(pending_f32(x, ab, act, slope)).double()
    check_stored_value(got, v8.mean(0), 8 * 2.0 ** -24 * v8.abs().mean(0), what, "apply+pool avg per-element", "average")


def check_upsample(raw, x, ab, act, slope, what):
    got = check_copies(raw, x.shape[1], what)
    ref = upsample_ref(pending_f32(x, ab, act, slope)).float()
    e = rel_l2(got, ref)
    note("upsample pending rel-L2", e, 1e-6)
    if not e < 1e-6:
        i = (got.double() - ref.double()).abs().flatten().argmax().item()
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), got.shape)]
        fail(what, "rel-L2 %.3g (< 1e-6) against float64 trilinear interpolation of act(a x + b), worst at (n, c, z, y, x) = %s" % (e, idx))
    return got


NAME_APPLY = "instnorm+act"
NAME_POOL = "instnorm+act+pool2<%s>"
NAME_UP = "upsample2<trilinear> with a pending norm"
NAME_STATS_ONLY = "instnorm statistics only (apply fused into the next %s)"


# ------------------------------------------------------------------------------------------------ host emulation, with planted defects
DEFECTS = ("halo_clamp", "half_swap", "sample_ab", "max_before_affine", "pool_lane", "border_act", "lo_copy_raw")


def emulate_zx(x, wgt, scale, bias, ab, act, slope, planar=False, defect=None):
    """What the zx launch stores for the stored input x, from the restated arithmetic.
    halo_clamp: the converter of tile (0, 0) clamps its halo row y = -1 (row 0 again) instead of reflecting it (row 1);
    half_swap: the two halves of the first tile's statistics land in each other's slot;
    sample_ab: sample 1 is normalised with sample 0's (a, b)."""
    n, _, d, h, w = x.shape
    ty, tx = zx_tile(h, w)
    use = ab
    if defect == "sample_ab":
        use = ab.clone()
        use[1] = ab[0]
    v = pending_f32(x, use, act, slope)
    out = ref_conv_mx(v, None, wgt, scale, bias, 0, direct_lo=True)
    if defect == "halo_clamp":
        # row 0 of the x range of tile (0, 0) holds the outputs that read the halo row: redo them from a tensor whose row y = -1 is
        # row 0.  A reflect-padded tensor convolved again and cropped gives the same interior, whatever its own padding holds.
        vp = F.pad(v, (1,) * 6, mode="reflect")
        vp[:, :, :, 0, :tx + 2] = vp[:, :, :, 1, :tx + 2]
        wrong = ref_conv_mx(vp, None, wgt, scale, bias, 0, direct_lo=True)[:, :, 1:-1, 1:-1, 1:-1]
        out[:, :, :, 0, :tx] = wrong[:, :, :, 0, :tx]
    res = dict(kernel=zx_name(h, w, ab is not None, planar), flag=0, stats=None)
    if planar:
        res["out32"] = out
        return res
    res["out"] = raw_of(out, copies=False)
    stats = slot_sums(out, bias)[0].float()
    if defect == "half_swap":
        stats[:, [0, 1]] = stats[:, [1, 0]]
    res["stats"] = stats
    return res


def emulate_apply(x, ab, act, slope, defect=None):
    """The apply pass in place.  sample_ab as above; lo_copy_raw: the xl8 copy bytes come from the un-normalised value."""
    use = ab
    if defect == "sample_ab":
        use = ab.clone()
        use[1] = ab[0]
    raw = raw_of(pending_f32(x, use, act, slope))
    if defect == "lo_copy_raw":
        k = x.shape[1] // 16
        raw[:, :, :, 2 * k:, :, :16] = to_ndhwc_mx(x)[:, :, :, 2 * k:, :, :16]
    return raw


def emulate_apply_pool(x, ab, act, slope, avg, defect=None):
    """(in-place tensor, pooled tensor).  max_before_affine: the maximum of the raw window goes through the affine (wrong wherever
    a < 0); pool_lane: the partner along x is taken from the other lane of the copy-exchange pair -- the neighbouring 8-channel group
    of the SAME column -- instead of from the next column."""
    v = pending_f32(x, ab, act, slope)
    red = (lambda t: t.double().mean(0).float()) if avg else (lambda t: t.max(0).values)
    pooled = red(pool_windows(v))
    if defect == "max_before_affine":
        pooled = pending_f32(pool_windows(x.float()).max(0).values, ab, act, slope)
    if defect == "pool_lane":
        n, c, d, h, w = v.shape
        other = v.reshape(n, c // 16, 2, 8, d, h, w).flip(2).reshape(n, c, d, h, w)       # group c8 ^ 1
        even = torch.stack([t[:, :, dz::2, dy::2, 0::2] for t in (v, other) for dz in (0, 1) for dy in (0, 1)])
        pooled = red(even)
    return raw_of(v), raw_of(pooled)


def emulate_upsample(x, ab, act, slope, defect=None):
    """border_act: the cells on the clamped border (output positions 0 and 2L - 1 of an axis) interpolate a x + b without the
    activation."""
    out = upsample_ref(pending_f32(x, ab, act, slope)).float()
    if defect == "border_act":
        plain = upsample_ref(pending_f32(x, ab, ACT_NONE, slope)).float()
        for ax in (2, 3, 4):
            for pos in (0, out.shape[ax] - 1):
                out.select(ax, pos).copy_(plain.select(ax, pos))
    return raw_of(out)
