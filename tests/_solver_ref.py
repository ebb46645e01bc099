"""CPU restatement of the registration's discrete stage (coupled_convex, inverse_consistency, the trilinear upsampling and
their composition run_stage1_registration), and the seeded inputs of its test cases.

TEST INFRASTRUCTURE ONLY: imported by the tests and by tools/make_golden_solver.py, never by the product path.  Written
from the formulas -- explicit loops over the displacement labels, explicit corner gathers for grid_sample / interpolate --
in fp32 with the reference's operation order, and pinned by tests/golden/solver_golden.npz, which holds outputs of the
reference's own functions (anatomix/registration/convex_adam_utils.py:494-603, instance_optimization.py:122-222) run in
fp32 on the CPU.
"""
import numpy as np

F32 = np.float32
COEFFS = np.array([0.003, 0.01, 0.03, 0.1, 0.3, 1.0], dtype=F32)
TINY = F32(1e-30)


# ---- inputs ------------------------------------------------------------------------------------------------------------

# case -> (h, w, d, channels, disp_hw, grid_sp) for the synthetic ones; the three of oracle.registration_inputs.CASES go
# through MIND-SSC + merged pooled features
SYNTH = {"hw3_ragged": (9, 7, 11, 6, 3, 2), "roll48": (48, 48, 48, 28, 1, 2)}
ROLL = (1, 0, -1)                     # grid cells; disp_soft channel c is the displacement along axis c of [h, w, d]
ROLL_NOISE = 0.02


def case_names():
    from oracle.registration_inputs import CASES
    return list(CASES) + list(SYNTH)


def _smooth(rs, shape, passes):
    a = rs.rand(*shape).astype(F32)
    for _ in range(passes):
        for ax in (-3, -2, -1):
            a = (a + np.roll(a, 1, ax) + np.roll(a, -1, ax)) / F32(3)
    return ((a - a.min()) / (a.max() - a.min())).astype(F32)


def features(case):
    """(feat_fix, feat_mov [C, h, w, d] on the coarse grid, disp_hw, grid_sp, (H, W, D))."""
    from oracle import registration_ref as RR
    from oracle.registration_inputs import CASES, inputs
    if case in CASES:
        img_f, img_m, feat_f, feat_m, _, _, g, hw, scale = inputs(case)
        fix = RR.merged_pooled(RR.mindssc(img_f, 1, 2), feat_f, scale, g)
        mov = RR.merged_pooled(RR.mindssc(img_m, 1, 2), feat_m, scale, g)
        return fix, mov, hw, g, tuple(int(v) for v in img_f.shape)
    h, w, d, c, hw, g = SYNTH[case]
    rs = np.random.RandomState(1234 + len(case))
    if case == "roll48":
        fix = (_smooth(rs, (c, h, w, d), 1) * 2).astype(F32)
        mov = (np.roll(fix, ROLL, (1, 2, 3)) + rs.randn(c, h, w, d).astype(F32) * F32(ROLL_NOISE)).astype(F32)
    else:
        fix = (_smooth(rs, (c, h, w, d), 1) * 2).astype(F32)
        mov = (np.roll(fix, (2, -1, 1), (1, 2, 3)) + rs.randn(c, h, w, d).astype(F32) * F32(0.05)).astype(F32)
    return fix, mov, hw, g, (h * g, w * g + (1 if case == "hw3_ragged" else 0), d * g)


def ssd_of(case, reverse=False):
    """The correlation volume every side of the solver tests starts from (oracle.registration_ref.correlate, fp32 numpy)."""
    from oracle import registration_ref as RR
    fix, mov, hw, g, sizes = features(case)
    ssd, amin = RR.correlate(mov, fix, hw) if reverse else RR.correlate(fix, mov, hw)
    return ssd, amin, hw, g, sizes


def smooth_fields(shape, seed, amp):
    """Two smooth [3, h, w, d] fields in normalised coordinates for the consistency sweeps (a few cells of displacement)."""
    rs = np.random.RandomState(seed)
    a = (_smooth(rs, (3,) + tuple(shape), 2) - F32(0.5)) * F32(amp)
    b = (_smooth(rs, (3,) + tuple(shape), 2) - F32(0.5)) * F32(amp)
    return a.astype(F32), b.astype(F32)


# ---- coupled_convex ------------------------------------------------------------------------------------------------------

def mesh(disp_hw):
    """[3, k^3]: mesh[:, m] = (m % k, (m / k) % k, m / k^2) - disp_hw, the label order F.affine_grid(disp_hw * eye(3, 4),
    (1, 1, k, k, k), align_corners=True).permute(0, 4, 1, 2, 3).reshape(3, -1) produces."""
    k = 2 * disp_hw + 1
    m = np.arange(k ** 3)
    return np.stack([m % k - disp_hw, (m // k) % k - disp_hw, m // (k * k) - disp_hw]).astype(F32)


def box3(x):
    """avg_pool3d(3, stride 1, padding 1), zero padding, divisor 27.  x [C, h, w, d]."""
    c, h, w, d = x.shape
    p = np.zeros((c, h + 2, w + 2, d + 2), F32)
    p[:, 1:-1, 1:-1, 1:-1] = x
    acc = np.zeros_like(x, dtype=F32)
    for tz in range(3):
        for ty in range(3):
            for tx in range(3):
                acc += p[:, tz:tz + h, ty:ty + w, tx:tx + d]
    return (acc / F32(27)).astype(F32)


def coupled_step(ssd, hist):
    """One iteration from the soft fields so far (hist: list of [3, h, w, d]): cost(m) = (((ssd(m) + c_0 p_0) + c_1 p_1) ...),
    p_i = (d0^2 + d1^2) + d2^2 with d = mesh_m - s_i.  Returns (label int64 [h, w, d] -- the FIRST minimum --, s [3, h, w, d],
    margin [h, w, d] = (second best - best) / max(|best|, tiny))."""
    ssd = np.asarray(ssd, F32)
    n = ssd.shape[0]
    hw = {27: 1, 125: 2, 343: 3}[n]
    ms = mesh(hw)
    best = np.full(ssd.shape[1:], np.inf, F32)
    second = np.full(ssd.shape[1:], np.inf, F32)
    label = np.zeros(ssd.shape[1:], np.int64)
    for m in range(n):
        v = ssd[m].copy()
        for i, s in enumerate(hist):
            d0, d1, d2 = ms[0, m] - s[0], ms[1, m] - s[1], ms[2, m] - s[2]
            v = v + COEFFS[i] * ((d0 * d0 + d1 * d1) + d2 * d2)
        assert v.dtype == F32
        less = v < best
        second = np.where(less, best, np.minimum(second, v))
        label = np.where(less, m, label)
        best = np.where(less, v, best)
    with np.errstate(invalid="ignore", over="ignore"):
        margin = (second - best) / np.maximum(np.abs(best), TINY)
    return label, box3(ms[:, label.reshape(-1)].reshape((3,) + label.shape)), margin


def coupled_convex(ssd, argmin=None):
    """Returns (s_6 [3, h, w, d], dict(labels=[7], soft=[s_0 .. s_6], margins=[7])); iteration 0 is the plain argmin."""
    hist, labels, margins = [], [], []
    for j in range(7):
        lab, s, mg = coupled_step(ssd, hist)
        if j == 0 and argmin is not None:
            lab = np.asarray(argmin, np.int64)
            s = box3(mesh({27: 1, 125: 2, 343: 3}[ssd.shape[0]])[:, lab.reshape(-1)].reshape((3,) + lab.shape))
        hist.append(s)
        labels.append(lab)
        margins.append(mg)
    return hist[-1], {"labels": labels, "soft": hist, "margins": margins}


def near_tie_share(margins, thr=1e-5):
    """Share of voxels whose margin is below thr in any of the six coupled iterations (1 .. 6)."""
    near = np.zeros(margins[1].shape, bool)
    for mg in margins[1:]:
        near |= ~(mg >= thr)
    return float(near.mean())


def disagree_share(a, b, tol=1e-4):
    """Share of voxels where any component of the two [3, ...] fields differs by more than tol."""
    return float((np.abs(np.asarray(a, F32) - np.asarray(b, F32)) > tol).any(0).mean())


# ---- inverse_consistency ---------------------------------------------------------------------------------------------------

def identity_coord(n):
    """F.affine_grid(eye, align_corners=False) along one axis: linspace(-1, 1, n) * (n - 1) / n in fp32, with
    torch.linspace's two-sided evaluation, each side one fused multiply-add (emulated in float64: the product of two
    fp32 numbers is exact there)."""
    if n <= 1:
        return np.zeros(n, F32)
    i = np.arange(n)
    step = np.float64(F32(2) / F32(n - 1))
    lin = np.where(i < n // 2, -1.0 + step * i, 1.0 - step * (n - 1 - i)).astype(F32)
    return (lin * F32(n - 1) / F32(n)).astype(F32)


def grid_sample(field, gx, gy, gz):
    """F.grid_sample(field[None], grid) defaults: trilinear, zeros, align_corners=False.  field [C, H, W, D]; gx (last
    axis), gy, gz normalised coordinates [H, W, D]."""
    c, H, W, D = field.shape
    ix = ((gx + F32(1)) * F32(D) - F32(1)) / F32(2)
    iy = ((gy + F32(1)) * F32(W) - F32(1)) / F32(2)
    iz = ((gz + F32(1)) * F32(H) - F32(1)) / F32(2)
    fx, fy, fz = np.floor(ix), np.floor(iy), np.floor(iz)
    wx = (fx + F32(1) - ix, ix - fx)
    wy = (fy + F32(1) - iy, iy - fy)
    wz = (fz + F32(1) - iz, iz - fz)
    out = np.zeros((c, H, W, D), F32)
    for j in range(8):                                   # corner order of grid_sampler_3d: x fastest, then y, then z
        bx, by, bz = j & 1, (j >> 1) & 1, j >> 2
        xx, yy, zz = fx.astype(np.int64) + bx, fy.astype(np.int64) + by, fz.astype(np.int64) + bz
        inside = (xx >= 0) & (xx < D) & (yy >= 0) & (yy < W) & (zz >= 0) & (zz < H)
        v = field[:, np.clip(zz, 0, H - 1), np.clip(yy, 0, W - 1), np.clip(xx, 0, D - 1)]
        v = np.where(inside[None], v, F32(0))
        out = out + v * (wx[bx] * wy[by] * wz[bz])[None]
    return out.astype(F32)


def inverse_consistency(a, b, iterations=20):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    _, H, W, D = a.shape
    idz, idy, idx = np.meshgrid(identity_coord(H), identity_coord(W), identity_coord(D), indexing="ij")
    for _ in range(iterations):
        na = F32(0.5) * (a - grid_sample(b, idx + a[0], idy + a[1], idz + a[2]))
        nb = F32(0.5) * (b - grid_sample(a, idx + b[0], idy + b[1], idz + b[2]))
        a, b = na.astype(F32), nb.astype(F32)
    return a, b


# ---- trilinear resize --------------------------------------------------------------------------------------------------------

def _linear_src(n_in, n_out):
    ratio = F32(n_in) / F32(n_out)
    src = ratio * (np.arange(n_out).astype(F32) + F32(0.5)) - F32(0.5)
    src = np.maximum(src, F32(0)).astype(F32)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(F32)).astype(F32)
    return i0, i1, F32(1) - l1, l1


def resize_trilinear(x, size, scale=None, flip=False):
    """F.interpolate(x.flip(0) * scale[:, None, None, None], size, mode="trilinear", align_corners=False).  x [C, h, w, d]."""
    x = np.asarray(x, F32)
    if flip:
        x = x[::-1]
    if scale is not None:
        x = (x * np.asarray(scale, F32)[:, None, None, None]).astype(F32)
    z0, z1, lz0, lz1 = _linear_src(x.shape[1], size[0])
    y0, y1, ly0, ly1 = _linear_src(x.shape[2], size[1])
    x0, x1, lx0, lx1 = _linear_src(x.shape[3], size[2])

    def g(zi, yi, xi):
        return x[:, zi[:, None, None], yi[None, :, None], xi[None, None, :]]
    lz0, lz1 = lz0[:, None, None], lz1[:, None, None]
    ly0, ly1 = ly0[None, :, None], ly1[None, :, None]
    out = (lz0 * (ly0 * (lx0 * g(z0, y0, x0) + lx1 * g(z0, y0, x1)) + ly1 * (lx0 * g(z0, y1, x0) + lx1 * g(z0, y1, x1))) +
           lz1 * (ly0 * (lx0 * g(z1, y0, x0) + lx1 * g(z1, y0, x1)) + ly1 * (lx0 * g(z1, y1, x0) + lx1 * g(z1, y1, x1))))
    return out.astype(F32)


# ---- run_stage1_registration -----------------------------------------------------------------------------------------------

def run_stage1(fix, mov, disp_hw, grid_sp, sizes, ic):
    """[3, h, w, d] in grid units (ic False) or [3, H, W, D] in voxels (ic True), as instance_optimization.py:122-222."""
    from oracle import registration_ref as RR
    ssd, amin = RR.correlate(fix, mov, disp_hw)
    soft, _ = coupled_convex(ssd, amin)
    if not ic:
        return soft
    ssd_, amin_ = RR.correlate(mov, fix, disp_hw)
    soft_, _ = coupled_convex(ssd_, amin_)
    h, w, d = soft.shape[1:]
    scale = np.array([F32(h - 1) / F32(2), F32(w - 1) / F32(2), F32(d - 1) / F32(2)], F32)
    a = (soft / scale[:, None, None, None])[::-1]
    b = (soft_ / scale[:, None, None, None])[::-1]
    ice, _ = inverse_consistency(a, b, 15)
    return resize_trilinear(ice, sizes, scale * F32(grid_sp), flip=True)
