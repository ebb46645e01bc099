"""numpy restatement of the two-view augmentation of the contrastive pretraining, written from the
definitions alone and independent of anatomix_amd: the reference of tests/test_pretrain_augment*.py.  Every function takes ``dt``
(numpy float64 or float32) and evaluates the same formulas in that type; the float32 evaluation's distance from the float64 one is
the e32 of the tests' bound.  Parameters are what the device receives: rounded to float32 first.  TorchIO is not available here;
test_pretrain_augment.py pins the pieces to grid_sample, scipy.ndimage.gaussian_filter, polygrid3d and the 3-D FFT definition."""
import math

import numpy as np

INTENSITY = ("blur", "noise", "bias", "gamma", "motion")


def f32(v, dt):
    """A parameter as the kernels receive it (float32), in the evaluation's type."""
    return np.asarray(v, np.float64).astype(np.float32).astype(dt)


# ---- flip + affine ------------------------------------------------------------------------------------------------------------
def rotation(degrees):
    a0, a1, a2 = (math.radians(float(v)) for v in degrees)
    Rx = np.array([[1, 0, 0], [0, math.cos(a0), -math.sin(a0)], [0, math.sin(a0), math.cos(a0)]])
    Ry = np.array([[math.cos(a1), 0, math.sin(a1)], [0, 1, 0], [-math.sin(a1), 0, math.cos(a1)]])
    Rz = np.array([[math.cos(a2), -math.sin(a2), 0], [math.sin(a2), math.cos(a2), 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def spatial_map(shape, flip_axes=(False, False, False), scales=None, degrees=None):
    """o -> source index, 3 x 4 float64.  The affine's forward map is F(p) = c + R diag(s) (p - c), its output voxel o samples the
    flipped image at q = F^-1(o) = c + diag(1 / s) R^T (o - c), and the flipped image at q is the input at n - 1 - q on a flipped axis."""
    n = np.asarray(shape, np.float64)
    c = (n - 1) / 2
    M = np.zeros((3, 4))
    A = np.eye(3)
    if scales is not None:
        A = np.linalg.inv(rotation(degrees) @ np.diag(np.asarray(scales, np.float64)))
    M[:, :3], M[:, 3] = A, c - A @ c
    for a in range(3):
        if flip_axes[a]:
            M[a] = -M[a]
            M[a, 3] += n[a] - 1
    return M


def rigid_map(shape, degrees, translation):
    """The rigid move F(p) = c + R (p - c) + t: o samples F^-1(o) = c + R^T (o - c - t)."""
    c = (np.asarray(shape, np.float64) - 1) / 2
    Rt = rotation(degrees).T
    M = np.zeros((3, 4))
    M[:, :3], M[:, 3] = Rt, c - Rt @ (c + np.asarray(translation, np.float64))
    return M


def seeded_map(seed, shape):
    """Seed 0 flip-only, 1 affine-only, 2.. both, from the transform's own ranges.  How many voxels a map puts within 1e-4 of a
    half-integer is a property of the map alone (they come in pairs mirrored about the centre; on 9 x 11 x 7 two pairs are already
    0.58 %): for seeds 0 .. 5 and the tests' three shapes these maps exclude at most 0.29 %, which the tests assert."""
    r = np.random.RandomState(3000 + seed)
    flips = r.uniform(size=3) < 0.5
    scales, degrees = r.uniform(0.6, 1.4, 3), r.uniform(-45, 45, 3)
    if seed == 0:
        return spatial_map(shape, (True, False, True))
    if seed == 1:
        return spatial_map(shape, (False,) * 3, scales, degrees)
    return spatial_map(shape, flips, scales, degrees)


def source_index(M, shape, dt):
    M = f32(M, dt)
    o = np.meshgrid(*[np.arange(n).astype(dt) for n in shape], indexing="ij")
    return [M[a, 0] * o[0] + M[a, 1] * o[1] + M[a, 2] * o[2] + M[a, 3] for a in range(3)]


def resample(img, lab, M, pad, dt):
    """-> (image trilinear with ``pad`` for a corner outside, label nearest by round-half-to-even with 0 outside (None without ``lab``),
    the three source indices).  A source index that is integral on all three axes takes the voxel itself."""
    img = img.astype(dt)
    S = img.shape
    pad = dt(pad)
    src = source_index(M, S, dt)
    i0 = [np.floor(s) for s in src]
    fr = [s - i for s, i in zip(src, i0)]
    out = np.zeros(S, dt)
    for c in range(8):
        off = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        idx = [(i + o).astype(np.int64) for i, o in zip(i0, off)]
        ok = np.ones(S, bool)
        w = np.ones(S, dt)
        for a in range(3):
            ok &= (idx[a] >= 0) & (idx[a] < S[a])
            w = w * (fr[a] if off[a] else 1 - fr[a])
        v = img[tuple(np.clip(i, 0, s - 1) for i, s in zip(idx, S))]
        out = out + w * np.where(ok, v, pad)
    whole = (fr[0] == 0) & (fr[1] == 0) & (fr[2] == 0)
    idx = [i.astype(np.int64) for i in i0]
    ok = np.ones(S, bool)
    for a in range(3):
        ok &= (idx[a] >= 0) & (idx[a] < S[a])
    out = np.where(whole, np.where(ok, img[tuple(np.clip(i, 0, s - 1) for i, s in zip(idx, S))], pad), out)
    olab = None
    if lab is not None:
        nidx = [np.rint(s).astype(np.int64) for s in src]
        ok = np.ones(S, bool)
        for a in range(3):
            ok &= (nidx[a] >= 0) & (nidx[a] < S[a])
        olab = np.where(ok, lab[tuple(np.clip(i, 0, s - 1) for i, s in zip(nidx, S))], 0).astype(np.uint8)
    return out, olab, src


def half_integer_margin(src):
    """Per voxel the smallest distance of a source index from a half-integer over the three axes."""
    return np.minimum.reduce([np.abs(s - np.floor(s) - 0.5) for s in src])


def is_integral_map(M):
    return bool(np.all(np.asarray(M) == np.rint(M)))


# ---- blur ---------------------------------------------------------------------------------------------------------------------
def gaussian_taps(sigma):
    """(radius, float64 taps): exp(-k^2 / 2 sigma^2) normalised to 1, radius = int(4 sigma + 0.5); sigma <= 1e-15: (0, [1])."""
    sigma = float(sigma)
    if sigma <= 1e-15:
        return 0, np.ones(1)
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * k * k)
    return r, phi / phi.sum()


def blur(x, sigmas, dt, round_taps=True):
    """Separable, half-sample symmetric reflection (numpy's 'symmetric' = scipy's 'reflect', repeated where the radius exceeds the
    axis); the last axis first.  ``round_taps``: the taps rounded to float32 as the device receives them."""
    x = x.astype(dt)
    for axis in (2, 1, 0):
        r, taps = gaussian_taps(sigmas[axis])
        if r == 0:
            continue
        taps = f32(taps, dt) if round_taps else taps.astype(dt)
        n = x.shape[axis]
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        xp = np.pad(x, pad, mode="symmetric")
        acc = np.zeros_like(x)
        for k in range(-r, r + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(r + k, r + k + n)
            acc = acc + taps[k + r] * xp[tuple(sl)]
        x = acc
    return x


# ---- noise, bias field, gamma -------------------------------------------------------------------------------------------------
def add_noise(x, std, noise, dt):
    return x.astype(dt) + f32(std, dt) * noise.astype(dt)


def coeff_index():
    return [(i, j, k) for i in range(4) for j in range(4 - i) for k in range(4 - i - j)]


def bias_exponent(shape, coeff, dt):
    c = f32(coeff, dt)
    ax = [np.linspace(-1, 1, n).astype(dt) if n > 1 else np.full(1, -1, dt) for n in shape]
    f = np.zeros(shape, dt)
    for q, (i, j, k) in enumerate(coeff_index()):
        f = f + c[q] * (ax[0][:, None, None] ** i * ax[1][None, :, None] ** j * ax[2][None, None, :] ** k).astype(dt)
    return f


def bias_field(x, coeff, dt):
    return x.astype(dt) * np.exp(bias_exponent(x.shape, coeff, dt))


def gamma(x, g, dt):
    x = x.astype(dt)
    return np.sign(x) * np.abs(x) ** f32(g, dt)


# ---- motion -------------------------------------------------------------------------------------------------------------------
def _motion_images(x, degrees, translation, dt):
    x = x.astype(dt)
    return [x] + [resample(x, None, rigid_map(x.shape, degrees[i], translation[i]), x.min(), dt)[0] for i in range(2)]


def motion(x, degrees, translation, times, dt):
    """The 3-D definition: K_i = fftshift(fftn(img_i)), the composite takes [0, c_1) of the last axis from K_0, [c_1, c_2) from K_1 and
    [c_2, W) from K_2, c_i = int(t_i W); real(ifftn(ifftshift(K)))."""
    ct = np.complex128 if dt == np.float64 else np.complex64
    imgs = _motion_images(x, degrees, translation, dt)
    W = x.shape[-1]
    cuts = [0] + [int(t * W) for t in times] + [W]
    K = [np.fft.fftshift(np.fft.fftn(i)).astype(ct) for i in imgs]
    comp = np.zeros_like(K[0])
    for i in range(3):
        comp[..., cuts[i]:cuts[i + 1]] = K[i][..., cuts[i]:cuts[i + 1]]
    return np.fft.ifftn(np.fft.ifftshift(comp)).astype(ct).real.astype(dt)


def motion_1d(x, degrees, translation, times, dt):
    """The same through complex 1-D transforms along the last axis only."""
    ct = np.complex128 if dt == np.float64 else np.complex64
    imgs = _motion_images(x, degrees, translation, dt)
    W = x.shape[-1]
    cuts = [0] + [int(t * W) for t in times] + [W]
    K = [np.fft.fftshift(np.fft.fft(i, axis=-1), axes=-1).astype(ct) for i in imgs]
    comp = np.zeros_like(K[0])
    for i in range(3):
        comp[..., cuts[i]:cuts[i + 1]] = K[i][..., cuts[i]:cuts[i + 1]]
    return np.fft.ifft(np.fft.ifftshift(comp, axes=-1), axis=-1).astype(ct).real.astype(dt)


# ---- the chain ----------------------------------------------------------------------------------------------------------------
def chain(A, B, seg, params, noise, dt):
    """The pair through flip + affine, then per view blur, noise, bias, gamma, motion, then the crop.  ``noise`` [2, D, H, W].
    -> ([image A, image B], label uint8, source indices or None)."""
    M = params["map"]
    views, lab, src = [A.astype(dt), B.astype(dt)], seg.astype(np.uint8), None
    if M is not None:
        out = [resample(v, seg, M, v.min(), dt) for v in views]
        views, lab, src = [o[0] for o in out], out[0][1], out[0][2]
    for v, rec in enumerate(params["views"]):
        x, on = views[v], rec["on"]
        if on["blur"]:
            x = blur(x, rec["sigma"], dt)
        if on["noise"]:
            x = add_noise(x, rec["noise_std"], noise[v], dt)
        if on["bias"]:
            x = bias_field(x, rec["coeff"], dt)
        if on["gamma"]:
            x = gamma(x, rec["gamma"], dt)
        if on["motion"]:
            x = motion_1d(x, rec["motion_degrees"], rec["motion_translation"], rec["motion_times"], dt)
        views[v] = x
    if params.get("crop_size", 0) > 0:
        half = params["crop_size"] // 2
        win = tuple(slice(s, s + 2 * half) for s in params["crop_start"])
        views, lab = [x[win] for x in views], lab[win]
        src = None if src is None else [s[win] for s in src]
    return views, lab, src


def blob_volume(shape, seed, n_labels=3):
    """A smooth image of ``n_labels`` blobs on a ramp and its label map (float64, labels 0 .. n_labels)."""
    r = np.random.RandomState(seed)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    img = 0.1 + 0.01 * (x[0] / shape[0] + 2 * x[1] / shape[1] + 3 * x[2] / shape[2])
    lab = np.zeros(shape)
    for n in range(n_labels):
        c = [r.uniform(0.25, 0.75) * s for s in shape]
        rad = r.uniform(0.18, 0.3) * min(shape)
        d2 = sum((x[a] - c[a]) ** 2 for a in range(3))
        img = img + (0.6 + 0.1 * n) * np.exp(-d2 / (2 * (0.6 * rad) ** 2))
        lab[d2 <= rad * rad] = n + 1
    return img, lab
