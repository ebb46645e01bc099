"""numpy restatement of the augmentation chain of segmentation finetuning, written from the definitions
alone and independent of anatomix_amd: the reference of tests/test_seg_augment*.py and tests/test_seg_train_gpu.py.  Every function
takes ``dt`` (numpy float64 or float32) and evaluates the same formulas in that type; the float32 evaluation's distance from the
float64 one is the e32 of the tests' bound.  Parameters are what the device receives: rounded to float32 first.  MONAI is not
available here; test_seg_augment.py pins the pieces to grid_sample, leggrid3d and the closed forms instead."""
import math

import numpy as np

SWITCH_NAMES = ("noise", "bias", "gibbs", "contrast", "smooth", "sharpen", "affine")
PROB = dict(noise=0.33, bias=0.33, gibbs=0.33, contrast=0.33, smooth=0.33, sharpen=0.33, affine=0.98)


def f32(v, dt):
    """A parameter as the kernels receive it (float32), in the evaluation's type."""
    return np.asarray(v, np.float64).astype(np.float32).astype(dt)


def scale_intensity(x, dt):
    x = x.astype(dt)
    mn, mx = x.min(), x.max()
    return x * dt(0) if mn == mx else (x - mn) / (mx - mn)


def legendre_values(x):
    return [np.ones_like(x), x, (3 * x * x - 1) / 2, (5 * x * x * x - 3 * x) / 2]


def coeff_index():
    return [(i, j, k) for i in range(4) for j in range(4 - i) for k in range(4 - i - j)]


def bias_exponent(shape, coeff, dt):
    c = f32(coeff, dt)
    P = [legendre_values(np.linspace(-1, 1, n).astype(dt) if n > 1 else np.full(1, -1, dt)) for n in shape]
    f = np.zeros(shape, dt)
    for q, (i, j, k) in enumerate(coeff_index()):
        f = f + c[q] * (P[0][i][:, None, None] * P[1][j][None, :, None] * P[2][k][None, None, :])
    return f


def crop(vol, corner, size):
    z, y, x = (int(c) for c in corner)
    return vol[z:z + size[0], y:y + size[1], x:x + size[2]]


def gibbs_radius(alpha, shape):
    return np.float32((1.0 - float(alpha)) * max(shape) * math.sqrt(2.0) / 2.0)


def gibbs(x, r, dt):
    """r: the float32 radius.  The mask compares 4 x the squared distance (an exact integer) with 4 r^2 in float64."""
    ax = [(2.0 * np.arange(n, dtype=np.float64) - (n - 1)) ** 2 for n in x.shape]
    mask = (ax[0][:, None, None] + ax[1][None, :, None] + ax[2][None, None, :]) <= 4.0 * float(r) * float(r)
    ct = np.complex128 if dt == np.float64 else np.complex64
    k = np.fft.fftshift(np.fft.fftn(x.astype(dt)).astype(ct)) * mask
    return np.fft.ifftn(np.fft.ifftshift(k)).astype(ct).real.astype(dt)


def adjust_contrast(x, gamma, dt):
    x = x.astype(dt)
    mn = x.min()
    rng = x.max() - mn
    return ((x - mn) / (rng + dt(1e-7))) ** f32(gamma, dt) * rng + mn


def gaussian_taps(sigma):
    sigma = float(sigma)
    tail = int(max(4.0 * sigma, 0.5) + 0.5)
    xs = range(-tail, tail + 1)
    if sigma == 0.0:
        return tail, np.array([1.0 if x == 0 else 0.0 for x in xs])
    t = 0.70710678 / sigma
    return tail, np.array([max(0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5))), 0.0) for x in xs])


def gaussian(x, sigmas, dt):
    """Separable, zero padding, taps not renormalised; the last axis first (the order does not matter in exact arithmetic)."""
    x = x.astype(dt)
    for axis in (2, 1, 0):
        r, taps = gaussian_taps(sigmas[axis])
        taps = f32(taps, dt)
        n = x.shape[axis]
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        xp = np.pad(x, pad)
        acc = np.zeros_like(x)
        for k in range(-r, r + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(r + k, r + k + n)
            acc = acc + taps[k + r] * xp[tuple(sl)]
        x = acc
    return x


def sharpen(x, sigma1, sigma2, alpha, dt):
    b = gaussian(x, sigma1, dt)
    return b + f32(alpha, dt) * (b - gaussian(b, sigma2, dt))


def affine_matrix(rotate, shear, scale):
    rx, ry, rz = (float(v) for v in rotate)
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    Sh = np.eye(3)
    Sh[0, 1], Sh[0, 2], Sh[1, 0] = shear
    return Rx @ Ry @ Rz @ Sh @ np.diag(np.asarray(scale, np.float64))


def seeded_matrix(seed):
    r = np.random.RandomState(1000 + seed)
    return affine_matrix(r.uniform(-math.pi / 4, math.pi / 4, 3), r.uniform(-0.2, 0.2, 3), 1 + r.uniform(-0.2, 0.2, 3))


def source_index(A, out_size, in_size, dt):
    A = f32(A, dt)
    o = np.meshgrid(*[np.arange(n).astype(dt) - dt((n - 1) / 2) for n in out_size], indexing="ij")
    return [A[a, 0] * o[0] + A[a, 1] * o[1] + A[a, 2] * o[2] + dt((in_size[a] - 1) / 2) for a in range(3)]


def affine(img, lab, A, out_size, dt):
    """-> (image trilinear with zeros outside, label nearest by round-half-to-even with 0 outside, the three source indices)."""
    img = img.astype(dt)
    S = img.shape
    src = source_index(A, out_size, S, dt)
    i0 = [np.floor(s) for s in src]
    fr = [s - i for s, i in zip(src, i0)]
    out = np.zeros(out_size, dt)
    for c in range(8):
        off = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
        idx = [(i + o).astype(np.int64) for i, o in zip(i0, off)]
        ok = np.ones(out_size, bool)
        w = np.ones(out_size, dt)
        for a in range(3):
            ok &= (idx[a] >= 0) & (idx[a] < S[a])
            w = w * (fr[a] if off[a] else 1 - fr[a])
        v = img[tuple(np.clip(i, 0, s - 1) for i, s in zip(idx, S))]
        out = out + np.where(ok, w * v, dt(0))
    nidx = [np.rint(s).astype(np.int64) for s in src]
    ok = np.ones(out_size, bool)
    for a in range(3):
        ok &= (nidx[a] >= 0) & (nidx[a] < S[a])
    olab = np.where(ok, lab[tuple(np.clip(i, 0, s - 1) for i, s in zip(nidx, S))], 0).astype(np.uint8)
    return out, olab, src


def half_integer_margin(src):
    """Per voxel the smallest distance of a source index from a half-integer over the three axes."""
    return np.minimum.reduce([np.abs(s - np.floor(s) - 0.5) for s in src])


def chain_sample(vol, lab, params, b, noise, dt, stop_after=None):
    """Sample b of the chain: crop, noise, bias, Gibbs, contrast, smooth, sharpen, affine, rescale.  ``vol`` is the resident
    (already rescaled) volume, ``noise`` the sample's standard-normal tensor.  -> (image, label uint8, source indices)."""
    on = {k: bool(params["on"][k][b]) for k in SWITCH_NAMES}
    crop_size = tuple(params["crop_size"])
    size = tuple(min(c, s) for c, s in zip(crop_size, vol.shape))
    x = crop(vol, params["corner"][b], size).astype(dt)
    y = crop(lab, params["corner"][b], size)
    if on["noise"]:
        x = x + f32(params["rand_std"][b], dt) * noise.astype(dt)
    if on["bias"]:
        x = x * np.exp(bias_exponent(size, params["coeff"][b], dt))
    if on["gibbs"]:
        x = gibbs(x, gibbs_radius(params["gibbs_alpha"][b], size), dt)
    if on["contrast"]:
        x = adjust_contrast(x, params["gamma"][b], dt)
    if on["smooth"]:
        x = gaussian(x, params["smooth_sigma"][b], dt)
    if on["sharpen"]:
        x = sharpen(x, params["sharpen_sigma1"][b], params["sharpen_sigma2"][b], params["sharpen_alpha"][b], dt)
    A = params["affine"][b] if on["affine"] else np.eye(3)
    x, y, src = affine(x, y, A, crop_size, dt)
    return scale_intensity(x, dt), y, src


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


def natural_key(s):
    import re
    return [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", s) if t != ""]


def describe_parser(parser):
    """What tests/golden/segtrain_cli.json records of an argparse parser: every flag with its help, and the exclusive groups."""
    import argparse
    flags = []
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        flags.append({"option_strings": list(a.option_strings), "dest": a.dest, "default": a.default, "required": bool(a.required),
                      "type": None if a.type is None else a.type.__name__, "nargs": a.nargs, "action": type(a).__name__, "help": a.help})
    groups = [{"required": bool(g.required), "dests": [a.dest for a in g._group_actions]} for g in parser._mutually_exclusive_groups]
    return {"flags": flags, "exclusive_groups": groups}
