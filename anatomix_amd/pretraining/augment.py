"""The two-view augmentation of the reference's pretraining loader (``H5SupCLDataset``, h5supcl_dataset.py:122-178, 260-303) on
the device, a pair at a time, on the kernels of csrc/amx_preaug.hip.  The reference runs TorchIO's transforms on whole volumes in
CPU workers; here the pair is moved to the GPU, the random parameters are drawn on the host (``draw_params``) and reach the kernels
through one small table, and every stage is one launch (the blur two) for both views.  Only the FFTs of the motion artefact are
``torch.fft``.

TorchIO is not a dependency.  Each transform is restated from TorchIO's documented algorithm (DESIGN.md section 4.16 has the
definitions); parity with an installed TorchIO is NOT pinned, and TorchIO's own random stream is not reproduced: ``draw_params`` has
one documented order of its own.

There is no host path: CPU tensors, other dtypes than float32 and more than one channel raise."""
from __future__ import annotations

import copy
import math

import numpy as np
import torch

from .. import _lib, _stream

SPATIAL, BLUR, NOISE, BIAS, GAMMA = 1, 2, 4, 8, 16
MAX_RADIUS = 8
INTENSITY_SWITCHES = (("blur", 0.33), ("noise", 0.33), ("bias", 0.5), ("gamma", 0.5), ("motion", 0.33))
FLIP_P, AFFINE_P, AFFINE_SCALES, AFFINE_DEGREES = 0.9, 0.5, 0.4, 45.0
BLUR_SIGMA, NOISE_STD, BIAS_COEFF, LOG_GAMMA = 2.0, 0.25, 0.5, 0.4
MOTION_DEGREES, MOTION_TRANSLATION, MOTION_TRANSFORMS = 10.0, 10.0, 2

# include/anatomix_amd.h: amx_preaug_view
VIEW_DTYPE = np.dtype([("flags", "<i4"), ("map", "<f4", (12,)), ("radius", "<i4", (3,)), ("taps", "<f4", (3, 17)), ("noise_std", "<f4"),
                       ("bias", "<f4", (20,)), ("gamma", "<f4")])
_IDENTITY_MAP = np.hstack([np.eye(3), np.zeros((3, 1))])


def _views(x, name="image"):
    """A contiguous float32 [views, D, H, W] device tensor (a [D, H, W] volume is one view), or an error: no host path, no conversion."""
    x = _stream.device_tensor(x, name, (torch.float32,), "augmentation")
    if x.dim() == 3:
        x = x[None]
    if x.dim() != 4:
        raise ValueError(f"{name}: [D, H, W] or the views stacked as [views, D, H, W], one channel each (got {tuple(x.shape)})")
    return x.contiguous()


def _volume(x, name, dtypes=(torch.float32,)):
    """One volume of a sample, [D, H, W] or [1, D, H, W], as a contiguous [D, H, W] device tensor."""
    x = _stream.device_tensor(x, name, dtypes, "augmentation")
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[0] != 1):
        raise ValueError(f"{name}: [D, H, W] or [1, D, H, W] with one channel (got {tuple(x.shape)})")
    return x.reshape(x.shape[-3:]).contiguous()


def _per_view(v, n, shape, name):
    return _stream.per_row(v, (n,) + tuple(shape), name, f"shape {tuple(shape)} or one per view of the {n}", got="got")


class _Table(_stream.RecordTable):
    """The per-view records of one pair."""
    DTYPE, STRUCT, SIZE_SYMBOL = VIEW_DTYPE, "amx_preaug_view", "amx_preaug_view_bytes"
    DEFAULTS = {"map": _IDENTITY_MAP.reshape(12), "gamma": 1.0}


# ---- parameters -----------------------------------------------------------------------------------------------------------------

def rotation(degrees):
    """R = Rz Rx Ry (float64): the rotations by ``degrees`` about spatial axis 2, axis 0 and axis 1."""
    a0, a1, a2 = (math.radians(float(v)) for v in degrees)
    Rx = np.array([[1, 0, 0], [0, math.cos(a0), -math.sin(a0)], [0, math.sin(a0), math.cos(a0)]])
    Ry = np.array([[math.cos(a1), 0, math.sin(a1)], [0, 1, 0], [-math.sin(a1), 0, math.cos(a1)]])
    Rz = np.array([[math.cos(a2), -math.sin(a2), 0], [math.sin(a2), math.cos(a2), 0], [0, 0, 1]])
    return Rz @ Rx @ Ry


def spatial_map(shape, flip_axes=(False, False, False), scales=None, degrees=None):
    """The 3 x 4 map (float64) from an output voxel to its source index for RandomFlip followed by RandomAffine.
    Affine: F(p) = c + R diag(s) (p - c) with c = (shape - 1) / 2, the output voxel o samples F^-1(o); flip of axis a: index n_a - 1 - q.
    ``scales`` / ``degrees`` None: no affine."""
    c = (np.asarray(shape, np.float64) - 1.0) / 2.0
    A = np.eye(3) if scales is None else np.diag(1.0 / np.asarray(scales, np.float64)) @ rotation(degrees).T
    t = c - A @ c
    flip = np.asarray(flip_axes, bool)
    D = np.diag(np.where(flip, -1.0, 1.0))
    f = np.where(flip, np.asarray(shape, np.float64) - 1.0, 0.0)
    return np.hstack([D @ A, (D @ t + f)[:, None]])


def rigid_map(shape, degrees, translation):
    """The 3 x 4 map of a rigid move about the centre: F(p) = c + R (p - c) + t in voxels, the output voxel o samples F^-1(o)."""
    c = (np.asarray(shape, np.float64) - 1.0) / 2.0
    Rt = rotation(degrees).T
    return np.hstack([Rt, (c - Rt @ (c + np.asarray(translation, np.float64)))[:, None]])


def gaussian_taps(sigma):
    """scipy.ndimage's ``_gaussian_kernel1d(sigma, 0, radius)`` with ``radius = int(4 sigma + 0.5)``: (radius, float64 taps that sum to
    1).  sigma <= 1e-15: (0, [1]), the axis gaussian_filter skips."""
    sigma = float(sigma)
    if not sigma >= 0.0 or math.isinf(sigma):
        raise ValueError(f"sigma must be finite and non-negative (got {sigma})")
    if sigma <= 1e-15:
        return 0, np.ones(1)
    r = int(4.0 * sigma + 0.5)
    k = np.arange(-r, r + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return r, phi / phi.sum()


def _flag(opt, name, default=True):
    return bool(getattr(opt, name, default))


def draw_params(rng, shape, opt):
    """Everything the reference's augmentation randomises for one pair of views of ``shape`` (D, H, W), from a
    ``numpy.random.RandomState``.  ``opt`` carries the reference's flags (``geo_augment, inten_augment, blur, noise, bias, gamma, motion``,
    True when absent as in base_options.py; ``apply_same_inten_augment``, False when absent; ``crop_size``; ``isTrain``).

    The draw order is this function's own (TorchIO's stream is not reproduced).  Every number is drawn whether or not its switch is on:
      1. flip: ``uniform()`` (acts when < 0.9), then ``uniform(size=3)`` (axis a flips when < 0.5);
      2. affine: ``uniform()`` (on when < 0.5), scales U(0.6, 1.4) x 3, degrees U(-45, 45) x 3;
      3. per view, A then B, per transform in chain order one ``uniform()`` for its switch (on when below 0.33, 0.33, 0.5, 0.5, 0.33)
         directly followed by its parameters: blur sigma U(0, 2) x 3; noise std U(0, 0.25) and ``noise_seed = randint(0, 2**31 - 1)``;
         bias 20 coefficients U(-0.5, 0.5); gamma ``log_gamma`` U(-0.4, 0.4); motion degrees U(-10, 10) [2, 3], translation
         U(-10, 10) [2, 3], time offsets U(-0.1, 0.1) x 2 (the times are (i + 1) / 3 + offset);
         with ``apply_same_inten_augment`` view B's record is then replaced by a copy of view A's, noise seed included;
      4. the crop (``crop_size > 0`` and ``isTrain``): per axis in axis order, only where the axis is longer than the window of
         2 (crop_size // 2), ``randint(half, extent - half)`` for the centre.
    Returns a dict; ``map`` [3, 4] is the folded flip + affine (None when neither is on), ``views`` the two intensity records."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3:
        raise ValueError(f"shape: (D, H, W) (got {shape})")
    geo = _flag(opt, "geo_augment")
    inten = _flag(opt, "inten_augment")
    p = dict(shape=shape)
    p["flip_on"] = bool(rng.uniform() < FLIP_P) and geo
    p["flip_axes"] = (rng.uniform(size=3) < 0.5) & p["flip_on"]
    p["affine_on"] = bool(rng.uniform() < AFFINE_P) and geo
    p["scales"] = rng.uniform(1.0 - AFFINE_SCALES, 1.0 + AFFINE_SCALES, 3)
    p["degrees"] = rng.uniform(-AFFINE_DEGREES, AFFINE_DEGREES, 3)
    views = []
    for _ in range(2):
        v = dict(on={})
        for name, prob in INTENSITY_SWITCHES:
            v["on"][name] = bool(rng.uniform() < prob) and inten and _flag(opt, name)
            if name == "blur":
                v["sigma"] = rng.uniform(0.0, BLUR_SIGMA, 3)
            elif name == "noise":
                v["noise_std"] = float(rng.uniform(0.0, NOISE_STD))
                v["noise_seed"] = int(rng.randint(0, 2 ** 31 - 1))
            elif name == "bias":
                v["coeff"] = rng.uniform(-BIAS_COEFF, BIAS_COEFF, 20)
            elif name == "gamma":
                v["gamma"] = float(np.exp(rng.uniform(-LOG_GAMMA, LOG_GAMMA)))
            else:
                v["motion_degrees"] = rng.uniform(-MOTION_DEGREES, MOTION_DEGREES, (MOTION_TRANSFORMS, 3))
                v["motion_translation"] = rng.uniform(-MOTION_TRANSLATION, MOTION_TRANSLATION, (MOTION_TRANSFORMS, 3))
                v["motion_times"] = (np.arange(1, MOTION_TRANSFORMS + 1) / (MOTION_TRANSFORMS + 1.0)
                                     + rng.uniform(-0.1, 0.1, MOTION_TRANSFORMS))
        views.append(v)
    if _flag(opt, "apply_same_inten_augment", False):
        views[1] = copy.deepcopy(views[0])
    p["views"] = views
    p["map"] = (spatial_map(shape, p["flip_axes"], p["scales"] if p["affine_on"] else None, p["degrees"])
                if (p["flip_axes"].any() or p["affine_on"]) else None)
    crop = int(getattr(opt, "crop_size", 0) or 0)
    p["crop_size"], p["crop_start"] = 0, None
    if crop > 0 and _flag(opt, "isTrain"):
        half = crop // 2
        p["crop_size"] = crop
        p["crop_start"] = tuple((int(rng.randint(half, n - half)) if n > 2 * half else half) - half for n in shape)
    return p


# ---- the stages on the stacked views --------------------------------------------------------------------------------------------

def _minmax(x):
    return _stream.minmax(x)       # amx_segaug_minmax as it stands: one row per view


def _spatial(x, lab, table, mm):
    n, d, h, w = x.shape
    out = torch.empty_like(x)
    olab = None if lab is None else torch.empty_like(lab)
    _lib.check_envelope(_lib.load().amx_preaug_spatial(_lib.ptr(x), _lib.ptr(lab), n, d, h, w, _lib.ptr(mm), _lib.ptr(out), _lib.ptr(olab),
                        *table.args, _lib.stream(x.device)))
    return out, olab


def _blur(x, table):
    n, d, h, w = x.shape
    out, tmp = torch.empty_like(x), torch.empty_like(x)
    _lib.check_envelope(_lib.load().amx_preaug_blur(_lib.ptr(x), _lib.ptr(out), _lib.ptr(tmp), n, d, h, w, *table.args, _lib.stream(x.device)))
    return out


def _intensity(x, noise, out, table):
    n, d, h, w = x.shape
    _lib.check_envelope(_lib.load().amx_preaug_intensity(_lib.ptr(x), _lib.ptr(noise), _lib.ptr(out), n, d, h, w, *table.args,
                        _lib.stream(x.device)))
    return out


def _set_taps(table, sigmas):
    """sigmas [views, 3] -> radius and taps.  A radius above the envelope is recorded as it is (the entry refuses it when the view's
    switch is on) and its taps are left out."""
    for v in range(sigmas.shape[0]):
        for a in range(3):
            r, taps = gaussian_taps(sigmas[v, a])
            table.host["radius"][v, a] = r
            if r <= MAX_RADIUS:
                table.host["taps"][v, a, :2 * r + 1] = taps


# ---- one public function per transform ------------------------------------------------------------------------------------------

def flip_affine(img, seg=None, flip_axes=(False, False, False), scales=None, degrees=None, matrix=None):
    """RandomFlip then RandomAffine with given parameters, in one launch for every view of ``img`` ([views, D, H, W] or [D, H, W]) and
    the label map ``seg`` (uint8 [D, H, W], optional) they share.  ``matrix``: the 3 x 4 map itself instead of flip / scales / degrees
    (see ``spatial_map``).  Image: trilinear, padded with the view's minimum; label: nearest.  Returns (image, label or None)."""
    x = _views(img)
    lab = None if seg is None else _volume(seg, "seg", (torch.uint8,))
    if lab is not None and (lab.device != x.device or lab.shape != x.shape[1:]):
        raise ValueError(f"seg {tuple(lab.shape)} on {lab.device} does not match the image {tuple(x.shape[1:])} on {x.device}")
    if matrix is not None:
        if scales is not None or degrees is not None or any(flip_axes):
            raise ValueError("flip_affine: a matrix, or flip_axes / scales / degrees, not both")
        M = np.asarray(matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else matrix, np.float64)
        if M.shape != (3, 4):
            raise ValueError(f"matrix: [3, 4] (got {M.shape})")
    else:
        if (scales is None) != (degrees is None):
            raise ValueError("flip_affine: scales and degrees come together")
        M = spatial_map(x.shape[1:], flip_axes, scales, degrees)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["map"] = SPATIAL, M.reshape(12)
        return _spatial(x, lab, t.device(x.device), _minmax(x))


def blur(img, sigma):
    """RandomBlur's arithmetic: ``scipy.ndimage.gaussian_filter(x, sigma)`` (truncate 4, mode 'reflect') per view; ``sigma`` a scalar,
    per axis, or [views, 3]; sigma <= 2."""
    x = _views(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"] = BLUR
        _set_taps(t, _per_view(sigma, x.shape[0], (3,), "sigma"))
        return _blur(x, t.device(x.device))


def add_noise(img, std, noise):
    """RandomNoise's arithmetic: img + std * noise, ``noise`` a standard-normal tensor of img's shape, ``std`` per view."""
    x, nz = _views(img), _views(noise, "noise")
    if nz.shape != x.shape or nz.device != x.device:
        raise ValueError(f"noise {tuple(nz.shape)} does not match the image {tuple(x.shape)}")
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["noise_std"] = NOISE, _per_view(std, x.shape[0], (), "std")
        return _intensity(x, nz, torch.empty_like(x), t.device(x.device))


def bias_field(img, coeff, order=3):
    """RandomBiasField's arithmetic: img * exp(f), f = sum c_ijk z^i y^j x^k over i + j + k <= 3 ((i, j, k) lexicographic, i along the
    first spatial axis) over linspace(-1, 1, size) per axis; ``coeff`` [20] or [views, 20]."""
    if order != 3:
        raise NotImplementedError(f"bias_field: order = 3 (got {order})")
    x = _views(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["bias"] = BIAS, _per_view(coeff, x.shape[0], (20,), "coeff")
        return _intensity(x, None, torch.empty_like(x), t.device(x.device))


def gamma(img, gamma):
    """RandomGamma's arithmetic: sign(x) |x|^gamma with the exponent ``gamma`` (= exp(log_gamma)) per view."""
    x = _views(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["gamma"] = GAMMA, _per_view(gamma, x.shape[0], (), "gamma")
        return _intensity(x, None, torch.empty_like(x), t.device(x.device))


def _motion_one(x, degrees, translation, times):
    """One volume [D, H, W].  The k-space masks depend on the last-axis frequency only, so the transforms over the other two axes
    cancel and complex 1-D FFTs along W compose the same result as the 3-D definition."""
    degrees, translation = np.asarray(degrees, np.float64), np.asarray(translation, np.float64)
    times = np.asarray(times, np.float64)
    if degrees.shape != (MOTION_TRANSFORMS, 3) or translation.shape != (MOTION_TRANSFORMS, 3) or times.shape != (MOTION_TRANSFORMS,):
        raise ValueError(f"motion: degrees and translation [{MOTION_TRANSFORMS}, 3], times [{MOTION_TRANSFORMS}]")
    W = x.shape[-1]
    cuts = [int(t * W) for t in times]
    if not 0 <= cuts[0] <= cuts[1] <= W:
        raise ValueError(f"motion: times must be ascending inside [0, 1] (got {times.tolist()})")
    mm = _minmax(x[None])
    k = torch.fft.fftshift(torch.fft.fft(x, dim=-1), dim=-1)
    bounds = cuts + [W]
    for i in range(MOTION_TRANSFORMS):
        t = _Table(1)
        t.host["flags"], t.host["map"] = SPATIAL, rigid_map(x.shape, degrees[i], translation[i]).reshape(12)
        moved, _ = _spatial(x[None], None, t.device(x.device), mm)
        lo, hi = bounds[i], bounds[i + 1]
        if hi > lo:
            k[..., lo:hi] = torch.fft.fftshift(torch.fft.fft(moved[0], dim=-1), dim=-1)[..., lo:hi]
    return torch.fft.ifft(torch.fft.ifftshift(k, dim=-1), dim=-1).real.contiguous()


def motion(img, degrees, translation, times):
    """RandomMotion(num_transforms=2)'s arithmetic on one volume [D, H, W] (or [1, D, H, W]): ``degrees`` and ``translation`` [2, 3]
    (voxels), ``times`` [2] in (0, 1).  The two rigid moves are the spatial kernel; the FFTs are torch.fft on the device.  TorchIO's
    de-meaning of the transforms is not reproduced."""
    x = _views(img)
    if x.shape[0] != 1:
        raise ValueError(f"motion: one volume (got {tuple(x.shape)})")
    with torch.cuda.device(x.device):
        return _motion_one(x[0], degrees, translation, times).view(img.shape)


# ---- the chain ------------------------------------------------------------------------------------------------------------------

def build_table(params):
    """The host table of one pair from ``draw_params``' dict (or one with the same keys)."""
    t = _Table(2)
    h = t.host
    M = params.get("map")
    for v, rec in enumerate(params["views"]):
        on = rec["on"]
        h["flags"][v] = ((SPATIAL if M is not None else 0) | (BLUR if on["blur"] else 0) | (NOISE if on["noise"] else 0)
                         | (BIAS if on["bias"] else 0) | (GAMMA if on["gamma"] else 0))
        h["noise_std"][v], h["bias"][v], h["gamma"][v] = rec["noise_std"], rec["coeff"], rec["gamma"]
    if M is not None:
        h["map"] = np.asarray(M, np.float64).reshape(12)
    _set_taps(t, np.asarray([rec["sigma"] for rec in params["views"]], np.float64))
    return t


def augment_pair(A, B, seg, params, crop_size=0, noise=None):
    """The reference's chain on one pair: flip + affine of both views and the label, then per view blur, noise, bias field, gamma and
    motion, then the crop.  ``A``, ``B``: float32 device tensors [D, H, W] or [1, D, H, W]; ``seg``: their label map, uint8 or float32
    (values 0 .. 255); ``params``: ``draw_params``' dict for this shape.  ``crop_size > 0`` cuts the window that ``params`` drew for that
    size.  ``noise``: the standard-normal tensor [2, D, H, W] of the noise stage; None draws each view's ``torch.randn`` from
    ``torch.Generator(device).manual_seed(noise_seed)`` of its record.
    Returns the four tensors of the reference's sample, (A, B, A_seg, B_seg), each [1, d, h, w] float32 on the device.  A stage that
    neither view has on is not launched; nothing is read back from the device."""
    a, b = _volume(A, "A"), _volume(B, "B")
    lab = _volume(seg, "seg", (torch.uint8, torch.float32))
    dev = a.device
    if b.device != dev or lab.device != dev:
        raise ValueError("augment_pair: A, B and seg must be on one device")
    if a.shape != b.shape or a.shape != lab.shape:
        raise ValueError(f"augment_pair: A {tuple(a.shape)}, B {tuple(b.shape)} and seg {tuple(lab.shape)} must share one shape")
    if tuple(params["shape"]) != tuple(a.shape):
        raise ValueError(f"augment_pair: the parameters were drawn for {tuple(params['shape'])}, the volumes are {tuple(a.shape)}")
    crop_size = int(crop_size)
    if crop_size > 0 and params.get("crop_size") != crop_size:
        raise ValueError(f"augment_pair: crop_size {crop_size}, but the parameters drew the window of {params.get('crop_size')}")
    recs = params["views"]
    with torch.cuda.device(dev):
        if lab.dtype != torch.uint8:
            lab = lab.to(torch.uint8)
        x = torch.stack([a, b])
        table = build_table(params).device(dev)                     # the one copy of the pair's parameters
        if params.get("map") is not None:
            x, lab = _spatial(x, lab, table, _minmax(x))
        if any(r["on"]["blur"] for r in recs):
            x = _blur(x, table)
        if any(r["on"][k] for r in recs for k in ("noise", "bias", "gamma")):
            nz = None
            if noise is not None:
                nz = _views(noise, "noise")
                if nz.shape != x.shape:
                    raise ValueError(f"noise: {tuple(x.shape)} (got {tuple(nz.shape)})")
            elif any(r["on"]["noise"] for r in recs):
                nz = torch.empty_like(x)
                for v, r in enumerate(recs):
                    if r["on"]["noise"]:
                        nz[v] = torch.randn(x.shape[1:], generator=torch.Generator(dev).manual_seed(int(r["noise_seed"])), device=dev,
                                            dtype=torch.float32)
            x = _intensity(x, nz, x, table)                         # in place: x is this function's own stack
        for v, r in enumerate(recs):
            if r["on"]["motion"]:
                x[v] = _motion_one(x[v], r["motion_degrees"], r["motion_translation"], r["motion_times"])
        if crop_size > 0:
            half = crop_size // 2
            win = tuple(slice(s, s + 2 * half) for s in params["crop_start"])
            x, lab = x[(slice(None),) + win], lab[win]
        segf = lab.float()[None].contiguous()
        return x[0][None].contiguous(), x[1][None].contiguous(), segf, segf.clone()
