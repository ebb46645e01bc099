"""The augmentation chain of the reference's segmentation finetuning (``get_train_transforms``, segmentation_utils.py:159-216)
on the device, a batch at a time, on the kernels of csrc/amx_segaug.hip.  The reference runs MONAI's transforms per sample in CPU
workers; here the few training volumes stay resident on the GPU, the per-sample random parameters are drawn on the host
(``draw_params``) and reach the kernels through one small table copied once per batch, and every stage is one launch for the
whole batch.  Only the two FFTs of the Gibbs transform are ``torch.fft``.

MONAI is not a dependency.  Each transform is restated from MONAI's documented algorithm (DESIGN.md section 4.15 has the
definitions); parity with an installed MONAI is NOT pinned, and the order in which MONAI's own random state is consumed depends on
its version and is not reproduced: ``draw_params`` has one documented order of its own.

There is no host path: CPU tensors, other dtypes than float32 and more than one channel raise."""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import _lib, _stream

NOISE, BIAS, GIBBS, CONTRAST, SMOOTH, SHARPEN, AFFINE, RESCALE = 1, 2, 4, 8, 16, 32, 64, 128
SWITCHES = (("noise", NOISE, 0.33), ("bias", BIAS, 0.33), ("gibbs", GIBBS, 0.33), ("contrast", CONTRAST, 0.33),
            ("smooth", SMOOTH, 0.33), ("sharpen", SHARPEN, 0.33), ("affine", AFFINE, 0.98))
MAX_RADIUS = 4
_OP_SCALE, _OP_CONTRAST = 0, 1
_GAUSS_SMOOTH, _GAUSS_SHARPEN = 0, 1

# include/anatomix_amd.h: amx_segaug_sample
SAMPLE_DTYPE = np.dtype([("vol", "<u8"), ("lab", "<u8"), ("flags", "<i4"), ("vol_dim", "<i4", (3,)), ("corner", "<i4", (3,)),
                         ("noise_std", "<f4"), ("bias", "<f4", (20,)), ("gibbs_r", "<f4"), ("gamma", "<f4"),
                         ("radius", "<i4", (3, 3)), ("taps", "<f4", (3, 3, 9)), ("sharpen_alpha", "<f4"), ("affine", "<f4", (9,))])
_GIBBS_R_WORD = SAMPLE_DTYPE.fields["gibbs_r"][1] // 4


def _image(x, name="image"):
    """A contiguous float32 [B, 1, D, H, W] device tensor, or an error: there is no host path and no conversion."""
    x = _stream.device_tensor(x, name, (torch.float32,), "augmentation")
    if x.dim() != 5 or x.shape[1] != 1:
        raise ValueError(f"{name}: [B, 1, D, H, W] with one channel (got {tuple(x.shape)})")
    return x.contiguous()


def _label(y, like, name="label"):
    if not isinstance(y, torch.Tensor) or not y.is_cuda or y.device != like.device:
        raise RuntimeError(f"{name}: a tensor on the image's device")
    if y.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"{name}: float32 or uint8 (got {y.dtype})")
    if y.dim() != 5 or y.shape[1] != 1:
        raise ValueError(f"{name}: [B, 1, D, H, W] with one channel (got {tuple(y.shape)})")
    return y.contiguous()


def _per_sample(v, B, width=None, name="parameter"):
    """A float64 array [B] (or [B, width]) from a scalar, one row, or one entry per sample."""
    return _stream.per_row(v, (B,) if width is None else (B, width), name,
                           f"a scalar, {'' if width is None else f'{width} values, '}or one per sample of the batch of {B}")


class _Table(_stream.RecordTable):
    """The per-sample records of one batch."""
    DTYPE, STRUCT, SIZE_SYMBOL = SAMPLE_DTYPE, "amx_segaug_sample", "amx_segaug_sample_bytes"
    DEFAULTS = {"affine": np.eye(3, dtype=np.float32).reshape(9), "gamma": 1.0}


def gaussian_taps(sigma):
    """MONAI's ``gaussian_1d(sigma, truncated=4, approx="erf")``: (tail, taps [2 tail + 1]) with tail = int(max(4 sigma, 0.5) + 0.5) and
    tap(x) = max(0.5 (erf(t (x + 0.5)) - erf(t (x - 0.5))), 0), t = 0.70710678 / sigma.  Not renormalised; sigma = 0 is the identity."""
    sigma = float(sigma)
    if not sigma >= 0.0 or math.isinf(sigma):
        raise ValueError(f"sigma must be finite and non-negative (got {sigma})")
    tail = int(max(4.0 * sigma, 0.5) + 0.5)
    if sigma == 0.0:
        return tail, [1.0 if x == 0 else 0.0 for x in range(-tail, tail + 1)]
    t = 0.70710678 / sigma
    return tail, [max(0.5 * (math.erf(t * (x + 0.5)) - math.erf(t * (x - 0.5))), 0.0) for x in range(-tail, tail + 1)]


def _set_taps(table, filt, sigmas):
    """sigmas [B, 3] -> radius and taps of filter ``filt``.  A radius above the envelope is recorded as it is (the entry refuses it
    when the sample's switch is on) and its taps are left out."""
    for b in range(sigmas.shape[0]):
        for a in range(3):
            r, taps = gaussian_taps(sigmas[b, a])
            table.host["radius"][b, filt, a] = r
            if r <= MAX_RADIUS:
                table.host["taps"][b, filt, a, :2 * r + 1] = taps


def gibbs_radius(alpha, shape):
    """r = (1 - alpha) max(shape) sqrt(2) / 2, rounded to float32: the value the mask is built from on every route."""
    return np.float32((1.0 - float(alpha)) * max(shape) * math.sqrt(2.0) / 2.0)


def affine_matrix(rotate=(0.0, 0.0, 0.0), shear=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0)):
    """A = Rx Ry Rz Shear Scale (3 x 3, float64) with MONAI's ``create_rotate`` matrices about the three spatial axes, the three shear
    values at [0, 1], [0, 2], [1, 0] and ``scale`` on the diagonal."""
    rx, ry, rz = (float(v) for v in rotate)
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    Sh = np.eye(3)
    Sh[0, 1], Sh[0, 2], Sh[1, 0] = (float(v) for v in shear)
    return Rx @ Ry @ Rz @ Sh @ np.diag([float(v) for v in scale])


def draw_params(rng, crop_size, volume_shapes, batch):
    """Everything ``get_train_transforms(crop_size)`` randomises, for one batch, from a ``numpy.random.RandomState``.

    ``volume_shapes``: the (D, H, W) of the volume each of the ``batch`` samples is cropped from.  The draw order is this
    function's own (MONAI's depends on its version and is not reproduced).  Per sample, in batch order:
      1. the crop corner, ``randint(0, dim - min(crop, dim) + 1)`` per axis;
      2. per transform in chain order (noise, bias, Gibbs, contrast, smooth, sharpen, affine) one ``uniform()`` for its switch (on when
         below ``prob``: 0.33, and 0.98 for the affine), directly followed by its parameters, which are drawn whether it is on or not:
         noise ``rand_std`` U(0, 0.1); bias 20 coefficients U(0, 0.05); Gibbs ``alpha`` U(0, 0.33); contrast ``gamma`` U(0.5, 4.5);
         smooth ``sigma`` U(0, 0.1) x 3; sharpen ``sigma1`` U(0.5, 1) x 3, then ``sigma2`` U(0.5, sigma1) x 3, then ``alpha`` U(10, 30);
         affine rotation U(-pi/4, pi/4) x 3, shear U(-0.2, 0.2) x 3, scale 1 + U(-0.2, 0.2) x 3.
    After the last sample: ``noise_seed = randint(0, 2**31 - 1)``.
    Returns a dict of arrays with the batch in front; ``affine`` [B, 3, 3] is the identity where the affine is off."""
    if len(volume_shapes) != batch:
        raise ValueError(f"volume_shapes: one shape per sample of the batch of {batch} (got {len(volume_shapes)})")
    crop = (int(crop_size),) * 3 if np.isscalar(crop_size) else tuple(int(c) for c in crop_size)
    p = dict(crop_size=crop, corner=np.zeros((batch, 3), np.int64), volume_shape=np.asarray(volume_shapes, np.int64).reshape(batch, 3),
             on={k: np.zeros(batch, bool) for k, _, _ in SWITCHES}, rand_std=np.zeros(batch), coeff=np.zeros((batch, 20)),
             gibbs_alpha=np.zeros(batch), gamma=np.zeros(batch), smooth_sigma=np.zeros((batch, 3)), sharpen_sigma1=np.zeros((batch, 3)),
             sharpen_sigma2=np.zeros((batch, 3)), sharpen_alpha=np.zeros(batch), rotate=np.zeros((batch, 3)), shear=np.zeros((batch, 3)),
             scale=np.zeros((batch, 3)), affine=np.zeros((batch, 3, 3)))
    prob = {k: pr for k, _, pr in SWITCHES}
    for b in range(batch):
        for a in range(3):
            dim = int(p["volume_shape"][b, a])
            p["corner"][b, a] = rng.randint(0, dim - min(crop[a], dim) + 1)
        p["on"]["noise"][b] = rng.uniform() < prob["noise"]
        p["rand_std"][b] = rng.uniform(0.0, 0.1)
        p["on"]["bias"][b] = rng.uniform() < prob["bias"]
        p["coeff"][b] = rng.uniform(0.0, 0.05, 20)
        p["on"]["gibbs"][b] = rng.uniform() < prob["gibbs"]
        p["gibbs_alpha"][b] = rng.uniform(0.0, 0.33)
        p["on"]["contrast"][b] = rng.uniform() < prob["contrast"]
        p["gamma"][b] = rng.uniform(0.5, 4.5)
        p["on"]["smooth"][b] = rng.uniform() < prob["smooth"]
        p["smooth_sigma"][b] = rng.uniform(0.0, 0.1, 3)
        p["on"]["sharpen"][b] = rng.uniform() < prob["sharpen"]
        p["sharpen_sigma1"][b] = rng.uniform(0.5, 1.0, 3)
        p["sharpen_sigma2"][b] = [rng.uniform(0.5, s1) for s1 in p["sharpen_sigma1"][b]]
        p["sharpen_alpha"][b] = rng.uniform(10.0, 30.0)
        p["on"]["affine"][b] = rng.uniform() < prob["affine"]
        p["rotate"][b] = rng.uniform(-math.pi / 4, math.pi / 4, 3)
        p["shear"][b] = rng.uniform(-0.2, 0.2, 3)
        p["scale"][b] = 1.0 + rng.uniform(-0.2, 0.2, 3)
        p["affine"][b] = affine_matrix(p["rotate"][b], p["shear"][b], p["scale"][b]) if p["on"]["affine"][b] else np.eye(3)
    p["noise_seed"] = int(rng.randint(0, 2 ** 31 - 1))
    return p


# ---- the stages on a batch ------------------------------------------------------------------------------------------------

def _minmax(x, scratch=None):
    return _stream.minmax(x, scratch)


def _pointwise(x, out, mm, op, table):
    _lib.check_envelope(_lib.load().amx_segaug_pointwise(_lib.ptr(x), _lib.ptr(out), x.shape[0], x[0].numel(), _lib.ptr(mm), op,
                        *table.args, _lib.stream(x.device)))
    return out


def _crop(table, B, size, noise, label_dtype, dev):
    img = torch.empty((B, 1) + tuple(size), dtype=torch.float32, device=dev)
    lab = torch.empty((B, 1) + tuple(size), dtype=torch.uint8, device=dev)
    _lib.check_envelope(_lib.load().amx_segaug_crop(B, *size, _lib.ptr(noise), _lib.SEG_LABEL[str(label_dtype).split(".")[1]],
                        _lib.ptr(img), _lib.ptr(lab), *table.args, _lib.stream(dev)))
    return img, lab


def _gaussian(x, mode, table):
    B, _, d, h, w = x.shape
    out = torch.empty_like(x)
    tmp = torch.empty((2,) + tuple(x.shape), dtype=torch.float32, device=x.device)
    _lib.check_envelope(_lib.load().amx_segaug_gaussian(_lib.ptr(x), _lib.ptr(out), _lib.ptr(tmp), B, d, h, w, mode, *table.args,
                        _lib.stream(x.device)))
    return out


def _gibbs_mask_grid(shape, dev, _cache={}):
    """4 x the squared distance of every k-space voxel from the centre (shape - 1) / 2: an exact integer, as float64."""
    key = (tuple(shape), str(dev))
    if key not in _cache:
        ax = [(2.0 * torch.arange(n, dtype=torch.float64, device=dev) - (n - 1)) ** 2 for n in shape]
        _cache.clear()
        _cache[key] = ax[0].view(-1, 1, 1) + ax[1].view(1, -1, 1) + ax[2].view(1, 1, -1)
    return _cache[key]


def _gibbs(x, which, table):
    """In place on the samples ``which`` (host indices; the others are not touched): k = fftshift(fftn(x)); k *= (distance from the
    centre <= r); x = real(ifftn(ifftshift(k))).  r is read from the device copy of the table."""
    if not which:
        return x
    dims = (-3, -2, -1)
    idx = torch.as_tensor(which, device=x.device)
    r = table.dev.view(torch.float32).view(x.shape[0], -1)[:, _GIBBS_R_WORD].index_select(0, idx).double()
    mask = _gibbs_mask_grid(x.shape[2:], x.device).unsqueeze(0) <= (4.0 * r * r).view(-1, 1, 1, 1)
    sub = x.index_select(0, idx)
    k = torch.fft.fftshift(torch.fft.fftn(sub, dim=dims), dim=dims) * mask.unsqueeze(1)
    x.index_copy_(0, idx, torch.fft.ifftn(torch.fft.ifftshift(k, dim=dims), dim=dims).real.contiguous())
    return x


def _affine(img, lab, size, table):
    B = img.shape[0]
    lib = _lib.load()
    out = torch.empty((B, 1) + tuple(size), dtype=torch.float32, device=img.device)
    olab = torch.empty((B, 1) + tuple(size), dtype=torch.uint8, device=img.device)
    nb = lib.amx_segaug_scratch_bytes(B, out[0].numel())
    sc = _lib.scratch(nb, img.device)
    _lib.check_envelope(lib.amx_segaug_affine(_lib.ptr(img), _lib.ptr(lab), B, *img.shape[2:], _lib.ptr(out), _lib.ptr(olab), *size,
                        *table.args, _lib.ptr(sc), nb, _lib.stream(img.device)))
    return out, olab, sc, nb


# ---- one public function per transform (MONAI's parameter names) ------------------------------------------------------------

def scale_intensity(img):
    """ScaleIntensity(minv=0, maxv=1) per sample: (x - min) / (max - min); x * 0 when min == max."""
    x = _image(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"] = RESCALE
        return _pointwise(x, torch.empty_like(x), _minmax(x), _OP_SCALE, t.device(x.device))


def _crop_whole(x, t, noise):
    """The crop stage over whole samples of ``x`` (corner 0): the route of the stand-alone noise and bias transforms."""
    B = x.shape[0]
    lab = torch.zeros((B,) + tuple(x.shape[2:]), dtype=torch.uint8, device=x.device)
    for b in range(B):
        t.host["vol"][b], t.host["lab"][b] = x[b].data_ptr(), lab[b].data_ptr()
        t.host["vol_dim"][b] = x.shape[2:]
    return _crop(t.device(x.device), B, x.shape[2:], noise, torch.uint8, x.device)[0]


def gaussian_noise(img, std, noise):
    """RandGaussianNoise's arithmetic: img + std * noise, ``noise`` a standard-normal tensor of img's shape, ``std`` per sample."""
    x, nz = _image(img), _image(noise, "noise")
    if nz.shape != x.shape:
        raise ValueError(f"noise {tuple(nz.shape)} does not match the image {tuple(x.shape)}")
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["noise_std"] = NOISE, _per_sample(std, x.shape[0], name="std")
        return _crop_whole(x, t, nz)


def bias_field(img, coeff, degree=3):
    """RandBiasField's arithmetic: img * exp(f), f the Legendre field of ``coeff`` ([20] or [B, 20]; (i, j, k) with i + j + k <= 3 in
    lexicographic order, i along the first spatial axis) over linspace(-1, 1, size) per axis."""
    if degree != 3:
        raise NotImplementedError(f"bias_field: degree = 3 (got {degree})")
    x = _image(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["bias"] = BIAS, _per_sample(coeff, x.shape[0], 20, name="coeff")
        return _crop_whole(x, t, None)


def gibbs_noise(img, alpha):
    """GibbsNoise(alpha): a centred sphere of radius (1 - alpha) max(shape) sqrt(2) / 2 of k-space is kept.  torch.fft on the device."""
    x = _image(img).clone()
    B = x.shape[0]
    with torch.cuda.device(x.device):
        t = _Table(B)
        t.host["flags"] = GIBBS
        t.host["gibbs_r"] = [gibbs_radius(a, x.shape[2:]) for a in _per_sample(alpha, B, name="alpha")]
        return _gibbs(x, list(range(B)), t.device(x.device))


def adjust_contrast(img, gamma):
    """AdjustContrast(gamma): ((x - min) / (range + 1e-7)) ** gamma * range + min per sample."""
    x = _image(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"], t.host["gamma"] = CONTRAST, _per_sample(gamma, x.shape[0], name="gamma")
        return _pointwise(x, torch.empty_like(x), _minmax(x), _OP_CONTRAST, t.device(x.device))


def gaussian_smooth(img, sigma):
    """GaussianSmooth(sigma, approx="erf"): separable, zero padding, ``sigma`` a scalar, per axis, or [B, 3]; sigma <= 1."""
    x = _image(img)
    with torch.cuda.device(x.device):
        t = _Table(x.shape[0])
        t.host["flags"] = SMOOTH
        _set_taps(t, 0, _per_sample(sigma, x.shape[0], 3, name="sigma"))
        return _gaussian(x, _GAUSS_SMOOTH, t.device(x.device))


def gaussian_sharpen(img, sigma1=3.0, sigma2=1.0, alpha=30.0):
    """GaussianSharpen(sigma1, sigma2, alpha): b = G_sigma1(img), b + alpha (b - G_sigma2(b)).  MONAI's defaults are kept, but
    sigma <= 1 is the envelope (what RandGaussianSharpen draws), so the default sigma1 raises."""
    x = _image(img)
    B = x.shape[0]
    with torch.cuda.device(x.device):
        t = _Table(B)
        t.host["flags"], t.host["sharpen_alpha"] = SHARPEN, _per_sample(alpha, B, name="alpha")
        _set_taps(t, 1, _per_sample(sigma1, B, 3, name="sigma1"))
        _set_taps(t, 2, _per_sample(sigma2, B, 3, name="sigma2"))
        return _gaussian(x, _GAUSS_SHARPEN, t.device(x.device))


def affine_resample(img, label, rotate=None, shear=None, scale=None, spatial_size=None, matrix=None):
    """Affine(mode=("bilinear", "nearest"), padding_mode="zeros") of an image and its label map in one kernel.  Either ``matrix``
    ([3, 3] or [B, 3, 3]: the source index of output voxel o is A (o - (size_out - 1) / 2) + (size_in - 1) / 2) or ``rotate``, ``shear``,
    ``scale`` (3 values each, see ``affine_matrix``).  Returns (image [B, 1, *spatial_size] float32, label uint8)."""
    x = _image(img)
    y = _label(label, x)
    if y.shape != x.shape:
        raise ValueError(f"label {tuple(y.shape)} does not match the image {tuple(x.shape)}")
    B = x.shape[0]
    if matrix is not None:
        if rotate is not None or shear is not None or scale is not None:
            raise ValueError("affine_resample: a matrix, or rotate / shear / scale, not both")
        A = np.asarray(matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else matrix, np.float64)
        A = np.broadcast_to(A, (B, 3, 3))
    else:
        A = np.broadcast_to(affine_matrix(rotate or (0, 0, 0), shear or (0, 0, 0), scale or (1, 1, 1)), (B, 3, 3))
    size = tuple(x.shape[2:]) if spatial_size is None else ((int(spatial_size),) * 3 if np.isscalar(spatial_size) else
                                                            tuple(int(s) for s in spatial_size))
    with torch.cuda.device(x.device):
        t = _Table(B)
        t.host["flags"], t.host["affine"] = AFFINE, A.reshape(B, 9)
        if y.dtype != torch.uint8:
            y = y.to(torch.uint8)
        out, olab, _, _ = _affine(x, y, size, t.device(x.device))
    return out, olab


# ---- the chain ----------------------------------------------------------------------------------------------------------------

def make_resident(image, device):
    """The leading ScaleIntensity of the whole volume, which has no randomness, applied once (what MONAI's CacheDataset caches too):
    a volume [D, H, W] (numpy or torch) -> float32 [D, H, W] on ``device``, rescaled by the same kernels."""
    v = torch.as_tensor(np.asarray(image, dtype=np.float32) if not isinstance(image, torch.Tensor) else image)
    v = v.to(device=device, dtype=torch.float32)
    if v.dim() != 3:
        raise ValueError(f"a volume [D, H, W] (got {tuple(v.shape)})")
    return scale_intensity(v[None, None])[0, 0]


def _volume3(v, name, dtypes):
    if not isinstance(v, torch.Tensor) or not v.is_cuda:
        raise RuntimeError(f"{name}: resident device tensors (there is no host path)")
    if v.dtype not in dtypes:
        raise TypeError(f"{name}: {' or '.join(str(d) for d in dtypes)} (got {v.dtype})")
    if v.dim() > 3 and any(s != 1 for s in v.shape[:-3]):
        raise ValueError(f"{name}: one channel, [D, H, W] (got {tuple(v.shape)})")
    if v.dim() < 3:
        raise ValueError(f"{name}: [D, H, W] (got {tuple(v.shape)})")
    return v.reshape(v.shape[-3:]).contiguous()


def build_table(volumes, labels, params):
    """The host table of one batch from ``draw_params``' dict (or one with the same keys) and the batch's resident volumes."""
    B = len(volumes)
    t = _Table(B)
    h = t.host
    on = params["on"]
    flags = np.full(B, RESCALE, np.int32)
    for k, bit, _ in SWITCHES:
        flags |= np.where(np.asarray(on[k], bool), bit, 0).astype(np.int32)
    h["flags"] = flags
    crop = params["crop_size"]
    for b in range(B):
        h["vol"][b], h["lab"][b] = volumes[b].data_ptr(), labels[b].data_ptr()
        h["vol_dim"][b] = volumes[b].shape
        size = [min(c, s) for c, s in zip(crop, volumes[b].shape)]
        h["gibbs_r"][b] = gibbs_radius(params["gibbs_alpha"][b], size)
    h["corner"] = params["corner"]
    h["noise_std"], h["bias"], h["gamma"] = params["rand_std"], params["coeff"], params["gamma"]
    h["sharpen_alpha"] = params["sharpen_alpha"]
    _set_taps(t, 0, np.asarray(params["smooth_sigma"], np.float64))
    _set_taps(t, 1, np.asarray(params["sharpen_sigma1"], np.float64))
    _set_taps(t, 2, np.asarray(params["sharpen_sigma2"], np.float64))
    A = np.asarray(params["affine"], np.float64).copy()
    A[~np.asarray(on["affine"], bool)] = np.eye(3)
    h["affine"] = A.reshape(B, 9)
    return t


def augment_batch(volumes, labels, params, noise=None):
    """The chain of ``get_train_transforms`` in the reference's order -- crop, noise, bias, Gibbs, contrast, smooth, sharpen, affine,
    rescale -- on one batch.  ``volumes``: per sample its resident, already rescaled volume (float32 [D, H, W] on the device, see
    ``make_resident``; the same tensor may appear several times); ``labels``: the matching label maps, all float32 or all uint8;
    ``params``: ``draw_params``' dict.  ``noise``: the standard-normal tensor [B, 1, d, h, w] of the noise stage; None draws
    ``torch.randn`` from ``torch.Generator(device).manual_seed(params["noise_seed"])``.
    Returns (image [B, 1, c, c, c] float32, label [B, 1, c, c, c] uint8).  A stage that no sample of the batch has switched on is
    not launched; nothing is read back from the device."""
    if len(volumes) == 0 or len(volumes) != len(labels):
        raise ValueError("augment_batch: one label map per volume, at least one")
    vols = [_volume3(v, "volumes", (torch.float32,)) for v in volumes]
    labs = [_volume3(v, "labels", (torch.float32, torch.uint8)) for v in labels]
    dev = vols[0].device
    B = len(vols)
    if any(v.device != dev for v in vols + labs):
        raise ValueError("augment_batch: volumes and labels must be on one device")
    if len({l.dtype for l in labs}) != 1:
        raise TypeError("augment_batch: the label maps must share one dtype")
    if any(l.shape != v.shape for v, l in zip(vols, labs)):
        raise ValueError("augment_batch: every label map must have its volume's shape")
    crop = tuple(int(c) for c in params["crop_size"])
    sizes = {tuple(min(c, s) for c, s in zip(crop, v.shape)) for v in vols}
    if len(sizes) != 1:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"augment_batch: the samples of a batch must share min(crop, volume) per axis (got {sorted(sizes)})")
    size = sizes.pop()
    with torch.cuda.device(dev):
        table = build_table(vols, labs, params)
        on = {k: [b for b in range(B) if params["on"][k][b]] for k, _, _ in SWITCHES}
        if noise is None:
            noise = torch.randn((B, 1) + size, generator=torch.Generator(dev).manual_seed(int(params["noise_seed"])), device=dev,
                                dtype=torch.float32)
        else:
            noise = _image(noise, "noise")
            if tuple(noise.shape) != (B, 1) + size:
                raise ValueError(f"noise: {(B, 1) + size} (got {tuple(noise.shape)})")
        table.device(dev)                                   # the one copy of the batch's parameters
        x, lab = _crop(table, B, size, noise, labs[0].dtype, dev)
        _gibbs(x, on["gibbs"], table)
        if on["contrast"]:
            _pointwise(x, x, _minmax(x), _OP_CONTRAST, table)
        if on["smooth"]:
            x = _gaussian(x, _GAUSS_SMOOTH, table)
        if on["sharpen"]:
            x = _gaussian(x, _GAUSS_SHARPEN, table)
        out, olab, sc, nb = _affine(x, lab, crop, table)
        _pointwise(out, out, _stream.minmax_finalize(sc, nb, B, out[0].numel(), dev), _OP_SCALE, table)
    return out, olab
