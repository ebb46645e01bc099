"""Step 2 of the reference's synthetic data generation (synthetic-data-generation/step2_generate_views.py with
datagen_utils.py:475-646) on the device, a batch of label maps at a time: the appearance model (``sample_gmm`` times
``1 + perl_mult_factor * draw_perlin_volume``) and the MONAI chain of ``get_transforms``, two views per label map.  The kernels are
csrc/amx_synth.hip and, for the stages the segmentation chain already has, csrc/amx_segaug.hip through
``anatomix_amd.segmentation.augment``.  Only the forward FFTs of the spike and the two FFTs of the Gibbs transform are ``torch.fft``.

Labels are [B, 1, D, H, W] uint8, views [B, 2, D, H, W] (the ``img`` layout of the pretraining HDF5 file); inside, a view is one of
n = 2 B rows, row = 2 sample + view.  The random parameters are drawn on the host (``draw_params``) and reach the kernels through
two small tables copied once per batch.

MONAI is not a dependency.  KSpaceSpikeNoise and SimulateLowResolution are restated from MONAI's documented algorithms (DESIGN.md
section 4.17); parity with an installed MONAI is NOT pinned and its random streams are not reproduced.  The reference's own
arithmetic (``sample_gmm``, ``draw_perlin_volume``) is pinned by tests/golden/datagen_golden.npz.

There is no host path: CPU tensors, other dtypes and shapes outside the envelope raise before anything is launched."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib, _stream
from ..segmentation import augment as SA

ZERO_BACKGROUND, SPIKE, SPIKE_FIXED, LOWRES = 1, 2, 4, 8
MAX_SCALES = 8
MAX_LDS_FLOATS = 12288
# chain order; (name, probability)
SWITCHES = (("bias", 0.98), ("spike", 0.2), ("contrast", 0.5), ("smooth", 0.5), ("gibbs", 0.5), ("sharpen", 0.25), ("lowres", 0.333))

# include/anatomix_amd.h: amx_synth_view
VIEW_DTYPE = np.dtype([("flags", "<i4"), ("nlabels", "<i4"), ("rank", "u1", (256,)), ("mean", "<f4", (256,)), ("std", "<f4", (256,)),
                       ("perl_mult", "<f4"), ("spike_loc", "<i4", (3,)), ("spike_slot", "<i4"), ("spike_factor", "<f4"),
                       ("spike_intensity", "<f4"), ("lowres", "<i4", (3,))])


class _Table(_stream.RecordTable):
    """The per-row records of one batch."""
    DTYPE, STRUCT, SIZE_SYMBOL = VIEW_DTYPE, "amx_synth_view", "amx_synth_view_bytes"
    DEFAULTS = {"nlabels": 1, "lowres": 1}


def _rows(x, name="image"):
    """A contiguous float32 device tensor [B, C, D, H, W] as rows [B C, 1, D, H, W], or an error."""
    x = _stream.device_tensor(x, name, (torch.float32,), "data generation")
    if x.dim() != 5:
        raise ValueError(f"{name}: [B, C, D, H, W] (got {tuple(x.shape)})")
    return x.contiguous().view((x.shape[0] * x.shape[1], 1) + tuple(x.shape[2:]))


def _labels(y):
    y = _stream.device_tensor(y, "labels", (torch.uint8,), "data generation")
    if y.dim() != 5 or y.shape[1] != 1:
        raise ValueError(f"labels: [B, 1, D, H, W] (got {tuple(y.shape)})")
    return y.contiguous()


def _per_row(v, n, width=None, name="parameter", dtype=np.float64):
    return _stream.per_row(v, (n,) if width is None else (n, width), name,
                           f"a scalar, {'' if width is None else f'{width} values, '}or one per view ({n})", dtype=dtype)


def coarse_shapes(shape, scales):
    """Per scale the shape ``ceil(shape / scale)`` of its coarse grid.  Every axis must divide by every scale (the reference's
    ``out +=`` fails otherwise), and a workgroup's collapsed coarse rows must fit its LDS."""
    shape = tuple(int(s) for s in shape)
    scales = tuple(int(s) for s in scales)
    if not 1 <= len(scales) <= MAX_SCALES:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_INVALID, f"1 to {MAX_SCALES} Perlin scales (got {len(scales)})")
    for s in scales:
        if s < 1 or any(n % s for n in shape):
            raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"scale {s} does not divide {shape}: outside the envelope of the reference's `out +=`")
    w = shape[2]
    need = ((1023 + w - 1) // w + 1) * sum(w // s for s in scales)
    if need > MAX_LDS_FLOATS:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"W = {w} with scales {scales} needs {need} floats of LDS per workgroup (at most {MAX_LDS_FLOATS})")
    return [tuple(n // s for n in shape) for s in scales]


def rank_table(unique):
    """The 256-entry label -> rank table of a sample from its sorted distinct labels (at most 256 integers in 0 .. 255)."""
    u = np.asarray(unique)
    if u.ndim != 1 or u.size < 1 or u.size > 256:
        raise ValueError(f"1 to 256 distinct labels per sample (got {u.size})")
    if not np.all(u == np.round(u)) or u.min() < 0 or u.max() > 255:
        raise ValueError("labels must be integers in 0 .. 255")
    u = u.astype(np.int64)
    if np.any(np.diff(u) <= 0):
        raise ValueError("the distinct labels must be sorted and unique")
    lut = np.zeros(256, np.uint8)
    lut[u] = np.arange(u.size)
    return lut


def draw_params(rng, labels_per_sample, shape, scales=(4, 8, 16, 32), perl_max_std=5.0, perl_mult_factor=0.02, means_range=(25, 255),
                stds_range=(5, 20), zero_background=0.25):
    """Everything ``process_volume`` randomises, for one batch, from a ``numpy.random.RandomState``.

    ``labels_per_sample``: per sample its sorted distinct labels; ``shape``: the (D, H, W) all samples share.  The draw order is this
    function's own (neither torch's nor MONAI's random streams are reproduced).  Per sample, in batch order, per view (0, then 1):
      1. ``means`` U(means_range) per label, then ``stds`` U(stds_range) per label;
      2. one ``uniform()`` for ``zero_background`` (on when below 0.25; always off for a sample with one label, where the reference yields NaN);
      3. one ``perl_std`` U(0, perl_max_std) per scale;
      4. per transform in chain order (bias, spike, contrast, smooth, Gibbs, sharpen, low resolution) one ``uniform()`` for its switch
         (on when below 0.98, 0.2, 0.5, 0.5, 0.5, 0.25, 0.333), directly followed by its parameters, drawn whether it is on or not:
         bias 20 coefficients U(0, 0.075); spike location ``randint(0, size)`` per axis, then ``u`` U(0.95, 1.1); contrast ``gamma``
         U(0.5, 2); smooth ``sigma`` U(0, 0.333) x 3; Gibbs ``alpha`` U(0, 0.333); sharpen ``sigma1`` U(0.5, 1) x 3, then ``sigma2``
         U(0.5, sigma1) x 3, then ``alpha`` U(10, 30); low resolution ``zoom`` U(0.5, 1).
    After the two views of a sample: its ``noise_seed = randint(0, 2**31 - 1)``.
    Returns a dict of arrays [B, 2, ...] (``means``, ``stds`` and ``unique_labels``: lists per sample)."""
    B, S = len(labels_per_sample), len(scales)
    shape = tuple(int(s) for s in shape)
    p = dict(shape=shape, scales=tuple(int(s) for s in scales), perl_mult_factor=float(perl_mult_factor),
             unique_labels=[np.asarray(u).astype(np.int64) for u in labels_per_sample], means=[], stds=[],
             zero_background=np.zeros((B, 2), bool), perl_std=np.zeros((B, 2, S)), on={k: np.zeros((B, 2), bool) for k, _ in SWITCHES},
             coeff=np.zeros((B, 2, 20)), spike_loc=np.zeros((B, 2, 3), np.int64), spike_factor=np.zeros((B, 2)), gamma=np.zeros((B, 2)),
             smooth_sigma=np.zeros((B, 2, 3)), gibbs_alpha=np.zeros((B, 2)), sharpen_sigma1=np.zeros((B, 2, 3)),
             sharpen_sigma2=np.zeros((B, 2, 3)), sharpen_alpha=np.zeros((B, 2)), zoom=np.zeros((B, 2)), noise_seed=np.zeros(B, np.int64))
    prob = dict(SWITCHES)
    for b in range(B):
        L = len(p["unique_labels"][b])
        means, stds = np.zeros((2, L)), np.zeros((2, L))
        for v in range(2):
            means[v] = rng.uniform(means_range[0], means_range[1], L)
            stds[v] = rng.uniform(stds_range[0], stds_range[1], L)
            p["zero_background"][b, v] = (rng.uniform() < zero_background) and L > 1
            p["perl_std"][b, v] = rng.uniform(0.0, perl_max_std, S)
            on = p["on"]
            on["bias"][b, v] = rng.uniform() < prob["bias"]
            p["coeff"][b, v] = rng.uniform(0.0, 0.075, 20)
            on["spike"][b, v] = rng.uniform() < prob["spike"]
            p["spike_loc"][b, v] = [rng.randint(0, n) for n in shape]
            p["spike_factor"][b, v] = rng.uniform(0.95, 1.1)
            on["contrast"][b, v] = rng.uniform() < prob["contrast"]
            p["gamma"][b, v] = rng.uniform(0.5, 2.0)
            on["smooth"][b, v] = rng.uniform() < prob["smooth"]
            p["smooth_sigma"][b, v] = rng.uniform(0.0, 0.333, 3)
            on["gibbs"][b, v] = rng.uniform() < prob["gibbs"]
            p["gibbs_alpha"][b, v] = rng.uniform(0.0, 0.333)
            on["sharpen"][b, v] = rng.uniform() < prob["sharpen"]
            p["sharpen_sigma1"][b, v] = rng.uniform(0.5, 1.0, 3)
            p["sharpen_sigma2"][b, v] = [rng.uniform(0.5, s1) for s1 in p["sharpen_sigma1"][b, v]]
            p["sharpen_alpha"][b, v] = rng.uniform(10.0, 30.0)
            on["lowres"][b, v] = rng.uniform() < prob["lowres"]
            p["zoom"][b, v] = rng.uniform(0.5, 1.0)
        p["means"].append(means)
        p["stds"].append(stds)
        p["noise_seed"][b] = rng.randint(0, 2 ** 31 - 1)
    return p


def concat_params(parts):
    """One batch from the ``draw_params`` dicts of its samples (same shape and scales)."""
    first = parts[0]
    if any(q["shape"] != first["shape"] or q["scales"] != first["scales"] or q["perl_mult_factor"] != first["perl_mult_factor"] for q in parts):
        raise ValueError("the samples of a batch must share shape, scales and perl_mult_factor")
    out = dict(shape=first["shape"], scales=first["scales"], perl_mult_factor=first["perl_mult_factor"])
    for k, v in first.items():
        if k in out:
            continue
        if isinstance(v, list):
            out[k] = [e for q in parts for e in q[k]]
        elif isinstance(v, dict):
            out[k] = {n: np.concatenate([q[k][n] for q in parts]) for n in v}
        else:
            out[k] = np.concatenate([q[k] for q in parts])
    return out


def low_resolution_shape(shape, zoom):
    """MONAI's target shape: ``int(round(n * zoom))`` per axis (at least 1)."""
    return tuple(max(int(round(n * float(zoom))), 1) for n in shape)


def draw_fields(params, device):
    """The standard-normal volume [B, 2, D, H, W] and, per scale, the coarse grids [B, 2, *coarse] multiplied by their drawn std:
    per sample from ``torch.Generator(device).manual_seed(noise_seed[b])``, the volume first, then the scales in order."""
    shape, B = params["shape"], len(params["unique_labels"])
    cs = coarse_shapes(shape, params["scales"])
    noise = torch.empty((B, 2) + shape, dtype=torch.float32, device=device)
    grids = [torch.empty((B, 2) + c, dtype=torch.float32, device=device) for c in cs]
    std = torch.as_tensor(np.asarray(params["perl_std"], np.float32), device=device)
    for b in range(B):
        gen = torch.Generator(device).manual_seed(int(params["noise_seed"][b]))
        noise[b] = torch.randn((2,) + shape, generator=gen, device=device, dtype=torch.float32)
        for s, c in enumerate(cs):
            grids[s][b] = torch.randn((2,) + c, generator=gen, device=device, dtype=torch.float32) * std[b, :, s].view(2, 1, 1, 1)
    return noise, grids


# ---- the stages on rows --------------------------------------------------------------------------------------------------------

def _scratch(n, V, dev):
    nb = _lib.load().amx_synth_scratch_bytes(n, V)
    return _lib.scratch(nb, dev), nb


def _finalize(sc, nb, n, V, dev):
    return _stream.minmax_finalize(sc, nb, n, V, dev)


def _appearance_table(params, B):
    """The appearance part of the records, validated on the host."""
    t = _Table(2 * B)
    h = t.host
    if len(params["unique_labels"]) != B or len(params["means"]) != B or len(params["stds"]) != B:
        raise ValueError(f"params: one entry per sample of the batch of {B}")
    zb = np.asarray(params["zero_background"], bool).reshape(B, 2)
    for b in range(B):
        u = np.asarray(params["unique_labels"][b])
        lut = rank_table(u)
        m, s = np.asarray(params["means"][b], np.float64), np.asarray(params["stds"][b], np.float64)
        if m.shape != (2, u.size) or s.shape != (2, u.size):
            raise ValueError(f"sample {b}: means and stds must be [2, {u.size}] (got {m.shape}, {s.shape})")
        for v in range(2):
            if u.size == 1 and zb[b, v]:
                raise ValueError(f"sample {b} view {v}: a single label with a zero background is a constant volume (the reference yields NaN)")
            r = 2 * b + v
            h["nlabels"][r], h["rank"][r] = u.size, lut
            h["mean"][r, :u.size], h["std"][r, :u.size] = m[v], s[v]
            h["flags"][r] = ZERO_BACKGROUND if zb[b, v] else 0
    h["perl_mult"] = float(params["perl_mult_factor"])
    return t


def _appearance(lab, params, noise, grids, table):
    """-> (views [B, 2, D, H, W] float32, the scratch holding their min / max partials, its size)."""
    B, shape, dev = lab.shape[0], tuple(lab.shape[2:]), lab.device
    V = int(np.prod(shape))
    lib = _lib.load()
    sc, nb = _scratch(2 * B, V, dev)
    st = _lib.stream(dev)
    _lib.check_envelope(lib.amx_synth_gmm_minmax(_lib.ptr(lab), _lib.ptr(noise), B, V, *table.args, _lib.ptr(sc), nb, st))
    mm = _finalize(sc, nb, 2 * B, V, dev)
    out = torch.empty((B, 2) + shape, dtype=torch.float32, device=dev)
    S = len(grids)
    gp = (ctypes.c_void_p * S)(*[g.data_ptr() for g in grids])
    scales = (ctypes.c_int * S)(*[int(s) for s in params["scales"]])
    _lib.check_envelope(lib.amx_synth_appearance(_lib.ptr(lab), _lib.ptr(noise), gp, scales, S, _lib.ptr(mm), _lib.ptr(out), B, *shape,
                        *table.args, _lib.ptr(sc), nb, st))
    return out, sc, nb


def _check_fields(lab, params, noise, grids):
    B, shape, dev = lab.shape[0], tuple(lab.shape[2:]), lab.device
    if tuple(params["shape"]) != shape:
        raise ValueError(f"params are drawn for {tuple(params['shape'])}, the labels are {shape}")
    cs = coarse_shapes(shape, params["scales"])
    if (noise is None) != (grids is None):
        raise ValueError("noise and grids: both or neither")
    if noise is None:
        return None, None
    noise = _rows(noise, "noise")
    if tuple(noise.shape) != (2 * B, 1) + shape or noise.device != dev:
        raise ValueError(f"noise: {(B, 2) + shape} on the labels' device (got {tuple(noise.shape)})")
    if len(grids) != len(cs):
        raise ValueError(f"grids: one per scale ({len(cs)}; got {len(grids)})")
    out = []
    for g, c in zip(grids, cs):
        g = _rows(g, "grids")
        if tuple(g.shape) != (2 * B, 1) + c or g.device != dev:
            raise ValueError(f"grids: {(B, 2) + c} on the labels' device (got {tuple(g.shape)})")
        out.append(g)
    return noise, out


def synthesize_views(labels, params, noise=None, grids=None):
    """The appearance model: per sample and view ``minmax(max(std[rank] z + mean[rank], 0)) * (1 + perl_mult_factor * P)`` with P the
    sum of the trilinearly upsampled coarse ``grids``.  ``params``: ``draw_params``' dict (``unique_labels``, ``means``, ``stds``,
    ``zero_background``, ``scales``, ``perl_mult_factor``, ``shape``; ``perl_std`` and ``noise_seed`` when the fields are drawn here).
    ``noise`` [B, 2, D, H, W] standard normal and ``grids`` (per scale [B, 2, *coarse], already multiplied by their std): both or
    neither; omitted, ``draw_fields`` draws them.  -> float32 [B, 2, D, H, W]."""
    lab = _labels(labels)
    noise, grids = _check_fields(lab, params, noise, grids)
    table = _appearance_table(params, lab.shape[0])
    with torch.cuda.device(lab.device):
        if noise is None:
            noise, grids = draw_fields(params, lab.device)
        return _appearance(lab, params, noise, grids, table.device(lab.device))[0]


def _spike(x, which, table):
    """In place on the rows ``which`` (host indices, whose records hold their slot in that order)."""
    if not which:
        return x
    n, V, dev = x.shape[0], x[0].numel(), x.device
    lib = _lib.load()
    sub = x.index_select(0, torch.as_tensor(which, device=dev)) if len(which) < n else x
    k = torch.view_as_real(torch.fft.fftn(sub[:, 0], dim=(-3, -2, -1)).contiguous())
    mean = torch.empty(len(which), dtype=torch.float32, device=dev)
    sc, nb = _scratch(len(which), V, dev)
    st = _lib.stream(dev)
    _lib.check_envelope(lib.amx_synth_logk_mean(_lib.ptr(k), len(which), V, _lib.ptr(mean), _lib.ptr(sc), nb, st))
    _lib.check_envelope(lib.amx_synth_spike(_lib.ptr(x), _lib.ptr(k), len(which), _lib.ptr(mean), n, *x.shape[2:], *table.args, st))
    return x


def _lowres(x, table):
    out = torch.empty_like(x)
    _lib.check_envelope(_lib.load().amx_synth_lowres(_lib.ptr(x), _lib.ptr(out), x.shape[0], *x.shape[2:], *table.args, _lib.stream(x.device)))
    return out


def _tail(x, dtype):
    if dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"dtype: torch.float32 or torch.uint8 (got {dtype})")
    n, V, dev = x.shape[0], x[0].numel(), x.device
    lib = _lib.load()
    sc, nb = _scratch(n, V, dev)
    _lib.check_envelope(lib.amx_synth_clip_minmax(_lib.ptr(x), n, V, _lib.ptr(sc), nb, _lib.stream(dev)))
    mm = _finalize(sc, nb, n, V, dev)
    out = torch.empty(x.shape, dtype=dtype, device=dev)
    _lib.check_envelope(lib.amx_synth_finish(_lib.ptr(x), _lib.ptr(out), n, V, _lib.ptr(mm), int(dtype == torch.uint8), _lib.stream(dev)))
    return out


# ---- one public function per new transform -------------------------------------------------------------------------------------

def kspace_spike_noise(img, loc, k_intensity=None, factor=1.0):
    """KSpaceSpikeNoise(loc, k_intensity): k = fftshift(fftn(x)); log(|k| + 1e-10) at ``loc`` becomes ``k_intensity``, the phase is kept;
    real(ifftn(ifftshift(k))).  ``k_intensity=None`` is RandKSpaceSpikeNoise's default ``factor * 2.5 * mean(log(|k| + 1e-10))``, taken
    on the device.  ``loc`` (3 indices into the shifted k-space), ``k_intensity`` and ``factor``: one, or one per view of [B, C, D, H, W].
    Implemented as one forward FFT, a reduction and one plane wave added per voxel."""
    x = _rows(img).clone()
    n = x.shape[0]
    loc = _per_row(loc, n, 3, "loc", np.int64)
    for a in range(3):
        if loc[:, a].min() < 0 or loc[:, a].max() >= x.shape[2 + a]:
            raise ValueError(f"loc: axis {a} must lie in 0 .. {x.shape[2 + a] - 1}")
    with torch.cuda.device(x.device):
        t = _Table(n)
        t.host["flags"] = SPIKE | (0 if k_intensity is None else SPIKE_FIXED)
        t.host["spike_loc"], t.host["spike_slot"] = loc, np.arange(n)
        t.host["spike_factor"] = _per_row(factor, n, name="factor")
        if k_intensity is not None:
            t.host["spike_intensity"] = _per_row(k_intensity, n, name="k_intensity")
        return _spike(x, list(range(n)), t.device(x.device)).view(img.shape)


def simulate_low_resolution(img, zoom):
    """SimulateLowResolution(zoom_range=(zoom, zoom), downsample_mode="nearest-exact", upsample_mode="trilinear"): a nearest-exact
    resize to ``int(round(n * zoom))`` per axis and a trilinear resize (align_corners=False) back, as one gather.  ``zoom``: one, or one
    per view of [B, C, D, H, W]."""
    x = _rows(img)
    n = x.shape[0]
    zoom = _per_row(zoom, n, name="zoom")
    if not np.all((zoom > 0) & (zoom <= 1)):
        raise ValueError("zoom: 0 < zoom <= 1")
    with torch.cuda.device(x.device):
        t = _Table(n)
        t.host["flags"] = LOWRES
        t.host["lowres"] = [low_resolution_shape(x.shape[2:], z) for z in zoom]
        return _lowres(x, t.device(x.device)).view(img.shape)


def clip_rescale(img, dtype=torch.float32):
    """ThresholdIntensity(above=True, threshold=0) and ScaleIntensity per view: max(x, 0), then (c - min) / (max - min) (c * 0 when
    min == max).  ``dtype=torch.uint8`` writes ``trunc(255 * y)`` in the same pass, as the reference's ``astype(np.uint8)``."""
    x = _rows(img)
    with torch.cuda.device(x.device):
        return _tail(x, dtype).view(img.shape)


# ---- the chain ----------------------------------------------------------------------------------------------------------------

def _chain_tables(params, n, shape):
    """(segmentation record table, synth record table) of the chain, without the appearance part."""
    on = {k: np.asarray(params["on"][k], bool).reshape(n) for k, _ in SWITCHES}
    seg = SA._Table(n)
    h = seg.host
    flags = np.full(n, SA.RESCALE, np.int32)
    for k, bit in (("bias", SA.BIAS), ("contrast", SA.CONTRAST), ("smooth", SA.SMOOTH), ("gibbs", SA.GIBBS), ("sharpen", SA.SHARPEN)):
        flags |= np.where(on[k], bit, 0).astype(np.int32)
    h["flags"] = flags
    h["vol_dim"] = shape
    h["bias"] = np.asarray(params["coeff"], np.float64).reshape(n, 20)
    h["gamma"] = np.asarray(params["gamma"], np.float64).reshape(n)
    h["sharpen_alpha"] = np.asarray(params["sharpen_alpha"], np.float64).reshape(n)
    h["gibbs_r"] = [SA.gibbs_radius(a, shape) for a in np.asarray(params["gibbs_alpha"], np.float64).reshape(n)]
    SA._set_taps(seg, 0, np.asarray(params["smooth_sigma"], np.float64).reshape(n, 3))
    SA._set_taps(seg, 1, np.asarray(params["sharpen_sigma1"], np.float64).reshape(n, 3))
    SA._set_taps(seg, 2, np.asarray(params["sharpen_sigma2"], np.float64).reshape(n, 3))
    syn = _Table(n)
    s = syn.host
    s["flags"] = np.where(on["spike"], SPIKE, 0) | np.where(on["lowres"], LOWRES, 0)
    s["spike_loc"] = np.asarray(params["spike_loc"], np.int64).reshape(n, 3)
    s["spike_factor"] = np.asarray(params["spike_factor"], np.float64).reshape(n)
    s["spike_slot"] = np.cumsum(on["spike"]) - 1
    s["lowres"] = [low_resolution_shape(shape, z) for z in np.asarray(params["zoom"], np.float64).reshape(n)]
    for a in range(3):
        if on["spike"].any() and (s["spike_loc"][on["spike"], a].min() < 0 or s["spike_loc"][on["spike"], a].max() >= shape[a]):
            raise ValueError(f"spike_loc: axis {a} must lie in 0 .. {shape[a] - 1}")
    return seg, syn, {k: [int(i) for i in np.nonzero(v)[0]] for k, v in on.items()}


def _chain(x, seg, syn, on, dtype, partials=None):
    """The chain on rows x [n, 1, D, H, W], which it may overwrite.  ``seg`` is not copied yet (its records point into x)."""
    n, V, dev = x.shape[0], x[0].numel(), x.device
    lab = torch.zeros((n, V), dtype=torch.uint8, device=dev) if on["bias"] else None
    for r in range(n):
        seg.host["vol"][r] = x[r].data_ptr()
        seg.host["lab"][r] = lab[r].data_ptr() if lab is not None else 0
    seg.device(dev)
    mm = SA._minmax(x) if partials is None else _finalize(partials[0], partials[1], n, V, dev)
    SA._pointwise(x, x, mm, SA._OP_SCALE, seg)
    if on["bias"]:
        x = SA._crop(seg, n, tuple(x.shape[2:]), None, torch.uint8, dev)[0]
    _spike(x, on["spike"], syn)
    if on["contrast"]:
        SA._pointwise(x, x, SA._minmax(x), SA._OP_CONTRAST, seg)
    if on["smooth"]:
        x = SA._gaussian(x, SA._GAUSS_SMOOTH, seg)
    SA._gibbs(x, on["gibbs"], seg)
    if on["sharpen"]:
        x = SA._gaussian(x, SA._GAUSS_SHARPEN, seg)
    if on["lowres"]:
        x = _lowres(x, syn)
    return _tail(x, dtype)


def augment_views(views, params, dtype=torch.float32):
    """The chain of ``get_transforms`` in the reference's order -- ScaleIntensity, bias field, k-space spike, AdjustContrast, Gaussian
    smooth, Gibbs, Gaussian sharpen, low resolution, threshold at 0, ScaleIntensity -- on views [B, 2, D, H, W] float32, every view
    with its own switches and parameters (``draw_params``' dict).  A stage that no view has switched on is not launched; nothing is
    read back from the device.  -> [B, 2, D, H, W] float32, or uint8 ``trunc(255 * y)``."""
    if dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"dtype: torch.float32 or torch.uint8 (got {dtype})")
    x = _rows(views, "views")
    if views.shape[1] != 2:
        raise ValueError(f"views: [B, 2, D, H, W] (got {tuple(views.shape)})")
    seg, syn, on = _chain_tables(params, x.shape[0], tuple(x.shape[2:]))
    with torch.cuda.device(x.device):
        return _chain(x.clone(), seg, syn.device(x.device), on, dtype).view(views.shape)


def generate_views(labels, params, dtype=torch.uint8, noise=None, grids=None):
    """``process_volume`` for a batch: the appearance model, then the chain.  ``labels`` [B, 1, D, H, W] uint8 on the device, ``params``
    from ``draw_params``; ``noise`` / ``grids`` as in ``synthesize_views``.  One copy of each parameter table per batch.
    -> [B, 2, D, H, W] ``dtype`` (uint8: what the reference stores)."""
    if dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"dtype: torch.float32 or torch.uint8 (got {dtype})")
    lab = _labels(labels)
    B, shape = lab.shape[0], tuple(lab.shape[2:])
    noise, grids = _check_fields(lab, params, noise, grids)
    syn = _appearance_table(params, B)
    seg, chain, on = _chain_tables(params, 2 * B, shape)
    for k in ("flags", "spike_loc", "spike_factor", "spike_slot", "lowres"):
        syn.host[k] = syn.host[k] | chain.host[k] if k == "flags" else chain.host[k]
    with torch.cuda.device(lab.device):
        if noise is None:
            noise, grids = draw_fields(params, lab.device)
        syn.device(lab.device)
        views, sc, nb = _appearance(lab, params, noise, grids, syn)
        return _chain(views.view((2 * B, 1) + shape), seg, syn, on, dtype, partials=(sc, nb)).view((B, 2) + shape)
