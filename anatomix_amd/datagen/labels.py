"""Step 1 of the reference's synthetic data generation (synthetic-data-generation/step1_generate_labels.py with
datagen_utils.py:26-447) on the device, a batch of label ensembles at a time: templates composed under random affine maps, a
3 x 3 x 3 median, the deformed-sphere foreground mask, and the envelope around it.  The kernels are csrc/amx_labels.hip.

Ensembles are [B, 1, D, H, W] uint8.  The random parameters are drawn on the host (``draw_params``) and reach the kernels through two
small tables copied once per batch; the templates, which come from files, are cropped to their non-zero bounding box on the host and
uploaded in one byte buffer.  Nothing is read back between the stages.

skimage is not a dependency.  ``skimage.filters.median``, ``morphology.dilation`` and ``morphology.erosion`` are restated as the scipy
calls skimage documents as its implementation; parity with an installed skimage is NOT pinned.  The
reference's own arithmetic (``crop_and_pad_3d_volume``, ``apply_random_affine_transform``, ``sample_corruption``) is pinned by
tests/golden/datagen_labels_golden.npz.

There is no host path: CPU tensors, other dtypes and shapes outside the envelope raise before anything is launched."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib, _stream

MASK, ENVELOPE = 1, 2
MAX_TEMPLATES = 64
IDENTIFIERS = ("unconstrained", "foreground_masked", "foreground_masked_enveloped")
MIN_ENVELOPE_AXIS = 9

# include/anatomix_amd.h: amx_labels_template, amx_labels_ensemble
TEMPLATE_DTYPE = np.dtype([("offset", "<i8"), ("crop", "<i4", (3,)), ("before", "<i4", (3,)), ("padded", "<i4", (3,)), ("reserved", "<i4"),
                           ("affine", "<f8", (12,))])
ENSEMBLE_DTYPE = np.dtype([("flags", "<i4"), ("first", "<i4"), ("count", "<i4"), ("radius", "<i4"), ("shift", "<i4", (3,)), ("ball", "<i4")])


class _Templates(_stream.RecordTable):
    """One record per template of the batch."""
    DTYPE, STRUCT, SIZE_SYMBOL = TEMPLATE_DTYPE, "amx_labels_template", "amx_labels_template_bytes"


class _Ensembles(_stream.RecordTable):
    """One record per ensemble of the batch."""
    DTYPE, STRUCT, SIZE_SYMBOL = ENSEMBLE_DTYPE, "amx_labels_ensemble", "amx_labels_ensemble_bytes"
    DEFAULTS = {"count": 1, "ball": 2}


def _volumes(x, name="labels"):
    x = _stream.device_tensor(x, name, (torch.uint8,), "data generation")
    if x.dim() != 5 or x.shape[1] != 1:
        raise ValueError(f"{name}: [B, 1, D, H, W] (got {tuple(x.shape)})")
    return x.contiguous()


def _per_ensemble(v, n, width=None, name="parameter", dtype=np.float64):
    return _stream.per_row(v, (n,) if width is None else (n, width), name,
                           f"a scalar, {'' if width is None else f'{width} values, '}or one per ensemble ({n})", dtype=dtype)


def _cube(shape):
    """The side of a cube the mask kernel takes, or an error."""
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or len(set(shape)) != 1:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"the foreground mask needs a cube (got {shape}): the reference mixes the axes otherwise")
    S = shape[0]
    if S % 16 or not 16 <= S <= 256:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"the foreground mask needs side % 16 == 0, 16 <= side <= 256 (got {S})")
    return S


# ---- parameters --------------------------------------------------------------------------------------------------------------

def rotation_matrix(degrees):
    """datagen_utils.py:28-66: ``Rx @ Ry @ Rz`` of the three angles in degrees, float64."""
    r = np.radians(np.asarray(degrees, np.float64))
    c, s = np.cos(r), np.sin(r)
    rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    return rx @ ry @ rz


def affine_matrix(scale, rotation_degrees, translation, shear, reflection):
    """datagen_utils.py:118-132: the 4 x 4 float64 output -> source map ``scale @ rotation @ shear`` with ``translation`` in its last
    column; ``reflection`` (three booleans) negates the scale of its axes, ``shear`` fills the upper triangle row by row."""
    sc = np.diag(np.asarray(scale, np.float64))
    sh = np.eye(3)
    sh[np.triu_indices(3, k=1)] = np.asarray(shear, np.float64)
    for i in range(3):
        if reflection[i]:
            sc[i, i] *= -1
    m = np.eye(4)
    m[:3, :3] = sc @ rotation_matrix(rotation_degrees) @ sh
    m[:3, 3] = np.asarray(translation, np.float64)
    return m


def draw_params(rng, n_templates_per_sample, side_length, rscale=0.5, rrotation=180.0, rtranslation=5.0, rshear=0.5, mask_above=0.33333,
                envelope_above=0.5, std_range=(1.0, 5.0)):
    """Everything ``generate_label_ensemble`` randomises except the choice of template files, for one batch, from a
    ``numpy.random.RandomState``.

    ``n_templates_per_sample``: per ensemble an integer, or a pair ``(min, max)`` from which the count is drawn as
    ``rng.randint(min, max)`` (``max`` exclusive, as in the reference).  The draw order is this function's own (the reference's numpy
    and torch streams are not reproduced).  Per ensemble, in batch order, with q = side_length / 128:
      1. the number of templates, when a pair is given;
      2. per template in order: ``scale`` U(1 - rscale, 1 + rscale) x 3, ``rotation`` U(-rrotation, rrotation) x 3 (degrees),
         ``translation`` U(-rtranslation, rtranslation) x 3, ``shear`` U(-rshear, rshear) x 3, ``reflection`` ``uniform() < 0.5`` x 3;
      3. one ``uniform()`` for the foreground mask (on when above 0.33333), then ``radius`` ``randint(round(48 q), round(72 q))``,
         ``centre`` ``randint(-round(32 q), round(32 q))`` x 3 and ``std`` U(q, 5 q) per noise scale (3);
      4. one ``uniform()`` for the envelope (on when above 0.5 and the mask is on), then ``ball`` ``randint(2, 5)``;
      5. ``noise_seed = randint(0, 2**31 - 1)``.
    Every number is drawn whether its switch is on or not.
    Returns a dict: ``side_length``, ``n_templates`` [B], ``affine`` (list per ensemble of [n, 4, 4] float64) with the drawn
    ``scale`` / ``rotation`` / ``translation`` / ``shear`` / ``reflection`` beside it, ``mask`` / ``envelope`` [B] bool, ``radius`` [B],
    ``centre`` [B, 3], ``std`` [B, 3], ``ball`` [B], ``noise_seed`` [B]."""
    B, S = len(n_templates_per_sample), int(side_length)
    q = S / 128
    p = dict(side_length=S, n_templates=np.zeros(B, np.int64), affine=[], scale=[], rotation=[], translation=[], shear=[], reflection=[],
             mask=np.zeros(B, bool), envelope=np.zeros(B, bool), radius=np.zeros(B, np.int64), centre=np.zeros((B, 3), np.int64),
             std=np.zeros((B, 3)), ball=np.zeros(B, np.int64), noise_seed=np.zeros(B, np.int64))
    for b, n in enumerate(n_templates_per_sample):
        n = int(rng.randint(int(n[0]), int(n[1]))) if np.ndim(n) else int(n)
        if n < 1:
            raise ValueError(f"ensemble {b}: at least one template (got {n})")
        p["n_templates"][b] = n
        d = {k: np.zeros((n, 3), bool if k == "reflection" else np.float64) for k in ("scale", "rotation", "translation", "shear", "reflection")}
        aff = np.zeros((n, 4, 4))
        for k in range(n):
            d["scale"][k] = rng.uniform(1.0 - rscale, 1.0 + rscale, 3)
            d["rotation"][k] = rng.uniform(-rrotation, rrotation, 3)
            d["translation"][k] = rng.uniform(-rtranslation, rtranslation, 3)
            d["shear"][k] = rng.uniform(-rshear, rshear, 3)
            d["reflection"][k] = rng.uniform(size=3) < 0.5
            aff[k] = affine_matrix(d["scale"][k], d["rotation"][k], d["translation"][k], d["shear"][k], d["reflection"][k])
        for k, v in d.items():
            p[k].append(v)
        p["affine"].append(aff)
        p["mask"][b] = rng.uniform() > mask_above
        p["radius"][b] = rng.randint(round(48 * q), round(72 * q))
        p["centre"][b] = rng.randint(-round(32 * q), round(32 * q), size=3)
        p["std"][b] = rng.uniform(std_range[0] * q, std_range[1] * q, 3)
        p["envelope"][b] = (rng.uniform() > envelope_above) and p["mask"][b]
        p["ball"][b] = rng.randint(2, 5)
        p["noise_seed"][b] = rng.randint(0, 2 ** 31 - 1)
    return p


def concat_params(parts):
    """One batch from the ``draw_params`` dicts of its ensembles (same side length)."""
    S = parts[0]["side_length"]
    if any(q["side_length"] != S for q in parts):
        raise ValueError("the ensembles of a batch must share their side length")
    out = dict(side_length=S)
    for k, v in parts[0].items():
        if k != "side_length":
            out[k] = [e for q in parts for e in q[k]] if isinstance(v, list) else np.concatenate([q[k] for q in parts])
    return out


def identifiers(params):
    """Per ensemble the reference's name of what it went through."""
    return [IDENTIFIERS[int(m) + int(m and e)] for m, e in zip(np.asarray(params["mask"], bool), np.asarray(params["envelope"], bool))]


def noise_scales(side_length):
    """The reference's (8, 16, 32) at 128^3, scaled to the side length."""
    S = _cube((side_length,) * 3)
    return (S // 16, S // 8, S // 4)


def draw_noise(params, device):
    """Per noise scale the coarse Gaussian grids [B, 3, n, n, n] (n = 16, 8, 4) multiplied by their drawn std: per ensemble from
    ``torch.Generator(device).manual_seed(noise_seed[b])``, the scales in order."""
    S = int(params["side_length"])
    B = len(params["noise_seed"])
    cs = [S // s for s in noise_scales(S)]
    std = torch.as_tensor(np.asarray(params["std"], np.float32).reshape(B, 3), device=device)
    grids = [torch.empty((B, 3, c, c, c), dtype=torch.float32, device=device) for c in cs]
    for b in range(B):
        gen = torch.Generator(device).manual_seed(int(params["noise_seed"][b]))
        for s, c in enumerate(cs):
            grids[s][b] = torch.randn((3, c, c, c), generator=gen, device=device, dtype=torch.float32) * std[b, s]
    return grids


# ---- templates ---------------------------------------------------------------------------------------------------------------

def crop_template(template):
    """A template file's volume as uint8, cropped to its non-zero bounding box (datagen_utils.py:164-173).  An all-zero template is an
    error: the reference redraws it before it gets here."""
    t = np.asarray(template)
    if t.ndim != 3:
        raise ValueError(f"template: a 3-D volume (got shape {t.shape})")
    t = t.astype(np.uint8, copy=False)
    box = []
    for a in range(3):      # the projections of the non-zero voxels, not their indices: three passes over the volume
        hit = np.flatnonzero(t.any(axis=tuple(i for i in range(3) if i != a)))
        if hit.size == 0:
            raise ValueError("template: all zero (the reference draws another file)")
        box.append(slice(int(hit[0]), int(hit[-1]) + 1))
    return np.ascontiguousarray(t[tuple(box)])


def pad_before(crop, size):
    """(pad-before, padded shape) per axis of ``crop_and_pad_3d_volume``: the padded shape is max(size, crop), and of an odd pad the
    extra voxel goes in front."""
    padded = [max(int(s), int(c)) for s, c in zip(size, crop)]
    pads = [P - int(c) for P, c in zip(padded, crop)]
    return [pad // 2 + (pad & 1) for pad in pads], padded


def _tables(templates, params, shape, base_offset=0):
    """(template records, ensemble records, the byte buffer) of a batch, validated on the host."""
    B = len(templates)
    n = np.asarray(params["n_templates"], np.int64).reshape(-1)
    if n.size != B or len(params["affine"]) != B:
        raise ValueError(f"params: one entry per ensemble of the batch of {B}")
    ens = _ensemble_table(params, B)
    crops, seen = [], {}
    for b, ts in enumerate(templates):
        if len(ts) != n[b]:
            raise ValueError(f"ensemble {b}: {n[b]} templates are drawn, {len(ts)} are given")
        if not 1 <= len(ts) <= MAX_TEMPLATES:
            raise _lib.AmxEnvelopeError(_lib.AMX_ERR_INVALID, f"ensemble {b}: 1 to {MAX_TEMPLATES} templates (got {len(ts)})")
        aff = np.asarray(params["affine"][b], np.float64)
        if aff.shape != (len(ts), 4, 4) or not np.all(np.isfinite(aff)):
            raise ValueError(f"ensemble {b}: affine must be finite [{len(ts)}, 4, 4] (got {aff.shape})")
        for t in ts:      # a volume drawn more than once in the batch (the same object) is cropped and uploaded once
            if id(t) not in seen:
                seen[id(t)] = len(seen), crop_template(t)
        crops.append([seen[id(t)] for t in ts])
    offsets, off = {}, int(base_offset)
    for slot, c in sorted(seen.values(), key=lambda e: e[0]):
        offsets[slot] = off
        off += c.size
    buf = np.zeros(off, np.uint8)
    for slot, c in seen.values():
        buf[offsets[slot]:offsets[slot] + c.size] = c.reshape(-1)
    tab = _Templates(int(n.sum()))
    h, k = tab.host, 0
    for b, cs in enumerate(crops):
        ens.host["first"][b], ens.host["count"][b] = k, len(cs)
        for j, (slot, c) in enumerate(cs):
            h["offset"][k], h["crop"][k] = offsets[slot], c.shape
            h["before"][k], h["padded"][k] = pad_before(c.shape, shape)
            h["affine"][k] = np.asarray(params["affine"][b][j], np.float64)[:3].reshape(12)
            k += 1
    return tab, ens, buf


def _ensemble_table(params, B):
    """The switches and the sphere / envelope parameters of the records."""
    t = _Ensembles(B)
    mask = np.asarray(params.get("mask", np.zeros(B, bool)), bool).reshape(-1)
    env = np.asarray(params.get("envelope", np.zeros(B, bool)), bool).reshape(-1)
    if mask.size != B or env.size != B:
        raise ValueError(f"params: one switch per ensemble of the batch of {B}")
    if np.any(env & ~mask):
        raise ValueError("an envelope needs the foreground mask")
    t.host["flags"] = np.where(mask, MASK, 0) | np.where(env, ENVELOPE, 0)
    if "radius" in params:
        t.host["radius"] = _per_ensemble(params["radius"], B, name="radius", dtype=np.int64)
        t.host["shift"] = _per_ensemble(params["centre"], B, 3, "centre", np.int64)
        if mask.any() and t.host["radius"][mask].min() < 0:
            raise ValueError("radius: not negative")
    if "ball" in params:
        ball = _per_ensemble(params["ball"], B, name="ball", dtype=np.int64)
        if env.any() and (ball[env].min() < 2 or ball[env].max() > 4):
            raise ValueError("ball: 2, 3 or 4")
        t.host["ball"] = np.clip(ball, 2, 4)
    return t


# ---- the stages on device tensors -----------------------------------------------------------------------------------------------

def _compose(tab, ens, buf, shape, dev):
    out = torch.empty((len(ens.host), 1) + shape, dtype=torch.uint8, device=dev)
    _lib.check_envelope(_lib.load().amx_labels_compose(_lib.ptr(buf), buf.numel(), *tab.args, len(tab.host), *ens.args, _lib.ptr(out),
                                                     len(ens.host), *shape, _lib.stream(dev)))
    return out


def _median(x, ens, require):
    out = torch.empty_like(x)
    _lib.check_envelope(_lib.load().amx_labels_median3(_lib.ptr(x), _lib.ptr(out), x.shape[0], *x.shape[2:], require, *ens.args, _lib.stream(x.device)))
    return out


def _check_grids(grids, B, S, dev):
    cs = [S // s for s in noise_scales(S)]
    if len(grids) != 3:
        raise ValueError(f"grids: one per noise scale (3; got {len(grids)})")
    out = []
    for g, c in zip(grids, cs):
        g = _stream.device_tensor(g, "grids", (torch.float32,), "data generation")
        if tuple(g.shape) != (B, 3, c, c, c) or g.device != dev:
            raise ValueError(f"grids: {(B, 3, c, c, c)} on {dev} (got {tuple(g.shape)} on {g.device})")
        out.append(g.contiguous())
    return out


def _sphere(grids, ens, S, dev):
    """The masks of the ensembles with MASK; the volumes of the others stay zero."""
    B = len(ens.host)
    out = torch.zeros((B, 1, S, S, S), dtype=torch.uint8, device=dev)
    gp = (ctypes.c_void_p * 3)(*[g.data_ptr() for g in grids])
    _lib.check_envelope(_lib.load().amx_labels_sphere_mask(gp, _lib.ptr(out), B, S, *ens.args, _lib.stream(dev)))
    return out


def _apply(lab, mask, ens):
    """In place on ``lab``; -> the maximum label per ensemble, int32 [B] on the device."""
    B, V, dev = lab.shape[0], lab[0].numel(), lab.device
    lib = _lib.load()
    nb = lib.amx_labels_scratch_bytes(B, V)
    sc = _lib.scratch(nb, dev)
    mx = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check_envelope(lib.amx_labels_apply_mask(_lib.ptr(lab), _lib.ptr(mask), _lib.ptr(mx), B, V, *ens.args, _lib.ptr(sc), nb, _lib.stream(dev)))
    return mx


def _envelope(lab, mask, mx, ens):
    _lib.check_envelope(_lib.load().amx_labels_envelope(_lib.ptr(lab), _lib.ptr(mask), _lib.ptr(mx), lab.shape[0], *lab.shape[2:], *ens.args,
                                                      _lib.stream(lab.device)))
    return lab


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device: the data generation runs on the GPU and has no host path (got {dev})")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _switch(on, B, name="on"):
    on = np.ones(B, bool) if on is None else np.ascontiguousarray(np.broadcast_to(np.asarray(on, bool), (B,)))
    return on


# ---- one public function per stage ---------------------------------------------------------------------------------------------

def compose_templates(templates, affine, shape, device="cuda:0"):
    """step1_generate_labels.py:69-95: per ensemble, template k (a host volume; cropped to its non-zero bounding box, padded to at
    least ``shape`` with the odd voxel in front, resampled through ``affine[b][k]`` [4, 4] float64 with scipy's ``order=0,
    mode='grid-wrap'``) writes label k wherever its sample is non-zero, in order, so the last one wins; only the ``[:D, :H, :W]``
    region is computed.  ``templates``: per ensemble a list of 1 .. 64 volumes.  -> uint8 [B, 1, D, H, W] on ``device``."""
    dev = _device(device)
    shape = tuple(int(s) for s in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"shape: (D, H, W) (got {shape})")
    params = dict(n_templates=[len(t) for t in templates], affine=affine)
    tab, ens, buf = _tables(templates, params, shape)
    with torch.cuda.device(dev):
        return _compose(tab.device(dev), ens.device(dev), torch.from_numpy(buf).to(dev), shape, dev)


def median3(volumes, on=None):
    """``skimage.filters.median`` with its defaults on uint8 [B, 1, D, H, W]: the exact median of the 3 x 3 x 3 neighbourhood, the
    border replicated.  ``on``: per ensemble whether it is filtered (default: all); the others are copied."""
    x = _volumes(volumes, "volumes")
    B = x.shape[0]
    ens = _Ensembles(B)
    ens.host["flags"] = np.where(_switch(on, B), MASK, 0)
    with torch.cuda.device(x.device):
        return _median(x, ens.device(x.device), MASK)


def deformed_sphere_mask(radius, centre, grids, side_length, on=None):
    """``~sample_corruption(...)`` of datagen_utils.py:371-447 per ensemble: 1 where the sphere of ``radius`` around
    ``side_length // 2 + centre`` is found by the nearest-neighbour, reflection-padded ``grid_sample`` of the displaced grid.
    ``grids``: per noise scale (side / 16, side / 8, side / 4) the coarse displacement [B, 3, n, n, n] float32 in voxels, already
    multiplied by its std, component 0 along W.  -> uint8 [B, 1, S, S, S]; ensembles with ``on`` false stay zero."""
    S = _cube((side_length,) * 3)
    if not grids:
        raise ValueError("grids: one per noise scale (3)")
    g0 = _stream.device_tensor(grids[0], "grids", (torch.float32,), "data generation")
    B, dev = g0.shape[0], g0.device
    grids = _check_grids(grids, B, S, dev)
    ens = _ensemble_table(dict(mask=_switch(on, B), radius=radius, centre=centre), B)
    with torch.cuda.device(dev):
        return _sphere(grids, ens.device(dev), S, dev)


def _pair(labels, mask):
    lab, m = _volumes(labels), _volumes(mask, "mask")
    if m.shape != lab.shape or m.device != lab.device:
        raise ValueError(f"mask: {tuple(lab.shape)} on the labels' device (got {tuple(m.shape)} on {m.device})")
    return lab, m


def apply_foreground_mask(labels, mask, on=None):
    """step1_generate_labels.py:115-116: ``label = mask ? label + 1 : 0`` per ensemble with ``on`` (default: all).
    -> (uint8 [B, 1, D, H, W], the maximum label per ensemble as int32 [B] on the device)."""
    lab, m = _pair(labels, mask)
    B = lab.shape[0]
    ens = _ensemble_table(dict(mask=_switch(on, B)), B)
    with torch.cuda.device(lab.device):
        out = lab.clone()
        return out, _apply(out, m, ens.device(lab.device))


def envelope(labels, mask, ball, max_label, on=None):
    """step1_generate_labels.py:123-138: ``label = 1 + max_label`` where ``dilation(mask, ball(r)) & ~erosion(mask, ball(r))``, with
    skimage's default border (scipy's ``reflect``).  ``ball``: 2, 3 or 4, one or one per ensemble; ``max_label``: int32 [B] on the
    device (``apply_foreground_mask``'s).  Every axis must be at least 9."""
    lab, m = _pair(labels, mask)
    B = lab.shape[0]
    if min(lab.shape[2:]) < MIN_ENVELOPE_AXIS:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"every axis must be at least {MIN_ENVELOPE_AXIS} (got {tuple(lab.shape[2:])})")
    mx = _stream.device_tensor(max_label, "max_label", (torch.int32,), "data generation")
    if tuple(mx.shape) != (B,) or mx.device != lab.device:
        raise ValueError(f"max_label: [{B}] on the labels' device (got {tuple(mx.shape)})")
    on = _switch(on, B)
    ens = _ensemble_table(dict(mask=on, envelope=on, ball=ball), B)
    with torch.cuda.device(lab.device):
        return _envelope(lab.clone(), m, mx.contiguous(), ens.device(lab.device))


# ---- the chain ----------------------------------------------------------------------------------------------------------------

def generate_labels(templates, params, device="cuda:0", grids=None):
    """``generate_label_ensemble`` for a batch: compose, median, and per ensemble's switches the foreground mask (deformed sphere,
    its median, applied) and the envelope.  ``templates``: per ensemble the host volumes of its template files in drawing order;
    ``params`` from ``draw_params``; ``grids`` as in ``deformed_sphere_mask`` (omitted: ``draw_noise`` draws them).  A stage that no
    ensemble has switched on is not launched; nothing is read back from the device.
    -> (uint8 [B, 1, S, S, S], the identifier per ensemble)."""
    dev = _device(device)
    S = int(params["side_length"])
    shape = (S, S, S)
    B = len(templates)
    mask_on = np.asarray(params["mask"], bool).reshape(-1)
    env_on = np.asarray(params["envelope"], bool).reshape(-1)
    if mask_on.any():
        _cube(shape)
        if grids is not None:
            grids = _check_grids(grids, B, S, dev)
    if env_on.any() and S < MIN_ENVELOPE_AXIS:
        raise _lib.AmxEnvelopeError(_lib.AMX_ERR_SHAPE, f"every axis must be at least {MIN_ENVELOPE_AXIS} (got {shape})")
    tab, ens, buf = _tables(templates, params, shape)
    with torch.cuda.device(dev):
        tab.device(dev), ens.device(dev)
        lab = _median(_compose(tab, ens, torch.from_numpy(buf).to(dev), shape, dev), ens, 0)
        if mask_on.any():
            if grids is None:
                grids = draw_noise(params, dev)
            mask = _median(_sphere(grids, ens, S, dev), ens, MASK)
            mx = _apply(lab, mask, ens)
            if env_on.any():
                _envelope(lab, mask, mx, ens)
    return lab, identifiers(params)
