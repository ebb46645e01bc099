"""numpy restatement of step 2 of the synthetic data generation, written from the definitions alone and
independent of anatomix_amd: the reference of tests/test_datagen*.py.  Every function takes ``dt`` (numpy float64 or float32) and
evaluates the same formulas in that type; the float32 evaluation's distance from the float64 one is the e32 of the tests' bound.
Parameters are what the device receives: rounded to float32 first.  The stages the segmentation chain already has come from
tests/_segaug_ref.py.  tests/test_datagen.py pins ``gmm`` and ``perlin`` to the reference's recorded outputs, ``low_resolution`` to
F.interpolate and ``spike`` to the FFT definition; MONAI is not available here."""
import numpy as np

import _segaug_ref as AR

f32 = AR.f32
SWITCH_NAMES = ("bias", "spike", "contrast", "smooth", "gibbs", "sharpen", "lowres")
PROB = dict(bias=0.98, spike=0.2, contrast=0.5, smooth=0.5, gibbs=0.5, sharpen=0.25, lowres=0.333)


def gmm(label_map, means, stds, z, zero_background, dt):
    """sample_gmm with its noise given: ``gmm_raw`` min-max normalised."""
    g = gmm_raw(label_map, means, stds, z, zero_background, dt)
    return (g - g.min()) / (g.max() - g.min())


def gmm_raw(label_map, means, stds, z, zero_background, dt):
    """Per sorted distinct label i, std[i] z + mean[i] (label 0 of the list skipped, i.e. 0, under ``zero_background``); clipped at 0."""
    labels = np.unique(label_map)
    m, s, z = f32(means, dt), f32(stds, dt), np.asarray(z).astype(dt)
    g = np.zeros(label_map.shape, dt)
    for i, lab in enumerate(labels):
        if i == 0 and zero_background:
            continue
        idx = label_map == lab
        g[idx] = s[i] * z[idx] + m[i]
    return np.maximum(g, dt(0))


def upsample_index(n, scale, cn):
    """torch's trilinear source index (align_corners=False) of the n output voxels of an axis, float32 as torch computes it:
    (lower neighbour, upper neighbour clamped to the last coarse point, weight of the upper one)."""
    rs = np.float32(1.0 / scale)
    src = np.maximum(rs * (np.arange(n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), cn - 1)
    return i0, np.minimum(i0 + 1, cn - 1), src - i0.astype(np.float32)


def _blend(x, axis, i0, i1, l1, dt):
    shp = [1, 1, 1]
    shp[axis] = -1
    l1 = l1.astype(dt).reshape(shp)
    return (dt(1) - l1) * np.take(x, i0, axis) + l1 * np.take(x, i1, axis)


def perlin(shape, scales, grids, dt):
    """draw_perlin_volume with its draws given: the sum over the scales of the trilinear upsample of ``grids[s]`` (shape
    ceil(shape / scale), already multiplied by its std); scale 1 adds the grid as it is (weights 1 and 0)."""
    out = np.zeros(shape, dt)
    for scale, g in zip(scales, grids):
        g = np.asarray(g).astype(dt)
        for axis in range(3):
            g = _blend(g, axis, *upsample_index(shape[axis], scale, g.shape[axis]), dt)
        out = out + g
    return out


def appearance(label_map, means, stds, z, zero_background, scales, grids, factor, dt):
    return gmm(label_map, means, stds, z, zero_background, dt) * (dt(1) + f32(factor, dt) * perlin(label_map.shape, scales, grids, dt))


def spike_fft(x, loc, k_intensity=None, factor=1.0):
    """KSpaceSpikeNoise by its definition, float64: k = fftshift(fftn(x)); log(|k| + 1e-10) at ``loc`` := k_intensity (None:
    factor * 2.5 * mean(log(|k| + 1e-10))), the phase kept; real(ifftn(ifftshift(.)))."""
    k = np.fft.fftshift(np.fft.fftn(np.asarray(x, np.float64)))
    log_abs, phase = np.log(np.abs(k) + 1e-10), np.angle(k)
    if k_intensity is None:
        k_intensity = float(np.float32(factor)) * 2.5 * log_abs.mean()
    k2 = k.copy()
    k2[tuple(loc)] = np.exp(float(k_intensity)) * np.exp(1j * phase[tuple(loc)])
    return np.fft.ifftn(np.fft.ifftshift(k2)).real


def spike(x, loc, k_intensity, factor, dt):
    """The same as one plane wave: x + Re(delta / N exp(2 pi i sum_a f_a r_a / n_a)), f_a = (loc_a - n_a // 2) mod n_a,
    delta = exp(k_intensity) exp(i phase) - k[f]; the phase argument reduced modulo n_a in integers."""
    x = np.asarray(x).astype(dt)
    ct = np.complex128 if dt == np.float64 else np.complex64
    k = np.fft.fftn(x).astype(ct)
    f = [(int(l) - n // 2) % n for l, n in zip(loc, x.shape)]
    kf = k[tuple(f)]
    if k_intensity is None:
        k_intensity = f32(factor, dt) * dt(2.5) * np.log(np.abs(k).astype(dt) + dt(1e-10)).mean(dtype=np.float64).astype(dt)
    else:
        k_intensity = f32(k_intensity, dt)
    mag = np.abs(kf).astype(dt)
    unit = kf / mag if mag > 0 else ct(1)
    delta = ((np.exp(dt(k_intensity)) * unit - kf) / dt(x.size)).astype(ct)
    turns = np.zeros(x.shape, dt)
    for a, n in enumerate(x.shape):
        shp = [1, 1, 1]
        shp[a] = -1
        turns = turns + (((f[a] * np.arange(n)) % n).astype(dt) / dt(n)).reshape(shp)
    ang = dt(2 * np.pi) * (turns - np.floor(turns))
    return x + (delta.real.astype(dt) * np.cos(ang) - delta.imag.astype(dt) * np.sin(ang))


def low_resolution_shape(shape, zoom):
    return tuple(max(int(round(n * float(zoom))), 1) for n in shape)


def lowres_index(n, t):
    """Per output voxel of an axis of n voxels resampled through t: the nearest-exact source voxels of its two low-resolution
    neighbours and the weight of the second.  float32 index arithmetic, as torch's."""
    sc, back = np.float32(t) / np.float32(n), np.float32(n) / np.float32(t)
    src = np.maximum(sc * (np.arange(n, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int64), t - 1)
    i1 = np.minimum(i0 + 1, t - 1)
    near = lambda j: np.minimum(np.floor((j.astype(np.float32) + np.float32(0.5)) * back).astype(np.int64), n - 1)   # noqa: E731
    return near(i0), near(i1), src - i0.astype(np.float32)


def low_resolution(x, zoom, dt):
    """SimulateLowResolution(nearest-exact down to int(round(n zoom)), trilinear align_corners=False up) as one 8-tap gather."""
    x = np.asarray(x).astype(dt)
    target = low_resolution_shape(x.shape, zoom)
    out = x
    for axis in (2, 1, 0):
        out = _blend(out, axis, *lowres_index(x.shape[axis], target[axis]), dt)
    return out


def tail(x, dt):
    """ThresholdIntensity(above=True, threshold=0), then ScaleIntensity."""
    return AR.scale_intensity(np.maximum(np.asarray(x).astype(dt), dt(0)), dt)


def chain_view(x, params, b, v, dt):
    """View v of sample b through the chain of get_transforms, from the appearance model's output ``x``."""
    on = {k: bool(params["on"][k][b][v]) for k in SWITCH_NAMES}
    shape = x.shape
    x = AR.scale_intensity(np.asarray(x).astype(dt), dt)
    if on["bias"]:
        x = x * np.exp(AR.bias_exponent(shape, params["coeff"][b][v], dt))
    if on["spike"]:
        x = spike(x, params["spike_loc"][b][v], None, params["spike_factor"][b][v], dt)
    if on["contrast"]:
        x = AR.adjust_contrast(x, params["gamma"][b][v], dt)
    if on["smooth"]:
        x = AR.gaussian(x, params["smooth_sigma"][b][v], dt)
    if on["gibbs"]:
        x = AR.gibbs(x, AR.gibbs_radius(params["gibbs_alpha"][b][v], shape), dt)
    if on["sharpen"]:
        x = AR.sharpen(x, params["sharpen_sigma1"][b][v], params["sharpen_sigma2"][b][v], params["sharpen_alpha"][b][v], dt)
    if on["lowres"]:
        x = low_resolution(x, params["zoom"][b][v], dt)
    return tail(x, dt)


def generate_view(label_map, params, b, v, z, grids, dt):
    """process_volume for view v of sample b with its fields given: the appearance model, then the chain."""
    x = appearance(label_map, params["means"][b][v], params["stds"][b][v], z, bool(params["zero_background"][b][v]), params["scales"],
                   grids, params["perl_mult_factor"], dt)
    return chain_view(x, params, b, v, dt)


def label_blobs(shape, labels, seed):
    """A label map of nested seeded blobs that uses every value of ``labels`` (uint8)."""
    r = np.random.RandomState(seed)
    x = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"))
    lab = np.full(shape, labels[0], np.uint8)
    for l in labels[1:]:
        c = [r.uniform(0.1, 0.9) * s for s in shape]
        rad = r.uniform(0.15, 0.4) * max(shape)
        lab[sum((x[a] - c[a]) ** 2 for a in range(3)) <= rad * rad] = l
    flat = lab.reshape(-1)
    flat[r.permutation(flat.size)[:len(labels)]] = labels          # every label present, wherever the blobs fell
    return lab


def replay_noise(label_map, seed, zero_background):
    """The standard-normal field sample_gmm consumes after ``torch.manual_seed(seed)``, in its order of draws: one ``rand(1)`` at the
    first label (which decides the zero background in the reference; the fixture forces the decision), one ``randn(count)`` per label
    that is not skipped.  0 where nothing is drawn.  float32 numpy."""
    import torch
    torch.manual_seed(int(seed))
    z = torch.zeros(label_map.shape)
    for i, lab in enumerate(np.unique(label_map)):
        if i == 0:
            torch.rand(1)
            if zero_background:
                continue
        idx = label_map == lab
        z[idx] = torch.randn(int(idx.sum()))
    return z.numpy()


def replay_grids(shape, scales, seed, max_std):
    """Per scale the coarse grid times its std as draw_perlin_volume draws them after ``torch.manual_seed(seed)``."""
    import torch
    torch.manual_seed(int(seed))
    out = []
    for scale in scales:
        coarse = tuple(int(np.ceil(n / scale)) for n in shape)
        std = max_std * torch.rand((1,), dtype=torch.float32) + 0
        out.append((std * torch.randn(coarse, dtype=torch.float32)).numpy())
    return out


def load_case(gold, name):
    """A fixture case as a dict; ``z`` is the full field (replayed from the seed where the fixture stores samples, and checked
    against them) and ``index`` the flat voxel indices of the stored outputs (None: all)."""
    c = {k: gold[f"{name}/{k}"] for k in ("labels", "means", "stds", "scales", "zero_background", "seed", "z", "gmm", "perlin", "view")}
    c["scales"] = tuple(int(s) for s in c["scales"])
    c["zero_background"] = bool(c["zero_background"])
    c["grids"] = [gold[f"{name}/grid_{s}"] for s in c["scales"]]
    c["index"] = gold[f"{name}/index"] if f"{name}/index" in gold else None
    if c["index"] is not None:
        z = replay_noise(c["labels"], int(c["seed"]), c["zero_background"])
        assert np.array_equal(z.reshape(-1)[c["index"]], c["z"]), "torch's CPU generator no longer replays the recorded noise"
        c["z"] = z
    return c


def at(a, index):
    return a if index is None else a.reshape(-1)[index]


# ---- the chain's test case: (16, 24, 32) with scales (4, 8), batch 3 ---------------------------------------------------------
CHAIN_SHAPE, CHAIN_SCALES = (16, 24, 32), (4, 8)
CHAIN_LABELS = ([0, 1, 2, 3], [0, 7, 255], [4, 9, 33, 120, 200])
_ALT = {k: i % 2 == 0 for i, k in enumerate(SWITCH_NAMES)}
_NOT_ALT = {k: not v for k, v in _ALT.items()}
_ON, _OFF = dict.fromkeys(SWITCH_NAMES, True), dict.fromkeys(SWITCH_NAMES, False)
# per sample (view 0, view 1)
PATTERNS = {"on": [(_ON, _ON)] * 3, "off": [(_OFF, _OFF)] * 3, "mixed": [(_ON, _ON), (_OFF, _OFF), (_ALT, _ALT)],
            "views_differ": [(_ALT, _NOT_ALT), (_NOT_ALT, _ALT), (_ON, _OFF)]}


def chain_case(draw_params, pattern):
    """(label maps [3] uint8, params, z [3, 2, D, H, W] float32, grids per scale [3, 2, *coarse] float32), seeded."""
    labs = [label_blobs(CHAIN_SHAPE, l, 300 + i) for i, l in enumerate(CHAIN_LABELS)]
    p = draw_params(np.random.RandomState(21), [np.unique(l) for l in labs], CHAIN_SHAPE, scales=CHAIN_SCALES)
    for b, pair in enumerate(PATTERNS[pattern]):
        for v, sw in enumerate(pair):
            for k, val in sw.items():
                p["on"][k][b, v] = val
    r = np.random.RandomState(22)
    z = r.standard_normal((3, 2) + CHAIN_SHAPE).astype(np.float32)
    grids = [(r.standard_normal((3, 2) + tuple(n // s for n in CHAIN_SHAPE)) * p["perl_std"][:, :, i, None, None, None]).astype(np.float32)
             for i, s in enumerate(CHAIN_SCALES)]
    return labs, p, z, grids


def chain_reference(case):
    """Per (sample, view), in row order: (ref64, e32) of generate_view."""
    labs, p, z, grids = case
    out = []
    for b in range(len(labs)):
        for v in range(2):
            a, c = (generate_view(labs[b], p, b, v, z[b, v], [g[b, v] for g in grids], dt) for dt in (np.float64, np.float32))
            out.append((a, float(np.abs(c.astype(np.float64) - a).max() / np.abs(a).max())))
    return out


BOUND = lambda e32: 5e-6 + 10 * e32      # noqa: E731  the project's rule (tests/test_seg_augment_gpu.py::check_image)


def uint8_band(ref64, bound):
    """Voxels where trunc(255 ref64) may legitimately differ by one: 255 ref64 within 255 bound of an integer >= 1."""
    y = 255.0 * ref64
    near = np.rint(y)
    return (np.abs(y - near) <= 255.0 * bound) & (near >= 1)
