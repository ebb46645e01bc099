"""Host checks of the backward walk (tests/_backward_walk.py): a torch fp32 emulation of the library's training operators, with
the rounding points of the 16-bit path, stands in for ``anatomix_amd.model.train_ops`` so that the REAL backward of
anatomix_amd/model/train.py runs on the CPU under the recorder.  The emulation must pass the walk, must give the parameter gradients
of oracle/train_lowp.py, its excluded-voxel share must stay under the cap, its k is measured here -- and every planted defect must
fail at its stage and module."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import _backward_walk as BW
import anatomix_amd
from anatomix_amd.model import train as TR
from oracle import train_lowp as TL
from oracle import unet_ref as R

SIZE = (8, 12, 40)
KW_BN = dict(dimension=3, input_nc=1, output_nc=16, num_downs=2, ngf=16)
LAYERS_BN = [6, 9, 13, 24, 31]                    # conv ids (pre-norm taps), a pool id
KW_IN = dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance", pooling="Avg", interp="trilinear", norm_eps=1e-2)
LAYERS_IN = [3, 13, 20, 23, 27, 34]               # ... and an upsample id


# ---- the emulated operators ----------------------------------------------------------------------------------------------------

def _cl(t, dt):                                   # fp32 NCDHW -> 16-bit NDHWC (THE rounding point)
    return t.permute(0, 2, 3, 4, 1).to(dt).contiguous()


def _nc(t):                                       # 16-bit NDHWC -> fp32 NCDHW
    return t.float().permute(0, 4, 1, 2, 3).contiguous()


def _pad16(t):
    c = t.shape[1]
    return t if c % 16 == 0 else F.pad(t, (0, 0) * 3 + (0, 16 - c % 16))


def _act(y, act, slope):
    return F.relu(y) if act == "relu" else F.leaky_relu(y, slope) if act == "lrelu" else y


def _fold(P, defect=None):
    """fp32 reflect-padding adjoint on the framed domain [N, C, D+4, H+4, W+4] -> [N, C, D, H, W]."""
    if defect == "fold_dh_swapped":               # the buffer read as [H+4][D+4] rows
        n, c, df, hf, wf = P.shape
        return _fold(P.reshape(n, c, hf, df, wf)).reshape(n, c, df - 4, hf - 4, wf - 4)
    out = P
    for ax in (2, 3, 4):
        L = out.shape[ax] - 4
        core = out.narrow(ax, 2, L).clone()
        if not (defect == "fold_z1_missing" and ax == 2):
            core.narrow(ax, 1, 1).add_(out.narrow(ax, 1, 1))
        core.narrow(ax, L - 2, 1).add_(out.narrow(ax, L + 2, 1))
        out = core
    return out


def _children(t, defect=None):
    n, c, d, h, w = t.shape
    t = t.reshape(n, c, d // 2, 2, h // 2, 2, w // 2, 2)
    if defect == "child_missing":
        t = t.clone()
        t[:, :, :, 1, :, 0, :, 1] = 0
    return t.sum((3, 5, 7))


def _vjp(fn, x, g):
    with torch.enable_grad():                     # (called inside an autograd Function's backward)
        x = x.detach().requires_grad_(True)
        return torch.autograd.grad(fn(x), x, g)[0]


def make_emulation():
    """A stand-in for ``train_ops``: same functions, CPU tensors, fp32 arithmetic, 16-bit stores.  ``E.defect = (name, module)`` plants
    one defect while the recorder reports that module as the current one (``E.current``)."""
    E = SimpleNamespace(defect=None, current=None, _CACHE={})
    on = lambda name: E.defect is not None and E.defect[0] == name and E.defect[1] == E.current

    def conv_raw(x0, x1, weight, weight_mode):
        xin = _nc(x0) if x1 is None else torch.cat((_nc(x0), _nc(TR._nearest_up2(x1))), 1)
        w = weight.detach().float().to(x0.dtype).float()
        if weight_mode == 1:
            w = w.transpose(0, 1).flip(2, 3, 4)
        return F.conv3d(F.pad(xin[:, :w.shape[1]], (1,) * 6, mode="reflect"), w)

    def conv_forward(x0, x1, weight, act="none", slope=0.3, out32=False, shift=None, weight_mode=0, wpk=None):
        z = conv_raw(x0, x1, weight, weight_mode)
        if shift is not None:
            z = z + shift.float().view(1, -1, 1, 1, 1)
        z = _pad16(_act(z, act, slope))
        return z if out32 else _cl(z, x0.dtype)

    def bn_train_forward(x, gamma, beta, eps, act="relu", slope=0.3, running_mean=None, running_var=None, momentum=0.1, out=None):
        xf = x.float()
        c = xf.shape[-1]
        mean = xf.double().mean((0, 1, 2, 3)).float()
        var = (xf.double() - mean.double()).square().mean((0, 1, 2, 3)).float()
        rstd = (var + eps).rsqrt()
        a = rstd if gamma is None else gamma.float() * rstd
        b = -mean * a if beta is None else beta.float() - mean * a
        y = _act(xf * a + b, act, slope).to(x.dtype)
        if running_mean is not None:
            m = xf[..., 0].numel()
            running_mean.mul_(1 - momentum).add_(momentum * mean[:running_mean.numel()])
            running_var.mul_(1 - momentum).add_(momentum * var[:running_var.numel()] * m / (m - 1))
        if out is not None:
            out.copy_(y)
            y = out
        return y, mean, rstd

    def new_framed(n, d, h, w, c, dtype, device):
        return torch.zeros((n, d + 4, h + 4, w + 4, c), dtype=dtype, device=device)

    def shared_framed(n, d, h, w, c, dtype, device):
        key = ("frame", device, n, d, h, w, c, dtype)
        if key not in E._CACHE:
            E._CACHE[key] = new_framed(n, d, h, w, c, dtype, device)
        return E._CACHE[key]

    def interior(fr):
        return fr[:, 2:-2, 2:-2, 2:-2, :]

    def bn_act_backward(dy, y, x, mean, rstd, gamma, act="relu", slope=0.3, framed=None, beta=None, recompute=False):
        g = dy.float()
        one = torch.ones_like(g)
        d1 = lambda u: one if act == "none" else torch.where(u > 0, one, (slope if act == "lrelu" else 0.0) * one)
        if mean is None:
            interior(framed).copy_((g * d1(y.float())).to(dy.dtype))
            return framed, None, None
        xf = x.float()
        a = rstd if gamma is None else gamma.float() * rstd
        b = -mean * a if beta is None else beta.float() - mean * a
        g = g * d1(xf * a + b)
        xh = (xf - mean) * rstd
        m = xf[..., 0].numel()
        dbeta = g.sum((0, 1, 2, 3))
        dgamma = (g * (_act(xf * a + b, act, slope) if on("dgamma_with_y") else xh)).sum((0, 1, 2, 3))
        dgx = (g * xh).sum((0, 1, 2, 3))
        interior(framed).copy_((a * (g - dbeta / m - xh * dgx / m)).to(dy.dtype))
        if on("frame_border"):
            framed[0, 1, 3, 3, 0] = 1.0
        return framed, dgamma, dbeta

    def conv_dgrad_framed(fr, weight, wpk=None):
        return conv_forward(fr, None, weight, weight_mode=1)

    def pad_fold(g, accumulate_into=None):
        f = _fold(_nc(g), "fold_dh_swapped" if on("fold_dh_swapped") else "fold_z1_missing" if on("fold_z1_missing") else None)
        if accumulate_into is None:
            return _cl(f, g.dtype)
        accumulate_into.copy_(_cl(_nc(accumulate_into) + f, g.dtype))
        return accumulate_into

    def conv_dgrad(fr, weight, cin_keep=None, accumulate_into=None):
        return pad_fold(conv_dgrad_framed(fr, weight), accumulate_into)

    def dgrad_direct_supported(fr, weight):
        # the shapes test_direct_data_gradient_equals_the_framed_route pins for the device's answer
        n, df, hf, wf, c = fr.shape
        cin, cout = c, (weight.shape[1] + 15) // 16 * 16
        return cin in (16, 32) and cout in (16, 32) and not (cout == 32 and cin == 16) and wf - 4 >= 32 and df - 4 >= 8 and hf - 4 >= 8

    def conv_dgrad_direct(fr, weight, wpk=None):
        P = _pad16(conv_raw(fr, None, weight, 1))                           # fp32 on the framed domain, never stored
        inner = P[:, :, 2:-2, 2:-2, 2:-2]
        out = inner.to(fr.dtype)                                            # the interior launch's store
        shell = _fold(P) - inner
        nf = BW._near_face(inner.shape)
        out = torch.where(nf, (out.float() + shell).to(fr.dtype), out)       # the shell launch: read back, add, store
        if on("direct_last_column"):
            out[0, :, 2:6, :, -1] = 0
        return out.permute(0, 2, 3, 4, 1).contiguous()

    def conv_wgrad(fr, x0, x1, cin_real, cout, out=None, accumulate=False):
        xin = _nc(x0) if x1 is None else torch.cat((_nc(x0), _nc(TR._nearest_up2(x1))), 1)
        xin = xin[:, :cin_real]
        G = _nc(interior(fr))[:, :cout]
        xp = F.pad(xin, (1,) * 6, mode="reflect")
        dw = torch.nn.grad.conv3d_weight(xp, (cout, cin_real, 3, 3, 3), G)
        if on("wgrad_unpadded_face"):                                        # tap kz = 0 reads x[0] for x[-1] instead of the reflected x[1]
            xr = xp.clone()
            xr[:, :, 0] = xp[:, :, 1]
            dw[:, :, 0, 1, 1] = torch.nn.grad.conv3d_weight(xr, (cout, cin_real, 3, 3, 3), G)[:, :, 0, 1, 1]
        if out is not None:
            out.copy_(out + dw if accumulate else dw)
            return out
        return dw

    def pool2(x, mode):
        return _cl((F.avg_pool3d if mode else F.max_pool3d)(_nc(x), 2), x.dtype)

    def pool2_max_backward(dp, inp, accumulate_into=None):
        x = _nc(inp)
        if on("pool_last_max"):                                              # the mirrored volume's first maximum is this one's last
            g = _vjp(lambda t: F.max_pool3d(t, 2), x.flip(2, 3, 4), _nc(dp).flip(2, 3, 4)).flip(2, 3, 4)
        else:
            g = _vjp(lambda t: F.max_pool3d(t, 2), x, _nc(dp))
        if accumulate_into is None or on("skip_overwritten"):
            res = _cl(g, dp.dtype)
            if accumulate_into is None:
                return res
            accumulate_into.copy_(res)
            return accumulate_into
        accumulate_into.copy_(_cl(_nc(accumulate_into) + g, dp.dtype))
        return accumulate_into

    def upsample2_trilinear(x):
        return _cl(F.interpolate(_nc(x), scale_factor=2, mode="trilinear"), x.dtype)

    def upsample2_trilinear_backward(g):
        n, d, h, w, c = g.shape
        z = torch.zeros(n, c, d // 2, h // 2, w // 2)
        return _cl(_vjp(lambda t: F.interpolate(t, scale_factor=2, mode="trilinear"), z, _nc(g)), g.dtype)

    def export_ncdhw(x):
        return _nc(x)

    def import_ncdhw(g, dst, accumulate=False):
        c = g.shape[1]
        if accumulate and on("tap_not_added"):
            return dst
        v = g.float().permute(0, 2, 3, 4, 1)
        dst[..., :c] = ((dst[..., :c].float() + v) if accumulate else v).to(dst.dtype)
        return dst

    def upcat_split_backward_framed(g, c0, c1, skip_into=None):
        f = _fold(_nc(g))
        dlow = _cl(_children(f[:, c0:c0 + c1], "child_missing" if on("child_missing") else None), g.dtype)
        if c0 == 0:
            return None, dlow
        if skip_into is None:
            return _cl(f[:, :c0], g.dtype), dlow
        skip_into.copy_(_cl(_nc(skip_into) + f[:, :c0], g.dtype))
        return skip_into, dlow

    E.__dict__.update(conv_forward=conv_forward, bn_train_forward=bn_train_forward, new_framed=new_framed, shared_framed=shared_framed,
                      interior=interior, bn_act_backward=bn_act_backward, conv_dgrad=conv_dgrad, conv_dgrad_framed=conv_dgrad_framed,
                      dgrad_direct_supported=dgrad_direct_supported, conv_dgrad_direct=conv_dgrad_direct, pad_fold=pad_fold,
                      wgrad_scratch=lambda *a: None, conv_wgrad=conv_wgrad, pool2=pool2, pool2_max_backward=pool2_max_backward,
                      upsample2_trilinear=upsample2_trilinear, upsample2_trilinear_backward=upsample2_trilinear_backward,
                      export_ncdhw=export_ncdhw, import_ncdhw=import_ncdhw, upcat_split_backward_framed=upcat_split_backward_framed,
                      _as_weight=lambda w: w.detach().float().contiguous(), pack_batch=lambda reqs, dt, dev: [None] * len(reqs))
    return E


# ---- running the real backward on the emulated operators ----------------------------------------------------------------------------

def run(kw, layers, precision, defect=None, seed=3, scale=4096.0, x_grad=False):
    """(recorder, model, out, taps, cotangents) of one forward + backward of train.py on the emulated operators."""
    E = make_emulation()
    E.defect = defect
    real, TR.T = TR.T, E
    try:
        net = anatomix_amd.Unet(**kw)
        net.load_state_dict(R.synthetic_state_dict(kw, seed, gain=2 ** 0.5), strict=True)
        net.precision = precision
        net.train()
        x = R.synthetic_input(11, 2, SIZE).requires_grad_(x_grad)
        final = len(net.model) - 1
        out, feats = TR.forward_train(net, x, sorted(set(layers) | {final}))
        feats = feats[:-1]
        g = torch.Generator().manual_seed(5)
        cots = [torch.randn(f.shape, generator=g) / f[0].numel() ** 0.5 for f in feats]
        loss = 0.1 * out.square().mean() + sum((f * c).sum() for f, c in zip(feats, cots))
        with BW.Recorder(TR, on_block=lambda idx: setattr(E, "current", idx)) as rec:
            (loss * scale).backward()
    finally:
        TR.T = real
    return rec, net, x, cots, E


K_FREE = {s: 0.0 for s in BW.K_SMALL}             # tol = R alone: k_needed then says what the emulation needs


@pytest.fixture(scope="module")
def clean():
    """The undisturbed runs, shared: (network, precision) -> (recorder, records judged with K_EMUL, model, x, cotangents)."""
    out = {}
    for name, kw, layers in (("bn", KW_BN, LAYERS_BN), ("in", KW_IN, LAYERS_IN)):
        for prec in ("f16", "bf16"):
            rec, net, x, cots, E = run(kw, layers, prec, x_grad=name == "in")
            out[name, prec] = (rec, BW.walk(rec, prec, BW.K_EMUL), net, x, cots, E)
    return out


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["bn", "in"])
def test_emulation_passes_the_walk(clean, name, prec):
    rec, recs, net, _, _, E = clean[name, prec]
    print(BW.report(recs))
    assert all(r.ok for r in recs), BW.report([r for r in recs if not r.ok])
    steps = TR.plan_network(net, [])
    want = {s.idx for s in steps if isinstance(s, (TR.ConvBlock, TR.Pool))}
    got = {r.module for r in recs if r.stage != "uptap"}
    assert got == want, (sorted(got), sorted(want))
    assert max(r.excluded for r in recs) <= BW.EXCLUDE_CAP
    routes = {b.route for b in rec.blocks.values()}
    assert routes == ({"stem", "direct", "fold", "upcat", "split48"} if name == "bn" else {"stem", "direct", "fold"}), routes
    for key, fr in E._CACHE.items():
        inner = fr.clone()
        inner[:, 2:-2, 2:-2, 2:-2] = 0
        assert not inner.any(), key


def test_emulation_k_is_what_the_module_states(clean):
    """The k the emulation needs, per stage kind: measured with tol = R alone.  _backward_walk.K_SMALL states it."""
    worst_k, worst_r = {}, {}
    for (name, prec), (rec, _, _, _, _, _) in clean.items():
        for r in BW.walk(rec, prec, K_FREE):
            if r.stage in BW.K_EMUL:
                worst_k[r.stage] = max(worst_k.get(r.stage, 0.0), r.k_needed)
                worst_r[r.stage, prec] = max(worst_r.get((r.stage, prec), 0.0), r.r_ratio)
    print("k needed by the emulation", worst_k)
    print("worst err / R", {k: round(v, 3) for k, v in worst_r.items()})
    assert set(worst_k) == set(BW.K_EMUL)
    for s, v in worst_k.items():
        assert v <= BW.K_SMALL[s] <= 1.01 * v + 1e-3, (s, v)         # covered, and not padded
        assert BW.K_EMUL[s] == max(BW.K_SMALL[s], BW.K_WALKED[s])


def test_emulation_gives_the_gradients_of_train_lowp(clean):
    """Same rounding points, same graph: the recorded parameter gradients against oracle/train_lowp.py, teacher-forced with the stored
    tensors (bounds: tests/test_train_step_gpu.py LOWP_BOUNDS, f16)."""
    rec, _, net, x, cots, _ = clean["bn", "f16"]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    forced = {}
    for b in rec.blocks.values():
        if b.X is not None:
            forced[b.module] = b.X.float().permute(0, 4, 1, 2, 3)
            forced[b.module + 2] = b.Y.float().permute(0, 4, 1, 2, 3)
    scale = 4096.0
    ref, _, _ = TL.parameter_gradients(x.detach(), sd, KW_BN, LAYERS_BN, [c * scale for c in cots], out_weight=0.1 * scale,
                                       lowp=torch.float16, forced=forced)
    n = 0
    for k, p in net.named_parameters():
        a, b = p.grad.double(), ref[k].double()
        e = float((a - b).norm() / b.norm().clamp_min(1e-30))
        assert e <= (2e-3 if a.dim() > 1 else 2e-2), (k, e)
        n += 1
    assert n == len(ref) and n > 30


def _first(rec, route=None, kind=None, pick=0, where=lambda b: True):
    ids = [i for i in rec.order if i in rec.blocks and (route is None or rec.blocks[i].route == route)
           and (kind is None or rec.blocks[i].kind == kind) and where(rec.blocks[i])]
    return ids[pick]


DEFECTS = [
    # (defect, network, how the module is chosen from the clean run, stage it must fail at)
    ("fold_dh_swapped", "bn", lambda r: _first(r, "fold"), "dgrad"),
    ("fold_z1_missing", "bn", lambda r: _first(r, "fold", pick=1), "dgrad"),
    ("pool_last_max", "bn", lambda r: min(r.pools), "pool"),
    ("child_missing", "bn", lambda r: _first(r, "upcat"), "dgrad"),
    ("dgamma_with_y", "bn", lambda r: _first(r, "direct", kind="norm"), "vec"),
    ("tap_not_added", "bn", lambda r: _first(r, where=lambda b: b.conv_tap is not None and b.dy is not None), "norm"),
    ("skip_overwritten", "bn", lambda r: max(r.pools), "pool"),
    ("frame_border", "bn", lambda r: _first(r, "upcat"), "frame"),
    ("direct_last_column", "bn", lambda r: _first(r, "direct"), "dgrad"),
    ("wgrad_unpadded_face", "bn", lambda r: _first(r, "fold"), "wgrad"),
]


@pytest.mark.parametrize("defect,net,choose,stage", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_fails_at_its_stage_and_module(clean, defect, net, choose, stage):
    module = choose(clean[net, "f16"][0])
    kw, layers = (KW_BN, LAYERS_BN) if net == "bn" else (KW_IN, LAYERS_IN)
    rec, *_ = run(kw, layers, "f16", defect=(defect, module))
    recs = BW.walk(rec, "f16", BW.K_GPU)                       # the bound the device is held to
    bad = [(r.module, r.stage) for r in recs if not r.ok]
    print(BW.report([r for r in recs if not r.ok]))
    assert bad and bad[0] == (module, stage), (module, stage, bad)
    if defect != "frame_border":                               # (a dirty frame stays dirty for every later block of that shape)
        assert set(bad) == {(module, stage)}, bad


def measure_k_at_walked_shapes():
    """_backward_walk.K_WALKED: the emulation's k on the 6M network at the shapes test_backward_walk_gpu.py walks (not a test: a minute)."""
    import numpy as np
    kw = R.VARIANTS["anatomix"]
    worst = {}
    for prec, batch, size in (("f16", 2, (32, 48, 80)), ("bf16", 2, (32, 48, 80)), ("f16", 1, (48, 32, 128)), ("bf16", 3, (32, 64, 32))):
        E = make_emulation()
        real, TR.T = TR.T, E
        try:
            net = anatomix_amd.Unet(**kw)
            net.load_state_dict(R.synthetic_state_dict(kw, 3, gain=2 ** 0.5), strict=True)
            net.precision = prec
            net.train()
            x = torch.from_numpy(np.random.RandomState(3).rand(batch, 1, *size).astype(np.float32))
            out, feats = TR.forward_train(net, x, [27, 31, 38, 45, 52])
            g = torch.Generator().manual_seed(5)
            loss = 0.1 * out.square().mean() + sum((f * (torch.randn(f.shape, generator=g) / f[0].numel() ** 0.5)).sum() for f in feats)
            with BW.Recorder(TR) as rec:
                (loss * (1024.0 if prec == "f16" else 1.0)).backward()
        finally:
            TR.T = real
        for r in BW.walk(rec, prec, K_FREE):
            if r.stage in K_FREE and r.k_needed > worst.get(r.stage, (0.0,))[0]:
                worst[r.stage] = (r.k_needed, prec, batch, size, r.module, r.route)
        print(prec, batch, size, {s: round(v[0], 4) for s, v in worst.items()}, flush=True)
    print(worst)


if __name__ == "__main__":
    measure_k_at_walked_shapes()
