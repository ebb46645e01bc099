"""GPU: the blocks' linear layers under autograd on the library's own kernels (``train_linear = "hip"``: amx_linear_forward +
amx_linear_backward, csrc/amx_linear_bwd.hip) against the float64 emulation of their three rounding points and against float64
autograd of F.linear (tests/_linear_ref.py)."""
import copy

import pytest
import torch

import _linear_ref as R
from _util import rel_l2
from _vit_walk import U32, c_f16
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.model.vit3d.architectures import _LinearFn
from oracle import vit_ref as V

pytestmark = pytest.mark.gpu
IDS = [str(s) for s in R.SHAPES]


def _forward(dev, x, w, b):
    lib = _lib.load()
    (N, K), M = w.shape, x.numel() // w.shape[1]
    y = torch.empty(M, N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nb = lib.amx_linear_train_scratch_bytes(M, K, N)
        assert nb > 0
        sc = _lib.scratch(nb, dev)
        _lib.check(lib.amx_linear_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), M, K, N, _lib.ptr(y), _lib.ptr(sc), nb, _lib.stream(dev)))
    return y


def _backward(dev, x, w, dy, outs=("dx", "dw", "db")):
    """{name: gradient} of one amx_linear_backward call; names missing from ``outs`` are passed as null."""
    lib = _lib.load()
    (N, K), M = w.shape, x.numel() // w.shape[1]
    new = lambda name, *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev) if name in outs else None
    g = dict(dx=new("dx", M, K), dw=new("dw", N, K), db=new("db", N))
    with torch.cuda.device(dev):
        nb = lib.amx_linear_train_scratch_bytes(M, K, N)
        sc = _lib.scratch(nb, dev)
        _lib.check(lib.amx_linear_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(dy), M, K, N, _lib.ptr(g["dx"]), _lib.ptr(g["dw"]),
                                           _lib.ptr(g["db"]), _lib.ptr(sc), nb, _lib.stream(dev)))
    return g


def _on(dev, idx):
    return [None if t is None else t.to(dev) for t in R.case(idx)[0]]


def _check_against_emulation(tag, got, emu, S, exact, M, K, N):
    """Check 1, nothing excluded: y, dx, dw per element within c_f16(L) S of the emulation (L = K, N, M: the reduction length); db
    within M 2^-24 sum |dy| of float64 (fp32 summation in any order).  Returns the failures; prints the worst err / tol."""
    failures = []
    for name, L in (("y", K), ("dx", N), ("dw", M), ("db", None)):
        if got.get(name) is None:
            continue
        assert torch.isfinite(got[name]).all(), (tag, name)
        ref, tol = (emu[name], c_f16(L) * S[name]) if L else (exact[name], M * U32 * S[name])
        ratio = ((got[name].double().cpu().reshape(ref.shape) - ref).abs() / tol.clamp_min(1e-300)).max().item()
        print(f"{tag} {name}: worst err / tol = {ratio:.3f}")
        if not ratio <= 1.0:
            failures.append((tag, name, ratio))
    return failures


@pytest.mark.parametrize("idx", range(len(R.SHAPES)), ids=IDS)
def test_every_element_against_the_emulation_and_float64(device, idx):
    """Checks 1 and 2 through the C ABI.  Against float64 every tensor is below 1e-3 rel-L2 and 4e-3 max-norm (the forward core's
    bars).

    Measured on an MI355X, worst err / tol over the six shapes: y 0.051, dx 0.044, dw 0.026 (all three largest at the small shapes,
    where few terms average out), db 0.013.  Against float64 (rel-L2 / max-norm): y 2.3-2.9e-4 / 2.4-3.9e-4, dx 2.7-3.0e-4 /
    2.7-3.4e-4, dw 2.7-3.0e-4 / 2.7-3.7e-4, db 0.4-1.1e-7 / 0.3-1.4e-7 -- the emulation's own error: what is left is the three
    roundings."""
    M, K, N, _ = R.SHAPES[idx]
    x, w, b, dy = _on(device, idx)
    _, exact, emu, S = R.case(idx)
    got = dict(_backward(device, x, w, dy, ("dx", "dw", "db") if b is not None else ("dx", "dw")), y=_forward(device, x, w, b))
    failures = _check_against_emulation(IDS[idx], got, emu, S, exact, M, K, N)
    for name in ("y", "dx", "dw", "db"):
        if exact[name] is None:
            continue
        e, m = R.errors(got[name], exact[name])
        print(f"{IDS[idx]} {name}: rel-L2 {e:.2e} max-norm {m:.2e} against float64")
        if not (e < 1e-3 and m < 4e-3):
            failures.append((name, e, m))
    assert not failures, failures


def test_autograd_function_on_a_batched_input(device):
    """The chunked shape through ``_LinearFn`` with x as [2, 1050, 132]: the same bits as the C ABI on the flat matrix."""
    idx = len(R.SHAPES) - 1
    x, w, b, dy = _on(device, idx)
    want = dict(_backward(device, x, w, dy), y=_forward(device, x, w, b))
    xb, wb, bb = [t.detach().clone().requires_grad_(True) for t in (x.view(*R.M5_LEADING, -1), w, b)]
    y = _LinearFn.apply(xb, wb, bb)
    assert y.shape == (*R.M5_LEADING, w.shape[0]) and torch.equal(y.reshape(want["y"].shape), want["y"])
    dx, dw, db = torch.autograd.grad(y, [xb, wb, bb], dy.view(*R.M5_LEADING, -1))
    assert dx.shape == xb.shape and torch.equal(dx.reshape(want["dx"].shape), want["dx"])
    assert torch.equal(dw, want["dw"]) and torch.equal(db, want["db"])


def test_null_outputs_bias_none_and_a_strided_gradient(device):
    x, w, b, dy = _on(device, 0)
    base = _backward(device, x, w, dy)
    for outs in (("dx",), ("dw",), ("db",), ("dx", "db"), ("dw", "db"), ("dx", "dw")):
        part = _backward(device, x, w, dy, outs)
        for name in ("dx", "dw", "db"):
            if name in outs:
                assert torch.equal(part[name], base[name]), (outs, name)
            else:
                assert part[name] is None
    # bias=None: the forward without the bias, no bias gradient
    y0 = _forward(device, x, w, None)
    assert torch.equal(y0, _forward(device, x, w, torch.zeros_like(b)))
    xr, wr = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    y = _LinearFn.apply(xr, wr, None)
    assert torch.equal(y, y0)
    # a non-contiguous incoming gradient
    strided = torch.empty(dy.shape[1], dy.shape[0], device=device).t()
    strided.copy_(dy)
    assert not strided.is_contiguous()
    dx, dw = torch.autograd.grad(y, [xr, wr], strided)
    assert torch.equal(dx, base["dx"]) and torch.equal(dw, base["dw"])
    # only the weight asks for a gradient: dx is not computed
    wr2 = w.detach().clone().requires_grad_(True)
    _LinearFn.apply(x, wr2, b).backward(dy)
    assert torch.equal(wr2.grad, base["dw"])
    # outside the envelope: refused before any launch, naming the shape
    with pytest.raises(_lib.AmxError, match=r"\(5, 6, 4\)"):
        _LinearFn.apply(torch.zeros(5, 6, device=device), torch.zeros(4, 6, device=device, requires_grad=True), None)


def test_backward_is_deterministic(device):
    idx = len(R.SHAPES) - 1
    x, w, b, dy = _on(device, idx)
    a, c = _backward(device, x, w, dy), _backward(device, x, w, dy)
    for name in ("dx", "dw", "db"):
        assert torch.equal(a[name], c[name]), name
    assert torch.equal(_forward(device, x, w, b), _forward(device, x, w, b))


def test_scale_of_the_incoming_gradient(device):
    """One power of two per call, found on the device: dy x 2^-20 and dy x 2^12 give the same bits times that power; a zero dy gives
    exact zeros; rows of dy 2^16 apart (the small rows land among the f16 subnormals once the large ones are normalised) still meet
    check 1 -- a flush of f16 subnormals would not.  Measured worst err / tol there: dx 0.074, dw 0.038, db 0.011."""
    idx = 0
    M, K, N, _ = R.SHAPES[idx]
    x, w, b, dy = _on(device, idx)
    base = _backward(device, x, w, dy)
    for p in (-20, 12):
        scaled = _backward(device, x, w, dy * 2.0 ** p)
        for name in ("dx", "dw", "db"):
            assert torch.equal(scaled[name], base[name] * 2.0 ** p), (p, name)
    zero = _backward(device, x, w, torch.zeros_like(dy))
    for name in ("dx", "dw", "db"):
        assert torch.equal(zero[name], torch.zeros_like(zero[name])), name
    cx, cw, cb, cdy = R.case(idx)[0]
    rows = torch.where(torch.rand(M, generator=torch.Generator().manual_seed(3)) < 0.5, 1.0, 2.0 ** -16)[:, None]
    wide = cdy * rows
    emu, S = R.emulated(cx, cw, cb, wide)
    sub = (wide * 2.0 ** -R.exponent(wide)).abs()
    assert ((sub > 0) & (sub < 2.0 ** -14)).sum() > 1000          # the case does reach the subnormals
    got = _backward(device, x, w, wide.to(device))
    failures = _check_against_emulation("rows 2^16 apart", got, emu, S, R.exact(cx, cw, cb, wide), M, K, N)
    assert not failures, failures


def test_module_wiring_of_train_linear(device):
    """PrimusV2 (32^3 input, depth 2, width 132, 2 heads) with loss y.square().mean() and train_attention = "torch": every parameter
    gradient under train_linear = "hip" and under "torch", each in rel-L2 against float64 CPU autograd of the same module.  Per
    parameter the "hip" error is at most 3 x the yardstick, and the yardstick is the larger of two errors: the torch route's own
    error against float64 for that parameter (the reference route) and f16's unit roundoff 2^-11 = 4.9e-4, the relative error
    one rounding of an operand may introduce; 3 x because two independently rounded operands (and the sum of their effects along
    the path) feed every gradient.  A wiring error -- a transposed weight, a dropped bias, a wrong row count -- gives errors of
    order 1.  Measured on an MI355X: the largest ratio err_hip / yardstick is 2.14 (eva.blocks.1.attn.q_norm.weight).

    The eight biases whose gradient is mathematically zero (a per-channel constant in front of InstanceNorm or ChannelDemean) are
    judged as zero to rounding on both routes, as in test_attention_train_gpu.py: |g| <= 1e-4 x the largest gradient of the same
    layer's weight."""
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=(32, 32, 32), eva_depth=2, embed_dim=132, eva_numheads=2)
    sd = V.synthetic_state_dict(kw, 1)
    m = PrimusV2(**kw)
    m.load_state_dict(sd, strict=True)
    x = V.synthetic_input(5, 2, (32, 32, 32))
    ref = copy.deepcopy(m).double()
    ref(x.double()).square().mean().backward()
    g_ref = {n: p.grad for n, p in ref.named_parameters()}
    m = m.to(device)
    m.train_attention = "torch"
    result = {}
    for mode in ("torch", "hip"):
        m.train_linear = mode
        m.zero_grad(set_to_none=True)
        y = m(x.to(device))
        y.square().mean().backward()
        result[mode] = (y.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    (y_t, g_t), (y_h, g_h) = result["torch"], result["hip"]
    assert g_t.keys() == g_h.keys() == g_ref.keys() and len(g_h) == len(list(m.parameters()))
    assert not torch.equal(y_h, y_t) and rel_l2(y_h, y_t) <= 1e-3
    mean_free = [n for n, mod in m.down_projection.named_modules()
                 if isinstance(mod, torch.nn.Conv3d) and mod.bias is not None and n != "proj"]
    zero = {f"down_projection.{n}" for n in mean_free} | {f"up_projection.decode.{len(m.up_projection.decode) - 1}"}
    assert len(zero) == 8 and all(f"{n}.bias" in g_t for n in zero)
    worst, failures = ("", 0.0), []
    for name in g_t:
        assert torch.isfinite(g_h[name]).all(), name
        layer = name[:-len(".bias")]
        if name.endswith(".bias") and layer in zero:
            for g in (g_t, g_h):
                ratio = (g[name].abs().max() / g[layer + ".weight"].abs().max()).item()
                assert ratio <= 1e-4, (name, ratio)
            continue
        e_h, e_t = R.errors(g_h[name], g_ref[name])[0], R.errors(g_t[name], g_ref[name])[0]
        ratio = e_h / max(e_t, 2.0 ** -11)
        if ratio > worst[1]:
            worst = (name, ratio)
        if not ratio <= 3.0:
            failures.append((name, e_h, e_t))
    print(f"largest err_hip / max(err_torch, 2^-11): {worst[1]:.3f} ({worst[0]})")
    assert not failures, failures
