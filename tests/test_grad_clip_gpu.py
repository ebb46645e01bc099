"""GPU: gradient clipping folded into FusedAdamW (amx_grad_norms + amx_adamw_step_clip_dev) against
torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW -- the reference's --clip_grad / --max_norm_G / --max_norm_F
(pretraining/models/supcl_model.py:631-655)."""
import numpy as np
import pytest
import torch

from anatomix_amd.pretraining import FusedAdamW, grad_norms

pytestmark = pytest.mark.gpu

# the tensor list of tests/test_optim_gpu.py (69 tensors: two launches of <= 48 descriptors, sizes 1, 3, 4099 and 128 * 128 * 27) ...
SHAPES = [(16, 1, 3, 3, 3), (16,), (64, 32, 3, 3, 3), (1,), (7, 5), (4099,), (128, 128, 3, 3, 3), (256, 128), (3,)] + [(33,)] * 60
OFFSET_NUMEL = 5000          # ... plus one tensor that starts 4 bytes into its storage: the scalar path, over more than one block
SPLIT = 35                   # tensors [0, SPLIT) are group 0, the rest group 1

KWS = [dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5),      # the reference's step
       dict(lr=1e-2, betas=(0.5, 0.9), eps=1e-6, weight_decay=0.1),
       dict(lr=1e-3, weight_decay=0.0, maximize=True)]


def _offset(t):
    """A copy of flat t that lives one element (4 bytes) into a fresh storage."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _params(device, seed):
    g = torch.Generator().manual_seed(seed)
    out = [torch.nn.Parameter(torch.randn(*s, generator=g).to(device)) for s in SHAPES]
    out.append(torch.nn.Parameter(_offset(torch.randn(OFFSET_NUMEL, generator=g).to(device))))
    return out


def _grads(params, seed, skip=()):
    """Gradient magnitudes from 1e-4 to 1 (per tensor); the last one at a 4-byte offset like its parameter."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k, p in enumerate(params):
        t = (torch.randn(*p.shape, generator=g) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=g))).to(p.device)
        if k == len(params) - 1:
            t = _offset(t)
        out.append(None if k in skip else t)
    return out


def _set(params, grads):
    for p, g in zip(params, grads):
        p.grad = None if g is None else (_offset(g) if g.data_ptr() % 16 else g.clone())


def _norm64(grads):
    sq = sum(float(np.sum(np.square(g.detach().cpu().numpy().astype(np.float64)))) for g in grads if g is not None)
    return float(np.sqrt(sq))


def test_norms_against_float64(device):
    """Fp32 path of the kernel: a thread adds the squares of its 16 values (15 additions), the wave butterfly adds 6 more = 21
    sequential fp32 additions; everything after that is double.  21 additions + the square's rounding, each <= 2^-24 relative
    on a sum of non-negative terms, halved by the square root: 22 * 2^-24 / 2 = 6.6e-7; times 2 for the final rounding to fp32
    and slack, as in the issue's derivation for a 32-addition path (2e-6): 1.4e-6."""
    params = _params(device, 0)
    grads = _grads(params, 100, skip={2, 40})
    _set(params, grads)
    groups = [params[:SPLIT], params[SPLIT:]]
    out = grad_norms(groups)
    again = grad_norms(groups)
    assert out.dtype == torch.float32 and out.shape == (2,) and torch.equal(out, again)
    want = [_norm64(grads[:SPLIT]), _norm64(grads[SPLIT:])]
    for k in range(2):
        rel = abs(float(out[k]) - want[k]) / want[k]
        print(f"group {k}: norm {float(out[k]):.9g} float64 {want[k]:.9g} rel {rel:.3e}")
        assert rel <= 1.4e-6, (k, rel)
    # an empty group gives 0 and leaves the others alone; so does a group whose gradients are all None
    for p in params[SPLIT:SPLIT + 3]:
        p.grad = None
    three = grad_norms([params[:SPLIT], [], params[SPLIT:SPLIT + 3]])
    assert float(three[1]) == 0.0 and float(three[2]) == 0.0 and torch.equal(three[0], out[0])
    # a NaN in group 1 stays there; an inf too
    _set(params, grads)
    params[-1].grad[17] = float("nan")
    bad = grad_norms(groups)
    assert torch.isnan(bad[1]) and torch.equal(bad[0], out[0])
    params[-1].grad[17] = float("inf")
    bad = grad_norms(groups)
    assert torch.isinf(bad[1]) and torch.equal(bad[0], out[0])


def test_grad_norms_writes_the_optimizers(device):
    params = _params(device, 1)
    opt_a, opt_b = FusedAdamW(params[:SPLIT], max_norm=1.0), FusedAdamW(params[SPLIT:])
    with pytest.raises(RuntimeError, match="never written"):
        _set(params, _grads(params, 5))
        opt_a.step()
    none = grad_norms([FusedAdamW([torch.nn.Parameter(torch.zeros(3, device=device))])])      # count == 0
    assert none.tolist() == [0.0]
    out = grad_norms([opt_a, opt_b])
    assert torch.equal(opt_a.total_norm, out[0]) and torch.equal(opt_b.total_norm, out[1]) and opt_a.total_norm.dim() == 0
    assert "total_norm" not in str(opt_a.state_dict().keys()) and set(opt_a.state_dict()) == {"state", "param_groups"}
    assert "max_norm" not in opt_a.state_dict()["param_groups"][0]


def _eight_steps(device, kw, norm_from_kernel):
    a = _params(device, 0)
    b = [torch.nn.Parameter(_offset(p.detach()) if p.data_ptr() % 16 else p.detach().clone()) for p in a]
    steps = [_grads(a, 100 + it, {2, 5} if it in (1, 2) else ()) for it in range(8)]
    norms = torch.tensor([float(torch.nn.utils.get_total_norm([g for g in gs if g is not None])) for gs in steps])
    max_norm = float(norms.median())
    clipped = int((max_norm / (norms + 1e-6) < 1.0).sum())
    assert clipped >= 2 and 8 - clipped >= 2, norms.tolist()              # both branches of the coefficient run
    opt_a, opt_b = FusedAdamW(a, max_norm=max_norm, **kw), torch.optim.AdamW(b, **kw)
    for gs in steps:
        _set(a, gs)
        _set(b, gs)
        total = torch.nn.utils.clip_grad_norm_(b, max_norm)
        if norm_from_kernel:
            grad_norms([opt_a])
        else:
            opt_a.total_norm.copy_(total)
            opt_a.mark_norm_written()
        opt_a.step()
        opt_b.step()
    return a, b, opt_a, opt_b


def _compare(a, b, opt_a, opt_b, kw, f):
    """The tolerances of test_fused_adamw_follows_torch_adamw times f."""
    for k, (p, q) in enumerate(zip(a, b)):
        assert torch.isfinite(p).all()
        assert torch.allclose(p, q, rtol=f * 2e-6, atol=f * (2e-6 * kw["lr"] * 8 + 1e-9)), (k, (p - q).abs().max().item())
        sa, sb = opt_a.state[p], opt_b.state[q]
        assert float(sa["step"]) == float(sb["step"]) == (6.0 if k in (2, 5) else 8.0)
        assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=f * 1e-6, atol=f * 1e-6 * float(sb["exp_avg"].abs().max()))
        assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=f * 2e-6, atol=f * 1e-30)


@pytest.mark.parametrize("kw", KWS)
def test_clipped_step_follows_clip_grad_norm_then_adamw(device, kw):
    """The arithmetic of the clip alone: torch's own norm goes into total_norm, so the two sides differ by the optimizers' fp32
    rounding only and the tolerances of the unclipped comparison hold unchanged."""
    _compare(*_eight_steps(device, kw, False), kw, 1.0)


@pytest.mark.parametrize("kw", KWS)
def test_clipped_step_end_to_end(device, kw):
    """The norm from amx_grad_norms: the gradient now carries the norm's error (<= 2e-6), so the tolerances double."""
    _compare(*_eight_steps(device, kw, True), kw, 2.0)


def test_infinite_max_norm_is_the_unclipped_step(device):
    a, b = _params(device, 3), _params(device, 3)
    kw = dict(lr=1e-2, weight_decay=1e-2)
    opt_a, opt_b = FusedAdamW(a, max_norm=float("inf"), **kw), FusedAdamW(b, max_norm=None, **kw)
    for it in range(3):
        gs = _grads(a, 20 + it)
        _set(a, gs)
        _set(b, gs)
        grad_norms([opt_a])
        opt_a.step()
        opt_b.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        for key in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(opt_a.state[p][key], opt_b.state[q][key])
    # a step that does clip leaves p.grad as it was (the step zeroes it anyway; the recorded norm is the one before clipping)
    opt_c = FusedAdamW(a, max_norm=1e-3, **kw)
    before = [p.grad.clone() for p in a]
    norm = grad_norms([opt_c])
    assert float(norm[0]) > 1e-3
    opt_c.step()
    for p, g in zip(a, before):
        assert torch.equal(p.grad, g)


def test_clipped_step_replays_from_a_graph(device):
    kw = dict(lr=1e-2, weight_decay=1e-2)
    grads = _grads(_params(device, 2), 9)
    small = [g * 0.01 for g in grads]
    big_norm, small_norm = _norm64(grads), _norm64(small)
    max_norm = (big_norm * small_norm) ** 0.5                          # between the two: `grads` clips, `small` does not
    order = [grads, small, grads]

    def fill(params, gs):
        torch._foreach_copy_([p.grad for p in params], gs)

    a = _params(device, 2)
    opt_a = FusedAdamW(a, max_norm=max_norm, **kw)
    _set(a, grads)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        grad_norms([opt_a])
        opt_a.step()                                                 # creates the state and the scratch outside the capture
    torch.cuda.current_stream(device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norm = grad_norms([opt_a])
        opt_a.step()
    seen = []
    for gs in order:
        fill(a, gs)
        graph.replay()
        seen.append(float(norm[0]))
    torch.cuda.synchronize(device)
    assert seen[0] > max_norm > seen[1] and seen[2] == seen[0]
    b = _params(device, 2)
    opt_b = FusedAdamW(b, max_norm=max_norm, **kw)
    _set(b, grads)
    for gs in [grads] + order:
        fill(b, gs)
        grad_norms([opt_b])
        opt_b.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
        assert float(opt_a.state[p]["step"]) == 4.0
