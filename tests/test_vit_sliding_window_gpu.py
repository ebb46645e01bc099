"""GPU: the 3D ViT under whole-volume sliding-window inference -- amx_vit_forward_windows (the last decoder product blends every
window into the fp32 volume in its epilogue) and amx_vit_sliding_window (the whole call) -- against the generic window loop of
sliding_window_inference around the same engine, against the float64 oracle, and through the callers (routing, segment_volume's
labels, extract_features).

Shapes (schedules from window_starts):
  A  roi 32^3,        volume (48, 32, 40), overlap 0.5 : 4 windows, z {0, 16}, x {0, 8}          -- 16-byte path
  B  roi 32^3,        volume (32, 37, 43), overlap 0.7 : 6 windows, y {0, 5},  x {0, 9, 11}      -- odd rows / corners: scalar path; the
                                                                                                  second batch is ragged (2 of 4)
  C  roi (32, 64, 32), volume (32, 80, 32), overlap 0.25: 2 windows, y {0, 16}                    -- non-cubic roi"""
import ctypes

import numpy as np
import pytest
import torch

from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2
from anatomix_amd.registration import sliding_window as SW
from anatomix_amd.registration.convex_adam_utils import extract_features
from anatomix_amd.registration.sliding_window import importance_map, sliding_window_inference, sliding_window_volume, window_starts
from anatomix_amd.segmentation.predict import segment_volume
from oracle import vit_ref as V
from test_sliding_window_call_gpu import centred_head, near_tie_check, rel_l2

pytestmark = pytest.mark.gpu

S, SC = (32, 32, 32), (32, 64, 32)
CASES = {                       # roi, volume, overlap, corners
    "A": (S, (48, 32, 40), 0.5, [(z, 0, x) for z in (0, 16) for x in (0, 8)]),
    "B": (S, (32, 37, 43), 0.7, [(0, y, x) for y in (0, 5) for x in (0, 9, 11)]),
    "C": (SC, (32, 80, 32), 0.25, [(0, 0, 0), (0, 16, 0)]),
}
SEED = {"A": 21, "B": 22, "C": 23}
GAUSS = dict(mode="gaussian", sigma_scale=0.25)
HEAD_SEED = 3                   # see test_logits_and_labels

_models, _generic, _oracle = {}, {}, {}


def kw_of(roi, **over):
    return dict(V.VIT_VARIANTS["anatomix-dev-vit"], input_shape=roi, eva_depth=2, **over)


def vit(roi, device):
    """(model, state dict) of the 4 x 4 x 4 (or 4 x 8 x 4) token grid, built once."""
    if roi not in _models:
        kw = kw_of(roi)
        sd = V.synthetic_state_dict(kw, 7)
        m = PrimusV2(**kw)
        m.load_state_dict(sd, strict=True)
        _models[roi] = (m.to(device).eval(), sd)
    return _models[roi]


def volume(case, device, n=1):
    return V.synthetic_input(SEED[case], n, CASES[case][1]).to(device)


def generic(case, device, mode):
    """The yardstick: the generic window loop around a plain callable, computed once per (case, mode) and left unchanged."""
    key = (case, mode)
    if key not in _generic:
        roi, _, overlap, _ = CASES[case]
        model, _ = vit(roi, device)
        kw = GAUSS if mode == "gaussian" else dict(mode="constant")
        with torch.no_grad():
            _generic[key] = sliding_window_inference(volume(case, device), roi, 4, lambda w: model(w), overlap=overlap, **kw)
    return _generic[key]


def oracle_windows(case):
    """oracle.vit_ref.forward of every window of the case in float64 (host), computed once: ([windows, 32, roi], the windows)."""
    if case not in _oracle:
        roi, size, _, corners = CASES[case]
        x = V.synthetic_input(SEED[case], 1, size)
        win = torch.cat([x[:, :, z:z + roi[0], y:y + roi[1], xx:xx + roi[2]] for (z, y, xx) in corners])
        sd = V.synthetic_state_dict(kw_of(roi), 7)
        _oracle[case] = (V.forward(win, sd, kw_of(roi), dtype=torch.float64), win)
    return _oracle[case]


def stream(device):
    return _lib.stream(device)


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_the_schedules_are_the_ones_the_cases_were_chosen_for(case):
    roi, size, overlap, corners = CASES[case]
    assert window_starts(size, roi, overlap) == corners
    lib = _lib.load()
    offs = (ctypes.c_int * (3 * len(corners)))()
    assert lib.amx_sw_plan(*size, *roi, overlap, offs, len(corners)) == len(corners)
    assert [tuple(offs[3 * i:3 * i + 3]) for i in range(len(corners))] == corners


# ---- 1. features -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["gaussian", "constant"])
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_features(device, case, mode):
    roi, size, overlap, corners = CASES[case]
    model, _ = vit(roi, device)
    kw = GAUSS if mode == "gaussian" else dict(mode="constant")
    x = volume(case, device)
    want = generic(case, device, mode)
    with torch.no_grad():
        got = sliding_window_volume(x, roi, model, overlap=overlap, **kw)
        assert got.shape == want.shape == (1, 32) + size and got.dtype == torch.float32 and torch.isfinite(got).all()
        err = rel_l2(got, want)
        print(f"case {case} {mode}: rel-L2 against the generic loop {err:.3e}")
        assert err <= 1e-6
        for _ in range(3):
            assert torch.equal(sliding_window_volume(x, roi, model, overlap=overlap, **kw), got)
    # the pieces, handed the map the whole call builds: plan, window batches, one-launch count map, finish -> bit-identical
    lib = _lib.load()
    n = lib.amx_sw_plan(*size, *roi, overlap, None, 0)
    offs = (ctypes.c_int * (3 * n))()
    assert lib.amx_sw_plan(*size, *roi, overlap, offs, n) == len(corners)
    wmap = torch.empty(roi, dtype=torch.float32, device=device)
    sigma = kw.get("sigma_scale", 0.125)
    _lib.check(lib.amx_sw_importance_map(_lib.ptr(wmap), *roi, _lib.SW_MAP[mode], sigma, stream(device)))
    acc = torch.zeros((32,) + size, dtype=torch.float32, device=device)
    cnt = torch.full(size, float("nan"), device=device)
    need = lib.amx_vit_windows_workspace_bytes(model._handle, 4)
    assert need == lib.amx_vit_sliding_window_workspace_bytes(model._handle, 4) > lib.amx_vit_workspace_bytes(model._handle, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    for w0 in range(0, n, 4):
        k = min(4, n - w0)
        grp = (ctypes.c_int * (3 * k))(*offs[3 * w0:3 * (w0 + k)])
        _lib.check(lib.amx_vit_forward_windows(model._handle, _lib.ptr(x), *size, k, grp, _lib.ptr(wmap), _lib.ptr(acc), _lib.ptr(ws), need,
                                               stream(device)))
    _lib.check(lib.amx_sw_count_all(_lib.ptr(cnt), *size, *roi, overlap, _lib.ptr(wmap), stream(device)))
    _lib.check(lib.amx_sw_finish(_lib.SW_OUT["features"], _lib.ptr(acc), _lib.ptr(cnt), 32, cnt.numel(), None, None, 0, None, stream(device)))
    assert torch.equal(acc[None], got)


def test_vector_and_scalar_rows_give_the_same_values(device):
    """One window of case A accumulated at an aligned corner of an aligned volume (16-byte path) and at an odd corner of a volume
    with an odd row length (scalar path): the same window, the same map, the same bits."""
    lib = _lib.load()
    model, _ = vit(S, device)
    x = V.synthetic_input(31, 1, S).to(device)
    wmap = importance_map(S, "gaussian", 0.25, device)
    res = []
    with torch.no_grad():
        model(x)                                            # the engine is loaded
    need = lib.amx_vit_windows_workspace_bytes(model._handle, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    for size, corner in (((36, 40, 40), (2, 4, 8)), ((35, 37, 39), (3, 5, 7))):
        vol = torch.zeros(size, device=device)
        z, y, xx = corner
        vol[z:z + 32, y:y + 32, xx:xx + 32] = x[0, 0]
        acc = torch.zeros((32,) + size, device=device)
        offs = (ctypes.c_int * 3)(*corner)
        _lib.check(lib.amx_vit_forward_windows(model._handle, _lib.ptr(vol), *size, 1, offs, _lib.ptr(wmap), _lib.ptr(acc), _lib.ptr(ws), need,
                                               stream(device)))
        inside = acc[:, z:z + 32, y:y + 32, xx:xx + 32].clone()
        acc[:, z:z + 32, y:y + 32, xx:xx + 32] = 0
        assert not acc.any()                                # nothing outside the window was touched
        res.append(inside)
    assert torch.equal(res[0], res[1])
    with torch.no_grad():
        assert torch.equal(res[0], wmap * model(x)[0])      # and they are the forward's values times the map


def test_window_weights_follow_the_key(device):
    """The window weights cached on the handle are rebuilt in place whenever (mode, sigma_scale) changes: every call of a sequence
    of keys on ONE model equals the same single call on a fresh model loaded from the same state dict (new handle, empty cache)."""
    roi, size, overlap, corners = CASES["A"]
    assert len(window_starts(size, roi, overlap)) == len(corners) == 4
    model, sd = vit(roi, device)
    x = volume("A", device)
    with torch.no_grad():
        for kw in (GAUSS, dict(mode="constant"), dict(mode="gaussian", sigma_scale=0.125), GAUSS):
            fresh = PrimusV2(**kw_of(roi))
            fresh.load_state_dict(sd, strict=True)
            want = sliding_window_volume(x, roi, fresh.to(device).eval(), overlap=overlap, **kw)
            got = sliding_window_volume(x, roi, model, overlap=overlap, **kw)
            assert got.shape == (1, 32) + size and torch.isfinite(got).all()
            assert torch.equal(got, want), kw


# ---- 2. float64 oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "B"])
def test_against_the_float64_oracle(device, case):
    """ref64: oracle.vit_ref.forward per window in float64, blended with the (fp32) window weights in float64.  The window average
    is a convex combination of the per-window outputs, so the per-window error cannot grow; the factor 2 covers the fp32
    accumulation and the division.  Bound: 2 x the largest per-window |forward_hip - oracle64|; nothing comes from the code under test."""
    roi, size, overlap, corners = CASES[case]
    model, _ = vit(roi, device)
    ref_win, win = oracle_windows(case)
    wmap = importance_map(roi, "gaussian", 0.25, "cpu").double()
    acc = torch.zeros((32,) + size, dtype=torch.float64)
    cnt = torch.zeros(size, dtype=torch.float64)
    for k, (z, y, x) in enumerate(corners):
        acc[:, z:z + roi[0], y:y + roi[1], x:x + roi[2]] += wmap * ref_win[k]
        cnt[z:z + roi[0], y:y + roi[1], x:x + roi[2]] += wmap
    ref64 = acc / cnt
    with torch.no_grad():
        per_window = (model.forward_hip(win.to(device)).double().cpu() - ref_win).abs().amax(dim=(1, 2, 3, 4))
        got = sliding_window_volume(volume(case, device), roi, model, overlap=overlap, **GAUSS)[0].double().cpu()
    err, bound = (got - ref64).abs().max().item(), 2 * per_window.max().item()
    print(f"case {case}: max |got - ref64| {err:.3e}; per-window engine error {[f'{v:.3e}' for v in per_window.tolist()]}, bound {bound:.3e}; "
          f"max |ref64| {ref64.abs().max().item():.3f}")
    assert err <= bound


# ---- 3. logits and labels --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A", "C"])
def test_logits_and_labels(device, case):
    """Head: centred_head(generic features, 5, HEAD_SEED).  The seed was checked beforehand on the host, with the float64 oracle
    in place of the engine (windows blended in float64, the head built from those features): every class wins somewhere and the
    share of voxels whose top-two margin is below 1e-4 is 0 of 61440 on A and 0 of 81920 on C (seeds 4 and 5: 4.9e-5 / 3.3e-5 on
    A, 1.2e-5 / 3.7e-5 on C), under the 0.1 % that the comparison allows to differ.  The same two properties are asserted here on
    the generic logits."""
    roi, size, overlap, _ = CASES[case]
    model, _ = vit(roi, device)
    x = volume(case, device)
    with torch.no_grad():
        head = centred_head(generic(case, device, "constant"), 5, HEAD_SEED)
        ref_logits = sliding_window_inference(x, roi, 4, lambda w: head(model(w)), overlap=overlap)
        top2 = ref_logits[0].double().topk(2, dim=0).values
        share = ((top2[0] - top2[1]) < 1e-4).double().mean().item()
        print(f"case {case}: share of voxels with a top-two margin below 1e-4: {share:.2e}; classes {torch.unique(ref_logits.argmax(1)).tolist()}")
        assert share < 1e-3 and torch.unique(ref_logits.argmax(1)).tolist() == [0, 1, 2, 3, 4]
        labels = sliding_window_volume(x, roi, model, overlap=overlap, head=head, out="labels")
        assert labels.shape == (1, 1) + size and labels.dtype == torch.uint8
        near_tie_check(labels[0, 0], ref_logits[0], f"case {case}, labels")
        assert torch.equal(segment_volume(torch.nn.Sequential(model, head), x[0, 0], roi=roi, overlap=overlap)[None, None],
                           sliding_window_volume(_val_scaled(x), roi, model, overlap=overlap, head=head, out="labels"))
        if case == "A":
            logits = sliding_window_volume(x, roi, model, overlap=overlap, head=head, out="logits")
            assert logits.shape == ref_logits.shape == (1, 5) + size and logits.dtype == torch.float32
            err = rel_l2(logits, ref_logits)
            print(f"case A, logits: rel-L2 against the generic loop {err:.3e}")
            assert err <= 1e-5


def _val_scaled(x):
    from anatomix_amd.segmentation.segmentation_utils import get_val_transforms
    return get_val_transforms()(x.detach().float())


# ---- 4. padding and batch --------------------------------------------------------------------------------------------------------
def test_padding_and_batch(device):
    model, _ = vit(S, device)
    x = V.synthetic_input(24, 1, (24, 32, 40)).to(device)
    with torch.no_grad():
        want = sliding_window_inference(x, S, 4, lambda w: model(w), overlap=0.5, **GAUSS)
        got = sliding_window_volume(x, S, model, overlap=0.5, **GAUSS)
    assert got.shape == want.shape == (1, 32, 24, 32, 40)
    err = rel_l2(got, want)
    print(f"padded volume: rel-L2 against the generic loop {err:.3e}")
    assert err <= 1e-6
    pair = V.synthetic_input(25, 2, (48, 32, 40)).to(device)
    with torch.no_grad():
        both = sliding_window_volume(pair, S, model, overlap=0.5, **GAUSS)
        singles = [sliding_window_volume(pair[i:i + 1], S, model, overlap=0.5, **GAUSS) for i in range(2)]
    assert both.shape == (2, 32, 48, 32, 40)
    assert torch.equal(both[0:1], singles[0]) and torch.equal(both[1:2], singles[1])
    assert not torch.equal(both[0], both[1])


# ---- 5. routing ------------------------------------------------------------------------------------------------------------------
def test_routing(device):
    roi, size, overlap, corners = CASES["A"]
    model, _ = vit(roi, device)
    x = volume("A", device)
    want = generic("A", device, "gaussian")
    with torch.no_grad():
        before = SW.CALLS["vit_windows"]
        got = sliding_window_inference(x, roi, 4, model, overlap=overlap, **GAUSS)
        assert SW.CALLS["vit_windows"] == before + 1 and SW.VIT_WINDOW_BATCH == 4          # 4 windows: one call
        err = rel_l2(got, want)
        print(f"routed features: rel-L2 against the generic loop {err:.3e}")
        assert got.shape == want.shape and err <= 1e-6
        head = centred_head(generic("A", device, "constant"), 5, HEAD_SEED)
        ref_logits = sliding_window_inference(x, roi, 4, lambda w: head(model(w)), overlap=overlap)
        before = SW.CALLS["vit_windows"]
        logits = sliding_window_inference(x, roi, 4, torch.nn.Sequential(model, head), overlap=overlap)
        assert SW.CALLS["vit_windows"] == before + 1
        err = rel_l2(logits, ref_logits)
        print(f"routed logits: rel-L2 against the generic loop {err:.3e}")
        assert logits.shape == ref_logits.shape and err <= 1e-5
        # a plain callable, and a model whose output norm the engine does not apply, keep the generic loop
        before = SW.CALLS["vit_windows"]
        sliding_window_inference(x, roi, 4, lambda w: model(w), overlap=overlap)
        other = PrimusV2(**kw_of(roi, out_norm="instance"))
        other.load_state_dict(V.synthetic_state_dict(kw_of(roi, out_norm="instance"), 7), strict=True)
        other = other.to(device).eval()
        y = sliding_window_inference(x, roi, 4, other, overlap=overlap)
        assert SW.CALLS["vit_windows"] == before and y.shape == (1, 32) + size and torch.isfinite(y).all()
        with pytest.raises(_lib.AmxEnvelopeError, match=r"out_norm.*sliding_window_inference"):
            sliding_window_volume(x, roi, other, overlap=overlap)
        with pytest.raises(_lib.AmxEnvelopeError, match="roi must be the model's input shape"):
            sliding_window_volume(x, (32, 32, 16), model, overlap=overlap)
    with pytest.raises(_lib.AmxEnvelopeError, match="no_grad"):
        sliding_window_volume(x, roi, model, overlap=overlap)


# ---- 6. engine state -------------------------------------------------------------------------------------------------------------
def test_the_forward_is_not_disturbed(device):
    model, _ = vit(S, device)
    x = V.synthetic_input(26, 2, S).to(device)
    with torch.no_grad():
        a = model(x)
        sliding_window_volume(volume("B", device), S, model, overlap=0.7, **GAUSS)
        sliding_window_inference(volume("A", device), S, 4, model, overlap=0.5)
        assert torch.equal(model(x), a)


# ---- 7. refusals at the C entry --------------------------------------------------------------------------------------------------
def _entry_buffers(device, size):
    return (torch.full((32,) + size, 3.0, device=device), torch.full(size, 3.0, device=device),
            torch.full(size, 9, dtype=torch.uint8, device=device))


def test_c_entry_refuses_before_launching(device):
    lib = _lib.load()
    roi, size, overlap, _ = CASES["A"]
    model, _ = vit(roi, device)
    x = volume("A", device)
    with torch.no_grad():
        sliding_window_volume(x, roi, model, overlap=overlap)             # handle, parameters and window weights are in place
    need = lib.amx_vit_sliding_window_workspace_bytes(model._handle, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    acc, cnt, out = _entry_buffers(device, size)
    w, b = torch.randn(33, 32, device=device), torch.randn(33, device=device)

    def call(size_=size, n_batch=4, classes=5, nbytes=need):
        return lib.amx_vit_sliding_window(model._handle, _lib.ptr(x), *size_, overlap, 0, 0.125, n_batch, _lib.SW_OUT["labels"], _lib.ptr(w),
                                          _lib.ptr(b), classes, _lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(out), _lib.ptr(ws), nbytes, stream(device))

    for kwargs, code in ((dict(nbytes=need - 1), _lib.AMX_ERR_WORKSPACE), (dict(n_batch=0), _lib.AMX_ERR_INVALID),
                         (dict(n_batch=17), _lib.AMX_ERR_INVALID), (dict(size_=(48, 32, 24)), _lib.AMX_ERR_SHAPE),
                         (dict(classes=33), _lib.AMX_ERR_INVALID)):
        assert call(**kwargs) == code, (kwargs, lib.amx_last_error())
        torch.cuda.synchronize()
        assert bool((acc == 3.0).all()) and bool((cnt == 3.0).all()) and bool((out == 9).all())
    assert lib.amx_vit_forward_windows(model._handle, _lib.ptr(x), *size, 17, (ctypes.c_int * 51)(), _lib.ptr(cnt), _lib.ptr(acc), _lib.ptr(ws),
                                       need, stream(device)) == _lib.AMX_ERR_INVALID
    assert lib.amx_vit_forward_windows(model._handle, _lib.ptr(x), *size, 1, (ctypes.c_int * 3)(0, 0, 9), _lib.ptr(cnt), _lib.ptr(acc),
                                       _lib.ptr(ws), need, stream(device)) == _lib.AMX_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((acc == 3.0).all())
    assert call() == 0                                                      # and the accepted call gives the caller's labels
    torch.cuda.synchronize()
    head = torch.nn.Conv3d(32, 5, 1).to(device).eval()
    with torch.no_grad():
        head.weight.copy_(w[:5].reshape(head.weight.shape))
        head.bias.copy_(b[:5])
        assert torch.equal(out[None, None], sliding_window_volume(x, roi, model, overlap=overlap, head=head, out="labels"))


def test_whole_call_is_refused_while_the_stream_is_capturing(device):
    lib = _lib.load()
    roi, size, overlap, _ = CASES["A"]
    model, _ = vit(roi, device)
    x = volume("A", device)
    with torch.no_grad():
        sliding_window_volume(x, roi, model, overlap=overlap)
    need = lib.amx_vit_sliding_window_workspace_bytes(model._handle, 4)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    acc, cnt, _ = _entry_buffers(device, size)
    t = torch.zeros(8, device=device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.add_(1.0)
        rc = lib.amx_vit_sliding_window(model._handle, _lib.ptr(x), *size, overlap, 0, 0.125, 4, _lib.SW_OUT["features"], None, None, 0,
                                        _lib.ptr(acc), _lib.ptr(cnt), None, _lib.ptr(ws), need, stream(device))
        msg = lib.amx_last_error()
    assert rc == _lib.AMX_ERR_INVALID and b"captured" in msg
    g.replay()
    torch.cuda.synchronize()
    assert bool((t == 1.0).all()) and bool((acc == 3.0).all()) and bool((cnt == 3.0).all())


# ---- 8. registration path --------------------------------------------------------------------------------------------------------
def test_extract_features_takes_the_fused_route(device):
    kw = dict(V.VIT_VARIANTS["anatomix-dev-vit"], eva_depth=2)
    assert tuple(kw["input_shape"]) == (128, 128, 128)
    model = PrimusV2(**kw)
    model.load_state_dict(V.synthetic_state_dict(kw, 8), strict=True)
    model = model.to(device).eval()
    rs = np.random.RandomState(8)
    fixed, moving = rs.rand(128, 128, 128).astype(np.float32), rs.rand(128, 128, 128).astype(np.float32)
    before = SW.CALLS["vit_windows"]
    f, m = extract_features(fixed, moving, model)
    assert SW.CALLS["vit_windows"] == before + 2                            # one window per volume
    for y in (f, m):
        assert y.shape == (1, 32, 128, 128, 128) and y.dtype == torch.float32 and torch.isfinite(y).all()
    assert not torch.equal(f, m)
