"""GPU: whole-volume sliding-window inference behind one C call (amx_sliding_window) and its pieces -- the one-launch count map,
the device-built window weights, the finishing pass (features / logits / labels) -- against the route that
sliding_window_inference takes today, and the prediction command on top."""
import ctypes
import json

import numpy as np
import pytest
import torch

import anatomix_amd
from anatomix_amd import _lib
from anatomix_amd.io.nifti import load_nifti, save_nifti
from anatomix_amd.registration import sliding_window as SW
from anatomix_amd.registration.metrics import dice_score
from anatomix_amd.registration.sliding_window import importance_map, sliding_window_inference, sliding_window_volume, window_starts
from anatomix_amd.segmentation.losses import predict_labels
from anatomix_amd.segmentation.segmentation_utils import UnetOutBlock
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu
KW = R.VARIANTS["anatomix"]
# maximum relative difference of amx_sw_importance_map against importance_map() as measured on the MI355X (see
# test_importance_map); the assertion is four times that, capped at 1e-6
MAP_REL_MEASURED = {"device": 0.0, "host": {(32, 32, 32): 2.63e-7, (64, 64, 64): 4.21e-7}}


@pytest.fixture(scope="module")
def model(device):
    m = anatomix_amd.Unet(**KW)
    m.load_state_dict(R.synthetic_state_dict(KW, 0), strict=True)
    return m.to(device).eval()


def centred_head(feat, classes, seed):
    """Conv3d(F, classes, 1) with random weights whose logits are O(1) and centred on the features ``feat`` [1, F, D, H, W], so that
    every class wins somewhere (a head of small random weights lets its bias decide every voxel)."""
    head = torch.nn.Conv3d(feat.shape[1], classes, 1).to(feat.device).eval()
    g = torch.Generator().manual_seed(seed)
    mean, std = feat.mean((0, 2, 3, 4)), feat.std((0, 2, 3, 4)) + 1e-6
    with torch.no_grad():
        w = torch.randn(classes, feat.shape[1], generator=g).to(feat.device) / std
        head.weight.copy_(w[:, :, None, None, None])
        head.bias.copy_(-(w @ mean))
    return head


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def stream(device):
    return _lib.stream(device)


def device_map(roi, mode, sigma_scale, device):
    out = torch.full(roi, float("nan"), dtype=torch.float32, device=device)
    _lib.check(_lib.load().amx_sw_importance_map(_lib.ptr(out), *roi, _lib.SW_MAP[mode], sigma_scale, stream(device)))
    return out


def near_tie_check(got, ref_logits, what):
    """``got`` uint8 labels against the arg-max of the float64 ``ref_logits`` [C, ...]: a voxel may differ only where the float64
    top-two margin is below 1e-4, and at most 0.1 % of the voxels may."""
    z = ref_logits.double()
    want = z.argmax(0)
    top2 = z.topk(2, dim=0).values
    margin = top2[0] - top2[1]
    diff = got.long() != want
    share = diff.double().mean().item()
    print(f"{what}: {int(diff.sum())} of {diff.numel()} voxels differ ({share:.2e}); largest margin among them "
          f"{float(margin[diff].max()) if diff.any() else 0.0:.2e}")
    assert not (diff & (margin >= 1e-4)).any()
    assert share <= 1e-3


# ---- 1. count map ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,overlap,windows", [((40, 36, 44), 0.8, 18), ((33, 35, 37), 0.5, 8)])
@pytest.mark.parametrize("mode", ["constant", "gaussian"])
def test_count_all_equals_the_sequence_of_count_launches(device, size, overlap, windows, mode):
    lib = _lib.load()
    roi = (32, 32, 32)
    wmap = importance_map(roi, mode, 0.125, device)
    if mode == "gaussian":
        assert int((wmap == wmap.min()).sum()) == 18992          # the floor is active
    starts = window_starts(size, roi, overlap)
    assert len(starts) == windows
    want = torch.zeros(size, dtype=torch.float32, device=device)
    for (z, y, x) in starts:
        _lib.check(lib.amx_sw_count(_lib.ptr(want), *size, z, y, x, *roi, _lib.ptr(wmap), stream(device)))
    got = torch.full(size, float("nan"), dtype=torch.float32, device=device)
    _lib.check(lib.amx_sw_count_all(_lib.ptr(got), *size, *roi, overlap, _lib.ptr(wmap), stream(device)))
    assert torch.equal(got, want)
    assert float(got.min()) > 0


# ---- 2. importance map ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roi,sigma_scale", [((32, 32, 32), 0.125), ((64, 64, 64), 0.25)])
def test_importance_map(device, roi, sigma_scale):
    """amx_sw_importance_map against importance_map().  Measured on the MI355X, maximum relative difference:
      * against the map torch builds on the device (the one sliding_window_inference uses): 0 for (32,32,32) / 0.125 and for
        (64,64,64) / 0.25 -- torch's device exp and HIP's expf agree on every value of these lines;
      * against the map torch builds on the host: 2.63e-7 for (32,32,32) / 0.125, 4.21e-7 for (64,64,64) / 0.25.
    Asserted: four times the measured value and not above 1e-6, i.e. equality with the device map and 1e-6 against the host map
    (4 x 2.63e-7 and 4 x 4.21e-7 are both above the cap).  Constant: exact.  The voxels at the floor match exactly."""
    const = device_map(roi, "constant", sigma_scale, device)
    assert torch.equal(const, importance_map(roi, "constant", sigma_scale, device))
    got = device_map(roi, "gaussian", sigma_scale, device)
    for where, measured in ((device, MAP_REL_MEASURED["device"]), ("cpu", MAP_REL_MEASURED["host"][roi])):
        want = importance_map(roi, "gaussian", sigma_scale, where).to(device)
        rel = ((got.double() - want.double()).abs() / want.double()).max().item()
        print(f"importance map {roi} sigma_scale {sigma_scale} against torch on {where}: max relative difference {rel:.3e}")
        assert rel <= min(4 * measured, 1e-6)
        assert int((got == got.min()).sum()) == int((want == want.min()).sum())
        assert torch.equal(got == got.min(), want == want.min())
    if roi == (32, 32, 32):
        assert int((got == got.min()).sum()) == 18992 and float(got.min()) == pytest.approx(1e-3, rel=1e-6)


# ---- 3. finish ------------------------------------------------------------------------------------------------------------------
V_ODD = 33 * 35 * 37


def finish(kind, acc, cnt, w, b, out, device):
    F_, V = acc.shape
    return _lib.load().amx_sw_finish(_lib.SW_OUT[kind], _lib.ptr(acc), _lib.ptr(cnt), F_, V, _lib.ptr(w), _lib.ptr(b),
                                     0 if w is None else w.shape[0], _lib.ptr(out), stream(device))


@pytest.mark.parametrize("F_,C", [(16, 5), (32, 32), (16, 2)])
def test_finish_modes(device, F_, C):
    assert V_ODD % 4 and (V_ODD * 4) % 16                    # odd: planes are not 16-byte aligned
    g = torch.Generator().manual_seed(0)
    acc = torch.randn(F_, V_ODD, generator=g).to(device)
    cnt = (torch.rand(V_ODD, generator=g) * 7.5 + 0.5).to(device)
    w = torch.randn(C, F_, generator=g).to(device)
    b = torch.randn(C, generator=g).to(device)
    # FEATURES: amx_sw_normalize bit for bit
    want = acc.clone()
    _lib.check(_lib.load().amx_sw_normalize(_lib.ptr(want), _lib.ptr(cnt), F_, V_ODD, stream(device)))
    got = acc.clone()
    _lib.check(finish("features", got, cnt, None, None, None, device))
    assert torch.equal(got, want)
    # LOGITS: float64 einsum
    ref = torch.einsum("cf,fv->cv", w.double(), acc.double() / cnt.double()) + b.double()[:, None]
    logits = torch.full((C, V_ODD), float("nan"), dtype=torch.float32, device=device)
    keep = acc.clone()
    _lib.check(finish("logits", acc, cnt, w, b, logits, device))
    assert torch.equal(acc, keep)                            # acc is left as it is
    err = ((logits.double() - ref).abs().max() / ref.abs().max()).item()
    print(f"finish logits F={F_} C={C}: max abs error / max |ref| = {err:.2e}, rel-L2 {rel_l2(logits, ref):.2e}")
    assert err <= 1e-5 and rel_l2(logits, ref) <= 1e-5
    # LABELS: arg-max of the float64 logits, up to near ties
    labels = torch.full((V_ODD,), 255, dtype=torch.uint8, device=device)
    _lib.check(finish("labels", acc, cnt, w, b, labels, device))
    assert torch.equal(acc, keep)
    near_tie_check(labels, ref, f"finish labels F={F_} C={C}")
    # no bias
    _lib.check(finish("logits", acc, cnt, w, None, logits, device))
    assert ((logits.double() - (ref - b.double()[:, None])).abs().max() / ref.abs().max()).item() <= 1e-5


def test_finish_aligned_volume_takes_the_vector_path_with_the_same_result(device):
    """V a multiple of 4 with aligned planes (the 16-byte path) against the same voxels inside an odd-sized call (the scalar path)."""
    g = torch.Generator().manual_seed(1)
    V = 4096 + 1024 + 4
    acc = torch.randn(16, V + 1, generator=g).to(device)
    cnt = (torch.rand(V + 1, generator=g) * 7.5 + 0.5).to(device)
    w, b = torch.randn(5, 16, generator=g).to(device), torch.randn(5, generator=g).to(device)
    odd_logits = torch.empty(5, V + 1, device=device)
    odd_labels = torch.empty(V + 1, dtype=torch.uint8, device=device)
    _lib.check(finish("logits", acc, cnt, w, b, odd_logits, device))
    _lib.check(finish("labels", acc, cnt, w, b, odd_labels, device))
    acc4, cnt4 = acc[:, :V].contiguous(), cnt[:V].contiguous()
    logits = torch.empty(5, V, device=device)
    labels = torch.empty(V, dtype=torch.uint8, device=device)
    _lib.check(finish("logits", acc4, cnt4, w, b, logits, device))
    _lib.check(finish("labels", acc4, cnt4, w, b, labels, device))
    assert torch.equal(logits, odd_logits[:, :V]) and torch.equal(labels, odd_labels[:V])


def test_finish_exact_ties_go_to_the_lowest_index(device):
    g = torch.Generator().manual_seed(2)
    acc = torch.randint(-8, 9, (16, V_ODD), generator=g).float().to(device)
    cnt = torch.ones(V_ODD, device=device)
    w = torch.randint(-3, 4, (5, 16), generator=g).float()
    w[3] = w[1]                                               # classes 1 and 3 tie everywhere
    b = torch.tensor([0.0, 2.0, -1.0, 2.0, 1.0])
    w, b = w.to(device), b.to(device)
    ref = torch.einsum("cf,fv->cv", w.double(), acc.double()) + b.double()[:, None]         # exact in fp32 too: small integers
    labels = torch.full((V_ODD,), 255, dtype=torch.uint8, device=device)
    _lib.check(finish("labels", acc, cnt, w, b, labels, device))
    index = torch.arange(5, device=device)[:, None].expand_as(ref)
    lowest = torch.where(ref == ref.max(0).values, index, 5).min(0).values        # the first index that holds the maximum
    assert torch.equal(labels.long(), lowest)
    assert int((labels == 1).sum()) > 0 and int((labels == 3).sum()) == 0


def test_finish_refuses_classes_above_the_envelope(device):
    acc = torch.randn(16, 4096, device=device)
    cnt = torch.ones(4096, device=device)
    w, b = torch.randn(33, 16, device=device), torch.randn(33, device=device)
    for kind, out in (("logits", torch.full((33, 4096), 7.0, device=device)),
                      ("labels", torch.full((4096,), 7, dtype=torch.uint8, device=device))):
        keep = out.clone()
        rc = finish(kind, acc, cnt, w, b, out, device)
        assert rc == _lib.AMX_ERR_INVALID and b"classes" in _lib.load().amx_last_error()
        with pytest.raises(_lib.AmxEnvelopeError):
            _lib.check_envelope(rc)
        torch.cuda.synchronize()
        assert torch.equal(out, keep)


# ---- 4. whole call, features ----------------------------------------------------------------------------------------------------
def test_whole_call_features(device, model):
    """(80,72,100), roi 64^3, overlap 0.8 = 24 windows = 6 batches of 4: the two-slot route.  Against sliding_window_inference on
    the same model the accumulations happen in the same order; only the device-built window weights differ."""
    size, roi = (80, 72, 100), (64, 64, 64)
    kw = dict(overlap=0.8, mode="gaussian", sigma_scale=0.25)
    x = R.synthetic_input(41, 1, size).to(device)
    assert len(window_starts(size, roi, 0.8)) == 24
    with torch.no_grad():
        want = sliding_window_inference(x, roi, 4, model, **kw)
        got = sliding_window_volume(x, roi, model, **kw)
        assert got.shape == want.shape == (1, 16) + size and torch.isfinite(got).all()
        err = rel_l2(got, want)
        print(f"whole call, features, device-built gaussian map: rel-L2 against sliding_window_inference {err:.3e}")
        assert err <= 1e-6
        for _ in range(3):
            assert torch.equal(sliding_window_volume(x, roi, model, **kw), got)
        # the constant map is exact on either route: the whole call is then bit-identical
        assert torch.equal(sliding_window_volume(x, roi, model, overlap=0.8, mode="constant"),
                           sliding_window_inference(x, roi, 4, model, overlap=0.8, mode="constant"))
        # the torch map handed to the lower-level pieces: plan, windows, one-launch count map, finish -> bit-identical
        lib = _lib.load()
        n = lib.amx_sw_plan(*size, *roi, 0.8, None, 0)
        offs = (ctypes.c_int * (3 * n))()
        assert lib.amx_sw_plan(*size, *roi, 0.8, offs, n) == 24
        starts = [tuple(offs[3 * i:3 * i + 3]) for i in range(n)]
        wmap = importance_map(roi, "gaussian", 0.25, device)
        acc = SW._run_fused(x, roi, starts, wmap, model, torch.zeros(size, device=device))
        cnt = torch.full(size, float("nan"), device=device)
        _lib.check(lib.amx_sw_count_all(_lib.ptr(cnt), *size, *roi, 0.8, _lib.ptr(wmap), stream(device)))
        _lib.check(lib.amx_sw_finish(_lib.SW_OUT["features"], _lib.ptr(acc), _lib.ptr(cnt), 16, cnt.numel(), None, None, 0, None, stream(device)))
        assert torch.equal(acc, want)


def test_whole_call_is_refused_while_the_stream_is_capturing(device, model):
    """The call does not go into a graph yet (the replayed whole gave other values than the eager call; its pieces replay correctly on
    their own): while the caller's stream is capturing the C entry returns AMX_ERR_INVALID, launches nothing and leaves the capture
    usable."""
    lib = _lib.load()
    size, roi = (64, 64, 96), (64, 64, 64)
    x = R.synthetic_input(46, 1, size).to(device)
    with torch.no_grad():
        sliding_window_volume(x, roi, model)                  # handle, weights and window weights are in place
    need = lib.amx_sliding_window_workspace_bytes(model._handle, 4, *roi)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    acc = torch.full((16,) + size, 3.0, device=device)
    cnt = torch.full(size, 3.0, device=device)
    t = torch.zeros(8, device=device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t.add_(1.0)
        rc = lib.amx_sliding_window(model._handle, _lib.ptr(x), *size, *roi, 0.25, 0, 0.125, 4, _lib.SW_OUT["features"], None, None, 0,
                                    _lib.ptr(acc), _lib.ptr(cnt), None, _lib.ptr(ws), need, stream(device))
        msg = lib.amx_last_error()
    assert rc == _lib.AMX_ERR_INVALID and b"captured" in msg
    g.replay()
    torch.cuda.synchronize()
    assert bool((t == 1.0).all()) and bool((acc == 3.0).all()) and bool((cnt == 3.0).all())


def test_window_weights_follow_the_key(device, model):
    """The window weights cached on the handle are rebuilt whenever (roi, mode, sigma_scale) changes, in place or reallocated: every
    call of a sequence of keys on ONE model equals the same single call on a freshly constructed model (new handle, empty cache).
    Roi 64 is 2 windows (one lane); roi 32 is 3 x 3 x 5 = 45 windows = 12 batches (two lanes) and another map size."""
    size = (64, 64, 96)
    assert len(window_starts(size, (64, 64, 64), 0.5)) == 2 and len(window_starts(size, (32, 32, 32), 0.5)) == 45
    x = R.synthetic_input(47, 1, size).to(device)
    sd = model.state_dict()
    keys = [(64, dict(mode="gaussian", sigma_scale=0.25)), (64, dict(mode="constant")), (64, dict(mode="gaussian", sigma_scale=0.125)),
            (32, dict(mode="gaussian", sigma_scale=0.125)), (64, dict(mode="gaussian", sigma_scale=0.25))]
    with torch.no_grad():
        for roi, kw in keys:
            fresh = anatomix_amd.Unet(**KW)
            fresh.load_state_dict(sd, strict=True)
            want = sliding_window_volume(x, roi, fresh.to(device).eval(), overlap=0.5, **kw)
            got = sliding_window_volume(x, roi, model, overlap=0.5, **kw)
            assert got.shape == (1, 16) + size and torch.isfinite(got).all()
            assert torch.equal(got, want), (roi, kw)


# ---- 5. whole call, labels and logits -------------------------------------------------------------------------------------------
def test_whole_call_labels_and_logits(device, model):
    size, roi = (64, 96, 80), (64, 64, 64)
    x = R.synthetic_input(42, 1, size).to(device)
    assert len(window_starts(size, roi, 0.7)) == 6
    with torch.no_grad():
        head = centred_head(sliding_window_inference(x, roi, 4, model, overlap=0.7), 5, 3)
        ref_logits = sliding_window_inference(x, roi, 4, torch.nn.Sequential(model, head), overlap=0.7)
        ref_labels = predict_labels(ref_logits)
        logits = sliding_window_volume(x, roi, model, overlap=0.7, head=head, out="logits")
        labels = sliding_window_volume(x, roi, model, overlap=0.7, head=head, out="labels")
    assert logits.shape == ref_logits.shape == (1, 5) + size and logits.dtype == torch.float32
    assert labels.shape == ref_labels.shape == (1, 1) + size and labels.dtype == torch.uint8
    err = rel_l2(logits, ref_logits)
    print(f"whole call, logits: rel-L2 against sliding_window_inference {err:.3e}; classes present {torch.unique(ref_labels).tolist()}")
    assert err <= 1e-5
    assert torch.unique(ref_labels).tolist() == [0, 1, 2, 3, 4]        # every class wins somewhere
    near_tie_check(labels[0, 0], ref_logits[0], "whole call, labels")
    assert int((labels != ref_labels).sum()) <= 1e-3 * labels.numel()
    # UnetOutBlock is the head load_model builds
    blk = UnetOutBlock(3, 16, 5).to(device).eval()
    blk.conv.conv.load_state_dict(head.state_dict())
    with torch.no_grad():
        assert torch.equal(sliding_window_volume(x, roi, model, overlap=0.7, head=blk, out="labels"), labels)


# ---- 6. padding and batch -------------------------------------------------------------------------------------------------------
def test_padding_and_batch(device, model):
    roi = (64, 64, 64)
    kw = dict(overlap=0.8, mode="gaussian", sigma_scale=0.25)
    x = R.synthetic_input(43, 1, (48, 64, 64)).to(device)
    with torch.no_grad():
        want = sliding_window_inference(x, roi, 4, model, **kw)
        got = sliding_window_volume(x, roi, model, **kw)
    assert got.shape == want.shape == (1, 16, 48, 64, 64)
    err = rel_l2(got, want)
    print(f"padded volume: rel-L2 against sliding_window_inference {err:.3e}")
    assert err <= 1e-6
    pair = R.synthetic_input(44, 2, (64, 64, 96)).to(device)
    with torch.no_grad():
        both = sliding_window_volume(pair, roi, model, **kw)
        singles = [sliding_window_volume(pair[i:i + 1], roi, model, **kw) for i in range(2)]
    assert both.shape == (2, 16, 64, 64, 96)
    assert torch.equal(both[0:1], singles[0]) and torch.equal(both[1:2], singles[1])
    assert not torch.equal(both[0], both[1])


# ---- 7. envelope ----------------------------------------------------------------------------------------------------------------
def test_output_nc_outside_the_envelope_raises_with_the_reason(device):
    m = anatomix_amd.Unet(**{**KW, "output_nc": 8}).to(device).eval()
    with pytest.raises(_lib.AmxEnvelopeError, match=r"output_nc.*sliding_window_inference"):
        sliding_window_volume(torch.zeros(1, 1, 64, 64, 64, device=device), 64, m)


def test_head_outside_the_envelope_raises_with_the_reason(device, model):
    x = torch.zeros(1, 1, 64, 64, 64, device=device)
    with torch.no_grad():
        with pytest.raises(_lib.AmxEnvelopeError, match="one 1x1x1 convolution"):
            sliding_window_volume(x, 64, model, out="labels")
        with pytest.raises(_lib.AmxEnvelopeError, match="one 1x1x1 convolution"):
            sliding_window_volume(x, 64, model, head=torch.nn.Sequential(torch.nn.Conv3d(16, 5, 1), torch.nn.ReLU()).to(device), out="logits")
        with pytest.raises(_lib.AmxEnvelopeError, match="classes"):
            sliding_window_volume(x, 64, model, head=torch.nn.Conv3d(16, 33, 1).to(device), out="labels")
        with pytest.raises(_lib.AmxEnvelopeError, match="roi width"):
            sliding_window_volume(x, (64, 64, 16), model)
    with pytest.raises(_lib.AmxEnvelopeError, match="no_grad"):
        sliding_window_volume(x, 64, model)


def test_c_entry_refuses_before_launching(device, model):
    """A workspace one byte short, a roi narrower than 32 and a volume smaller than the roi: the C entry returns its error and
    leaves every buffer untouched."""
    lib = _lib.load()
    size, roi = (64, 64, 96), (64, 64, 64)
    x = R.synthetic_input(45, 1, size).to(device)
    with torch.no_grad():
        sliding_window_volume(x, roi, model)                  # handle and weights are in place
    need = lib.amx_sliding_window_workspace_bytes(model._handle, 4, *roi)
    assert need == 2 * ((lib.amx_unet_workspace_bytes(model._handle, 4, *roi) + 255) // 256 * 256)
    ws = torch.empty(need, dtype=torch.uint8, device=device)
    w, b = torch.randn(5, 16, device=device), torch.randn(5, device=device)
    acc = torch.full((16,) + size, 3.0, device=device)
    cnt = torch.full(size, 3.0, device=device)
    out = torch.full(size, 9, dtype=torch.uint8, device=device)

    def call(size_, roi_, nbytes):
        return lib.amx_sliding_window(model._handle, _lib.ptr(x), *size_, *roi_, 0.5, 0, 0.125, 4, _lib.SW_OUT["labels"], _lib.ptr(w),
                                      _lib.ptr(b), 5, _lib.ptr(acc), _lib.ptr(cnt), _lib.ptr(out), _lib.ptr(ws), nbytes, stream(device))

    for args, code in (((size, roi, need - 1), _lib.AMX_ERR_WORKSPACE), (((64, 64, 96), (64, 64, 16), need), _lib.AMX_ERR_SHAPE),
                       (((64, 64, 48), roi, need), _lib.AMX_ERR_SHAPE)):
        assert call(*args) == code
        torch.cuda.synchronize()
        assert bool((acc == 3.0).all()) and bool((cnt == 3.0).all()) and bool((out == 9).all())
    with pytest.raises(_lib.AmxError, match="workspace needs"):
        _lib.check(call(size, roi, need - 1))
    assert call(size, roi, need) == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(out[None, None], sliding_window_volume(x, roi, model, overlap=0.5, head=_conv(w, b), out="labels"))


def _conv(w, b):
    c = torch.nn.Conv3d(w.shape[1], w.shape[0], 1).to(w.device)
    with torch.no_grad():
        c.weight.copy_(w.reshape(c.weight.shape))
        c.bias.copy_(b)
    return c.eval()


# ---- 8. command -----------------------------------------------------------------------------------------------------------------
def test_predict_command(device, model, tmp_path):
    from anatomix_amd.segmentation import predict
    blk = UnetOutBlock(3, 16, 5).to(device)
    with torch.no_grad():
        probe = model(R.synthetic_input(9, 1, (32, 32, 32)).to(device))
    blk.conv.conv.load_state_dict(centred_head(probe, 5, 5).state_dict())
    full = torch.nn.Sequential(model, blk).eval()
    ckpt = tmp_path / "best.pth"
    torch.save(full.state_dict(), ckpt)
    affine = np.array([[0.0, -1.5, 0.0, 10.0], [2.0, 0.0, 0.0, -20.0], [0.0, 0.0, 1.25, 5.0], [0.0, 0.0, 0.0, 1.0]])
    rs = np.random.RandomState(9)
    images, labels = [], []
    for k, shape in enumerate([(40, 36, 44), (32, 48, 40)]):
        vol = (rs.rand(*shape) * 700 - 50).astype(np.float32)
        lab = np.clip((vol + 50) / 700 * 5, 0, 4).astype(np.uint8)
        images.append(str(tmp_path / f"case{k}.nii.gz"))
        labels.append(str(tmp_path / f"case{k}_label.nii.gz"))
        save_nifti(images[-1], vol, affine)
        save_nifti(labels[-1], lab, affine)
    out_dir = tmp_path / "out"
    res = predict.main(["--images", *images, "--labels", *labels, "--ckpt", str(ckpt), "--n_classes", "4", "--out_dir", str(out_dir),
                        "--roi", "32", "--overlap", "0.7", "--device", str(device)])
    dice = json.load(open(out_dir / "dice.json"))
    assert sorted(dice) == ["case0", "case1"] and res["dice"] == dice
    for k in range(2):
        path = out_dir / f"case{k}_seg.nii.gz"
        assert str(path) == res["paths"][k] and path.exists()
        data, aff, hdr = load_nifti(str(path))
        raw, _, _ = load_nifti(images[k])
        assert data.shape == raw.shape and np.allclose(aff, affine)
        seg = torch.from_numpy(np.ascontiguousarray(data)).to(device)
        assert torch.equal(seg, seg.round()) and 0 <= float(seg.min()) and float(seg.max()) <= 4
        want = predict.segment_volume(full, torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).to(device), roi=32, overlap=0.7)
        assert want.dtype == torch.uint8 and want.shape == raw.shape
        assert torch.equal(seg.to(torch.uint8), want)
        assert len(torch.unique(want)) >= 3                      # not one class everywhere
        lab = torch.from_numpy(np.ascontiguousarray(load_nifti(labels[k])[0]).astype(np.uint8)).to(device)
        mean, per = dice_score(lab, want)
        assert dice[f"case{k}"]["mean"] == mean and dice[f"case{k}"]["per_class"] == {str(l): v for l, v in per.items()}
    # the file holds uint8 voxels (NIfTI-1 datatype code 2 at byte 70 of the header)
    import gzip
    import struct
    with gzip.open(out_dir / "case0_seg.nii.gz", "rb") as f:
        assert struct.unpack("<h", f.read(72)[70:72])[0] == 2
