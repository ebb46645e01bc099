"""GPU: the fused sliding-window path (one amx_unet_forward_window call per window: gather in the stem's
loader, weighted accumulate in the last conv's epilogue) against (a) the generic torch path driving the
same HIP model and (b) the numpy oracle driving the CPU oracle network."""
import numpy as np
import pytest
import torch

import anatomix_amd
from anatomix_amd.registration.sliding_window import _fused_ok, sliding_window_inference, window_starts
from anatomix_amd.registration.convex_adam_utils import extract_features
from oracle import sliding_window_ref as O
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu
KW = R.VARIANTS["anatomix"]


def _model(device):
    m = anatomix_amd.Unet(**KW)
    sd = R.synthetic_state_dict(KW, 0)
    m.load_state_dict(sd, strict=True)
    return m.to(device).eval(), sd


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_fused_equals_generic_path(device):
    m, _ = _model(device)
    x = torch.from_numpy(np.random.RandomState(5).rand(1, 1, 96, 64, 80).astype(np.float32)).to(device)
    with torch.no_grad():
        assert _fused_ok(m, x, (64, 64, 64))
        fused = sliding_window_inference(x, (64, 64, 64), 2, m, overlap=0.8, mode="gaussian", sigma_scale=0.25)
        generic = sliding_window_inference(x, (64, 64, 64), 2, lambda t: m(t), overlap=0.8, mode="gaussian", sigma_scale=0.25)
    assert fused.shape == (1, 16, 96, 64, 80) and torch.isfinite(fused).all()
    assert rel_l2(fused, generic) < 1e-5


def test_fused_matches_cpu_oracle(device):
    m, sd = _model(device)
    vol = np.random.RandomState(6).rand(1, 64, 96, 64).astype(np.float32)
    with torch.no_grad():
        got = sliding_window_inference(torch.from_numpy(vol)[None].to(device), (64, 64, 64), 2, m, overlap=0.5,
                                       mode="gaussian", sigma_scale=0.25).cpu()[0]
        torch.set_num_threads(16)
        ref = O.sliding_window(vol, (64, 64, 64), lambda a: R.forward(torch.from_numpy(a), sd, KW).numpy(), 0.5, "gaussian", 0.25)
    assert len(window_starts((64, 96, 64), (64, 64, 64), 0.5)) == 2
    assert rel_l2(got, torch.from_numpy(ref)) <= 1e-3


def test_extract_features_surface(device):
    """convex_adam_utils.extract_features: two volumes -> two [1,16,D,H,W] feature tensors; volumes smaller
    than the 128^3 ROI along an axis are zero padded first and cropped back."""
    m, _ = _model(device)
    rs = np.random.RandomState(7)
    fixed = (rs.rand(128, 144, 128) * 900 - 100).astype(np.float32)
    moving = (rs.rand(112, 128, 128) * 50).astype(np.float32)
    f, mv = extract_features(fixed, moving, m, fixminclip=0.0, fixmaxclip=500.0)
    assert f.shape == (1, 16, 128, 144, 128) and mv.shape == (1, 16, 112, 128, 128)
    assert torch.isfinite(f).all() and torch.isfinite(mv).all() and f.is_cuda


def test_two_window_batches_in_flight_give_identical_sums(device):
    """amx_unet_forward_windows_pipelined: consecutive window batches alternate two streams, only the accumulating launches are
    ordered -- the accumulated volume must be bit-identical to the single-stream sequence, repeatedly (no race on overlaps)."""
    from anatomix_amd.registration import sliding_window as SW
    m, _ = _model(device)
    x = R.synthetic_input(31, 1, (96, 80, 112)).to(device)
    kw = dict(overlap=0.8, mode="gaussian", sigma_scale=0.25)
    assert len(window_starts((96, 80, 112), (64, 64, 64), 0.8)) >= 16
    with torch.no_grad():
        SW.PIPELINE_WINDOWS = False
        try:
            want = sliding_window_inference(x, (64, 64, 64), 2, m, **kw)
        finally:
            SW.PIPELINE_WINDOWS = True
        for _ in range(3):
            got = sliding_window_inference(x, (64, 64, 64), 2, m, **kw)
            assert torch.equal(got, want)


def test_real_operating_point_roi128_overlap08_matches_cpu_oracle(device):
    """The reference's own configuration (convex_adam_utils.py:202-219: roi 128^3, overlap 0.8 -> scan interval 25, gaussian
    sigma_scale 0.25) on a 128 x 128 x 160 volume = 3 windows (x starts 0, 25, 32), fused HIP path vs the numpy oracle driving
    the fp32 CPU network.  f16 storage (the default of this variant): <= 1e-3 rel-L2."""
    m, sd = _model(device)
    vol = np.random.RandomState(8).rand(1, 128, 128, 160).astype(np.float32)
    starts = window_starts((128, 128, 160), (128, 128, 128), 0.8)
    assert [tuple(s) for s in starts] == [(0, 0, 0), (0, 0, 25), (0, 0, 32)]
    with torch.no_grad():
        x = torch.from_numpy(vol)[None].to(device)
        assert _fused_ok(m, x, (128, 128, 128))
        got = sliding_window_inference(x, (128, 128, 128), 2, m, overlap=0.8, mode="gaussian", sigma_scale=0.25).cpu()[0]
        torch.set_num_threads(16)
        ref = O.sliding_window(vol, (128, 128, 128), lambda a: R.forward(torch.from_numpy(a), sd, KW).numpy(), 0.8, "gaussian", 0.25)
    assert got.shape == (16, 128, 128, 160) and torch.isfinite(got).all()
    assert rel_l2(got, torch.from_numpy(ref)) <= 1e-3


def test_config2_full_schedule_256_cubed_343_windows(device):
    """BASELINE configs[1] at its full size: one 256^3 volume, roi 128, overlap 0.8, gaussian 0.25 = 7 x 7 x 7 = 343 windows with
    three-axis overlap, through extract_features' path (fused window batches, two batches in flight).  Checked on the output block
    that exactly 8 windows cover (oracle/sliding_window_ref.block_probe: 8 CPU forwards of the fp32 oracle, ~15 s)."""
    m, _ = _model(device)
    vol = R.synthetic_input(77, 1, (256, 256, 256)).to(device)
    assert len(window_starts((256, 256, 256), (128, 128, 128), 0.8)) == 343
    with torch.no_grad():
        assert _fused_ok(m, vol, (128, 128, 128))
        y = sliding_window_inference(vol, (128, 128, 128), 4, m, overlap=0.8, mode="gaussian", sigma_scale=0.25)
        torch.cuda.synchronize()
    assert y.shape == (1, 16, 256, 256, 256) and torch.isfinite(y).all()
    p = O.block_probe(y, vol, 128, "anatomix")
    assert p is not None
    assert p["rel_l2_vs_fp32_cpu_oracle"] <= 1e-3, p
    assert p["max_rel_vs_fp32_cpu_oracle"] <= 1.5e-3, p


def test_segmentation_validation_predictor_takes_the_fused_path(device):
    """train_segmentation.py:194-199: sliding_window_inference(val_images, roi, 4, nn.Sequential(Unet, UnetOutBlock), overlap=0.7),
    constant importance map.  The 1x1x1 head commutes with the window averaging, so the windows run fused up to the Unet's output
    and the head is applied once; the generic loop (head inside every window) is the reference order of operations."""
    from anatomix_amd.registration import sliding_window as SW
    m, _ = _model(device)
    torch.manual_seed(0)
    head = torch.nn.Conv3d(16, 5, kernel_size=1, bias=True).to(device)      # what MONAI's UnetOutBlock(3, 16, n_classes + 1) holds
    wrapped = torch.nn.Sequential(m, torch.nn.Sequential(torch.nn.Sequential(head))).eval()
    x = torch.from_numpy(np.random.RandomState(6).rand(1, 1, 64, 96, 80).astype(np.float32)).to(device)
    with torch.no_grad():
        assert SW._split_unet_and_head(wrapped, x, (64, 64, 64)) is not None
        calls = []
        orig = SW._run_fused
        SW._run_fused = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
        try:
            fused = sliding_window_inference(x, (64, 64, 64), 4, wrapped, overlap=0.7)
        finally:
            SW._run_fused = orig
        generic = sliding_window_inference(x, (64, 64, 64), 4, lambda t: wrapped(t), overlap=0.7)
    assert calls and fused.shape == generic.shape == (1, 5, 64, 96, 80)
    assert rel_l2(fused, generic) < 1e-5
    # a head that is not per-voxel affine keeps the generic loop
    nonlin = torch.nn.Sequential(m, torch.nn.Sequential(head, torch.nn.Softmax(dim=1))).eval()
    with torch.no_grad():
        assert SW._split_unet_and_head(nonlin, x, (64, 64, 64)) is None
    with torch.enable_grad():
        assert SW._split_unet_and_head(wrapped, x, (64, 64, 64)) is None


def test_output_widths_the_fused_step_cannot_accumulate_use_the_generic_loop(device):
    """output_nc = 8 leaves the network through the export pass (amx_unet.hip: final_via_export): the fused window entry would
    return AMX_ERR_SHAPE, so the dispatcher must not pick it (advisor finding, round 3)."""
    kw = dict(dimension=3, input_nc=1, output_nc=8, num_downs=2, ngf=16)
    m = anatomix_amd.Unet(**kw)
    sd = R.synthetic_state_dict(kw, 1)
    m.load_state_dict(sd)
    m = m.to(device).eval()
    x = torch.from_numpy(np.random.RandomState(7).rand(1, 1, 32, 48, 64).astype(np.float32)).to(device)
    with torch.no_grad():
        assert not _fused_ok(m, x, (32, 32, 32))
        got = sliding_window_inference(x, (32, 32, 32), 2, m, overlap=0.5).cpu()
    ref = O.sliding_window(x.cpu().numpy()[0], (32, 32, 32), lambda a: R.forward(torch.from_numpy(a), sd, kw).numpy(), 0.5, "constant", 0.125)
    assert got.shape == (1, 8, 32, 48, 64) and rel_l2(got[0], torch.from_numpy(ref)) <= 1e-3
