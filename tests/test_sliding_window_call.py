"""No GPU: the host side of the single-call sliding window -- amx_sw_plan against window_starts (count, order, corners), its
refusals, and the surface of the prediction command."""
import ctypes

import pytest
import torch

from anatomix_amd import _lib
from anatomix_amd.registration.sliding_window import window_starts

# (size, roi, overlap, windows)
CASES = [((80, 72, 100), (64, 64, 64), 0.8, 24),
         ((64, 96, 80), (64, 64, 64), 0.7, 6),
         ((40, 36, 44), (32, 32, 32), 0.8, 18),
         ((33, 35, 37), (32, 32, 32), 0.5, 8),
         ((256, 256, 256), (128, 128, 128), 0.8, 343)]


def plan(size, roi, overlap, capacity=None, fill=-7):
    """(status or count, corners written, the whole buffer) of amx_sw_plan with a buffer of ``capacity`` windows + 4 guard windows."""
    lib = _lib.load()
    if capacity is None:
        capacity = max(lib.amx_sw_plan(*size, *roi, overlap, None, 0), 0)
    buf = (ctypes.c_int * (3 * (capacity + 4)))(*([fill] * (3 * (capacity + 4))))
    n = lib.amx_sw_plan(*size, *roi, overlap, buf, capacity)
    vals = list(buf)
    return n, [tuple(vals[3 * i:3 * i + 3]) for i in range(min(max(n, 0), capacity))], vals


@pytest.mark.parametrize("size,roi,overlap,windows", CASES)
def test_plan_equals_window_starts(size, roi, overlap, windows):
    want = window_starts(size, roi, overlap)
    n, got, vals = plan(size, roi, overlap)
    assert n == windows == len(want)
    assert got == [tuple(s) for s in want]
    assert all(v == -7 for v in vals[3 * n:])                 # nothing past the windows
    for (z, y, x) in got:
        assert 0 <= z <= size[0] - roi[0] and 0 <= y <= size[1] - roi[1] and 0 <= x <= size[2] - roi[2]


def test_plan_last_corner_of_the_first_case():
    assert plan((80, 72, 100), (64, 64, 64), 0.8)[1][-1] == (16, 8, 36)


def test_plan_axis_equal_to_the_roi():
    """An axis equal to the roi has one start (interval = roi), whatever the overlap."""
    for size, roi, ov in [((64, 96, 64), (64, 64, 64), 0.5), ((32, 32, 32), (32, 32, 32), 0.9), ((40, 32, 70), (32, 32, 48), 0.25)]:
        want = window_starts(size, roi, ov)
        n, got, _ = plan(size, roi, ov)
        assert n == len(want) and got == [tuple(s) for s in want]
        for k in range(3):
            if size[k] == roi[k]:
                assert {c[k] for c in got} == {0}
    assert plan((32, 32, 32), (32, 32, 32), 0.9)[0] == 1


def test_plan_interval_floored_to_one():
    """int(roi * (1 - overlap)) == 0 -> interval 1: one window per voxel of slack."""
    size, roi, ov = (35, 32, 34), (32, 32, 32), 0.99
    assert int(32 * (1 - ov)) == 0
    want = window_starts(size, roi, ov)
    n, got, _ = plan(size, roi, ov)
    assert n == 4 * 1 * 3 == len(want) and got == [tuple(s) for s in want]
    assert sorted({c[0] for c in got}) == [0, 1, 2, 3]


def test_plan_overlap_is_taken_in_double():
    """The interval is int(roi * (1 - overlap)) in double, as Python forms it (0.8 -> int(128 * 0.19999999999999996) = 25): every
    overlap in steps of 0.05 gives the corners of the Python arithmetic."""
    for i in range(0, 20):
        ov = i * 0.05
        for size, roi in [((100, 64, 77), (64, 64, 64)), ((50, 41, 33), (32, 32, 32))]:
            want = window_starts(size, roi, ov)
            n, got, _ = plan(size, roi, ov)
            assert n == len(want) and got == [tuple(s) for s in want], (ov, size)


def test_plan_volume_smaller_than_roi_is_a_shape_error():
    lib = _lib.load()
    for size in [(31, 40, 40), (40, 31, 40), (40, 40, 31)]:
        n, got, vals = plan(size, (32, 32, 32), 0.5, capacity=4)
        assert n == _lib.AMX_ERR_SHAPE and got == [] and all(v == -7 for v in vals)
        assert b"smaller than the roi" in lib.amx_last_error()
    assert plan((40, 40, 40), (32, 32, 32), 1.0, capacity=4)[0] == _lib.AMX_ERR_INVALID
    assert plan((40, 40, 40), (32, 32, 32), -0.1, capacity=4)[0] == _lib.AMX_ERR_INVALID


def test_plan_capacity_too_small_returns_the_count_and_stays_inside():
    size, roi, ov = (40, 36, 44), (32, 32, 32), 0.8
    want = [tuple(s) for s in window_starts(size, roi, ov)]
    for cap in (0, 1, 5, 17):
        n, got, vals = plan(size, roi, ov, capacity=cap)
        assert n == 18
        assert got == want[:cap]
        assert all(v == -7 for v in vals[3 * cap:])
    assert _lib.load().amx_sw_plan(*size, *roi, ov, None, 0) == 18
    assert _lib.load().amx_sw_plan(*size, *roi, ov, None, 3) == _lib.AMX_ERR_INVALID


def test_predict_parser_defaults():
    from anatomix_amd.segmentation import predict, train_segmentation
    opt = predict.build_parser().parse_args(["--images", "a.nii.gz", "b.nii.gz", "--ckpt", "c.pth"])
    assert opt.images == ["a.nii.gz", "b.nii.gz"] and opt.ckpt == "c.pth" and opt.labels is None
    assert (opt.roi, opt.overlap, opt.device, opt.out_dir) == (128, 0.7, "cuda", "segmentations")
    ref = train_segmentation.build_parser().parse_args(["--pretrained_ckpt", "scratch"])
    for flag in ("n_classes", "num_downs", "ngf", "output_nc", "norm", "interp", "pooling"):
        assert getattr(opt, flag) == getattr(ref, flag), flag
    assert opt.roi == ref.crop_size
    with pytest.raises(SystemExit):
        predict.build_parser().parse_args(["--ckpt", "c.pth"])
    assert callable(predict.main)


def test_segment_volume_refuses_a_cpu_tensor():
    import anatomix_amd
    from anatomix_amd.segmentation.predict import segment_volume
    from anatomix_amd.segmentation.segmentation_utils import UnetOutBlock
    from oracle import unet_ref as R
    model = torch.nn.Sequential(anatomix_amd.Unet(**R.VARIANTS["anatomix"]), UnetOutBlock(3, 16, 5)).eval()
    with pytest.raises(RuntimeError, match="no host path"):
        segment_volume(model, torch.zeros(32, 32, 32), roi=32)


def test_sliding_window_volume_refuses_a_cpu_tensor_and_names_the_other_route():
    import anatomix_amd
    from anatomix_amd.registration.sliding_window import sliding_window_volume
    from oracle import unet_ref as R
    m = anatomix_amd.Unet(**R.VARIANTS["anatomix"]).eval()
    with pytest.raises(_lib.AmxEnvelopeError, match="no host path.*sliding_window_inference"):
        sliding_window_volume(torch.zeros(1, 1, 32, 32, 32), 32, m)
    with pytest.raises(ValueError, match="out must be"):
        sliding_window_volume(torch.zeros(1, 1, 32, 32, 32), 32, m, out="probabilities")
