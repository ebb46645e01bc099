"""The conv launchers report what they ran to their caller and keep nothing between calls: a profiled forward launches what a
plain forward launches and names every conv it ran, and neither a statistics slot count nor a route survives from one forward
into the next -- not across shapes, not across networks.
"""
import pytest
import torch

import anatomix_amd
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu

DEV = R.VARIANTS["anatomix-dev"]
# the instance-norm, nearest-upsample mix of test_unet_dev_gpu.py::test_mixed_mode_networks
MIX = dict(dimension=3, input_nc=1, output_nc=16, num_downs=2, ngf=16, norm="instance", interp="nearest", pooling="Max", norm_eps=1e-2,
           activation="lrelu")


def _model(device, kw, seed, precision=None):
    m = anatomix_amd.Unet(**kw)
    m.load_state_dict(R.synthetic_state_dict(kw, seed), strict=True)
    m.precision = precision          # None: the default of the configuration
    return m.to(device).eval()


@pytest.mark.parametrize("variant,precision,size", [("anatomix", "f16", (32, 32, 32)), ("anatomix", "bf16x2", (32, 32, 32)),
                                                    ("anatomix-dev", None, (64, 64, 64))])
def test_profile_forward_equals_forward_and_names_every_conv(device, variant, precision, size):
    m = _model(device, R.VARIANTS[variant], 0, precision)
    x = R.synthetic_input(100, 1, size).to(device)
    with torch.no_grad():
        y = m(x)
        yp, recs = m.profile_forward(x)
    assert torch.equal(y, yp)
    convs = [r for r in recs if isinstance(m.model[r["module_idx"]], torch.nn.Conv3d)]
    assert convs
    for r in convs:
        assert r["kernel"].startswith("conv3d_"), r


def test_nothing_survives_from_one_launch_into_the_next(device):
    """m(a), m(b), m2(b), m(a): the first and the last result are equal bit for bit, and equal to m(a) of a fresh model.  a = 64^3;
    b = 32 x 48 x 32 for the two-level network m2.  anatomix-dev has five levels and refuses that shape (its bottleneck would be one
    voxel), so it takes b at twice the size, 64 x 96 x 64: another shape than a, hence other slot counts and grids, all the same."""
    m, m2 = _model(device, DEV, 0), _model(device, MIX, 3)
    a = R.synthetic_input(100, 1, (64, 64, 64)).to(device)
    b_dev = R.synthetic_input(7, 1, (64, 96, 64)).to(device)
    b = R.synthetic_input(7, 1, (32, 48, 32)).to(device)
    with torch.no_grad():
        first = m(a).clone()
        m(b_dev)
        m2(b)
        last = m(a)
        fresh = _model(device, DEV, 0)(a)
    assert torch.isfinite(first).all()
    assert torch.equal(first, last)
    assert torch.equal(first, fresh)
