"""GPU parity of precision ``f16x2mx`` (AMX_PREC_F16X2_MX, include/anatomix_amd.h): strict f16 hi + lo storage whose two correction
products (Wh*xl + Wl*xh) run on CDNA4's block-scaled fp8 matrix instruction from e4m3 copies stored beside the pair -- 2.0 instead of
3.0 MFMA-equivalents per product.  It is the compliant mode of the InstanceNorm variant ``anatomix-dev`` (BASELINE configs[3],
/root/reference/anatomix/model/load_from_hf.py:18-24; the reference's inference callers run fp32,
anatomix/registration/convex_adam_utils.py:194-219), so it is held to the same 1e-3 bar as ``strict``:

  * the conv kernel against a CPU restatement of EXACTLY its arithmetic (f16 main product + e4m3 corrections under one block scale)
    on every tile configuration of the generic kernel -- layout, tap order, scale and conversion bugs show up at 1e-2, the bound is 2e-6;
  * the passes that write the e4m3 copies (norm apply, pool, upsample): value identical to f16x2, copy bytes identical to torch's
    float8_e4m3fn conversion;
  * the whole network against the fp32 oracle and the golden vectors captured from the imported reference.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _util import check_copies as _check_copies
from _util import from_ndhwc_mx, max_rel, ref_conv_fp64, ref_conv_mx, rel_l2, run_conv, to_ndhwc_mx
import anatomix_amd
from anatomix_amd import _lib
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-3
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "unet_forward_golden.npz"))
TAPG = np.load(os.path.join(os.path.dirname(__file__), "golden", "unet_taps_golden.npz"))
P = "f16x2mx"

CASES = [
    # (c0, c1, cout, (d,h,w), n, act): one per brick / Q / NCH configuration of the generic kernel + ragged and two-segment inputs
    (16, 0, 16, (8, 16, 32), 2, 0),       # Q=1, 4x8x32
    (32, 0, 32, (8, 8, 64), 1, 1),        # Q=2, 4x4x32: the level-0 layers of anatomix-dev
    (32, 64, 32, (8, 8, 32), 1, 1),       # 96 -> 32, second segment through the nearest gather
    (64, 0, 64, (8, 8, 32), 1, 1),        # Q=4, W>=32
    (32, 0, 64, (8, 8, 16), 1, 1),        # W=16 class
    (64, 128, 64, (8, 8, 16), 1, 2),      # 192 -> 64 @16, leaky relu
    (128, 0, 128, (16, 16, 16), 1, 1),    # loader-wave configuration
    (128, 0, 256, (8, 8, 8), 1, 1),       # 8^3 bricks
    (256, 0, 256, (8, 8, 8), 2, 1),
    (48, 0, 16, (6, 10, 20), 1, 1),       # ragged: partial bricks on every axis, 3 chunks
    (16, 0, 16, (2, 2, 2), 1, 1),         # minimum legal size for reflect
    (64, 0, 128, (4, 4, 4), 1, 1),
    (16, 0, 16, (33, 17, 35), 1, 1),      # odd sizes
]


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%d+%d_o%d_%dx%dx%d_n%d_a%d" % (c[0], c[1], c[2], *c[3], c[4], c[5]))
def test_conv_mx_matches_its_restated_arithmetic(device, case):
    c0, c1, cout, (d, h, w), n, act = case
    rs = np.random.RandomState(hash((c0, c1, cout, d, h, w)) & 0xFFFF)
    # activations with a realistic spread of magnitudes (post-norm, post-ReLU like): exercises the e4m3 subnormal range too
    x0 = torch.from_numpy((rs.randn(n, c0, d, h, w) * np.exp(rs.randn(1, c0, 1, 1, 1))).astype(np.float32)).clamp_min(-0.2)
    x1 = torch.from_numpy(rs.randn(n, c1, d // 2, h // 2, w // 2).astype(np.float32)) if c1 else None
    wgt = torch.from_numpy((rs.randn(cout, c0 + c1, 3, 3, 3) / np.sqrt(27.0 * (c0 + c1))).astype(np.float32))
    scale = torch.from_numpy(rs.uniform(0.5, 1.5, cout).astype(np.float32))
    shift = torch.from_numpy((rs.randn(cout) * 0.1).astype(np.float32))
    got = run_conv(device, x0, x1, wgt, scale, shift, act, P)
    ref = ref_conv_mx(x0, x1, wgt, scale, shift, act)
    assert torch.isfinite(got).all()
    # what is left: fp32 accumulation (up to 10368 terms), the fp8 instruction's own accumulation of the 2^-11-sized corrections,
    # and the f16 hi + lo split of the stored result (2^-22)
    assert rel_l2(got, ref) < 2e-6 and max_rel(got, ref) < 1e-5, (rel_l2(got, ref), max_rel(got, ref))
    # and against the un-rounded fp32 operands: 15-16 significant operand bits
    full = ref_conv_fp64(x0, x1, wgt, scale, shift, act)
    assert rel_l2(got, full) < 4e-5, rel_l2(got, full)


def test_conv_mx_planar_output_and_saturating_copies(device):
    """fp32 planar epilogue (the output conv) + activations beyond e4m3's range: their correction terms are clipped, nothing overflows."""
    rs = np.random.RandomState(5)
    x0 = torch.from_numpy(rs.randn(1, 32, 8, 8, 32).astype(np.float32))
    x0[0, 3, 2, 2, 5] = 3000.0
    x0[0, 7, 1, 4, 9] = -900.0
    wgt = torch.from_numpy((rs.randn(32, 32, 3, 3, 3) / np.sqrt(27.0 * 32)).astype(np.float32))
    shift = torch.from_numpy((rs.randn(32) * 0.1).astype(np.float32))
    got = run_conv(device, x0, None, wgt, None, shift, 0, P, planar=True)
    ref = ref_conv_mx(x0, None, wgt, None, shift, 0)
    assert torch.isfinite(got).all() and rel_l2(got, ref) < 2e-6, rel_l2(got, ref)


@pytest.mark.parametrize("shape", [(1, 32, 4, 6, 8), (2, 64, 3, 5, 7), (1, 256, 2, 2, 2)])
def test_mx_elementwise_passes_write_value_and_copies(device, shape):
    lib = _lib.load()
    n, c, d, h, w = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g) * (0.1 + 3.0 * torch.rand(1, c, 1, 1, 1, generator=g))
    xq = from_ndhwc_mx(to_ndhwc_mx(x), c)[0]                                   # the stored (hi + lo) values
    # --- trilinear upsample
    dx = to_ndhwc_mx(x).to(device)
    out = torch.full((n, 2 * d, 2 * h, 3 * c // 16, 2 * w, 32), 0x7f, dtype=torch.uint8, device=device)
    _lib.check(lib.amx_upsample2_trilinear(_lib.ptr(dx), _lib.ptr(out), n, d, h, w, c, _lib.PRECISION[P], _stream(device)))
    torch.cuda.synchronize(device)
    got = _check_copies(out.cpu(), c, "upsample")
    ref = F.interpolate(xq.double(), scale_factor=2, mode="trilinear").float()
    assert rel_l2(got, ref) < 1e-6
    # --- average / max pool of the upsampled tensor
    for avg in (1, 0):
        pooled = torch.full((n, d, h, 3 * c // 16, w, 32), 0x7f, dtype=torch.uint8, device=device)
        _lib.check(lib.amx_pool2(_lib.ptr(out), _lib.ptr(pooled), n, d, h, w, c, avg, _lib.PRECISION[P], _stream(device)))
        torch.cuda.synchronize(device)
        gp = _check_copies(pooled.cpu(), c, "pool")
        rp = (F.avg_pool3d if avg else F.max_pool3d)(got.double(), 2).float()
        assert rel_l2(gp, rp) < 1e-6
    # --- instance norm + ReLU in place (a raw conv output carries no copies: poison them first)
    # (the entry has no row length: a sample is ONE row of d*h*w voxels)
    xrow = x.reshape(n, c, 1, 1, d * h * w)
    raw = to_ndhwc_mx(xrow)
    raw[:, :, :, 2 * (c // 16):] = 0x7f
    dn = raw.to(device)
    scratch = torch.empty(lib.amx_instance_norm_scratch_bytes(n, c), dtype=torch.uint8, device=device)
    _lib.check(lib.amx_instance_norm(_lib.ptr(dn), None, None, 1e-2, n, d * h * w, c, 1, 0.3, _lib.ptr(scratch), _lib.PRECISION[P],
                                     _stream(device)))
    torch.cuda.synchronize(device)
    gn = _check_copies(dn.cpu(), c, "instance norm")
    rn = F.relu(F.instance_norm(xq.double(), eps=1e-2)).float().reshape(n, c, 1, 1, d * h * w)
    assert rel_l2(gn, rn) < 2e-6


def _model(device, variant, seed, precision=P):
    kw = R.VARIANTS[variant] if isinstance(variant, str) else variant
    m = anatomix_amd.Unet(**kw)
    sd = R.synthetic_state_dict(kw, seed)
    m.load_state_dict(sd, strict=True)
    m.precision = precision
    return m.to(device).eval(), sd, kw


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("size,n", [((64, 64, 64), 1), ((64, 96, 64), 2)])
def test_dev_mx_meets_the_north_star(device, size, n, seed):
    m, sd, kw = _model(device, "anatomix-dev", seed)
    x = R.synthetic_input(100 + seed, n, size)
    with torch.no_grad():
        y = m(x.to(device)).cpu()
        ref = R.forward(x, sd, kw)
    e, mx = rel_l2(y, ref), max_rel(y, ref)
    print(f"anatomix-dev {P} seed {seed} {size} n={n}: rel-L2 {e:.2e} max-rel {mx:.2e}")
    assert torch.isfinite(y).all() and e <= 6e-4 and mx <= NORTH_STAR, (e, mx)


def test_dev_mx_at_the_128_cube_operating_size(device):
    """BASELINE configs[3]: 1x1x128^3, full fp32 oracle on the host, plus the reference's golden probes."""
    m, sd, kw = _model(device, "anatomix-dev", 0)
    x = R.synthetic_input(100, 1, (128, 128, 128))
    with torch.no_grad():
        y = m(x.to(device)).cpu()
        ref = R.forward(x, sd, kw)
    e, mx = rel_l2(y, ref), max_rel(y, ref)
    print(f"anatomix-dev {P} 128^3: rel-L2 {e:.2e} max-rel {mx:.2e}")
    assert e <= 6e-4 and mx <= NORTH_STAR, (e, mx)
    tag = "anatomix-dev|s0|128|g1.0000"          # probes of the REFERENCE's own forward at this size (oracle/make_golden.py)
    got = y.flatten()[torch.from_numpy(GOLD[tag + "|idx"]).long()]
    assert rel_l2(got, torch.from_numpy(GOLD[tag + "|val"]).float()) <= NORTH_STAR


def test_dev_mx_golden_probes_and_taps_from_the_reference(device):
    for seed in (0, 1):
        tag = f"anatomix-dev|s{seed}|64|g1.0000"
        m, sd, kw = _model(device, "anatomix-dev", seed)
        x = R.synthetic_input(100 + seed, 1, (64, 64, 64))
        with torch.no_grad():
            y = m(x.to(device)).cpu()
        got = y.flatten()[torch.from_numpy(GOLD[tag + "|idx"]).long()]
        assert rel_l2(got, torch.from_numpy(GOLD[tag + "|val"]).float()) <= NORTH_STAR
    tag = "anatomix-dev|s0|64"
    taps = [int(t) for t in TAPG[tag + "|taps"]]
    m, sd, kw = _model(device, "anatomix-dev", 0)
    x = R.synthetic_input(100, 1, (64,) * 3)
    with torch.no_grad():
        y, feats = m(x.to(device), taps)
    for t, f in zip(taps, feats):
        f = f.cpu()
        got = f.reshape(-1)[torch.from_numpy(TAPG[tag + f"|tap{t}|idx"])]
        assert rel_l2(got, torch.from_numpy(TAPG[tag + f"|tap{t}|val"])) <= NORTH_STAR, t


@pytest.mark.parametrize("kw,size", [
    (dict(dimension=3, input_nc=1, output_nc=16, num_downs=3, ngf=16, norm="instance_affine", interp="trilinear", pooling="Avg"),
     (32, 48, 32)),
    (dict(dimension=3, input_nc=1, output_nc=16, num_downs=2, ngf=16, norm="instance", interp="nearest", pooling="Max",
          norm_eps=1e-2, activation="lrelu"), (32, 48, 32)),                                  # nearest upsample: the gather path
    (dict(dimension=3, input_nc=1, output_nc=24, num_downs=2, ngf=24, norm="instance", interp="trilinear", pooling="Avg"),
     (16, 16, 32)),                                                                           # padded widths, output through the export pass
    # 32-wide level 0 at whole 2x32 tiles: the normalise-on-load kernel (pending norms, its fp32 planar output conv), statistics in the
    # stem, apply + MAX pool in one pass, pending norm inside the trilinear upsample
    (dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance", interp="trilinear", pooling="Max", norm_eps=1e-2),
     (32, 64, 64)),
    (dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance_affine", interp="nearest", pooling="Avg",
          activation="lrelu"), (16, 36, 32)),                                                 # H = 36: 18 tiles of 2 rows
])
def test_mx_other_instance_norm_networks(device, kw, size):
    m, sd, _ = _model(device, kw, 3)
    x = R.synthetic_input(7, 2, size)
    with torch.no_grad():
        y = m(x.to(device)).cpu()
        ref = R.forward(x, sd, kw)
    assert y.shape == ref.shape and rel_l2(y, ref) <= 5e-4, (kw, rel_l2(y, ref))


def test_mx_is_refused_where_it_is_not_implemented(device):
    m = anatomix_amd.Unet(**R.VARIANTS["anatomix"])
    m.load_state_dict(R.synthetic_state_dict(R.VARIANTS["anatomix"], 0))
    m.precision = P
    m = m.to(device).eval()
    with pytest.raises(_lib.AmxError, match="InstanceNorm"), torch.no_grad():
        m(R.synthetic_input(1, 1, (32, 32, 32)).to(device))


def test_mx_determinism_and_batch_independence(device):
    m, sd, kw = _model(device, "anatomix-dev", 0)
    x = R.synthetic_input(5, 2, (64, 64, 64)).to(device)
    with torch.no_grad():
        y2, y0, y1, y2b = m(x), m(x[:1]), m(x[1:]), m(x)
    assert torch.equal(y2[:1], y0) and torch.equal(y2[1:], y1) and torch.equal(y2, y2b)


@pytest.mark.parametrize("key,gain", [("model.3.weight", 1e6),      # raw conv output of the normalise-on-load kernel beyond f16
                                      ("model.1.weight", 1e6)])     # InstanceNorm gain: the value its converters normalise to
def test_mx_f16_range_is_guarded_in_the_fused_kernels(device, key, gain):
    kw = dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance_affine", interp="trilinear", pooling="Avg")
    sd = R.synthetic_state_dict(kw, 2)
    sd[key] = sd[key] * gain
    m = anatomix_amd.Unet(**kw)
    m.load_state_dict(sd)
    m.precision = P
    m = m.to(device).eval()
    with torch.no_grad():
        y = m(R.synthetic_input(4, 1, (16, 32, 32)).to(device))
        with pytest.raises(_lib.AmxOverflowError):
            m.check_numerics()
    assert torch.isnan(y).all()
