"""GPU: the epilogues of the z-march family (amx_conv3d_zmarch.hip, amx_conv3d_upcat.hip) after their per-step instruction stream
was cut -- one kernel symbol per activation, a predicate-free fast path for whole tiles and whole steps, advancing store pointers,
the range check and the fused pool on the vector unit.  None of that may change a stored bit:

  * every case is compared with the digest of what the commit before that work stored for the same seeded, CPU-generated inputs
    (tests/golden/zmarch_epilogue_digests.json, written by tools/make_golden_zmarch_epilogue.py on an MI355X at that commit; the
    range flags of that commit are recorded there too);
  * and with the float64 formulation of tests/test_conv_kernel_gpu.py at that file's tolerances.

Single layers go through amx_conv3d_k3_reflect_probe: the single-layer entry with the launch-side options of the forward (fused
max-pool output, importance map of the fp32 planar epilogue, range flag), which also returns the launch's ConvLaunchInfo name.  Every
case asserts that name, so none can pass on another route.  The stem-fed pair is reached through the 6 M model, where every launch
names its kernel (profile_forward).

Shapes: (2, 9, 10, 40) has an odd depth (a one-plane tail step) and partial tiles in y and x, so the guarded path and the fast path
run in one launch; (1, 8, 8, 32) is one whole tile: the pure fast path.  (Depths below 8 and heights below 8 are outside the z-march
kernels -- conv_zmarch_eligible -- and would test another kernel.)  Each activation is its own kernel symbol and has its own case.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import anatomix_amd
from _util import TORCH_T, from_ndhwc, max_rel, ref_conv, ref_conv_upcat_merged, to_ndhwc
from anatomix_amd import _lib
from anatomix_amd._lib import AmxOverflowError
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zmarch_epilogue_digests.json")
RAGGED, WHOLE, ODDW, POOLS, UP_WHOLE, UP_RAGGED = (2, 9, 10, 40), (1, 8, 8, 32), (1, 9, 10, 41), (2, 8, 12, 40), (2, 8, 8, 32), (1, 6, 12, 40)


def _case(c0, c1, co, s, a, planar=False, pool=False, wmap=False):
    cid = "c%d+%d_o%d_%s_a%d%s%s%s" % (c0, c1, co, "x".join(map(str, s)), a, "_planar" if planar else "", "_pool" if pool else "", "_wmap" if wmap else "")
    return (cid, c0, c1, co, s, a, planar, pool, wmap)


# (id, c0, c1, cout, (n, d, h, w), act, planar, pool, wmap)
LAYER_CASES = [
    _case(16, 0, 16, RAGGED, 1), _case(16, 0, 32, RAGGED, 1), _case(32, 0, 32, RAGGED, 1),
    _case(16, 0, 16, WHOLE, 1), _case(16, 0, 32, WHOLE, 1), _case(32, 0, 32, WHOLE, 1),
    _case(16, 0, 16, RAGGED, 0), _case(16, 0, 16, RAGGED, 2), _case(32, 0, 32, RAGGED, 0), _case(32, 0, 32, WHOLE, 2),
    _case(16, 0, 16, WHOLE, 0, planar=True), _case(16, 0, 16, RAGGED, 0, planar=True),      # fp32 planar: storer waves / direct ragged stores
    _case(16, 32, 16, UP_WHOLE, 1), _case(16, 32, 16, UP_RAGGED, 1), _case(16, 32, 16, UP_RAGGED, 0),
    # the fused max-pool: full and pooled tensor (relu: packed pool; no activation / leaky relu: fp32 pool)
    _case(16, 0, 16, POOLS, 1, pool=True), _case(16, 0, 32, POOLS, 1, pool=True), _case(32, 0, 32, POOLS, 1, pool=True),
    _case(32, 0, 32, POOLS, 0, pool=True), _case(16, 0, 16, POOLS, 2, pool=True),
    # fp32 planar output accumulating importance-weighted values into a pre-filled tensor: storer waves, 16-byte direct stores
    # (W % 4 == 0), scalar direct stores (odd W), and the merged-tap kernel's planar epilogue
    _case(16, 0, 16, WHOLE, 0, planar=True, wmap=True), _case(16, 0, 16, RAGGED, 0, planar=True, wmap=True),
    _case(16, 0, 16, ODDW, 0, planar=True, wmap=True), _case(16, 0, 16, ODDW, 0, planar=True),
    _case(16, 32, 16, UP_RAGGED, 0, planar=True, wmap=True), _case(16, 32, 16, UP_RAGGED, 0, planar=True),
]
ZERO_CASES = [LAYER_CASES[0], LAYER_CASES[2], LAYER_CASES[12]]
MODEL_CASES = [(1, (32, 32, 64)), (1, (32, 48, 96)), (2, (32, 32, 48))]
KW = R.VARIANTS["anatomix"]
TAPS = [5, 8, 9, 12, 15, 16, 57, 61, 64, 65]      # activations behind the z-march / upcat16 launches, the fused pools, the output conv


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def layer_inputs(c0, c1, cout, shape, special):
    n, d, h, w = shape
    rs = np.random.RandomState((c0 * 131 + c1 * 17 + cout * 7 + d * 1009 + h * 101 + w) & 0xFFFF)
    x0 = rs.randn(n, c0, d, h, w).astype(np.float32)
    if special:        # exact zeros and whole zero neighbourhoods (pre-activation == shift), for the signed-zero case
        x0[:, :, : d // 2] = 0.0
    x1 = rs.randn(n, c1, d // 2, h // 2, w // 2).astype(np.float32) if c1 else None
    if special and c1:
        x1[:, :, : d // 4] = 0.0
    wgt = (rs.randn(cout, c0 + c1, 3, 3, 3) / np.sqrt(27.0 * (c0 + c1))).astype(np.float32)
    scale = rs.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = (rs.randn(cout) * 0.1).astype(np.float32)
    if special:        # shifts of exactly zero and negatives far below the f16 subnormal range (2^-24): relu must store +0 for all
        shift[0::4] = 0.0
        shift[1::4] = -1.0e-9
        shift[2::4] = -3.0e-8
    wmap = rs.uniform(0.1, 1.0, (d, h, w)).astype(np.float32)
    prefill = rs.randn(n, cout, d, h, w).astype(np.float32)
    t = torch.from_numpy
    return t(x0), (t(x1) if c1 else None), t(wgt), t(scale), t(shift), t(wmap), t(prefill)


def probe(device, x0, x1, wgt, scale, shift, act, precision, planar=False, pool=False, wmap=None, prefill=None, slope=0.3):
    """amx_conv3d_k3_reflect_probe on CPU NCDHW float tensors -> dict(out, pool (or None), flag, kernel), outputs as NCDHW fp32 on the CPU."""
    lib = _lib.load()
    tdt = TORCH_T[precision]
    n, c0, d, h, w = x0.shape
    cout, c1 = wgt.shape[0], (0 if x1 is None else x1.shape[1])
    dev = lambda t: None if t is None else t.float().contiguous().to(device)
    dx0 = to_ndhwc(x0, tdt).to(device)
    dx1 = None if x1 is None else to_ndhwc(x1, tdt).to(device)
    dw, dsc, dsh, dwm = dev(wgt.reshape(cout, c0 + c1, 27)), dev(scale), dev(shift), dev(wmap)
    wpk = torch.empty(lib.amx_conv3d_packed_bytes(c0 + c1, cout), dtype=torch.uint8, device=device)
    o16 = o32 = p16 = None
    if planar:
        o32 = dev(prefill) if prefill is not None else torch.full((n, cout, d, h, w), float("nan"), dtype=torch.float32, device=device)
    else:
        o16 = torch.full((n, d, h, w, cout), float("nan"), dtype=tdt, device=device)
    if pool:
        p16 = torch.full((n, d // 2, h // 2, w // 2, cout), float("nan"), dtype=tdt, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    name = ctypes.create_string_buffer(64)
    st = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    _lib.check(lib.amx_conv3d_k3_reflect_probe(_lib.ptr(dx0), c0, _lib.ptr(dx1), c1, _lib.ptr(dw), _lib.ptr(dsc), _lib.ptr(dsh), cout, n, d, h, w,
                                               act, slope, _lib.PRECISION[precision], _lib.ptr(wpk), _lib.ptr(o16), _lib.ptr(o32), _lib.ptr(p16),
                                               _lib.ptr(dwm), _lib.ptr(flag), ctypes.cast(name, ctypes.c_void_p), st))
    torch.cuda.synchronize(device)
    return dict(out=o32.cpu() if planar else from_ndhwc(o16.float().cpu()), pool=None if p16 is None else from_ndhwc(p16.float().cpu()),
                flag=int(flag.item()), kernel=name.value.decode())


def run_layer(device, case, precision, special=False):
    _, c0, c1, cout, shape, act, planar, pool, wm = case
    x0, x1, wgt, scale, shift, wmap, prefill = layer_inputs(c0, c1, cout, shape, special)
    if planar:
        scale = shift = None
    got = probe(device, x0, x1, wgt, scale, shift, act, precision, planar=planar, pool=pool, wmap=wmap if wm else None, prefill=prefill if wm else None)
    return got, (x0, x1, wgt, scale, shift, wmap, prefill)


def assert_kernel(case, name):
    """The launch's own name (ConvLaunchInfo): family, channels, output mode, storer waves, fused pool."""
    _, c0, c1, cout, (n, d, h, w), act, planar, pool, wm = case
    if c1:
        assert name.startswith("conv3d_upcat16<") and name.endswith(",o%d>" % int(planar)), name
        return
    assert name.startswith("conv3d_k3_zmarch<") and ",%d->%d," % (c0, cout) in name and ",o%d" % int(planar) in name, name
    assert name.endswith(",pool>") == pool, name
    assert ("+s2," in name) == (planar and h % 8 == 0 and w % 32 == 0), name


# ---- the range flag: centre-tap-only weights of 2.0 (output channel c = 2 x input channel c, exact), one voxel set
def flag_cases():
    """(id, c0, c1, cout, shape, act, (z, y, x), value, raises in f16)"""
    out = []
    for c0, c1, co, whole, ragged, edge in [(16, 0, 16, WHOLE, RAGGED, (8, 9, 39)), (32, 0, 32, WHOLE, RAGGED, (8, 9, 39)),
                                            (16, 32, 16, UP_WHOLE, UP_RAGGED, (5, 11, 39))]:
        tag = "c%d+%d" % (c0, c1)
        out += [
            (tag + "_80000_first_step", c0, c1, co, whole, 1, (0, 0, 0), 40000.0, True),        # fast path, first interior step
            (tag + "_80000_tail_edge", c0, c1, co, ragged, 1, edge, 40000.0, True),             # guarded path: last plane, partial tile in y and x
            (tag + "_65504_exact", c0, c1, co, whole, 1, (0, 0, 0), 32752.0, False),             # the largest f16: not an overflow
            (tag + "_65504_exact_edge", c0, c1, co, ragged, 0, edge, -32752.0, False),
            (tag + "_minus80000_relu", c0, c1, co, whole, 1, (1, 2, 3), -40000.0, False),        # relu(-80000) = 0 is what is stored
            (tag + "_minus80000_none", c0, c1, co, ragged, 0, edge, -40000.0, True),             # the magnitude counts, not the sign
            (tag + "_nan_none", c0, c1, co, whole, 0, (2, 3, 4), float("nan"), True),
            (tag + "_nan_lrelu", c0, c1, co, ragged, 2, edge, float("nan"), True),
            (tag + "_nan_relu", c0, c1, co, whole, 1, (2, 3, 4), float("nan"), False),           # relu(NaN) = 0 is stored (v > 0 ? v : 0): nothing to flag
        ]
    return out


FLAG_CASES = flag_cases()


def run_flag(device, fc, precision):
    _, c0, c1, cout, shape, act, (z, y, x), value, _ = fc
    n, d, h, w = shape
    x0 = torch.zeros(n, c0, d, h, w)
    x0[n - 1, 3, z, y, x] = value
    x1 = torch.zeros(n, c1, d // 2, h // 2, w // 2) if c1 else None
    wgt = torch.zeros(cout, c0 + c1, 3, 3, 3)
    for c in range(min(cout, c0)):
        wgt[c, c, 1, 1, 1] = 2.0
    return probe(device, x0, x1, wgt, None, None, act, precision)


def all_entries(device):
    """Every golden entry: key -> digest (or the flag as an int).  tools/make_golden_zmarch_epilogue.py writes them at the reference commit."""
    for precision in ("f16", "bf16"):
        for case in LAYER_CASES:
            got, _ = run_layer(device, case, precision)
            yield "layer/%s/%s" % (case[0], precision), digest(got["out"])
            if got["pool"] is not None:
                yield "pool/%s/%s" % (case[0], precision), digest(got["pool"])
        for case in ZERO_CASES:
            yield "zero/%s/%s" % (case[0], precision), digest(run_layer(device, case, precision, special=True)[0]["out"])
        for fc in FLAG_CASES:
            got = run_flag(device, fc, precision)
            yield "flag/%s/%s" % (fc[0], precision), got["flag"]
            yield "flagout/%s/%s" % (fc[0], precision), digest(got["out"])
        for n, size in MODEL_CASES:
            _, taps, kern = run_model(device, precision, n, size)
            for i in TAPS:
                yield "model/%s/n%d_%dx%dx%d/tap%d" % (precision, n, *size, i), digest(taps[i])


def model(device, precision, sd=None):
    m = anatomix_amd.Unet(**KW)
    m.load_state_dict(sd if sd is not None else R.synthetic_state_dict(KW, 0), strict=True)
    m.precision = precision
    return m.to(device).eval()


def run_model(device, precision, n, size):
    m = model(device, precision)
    x = R.synthetic_input(300 + n, n, size).to(device)
    with torch.no_grad():
        y, feats = m.forward_hip_taps(x, TAPS)
        _, recs = m.profile_forward(x)
    return y, dict(zip(TAPS, feats)), {r["module_idx"]: r["kernel"] for r in recs}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layer_bits_and_fp64(device, case, precision):
    got, (x0, x1, wgt, scale, shift, wmap, prefill) = run_layer(device, case, precision)
    _, c0, c1, cout, shape, act, planar, pool, wm = case
    assert_kernel(case, got["kernel"])
    out = got["out"]
    assert torch.isfinite(out).all() and got["flag"] == 0
    ref = (ref_conv_upcat_merged if c1 else ref_conv)(x0, x1, wgt, scale, shift, act, precision)
    ulp = 2.0 ** -10 if precision == "f16" else 2.0 ** -7
    tol = ulp * ref.abs().double() + 1e-3 * ulp + 2e-5          # output stored in the 16-bit type: one rounding of the result
    if planar:
        if wm:      # out = prefill + wmap * value, accumulated in fp32
            ref = (prefill.double() + wmap.double()[None, None] * ref.double()).float()
        assert max_rel(out, ref) < 2e-5, max_rel(out, ref)
    else:
        err = (out.double() - ref.double()).abs()
        assert (err <= tol).all(), err.max().item()
    want = golden()
    assert digest(out) == want["layer/%s/%s" % (case[0], precision)]
    if pool:
        pooled = got["pool"]
        assert torch.equal(pooled, F.max_pool3d(out, 2))                                   # the pool of what was stored, bit for bit
        perr = (pooled.double() - F.max_pool3d(ref.double(), 2)).abs()                     # |max a - max b| <= max |a - b| over the window
        assert (perr <= F.max_pool3d(tol, 2)).all(), perr.max().item()
        assert digest(pooled) == want["pool/%s/%s" % (case[0], precision)]


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("case", ZERO_CASES, ids=lambda c: c[0])
def test_non_positive_preactivations_store_plus_zero(device, case, precision):
    """Pre-activations that are exact zeros and negatives below the f16 subnormal range: behind the relu every one is stored as +0
    (a packed 16-bit relu would keep the -0 that the rounding of a tiny negative gives), bit for bit as before."""
    got = run_layer(device, case, precision, special=True)[0]
    assert_kernel(case, got["kernel"])
    out = got["out"]
    zero_half = out[:, :, : case[4][1] // 2 - 1]        # outputs whose whole neighbourhood is zero: relu(shift)
    assert (zero_half[:, 0::4] == 0).all() and (zero_half[:, 1::4] == 0).all() and (zero_half[:, 2::4] == 0).all()
    assert not torch.signbit(out).any()
    assert digest(out) == golden()["zero/%s/%s" % (case[0], precision)]


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("fc", FLAG_CASES, ids=[f[0] for f in FLAG_CASES])
def test_range_flag_exact(device, fc, precision):
    """The predicate is !(|v| <= 65504) on the activated value about to be stored, NaN included; nothing is raised for bf16."""
    cid, c0, c1, cout, shape, act, (z, y, x), value, raises = fc
    got = run_flag(device, fc, precision)
    assert_kernel((cid, c0, c1, cout, shape, act, False, False, False), got["kernel"])
    v = got["out"][shape[0] - 1, 3, z, y, x].item()
    if precision == "f16":
        assert got["flag"] == int(raises), (got["flag"], v)
        if value == value and abs(value) == 32752.0:
            assert v == (2.0 * value if (act == 0 or value > 0) else 0.0)      # exactly +-65504, stored as such
    else:
        assert got["flag"] == 0
    if value != value and act == 1:
        assert v == 0.0
    want = golden()
    assert got["flag"] == want["flag/%s/%s" % (cid, precision)]                # as the reference commit raised it
    assert digest(got["out"]) == want["flagout/%s/%s" % (cid, precision)]


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("n,size", MODEL_CASES, ids=["n%d_%dx%dx%d" % (n, *s) for n, s in MODEL_CASES])
def test_model_launches_bits_and_pools(device, precision, n, size):
    y, taps, kern = run_model(device, precision, n, size)
    whole_x = size[2] % 32 == 0
    # the intended kernels ran: the stem-fed pair (whole x tiles), the fused pools, upcat16, the storer waves of the planar output
    if whole_x:
        assert "stem1->16->16" in kern[0] and "conv3d_k3_zmarch" in kern[0] and 3 not in kern
    else:
        assert kern[3].startswith("conv3d_k3_zmarch<") and "16->16" in kern[3]
    assert kern[6].startswith("conv3d_k3_zmarch<") and "16->16" in kern[6] and kern[6].endswith(",pool>") and 9 not in kern
    assert kern[59].startswith("conv3d_upcat16<") and kern[62].startswith("conv3d_k3_zmarch<")
    assert kern[65].startswith("conv3d_k3_zmarch<") and ",o1" in kern[65] and (("+s2," in kern[65]) == (whole_x and size[1] % 8 == 0))
    if size[2] >= 64:                                    # level 1 is wide enough for the 32-channel z-march kernels
        assert "16->32" in kern[10] and kern[10].startswith("conv3d_k3_zmarch<")
        assert "32->32" in kern[13] and kern[13].endswith(",pool>") and 16 not in kern
        assert "32->32" in kern[55] and kern[55].startswith("conv3d_k3_zmarch<")
    # the pooled tensors are the max-pool of the full-resolution tensors, bit for bit
    assert torch.equal(taps[9], F.max_pool3d(taps[8], 2)) and torch.equal(taps[16], F.max_pool3d(taps[15], 2))
    assert torch.isfinite(y).all() and torch.equal(taps[65], y)
    want = golden()
    key = "model/%s/n%d_%dx%dx%d" % (precision, n, *size)
    for i in TAPS:
        assert digest(taps[i]) == want["%s/tap%d" % (key, i)], f"module {i}"


def _scaled(key, factor=None, add=None):
    sd = R.synthetic_state_dict(KW, 0)
    if factor is not None:
        sd[key] = sd[key] * factor
    if add is not None:
        sd[key] = sd[key] + add
    return sd


# BatchNorm gains / shifts behind: the stem-fed pair's 16 -> 16 conv (module 3), the 16 -> 16 + pool conv (6), the 32 -> 32 + pool conv
# (13, two-chunk instance: its range check is reduced per step), upcat16 (59); test_model_launches_bits_and_pools asserts the kernels of
# this shape
@pytest.mark.parametrize("bn", [4, 7, 14, 60])
def test_range_flag_from_each_epilogue(device, bn):
    x = R.synthetic_input(100, 1, (32, 32, 64)).to(device)
    with torch.no_grad():
        m = model(device, "f16", _scaled("model.%d.weight" % bn, factor=3e5))
        y = m(x)
        torch.cuda.synchronize()
        assert torch.isnan(y).all()
        with pytest.raises(AmxOverflowError, match="f16 range"):
            m.check_numerics()
        # far below zero behind the relu: +0 is the right answer and no overflow
        m = model(device, "f16", _scaled("model.%d.bias" % bn, add=-1e6))
        y = m(x)
        m.check_numerics()
        assert torch.isfinite(y).all()
        # bf16 has fp32's exponent range: nothing is raised
        m = model(device, "bf16", _scaled("model.%d.weight" % bn, factor=3e5))
        y = m(x)
        m.check_numerics()
        assert torch.isfinite(y).all()
