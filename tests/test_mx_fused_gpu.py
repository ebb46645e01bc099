"""GPU: the fused launches of the f16x2mx schedule, each alone through its probe entry (include/anatomix_amd.h: amx_conv3d_zx_probe,
amx_instance_norm_probe, amx_instance_norm_apply_pool_probe, amx_upsample2_trilinear_pending), against the float64 restatements of
tests/_mx_fused_ref.py; tests/test_mx_fused.py proves on the host that each comparison made here fails on a planted defect and names
the launch.  Run this module after touching amx_conv3d_zx.hip or the f16x2mx passes of amx_norm.hip -- as a whole: the route test at
its end needs the kernel names the probe tests collect.

What the probes prove is the launches.  How Forward (amx_unet.hip) binds them -- which tensor, which (a, b) buffer, which slot count --
stays under the end-to-end tests of test_mx_precision_gpu.py; ROUTE_TABLE below pins which of them a plain forward makes.

Where this module departs from the text of its issue, and why:
  * apply + pool at (1, 2, 4, 40, 48): w c / 8 = 240 is no multiple of 64, so in_apply_pool_eligible refuses it (a wave of the kernel
    must hold whole lane quads of one row).  The case stays, as the refusal it is; (1, 2, 4, 40, 64), w c / 8 = 320 = 256 + 64, is the
    eligible shape with a tail in the kernel's t loop.
  * routes of anatomix-dev: num_downs = 5 needs 64 voxels per axis, so (16, 16, 32) and (16, 32, 32) are refused by the handle; the
    smallest legal volume (64, 64, 64) and (64, 96, 64) stand in.
  * per-element bounds of stored values carry the term 2^-22 |y| for the pair, which an f16 lo below 2^-14 (a subnormal, spacing
    2^-24) cannot meet when |y| < 2^-3: _mx_fused_ref.check_stored_value holds that bound wherever it can hold and, everywhere, the
    exact interval it abbreviates.
  * skip_lo of the in-place apply: store8 skips the lo store, so the lo planes keep the INPUT's lo bytes (they were read as input and
    cannot hold poison); the poison survives in the lo planes of the separate outputs (pooled tensor, upsampled tensor).

Tolerance of (a, b): 8 x the worst relative deviation that tests/_mx_fused_ref.finalize_f32, an all-fp32 emulation of the slot-wise
summation and of the finalize, shows against float64 on the very inputs of the case (the device adds fp32 slots in float64, or in fp32
chunks above 512 slots, and rounds rstd, the mean and the products to fp32; the factor is for its lane order).

Figures of one MI355X run (profiles/mx_fused_gpu.txt holds all of them; AMX_FUSED_REPORT=<file> appends them after a run of this
module).  Per launch kind the worst error / tolerance ("per-element" and "slots": the worst ratio itself), then the measured deviation of
(a, b), the fp32 emulation's and the bound:
  (a, b) deviation / (8 x emulation)                   worst error / tolerance 0.037 (error 8.53e-07, tolerance 2.32e-05)
  apply+pool avg per-element                           worst error / tolerance 0.425 (error 0.425, tolerance 1)
  apply+pool in-place per-element                      worst error / tolerance 0.805 (error 0.805, tolerance 1)
  apply+pool max, pairs off                            worst error / tolerance 0.000 (error 0, tolerance 0.5)
  norm apply per-element                               worst error / tolerance 0.808 (error 0.808, tolerance 1)
  norm apply rel-L2 vs float64 instance norm           worst error / tolerance 0.115 (error 2.3e-07, tolerance 2e-06)
  upsample pending rel-L2                              worst error / tolerance 0.087 (error 8.71e-08, tolerance 1e-06)
  zx conv max-rel vs restated arithmetic               worst error / tolerance 0.053 (error 5.29e-07, tolerance 1e-05)
  zx conv rel-L2 vs float64 of unrounded operands      worst error / tolerance 0.299 (error 1.19e-05, tolerance 4e-05)
  zx conv rel-L2 vs restated arithmetic                worst error / tolerance 0.108 (error 2.15e-07, tolerance 2e-06)
  zx statistics slots                                  worst error / tolerance 0.018 (error 0.0175, tolerance 1)
  (a, b) chain 2x10x8x32 affine               device 2.15e-07  fp32 emulation 1.1e-06  bound 8.77e-06
  (a, b) chain 2x10x8x32 plain                device 2.48e-07  fp32 emulation 1.15e-06  bound 9.2e-06
  (a, b) chain 3x8x6x64 affine                device 3.24e-07  fp32 emulation 1.87e-06  bound 1.49e-05
  (a, b) chain 3x8x6x64 plain                 device 3.65e-07  fp32 emulation 2.01e-06  bound 1.61e-05
  finalize alone, 24 cases: the worst device deviation / bound is that of
  (a, b) finalize 513 slots c32 plain         device 8.53e-07  fp32 emulation 2.9e-06  bound 2.32e-05
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mx_fused_ref as M
import anatomix_amd
from _util import check_copies, from_ndhwc_mx, rel_l2, to_ndhwc_mx
from anatomix_amd import _lib
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu

P = _lib.PRECISION["f16x2mx"]
SLOPE = 0.3
REACHED = set()          # kernel / launch names the probe tests reached, for test_routes_of_the_plain_forwards
AB_FIGURES = {}          # case -> (device deviation, emulation deviation)

# (N, D, H, W) of the zx cases and why each is there
ZX_SHAPES = [
    (1, 4, 4, 16),       # 4x16, one tile: every halo voxel is a reflection; D + 2 = 6 = R planes, the ring does not wrap
    (1, 4, 2, 32),       # 2x32, the smallest shape of the other tile
    (2, 10, 8, 32),      # 4x16, grid 8: the (nb & 7) == 0 block remap; 5 steps (odd), the ring wraps twice
    (1, 6, 12, 48),      # 4x16, 3 x 3 tiles, grid 9 (no remap), one interior tile without a reflected voxel
    (2, 6, 2, 128),      # 2x32, grid 8: the remap on the wide tile
    (3, 8, 6, 64),       # 2x32, nby = 3, nbx = 2, three samples
    (2, 16, 6, 32),      # 2x32, a long march
]
ZX_TILES = [(4, 16), (2, 32), (4, 16), (4, 16), (2, 32), (2, 32), (2, 32)]
PLANAR_SHAPES = [(1, 4, 2, 32), (2, 10, 8, 32), (3, 8, 6, 64)]
MODES = ["raw", "relu", "lrelu"]      # no in_ab | in_ab + ReLU | in_ab + leaky ReLU with a < 0 and a = 0
sid = lambda s: "x".join(map(str, s))


def _seed(shape, salt=0):
    return (hash(tuple(shape)) + salt) & 0xFFFF


@functools.lru_cache(maxsize=None)
def zx_inputs(shape, mode, offset=0.0):
    """Stored input, weights, scale, bias, (a, b), activation of a zx case; per-channel magnitudes spread by exp(randn) as in
    test_conv_mx_matches_its_restated_arithmetic (the e4m3 subnormal range is exercised), (a, b) different per sample and channel."""
    n, d, h, w = shape
    rs = np.random.RandomState(_seed(shape))
    x = rs.randn(n, 32, d, h, w) * np.exp(rs.randn(1, 32, 1, 1, 1)) + offset * rs.randn(1, 32, 1, 1, 1)
    x = torch.from_numpy(x.astype(np.float32))
    if mode == "raw":
        x = x.clamp_min(-0.2)
    x = M.stored(x)
    wgt = torch.from_numpy((rs.randn(32, 32, 3, 3, 3) / np.sqrt(27.0 * 32)).astype(np.float32))
    scale = torch.from_numpy(rs.uniform(0.5, 1.5, 32).astype(np.float32))
    bias = torch.from_numpy((rs.randn(32) * 0.1).astype(np.float32))
    a = np.exp(0.5 * rs.randn(n, 32))
    if mode == "lrelu":
        a = a * np.where(rs.rand(n, 32) < 0.3, -1.0, 1.0)
        a[:, 5::11] = 0.0
        a[:, 0] = -1.0 - a[:, 0]
    ab = None if mode == "raw" else torch.from_numpy(np.stack((a, 0.5 * rs.randn(n, 32)), -1).astype(np.float32))
    act = {"raw": M.ACT_NONE, "relu": M.ACT_RELU, "lrelu": M.ACT_LRELU}[mode]
    return x, wgt, scale, bias, ab, act


@functools.lru_cache(maxsize=None)
def zx_case_refs(shape, mode, with_scale=True):
    x, wgt, scale, bias, ab, act = zx_inputs(shape, mode)
    return M.zx_refs(x, wgt, scale if with_scale else None, bias, ab, act, SLOPE)


def dev_f32(t, device):
    return None if t is None else t.float().contiguous().to(device)


def run_zx(device, x, wgt, scale, bias, ab, act, planar=False, stats=True, out_act=0, raw_in=None, d_ab=None):
    """amx_conv3d_zx_probe -> dict(code, kernel, out | out32, stats, flag); x: stored values NCDHW (raw_in: its row-planar bytes)."""
    lib = _lib.load()
    n, _, d, h, w = x.shape
    dx = (raw_in if raw_in is not None else to_ndhwc_mx(x)).to(device)
    dw, dsc, dbi = dev_f32(wgt.reshape(32, 32, 27), device), dev_f32(scale, device), dev_f32(bias, device)
    dab = d_ab if d_ab is not None else dev_f32(ab, device)
    ws = torch.empty(lib.amx_conv3d_zx_probe_workspace_bytes(), dtype=torch.uint8, device=device)
    slots = max(lib.amx_conv3d_zx_probe_stats_slots(h, w), 1)
    o16 = o32 = dst = None
    if planar:
        o32 = torch.full((n, 32, d, h, w), float("nan"), dtype=torch.float32, device=device)
    else:
        o16 = M.poisoned_raw(n, d, h, w, 32).to(device)
    if stats:
        dst = torch.full((n, slots, 32, 2), float("nan"), dtype=torch.float32, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    name = ctypes.create_string_buffer(64)
    code = lib.amx_conv3d_zx_probe(_lib.ptr(dx), _lib.ptr(dw), _lib.ptr(dsc), _lib.ptr(dbi), _lib.ptr(dab), act, SLOPE, n, d, h, w, out_act, _lib.ptr(ws),
                                   ws.numel(), _lib.ptr(o16), _lib.ptr(o32), _lib.ptr(dst), _lib.ptr(flag), ctypes.cast(name, ctypes.c_void_p),
                                   _lib.stream(device))
    torch.cuda.synchronize(device)
    res = dict(code=code, kernel=name.value.decode(), flag=int(flag.item()), stats=None if dst is None else dst.cpu())
    if planar:
        res["out32"] = o32.cpu()
    else:
        res["out"] = o16.cpu()
    if code == 0:
        REACHED.add(res["kernel"])
    return res


# ------------------------------------------------------------------------------------------------ the zx conv
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,tile", list(zip(ZX_SHAPES, ZX_TILES)), ids=[sid(s) for s in ZX_SHAPES])
def test_zx_layer_matches_its_restated_arithmetic(device, shape, tile, mode):
    """16-bit output + statistics: kernel name, both references, the stored pair, the untouched copy section, every slot, the range
    flag; a second run gives the same bytes and the same slots."""
    x, wgt, scale, bias, ab, act = zx_inputs(shape, mode)
    assert M.zx_tile(*shape[2:]) == tile
    res = run_zx(device, x, wgt, scale, bias, ab, act)
    _lib.check(res["code"])
    assert "%dx%d," % tile in res["kernel"] and (",norm-in" in res["kernel"]) == (ab is not None) and ",o1" not in res["kernel"]
    M.check_zx(res, x, wgt, scale, bias, ab, act, SLOPE, False, refs=zx_case_refs(shape, mode))
    again = run_zx(device, x, wgt, scale, bias, ab, act)
    assert torch.equal(res["out"], again["out"]) and torch.equal(res["stats"], again["stats"]), res["kernel"] + ": two runs differ"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=sid)
def test_zx_layer_with_the_fp32_planar_output(device, shape, mode):
    """The network's output conv: fp32 NCDHW, no statistics, no activation, no map."""
    x, wgt, _, bias, ab, act = zx_inputs(shape, mode)
    res = run_zx(device, x, wgt, None, bias, ab, act, planar=True, stats=False)
    _lib.check(res["code"])
    assert res["kernel"].endswith(",o1>")
    M.check_zx(res, x, wgt, None, bias, ab, act, SLOPE, True, refs=zx_case_refs(shape, mode, False))
    again = run_zx(device, x, wgt, None, bias, ab, act, planar=True, stats=False)
    assert torch.equal(res["out32"], again["out32"])


@pytest.mark.parametrize("shape", [(2, 10, 8, 32), (2, 6, 2, 128)], ids=sid)
def test_zx_identity_pairs_give_the_bytes_of_no_pending_norm(device, shape):
    """in_ab = (1, 0) without an activation against in_ab = null: the converter runs the same x * a + b either way (a = 1, b = 0 are
    its defaults), and the stored pair sums exactly in fp32."""
    x, wgt, scale, bias, _, _ = zx_inputs(shape, "raw")
    one = torch.stack((torch.ones(shape[0], 32), torch.zeros(shape[0], 32)), -1)
    plain = run_zx(device, x, wgt, scale, bias, None, M.ACT_NONE)
    ident = run_zx(device, x, wgt, scale, bias, one, M.ACT_NONE)
    _lib.check(plain["code"]), _lib.check(ident["code"])
    assert ",norm-in" in ident["kernel"] and ",norm-in" not in plain["kernel"]
    assert torch.equal(plain["out"], ident["out"]) and torch.equal(plain["stats"], ident["stats"]) and plain["flag"] == ident["flag"] == 0


def test_zx_samples_are_independent(device):
    shape = (3, 8, 6, 64)
    x, wgt, scale, bias, ab, act = zx_inputs(shape, "lrelu")
    full = run_zx(device, x, wgt, scale, bias, ab, act)
    _lib.check(full["code"])
    for k in range(3):
        one = run_zx(device, x[k:k + 1], wgt, scale, bias, ab[k:k + 1], act)
        _lib.check(one["code"])
        assert torch.equal(one["out"][0], full["out"][k]) and torch.equal(one["stats"][0], full["stats"][k]), k


@pytest.mark.parametrize("planar", [False, True])
def test_zx_range_flag_is_raised_by_an_output_beyond_f16(device, planar):
    shape = (1, 4, 2, 32)
    x, wgt, _, bias, ab, act = zx_inputs(shape, "relu")
    res = run_zx(device, x, wgt, torch.full((32,), 1.0e6), bias, ab, act, planar=planar, stats=not planar)
    _lib.check(res["code"])
    # (the fp32 planar epilogue stores no f16 and raises nothing: amx_conv3d_zx.hip, `if (!p.out32) raise_flag`)
    assert res["flag"] == (0 if planar else 1), res
    big = torch.stack((torch.full((1, 32), 1.0e6), torch.zeros(1, 32)), -1)
    res = run_zx(device, x, wgt, None, bias, big, M.ACT_NONE, planar=planar, stats=not planar)      # the operand the converters normalise to
    assert res["code"] == 0 and res["flag"] == 1, res


@pytest.mark.parametrize("shape,planar,stats,out_act,code", [
    ((1, 5, 4, 16), False, True, 0, _lib.AMX_ERR_SHAPE),       # odd D
    ((1, 2, 4, 16), False, True, 0, _lib.AMX_ERR_SHAPE),       # D = 2
    ((1, 4, 6, 16), False, True, 0, _lib.AMX_ERR_SHAPE),       # H = 6 with W = 16: neither tile fits
    ((1, 4, 4, 24), False, True, 0, _lib.AMX_ERR_SHAPE),       # W = 24
    ((1, 4, 2, 32), True, True, 0, _lib.AMX_ERR_INVALID),      # a planar output with statistics
    ((1, 4, 2, 32), True, False, 1, _lib.AMX_ERR_INVALID),     # a planar output with an activation
], ids=["odd_d", "d2", "h6_w16", "w24", "planar_stats", "planar_act"])
def test_zx_probe_refuses_what_the_kernel_does_not_take(device, shape, planar, stats, out_act, code):
    n, d, h, w = shape
    rs = np.random.RandomState(1)
    x = M.stored(torch.from_numpy(rs.randn(n, 32, d, h, w).astype(np.float32)))
    wgt = torch.from_numpy((rs.randn(32, 32, 3, 3, 3) / 30.0).astype(np.float32))
    res = run_zx(device, x, wgt, None, None, None, 0, planar=planar, stats=stats, out_act=out_act)
    assert res["code"] == code and res["kernel"] == "", res
    # nothing was launched: outputs and slots keep what the caller put there
    if planar:
        assert torch.isnan(res["out32"]).all()
    else:
        assert (res["out"] == M.POISON).all()
    assert res["stats"] is None or torch.isnan(res["stats"]).all()
    assert not M.zx_eligible(d, h, w) or planar


# ------------------------------------------------------------------------------------------------ instance norm
def run_norm(device, raw, n, vox, c, w, act, gamma=None, beta=None, eps=1e-2, part=None, kshift=None, skip_lo=0, apply=1):
    """amx_instance_norm_probe -> (code, raw after the call (CPU) or None, ab [n, c, 2] (CPU), flag)."""
    lib = _lib.load()
    slots = 0 if part is None else part.shape[1]
    need = lib.amx_instance_norm_probe_scratch_bytes(n, c, slots)
    scratch = torch.full((need // 4,), float("nan"), dtype=torch.float32, device=device)
    if part is not None:
        scratch[:part.numel()] = part.float().reshape(-1).to(device)
    dx = None if raw is None else raw.to(device)
    ab = torch.full((n, c, 2), float("nan"), dtype=torch.float32, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    dg, db, dk = dev_f32(gamma, device), dev_f32(beta, device), dev_f32(kshift, device)      # (held: a temporary's memory is reused at once)
    code = lib.amx_instance_norm_probe(_lib.ptr(dx), _lib.ptr(dg), _lib.ptr(db), eps, n, vox, c, w, act, SLOPE, _lib.ptr(scratch), need, P, slots,
                                       _lib.ptr(dk), skip_lo, apply, _lib.ptr(ab), _lib.ptr(flag), _lib.stream(device))
    torch.cuda.synchronize(device)
    return code, (None if dx is None else dx.cpu()), ab.cpu(), int(flag.item()), ab


def assert_ab(case, ab, part, kshift, vox, eps, gamma, beta, part32=None):
    """Device pairs against float64, within 8 x the deviation of the all-fp32 emulation on the same sums."""
    ref, bscale = M.finalize_f64(part, kshift, vox, eps, gamma, beta)
    emu = M.ab_deviation(M.finalize_f32(part if part32 is None else part32, kshift, vox, eps, gamma, beta), ref, bscale)
    dev = M.ab_deviation(ab, ref, bscale)
    AB_FIGURES[case] = (dev, emu)
    M.note("(a, b) deviation / (8 x emulation)", dev, 8 * emu)
    assert dev <= 8 * emu, "%s: (a, b) deviate by %.3g from float64, the fp32 emulation by %.3g (bound 8 x)" % (case, dev, emu)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", [(2, 10, 8, 32), (3, 8, 6, 64)], ids=sid)
def test_chain_conv_statistics_finalize_pending_conv(device, shape, affine):
    """zx with statistics -> finalize from its slots (apply = 0, shift = the conv bias) -> zx with that pending norm.  Channel means lie
    up to five standard deviations from the bias, so the shifted sums carry a real offset."""
    n, d, h, w = shape
    x, wgt, scale, bias, _, _ = zx_inputs(shape, "relu", 5.0)
    first = run_zx(device, x, wgt, scale, bias, None, M.ACT_NONE)
    _lib.check(first["code"])
    raw1 = M.check_zx(first, x, wgt, scale, bias, None, M.ACT_NONE, SLOPE, False)
    rs = np.random.RandomState(_seed(shape, 7))
    gamma = torch.from_numpy(rs.uniform(0.5, 1.5, 32).astype(np.float32)) if affine else None
    beta = torch.from_numpy((0.3 * rs.randn(32)).astype(np.float32)) if affine else None
    code, _, ab, flag, d_ab = run_norm(device, first["out"], n, d * h * w, 32, w, M.ACT_RELU, gamma, beta, 1e-2, part=first["stats"], kshift=bias, apply=0)
    _lib.check(code)
    REACHED.add(M.NAME_STATS_ONLY % "conv")
    off = ((raw1.mean((2, 3, 4)) - bias[None]).abs() / raw1.std((2, 3, 4))).max().item()
    assert off > 1.0, off                                        # the offset the case is about is there
    # float64 statistics of the STORED raw tensor (sums about the bias, which float64 carries without loss); emulation: fp32 slots
    assert_ab("chain %s %s" % (sid(shape), "affine" if affine else "plain"), ab, M.slot_sums(raw1, bias)[0], bias, d * h * w, 1e-2, gamma, beta,
              part32=M.slot_sums(raw1, bias, torch.float32)[0])
    assert flag == 0
    w2 = wgt.flip(0).contiguous()
    last = run_zx(device, raw1, w2, None, bias, None, M.ACT_RELU, raw_in=first["out"], d_ab=d_ab)
    _lib.check(last["code"])
    M.check_zx(last, raw1, w2, None, bias, ab, M.ACT_RELU, SLOPE, False)


@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("slots", [1, 31, 33, 512, 513, 1000])
def test_finalize_alone_on_synthetic_partial_sums(device, slots, c):
    """Only the summation differs from the float64 sum of the same floats; 513 and 1000 slots take in_prereduce_kernel."""
    n, per = 2, 8
    rs = np.random.RandomState(slots * 3 + c)
    v = rs.randn(n, slots, c, per) * np.exp(0.5 * rs.randn(1, 1, c, 1)) + 2.0 * rs.randn(1, 1, c, 1)
    v = torch.from_numpy(v.astype(np.float32))
    part = torch.stack((v.sum(-1), (v * v).sum(-1)), -1)                    # [n, slots, c, 2] fp32
    kshift = torch.from_numpy((0.2 * rs.randn(c)).astype(np.float32))
    gamma = torch.from_numpy(rs.uniform(0.5, 1.5, c).astype(np.float32))
    beta = torch.from_numpy((0.3 * rs.randn(c)).astype(np.float32))
    for g, b in ((None, None), (gamma, beta)):
        code, _, ab, flag, _ = run_norm(device, None, n, slots * per, c, per, M.ACT_NONE, g, b, 1e-2, part=part, kshift=kshift, apply=0)
        _lib.check(code)
        assert_ab("finalize %d slots c%d %s" % (slots, c, "affine" if g is not None else "plain"), ab, part, kshift, slots * per, 1e-2, g, b)


def _norm_input(shape, seed):
    n, c, d, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * (0.1 + 3.0 * torch.rand(1, c, 1, 1, 1, generator=g)) + torch.randn(1, c, 1, 1, 1, generator=g)
    return M.stored(x)


@pytest.mark.parametrize("shape", [(2, 32, 4, 6, 8), (1, 48, 2, 3, 40), (2, 64, 3, 5, 7)], ids=sid)      # c = 48: the generic apply kernel
def test_norm_apply_with_a_real_row_length(device, shape):
    """apply = 1 on rows of W voxels (amx_instance_norm takes a sample as one row): statistics pass, finalize, apply."""
    n, c, d, h, w = shape
    x = _norm_input(shape, 11)
    raw = M.raw_of(x, copies=False)                                          # a raw conv output carries no copies
    code, out, ab, flag, _ = run_norm(device, raw, n, d * h * w, c, w, M.ACT_RELU, apply=1)
    _lib.check(code)
    REACHED.add(M.NAME_APPLY)
    got = check_copies(out, c, M.NAME_APPLY)
    ref = F.relu(F.instance_norm(x.double(), eps=1e-2)).float()
    e = rel_l2(got, ref)
    M.note("norm apply rel-L2 vs float64 instance norm", e, 2e-6)
    assert e < 2e-6 and flag == 0, e
    M.check_apply(out, x, ab, M.ACT_RELU, SLOPE, M.NAME_APPLY)               # per element, with the pairs the launch itself used
    # skip_lo = 1: store8 leaves the lo store out, so the lo planes keep the input's lo; hi and the copies are those of skip_lo = 0
    code, out1, ab1, _, _ = run_norm(device, raw, n, d * h * w, c, w, M.ACT_RELU, apply=1, skip_lo=1)
    _lib.check(code)
    k = c // 16
    assert torch.equal(ab1, ab)
    assert torch.equal(out1[:, :, :, :k], out[:, :, :, :k]) and torch.equal(out1[:, :, :, 2 * k:], out[:, :, :, 2 * k:])
    assert torch.equal(out1[:, :, :, k:2 * k], raw[:, :, :, k:2 * k])


# ------------------------------------------------------------------------------------------------ apply + pool
POOL_SHAPES = [(1, 2, 2, 16, 32), (2, 4, 6, 8, 64), (1, 2, 4, 40, 64)]       # (N, D, H, W, C); w c / 8 = 64 | 64 | 320 = 256 + 64


def _pool_input(shape, act):
    n, d, h, w, c = shape
    rs = np.random.RandomState(_seed(shape, act))
    x = M.stored(torch.from_numpy((rs.randn(n, c, d, h, w) * np.exp(0.7 * rs.randn(1, c, 1, 1, 1))).astype(np.float32)))
    a = rs.randn(n, c) * np.exp(0.5 * rs.randn(n, c))
    a[:, 3::5] = 0.0
    ab = torch.from_numpy(np.stack((a, 0.5 * rs.randn(n, c)), -1).astype(np.float32))
    return x, ab


def run_pool(device, raw, ab, shape, act, avg, skip_lo=0, pool_skip_lo=0):
    lib = _lib.load()
    n, d, h, w, c = shape
    dx = raw.to(device)
    pooled = M.poisoned_raw(n, max(d // 2, 1), max(h // 2, 1), max(w // 2, 1), c).to(device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    dab = dev_f32(ab, device)
    code = lib.amx_instance_norm_apply_pool_probe(_lib.ptr(dx), _lib.ptr(dab), _lib.ptr(pooled), n, d, h, w, c, act, SLOPE, avg, skip_lo,
                                                  pool_skip_lo, P, _lib.ptr(flag), _lib.stream(device))
    torch.cuda.synchronize(device)
    return code, dx.cpu(), pooled.cpu(), int(flag.item())


@pytest.mark.parametrize("act", [M.ACT_RELU, M.ACT_LRELU], ids=["relu", "lrelu"])
@pytest.mark.parametrize("avg", [1, 0], ids=["avg", "max"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=sid)
def test_apply_and_pool_in_one_launch(device, shape, avg, act):
    n, d, h, w, c = shape
    x, ab = _pool_input(shape, act)
    raw = M.raw_of(x, copies=False)
    what = M.NAME_POOL % ("avg" if avg else "max")
    code, inplace, pooled, flag = run_pool(device, raw, ab, shape, act, avg)
    _lib.check(code)
    REACHED.add(what)
    M.check_apply(inplace, x, ab, act, SLOPE, what, kind="apply+pool in-place")
    if avg:
        M.check_avg_pool(pooled, x, ab, act, SLOPE, what)
    else:
        M.check_max_pool(pooled, inplace, c, what)
    assert flag == 0
    k = c // 16
    for sl, psl in ((1, 0), (0, 1), (1, 1)):
        code, ip, pl, flag = run_pool(device, raw, ab, shape, act, avg, sl, psl)
        _lib.check(code)
        assert flag == 0
        for got, full, skipped, untouched in ((ip, inplace, sl, raw), (pl, pooled, psl, None)):
            assert torch.equal(got[:, :, :, :k], full[:, :, :, :k]) and torch.equal(got[:, :, :, 2 * k:], full[:, :, :, 2 * k:]), (what, sl, psl)
            lo = got[:, :, :, k:2 * k]
            if not skipped:
                assert torch.equal(lo, full[:, :, :, k:2 * k]), (what, sl, psl)
            elif untouched is None:
                assert (lo == M.POISON).all(), (what, sl, psl)            # the pooled tensor's lo planes keep the caller's poison
            else:
                assert torch.equal(lo, untouched[:, :, :, k:2 * k]), (what, sl, psl)      # in place: the input's lo


@pytest.mark.parametrize("shape", [(1, 2, 4, 40, 48),      # w c / 8 = 240: no multiple of 64 (the issue's third shape: see the module docstring)
                                   (1, 2, 2, 15, 64),      # odd W
                                   (1, 2, 2, 8, 32)],      # w c / 8 = 32
                         ids=sid)
def test_apply_and_pool_probe_refuses_what_its_launcher_is_not_eligible_for(device, shape):
    n, d, h, w, c = shape
    x, ab = _pool_input(shape, 1)
    raw = M.raw_of(x, copies=False)
    code, inplace, pooled, _ = run_pool(device, raw, ab, shape, M.ACT_RELU, 1)
    assert code == _lib.AMX_ERR_SHAPE and torch.equal(inplace, raw) and (pooled == M.POISON).all()


def test_apply_and_pool_raises_the_range_flag(device):
    shape = POOL_SHAPES[0]
    x, ab = _pool_input(shape, 1)
    ab = ab.clone()
    ab[:, :, 0] = 1.0e6
    code, _, _, flag = run_pool(device, M.raw_of(x, copies=False), ab, shape, M.ACT_RELU, 1)
    assert code == 0 and flag == 1


# ------------------------------------------------------------------------------------------------ upsample with a pending norm
def run_upsample(device, raw, ab, shape, act, skip_lo=0):
    lib = _lib.load()
    n, d, h, w, c = shape
    out = M.poisoned_raw(n, 2 * d, 2 * h, 2 * w, c).to(device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    dab = ab if (ab is None or ab.is_cuda) else dev_f32(ab, device)
    dx = raw.to(device)
    code = lib.amx_upsample2_trilinear_pending(_lib.ptr(dx), _lib.ptr(out), n, d, h, w, c, P, skip_lo, _lib.ptr(dab), act, SLOPE,
                                               _lib.ptr(flag), _lib.stream(device))
    torch.cuda.synchronize(device)
    return code, out.cpu(), int(flag.item())


@pytest.mark.parametrize("act", [M.ACT_RELU, M.ACT_LRELU], ids=["relu", "lrelu"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 32), (2, 3, 5, 7, 64), (1, 2, 2, 40, 48)], ids=sid)
def test_upsample_with_a_pending_norm(device, shape, act):
    n, d, h, w, c = shape
    x, ab = _pool_input(shape, act + 10)                                      # per-sample pairs: a sample mix-up shows
    raw = M.raw_of(x, copies=False)
    code, out, flag = run_upsample(device, raw, ab, shape, act)
    _lib.check(code)
    M.check_upsample(out, x, ab, act, SLOPE, M.NAME_UP)
    assert flag == 0
    k = c // 16
    code, out1, _ = run_upsample(device, raw, ab, shape, act, skip_lo=1)
    _lib.check(code)
    assert torch.equal(out1[:, :, :, :k], out[:, :, :, :k]) and torch.equal(out1[:, :, :, 2 * k:], out[:, :, :, 2 * k:])
    assert (out1[:, :, :, k:2 * k] == M.POISON).all()
    # identity pairs, no activation: the bytes of amx_upsample2_trilinear
    one = torch.stack((torch.ones(n, c), torch.zeros(n, c)), -1)
    code, ident, _ = run_upsample(device, raw, one, shape, M.ACT_NONE)
    _lib.check(code)
    plain = M.poisoned_raw(n, 2 * d, 2 * h, 2 * w, c).to(device)
    dx = raw.to(device)
    _lib.check(_lib.load().amx_upsample2_trilinear(_lib.ptr(dx), _lib.ptr(plain), n, d, h, w, c, P, _lib.stream(device)))
    torch.cuda.synchronize(device)
    assert torch.equal(ident, plain.cpu())
    big = ab.clone()
    big[:, :, 0] = 1.0e6
    code, _, flag = run_upsample(device, raw, big, shape, M.ACT_NONE)
    assert code == 0 and flag == 1


def test_chain_statistics_finalize_pending_upsample(device):
    """The decoder's form: statistics pass + finalize (apply = 0), the pairs handed to the upsample."""
    shape = (2, 3, 4, 8, 32)
    n, d, h, w, c = shape
    x = _norm_input((n, c, d, h, w), 5)
    raw = M.raw_of(x, copies=False)
    code, same, ab, flag, d_ab = run_norm(device, raw, n, d * h * w, c, w, M.ACT_RELU, apply=0)
    _lib.check(code)
    REACHED.add(M.NAME_STATS_ONLY % "upsample")
    assert torch.equal(same, raw)                                             # apply = 0: the tensor stays raw
    code, out, flag = run_upsample(device, raw, d_ab, shape, M.ACT_RELU)
    _lib.check(code)
    M.check_upsample(out, x, ab, M.ACT_RELU, SLOPE, M.NAME_UP)
    ref = F.interpolate(F.relu(F.instance_norm(x.double(), eps=1e-2)), scale_factor=2, mode="trilinear").float()
    assert rel_l2(from_ndhwc_mx(out, c)[0], ref) < 2e-6


# ------------------------------------------------------------------------------------------------ routes of the plain forwards
DEV = R.VARIANTS["anatomix-dev"]
NET_MAX = dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance", interp="trilinear", pooling="Max", norm_eps=1e-2)
NET_AVG = dict(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance_affine", interp="nearest", pooling="Avg", activation="lrelu")
ZX4 = "conv3d_k3_zx<f16x2mx,32->32,2x4x16,m4+x4+cv4,r6%s>"
TO_CONV, TO_UP = M.NAME_STATS_ONLY % "conv", M.NAME_STATS_ONLY % "upsample"
# case -> {module id: name}, the zx convs and the fused norms of a plain profiled forward (every other launch is left out).  Filled
# from an MI355X run; a change of route fails here and has to be stated.
def _routes(pool, to_conv, zx_in, pools, ups, tail):
    t = {m: to_conv for m in (1, 4)}
    t.update({m: zx_in for m in (3, 6)})
    t.update({m: M.NAME_POOL % pool for m in pools})
    t.update({m: TO_UP for m in ups})
    t.update({tail: to_conv, tail + 2: zx_in, tail + 3: to_conv, tail + 5: zx_in[:-1] + ",o1>"})
    return t


_DEV = _routes("avg", TO_CONV, ZX4 % ",norm-in", (7, 14, 21, 28, 35), (42, 49, 56, 63, 70), 74)
ROUTE_TABLE = {
    # stem norm and both level-0 norms pending into the zx convs (4x16 tiles: every H here is a multiple of 4), every encoder norm
    # applied with its pool, every decoder norm pending into its upsample, the output conv on the fp32 planar zx epilogue
    "dev_64x64x64": _DEV,
    "dev_64x96x64": _DEV,
    "max_32x64x64": _routes("max", TO_CONV, ZX4 % ",norm-in", (7, 14), (21, 28), 32),
    "avg_16x36x32": _routes("avg", TO_CONV, ZX4 % ",norm-in", (7, 14), (), 32),      # nearest upsample: the decoder norms are applied in place
}
ROUTE_CASES = [("dev_64x64x64", DEV, 1, (64, 64, 64)), ("dev_64x96x64", DEV, 1, (64, 96, 64)), ("max_32x64x64", NET_MAX, 2, (32, 64, 64)),
               ("avg_16x36x32", NET_AVG, 2, (16, 36, 32))]


def _fused(name):
    return name.startswith("conv3d_k3_zx") or name.startswith("instnorm statistics only") or name.startswith("instnorm+act+pool2")


@pytest.mark.parametrize("case,kw,n,size", ROUTE_CASES, ids=[c[0] for c in ROUTE_CASES])
def test_routes_of_the_plain_forwards(device, case, kw, n, size):
    m = anatomix_amd.Unet(**kw)
    m.load_state_dict(R.synthetic_state_dict(kw, 3), strict=True)
    m.precision = "f16x2mx"
    m = m.to(device).eval()
    x = R.synthetic_input(7, n, size).to(device)
    with torch.no_grad():
        yp, recs = m.profile_forward(x)
        y = m(x)
    assert torch.equal(y, yp), case                                           # the profiled route is the production one
    got = {r["module_idx"]: r["kernel"] for r in recs if _fused(r["kernel"])}
    if os.environ.get("AMX_FUSED_REPORT"):
        with open(os.environ["AMX_FUSED_REPORT"], "a") as f:
            f.write("route %s: %r\n" % (case, got))
    assert got == ROUTE_TABLE.get(case), (case, got)
    missing = sorted(set(got.values()) - REACHED)
    assert not missing, "%s launches what no probe test of this module reached (run the module as a whole): %s" % (case, missing)


def test_zz_report_figures():
    """Not a check of the device: appends the worst error / tolerance per launch kind to AMX_FUSED_REPORT when that is set."""
    path = os.environ.get("AMX_FUSED_REPORT")
    if path:
        with open(path, "a") as f:
            for kind, (r, e, t) in sorted(M.WORST.items()):
                f.write("%-52s worst error / tolerance %.3f (error %.3g, tolerance %.3g)\n" % (kind, r, e, t))
            for case, (dev, emu) in sorted(AB_FIGURES.items()):
                f.write("(a, b) %-36s device %.3g  fp32 emulation %.3g  bound %.3g\n" % (case, dev, emu, 8 * emu))
