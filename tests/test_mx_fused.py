"""Host proof of tests/_mx_fused_ref.py, the references and comparisons of tests/test_mx_fused_gpu.py (the fused launches of the
f16x2mx schedule): the slot map covers every voxel once, the references reduce to plain float64 torch operators when nothing is
pending, the emulated launches pass every comparison, and each planted defect makes the comparison the GPU test uses fail with the
name of the launch it was planted in."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _mx_fused_ref as M
from _util import from_ndhwc_mx, ref_conv_mx, rel_l2
from anatomix_amd import _lib

NEW_SYMBOLS = ("amx_conv3d_zx_probe", "amx_conv3d_zx_probe_workspace_bytes", "amx_conv3d_zx_probe_stats_slots", "amx_instance_norm_probe",
               "amx_instance_norm_probe_scratch_bytes", "amx_instance_norm_apply_pool_probe", "amx_upsample2_trilinear_pending")
SLOPE = 0.3


def test_probe_entries_are_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "anatomix_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr), name
    assert len(_lib.SYMBOLS["amx_conv3d_zx_probe"][1]) == 20 and len(_lib.SYMBOLS["amx_instance_norm_probe"][1]) == 20
    assert len(_lib.SYMBOLS["amx_conv3d_k3_reflect_probe"][1]) == 23          # keeps its signature


@pytest.mark.parametrize("hw,tile", [((4, 16), (4, 16)), ((2, 32), (2, 32)), ((8, 32), (4, 16)), ((12, 48), (4, 16)), ((2, 128), (2, 32)),
                                     ((6, 64), (2, 32)), ((6, 32), (2, 32)), ((36, 32), (4, 16)), ((16, 32), (4, 16))])
def test_slot_map_covers_every_voxel_once(hw, tile):
    h, w = hw
    assert M.zx_tile(h, w) == tile
    sm = M.slot_map(h, w)
    counts = torch.bincount(sm.reshape(-1), minlength=h * w // 32)
    assert counts.numel() == h * w // 32 and (counts == 32).all()              # h w / 32 slots of 2 x 16 voxels: a partition
    ty, tx = tile
    for s in range(h * w // 32):
        ys, xs = (sm == s).nonzero(as_tuple=True)
        assert ys.max() - ys.min() == 1 and xs.max() - xs.min() == 15          # two rows, sixteen columns
        by, bx, half = s // 2 // (w // tx), s // 2 % (w // tx), s % 2
        assert ys.min() == by * ty + (2 * half if tx == 16 else 0) and xs.min() == bx * tx + (0 if tx == 16 else 16 * half)
    # the sums of a tensor of ones: 32 D per slot and channel
    one = torch.ones(1, 32, 6, h, w)
    s, a = M.slot_sums(one, None)
    assert (s == 32 * 6).all() and (a == 32 * 6).all()


def _inputs(shape, seed, c=32, offset=False):
    n, d, h, w = shape
    rs = np.random.RandomState(seed)
    x = rs.randn(n, c, d, h, w) * np.exp(rs.randn(1, c, 1, 1, 1))
    if offset:
        x = x + 3.0 * rs.randn(1, c, 1, 1, 1)
    x = M.stored(torch.from_numpy(x.astype(np.float32)))
    wgt = torch.from_numpy((rs.randn(32, 32, 3, 3, 3) / np.sqrt(27.0 * 32)).astype(np.float32))
    scale = torch.from_numpy(rs.uniform(0.5, 1.5, 32).astype(np.float32))
    bias = torch.from_numpy((rs.randn(32) * 0.1).astype(np.float32))
    a = rs.randn(n, c) * np.exp(0.5 * rs.randn(n, c))
    a[:, 1::7] = 0.0
    a[:, 0] = -np.abs(a[:, 0]) - 0.1
    ab = torch.from_numpy(np.stack((a, rs.randn(n, c)), -1).astype(np.float32))
    return x, wgt, scale, bias, ab


def _identity(n, c=32):
    return torch.stack((torch.ones(n, c), torch.zeros(n, c)), -1)


def test_references_reduce_to_plain_float64_operators_when_nothing_is_pending():
    x, wgt, scale, bias, _ = _inputs((2, 4, 4, 16), 1)
    one = _identity(2)
    assert torch.equal(M.pending_f32(x, one, M.ACT_NONE, SLOPE), x) and torch.equal(M.pending_f32(x, None, 0, SLOPE), x)
    assert torch.equal(M.pending_f64(x, one, M.ACT_NONE, SLOPE), x.double())
    assert torch.equal(M.pending_f64(x, one, M.ACT_RELU, SLOPE), F.relu(x.double()))
    assert torch.allclose(M.pending_f64(x, one, M.ACT_LRELU, SLOPE), F.leaky_relu(x.double(), SLOPE), rtol=1e-7, atol=0)
    # zx: the restated arithmetic of a stored pair, and a plain float64 convolution within the operands' 2^-14
    ref, full = M.zx_refs(x, wgt, scale, bias, one, M.ACT_NONE, SLOPE)
    assert torch.equal(ref, M.zx_refs(x, wgt, scale, bias, None, 0, SLOPE)[0])
    assert rel_l2(ref, ref_conv_mx(x, None, wgt, scale, bias, 0)) < 1e-6       # direct lo copy against the stored one: e4m3 roundings of 2^-11
    plain = F.conv3d(F.pad(x.double(), (1,) * 6, mode="reflect"), (wgt * scale[:, None, None, None, None]).double()) + bias.double()[None, :, None, None, None]
    assert rel_l2(full, plain) < 2e-7 and rel_l2(ref, plain) < 4e-5           # (full is returned as fp32; its gain is applied in float64)
    # statistics -> (a, b): F.instance_norm in float64
    s, _ = M.slot_sums(x, bias)
    ab64, _ = M.finalize_f64(s, bias, 4 * 4 * 16, 1e-5)
    want = F.instance_norm(x.double(), eps=1e-5)
    assert torch.allclose(M.pending_f64(x, ab64, M.ACT_NONE, SLOPE), want, rtol=1e-9, atol=1e-9)
    dev = M.ab_deviation(M.finalize_f32(s.float(), bias, 4 * 4 * 16, 1e-5), ab64, M.finalize_f64(s, bias, 4 * 4 * 16, 1e-5)[1])
    assert 0 < dev < 1e-4
    # pool and upsample
    v8 = M.pool_windows(x)
    assert torch.equal(v8.max(0).values, F.max_pool3d(x, 2)) and torch.allclose(v8.double().mean(0), F.avg_pool3d(x.double(), 2), rtol=1e-12)
    assert torch.equal(M.upsample_ref(x), F.interpolate(x.double(), scale_factor=2, mode="trilinear"))


@pytest.mark.parametrize("shape", [(2, 4, 4, 16), (2, 4, 2, 32)])
@pytest.mark.parametrize("act", [M.ACT_RELU, M.ACT_LRELU])
def test_emulated_launches_pass_every_comparison(shape, act):
    x, wgt, scale, bias, ab = _inputs(shape, 2)
    for use in (None, ab):
        M.check_zx(M.emulate_zx(x, wgt, scale, bias, use, act, SLOPE), x, wgt, scale, bias, use, act, SLOPE, False)
    M.check_zx(M.emulate_zx(x, wgt, None, bias, ab, act, SLOPE, planar=True), x, wgt, None, bias, ab, act, SLOPE, True)
    M.check_apply(M.emulate_apply(x, ab, act, SLOPE), x, ab, act, SLOPE, M.NAME_APPLY)
    for avg in (0, 1):
        inplace, pooled = M.emulate_apply_pool(x, ab, act, SLOPE, avg)
        M.check_apply(inplace, x, ab, act, SLOPE, M.NAME_POOL % ("avg" if avg else "max"))
        if avg:
            M.check_avg_pool(pooled, x, ab, act, SLOPE, M.NAME_POOL % "avg")
        else:
            M.check_max_pool(pooled, inplace, 32, M.NAME_POOL % "max")
    M.check_upsample(M.emulate_upsample(x, ab, act, SLOPE), x, ab, act, SLOPE, M.NAME_UP)


# defect -> (the launch whose comparison has to fail, a phrase of its message)
def _planted(defect, shape, act):
    x, wgt, scale, bias, ab = _inputs(shape, 3)
    h, w = shape[2:]
    if defect == "halo_clamp":
        return M.zx_name(h, w, True, False), "restated arithmetic", lambda: M.check_zx(
            M.emulate_zx(x, wgt, scale, bias, ab, act, SLOPE, defect=defect), x, wgt, scale, bias, ab, act, SLOPE, False)
    if defect == "half_swap":
        return M.zx_name(h, w, False, False), "statistics slot", lambda: M.check_zx(
            M.emulate_zx(x, wgt, scale, bias, None, act, SLOPE, defect=defect), x, wgt, scale, bias, None, act, SLOPE, False)
    if defect == "sample_ab":
        return M.zx_name(h, w, True, True), "restated arithmetic", lambda: M.check_zx(
            M.emulate_zx(x, wgt, scale, bias, ab, act, SLOPE, planar=True, defect=defect), x, wgt, scale, bias, ab, act, SLOPE, True)
    if defect == "max_before_affine":
        def run():
            inplace, pooled = M.emulate_apply_pool(x, ab, act, SLOPE, 0, defect=defect)
            M.check_apply(inplace, x, ab, act, SLOPE, M.NAME_POOL % "max")
            M.check_max_pool(pooled, inplace, 32, M.NAME_POOL % "max")
        return M.NAME_POOL % "max", "max-pooled pair", run
    if defect == "pool_lane":
        def run():
            inplace, pooled = M.emulate_apply_pool(x, ab, act, SLOPE, 1, defect=defect)
            M.check_apply(inplace, x, ab, act, SLOPE, M.NAME_POOL % "avg")
            M.check_avg_pool(pooled, x, ab, act, SLOPE, M.NAME_POOL % "avg")
        return M.NAME_POOL % "avg", "average at", run
    if defect == "border_act":
        return M.NAME_UP, "trilinear", lambda: M.check_upsample(M.emulate_upsample(x, ab, act, SLOPE, defect=defect), x, ab, act, SLOPE, M.NAME_UP)
    if defect == "lo_copy_raw":
        return M.NAME_APPLY, "copy bytes differ", lambda: M.check_apply(M.emulate_apply(x, ab, act, SLOPE, defect=defect), x, ab, act, SLOPE, M.NAME_APPLY)
    raise KeyError(defect)


@pytest.mark.parametrize("shape", [(2, 4, 4, 16), (2, 4, 2, 32)], ids=["4x16", "2x32"])
@pytest.mark.parametrize("defect", M.DEFECTS)
def test_planted_defect_fails_the_comparison_of_its_launch(defect, shape):
    launch, phrase, run = _planted(defect, shape, M.ACT_LRELU if defect in ("max_before_affine", "border_act") else M.ACT_RELU)
    with pytest.raises(AssertionError) as e:
        run()
    assert str(e.value).startswith(launch + ":") and phrase in str(e.value), str(e.value)


def test_planted_defects_reach_the_other_launches_too():
    """sample_ab in the apply pass, pool_lane under the maximum: the same defects where another comparison has to see them."""
    x, _, _, _, ab = _inputs((2, 4, 4, 16), 4)
    with pytest.raises(AssertionError, match=re.escape(M.NAME_APPLY) + ": in-place value at .n, c, z, y, x. = .1,"):
        M.check_apply(M.emulate_apply(x, ab, M.ACT_RELU, SLOPE, defect="sample_ab"), x, ab, M.ACT_RELU, SLOPE, M.NAME_APPLY)
    inplace, pooled = M.emulate_apply_pool(x, ab, M.ACT_LRELU, SLOPE, 0, defect="pool_lane")
    with pytest.raises(AssertionError, match="max-pooled pair"):
        M.check_max_pool(pooled, inplace, 32, M.NAME_POOL % "max")
    # a conv epilogue that writes into the copy section, and one whose pair is not a split
    res = M.emulate_zx(x, *_inputs((2, 4, 4, 16), 4)[1:4], None, 0, SLOPE)
    res["out"][0, 0, 0, 4, 0, 0] = 0
    with pytest.raises(AssertionError, match="copy section"):
        M.check_pair(res["out"], 32, "zx", True)
    val, _, hi, lo = from_ndhwc_mx(res["out"], 32, parts=True)
    assert (lo.float().abs() <= hi.float().abs() * 2.0 ** -11 + 2.0 ** -25).all() and torch.isfinite(val).all()
