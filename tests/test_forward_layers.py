"""The layer walk (tests/_layer_walk.py) checks itself, on the CPU: fed with the taps of an emulated 16-bit forward it passes with
room to spare, and it names the module of every planted defect.  This is the proof that the net the GPU module
(tests/test_forward_layers_gpu.py) casts over the production forward is sharp.

6 M model, gain 1.0, 2 x (32, 32, 48), the routes the production forward takes at that size (upcat16 at level 0, the merged-tap
pair at level 1, the generic kernel below).  Worst err/tol over all layers of the clean emulation, measured when this was written:
f16 0.493, bf16 0.497 (a store rounding costs half an ulp, the bound allows one), 0 voxels over the bound; the output conv at
0.038 / 0.015 of its bound; merged-route share of voxels over the one-rounding bound 5.3e-5 / 5.1e-6 (cap 2e-3).
"""
import pytest
import torch
import torch.nn.functional as F

from _layer_walk import ULP, conv_params, emulate, groups, report, walk
from _util import q_storage, ref_conv, rel_l2
from oracle import unet_ref as R

KW = R.VARIANTS["anatomix"]
N, SIZE = 2, (32, 32, 48)
ROUTES = {59: "conv3d_upcat16<emulated>", 52: "conv3d_k3_v2<emulated> + upmerge<emulated>"}
CHECKED = [g["module"] for g in groups(KW)[0]]          # every conv and every pool


@pytest.fixture(scope="module")
def clean():
    """precision -> (state dict, input, taps of the emulated forward); built once, never modified (the tests copy what they edit)."""
    torch.manual_seed(0)
    sd = R.synthetic_state_dict(KW, 0, gain=1.0)
    x = R.synthetic_input(100, N, SIZE)
    return {p: (sd, x, emulate(KW, sd, x, p, ROUTES)) for p in ("f16", "bf16")}


def _failed(recs):
    return sorted(r.module for r in recs if not r.ok)


@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_walk_passes_on_the_emulated_forward(clean, precision):
    sd, x, taps = clean[precision]
    recs = walk(KW, sd, x, taps, precision, ROUTES)
    print(report(recs))
    assert [r.module for r in recs] == CHECKED
    assert not _failed(recs), report(recs)
    worst = max(r.ratio for r in recs)
    print(f"{precision}: worst err/tol {worst:.3f}, output conv {recs[-1].ratio:.3f}, merged share "
          f"{max(r.emul_share for r in recs):.2e}")
    assert worst < 0.6, report(recs)
    assert sum(r.over for r in recs) == 0
    assert all(r.ref_absmax > 0.1 for r in recs), report(recs)
    assert {r.kind for r in recs} == {"conv", "upcat16", "upmerge", "planar", "pool"}


def test_emulation_without_merged_routes_is_forward_lowp(clean):
    """The per-module collector is forward_lowp's arithmetic.  With every concat conv on the generic route its output is that
    function's up to the fold: forward_lowp folds the BatchNorm in float64, the collector in float32 as the HIP path does, and a
    handful of f16 weights per layer (up to 88) round the other way.  Twenty layers carry that to 4.0e-4 at the output, the size of
    the kernel-to-emulation distance tests/test_unet_gpu.py allows 1e-3 for; the same limit here."""
    sd, x, _ = clean["f16"]
    d = rel_l2(emulate(KW, sd, x, "f16", {})[65], R.forward_lowp(x, sd, KW, torch.float16))
    print(f"collector vs forward_lowp: rel-L2 {d:.2e}")
    assert d < 1e-3


def _walk_with(clean, edits, precision="f16"):
    sd, x, taps = clean[precision]
    return walk(KW, sd, x, {**taps, **edits}, precision, ROUTES)


def test_one_voxel_two_ulp_off_at_the_bottleneck_is_found(clean):
    t = clean["f16"][2][33].clone()
    i = int(t.abs().argmax())
    t.view(-1)[i] *= 1.0 + 2.0 * ULP["f16"]
    recs = _walk_with(clean, {33: t})
    bad = _failed(recs)
    assert 31 in bad and set(bad) <= {31, 34}, report(recs)       # (34 reads the edited tensor; a 2-ulp input error may or may not show)
    r = next(r for r in recs if r.module == 31)
    assert r.over == 1 and r.worst == tuple(int(v) for v in torch.unravel_index(torch.tensor(i), t.shape)), r


def test_last_x_column_taken_from_its_neighbour_is_found(clean):
    t = clean["f16"][2][8].clone()
    t[..., -1] = t[..., -2]
    recs = _walk_with(clean, {8: t})
    bad = _failed(recs)
    assert 6 in bad and set(bad) <= {6, 9, 59}, report(recs)      # its pool and the decoder conv that reads it as skip may follow
    r = next(r for r in recs if r.module == 6)
    assert r.worst[-1] == SIZE[2] - 1, r


def test_pool_plane_taken_from_the_plane_above_is_found(clean):
    t = clean["f16"][2][16].clone()
    t[:, :, 3] = t[:, :, 4]
    recs = _walk_with(clean, {16: t})
    bad = _failed(recs)
    assert 16 in bad and set(bad) <= {16, 17}, report(recs)
    r = next(r for r in recs if r.module == 16)
    assert r.worst[2] == 3 and r.ratio == float("inf"), r


def test_swapped_skip_and_low_inputs_are_found(clean):
    """Module 45 (192 -> 64 at level 2): the stored result is that of cat(up(low), skip), the two segments in the wrong order."""
    sd, x, taps = clean["f16"]
    gs, plan, full = groups(KW)
    g = next(g for g in gs if g["module"] == 45)
    w, s, sh = conv_params(sd, full, g, plan)
    w = w * s[:, None, None, None, None]
    xin = torch.cat((F.interpolate(taps[g["src"]], scale_factor=2, mode="nearest"), taps[g["skip"]]), 1)
    y = q_storage(F.relu(R.conv3_reflect(xin, q_storage(w, "f16"), sh)), "f16")
    recs = _walk_with(clean, {g["out"]: y})
    bad = _failed(recs)
    assert 45 in bad and set(bad) <= {45, 48}, report(recs)
    assert next(r for r in recs if r.module == 45).over > y.numel() // 4


def test_output_conv_and_strict_measures_are_live(clean):
    """The rel-L2 / max-rel measures (output conv, strict) see a defect: one output voxel 1e-4 off fails module 65, and an f16-rounded
    tensor is no strict (bf16x2) result, while the float64 reference's own value is."""
    sd, x, taps = clean["f16"]
    t = taps[65].clone()
    t[1, 3, 5, 7, 47] += 1e-4
    r, = walk(KW, sd, x, {**taps, 65: t}, "f16", ROUTES, only={65})
    assert not r.ok and r.worst == (1, 3, 5, 7, 47), r
    r, = walk(KW, sd, x, taps, "strict", {}, only={3})
    assert r.kind == "strict" and not r.ok and r.rel_l2 > 1e-4, r
    gs, plan, full = groups(KW)
    g = next(g for g in gs if g["module"] == 3)
    w, s, sh = conv_params(sd, full, g, plan)
    r, = walk(KW, sd, x, {**taps, 5: ref_conv(taps[2], None, w, s, sh, 1, "bf16x2")}, "strict", {}, only={3})
    assert r.ok and r.ratio < 0.01, r
