"""GPU: the ViT's patch decoder on sampled rows (``decode_rows``: amx_vit_decode_rows_forward / _backward, csrc/amx_vit_decode_rows.hip)
against float64 CPU autograd through the dense modules + gather.

The bar is relative to the stock route: both are fp32 and differ only in summation order, so per tensor (rows, d_tokens, every
parameter gradient) the rel-L2 error of the HIP route against float64 may be at most 4 times the larger of (the error of the fp32
torch dense route on the same device in the same test, 2^-22).  A wrong bit, slice or missing term gives errors of order 1."""
import copy

import pytest
import torch

import _decode_rows_ref as R
from anatomix_amd import _lib
from anatomix_amd.model.vit3d.architectures import decode_rows

pytestmark = pytest.mark.gpu

_cache = {}


def _hip(dec, on, tokens, coords, drows, grid, skip=()):
    """The rows route on the modules' device: {"rows", "d_tokens", parameter names...}; names in ``skip`` get no gradient (their
    pointer is null in the backward call)."""
    params = R.named_params(dec, on)
    for k, p in params.items():
        p.grad = None
        p.requires_grad_(k not in skip)
    tok = tokens.detach().clone().requires_grad_("d_tokens" not in skip)
    rows = decode_rows(tok, coords, dec, on, grid)
    rows.backward(drows)
    out = {"rows": rows.detach(), "d_tokens": tok.grad}
    out.update({k: p.grad for k, p in params.items()})
    for p in params.values():
        p.requires_grad_(True)
    return out


def _case(name, device):
    """float64 CPU reference, fp32 torch dense route and fp32 rows route of one case, computed once and left unchanged."""
    if name not in _cache:
        dec, on, tokens, coords, drows, grid, _ = R.case_inputs(name)
        ref = R.run_dense(dec, on, tokens, coords, drows, grid)
        dec32 = copy.deepcopy(dec).float().to(device)
        on32 = None if on is None else copy.deepcopy(on).float().to(device)
        t32, c32, d32 = tokens.float().to(device), coords.to(device), drows.float().to(device)
        stock = {k: v.clone() for k, v in R.run_dense(dec32, on32, t32, c32, d32, grid).items()}
        hip = {k: v.clone() for k, v in _hip(dec32, on32, t32, c32, d32, grid).items()}
        torch.cuda.synchronize()
        _cache[name] = dict(ref=ref, stock=stock, hip=hip, mods=(dec32, on32), inputs=(t32, c32, d32, grid))
    return _cache[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_rows_and_every_gradient_against_float64(device, name):
    c = _case(name, device)
    assert c["hip"].keys() == c["ref"].keys()
    ratios = {}
    for k, ref in c["ref"].items():
        e_hip, e_stock = R.rel_l2(c["hip"][k], ref), R.rel_l2(c["stock"][k], ref)
        ratios[k] = (e_hip, e_stock, e_hip / max(e_stock, R.FLOOR))
    print(name, {k: "hip %.2e torch %.2e ratio %.2f" % v for k, v in ratios.items()})
    for k, (e_hip, e_stock, _) in ratios.items():
        assert e_hip <= R.bar(e_stock), (name, k, e_hip, e_stock)


def test_unselected_slices_and_untouched_tokens_are_exact_zeros(device):
    c = _case("f_one_octant", device)
    coords = c["inputs"][1].cpu()
    touched = sorted({int(((z >> 3) * 2 + (y >> 3)) * 2 + (x >> 3)) for z, y, x in coords.tolist()})
    assert len(touched) == 6
    dtok = c["hip"]["d_tokens"]
    for t in range(8):
        assert (dtok[:, t].abs().sum() > 0) == (t in touched), t
        if t not in touched:
            assert torch.equal(dtok[:, t], torch.zeros_like(dtok[:, t]))
    for s in (1, 2, 3):
        dw = c["hip"][f"w{s}"]
        for kz in (0, 1):
            for ky in (0, 1):
                for kx in (0, 1):
                    sl = dw[:, :, kz, ky, kx]
                    if (kz, ky, kx) == (1, 0, 1):
                        assert sl.abs().sum() > 0
                    else:
                        assert torch.equal(sl, torch.zeros_like(sl)), (s, kz, ky, kx)


@pytest.mark.parametrize("name", ["a_one_patch", "e_repeats", "d_odd_affine"])
def test_two_calls_give_the_same_bits(device, name):
    c = _case(name, device)
    again = _hip(*c["mods"], *c["inputs"])
    for k, v in c["hip"].items():
        assert torch.equal(v, again[k]), k


def test_a_null_gradient_leaves_the_others_unchanged(device):
    c = _case("d_odd_affine", device)
    for skip in (("d_tokens",), ("w1", "b2", "g1", "ow"), ("w3", "be2", "ob", "b1", "w2")):
        got = _hip(*c["mods"], *c["inputs"], skip=skip)
        for k, v in c["hip"].items():
            if k in skip:
                assert got[k] is None, k
            else:
                assert torch.equal(v, got[k]), (skip, k)


def test_out_of_envelope_shapes_raise_naming_the_shape(device):
    dec, on = R.build_modules(1064, 16, "none", 1, dtype=torch.float32)
    dec = dec.to(device)
    coords = R.draw_distinct(8, (16, 16, 16), 2).to(device)
    with pytest.raises(_lib.AmxError, match="1064"):
        decode_rows(torch.zeros(1, 8, 1064, device=device), coords, dec, None, (2, 2, 2))
    dec, _ = R.build_modules(264, 72, "none", 1, dtype=torch.float32)
    with pytest.raises(_lib.AmxError, match="72"):
        decode_rows(torch.zeros(1, 8, 264, device=device), coords, dec.to(device), None, (2, 2, 2))
    # the C entry itself: AMX_ERR_SHAPE with the shape in the message
    lib = _lib.load()
    assert lib.amx_vit_decode_rows_scratch_bytes(1, 8, 1064, 336, 104, 16) == 0
    import ctypes
    arr = (ctypes.c_void_p * 12)(*[coords.data_ptr()] * 12)
    rc = lib.amx_vit_decode_rows_forward(_lib.ptr(coords), _lib.ptr(coords), arr, 1, 8, 2, 2, 2, 1064, 336, 104, 16, 1e-6, 0, 0.0, _lib.ptr(coords),
                                         _lib.ptr(coords), 1 << 20, None)
    assert rc == _lib.AMX_ERR_SHAPE and "1064" in lib.amx_last_error().decode()


def test_out_of_range_coordinates_raise_before_any_launch(device):
    c = _case("a_one_patch", device)
    dec, on = c["mods"]
    t32, c32, _, grid = c["inputs"]
    for bad in ([16, 0, 0], [0, -1, 0], [0, 0, 1 << 40]):
        coords = c32.clone()
        coords[3] = torch.tensor(bad, device=device)
        with pytest.raises(ValueError, match="outside the volume"):
            decode_rows(t32, coords, dec, on, grid)
    with pytest.raises(ValueError, match="int64"):
        decode_rows(t32, c32.int(), dec, on, grid)
