"""GPU: the engine forward of the 3D ViT, stage by stage (tests/_vit_walk.py; its self-check on the host is tests/test_vit_walk.py).

Every stage of ``amx_vit_forward`` -- tokenizer stem and stages, token projection, each block's norms, attention group, residual
products and SwiGLU, final norm, decoder stages, ChannelDemean, output -- is compared with a float64 reference of the tensors the GPU
itself stored in front of it (``forward_hip(x, taps=...)``: copies enqueued behind the producing launch, no launch added or moved),
per element, with no share of elements excluded.  The output with taps equals the output without, bit for bit.

Cases (tests/_vit_walk.py ``CASES``): A flagship widths at 32^3 x 2; B ragged shapes and every flag off (T = 67, M = 201, hidden 607,
36 classes, grid 2 x 8 x 4); C PrimusV2-L widths; D the tokenizer alone at 32 x 64^3, the batch that selects the 64-voxel-per-wave
conv kernels (float64 convolutions on samples 0, 17, 31; statistics over all samples).

ROUTE_TABLE pins the kernel instance of every stage per case: a routing change fails here, and whoever makes it picks shapes that reach
the new route.  NOT_WALKED is the ledger of the instances a plain 128^3 forward (batch 1 and 4) runs that no case walks, each with its
reason; test_instances_of_the_128_forward_are_walked_or_listed fails on a missing and on a stale entry.

Worst err / tol per stage kind over the four cases of one run on an MI355X (CPU emulation of cases A and B in brackets;
profiles/vit_walk_gpu.txt has every stage with its route): split 0.052 (0.068), resid 0.013 (0.031), f16 0.4993 (0.4993: half of the
bound is the f16 store itself), hi + lo 0.40 (0.36), statistics 0.22 (0.22), attention group 0.36 (0.38).  No element of any stage of
any case is over its bound.
"""
import ctypes

import pytest
import torch

import _vit_walk as W
from anatomix_amd import _lib
from anatomix_amd.model.vit3d import PrimusV2

pytestmark = pytest.mark.gpu


def _parts(route):
    return [p for p in route.split(" + ") if p]


def _model(name, device):
    kw, sd, x, cs = W.case(name)
    m = PrimusV2(**kw)
    m.load_state_dict(sd, strict=True)
    return m.to(device).eval(), kw, sd, x, cs


def _stages(name, cfg, cs):
    return list(W.D_STAGES) if name == "D" else W.tap_names(cfg, cs["n_blocks"])


_RUNS = {}


def _run(name, device):
    """(records, routes) of a case: one plain forward, one forward with every tap of the case, the walk."""
    if name in _RUNS:
        return _RUNS[name]
    m, kw, sd, x, cs = _model(name, device)
    cfg = W.Cfg(sd, kw, x.shape)
    names = _stages(name, cfg, cs)
    xd = x.to(device)
    with torch.no_grad():
        y0 = m.forward_hip(xd, n_blocks=cs["n_blocks"])
        y, got = m.forward_hip(xd, n_blocks=cs["n_blocks"], taps={n: n != "y" for n in names})
    assert torch.equal(y, y0), "a forward with taps returns the bits of one without"
    taps, routes = W.split_taps(got)
    if "y" in names:
        taps["y"] = y.cpu().reshape(-1)
    del got, m
    recs = W.walk(sd, kw, x, taps, only=names, samples=cs["samples"], routes=routes)
    _RUNS[name] = (recs, routes, names)
    return _RUNS[name]


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_every_stage_matches_float64_of_the_stored_tensors(device, name):
    recs, routes, names = _run(name, device)
    print(f"case {name}\n{W.report(recs)}")
    assert [r.stage for r in recs] == names, "every requested stage was walked"
    bad = [str(r) for r in recs if not r.ok or r.over or not r.ref_absmax > 0.1]
    assert not bad, "\n".join(bad)


# ---- routes.  Stage -> kernel instance, per case, as the launchers report it (VitLaunchInfo, amx_gemm.h).
def _tokenizer(mt, stages=3):
    """Stem and ``stages`` tokenizer stages; ``mt[k]``: row tiles per wave of stage k's convs (2: 32 voxels, 4: 64 voxels per wave --
    ``tokconv_mt`` takes 4 from 131072 output voxels per launch on); 2 column tiles below 64 output channels, 4 from there on."""
    r = {"h0": "tokstem<1,split>", "p0": "tokstem<1,split>"}
    for k in range(stages):
        nt = 2 if k == 0 else 4
        r.update({f"s{k}.raw1": f"tokconv<27,2,{mt[k]},{nt},split>", f"s{k}.ss1": "tok_finalize", f"s{k}.a1": "tok_apply",
                  f"s{k}.raw2": f"tokconv<27,1,{mt[k]},{nt},split>", f"s{k}.ss2": "tok_finalize",
                  f"s{k}.raws": f"tokconv<1,1,{mt[k]},{nt},split>", f"s{k}.sss": "tok_finalize", f"s{k}.h": "tok_combine"})
        if k < 2:
            r[f"s{k}.p"] = "tok_combine"
    return r


def _block(b, ln, qkv, proj, fc1, ln_mlp, fc2):
    return {f"b{b}.ln1": ln, f"b{b}.attn": f"{qkv[0]} + {qkv[1]} + attn_fwd", f"b{b}.ln_attn": ln, f"b{b}.tok1": proj, f"b{b}.ln2": ln,
            f"b{b}.hd": fc1, f"b{b}.ln_mlp": ln_mlp, f"b{b}.tok2": fc2}


_WS_QKV = ("wsgemm<1,5,4,QK,f16,8w>", "wsgemm<1,5,4,VT,f16,8w>")
_A_BLOCK = dict(ln="ln_rows_vec<f32,2>", qkv=_WS_QKV, proj="wsgemm<2,5,4,RESID,f16,4w>", fc1="wsgemm<2,4,4,SWIGLU,f16,4w>",
                ln_mlp="ln_rows_vec<f16,5>", fc2="gemm<2,5,RESID,f16,pf2>")      # fc2: 33 K steps x 5 tiles do not fit LDS -> direct kernel
ROUTE_TABLE = {
    # flagship widths: what a 128^3 forward runs at batch 1 and 4 (the ledger below has nothing left over)
    "A": {**_tokenizer((2, 2, 2)), "tokens": "wsgemm<2,5,2,TOKENS,split,4w>", **_block(0, **_A_BLOCK), **_block(1, **_A_BLOCK),
          "d.ln": "ln_rows_vec<f32,2,split>", "d0.raw": "wsgemm<1,4,2,SCATTER,split,8w>", "d1.in": "ln_rows_vec<f32,1,gelu,split>",
          "d2.in": "wsgemm<1,8,2,SCATTER_LN,split,8w>",                   # cp == 128: LayerNorm + GELU inside the product, no d1.raw
          "d.mean": "colsum + demean", "y": "wsgemm<1,4,2,PLANAR,split,4w>"},
    # hidden 607: the scalar ln_rows (C % 4 != 0) behind the ragged (gate, value) tile pair; fc2's 19 K steps x 5 tiles fit LDS here
    "B": {**_tokenizer((2, 2, 2)), "tokens": "wsgemm<2,5,2,TOKENS,split,4w>",
          **_block(0, **dict(_A_BLOCK, ln_mlp="ln_rows<f16,17>", fc2="wsgemm<2,5,4,RESID,f16,4w>")),
          "d.ln": "ln_rows_vec<f32,2,split>", "d0.raw": "wsgemm<2,5,2,SCATTER,split,4w>", "d1.in": "ln_rows_vec<f32,1,gelu,split>",
          "d1.raw": "wsgemm<2,4,2,SCATTER,split,4w>", "d2.in": "ln_rows_vec<f32,1,gelu,split>", "y": "wsgemm<1,4,2,PLANAR,split,4w>"},
    # PrimusV2-L: a head's 5 tiles x 33 K steps do not fit LDS (q | k and v on the direct kernel), nor do 4 split tiles of decoder stage 0
    "C": {**_tokenizer((2, 2, 2)), "tokens": "wsgemm<2,4,2,TOKENS,split,4w>",
          **_block(0, ln="ln_rows_vec<f32,5>", qkv=("gemm<2,5,QK,f16,pf2>", "gemm<2,5,VT,f16,pf2>"), proj="wsgemm<2,4,4,RESID,f16,4w>",
                   fc1="wsgemm<2,4,4,SWIGLU,f16,4w>", ln_mlp="ln_rows_vec<f16,12>", fc2="gemm<2,4,RESID,f16,pf2>"),
          "d.ln": "ln_rows_vec<f32,5,split>", "d0.raw": "gemm<2,4,SCATTER,split,pf1>", "d1.in": "ln_rows_vec<f32,2,gelu,split>",
          "d1.raw": "wsgemm<2,5,2,SCATTER,split,4w>", "d2.in": "ln_rows_vec<f32,1,gelu,split>", "d.mean": "colsum + demean",
          "y": "wsgemm<1,4,2,PLANAR,split,4w>"},
    # 32 x 32^3 and 32 x 16^3 output voxels: 64 voxels per wave at stages 0 and 1
    "D": _tokenizer((4, 4), stages=2),
}


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_routes_are_the_pinned_ones(device, name):
    _, routes, names = _run(name, device)
    got = {n: routes[n] for n in names}
    print(f'    "{name}": {{\n' + "".join(f'        "{k}": "{v}",\n' for k, v in got.items()) + "    },")
    assert got == ROUTE_TABLE.get(name), "routing changed: pick shapes that reach the new instance, then pin it"


# Instances of the plain 128^3 forward (batch 1 and 4) that no case walks: instance -> reason.  Empty on purpose: cases A and D
# together reach every instance those forwards launch (D exists for the 64-voxel-per-wave tokenizer convs, which only a large batch
# selects).  An instance that a routing change adds to the 128^3 forward fails the test below until a case walks it or it is listed here.
NOT_WALKED = {}


def _instances(device, kw, batch, n_blocks=-1):
    """Instance names of a forward: routes only (no copies, no reference)."""
    from oracle import vit_ref as V
    m = PrimusV2(**kw).to(device).eval()
    cfg = W.Cfg(m.state_dict(), kw, (batch, 1) + tuple(kw["input_shape"]))
    x = torch.rand(batch, 1, *kw["input_shape"], device=device)
    with torch.no_grad():
        _, got = m.forward_hip(x, n_blocks=n_blocks, taps={n: False for n in W.tap_names(cfg, n_blocks)})
    return {p for _, route in got.values() for p in _parts(route)}


def test_instances_of_the_128_forward_are_walked_or_listed(device):
    walked = set()
    for name, cs in W.CASES.items():
        walked |= _instances(device, cs["kw"], cs["batch"], cs["n_blocks"])
    kw128 = dict(W.CASES["A"]["kw"], input_shape=(128, 128, 128), eva_depth=1)
    plain = _instances(device, kw128, 1) | _instances(device, kw128, 4)
    print("128^3 instances:", sorted(plain))
    print("not walked:", sorted(plain - walked))
    missing = sorted(plain - walked - set(NOT_WALKED))
    stale = sorted(k for k in NOT_WALKED if k not in plain or k in walked)
    assert not missing, f"instances of the 128^3 forward neither walked nor listed: {missing}"
    assert not stale, f"NOT_WALKED entries that are walked by now or no longer run: {stale}"


# ---- refusals of the tap entry
def test_tap_entry_refuses_unknown_names_short_buffers_and_an_unloaded_handle(device):
    m, kw, sd, x, cs = _model("B", device)
    lib = _lib.load()
    xd = x.to(device)
    with torch.no_grad():
        y0 = m.forward_hip(xd)
        with pytest.raises(_lib.AmxError) as ei:
            m.forward_hip(xd, taps=["b0.ln1", "b0.nonsense"])
        assert ei.value.code == _lib.AMX_ERR_INVALID and "b0.nonsense" in str(ei.value)
        with pytest.raises(_lib.AmxError) as ei:
            m.forward_hip(xd, n_blocks=0, taps=["b0.ln1"])              # not produced by this forward
        assert ei.value.code == _lib.AMX_ERR_INVALID
    assert lib.amx_vit_tap_bytes(m._handle, 3, b"b0.nonsense") == 0
    need = lib.amx_vit_tap_bytes(m._handle, 3, b"tokens")
    assert need == 3 * 67 * 240 * 4
    with torch.cuda.device(device):
        ws_need = lib.amx_vit_workspace_bytes(m._handle, 3)
        ws = torch.empty(ws_need, dtype=torch.uint8, device=device)
        y = torch.full_like(y0, 7.0)
        buf = torch.zeros(need, dtype=torch.uint8, device=device)
        req = (_lib.VitTap * 1)()
        req[0].name, req[0].d_dst, req[0].bytes = b"tokens", buf.data_ptr(), need - 4
        rc = lib.amx_vit_forward_taps(m._handle, _lib.ptr(xd), _lib.ptr(y), 3, _lib.ptr(ws), ws_need, -1, req, 1, _lib.stream(device))
        assert rc == _lib.AMX_ERR_WORKSPACE and b"tokens" in lib.amx_last_error()
        torch.cuda.synchronize(device)
        assert bool((y == 7.0).all()) and not bool(buf.any()), "refused before the first launch"
        # a handle that was never loaded
        hnd = ctypes.c_void_p()
        _lib.check(lib.amx_vit_create(ctypes.byref(hnd), ctypes.byref(_lib.VitCfg(**m._vit_cfg))))
        try:
            req[0].bytes = need
            rc = lib.amx_vit_forward_taps(hnd, _lib.ptr(xd), _lib.ptr(y), 3, _lib.ptr(ws), ws_need, -1, req, 1, _lib.stream(device))
            assert rc == _lib.AMX_ERR_NOT_LOADED
        finally:
            lib.amx_vit_destroy(hnd)
