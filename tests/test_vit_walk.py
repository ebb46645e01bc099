"""Host: the ViT stage walk (tests/_vit_walk.py) checked on the CPU before it is trusted on the GPU (tests/test_vit_walk_gpu.py).

  * the stage references, chained without teacher forcing in float64, ARE the oracle (``oracle.vit_ref.forward(dtype=float64)``) to 1e-9;
  * the walk passes on the clean CPU emulation of cases A and B with 0 elements over any bound, every stage's reference is clearly
    nonzero, and the worst err / tol per stage kind stays under a limit with a visible margin.  Measured on this emulation
    (worst err / tol [limit]): split 0.068 [0.15], resid 0.031 [0.08], f16 0.4993 [0.51], hilo 0.36 [0.6], stats 0.22 [0.45],
    attn 0.38 [0.6] -- f16 sits at one half by construction: half of the bound is the storage rounding itself;
  * eleven planted defects, each of the kind a whole-network rel-L2 averages away, fail exactly the stage that produced the tensor
    (at most the stages that read it fail as well);
  * ``only=`` restricts the walk.
"""

import pytest
import torch

import _vit_walk as W
from oracle import vit_ref as V

LIMIT = {"split": 0.15, "resid": 0.08, "f16": 0.51, "hilo": 0.6, "stats": 0.45, "attn": 0.6}


class _Case:
    def __init__(self, name):
        self.kw, self.sd, self.x, self.cs = W.case(name)
        self.cfg = W.Cfg(self.sd, self.kw, self.x.shape)
        self.taps = W.emulate(self.sd, self.kw, self.x)
        self.recs = {r.stage: r for r in W.walk(self.sd, self.kw, self.x, self.taps)}

    def helper(self, taps):
        return W._Walk(self.sd, self.kw, self.x, taps, None, None, None)


_CACHE = {}


@pytest.fixture
def case():
    def get(name):
        if name not in _CACHE:
            _CACHE[name] = _Case(name)
        return _CACHE[name]
    return get


def _oracle_sd(cs):
    """The oracle multiplies by gamma_1 / gamma_2 unconditionally: ones stand for 'no LayerScale'."""
    sd = dict(cs.sd)
    for b in range(cs.kw["eva_depth"]):
        for g in ("gamma_1", "gamma_2"):
            sd.setdefault(f"eva.blocks.{b}.{g}", torch.ones(cs.kw["embed_dim"]))
    return sd


@pytest.mark.parametrize("name", ["A", "B"])
def test_stage_references_compose_to_the_oracle(case, name):
    """Case A, and case B = every flag off (no QK norm, no inner norm, no LayerScale, no output norm)."""
    cs = case(name)
    ref = V.forward(cs.x, _oracle_sd(cs), cs.kw, dtype=torch.float64)
    got = W.chain64(cs.sd, cs.kw, cs.x)
    e = float((got - ref).norm() / ref.norm())
    print(f"case {name}: chained stage references vs oracle rel-L2 {e:.2e}")
    assert got.shape == ref.shape and e < 1e-9, e


@pytest.mark.parametrize("name", ["A", "B"])
def test_walk_passes_on_the_clean_emulation(case, name):
    cs = case(name)
    print(W.report(cs.recs.values()))
    assert list(cs.recs) == W.tap_names(cs.cfg), "every tap is a stage of the walk, in launch order"
    worst = {}
    for r in cs.recs.values():
        assert r.ok and r.over == 0 and r.pad_bad == 0, str(r)
        assert r.ref_absmax > 0.1, f"{r.stage}: a reference of {r.ref_absmax} checks nothing"
        worst[r.kind] = max(worst.get(r.kind, 0.0), r.ratio)
    print({k: round(v, 4) for k, v in worst.items()})
    assert set(worst) == set(LIMIT)
    for kind, v in worst.items():
        assert v < LIMIT[kind], (kind, v)


def test_constants_have_their_margin(case):
    """C_SS, C_MEAN, C_ATT are at least twice what the emulation needs (err / tol <= 0.5 on the stages they bound) and _EMU_WORST
    records what it needs."""
    need = {"C_SS": 0.0, "C_MEAN": 0.0, "C_ATT": 0.0}
    for name in ("A", "B"):
        for r in case(name).recs.values():
            if r.stage.split(".")[-1] in ("ss1", "ss2", "sss"):
                need["C_SS"] = max(need["C_SS"], r.ratio * W.C_SS)
            elif r.stage == "d.mean":
                need["C_MEAN"] = max(need["C_MEAN"], r.ratio * (W.C_MEAN + W.U16 ** 2 / W.U32))      # in U32 (the bound carries U16^2 = 4 U32 too)
            elif r.kind == "attn":
                need["C_ATT"] = max(need["C_ATT"], r.ratio * W.C_ATT)
    print(need)
    for k, v in need.items():
        assert 2 * v <= getattr(W, k), (k, v)
        assert v <= W._EMU_WORST[k] * 1.05 and v >= W._EMU_WORST[k] * 0.5, (k, v, W._EMU_WORST[k])


def test_only_restricts_the_walk(case):
    cs = case("B")
    recs = W.walk(cs.sd, cs.kw, cs.x, cs.taps, only=["tokens", "b0.hd"])
    assert [r.stage for r in recs] == ["tokens", "b0.hd"]
    part = {k: v for k, v in cs.taps.items() if k in ("d.ln", "d0.raw")}
    assert [r.stage for r in W.walk(cs.sd, cs.kw, cs.x, part)] == ["d0.raw"], "a stage needs its result and its inputs"


# ---------------------------------------------------------------------------------------------------------------- planted defects
def _planted(cs, stage, taps):
    """Re-walks ``stage`` and the stages that read it on ``taps`` (every other stage has the inputs and the result of the clean walk:
    its record cannot change); asserts that ``stage`` fails and returns its record."""
    rd = W.readers(stage, cs.cfg)
    recs = {r.stage: r for r in W.walk(cs.sd, cs.kw, cs.x, taps, only=[stage] + rd)}
    assert set(recs) == {stage, *rd}
    assert cs.recs[stage].ok and not recs[stage].ok, str(recs[stage])
    print(W.report(recs.values()))
    return recs[stage]


def _with(cs, name, value):
    taps = dict(cs.taps)
    taps[name] = value
    return taps


def test_defect_a_one_token_element_off_by_four_ulps(case):
    """In a product row 4 fp32 ulps are inside any sound bound of a 128-term fp32 accumulation (the row's own S is worth more);
    the register rows are copies, their bound is equality: that is where 4 ulps show."""
    cs, c = case("A"), case("A").cfg
    tok = cs.taps["tokens"].clone().reshape(c.n, c.T, c.E)
    bits = tok[1, 2].view(torch.int32)
    bits[5] += 4
    r = _planted(cs, "tokens", _with(cs, "tokens", tok.reshape(-1)))
    assert r.over == 1 and r.worst == (1, 2, 5)


def test_defect_b_last_key_left_out_of_one_head(case):
    cs, c = case("A"), case("A").cfg
    q, k, v = cs.helper(cs.taps).qkv64("b0", "eva.blocks.0.", torch.float32)
    h = 3
    part = W._attn32(q[:, h:h + 1], k[:, h:h + 1, :c.T - 1], v[:, h:h + 1, :c.T - 1], c.T - 1)       # [n, 1, T, hd]
    att = cs.taps["b0.attn"].clone().reshape(c.n, c.T, c.heads, c.hd)
    att[:, :, h] = part[:, 0]
    r = _planted(cs, "b0.attn", _with(cs, "b0.attn", att.reshape(-1)))
    assert r.worst[1] // c.hd == h


def test_defect_c_rotary_embedding_on_the_register_rows(case):
    cs, c = case("A"), case("A").cfg
    q, k, v = cs.helper(cs.taps).qkv64("b0", "eva.blocks.0.", torch.float32, rope_prefix=True)
    att = W._attn32(q, k, v, c.T).transpose(1, 2).reshape(-1)
    _planted(cs, "b0.attn", _with(cs, "b0.attn", att.contiguous()))


def test_defect_d_final_norm_without_skipping_the_registers(case):
    cs, c = case("A"), case("A").cfg
    tok = cs.taps["b1.tok2"].reshape(c.n, c.T, c.E)[:, :c.V].reshape(c.n * c.V, c.E)            # rows 0 .. V - 1 instead of nreg .. T - 1
    rows = W.split16(W._ln32(tok, cs.sd["eva.norm.weight"], cs.sd["eva.norm.bias"], 1e-6))
    _planted(cs, "d.ln", _with(cs, "d.ln", tuple(W._padded(r, c.Ep).reshape(-1) for r in rows)))


def test_defect_e_dy_and_dx_parities_swapped_on_the_non_cubic_grid(case):
    cs, c = case("B"), case("B").cfg
    gd, gh, gw = c.grid
    raw = cs.taps["d0.raw"].reshape(c.n, gd, 2, gh, 2, gw, 2, c.dec[1])
    bad = raw.transpose(4, 6)                                      # [.., y, dy, x, dx, c]: the value of (dx, dy) at (dy, dx)
    assert bad.shape == raw.shape and not torch.equal(bad, raw)
    _planted(cs, "d0.raw", _with(cs, "d0.raw", bad.reshape(-1).contiguous()))


def test_defect_f_sample_one_demeaned_with_the_constant_of_sample_zero(case):
    cs, c = case("A"), case("A").cfg
    mean = cs.taps["d.mean"].reshape(c.n, c.dec[3])
    y = cs.taps["y"].clone().reshape(c.n, c.dec[3], -1)
    y[1] += (mean[1] - mean[0]).reshape(-1, 1)
    r = _planted(cs, "y", _with(cs, "y", y.reshape(-1)))
    assert r.worst[0] == 1


def test_defect_g_pooled_plane_averaged_from_the_hi_plane_only(case):
    cs, c = case("A"), case("A").cfg
    d = c.vol[0] // 2
    hi = cs.taps["s0.h"][0].float().reshape(c.n, d, d, d, 32)
    pair = W.split16(W.pool_cl(hi))
    _planted(cs, "s0.p", _with(cs, "s0.p", tuple(p.reshape(-1) for p in pair)))


def test_defect_h_last_row_of_the_mlp_residual_not_written(case):
    cs, c = case("B"), case("B").cfg
    t2 = cs.taps["b0.tok2"].clone().reshape(c.M, c.E)
    t2[c.M - 1] = cs.taps["b0.tok1"].reshape(c.M, c.E)[c.M - 1]
    r = _planted(cs, "b0.tok2", _with(cs, "b0.tok2", t2.reshape(-1)))
    assert r.worst[0] == c.M - 1


def test_defect_i_gate_and_value_swapped_in_the_partial_tile_pair(case):
    cs, c = case("B"), case("B").cfg
    assert c.hid % 16 and c.hid % 4
    h16, lo = W.up(c.hid, 16), 16 * (c.hid // 16)
    sd, p = cs.sd, "eva.blocks.0.mlp."
    a = cs.taps["b0.ln2"].reshape(c.M, c.Ep)[:, :c.E].float()
    g = a @ sd[p + "fc1_g.weight"].half().float().t() + sd[p + "fc1_g.bias"]
    v = a @ sd[p + "fc1_x.weight"].half().float().t() + sd[p + "fc1_x.bias"]
    hd = cs.taps["b0.hd"].clone().reshape(c.M, h16)
    hd[:, lo:c.hid] = (v / (1.0 + torch.exp(-v)) * g).half()[:, lo:]
    r = _planted(cs, "b0.hd", _with(cs, "b0.hd", hd.reshape(-1)))
    assert r.worst[1] >= lo


def test_defect_j_nonzero_in_a_padding_column(case):
    cs, c = case("B"), case("B").cfg
    assert c.Ep > c.E
    ln1 = cs.taps["b0.ln1"].clone().reshape(c.M, c.Ep)
    ln1[5, c.E + 3] = 0.5
    r = _planted(cs, "b0.ln1", _with(cs, "b0.ln1", ln1.reshape(-1)))
    assert r.pad_bad == 1 and r.over == 1


def test_defect_k_token_row_of_the_wrong_sample_at_the_batch_boundary(case):
    cs, c = case("B"), case("B").cfg
    assert c.T % 16, "rows T - T % 16 .. of sample 0 and the first rows of sample 1 share a 16-row tile"
    t1 = cs.taps["b0.tok1"].clone().reshape(c.M, c.E)
    t1[c.T] = t1[0]                                               # sample 1's first row written from sample 0's
    r = _planted(cs, "b0.tok1", _with(cs, "b0.tok1", t1.reshape(-1)))
    assert r.worst[0] == c.T
