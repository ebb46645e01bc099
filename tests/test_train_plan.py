"""Host only: ``plan_network`` (anatomix_amd/model/train.py) -- the typed steps the training function drives, and everything it refuses
before the first launch.  No GPU: the plan holds no tensors."""
import contextlib
import io
from types import SimpleNamespace

import pytest
import torch.nn as nn

import anatomix_amd
from anatomix_amd.model import train as TR
from oracle import pretrain_inputs as PI
from oracle import unet_ref as R

SAMPLED_AT = "sampled taps are implemented at conv ids (pre-norm outputs) and the output conv"
SHALLOW = dict(dimension=3, input_nc=1, output_nc=16, num_downs=2, ngf=16)


def _unet(**kw):
    with contextlib.redirect_stdout(io.StringIO()):           # (the constructor prints its skip ids, as the reference does)
        return anatomix_amd.Unet(**kw).train()


def _blocks(steps):
    return [s for s in steps if isinstance(s, TR.ConvBlock)]


def test_plan_of_the_6m_variant():
    m = _unet(**R.VARIANTS["anatomix"])
    steps = TR.plan_network(m, PI.NCE_LAYERS, sampled=True)
    blocks = _blocks(steps)
    assert len(blocks) == sum(isinstance(mod, nn.Conv3d) for mod in m.model) == 20
    assert [b.kind for b in blocks].count("output") == 1 and steps[-1].kind == "output" and steps[-1].idx == len(m.model) - 1
    assert all(b.kind == "norm" and b.norm is m.model[b.idx + 1] and b.alias_ids == (b.idx + 1, b.idx + 2) for b in blocks[:-1])
    # every Up reads the skip the reference pops there: decoder_idx[k] takes what encoder_idx[-1 - k] pushed (network.py:491-495)
    by_name = {b.name: b for b in blocks}
    ups = [s for s in steps if isinstance(s, TR.Up)]
    assert [u.idx for u in ups] == m.decoder_idx
    for k, u in enumerate(ups):
        assert by_name[u.skip].last_id == m.encoder_idx[-1 - k] and by_name[u.skip].push_skip
        nxt = steps[steps.index(u) + 1]
        assert (nxt.src, nxt.low, nxt.cat) == (u.skip, u.low, "fused") and nxt.inputs == (u.skip, u.low)
    assert sorted(b.last_id for b in blocks if b.push_skip) == m.encoder_idx
    # every tap id is served by exactly one record
    served = [t for s in steps for t in s.tap_ids]
    assert sorted(served) == sorted(PI.NCE_LAYERS)
    assert all(how == "sampled" for b in blocks for _, how in b.taps)
    dense = TR.plan_network(m, [0, 1, 2, 9, 37, 65])
    hows = {t: how for b in _blocks(dense) for t, how in b.taps}
    assert hows == {0: "pre", 1: "act", 2: "act", 65: "output"}
    assert [s.idx for s in dense if not isinstance(s, TR.ConvBlock) and s.tap] == [9, 37]


@pytest.mark.parametrize("interp,cat", [("trilinear", "materialised"), ("nearest", "fused")])
def test_concat_inputs_are_materialised_for_trilinear_and_fused_for_nearest(interp, cat):
    m = _unet(dimension=3, input_nc=1, output_nc=32, num_downs=2, ngf=32, norm="instance", pooling="Avg", interp=interp, norm_eps=1e-2)
    steps = TR.plan_network(m, [3, 13, 20, 27, 34])
    behind_up = [steps[i + 1] for i, s in enumerate(steps) if isinstance(s, TR.Up)]
    assert len(behind_up) == 2 and all(b.cat == cat and b.low is not None for b in behind_up)
    for b in behind_up:
        assert b.inputs == ((f"cat{b.idx}", None) if cat == "materialised" else (b.src, b.low))
    assert all(b.cat is None and b.low is None for b in _blocks(steps) if b not in behind_up)
    assert all(s.avg for s in steps if isinstance(s, TR.Pool))
    assert all(isinstance(b.norm, nn.InstanceNorm3d) and b.kind == "norm" for b in _blocks(steps)[:-1])


def test_an_eval_mode_batchnorm_makes_its_block_frozen():
    m = _unet(**SHALLOW)
    m.model[4].eval()
    kinds = {b.idx: b.kind for b in _blocks(TR.plan_network(m))}
    assert kinds[3] == "frozen" and kinds[len(m.model) - 1] == "output"
    assert all(k == "norm" for i, k in kinds.items() if i not in (3, len(m.model) - 1))


def _cases():
    """(name, model, layers, sampled, message, whether sampled_unsupported_reason sees it)"""
    m = _unet(**SHALLOW)
    kinds = [type(mod).__name__ for mod in m.model]
    frozen = _unet(**SHALLOW)
    frozen.model[4].eval()
    no_skip = _unet(use_skip_connection=False, **SHALLOW)
    foreign = _unet(**SHALLOW)
    foreign.model[5] = nn.Identity()
    return [
        ("norm id", m, [1], True, SAMPLED_AT, True),
        ("pool id", m, [kinds.index("MaxPool3d")], True, SAMPLED_AT, True),
        ("up id", m, [kinds.index("Upsample")], True, SAMPLED_AT, True),
        ("frozen block", frozen, [3], True, "sampled taps at a frozen-statistics block", True),
        ("no skip connections", no_skip, [], False, "upsample without skip connection in the HIP training path", False),
        ("foreign module", foreign, [], False, "module 5 (Identity) in the HIP training path", False),
    ]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_what_the_plan_refuses_raises_before_any_launch(case):
    _, m, layers, sampled, message, seen_by_reason = case
    with pytest.raises(NotImplementedError) as e:
        TR.plan_network(m, layers, sampled)
    assert str(e.value) == message
    if seen_by_reason:
        # (a stand-in for a CUDA input: the reason functions only read its shape)
        x = SimpleNamespace(dim=lambda: 5, shape=(2, 1, 32, 32, 32), is_cuda=True)
        assert TR.sampled_unsupported_reason(m, x, layers) == message
        assert TR.unsupported_reason(m, x, layers) is None          # the same taps, dense: covered
