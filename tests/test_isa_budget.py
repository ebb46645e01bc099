"""The instruction budget of the z-march family as compiled (tools/isa_budget.py; no GPU: hipcc cross-compiles to gfx950 assembly).

From the code-object metadata: every f16 / bf16 instance of conv3d_k3_zmarch_kernel (strict-precision SPLIT instances apart: they
spill 2 - 12 registers and are a later piece of work) and of conv3d_upcat16_kernel keeps all its values in registers -- 0 spilled
VGPRs, 0 bytes of scratch memory.  A spill in these kernels is traffic through the vector-memory queue whose back-pressure stalls the
consumer waves, inside the per-step loop.

From the assembly: no instance's per-step loop (the outermost loop that holds the MFMAs: one z-step of one wave) has more non-MFMA
instructions than the same instance had before the epilogue work -- the figures of profiles/r07_isa_budget_before.txt, read here, not
restated.  Since that work the activation is a template argument (the last one): each activation's kernel is held to the figure of
the one kernel that served all three.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_budget  # noqa: E402

FILES = ["amx_conv3d_zmarch.hip", "amx_conv3d_upcat.hip"]
pytestmark = pytest.mark.skipif(not os.path.exists(isa_budget.HIPCC), reason="needs hipcc")


def _args(kernel):
    name, rest = kernel.split("<", 1)
    return name, rest.rstrip(">").split(",")


def _is_split(kernel):
    name, a = _args(kernel)
    return name == "conv3d_k3_zmarch_kernel" and a[9] == "true"       # <T, NCK, QT, TY, TX, R, OUTMODE, NS, POOL, SPLIT, STEM[, ACT]>


@pytest.fixture(scope="module")
def rows():
    return [r for f in FILES for r in isa_budget.budget(os.path.join(ROOT, "anatomix_amd", "csrc", f))]


@pytest.fixture(scope="module")
def before():
    with open(os.path.join(ROOT, "profiles", "r07_isa_budget_before.txt")) as f:
        return isa_budget.parse_table(f.read())


def test_tool_sees_every_instance(rows, before):
    """Every instance of the committed `before` table is still compiled and still found by the tool, with the MFMA count it had."""
    have = {(_args(r["kernel"])[0], tuple(_args(r["kernel"])[1][:-1]), r["mfma"]) for r in rows}
    want = {(_args(r["kernel"])[0], tuple(_args(r["kernel"])[1]), r["mfma"]) for r in before}
    assert want and not want - have, sorted(want - have)


def test_no_spills_and_no_scratch(rows):
    bad = [(r["kernel"], r["spill"], r["scratch_bytes"]) for r in rows if not _is_split(r["kernel"]) and (r["spill"] or r["scratch_bytes"])]
    assert not bad, bad
    assert all(r["scr"] == 0 for r in rows if not _is_split(r["kernel"]))


def test_per_step_stream_is_no_longer_than_before(rows, before):
    """Per (instance, loop): the MFMA count is unchanged and the non-MFMA count does not exceed the parent's.  Loops are matched by
    their MFMA count (the stem-fed instance has two: the consumers' step and the stem waves' plane)."""
    ref = {}
    for r in before:
        name, a = _args(r["kernel"])
        ref[(name, tuple(a), r["mfma"])] = r["non_mfma"]
    assert ref
    seen = 0
    for r in rows:
        if _is_split(r["kernel"]):
            continue
        name, a = _args(r["kernel"])
        key = (name, tuple(a[:-1]), r["mfma"])                        # (the activation is the one new template argument)
        assert key in ref, (r["kernel"], r["mfma"])
        assert r["non_mfma"] <= ref[key], (r["kernel"], r["loop"], r["non_mfma"], ref[key])
        seen += 1
    assert seen >= len([r for r in before if not _is_split(r["kernel"])])
