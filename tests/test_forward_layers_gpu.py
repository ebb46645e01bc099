"""GPU: the production forward of the 6 M model, layer by layer, at ragged volume sizes (tests/_layer_walk.py).

Run A is ``forward_hip_taps`` at every activation id from 5 on, the pool ids and the output conv: taps that are plain exports and
leave the launch schedule of the plain forward alone.  Run B adds the stem's activation id 2, which splits the stem pair into its
two launches.  Both must return the plain forward's output bit for bit, and agree with each other bit for bit on every common tap
(the fused stem pair needs no tolerance of its own).  Every layer is then compared with a float64 convolution of the tensors the
GPU itself stored in front of it, at the one-rounding bound of the single-layer tests.

ROUTE_TABLE pins the kernel family of every conv (and which pools run on their own) per case: a routing change fails here, and
whoever makes it picks shapes that reach the new route.  test_bench_kernels_are_walked_or_listed is the ledger of what the walk
does not reach: NOT_WALKED.

Largest err/tol per route family over all cases of one run on an MI355X, f16 / bf16 (0.5 is the store rounding itself; strict:
the worse of rel-L2 and max-rel against its limit):
  conv3d_stem 0.494 / 0.497          conv3d_k3_zmarch 0.578 / 0.497 (stem pair included)      conv3d_k3_v2 0.510 / 0.497
  conv3d_k3_ks 0.508 / 0.496         conv3d_upcat16 0.479 / 0.495                             output conv (planar) 0.015 / 0.011
  conv3d_k3_v2 + upmerge 0.267 / 0.123      conv3d_k3_ks + upmerge 0.133 / 0.099      conv3d_k3_zmarch + upmerge 0.264 / 0.239
  merged routes, share of voxels over the one-rounding bound: 5.2e-5 / 1.6e-5 (CPU emulation of the two launches 5.5e-5 / 4.4e-6, cap 2e-3)
  pools (fused epilogue and pool2): bit-equal.      strict: 0.158 stem, 0.185 z-march, 0.220 generic, 0.230 / 0.357 merged routes.
The f16 figures above 0.5 are two weights of modules 17 and 62 that the device folds one fp32 ulp away from the host
(_layer_walk.conv_params); no voxel of any case is over its bound.
"""
import pytest
import torch

import anatomix_amd
from _layer_walk import family, groups, report, routes_of, walk
from oracle import unet_ref as R

pytestmark = pytest.mark.gpu

KW = R.VARIANTS["anatomix"]
GROUPS = groups(KW)[0]
CONVS = [g["module"] for g in GROUPS if g["op"] == "conv"]
POOLS = [g["module"] for g in GROUPS if g["op"] == "pool"]                      # 9, 16, 23, 30
ACTS = [g["out"] for g in GROUPS if g["op"] == "conv" and not g["final"]]       # 2, 5, 8, 12, ..., 64
TAPS_A = sorted(ACTS[1:] + POOLS + [CONVS[-1]])
TAPS_B = sorted(TAPS_A + ACTS[:1])

# (n, (D, H, W)): what each reaches is the table of the issue this module answers, restated by ROUTE_TABLE below
CASES = [
    (2, (32, 32, 48)),      # W % 32 != 0: two-launch stem, partial x tiles at level 0; level 1 W = 24, level 2 W = 12; bottom 2 x 2 x 3
    (1, (48, 80, 96)),      # stem pair, 3 x 10 tiles, ragged z segments; level 1 W = 48; bottom 3 x 5 x 6
    (3, (80, 48, 32)),      # one x tile, batch 3, D the long axis; level 1 W = 16; bottom 5 x 3 x 2
    (1, (32, 48, 160)),     # W > 128, five x tiles; level 1 W = 80, level 2 W = 40
    (2, (64, 32, 112)),     # W % 32 != 0 with W >= 64; level 1 W = 56; level 3 W = 14, bottom W = 7
]
IDS = ["n%d_%dx%dx%d" % (n, *s) for n, s in CASES]

# The deepest two levels of the benchmark's batch: 4 x 128^3 on the GPU, the walk over levels 3 and 4 only (4 x 16^3 and 4 x 8^3
# voxels: cheap in float64).  Reaches the split-K instances that only a batch of 8^3 bottlenecks selects.
DEEP_CASE = (4, (128, 128, 128))
DEEP_MODULES = [24, 27, 30, 31, 34, 38, 41]
DEEP_TAPS = [23, 26, 29, 30, 33, 36, 40, 43]


def _table(**fam):
    return {m: f.replace("__", " + ") for f, ms in fam.items() for m in ms}


# Kernel family per conv module (the name up to '<', "+ upmerge" where the merged-tap launch is attached); a pool id is listed where
# the pool is a launch of its own and absent where the conv in front wrote it; no entry at module 3 = the stem pair (one record at
# module 0).  f16 and bf16 take the same routes.  Filled from a run on an MI355X and reviewed against the comments at CASES:
#   * (32, 32, 48): level 2 (W = 12) runs the generic kernel, not split-K bricks: its layers are packed four tiles wide, which
#     conv3d_k3_ks takes from W = 16 on.  The 8-cell split-K bricks are walked at level 3 of (64, 32, 112) (W = 14) and in DEEP_CASE.
ROUTES_16 = {
    (2, (32, 32, 48)): _table(conv3d_stem=[0], conv3d_k3_zmarch=[3, 6, 62, 65], conv3d_upcat16=[59], pool2=[16, 23, 30],
                              conv3d_k3_v2=[10, 13, 17, 20, 24, 27, 31, 34, 38, 41, 45, 48, 55], conv3d_k3_v2__upmerge=[52]),
    (1, (48, 80, 96)): _table(conv3d_k3_zmarch=[0, 6, 10, 13, 55, 62, 65], conv3d_k3_ks=[17, 20, 24, 27, 41, 48], pool2=[23, 30],
                              conv3d_k3_v2=[31, 34, 38], conv3d_k3_ks__upmerge=[45], conv3d_k3_zmarch__upmerge=[52], conv3d_upcat16=[59]),
    (3, (80, 48, 32)): _table(conv3d_k3_zmarch=[0, 6, 62, 65], conv3d_upcat16=[59], pool2=[16, 23, 30],
                              conv3d_k3_v2=[10, 13, 17, 20, 24, 27, 31, 34, 38, 41, 45, 48, 55], conv3d_k3_v2__upmerge=[52]),
    (1, (32, 48, 160)): _table(conv3d_k3_zmarch=[0, 6, 10, 13, 55, 62, 65], conv3d_k3_ks=[17, 20, 24, 27, 31, 34, 41, 48], pool2=[23, 30],
                               conv3d_k3_v2__upmerge=[38], conv3d_k3_ks__upmerge=[45], conv3d_k3_zmarch__upmerge=[52], conv3d_upcat16=[59]),
    (2, (64, 32, 112)): _table(conv3d_stem=[0], conv3d_k3_zmarch=[3, 6, 10, 13, 55, 62, 65], conv3d_k3_ks=[17, 20, 24, 27, 41, 48],
                               pool2=[23, 30], conv3d_k3_v2=[31, 34, 38], conv3d_k3_ks__upmerge=[45], conv3d_k3_zmarch__upmerge=[52],
                               conv3d_upcat16=[59]),
}
ROUTE_TABLE = {
    "f16": ROUTES_16, "bf16": ROUTES_16,
    # split operands: no stem pair, no upcat16 (the 48 -> 16 layer runs as skip conv + merged taps), no split-K
    "strict": {
        (2, (32, 32, 48)): _table(conv3d_stem=[0], conv3d_k3_zmarch=[3, 6, 62, 65], pool2=[16, 23, 30], conv3d_k3_zmarch__upmerge=[59],
                                  conv3d_k3_v2=[10, 13, 17, 20, 24, 27, 31, 34, 38, 41, 45, 48, 55], conv3d_k3_v2__upmerge=[52]),
        (1, (48, 80, 96)): _table(conv3d_stem=[0], conv3d_k3_zmarch=[3, 6, 62, 65], pool2=[16, 23, 30], conv3d_k3_zmarch__upmerge=[59],
                                  conv3d_k3_v2=[10, 13, 17, 20, 24, 27, 31, 34, 38, 41, 48, 55], conv3d_k3_v2__upmerge=[45, 52]),
    },
}

# Kernel instances of the benchmark's workloads that no walked case runs: the honest list of what this module does not cover.
# (A merged pair's record holds both names cut short -- 34 and 26 characters -- so its instances are known by those prefixes.)
NOT_WALKED = {
    "upmerge<f16,q2,2x4x16,b3,k": "module 52 at 128^3: the 4-tile brick is chosen from 2048 sixteen-cell tiles of the low-resolution tensor on "
                                  "(n * D/4 * H/4 * ceil(W/64)); the smallest such volume has 2^20 voxels, half a benchmark volume, and its "
                                  "float64 reference takes far longer than a test may.  The 2-tile brick of the same kernel is walked.",
}

_cache = {}


def _model(device, precision):
    key = ("model", precision)
    if key not in _cache:
        m = anatomix_amd.Unet(**KW)
        sd = R.synthetic_state_dict(KW, 0, gain=1.0)
        m.load_state_dict(sd, strict=True)
        m.precision = precision
        _cache[key] = (m.to(device).eval(), sd)
    return _cache[key]


def _profile(device, precision, n, size, keep=True):
    """(output, launch records) of one profiled plain forward; the records are kept per shape and precision for the table tests."""
    m, _ = _model(device, precision)
    with torch.no_grad():
        y, recs = m.profile_forward(R.synthetic_input(100 + n, n, size).to(device))
    if keep:
        _cache[(precision, n, size)] = recs
    return y, recs


def _records(device, precision, n, size):
    key = (precision, n, size)
    return _cache[key] if key in _cache else _profile(device, precision, n, size)[1]


def _families(recs):
    """module id -> family for every conv record, 'pool2' for the pools that run as a launch of their own."""
    return {r["module_idx"]: family(r["kernel"]) for r in recs}


def _instances(recs):
    """Full kernel instance names; a merged pair counts as its two launches (the first name is cut at 34 characters there)."""
    return {part.strip() for r in recs for part in r["kernel"].split(" + ")}


def _walk_case(device, precision, n, size):
    m, sd = _model(device, precision)
    x = R.synthetic_input(100 + n, n, size)
    xd = x.to(device)
    with torch.no_grad():
        y = m(xd)
        ya, fa = m.forward_hip_taps(xd, TAPS_A)
        yb, fb = m.forward_hip_taps(xd, TAPS_B)
    yp, recs = _profile(device, precision, n, size)
    # the taps rerouted nothing that changes a value, and the profiled forward is the plain one
    assert torch.equal(ya, y) and torch.equal(yb, y) and torch.equal(yp, y)
    assert torch.equal(fa[-1], ya) and torch.equal(fb[-1], yb)            # the tap at the output conv IS the output
    ta = {i: f.cpu() for i, f in zip(TAPS_A, fa)}
    tb = {i: f.cpu() for i, f in zip(TAPS_B, fb)}
    for i in TAPS_A:                                                       # the stem pair against its two launches, and all behind it
        assert torch.equal(ta[i], tb[i]), f"tap {i}: run A (production schedule) differs from run B (tap inside the stem pair)"
    routes = routes_of(recs)
    if CONVS[1] not in routes:                                             # the pair is one record at the stem's id
        assert "stem1->16->16" in routes[CONVS[0]]
        routes[CONVS[1]] = routes[CONVS[0]]
    out = walk(KW, sd, x, tb, precision, routes)
    print(f"\n{precision} n={n} {size}\n{report(out)}")
    assert [r.module for r in out] == [g["module"] for g in GROUPS]        # every conv and every pool was checked
    assert all(r.ref_absmax > 0.1 for r in out), report(out)               # no dead tensor passes
    assert all(r.ok for r in out), report([r for r in out if not r.ok])
    return out


@pytest.mark.parametrize("precision", ["f16", "bf16"])
@pytest.mark.parametrize("n,size", CASES, ids=IDS)
def test_every_layer_of_the_production_forward(device, n, size, precision):
    _walk_case(device, precision, n, size)


def test_deep_levels_of_the_benchmark_batch(device):
    """4 x 128^3, f16: levels 3 and 4 as the benchmark runs them (the taps stay behind the stem pair and off the conv ids)."""
    n, size = DEEP_CASE
    m, sd = _model(device, "f16")
    x = R.synthetic_input(100 + n, n, size)
    xd = x.to(device)
    with torch.no_grad():
        y = m(xd)
        ya, fa = m.forward_hip_taps(xd, DEEP_TAPS)
        yp, recs = _profile(device, "f16", n, size)
    same = torch.equal(ya, y) and torch.equal(yp, y)
    taps = {i: f.cpu() for i, f in zip(DEEP_TAPS, fa)}
    del y, ya, yp, fa
    m._workspace = None                                  # (sized for 4 x 128^3: not kept for the rest of the session)
    assert same
    out = walk(KW, sd, x, taps, "f16", routes_of(recs))
    print(f"\nf16 n={n} {size}, levels 3 and 4\n{report(out)}")
    assert [r.module for r in out] == DEEP_MODULES
    assert all(r.ref_absmax > 0.1 for r in out), report(out)
    assert all(r.ok for r in out), report([r for r in out if not r.ok])


@pytest.mark.parametrize("n,size", CASES[:2], ids=IDS[:2])
def test_every_layer_strict(device, n, size):
    out = _walk_case(device, "strict", n, size)
    assert {r.kind for r in out} == {"strict", "pool"}


@pytest.mark.parametrize("precision,n,size", [(p, n, s) for p in ("f16", "bf16") for n, s in CASES] + [("strict", n, s) for n, s in CASES[:2]],
                         ids=[p + "-" + i for p in ("f16", "bf16") for i in IDS] + ["strict-" + i for i in IDS[:2]])
def test_route_table(device, precision, n, size):
    got = _families(_records(device, precision, n, size))
    want = ROUTE_TABLE[precision][(n, size)]
    assert got == want, f"{precision} n={n} {size}: routes changed\n got  {got}\n want {want}"


def test_bench_kernels_are_walked_or_listed(device):
    """Every kernel instance of the benchmark's workloads (6 M model, f16, 128^3 at batch 1 and 4) runs in some walked case, or
    is listed in NOT_WALKED with the reason.  Needs no CPU reference: profiled forwards only."""
    walked = set()
    for n, size in CASES:
        walked |= _instances(_records(device, "f16", n, size))
    walked |= _instances([r for r in _records(device, "f16", *DEEP_CASE) if r["module_idx"] in DEEP_MODULES])
    bench = set()
    for n in (1, 4):
        bench |= _instances(_records(device, "f16", n, (128, 128, 128)))
    _model(device, "f16")[0]._workspace = None          # (sized for 4 x 128^3: not kept for the rest of the session)
    missing = sorted(bench - walked - set(NOT_WALKED))
    stale = sorted(k for k in NOT_WALKED if k in walked or k not in bench)
    print("bench instances:\n  " + "\n  ".join(sorted(bench)))
    assert not missing, "bench kernels that no walked case runs and NOT_WALKED does not list:\n  " + "\n  ".join(missing)
    assert not stale, "NOT_WALKED entries that are walked after all, or that the benchmark no longer runs:\n  " + "\n  ".join(stale)
    assert all(isinstance(v, str) and len(v) > 10 for v in NOT_WALKED.values())
