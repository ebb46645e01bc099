"""GPU: the label-overlap and Jacobian kernels through the C ABI (csrc/amx_regmetrics.hip) and their Python surface, against
numpy on the host, the float64 restatement tests/_regmetrics_ref.py and the fixtures captured from the reference's JacobianDet and
from sklearn's f1_score (tools/make_golden_regmetrics.py -> tests/golden/regmetrics_golden.npz).

Bounds.  Label counts: exact equality with numpy.bincount.  Dice: 1e-12 (exact integer counts, both sides divide in double).
Determinant field: max abs error <= (5e-6 + 10 x ref_vs_f64) x max|reference| against float64, the project's bound for an fp32
kernel with another summation order, ref_vs_f64 being the fp32 reference's own distance from float64 (fixture).  Statistics,
against numpy float64 on the kernel's own field: count, min, max exact; mean and the log figures 1e-6 relative (sums in double,
one rounding to fp32 at the end: 6e-8).  No bound comes from the code under test; every test prints its figure before it asserts."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _regmetrics_ref as MR

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "regmetrics_golden.npz"))
TORCH_DT = {"f32": torch.float32, "i64": torch.int64, "u8": torch.uint8}
DTYPE_PAIRS = [("f32", "f32"), ("u8", "f32"), ("i64", "u8")]
# The overlap launch uses at most 2048 workgroups of 256 threads, a thread taking 4 quads of 4 voxels per turn: one sweep of the
# grid is 2048 * 256 * 16 = 8388608 voxels.  One full sweep plus an odd rest makes the grid-stride loop run twice.
SWEEP = 2048 * 256 * 16
MULTI_SWEEP = SWEEP + 4099
INVALID = -1


def dev():
    return torch.device("cuda:0")


def lib():
    from anatomix_amd import _lib
    return _lib.load()


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


def code(t):
    from anatomix_amd import _lib
    return _lib.SEG_LABEL[{torch.float32: "float32", torch.int64: "int64", torch.uint8: "uint8"}[t.dtype]]


def overlap_raw(a, b, bins, sentinel=-7):
    """amx_label_overlap on two device tensors (views allowed) -> (status, counts [bins, 3], bad) as numpy."""
    from anatomix_amd import _lib
    out = torch.full((3 * max(bins, 1) + 1,), sentinel, dtype=torch.int64, device=dev())
    rc = lib().amx_label_overlap(_lib.ptr(a), code(a), _lib.ptr(b), code(b), a.numel(), bins, _lib.ptr(out), _lib.ptr(out[-1:]), stream())
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return rc, o[:-1].reshape(-1, 3), int(o[-1])


def labels(pattern, n, bins, seed):
    """blocky: runs of 4096 equal labels (whole waves see one label); random: one draw per voxel; mix: both and runs of 7."""
    rs = np.random.RandomState(seed)

    def runs(length, count):
        return np.repeat(rs.randint(0, bins, -(-count // length)), length)[:count]
    if pattern == "blocky":
        return runs(4096, n)
    if pattern == "random":
        return rs.randint(0, bins, n)
    third = n // 3
    return np.concatenate([runs(4096, third), rs.randint(0, bins, third), runs(7, n - 2 * third)])


def pair(pattern, n, bins, seed=0):
    a = labels(pattern, n, bins, seed)
    b = np.roll(a, 129)
    flip = np.random.RandomState(seed + 1).rand(n) < 0.02
    return a, np.where(flip, np.random.RandomState(seed + 2).randint(0, bins, n), b)


def check_counts(a_np, b_np, a, b, bins, what):
    rc, counts, bad = overlap_raw(a, b, bins)
    want, want_bad = MR.overlap_counts(a_np, b_np, bins)
    diff = int(np.abs(counts - want).max())
    print(f"{what}: voxels {a.numel()} bins {bins}: status {rc}, largest count difference {diff}, bad {bad} (numpy {want_bad}), "
          f"both-count total {int(counts[:, 2].sum())}")
    assert rc == 0 and diff == 0 and bad == want_bad
    return counts


@pytest.mark.parametrize("voxels", [1, 63, 4099, MULTI_SWEEP])
@pytest.mark.parametrize("da,db", DTYPE_PAIRS)
def test_overlap_sizes_and_dtypes(voxels, da, db):
    a_np, b_np = pair("mix", voxels, 6)
    a, b = torch.from_numpy(a_np).to(dev()).to(TORCH_DT[da]), torch.from_numpy(b_np).to(dev()).to(TORCH_DT[db])
    check_counts(a_np, b_np, a, b, 6, f"{da}/{db} mix")
    if voxels == 4099:
        first = overlap_raw(a, b, 6)
        assert all(np.array_equal(x, y) for x, y in zip(first, overlap_raw(a, b, 6)))           # run to run


@pytest.mark.parametrize("skew", ["a_only", "both"])
@pytest.mark.parametrize("da,db", DTYPE_PAIRS)
def test_overlap_unaligned_views(skew, da, db):
    """Views that start one element into their buffers: with both volumes skewed alike the kernel peels a head and keeps its wide
    loads; with one of them skewed no head aligns both and every voxel takes the one-by-one path."""
    n = 4099
    a_np, b_np = pair("mix", n + 1, 6, seed=3)
    a_full, b_full = torch.from_numpy(a_np).to(dev()).to(TORCH_DT[da]), torch.from_numpy(b_np).to(dev()).to(TORCH_DT[db])
    a = a_full[1:]
    b, b_ref = (b_full[1:], b_np[1:]) if skew == "both" else (b_full[:-1], b_np[:-1])
    assert a.data_ptr() % 16 != 0 or da == "u8"
    check_counts(a_np[1:], b_ref, a, b, 6, f"{da}/{db} offset view ({skew})")


@pytest.mark.parametrize("bins", [1, 6, 256, 1024])
@pytest.mark.parametrize("pattern", ["blocky", "random", "mix"])
def test_overlap_bins_and_patterns(bins, pattern):
    n = 70001
    a_np, b_np = pair(pattern, n, bins, seed=bins)
    a, b = torch.from_numpy(a_np).to(dev()).float(), torch.from_numpy(b_np).to(dev())
    counts = check_counts(a_np, b_np, a, b, bins, f"{pattern}")
    assert int(counts[:, 0].sum()) == n and int(counts[:, 1].sum()) == n


def test_overlap_bad_values_are_counted_and_left_out():
    from anatomix_amd.registration import label_overlap
    n, bins = 9001, 6
    a_np, b_np = pair("mix", n, bins, seed=11)
    a_np, b_np = a_np.astype(np.float64), b_np.astype(np.float64)
    rs = np.random.RandomState(12)
    bad_vals = [2.5, -1.0, np.nan, float(bins), np.inf, 1e10, -0.5]
    ia, ib = rs.choice(n, 40, replace=False), rs.choice(n, 40, replace=False)
    ib[:5] = ia[:5]                                                 # bad in both volumes at one voxel: counted once
    a_np[ia] = rs.choice(bad_vals, 40)
    b_np[ib] = rs.choice(bad_vals, 40)
    a_np[:256] = 2.5                                                # a whole wave of bad voxels (the uniform path)
    a, b = torch.from_numpy(a_np).to(dev()).float(), torch.from_numpy(b_np).to(dev()).float()
    check_counts(a_np, b_np, a, b, bins, "f32/f32 bad values")
    with pytest.raises(ValueError, match=str(MR.overlap_counts(a_np, b_np, bins)[1]) + " voxels"):
        label_overlap(a, b, bins=bins)
    # integer volumes: negative and too large values
    ai = torch.from_numpy(np.where(np.isfinite(a_np) & (a_np == np.floor(a_np)) & (np.abs(a_np) < 100), a_np, -3)).to(dev()).long()
    bu = torch.from_numpy(np.where(np.isfinite(b_np) & (b_np >= 0) & (b_np < 200) & (b_np == np.floor(b_np)), b_np, 255)).to(dev()).to(torch.uint8)
    check_counts(ai.cpu().numpy(), bu.cpu().numpy(), ai, bu, bins, "i64/u8 bad values")
    big = torch.tensor([1 << 40, -(1 << 40), 3, (1 << 32) + 3], dtype=torch.int64, device=dev())
    rc, counts, bad = overlap_raw(big, torch.full((4,), 3, dtype=torch.uint8, device=dev()), bins)
    assert rc == 0 and bad == 3 and counts[3].tolist() == [1, 1, 1] and int(counts.sum()) == 3


# (sparse_labels has labels above 255, which uint8 cannot hold)
@pytest.mark.parametrize("case,dt", [(c, t) for c in MR.DICE_CASES for t in ("f32", "i64", "u8") if not (c == "sparse_labels" and t == "u8")])
def test_dice_score_is_sklearn(case, dt):
    """Against the recorded sklearn.metrics.f1_score(average='macro', labels=unique(fixed)[1:]).  `no_zero` has no label 0 in the
    fixed map: the [1:] rule then drops label 1, as the reference's call does."""
    from anatomix_amd.registration import dice_score
    fix, mov = MR.dice_pair(case)
    f, m = torch.from_numpy(fix).to(dev()).to(TORCH_DT[dt]), torch.from_numpy(mov).to(dev()).float()
    got, per = dice_score(f, m)
    want = float(G["dice|" + case])
    print(f"dice {case} ({dt}/f32): {got:.15f}  sklearn {want:.15f}  difference {abs(got - want):.2e}  labels {sorted(per)}")
    assert abs(got - want) <= 1e-12
    assert sorted(per) == np.unique(fix).astype(int).tolist()[1:]
    if case == "no_zero":
        assert 1 not in per and 0 not in per


def test_overlap_invalid_arguments_launch_nothing():
    from anatomix_amd import _lib
    a = torch.zeros(64, dtype=torch.float32, device=dev())
    out = torch.full((3 * 1024 + 1,), -7, dtype=torch.int64, device=dev())
    L, st = lib(), stream()

    def call(pa, ca, pb, cb, n, bins, pc, pbad):
        return L.amx_label_overlap(pa, ca, pb, cb, n, bins, pc, pbad, st)
    p, po, pbad = _lib.ptr(a), _lib.ptr(out), _lib.ptr(out[-1:])
    assert call(p, 0, p, 0, 64, 0, po, pbad) == INVALID
    assert call(p, 0, p, 0, 64, 1025, po, pbad) == INVALID
    assert call(p, 3, p, 0, 64, 6, po, pbad) == INVALID and call(p, 0, p, -1, 64, 6, po, pbad) == INVALID
    assert call(None, 0, p, 0, 64, 6, po, pbad) == INVALID and call(p, 0, None, 0, 64, 6, po, pbad) == INVALID
    assert call(p, 0, p, 0, 64, 6, None, pbad) == INVALID and call(p, 0, p, 0, 64, 6, po, None) == INVALID
    assert call(p, 0, p, 0, 0, 6, po, pbad) != 0
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                 # nothing was zeroed, nothing was counted
    assert call(p, 0, p, 0, 64, 6, po, pbad) == 0
    torch.cuda.synchronize()
    assert out[:3].tolist() == [64, 64, 64] and int(out[-1]) == 0


# ---- Jacobian ---------------------------------------------------------------------------------------------------------------
def jacobian_raw(disp, ident, want_field=True, want_stats=True):
    """amx_jacobian_det on a device field [3, H, W, D] -> (status, field or None, stats or None) as numpy."""
    from anatomix_amd import _lib
    _, h, w, d = disp.shape
    jd = torch.full((h - 1, w - 1, d - 1), float("nan"), device=dev()) if want_field else None
    stats = torch.full((6,), float("nan"), device=dev()) if want_stats else None
    nb = lib().amx_jacobian_det_scratch_bytes(h, w, d)
    sc = torch.empty(nb, dtype=torch.uint8, device=dev())
    rc = lib().amx_jacobian_det(_lib.ptr(disp), h, w, d, ident, _lib.ptr(jd), _lib.ptr(stats), _lib.ptr(sc), nb, stream())
    torch.cuda.synchronize()
    return rc, None if jd is None else jd.cpu().numpy(), None if stats is None else stats.cpu().numpy()


def field_bound(ref_vs_f64, j64):
    return (5e-6 + 10.0 * ref_vs_f64) * float(np.abs(j64).max())


def check_jacobian(disp_np, ident, ref_vs_f64, what):
    j64 = MR.jacobian_f64(disp_np, ident)
    disp = torch.from_numpy(disp_np).to(dev())
    rc, jd, stats = jacobian_raw(disp, ident)
    assert rc == 0 and jd.shape == j64.shape
    b = field_bound(ref_vs_f64, j64)
    err = float(np.abs(jd.astype(np.float64) - j64).max())
    print(f"{what}: field max abs error {err:.3e}, bound {b:.3e} (ref_vs_f64 {ref_vs_f64:.3e}, max|J| {np.abs(j64).max():.4f})")
    assert err <= b
    # statistics against numpy float64 on the kernel's own field
    want = MR.jacobian_stats(jd)
    n = jd.size
    print(f"   stats kernel {stats.tolist()}\n   stats numpy  {want.tolist()}")
    assert stats[0] == np.float32((jd <= 0).sum() / n) and stats[1] == jd.min() and stats[2] == jd.max()
    for i in (3, 4, 5):
        if np.isnan(want[i]):
            assert np.isnan(stats[i])
        else:
            assert abs(float(stats[i]) - want[i]) <= 1e-6 * abs(want[i]), (i, stats[i], want[i])
    # folding share against the float64 field: voxels within the field bound of zero may fall on either side
    lo, hi = (j64 < -b).sum() / n, (j64 <= b).sum() / n
    print(f"   folding share {float(stats[0]):.6f} in [{lo:.6f}, {hi:.6f}]")
    assert np.float32(lo) <= stats[0] <= np.float32(hi)
    # each output alone gives the same bits, and so does a second call
    rc1, jd1, _ = jacobian_raw(disp, ident, True, False)
    rc2, _, st2 = jacobian_raw(disp, ident, False, True)
    rc3, jd3, st3 = jacobian_raw(disp, ident)
    assert rc1 == rc2 == rc3 == 0
    assert np.array_equal(jd1, jd, equal_nan=True) and np.array_equal(jd3, jd, equal_nan=True)
    assert np.array_equal(st2, stats, equal_nan=True) and np.array_equal(st3, stats, equal_nan=True)
    return jd


@pytest.mark.parametrize("shape,kind", MR.jac_cases())
@pytest.mark.parametrize("ident", [0, 1])
def test_jacobian_against_float64(shape, kind, ident):
    key = MR.jac_key(shape, kind, ident)
    check_jacobian(MR.jac_field(shape, kind), ident, float(G[key + "|ref_vs_f64"]), key)


@pytest.mark.parametrize("shape", [(66, 66, 130), (130, 130, 128)])
def test_jacobian_grid_stride(shape):
    """More determinants than one sweep of the launch covers (2048 workgroups x 256 threads, a thread taking 1 determinant on the
    scalar path and 4 on the 16-byte path, D % 4 == 0): 65 * 65 * 129 = 545025 > 524288 and 129 * 129 * 32 = 532512 > 524288.  Not in
    the fixture: ref_vs_f64 is taken here, from the fp32 restatement that the generator proved bit-equal to the reference."""
    disp = MR.jac_field(shape, "fold")
    y, g = MR.reference_inputs(disp, 1)
    r32, j64 = MR.jacobian_det(y, g)[0].numpy(), MR.jacobian_f64(disp, 1)
    e = float(np.abs(r32.astype(np.float64) - j64).max() / np.abs(r32).max())
    check_jacobian(disp, 1, e, f"jac|{shape}|fold|id1")


@pytest.mark.parametrize("shape,kind", [((33, 17, 9), "fold"), ((7, 6, 132), "smooth"), ((5, 3, 2), "fold")])
def test_python_surface_against_fixture(shape, kind):
    from anatomix_amd.registration import JACOBIAN_STATS, JacobianDet, generate_grid, jacobian_determinant, jacobian_statistics
    disp = MR.jac_field(shape, kind)
    key = MR.jac_key(shape, kind, 1)
    want = G[key + "|full"]
    b = (5e-6 + 10.0 * float(G[key + "|ref_vs_f64"])) * float(np.abs(want).max())
    y, _ = MR.reference_inputs(disp, 1)
    got = JacobianDet(torch.cat([y, y]).to(dev()), generate_grid(shape))
    assert got.shape == (2,) + want.shape and torch.equal(got[0], got[1])
    fast, stats = jacobian_determinant(torch.from_numpy(disp).to(dev())[None], return_stats=True)
    e1 = float(np.abs(got[0].cpu().numpy().astype(np.float64) - want).max())
    e2 = float(np.abs(fast[0].cpu().numpy().astype(np.float64) - want).max())
    print(f"{key}: JacobianDet max abs error {e1:.3e}, jacobian_determinant {e2:.3e}, bound {b:.3e} against the reference's fp32")
    assert e1 <= b and e2 <= b
    d = jacobian_statistics(torch.from_numpy(disp).to(dev())[None])
    assert list(d) == list(JACOBIAN_STATS) and np.array_equal(np.array(list(d.values()), np.float32), stats.cpu().numpy(), equal_nan=True)
    assert jacobian_determinant(torch.from_numpy(disp).to(dev())[None]).shape == (1,) + want.shape


def test_jacobian_invalid_arguments_launch_nothing():
    from anatomix_amd import _lib
    L, st = lib(), stream()
    disp = torch.zeros(3, 4, 5, 6, device=dev())
    jd = torch.full((3, 4, 5), -7.0, device=dev())
    stats = torch.full((6,), -7.0, device=dev())
    nb = L.amx_jacobian_det_scratch_bytes(4, 5, 6)
    sc = torch.empty(nb, dtype=torch.uint8, device=dev())
    pd, pj, ps, pc = _lib.ptr(disp), _lib.ptr(jd), _lib.ptr(stats), _lib.ptr(sc)
    assert nb > 0 and L.amx_jacobian_det_scratch_bytes(1, 5, 6) == 0
    for hwd in ((1, 5, 6), (4, 1, 6), (4, 5, 1), (0, 5, 6)):
        assert L.amx_jacobian_det(pd, *hwd, 1, pj, ps, pc, nb, st) == INVALID
    assert L.amx_jacobian_det(None, 4, 5, 6, 1, pj, ps, pc, nb, st) == INVALID
    assert L.amx_jacobian_det(pd, 4, 5, 6, 1, None, None, pc, nb, st) == INVALID                     # both outputs null
    assert L.amx_jacobian_det(pd, 4, 5, 6, 1, pd, ps, pc, nb, st) == INVALID                         # d_jdet aliases d_disp
    inside = ctypes.c_void_p(disp.data_ptr() + 4 * 100)
    assert L.amx_jacobian_det(pd, 4, 5, 6, 1, inside, ps, pc, nb, st) == INVALID                     # ... or lies inside it
    assert L.amx_jacobian_det(pd, 4, 5, 6, 1, pj, ps, pc, nb - 1, st) == INVALID                     # too little scratch
    assert L.amx_jacobian_det(pd, 4, 5, 6, 1, pj, ps, None, nb, st) == INVALID
    torch.cuda.synchronize()
    assert bool((jd == -7).all()) and bool((stats == -7).all()) and bool((disp == 0).all())
    assert L.amx_jacobian_det(pd, 4, 5, 6, 1, pj, None, None, 0, st) == 0                              # the field alone needs no scratch
    torch.cuda.synchronize()
    assert bool((jd == 1).all())
