"""Generates tests/golden/regmetrics_golden.npz and tests/golden/regdriver_cli.json from the REFERENCE, on the seeded inputs of
tests/_regmetrics_ref.py.  Run on the build machine only:
    python tools/make_golden_regmetrics.py

Same mechanism as tools/make_golden_instopt.py: ``anatomix.registration`` cannot be imported (its __init__ pulls MONAI /
nibabel), so the reference's files are parsed with ``ast``.  From convex_adam_utils.py ONLY generate_grid and JacobianDet are
compiled in memory and called.  From the driver only the statements of its ``__main__`` block that build the parser (assignments
and ``add_argument`` calls; not ``parse_args``, not the call of ``convex_adam``) are executed, and the resulting parser object is
read: per flag its option strings, dest, default, required, type name and nargs, plus the exclusive groups.  Nothing of the
reference is written into this repository; the fixtures hold outputs only:
  * generate_grid for two shapes;
  * per Jacobian case (shape x smooth/fold x add_identity) the reference's fp32 determinants (the full field up to 2^15
    elements, otherwise 4096 seeded indices), ``ref_vs_f64`` = max |reference fp32 - float64 restatement| / max |reference|,
    the float64 statistics and the float64 count of non-positive determinants;
  * per Dice case the value of sklearn.metrics.f1_score called exactly as the driver calls it.

The generator asserts what the tests rely on:
  * the fp32 restatement equals the reference bit for bit, and the restated generate_grid equals the reference's;
  * every case meant to fold has non-positive determinants in float64, every smooth case has none;
  * the count-based Dice restatement equals sklearn's value to 1e-12.
"""
import argparse
import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _regmetrics_ref as MR                                # noqa: E402

REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "anatomix", "registration")


def reference_functions():
    ns = {"torch": torch, "np": np}
    path = os.path.join(REF, "convex_adam_utils.py")
    names = {"generate_grid", "JacobianDet"}
    body = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == names
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns


def reference_parser():
    """The parser object the reference's ``__main__`` block builds, without parsing anything and without calling the driver."""
    path = os.path.join(REF, "run_convex_adam_with_network_feats.py")
    main = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.If) and "__main__" in ast.dump(n.test)]
    assert len(main) == 1
    keep = []
    for st in main[0].body:
        src = ast.dump(st)
        if "parse_args" in src or "convex_adam" in src:
            continue
        assert isinstance(st, (ast.Assign, ast.Expr)), ast.dump(st)[:80]
        keep.append(st)
    ns = {"argparse": argparse}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["parser"]


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(a, np.float64)).max())


def main():
    from sklearn.metrics import f1_score
    ref = reference_functions()
    out = {}
    for shape in MR.GRID_SHAPES:
        g = ref["generate_grid"](shape)
        assert g.dtype == MR.generate_grid(shape).dtype and np.array_equal(g, MR.generate_grid(shape)), shape
        out["grid|{}x{}x{}".format(*shape)] = g
    for shape, kind in MR.jac_cases():
        disp = MR.jac_field(shape, kind)
        for ident in (0, 1):
            y, grid = MR.reference_inputs(disp, ident)
            if ident:
                assert np.array_equal(grid[0].numpy(), ref["generate_grid"](shape).astype(np.float32))
            r = ref["JacobianDet"](y, grid)[0].numpy()
            mine = MR.jacobian_det(y, grid)[0].numpy()
            assert r.dtype == np.float32 and r.shape == tuple(s - 1 for s in shape)
            assert np.array_equal(r, mine), (shape, kind, ident, "the fp32 restatement is not the reference bit for bit")
            j64 = MR.jacobian_f64(disp, ident)
            key = MR.jac_key(shape, kind, ident)
            if r.size <= MR.FULL_MAX:
                out[key + "|full"] = r
            else:
                idx = np.random.RandomState(17).randint(0, r.size, 4096)
                out[key + "|idx"], out[key + "|val"] = idx.astype(np.int64), r.reshape(-1)[idx]
            e = rel(r, j64)
            nonpos = int((j64 <= 0).sum())
            out[key + "|ref_vs_f64"] = np.float64(e)
            out[key + "|stats64"] = MR.jacobian_stats(j64)
            out[key + "|nonpos64"] = np.int64(nonpos)
            print(f"{key}: ref_vs_f64 {e:.3e}  max|ref| {np.abs(r).max():.4f}  non-positive {nonpos} / {r.size}")
            if ident:
                assert (nonpos > 0) == (kind == "fold"), (key, nonpos)
    for case in MR.DICE_CASES:
        fix, mov = MR.dice_pair(case)
        want = f1_score(fix.flatten(), mov.flatten(), average='macro', labels=np.unique(fix).astype(int).tolist()[1:])
        counts, bad = MR.overlap_counts(fix, mov, 1024)
        got, per = MR.dice_from_counts(counts)
        print(f"dice|{case}: sklearn {want:.15f}  from counts {got:.15f}  labels {sorted(per)}")
        assert bad == 0 and abs(got - want) <= 1e-12, (case, got, want)
        out["dice|" + case] = np.float64(want)
    path = os.path.join(ROOT, "tests", "golden", "regmetrics_golden.npz")
    np.savez_compressed(path, **out)
    cli = os.path.join(ROOT, "tests", "golden", "regdriver_cli.json")
    with open(cli, "w") as f:
        json.dump(MR.describe_parser(reference_parser()), f, indent=1, sort_keys=True)
        f.write("\n")
    for p in (path, cli):
        print("wrote", p, os.path.getsize(p), "bytes")
        assert os.path.getsize(p) < 1000000
    # this package's parser against what was just recorded
    from anatomix_amd.registration.run_convex_adam_with_network_feats import build_parser
    assert MR.describe_parser(build_parser()) == json.load(open(cli))


if __name__ == "__main__":
    main()
