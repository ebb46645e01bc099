"""Generates tests/golden/segtrain_cli.json from the REFERENCE's train_segmentation.py.  Run on the build machine only:
    python tools/make_golden_segtrain.py

Same mechanism as tools/make_golden_regmetrics.py: the reference's file cannot be imported (it pulls MONAI and TensorBoard), so it
is parsed with ``ast``.  Only the statements of its ``__main__`` block that build the parser (assignments and ``add_argument``
calls; not ``parse_args``, not the call of ``main``) are executed, and the resulting parser object is read: per flag its option
strings, dest, default, required, type name, nargs, action and help, plus the exclusive groups.  Nothing of the reference's text is
written into this repository; the fixture holds what the parser object reports."""
import argparse
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _segaug_ref as AR                                    # noqa: E402

REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "anatomix", "segmentation")


def reference_parser():
    path = os.path.join(REF, "train_segmentation.py")
    main = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.If) and "__main__" in ast.dump(n.test)]
    assert len(main) == 1
    keep = []
    for st in main[0].body:
        src = ast.dump(st)
        if "parse_args" in src or "id='main'" in src:
            continue
        assert isinstance(st, (ast.Assign, ast.Expr)), ast.dump(st)[:80]
        keep.append(st)
    ns = {"argparse": argparse}
    exec(compile(ast.Module(body=keep, type_ignores=[]), path, "exec"), ns)
    return ns["parser"]


def main():
    desc = AR.describe_parser(reference_parser())
    path = os.path.join(ROOT, "tests", "golden", "segtrain_cli.json")
    with open(path, "w") as f:
        json.dump(desc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes,", len(desc["flags"]), "flags")
    assert os.path.getsize(path) < 1000000
    # this package's parser against what was just recorded: the reference's flags first, in its order
    from anatomix_amd.segmentation.train_segmentation import build_parser
    mine = AR.describe_parser(build_parser())
    n = len(desc["flags"])
    assert mine["flags"][:n] == desc["flags"], [(a, b) for a, b in zip(mine["flags"], desc["flags"]) if a != b][:1]
    assert mine["exclusive_groups"] == desc["exclusive_groups"]
    assert [f["dest"] for f in mine["flags"][n:]] == ["seed", "out_dir", "no_augment"]


if __name__ == "__main__":
    main()
