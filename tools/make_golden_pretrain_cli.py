"""Generates tests/golden/pretrain_cli.json from the REFERENCE's pretraining launcher and trainer options.  Run on the build machine
only:
    python tools/make_golden_pretrain_cli.py

Same mechanism as tools/make_golden_segtrain.py: the reference's files cannot be imported (they pull their whole package), so they
are parsed with ``ast`` and only parser-building statements are executed -- ``add_argument`` / ``set_defaults`` calls, assignments
to ``parser`` and returns; never ``parse_args`` / ``parse_known_args``, never the launcher's ``main``.  What is recorded:

  flags, exclusive_groups   the launcher's parser (scripts/pretrain_anatomix.py ``__main__`` with options/primus_options.py), per flag
                            its option strings, dest, default, required, type name, nargs, action and help
  passed                    the trainer flags the launcher's command line carries (the "--x" constants of its ``main``)
  trainer_defaults          dest -> default of the trainer's parser: BaseOptions.initialize, TrainOptions.initialize and
                            SupCLModel.modify_commandline_options applied in that order

Nothing of the reference's text is written into this repository; the fixture holds what the parser objects report."""
import argparse
import ast
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _segaug_ref as AR                                    # noqa: E402

REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "pretraining")


def _tree(*parts):
    path = os.path.join(REF, *parts)
    return path, ast.parse(open(path).read())


def _function(body, name):
    fn = [n for n in body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(fn) == 1, name
    return fn[0]


def _class(tree, name):
    cl = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(cl) == 1, name
    return cl[0]


def _exec(path, nodes, ns):
    mod = ast.Module(body=list(nodes), type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, path, "exec"), ns)
    return ns


def _parser_statements(fn):
    """``fn`` reduced to what builds the parser: parser.add_argument / parser.set_defaults calls, ``parser = ...`` and returns."""
    keep = []
    for st in fn.body:
        if isinstance(st, ast.Expr) and isinstance(st.value, ast.Call) and isinstance(st.value.func, ast.Attribute) and \
                st.value.func.attr in ("add_argument", "set_defaults"):
            keep.append(st)
        elif isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Name) and st.targets[0].id == "parser" \
                and "parse_known_args" not in ast.dump(st):
            keep.append(st)
        elif isinstance(st, ast.Return):
            keep.append(st)
    out = ast.FunctionDef(name=fn.name, args=fn.args, body=keep, decorator_list=[], returns=None, type_comment=None)
    if sys.version_info >= (3, 12):
        out.type_params = []
    return out


def _namespace():
    """str2bool of util/util.py and the two functions of options/primus_options.py, as the option modules see them."""
    path, tree = _tree("util", "util.py")
    util = _exec(path, [_function(tree.body, "str2bool")], {"argparse": argparse})

    class Util:
        str2bool = staticmethod(util["str2bool"])
    path, tree = _tree("options", "primus_options.py")
    ns = {"argparse": argparse, "util": Util}
    _exec(path, [_function(tree.body, "primus_out_norm_mode"), _function(tree.body, "add_primus_arguments")], ns)
    return ns


def launcher_parser(ns):
    path, tree = _tree("scripts", "pretrain_anatomix.py")
    main = [n for n in tree.body if isinstance(n, ast.If) and "__main__" in ast.dump(n.test)]
    assert len(main) == 1
    keep = []
    for st in main[0].body:
        src = ast.dump(st)
        if "parse_args" in src or "id='main'" in src:
            continue
        assert isinstance(st, (ast.Assign, ast.Expr)), src[:80]
        keep.append(st)
    ns = dict(ns)
    _exec(path, keep, ns)
    passed = [c.value[2:] for c in ast.walk(_function(tree.body, "main")) if isinstance(c, ast.Constant) and isinstance(c.value, str)
              and c.value.startswith("--")]
    return ns["parser"], passed


def trainer_parser(ns):
    ns = dict(ns)
    path, tree = _tree("options", "base_options.py")
    _exec(path, [_parser_statements(_function(_class(tree, "BaseOptions").body, "initialize"))], ns)
    base = ns.pop("initialize")

    class BaseOptions:
        initialize = staticmethod(base)
    ns["BaseOptions"] = BaseOptions
    path, tree = _tree("options", "train_options.py")
    _exec(path, [_parser_statements(_function(_class(tree, "TrainOptions").body, "initialize"))], ns)
    train = ns.pop("initialize")
    path, tree = _tree("models", "supcl_model.py")
    _exec(path, [_parser_statements(_function(_class(tree, "SupCLModel").body, "modify_commandline_options"))], ns)
    parser = argparse.ArgumentParser()
    parser = train(None, parser)
    return ns["modify_commandline_options"](parser, True)


def main():
    ns = _namespace()
    parser, passed = launcher_parser(ns)
    desc = AR.describe_parser(parser)
    trainer = trainer_parser(ns)
    desc["passed"] = passed
    desc["trainer_defaults"] = {a.dest: trainer.get_default(a.dest) for a in trainer._actions if not isinstance(a, argparse._HelpAction)}
    path = os.path.join(ROOT, "tests", "golden", "pretrain_cli.json")
    with open(path, "w") as f:
        json.dump(desc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes,", len(desc["flags"]), "flags,", len(desc["trainer_defaults"]), "trainer options")
    assert os.path.getsize(path) < 1000000
    # this package's parser and defaults against what was just recorded
    from anatomix_amd.pretraining.pretrain_anatomix import EXTRA_FLAGS, TRAINER_DEFAULTS, build_parser
    mine = AR.describe_parser(build_parser())
    n = len(desc["flags"])
    assert mine["flags"][:n] == desc["flags"], [(a, b) for a, b in zip(mine["flags"], desc["flags"]) if a != b][:1]
    assert mine["exclusive_groups"] == desc["exclusive_groups"]
    assert [f["dest"] for f in mine["flags"][n:]] == list(EXTRA_FLAGS)
    for k, v in TRAINER_DEFAULTS.items():
        assert desc["trainer_defaults"][k] == v, (k, v, desc["trainer_defaults"][k])
    assert set(desc["trainer_defaults"]) == set(TRAINER_DEFAULTS) | set(passed), \
        set(desc["trainer_defaults"]) ^ (set(TRAINER_DEFAULTS) | set(passed))


if __name__ == "__main__":
    main()
