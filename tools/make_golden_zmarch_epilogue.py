#!/usr/bin/env python3
"""Writes tests/golden/zmarch_epilogue_digests.json: SHA-256 digests of what the z-march family stores (and the range flags it
raises) for the seeded cases of tests/test_zmarch_epilogue_gpu.py (the case list and the input generators are that module's own).  Run it on an MI355X at the commit
whose outputs are the reference -- the test then demands bit identity with that commit:

    python tools/make_golden_zmarch_epilogue.py [--out FILE] [--lib-root DIR]

--lib-root: the checkout whose anatomix_amd package (and built library) computes the outputs; default: this checkout.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "zmarch_epilogue_digests.json"))
    ap.add_argument("--lib-root", default=ROOT)
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.lib_root), os.path.join(ROOT, "tests")]
    import torch
    import test_zmarch_epilogue_gpu as Z

    device = torch.device("cuda:0")
    out = dict(Z.all_entries(device))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %d entries to %s" % (len(out), args.out))


if __name__ == "__main__":
    main()
