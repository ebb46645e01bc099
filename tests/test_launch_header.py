"""The shared headers declare only what is shared.

``amx_launch.h`` and ``amx_gemm.h`` exist for the host functions that one ``.hip`` file defines and ANOTHER calls.  A launcher that
only its own file calls is ``static`` there and has no declaration (csrc/README.md states the rule).  Plain text matching on the
project's own sources: every function declared in the two headers must be named, as a whole word, in at least two ``csrc/*.hip``
files.  ``inline`` and ``template`` definitions are not declarations and are not collected.
"""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anatomix_amd", "csrc")
HEADERS = ("amx_launch.h", "amx_gemm.h")
DECLARATION = re.compile(r"^(?:hipError_t|size_t|int|bool|void)\s+(\w+)\s*\(", re.M)


def test_every_declared_function_is_used_by_two_files():
    # the whole words of each unit, comments and strings included
    units = {os.path.basename(p): set(re.findall(r"\w+", open(p).read())) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}
    assert len(units) > 20
    declared = [(h, name) for h in HEADERS for name in DECLARATION.findall(open(os.path.join(CSRC, h)).read())]
    assert len(declared) > 50 and ("amx_launch.h", "launch_conv") in declared and ("amx_gemm.h", "launch_gemm") in declared
    stale = []
    for header, name in declared:
        users = [unit for unit, words in units.items() if name in words]
        if len(users) < 2:
            stale.append("%s: %s (named only in %s)" % (header, name, ", ".join(users) or "no file"))
    assert not stale, "declared in a shared header but used by fewer than two .hip files:\n  " + "\n  ".join(stale)
