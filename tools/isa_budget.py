#!/usr/bin/env python3
"""Instruction budget of the kernels of one .hip file, from its gfx950 assembly (no GPU needed).

    python tools/isa_budget.py anatomix_amd/csrc/amx_conv3d_zmarch.hip [more.hip ...] [--json]

Compiles each file with the Makefile's flags (`hipcc --offload-arch=gfx950 -O3 -std=c++17 -S`, device side only) and prints one row
per kernel instance and outermost loop that contains MFMAs -- for the z-march kernels that loop is one z-step of one wave:
  * from the code-object metadata: .vgpr_count, .vgpr_spill_count, .private_segment_fixed_size (scratch bytes per lane);
  * for the loop: the number of MFMAs and of the other instructions by class.
Instructions are classified by mnemonic prefix only (v_mfma, other v_, s_, ds_, global_, scratch_, the rest); counts are static
(every block of the loop once; `non-mfma` is their sum without the MFMAs).  step-min / step-max: the non-MFMA instructions on the
cheapest and the dearest way once round the loop, from the branch structure -- bounds of what one step executes when a loop holds
alternative paths (a fast and a guarded epilogue); compiler-made flag-and-branch chains let step-max count paths no step takes.
A size report: `profiles/r07_isa_budget_*.txt` hold its output before and after the
epilogue work, and tests/test_isa_budget.py compares a fresh run with them.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]      # csrc/Makefile CXXFLAGS
CLASSES = ["mfma", "valu", "salu", "lds", "global", "scr", "other"]

_LABEL = re.compile(r"^(\.LBB\d+_\d+):")
_HEADER = re.compile(r"Loop Header: Depth=1\b")
_IN_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=1\b")
_INSN = re.compile(r"^\t([a-z][a-z0-9_]+)")


def classify(mnemonic):
    if mnemonic.startswith("v_mfma") or mnemonic.startswith("v_smfma"):
        return "mfma"
    for prefix, cls in (("v_", "valu"), ("s_", "salu"), ("ds_", "lds"), ("global_", "global"), ("scratch_", "scr")):
        if mnemonic.startswith(prefix):
            return cls
    return "other"


def compile_asm(path):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.abspath(path)], check=True, cwd=os.path.dirname(os.path.abspath(path)),
                       stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read().splitlines()


def demangle(names):
    """Readable instance names from the Itanium symbols of amx:: kernel templates whose arguments are the storage type, ints and bools
    (the platform's c++filt does not know the 16-bit float types); any other symbol is kept as it is."""
    short = {}
    for sym in names:
        short[sym] = sym
        m = re.match(r"^_ZN3amx(\d+)", sym)
        if not m:
            continue
        start = m.end()
        name, rest = sym[start:start + int(m.group(1))], sym[start + int(m.group(1)):]
        if not rest.startswith("I"):
            short[sym] = name
            continue
        args = []
        for t in re.finditer(r"(DF16_)|(DF16b)|Li(\d+)E|Lb([01])E|(EE)", rest[1:]):
            if t.group(5):
                break
            args.append("f16" if t.group(1) else "bf16" if t.group(2) else t.group(3) if t.group(3) is not None else ("false", "true")[int(t.group(4))])
        short[sym] = "%s<%s>" % (name, ",".join(args))
    return short


def metadata(lines):
    """kernel symbol -> {vgpr_count, vgpr_spill_count, private_segment_fixed_size} from the .amdgpu_metadata document."""
    meta, cur = {}, None
    inside = False
    for ln in lines:
        if ln.strip() == ".amdgpu_metadata":
            inside = True
        elif ln.strip() == ".end_amdgpu_metadata":
            inside = False
        if not inside:
            continue
        if ln.startswith("  - "):
            cur = {}
            ln = "    " + ln[4:]
        m = re.match(r"^    \.(name|vgpr_count|vgpr_spill_count|private_segment_fixed_size|agpr_count|sgpr_count):\s+(\S+)", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    return meta


_BB = re.compile(r"^; %bb\.\d+:")
_BRANCH = re.compile(r"^\t(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)")


def loops_of(body):
    """Outermost loops of one function body: [(header, {class: count}, shortest, longest)] in program order.  A depth-1 loop is every
    basic block that names its header (as its own loop or as the parent of a nested one), plus the header block itself.  shortest /
    longest: the non-MFMA instructions on the cheapest and on the dearest way once round the loop (header back to header; inner
    loops -- the flag polls -- taken once), i.e. the bounds of what one step executes, where the class counts are static."""
    blocks, cur = [], {"label": None, "loop": None, "insns": [], "succ": [], "fall": True}

    # an inner loop's header names its depth-1 parent; the blocks of the inner loop name only the inner header
    parent_of, last = {}, None
    for ln in body:
        m = _LABEL.match(ln)
        if m:
            last = m.group(1)[2:]
        elif _INSN.match(ln):
            last = None
        mm = _PARENT.search(ln)
        if mm and last:
            parent_of.setdefault(last, mm.group(1))

    def start(label, line):
        nonlocal cur
        blocks.append(cur)
        loop = label if (label and _HEADER.search(line)) else None
        mm = _IN_LOOP.search(line)
        if mm:
            loop = mm.group(1) if mm.group(2) == "1" else parent_of.get(mm.group(1))
        elif _PARENT.search(line):
            loop = _PARENT.search(line).group(1)
        cur = {"label": label, "loop": loop, "insns": [], "succ": [], "fall": True, "pending": True}

    for ln in body:
        m = _LABEL.match(ln)
        if m:
            start(m.group(1)[2:], ln)
            continue
        if _BB.match(ln):
            start(None, ln)
            continue
        if ln.startswith(";") and cur.get("pending") and cur["loop"] is None:     # a nested block's comment continues on the next lines
            mm = _PARENT.search(ln)
            if mm:
                cur["loop"] = mm.group(1)
            continue
        m = _INSN.match(ln)
        if not m:
            continue
        cur["pending"] = False
        cur["insns"].append(m.group(1))
        br = _BRANCH.match(ln)
        if br or m.group(1) == "s_endpgm":
            if br:
                cur["succ"].append(br.group(2)[2:])
            if m.group(1) in ("s_branch", "s_endpgm"):
                cur["fall"] = False
            loop = cur["loop"]
            start(None, "")                                                        # the rest is a block of its own, in the same loop
            cur["loop"] = loop
    blocks.append(cur)
    by_label = {b["label"]: i for i, b in enumerate(blocks) if b["label"]}
    order, counts, members = [], {}, {}
    for i, b in enumerate(blocks):
        if b["loop"] is None:
            continue
        if b["loop"] not in counts:
            order.append(b["loop"])
            counts[b["loop"]] = dict.fromkeys(CLASSES, 0)
            members[b["loop"]] = set()
        members[b["loop"]].add(i)
        for ins in b["insns"]:
            counts[b["loop"]][classify(ins)] += 1

    def succ(i):
        out = [by_label[t] for t in blocks[i]["succ"] if t in by_label]
        if blocks[i]["fall"] and i + 1 < len(blocks):
            out.append(i + 1)
        return out

    def round_trip(h):
        head = by_label.get(h)
        if head is None:
            return -1, -1
        cost = lambda i: sum(1 for ins in blocks[i]["insns"] if classify(ins) != "mfma")
        memo, onstack = {}, set()

        def go(i):                       # (cheapest, dearest) way from block i back to the header, None when there is none
            if i in memo:
                return memo[i]
            onstack.add(i)
            best = None
            for j in succ(i):
                if j == head:
                    r = (0, 0)
                elif j not in members[h] or j in onstack:
                    continue
                else:
                    r = go(j)
                if r is not None:
                    best = r if best is None else (min(best[0], r[0]), max(best[1], r[1]))
            onstack.discard(i)
            memo[i] = None if best is None else (best[0] + cost(i), best[1] + cost(i))
            return memo[i]

        sys.setrecursionlimit(max(10000, sys.getrecursionlimit()))
        r = go(head)
        return r if r else (-1, -1)

    return [(h, counts[h]) + round_trip(h) for h in order]


def budget(path):
    lines = compile_asm(path)
    meta = metadata(lines)
    names = demangle(sorted(meta))
    rows = []
    i = 0
    while i < len(lines):
        m = re.match(r"^(\w+):\s*(;.*)?$", lines[i])
        if not m or m.group(1) not in meta:
            i += 1
            continue
        sym = m.group(1)
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        md = meta[sym]
        k = 0
        for header, c, lo, hi in loops_of(lines[i + 1:j]):
            if not c["mfma"]:
                continue
            rows.append(dict(file=os.path.basename(path), kernel=names[sym], loop=k, vgpr=int(md.get("vgpr_count", -1)),
                             spill=int(md.get("vgpr_spill_count", -1)), scratch_bytes=int(md.get("private_segment_fixed_size", -1)),
                             non_mfma=sum(v for q, v in c.items() if q != "mfma"), step_min=lo, step_max=hi, **c))
            k += 1
        i = j
    return rows


COLUMNS = ["vgpr", "spill", "scratch_bytes", "loop", "mfma", "valu", "salu", "lds", "global", "scr", "other", "non_mfma", "step_min", "step_max"]


def render(rows):
    fmt = "%-5s %-5s %-7s %-4s | %5s %5s %5s %5s %6s %5s %5s %8s %8s %8s | %s"
    out = [fmt % ("vgpr", "spill", "scratch", "loop", "mfma", "valu", "salu", "lds", "global", "scr", "other", "non-mfma", "step-min", "step-max",
                  "kernel")]
    out += [fmt % (tuple(r[c] for c in COLUMNS) + (r["kernel"],)) for r in rows]
    return "\n".join(out)


def parse_table(text):
    """The rows of a rendered table (a committed profiles/r07_isa_budget_*.txt) back as dicts."""
    rows = []
    for ln in text.splitlines():
        parts = ln.split("|")
        nums = " ".join(parts[:2]).split() if len(parts) == 3 else []
        if len(nums) == len(COLUMNS) and all(re.fullmatch(r"-?\d+", x) for x in nums):
            rows.append(dict(zip(COLUMNS, (int(x) for x in nums)), kernel=parts[2].strip()))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("files", nargs="+")
    ap.add_argument("--json", action="store_true", help="one JSON list instead of the table")
    args = ap.parse_args()
    rows = [r for f in args.files for r in budget(f)]
    print(json.dumps(rows, indent=1) if args.json else render(rows))


if __name__ == "__main__":
    sys.exit(main())
