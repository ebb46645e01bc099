"""Generates tests/golden/instopt_golden.npz by running the REFERENCE's create_warp / run_instance_opt in fp32 on the CPU, on
the seeded inputs of tests/_instopt_ref.py.  Run on the build machine only:
    python tools/make_golden_instopt.py

Same mechanism as tools/make_golden_solver.py: ``anatomix.registration`` cannot be imported (its __init__ pulls MONAI /
nibabel), so the two reference files are parsed with ``ast`` and ONLY apply_avg_pool3d, diffusion_regularizer, create_warp
and run_instance_opt are compiled in memory and called, with ``.cuda()`` shimmed to the identity.  Nothing of the reference
is written into this repository; the fixture holds outputs only: per (case, niter) the full field where it has at most 2^14
elements, otherwise its values at 4096 seeded indices (one index set per case), and ``ref_vs_f64`` = max |reference fp32 -
float64 restatement| / max |reference|.  (Full fields up to 2^15 elements, or the gradient-free niter = 1 run on every
case, would put the file above tests/golden/solver_golden.npz, which it has to stay below.)  For the teacher-forced single
iterations it holds ``e32``, the same distance for the gradient of one iteration started from the fp32 trajectory's state.
The warp entries are F.grid_sample as the reference's driver composes it (run_convex_adam_with_network_feats.py:238-266).

The generator asserts what the tests rely on:
  * the fp32 restatement equals the reference bit for bit, for every (case, niter) and both selected_smooth values;
  * ref_vs_f64 <= 1e-4 for every (case, niter) kept;
  * at least 25 % of the samples of the large-displacement case have a corner outside the volume;
  * in the nearest-mode warp at most 0.5 % of the voxels have a sample coordinate within 1e-4 of a half-integer.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _instopt_ref as IR                                   # noqa: E402

REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "anatomix", "registration")


def reference_functions():
    torch.Tensor.cuda = lambda self, *a, **k: self          # noqa: E731  generator-only shims
    nn.Module.cuda = lambda self, *a, **k: self             # noqa: E731
    ns = {"torch": torch, "F": F, "np": np, "nn": nn}
    wanted = {"convex_adam_utils.py": {"apply_avg_pool3d", "diffusion_regularizer"},
              "instance_optimization.py": {"create_warp", "run_instance_opt"}}
    for fname, names in wanted.items():
        tree = ast.parse(open(os.path.join(REF, fname)).read())
        body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert {n.name for n in body} == names, (fname, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), os.path.join(REF, fname), "exec"), ns)
    return ns


FULL_MAX = 1 << 14


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def store(out, key, arr, idx):
    if arr.size <= FULL_MAX:
        out[key + "|full"] = arr
    else:
        out[key + "|val"] = arr.reshape(-1)[idx]


def main():
    torch.set_num_threads(8)
    ref = reference_functions()
    out = {}
    for case in IR.case_names():
        H, W, D, g, c, amp = IR.CASES[case]
        disp, fix, mov = IR.inputs(case)
        sizes = (H, W, D)
        assert 3 * H * W * D < 1 << 16
        idx = np.random.RandomState(17).randint(0, 3 * H * W * D, 4096).astype(np.uint16)
        if 3 * H * W * D > FULL_MAX:
            out[f"{case}|idx"] = idx
        # create_warp: the restatement's initial weight is the reference's
        net = ref["create_warp"](IR.tt(disp)[None], sizes, g)
        w0 = IR.initial_weight(disp, g)
        assert isinstance(net, nn.Sequential) and torch.equal(net[0].weight.data, w0), case
        share = IR.out_of_range_share(IR.smooth3(w0)[0].numpy())
        print(f"{case}: grid {IR.grid_of(case)} c {c}  max|weight0| {float(w0.abs().max()):.3f} cells  out-of-range share {share:.3f}")
        out[f"{case}|out_of_range_share"] = np.float64(share)
        if case == "far":
            assert share >= 0.25, share
        runs = [(n, 0) for n in IR.NITERS[case]] + ([(IR.SMOOTH_NITER, 3), (IR.SMOOTH_NITER, 5)] if case == IR.SMOOTH_CASE else [])
        for niter, smooth in runs:
            r = ref["run_instance_opt"](IR.tt(disp)[None], IR.tt(fix)[None], IR.tt(mov)[None], g, IR.LAMBDA, sizes, niter, smooth,
                                        lr=IR.LR)[0].detach().numpy()
            mine, _ = IR.run(disp, fix, mov, g, IR.LAMBDA, niter, smooth)
            assert r.dtype == np.float32 and r.shape == (3, H, W, D)
            assert np.array_equal(r, mine), (case, niter, smooth, "the fp32 restatement is not the reference bit for bit")
            m64, _ = IR.run(disp, fix, mov, g, IR.LAMBDA, niter, smooth, dtype=torch.float64)
            e = rel(r, m64)
            print(f"  niter {niter:3d} smooth {smooth}: bit-identical restatement; ref_vs_f64 {e:.3e}  max|ref| {np.abs(r).max():.4f}")
            assert e <= 1e-4, (case, niter, smooth, e)
            key = f"{case}|n{niter}|s{smooth}"
            store(out, key, r, idx)
            out[key + "|ref_vs_f64"] = np.float64(e)
        if case in IR.NITER1_CASES:                               # niter = 1: gradient-free
            r1 = ref["run_instance_opt"](IR.tt(disp)[None], IR.tt(fix)[None], IR.tt(mov)[None], g, IR.LAMBDA, sizes, 1, 0,
                                         lr=IR.LR)[0].detach().numpy()
            assert np.array_equal(r1, IR.run(disp, fix, mov, g, IR.LAMBDA, 1, 0)[0])
            store(out, f"{case}|n1|s0", r1, idx)
        # teacher-forced single iterations from the fp32 trajectory's state: the fp32 gradient's own distance from float64
        _, tr = IR.run(disp, fix, mov, g, IR.LAMBDA, max(IR.TF_ITERS) + 1, 0, record=IR.TF_ITERS)
        pf, pm = IR.tt(IR.pooled(fix, g))[None], IR.tt(IR.pooled(mov, g))[None]
        for it in IR.TF_ITERS:
            g64 = IR.iteration(IR.tt(tr[it]["weight"]), pf, pm, IR.LAMBDA, torch.float64)[0].numpy()
            e32 = rel(tr[it]["grad"], g64)
            print(f"  iteration {it}: e32 of grad {e32:.3e}  max|grad| {np.abs(g64).max():.3e}  loss {tr[it]['loss']:.6f} reg {tr[it]['reg']:.6f}")
            out[f"{case}|it{it}|e32"] = np.float64(e32)
    # the driver's warp
    vol, lab, wd = IR.warp_inputs()
    out["warp|bilinear|full"] = IR.warp(vol, wd, "bilinear")
    out["warp|nearest|full"] = IR.warp(lab, wd, "nearest").astype(np.int8)
    near = float(IR.near_half_mask(wd).mean())
    print(f"warp {IR.WARP_SHAPE}: share of voxels within 1e-4 of a half-integer coordinate {near:.4%}; bilinear vs float64 "
          f"{rel(out['warp|bilinear|full'], IR.warp(vol, wd, 'bilinear', torch.float64)):.3e}")
    assert near <= 0.005, near
    out["warp|near_half_share"] = np.float64(near)
    path = os.path.join(ROOT, "tests", "golden", "instopt_golden.npz")
    np.savez_compressed(path, **out)
    size, lim = os.path.getsize(path), os.path.getsize(os.path.join(ROOT, "tests", "golden", "solver_golden.npz"))
    print("wrote", path, size, "bytes")
    assert size < lim, (size, lim)


if __name__ == "__main__":
    main()
