"""Generates tests/golden/solver_golden.npz by running the REFERENCE's coupled_convex, inverse_consistency and
run_stage1_registration in fp32 on the CPU, on seeded inputs.  Run on the build machine only:
    python tools/make_golden_solver.py

Same mechanism as oracle/make_golden_registration.py: ``anatomix.registration`` cannot be imported (its __init__ pulls
MONAI / nibabel), so the two reference files are parsed with ``ast`` and ONLY the function definitions needed are compiled
in memory and called.  Nothing of the reference is written into this repository; the fixture holds outputs only.
``.cuda()`` is shimmed to the identity.  The reference's GPU caller builds its mesh with ``.half()``; its functions are
dtype-generic, so the fixtures are taken with ``.half()`` shimmed to ``.float()`` -- the reference's own arithmetic without
the half rounding -- and, where this torch can run it on the CPU, the half variant is recorded as ``...|half`` entries that
document how far the reference's half caller sits from its fp32 self (not a test target).

For every coupled_convex case the generator asserts the conditions the GPU test relies on: the restatement
(tests/_solver_ref.py) against the reference's fp32 output disagrees on at most 27 x (near-tie share) of the voxels and
never on more than 1 %; both shares are stored.  On the rolled case it asserts the known-answer figures for the
reference's own output.
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _solver_ref as SR                                   # noqa: E402

# where the reference checkout lives (the location oracle/make_golden_registration.py uses, unless overridden)
REF = os.path.join(os.environ.get("ANATOMIX_REFERENCE", "/root/reference"), "anatomix", "registration")
HALF = {"on": False}


def reference_functions():
    torch.Tensor.cuda = lambda self, *a, **k: self          # noqa: E731  generator-only shims
    real_half = torch.Tensor.half
    torch.Tensor.half = lambda self, *a, **k: real_half(self) if HALF["on"] else self.float()   # noqa: E731
    ns = {"torch": torch, "F": F, "np": np}
    wanted = {"convex_adam_utils.py": {"apply_avg_pool3d", "correlate", "coupled_convex", "inverse_consistency"},
              "instance_optimization.py": {"run_stage1_registration"}}
    for fname, names in wanted.items():
        tree = ast.parse(open(os.path.join(REF, fname)).read())
        body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
        assert {n.name for n in body} == names, (fname, names)
        exec(compile(ast.Module(body=body, type_ignores=[]), os.path.join(REF, fname), "exec"), ns)
    return ns


def ref_mesh(hw, dtype=torch.float32):
    k = 2 * hw + 1
    return F.affine_grid(hw * torch.eye(3, 4).unsqueeze(0), (1, 1, k, k, k), align_corners=True).permute(0, 4, 1, 2, 3) \
        .reshape(3, -1, 1).to(dtype)


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def main():
    torch.set_num_threads(8)
    ref = reference_functions()
    out = {}
    for case in SR.case_names():
        fix, mov, hw, g, sizes = SR.features(case)
        h, w, d = fix.shape[1:]
        # the label order, and the integer values up to the rounding of affine_grid's linspace (disp_hw = 3: 1 ulp off)
        assert np.abs(SR.mesh(hw) - ref_mesh(hw).reshape(3, -1).numpy()).max() < 1e-6, "label order / mesh values"
        # -- coupled_convex, both directions, from the correlation volume all sides share
        for tag, rev in (("fwd", False), ("bwd", True)):
            ssd, amin, _, _, _ = SR.ssd_of(case, rev)
            keep = ssd.copy()
            with torch.no_grad():
                soft = ref["coupled_convex"](tt(ssd.copy()), tt(amin), ref_mesh(hw), g, sizes)[0].numpy()
            mine, aux = SR.coupled_convex(keep, amin)
            near, dis = SR.near_tie_share(aux["margins"]), SR.disagree_share(mine, soft)
            print(f"{case}|{tag}: grid {h}x{w}x{d} hw {hw}  near-tie share {near:.3e}  restatement-vs-reference disagree {dis:.3e}"
                  f"  max|s| {np.abs(soft).max():.4f}")
            assert dis <= 27 * near and dis <= 0.01, (case, tag, near, dis)
            q = np.rint(soft * 27).astype(np.int8)                    # |27 s| <= 27 disp_hw <= 81
            assert np.abs(q / np.float32(27) - soft).max() < 1e-5       # box3 of integers: multiples of 1/27
            out[f"{case}|{tag}|soft_x27"] = q
            out[f"{case}|{tag}|near_tie_share"] = np.float64(near)
            out[f"{case}|{tag}|ref_disagree"] = np.float64(dis)
            if tag == "fwd":
                try:
                    HALF["on"] = True
                    with torch.no_grad():
                        sh = ref["coupled_convex"](tt(ssd.copy()), tt(amin), ref_mesh(hw, torch.float16), g, sizes)[0].float().numpy()
                    print(f"    half-mesh caller vs fp32: disagree {SR.disagree_share(sh, soft):.3e}, max abs {np.abs(sh - soft).max():.3e}")
                    out[f"{case}|fwd|soft|half"] = sh.astype(np.float16)
                except Exception as e:                                   # noqa: BLE001
                    print("    half variant not runnable on this CPU build:", type(e).__name__, str(e)[:80])
                finally:
                    HALF["on"] = False
        # -- run_stage1_registration, both branches (the reference's own correlate inside)
        with torch.no_grad():
            s1 = ref["run_stage1_registration"](tt(fix)[None], tt(mov)[None], hw, g, sizes, fix.shape[0], False)[0].numpy()
            hr = ref["run_stage1_registration"](tt(fix)[None], tt(mov)[None], hw, g, sizes, fix.shape[0], True)[0].numpy()
            hr_rev = ref["run_stage1_registration"](tt(mov)[None], tt(fix)[None], hw, g, sizes, fix.shape[0], True)[0].numpy()
        assert hr.shape == (3,) + tuple(sizes) and hr.dtype == np.float32
        mine_s1 = SR.run_stage1(fix, mov, hw, g, sizes, False)
        mine_hr = SR.run_stage1(fix, mov, hw, g, sizes, True)
        dis1 = SR.disagree_share(mine_s1, s1)
        e_hr = float(np.abs(mine_hr - hr).max() / np.abs(hr).max())
        print(f"{case}|stage1: ic=False disagree {dis1:.3e}; ic=True restatement-vs-reference rel max {e_hr:.3e}")
        out[f"{case}|stage1|soft_x27"] = np.rint(s1 * 27).astype(np.int8)
        out[f"{case}|stage1|ref_disagree"] = np.float64(dis1)
        rs = np.random.RandomState(17)
        idx = rs.randint(0, hr.size, 4096).astype(np.int32)
        out[f"{case}|stage1_ic|idx"], out[f"{case}|stage1_ic|val"] = idx, hr.reshape(-1)[idx]
        if hr.size <= 1 << 15:
            out[f"{case}|stage1_ic|full"] = hr
        if case == "roll48":
            roll = np.array(SR.ROLL, np.float32)[:, None, None, None]
            inner = (slice(None), slice(4, -4), slice(4, -4), slice(4, -4))
            ok = (np.abs(s1 - roll)[inner] <= 0.05).all(0).mean()
            G = 4 * g
            innerH = (slice(None), slice(G, -G), slice(G, -G), slice(G, -G))
            e_up = np.abs(hr - g * roll)[innerH].max()
            e_anti = np.abs(hr + hr_rev)[innerH].max()
            print(f"    known answer: within 0.05 of the roll on {ok:.5f} of the interior; ic=True |hr - g*roll| max {e_up:.4f}, "
                  f"|run(f,m) + run(m,f)| max {e_anti:.4f}")
            assert ok >= 0.99 and e_up <= 0.1 and e_anti <= 0.1, "lower ROLL_NOISE in tests/_solver_ref.py"
        # -- inverse_consistency and the resize on their own (continuous)
        a, b = SR.smooth_fields((h, w, d), 7, 6.0 / max(h, w, d))
        for it in (1, 15):
            with torch.no_grad():
                ra, rb = ref["inverse_consistency"](tt(a)[None], tt(b)[None], iterations=it)
            ma, mb = SR.inverse_consistency(a, b, it)
            e = max(np.abs(ma - ra[0].numpy()).max(), np.abs(mb - rb[0].numpy()).max()) / np.abs(ra.numpy()).max()
            print(f"{case}|ic{it}: restatement-vs-reference rel max {e:.3e}")
            for nm, arr in (("a", ra[0].numpy()), ("b", rb[0].numpy())):
                idx = rs.randint(0, arr.size, 1024).astype(np.int32)
                out[f"{case}|ic{it}|{nm}|idx"], out[f"{case}|ic{it}|{nm}|val"] = idx, arr.reshape(-1)[idx]
                if arr.size <= 1 << 14:
                    out[f"{case}|ic{it}|{nm}|full"] = arr
        scale = np.array([h - 1, w - 1, d - 1], np.float32) / 2 * g
        for nm, size in (("up", tuple(sizes)), ("odd", (h + 3, 2 * w - 1, d - 2))):
            with torch.no_grad():
                r = F.interpolate(tt(a)[None].flip(1) * tt(scale).view(1, 3, 1, 1, 1), size=size, mode="trilinear",
                                  align_corners=False)[0].numpy()
            mres = SR.resize_trilinear(a, size, scale, flip=True)
            print(f"{case}|resize_{nm} {size}: restatement-vs-reference rel max {np.abs(mres - r).max() / np.abs(r).max():.3e}")
            idx = rs.randint(0, r.size, 1024).astype(np.int32)
            out[f"{case}|resize_{nm}|idx"], out[f"{case}|resize_{nm}|val"] = idx, r.reshape(-1)[idx]
    path = os.path.join(ROOT, "tests", "golden", "solver_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
