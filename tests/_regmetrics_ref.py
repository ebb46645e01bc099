"""Restatement of the reference's Jacobian utilities (anatomix/registration/convex_adam_utils.py:226-282) and of the Dice score
its driver prints (run_convex_adam_with_network_feats.py:283-295), with the seeded inputs of the fixtures
tests/golden/regmetrics_golden.npz.  tools/make_golden_regmetrics.py asserts that the fp32 restatement equals the reference bit
for bit and that the count-based Dice equals sklearn's f1_score; the tests hold the kernels to the float64 restatement."""
import argparse

import numpy as np
import torch

GRID_SHAPES = ((2, 3, 4), (5, 4, 7))

# Jacobian cases: shape of the displacement field, and whether it is smooth (no folding) or folds.  The last two shapes have an
# extent D that is a multiple of 4: the kernel's 16-byte path; the others take its scalar path.
JAC_SHAPES = ((2, 2, 2), (5, 3, 2), (33, 17, 9), (9, 8, 130), (6, 5, 8), (7, 6, 132))
JAC_KINDS = ("smooth", "fold")
FULL_MAX = 1 << 15


def jac_cases():
    return [(s, k) for s in JAC_SHAPES for k in JAC_KINDS]


def jac_key(shape, kind, add_identity):
    return "jac|{}x{}x{}|{}|id{}".format(*shape, kind, int(add_identity))


def jac_field(shape, kind):
    """Displacement field [3, H, W, D] in voxels, channel a along axis a (float32, seeded by shape and kind).  smooth: one slow
    sine per channel, amplitude 0.4 voxels (determinants stay positive); fold: white noise of +-1.5 voxels."""
    H, W, D = shape
    rs = np.random.RandomState(1000 * H + 10 * W + D + (7 if kind == "fold" else 0))
    if kind == "fold":
        return ((rs.rand(3, H, W, D) - 0.5) * 3.0).astype(np.float32)
    i, j, k = np.meshgrid(np.arange(H), np.arange(W), np.arange(D), indexing="ij")
    out = np.empty((3, H, W, D), np.float32)
    for a in range(3):
        f, ph = rs.rand(3) * 0.6, rs.rand() * 6.28
        out[a] = 0.4 * np.sin(f[0] * i + f[1] * j + f[2] * k + ph)
    return out


def generate_grid(imgshape):
    """Component c of the grid is the index along axis 2 - c (int64, [H, W, D, 3])."""
    h, w, d = imgshape
    i, j, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(d), indexing="ij")
    return np.stack([k, j, i], axis=-1)


def jacobian_det(y_pred, sample_grid):
    """The reference's arithmetic, operation for operation, in the dtype of its arguments: [N, H, W, D, 3] -> [N, H-1, W-1, D-1]."""
    J = y_pred + sample_grid
    base = J[:, :-1, :-1, :-1, :]
    dy = J[:, 1:, :-1, :-1, :] - base
    dx = J[:, :-1, 1:, :-1, :] - base
    dz = J[:, :-1, :-1, 1:, :] - base
    d0 = dx[:, :, :, :, 0] * (dy[:, :, :, :, 1] * dz[:, :, :, :, 2] - dy[:, :, :, :, 2] * dz[:, :, :, :, 1])
    d1 = dx[:, :, :, :, 1] * (dy[:, :, :, :, 0] * dz[:, :, :, :, 2] - dy[:, :, :, :, 2] * dz[:, :, :, :, 0])
    d2 = dx[:, :, :, :, 2] * (dy[:, :, :, :, 0] * dz[:, :, :, :, 1] - dy[:, :, :, :, 1] * dz[:, :, :, :, 0])
    return d0 - d1 + d2


def reference_inputs(disp, add_identity, dtype=torch.float32):
    """(y_pred [1, H, W, D, 3], grid) of the reference's call for a field in axis order: the components flipped into the grid's
    order; with add_identity the grid of the volume, else zeros (the field is the map itself)."""
    y = torch.from_numpy(np.ascontiguousarray(disp)).to(dtype).permute(1, 2, 3, 0).flip(-1)[None]
    grid = torch.from_numpy(generate_grid(disp.shape[1:]))[None].to(dtype)
    return y, (grid if add_identity else torch.zeros_like(grid))


def jacobian_f64(disp, add_identity):
    y, g = reference_inputs(disp, add_identity, torch.float64)
    return jacobian_det(y, g)[0].numpy()


def jacobian_stats(J):
    """The six statistics in float64: share <= 0, min, max, mean, mean and population deviation of log J over the positive ones."""
    J = np.asarray(J, np.float64).reshape(-1)
    lg = np.log(J[J > 0])
    return np.array([(J <= 0).mean(), J.min(), J.max(), J.mean(), lg.mean() if lg.size else np.nan, lg.std() if lg.size > 1 else 0.0])


# ---- Dice -------------------------------------------------------------------------------------------------------------------
DICE_SHAPE = (24, 20, 18)
DICE_CASES = ("blocky", "no_zero", "sparse_labels", "absent_in_moved")


def _blocks(rs, labels, shape, cell):
    g = [-(-s // cell) for s in shape]
    coarse = rs.choice(labels, size=g)
    return np.kron(coarse, np.ones((cell,) * 3, dtype=coarse.dtype))[:shape[0], :shape[1], :shape[2]]


def dice_pair(case):
    """(fixed, moved) label maps as float64 volumes, what get_fdata() returns."""
    rs = np.random.RandomState(DICE_CASES.index(case) + 31)
    labels = {"blocky": [0, 1, 2, 3, 4, 5], "no_zero": [1, 2, 3, 4], "sparse_labels": [0, 3, 7, 200, 1023],
              "absent_in_moved": [0, 1, 2, 3]}[case]
    fixed = _blocks(rs, labels, DICE_SHAPE, 4)
    moved = np.roll(fixed, (1, -1, 2), (0, 1, 2))
    noise = rs.rand(*DICE_SHAPE) < 0.05
    moved = np.where(noise, rs.choice(labels, size=DICE_SHAPE), moved)
    if case == "absent_in_moved":
        moved = np.where(moved == 2, 9, moved)          # label 2 never found (score 0), label 9 only in the moved map
    return fixed.astype(np.float64), moved.astype(np.float64)


def overlap_counts(a, b, bins):
    """numpy: counts [bins, 3] and the number of bad voxels, as amx_label_overlap defines them."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)

    def ok(v):
        with np.errstate(invalid="ignore"):
            return (v >= 0) & (v < bins) & (v == np.floor(v))
    good = ok(a.astype(np.float64)) & ok(b.astype(np.float64))
    ia, ib = a[good].astype(np.int64), b[good].astype(np.int64)
    out = np.zeros((bins, 3), np.int64)
    out[:, 0] = np.bincount(ia, minlength=bins)
    out[:, 1] = np.bincount(ib, minlength=bins)
    out[:, 2] = np.bincount(ia[ia == ib], minlength=bins)
    return out, int((~good).sum())


def dice_from_counts(counts):
    labels = [l for l in range(counts.shape[0]) if counts[l, 0] > 0][1:]
    per = {l: 2.0 * float(counts[l, 2]) / float(counts[l, 0] + counts[l, 1]) for l in labels}
    return sum(per.values()) / len(per), per


# ---- command line ----------------------------------------------------------------------------------------------------------
def describe_parser(parser):
    """What the fixture regdriver_cli.json records of an argparse parser: every flag and the exclusive groups."""
    flags = []
    for a in parser._actions:
        if isinstance(a, argparse._HelpAction):
            continue
        flags.append({"option_strings": list(a.option_strings), "dest": a.dest, "default": a.default, "required": bool(a.required),
                      "type": None if a.type is None else a.type.__name__, "nargs": a.nargs, "action": type(a).__name__})
    groups = [{"required": bool(g.required), "dests": [a.dest for a in g._group_actions]} for g in parser._mutually_exclusive_groups]
    return {"flags": flags, "exclusive_groups": groups}
