"""Bitwise A/B of two builds of libanatomix_amd.so.  Section ``streams``: the entries of the streaming units (segmentation loss, the
three augmentation units, registration metrics, instance optimisation, MIND-SSC / correlation) -- the proof that a refactor of their
shared helpers changed no summation order and no contraction.  Section ``unet``: the UNet forward (output, feature taps, encode_only,
sliding window by window batches and as one call, the kernel names of a profiled forward) on the shipped variants and on every
configuration tests/test_unet_gpu.py parametrises, and the single-layer conv entries, one shape per route of the conv dispatch -- the
proof that a refactor of the launch path moved no layer to another kernel and changed no launch.  Section ``vit``: the 3D ViT's forward
and both of its sliding-window routes on the cases of tests/test_vit_sliding_window_gpu.py.  Section ``train``: the training
function (model/train.py) over every configuration tests/test_train_step_gpu.py parametrises, the 6 M variant on both tap routes, and
eager / graphed contrastive steps with FusedAdamW -- the proof that a refactor of the Python side of the training path changed no
launch.  ``train_step`` is the step case alone, at ``--size``.

    python tools/ab_bitwise.py --old PATH/libanatomix_amd.so [--new PATH/libanatomix_amd.so] [--section streams|unet|vit|all]
    python tools/ab_bitwise.py --old-tree PATH --section train|train_step [--size 32]

``--old-tree PATH``: a directory holding another commit's ``anatomix_amd/``, ``oracle/`` and ``tests/`` (``git archive``); the old side's
child puts it first on ``sys.path`` and both sides load the SAME library (``--new``) unless ``--old`` names another.  The old side then
runs twice: a quantity that is not bit-stable on the old side alone is reported as such and held to the loosest tolerance of the
deterministic comparisons that cover it in the suite (1e-4 relative, test_graphed_contrastive_step_matches_eager_on_the_same_coordinates)
instead of bit for bit.  ``--expect-different REGEX`` names what the caller knows to differ (a path one tree repaired): those names are
counted in a line of their own and do not set the exit status.

One process uses one library (anatomix_amd/_lib.py reads AMX_LIB_PATH at import), so each side runs in a fresh child process of
its own (``--child``), one after the other and each under its own time limit.  A child runs every entry on seeded inputs and
prints one SHA-256 per output tensor; the two listings are compared here and THAT comparison sets the exit status: 0 identical,
1 different, 2 a child failed (the second one is then not started)."""
import argparse
import contextlib
import ctypes
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- child: one listing --------------------------------------------------------------------------------------------------

def unet_section(dev, emit, tree):
    """The 6 M variant and anatomix-dev in every precision they support (forward, taps, encode_only, both sliding-window routes), the
    other configurations of tests/test_unet_gpu.py -- between them every branch of the forward's conv plan -- and the single-layer
    entries on one shape per route."""
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    import _util as U              # run_conv / run_conv_merged: the tensor layouts of the single-layer entries
    import anatomix_amd
    from anatomix_amd.registration.sliding_window import sliding_window_inference, sliding_window_volume
    from oracle import unet_ref as R

    def emit_names(name, names):
        """Kernel names: one compared line each, and the whole list hashed like a tensor."""
        for i, k in enumerate(names):
            print(f"{name}[{i}] (text) {k}", flush=True)
        emit(name, torch.frombuffer(bytearray("\n".join(names).encode()), dtype=torch.uint8))

    # (variant, precisions, (forward shape, sliding-window volume) pairs, roi).  anatomix-dev at 64^3 runs its five levels at
    # W = 64, 32, 16, 8, 4: every row of the generic kernel's brick table.  Modules 2 / 5: inside / right behind the stem pair.
    nets = (("anatomix", ("f16", "bf16", "f16x2", "strict"), (((32, 32, 32), (32, 32, 48)), ((48, 64, 96), (48, 64, 96))), 32),
            ("anatomix-dev", ("f16", "bf16", "f16x2", "strict", "f16x2mx"), (((64, 64, 64), (64, 64, 96)),), 64))
    for variant, precisions, shapes, roi in nets:
        kw = R.VARIANTS[variant]
        with contextlib.redirect_stdout(sys.stderr):       # (the constructor prints its skip ids, as the reference does)
            m = anatomix_amd.Unet(**kw)
        m.load_state_dict(R.synthetic_state_dict(kw, 0), strict=True)
        m = m.to(dev).eval()
        for precision in precisions:
            m.precision = precision
            for shape, volume in shapes:
                tag = f"unet/{variant}/{precision}/{'x'.join(map(str, shape))}"
                x = R.synthetic_input(100, 1, shape).to(dev)
                with torch.no_grad():
                    emit(f"{tag}/forward", m(x))
                    for module in (2, 5):
                        y, feats = m.forward_hip_taps(x, [module])
                        emit(f"{tag}/taps{module}/out", y)
                        emit(f"{tag}/taps{module}/feat", feats[0])
                    xv = R.synthetic_input(101, 1, volume).to(dev)
                    emit(f"{tag}/sliding_window_{'x'.join(map(str, volume))}",
                         sliding_window_inference(xv, roi, 4, m, overlap=0.25, mode="gaussian"))
                    if shape == shapes[0][0]:
                        # encode_only ending at the conv, norm and activation id of one group (the one behind the stem: no pair then),
                        # and the whole-volume call: the window route with its event gates
                        for module in (3, 4, 5):
                            emit(f"{tag}/encode_only{module}/feat", m.forward_hip_taps(x, [module], encode_only=True)[0])
                        emit(f"{tag}/sliding_window_volume_{'x'.join(map(str, volume))}",
                             sliding_window_volume(xv, roi, m, overlap=0.25, mode="gaussian"))
                    y, recs = m.profile_forward(x)
                emit(f"{tag}/profile_forward/out", y)
                emit_names(f"{tag}/profile_forward/names", [r["kernel"] for r in recs])

    # ---- the whole-volume call with a head: logits and labels of tests/test_sliding_window_call_gpu.py (6 windows: one lane)
    from test_sliding_window_call_gpu import centred_head
    kw = R.VARIANTS["anatomix"]
    with contextlib.redirect_stdout(sys.stderr):
        m = anatomix_amd.Unet(**kw)
    m.load_state_dict(R.synthetic_state_dict(kw, 0), strict=True)
    m = m.to(dev).eval()
    xv = R.synthetic_input(42, 1, (64, 96, 80)).to(dev)
    with torch.no_grad():
        feat = sliding_window_volume(xv, 64, m, overlap=0.7)
        emit("unet/anatomix/sliding_window_volume_64x96x80/features", feat)
        head = centred_head(feat, 5, 3)
        for out in ("logits", "labels"):
            emit(f"unet/anatomix/sliding_window_volume_64x96x80/{out}", sliding_window_volume(xv, 64, m, overlap=0.7, head=head, out=out))

    # ---- every configuration tests/test_unet_gpu.py parametrises beside the shipped ones, at its shapes, seeds and tap lists: the
    # export-pass outputs, doubleconv=False, padded widths, ngf = 8, instance norm + Avg + trilinear, no skips, input_nc > 1
    import test_unet_gpu as T
    cases = lambda test: test.pytestmark[0].args[1]
    configs = ([(kw, size, [], 4) for kw, size in cases(T.test_small_volumes_and_wide_outputs)]
               + [(kw, size, layers, 6) for kw, size, layers in cases(T.test_widths_that_are_not_multiples_of_16)]
               + [(kw, size, layers, 8) for kw, size, layers in cases(T.test_input_and_output_channel_counts_of_the_constructor_envelope)])
    for k, (kw, size, layers, seed) in enumerate(configs):
        full = {**dict(ngf=24), **kw}
        with contextlib.redirect_stdout(sys.stderr):
            m = anatomix_amd.Unet(**kw)
        m.load_state_dict(R.synthetic_state_dict(full, seed), strict=True)
        m = m.to(dev).eval()
        tag = "unet/config%d/%s/%s" % (k, ",".join(f"{a}={full[a]}" for a in sorted(full) if a != "dimension"), "x".join(map(str, size)))
        x = torch.cat([R.synthetic_input(50 + ch, 2, size) for ch in range(kw["input_nc"])], dim=1).to(dev)
        with torch.no_grad():
            y, feats = m(x, layers) if layers else (m(x), [])
            emit(f"{tag}/forward", y)
            for layer, f in zip(sorted(layers), feats):
                emit(f"{tag}/tap{layer}", f)
            y, recs = m.profile_forward(x)
        emit(f"{tag}/profile_forward/out", y)
        emit_names(f"{tag}/profile_forward/names", [r["kernel"] for r in recs])

    # ---- amx_conv3d_k3_reflect_ws / amx_conv3d_upcat_merged: (route, c0, c1, cout, size, precision, planar output)
    g = torch.Generator().manual_seed(20250301)
    layers = (("zmarch", 16, 0, 16, 32, "f16", False), ("zmarch_out32", 16, 0, 16, 32, "f16", True), ("ks", 64, 0, 64, 16, "f16", False),
              ("ks_split", 128, 0, 256, 8, "f16", False), ("v2_upseg", 32, 64, 32, 32, "f16", False), ("upcat16", 16, 32, 16, 32, "f16", False),
              ("upmerge", 32, 64, 32, 32, "f16", False), ("ks_shape_mx", 64, 0, 64, 16, "f16x2mx", False),
              ("v2_upseg_mx", 32, 64, 32, 32, "f16x2mx", False))
    for route, c0, c1, cout, s, precision, planar in layers:
        x0 = torch.randn(1, c0, s, s, s, generator=g)
        x1 = torch.randn(1, c1, s // 2, s // 2, s // 2, generator=g) if c1 else None
        w = torch.randn(cout, c0 + c1, 3, 3, 3, generator=g) / (27 * (c0 + c1)) ** 0.5
        scale, shift = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g) * 0.1
        if route == "upmerge":
            out = U.run_conv_merged(dev, x0, x1, w, scale, shift, 1, precision)
        else:
            out = U.run_conv(dev, x0, x1, w, scale, shift, 1, precision, planar=planar)      # (offers the split-K scratch)
        emit(f"conv_layer/{route}/{c0}+up{c1}->{cout}@{s}/{precision}/out", out)


def vit_section(dev, emit, tree):
    """The 3D ViT on cases A, B, C of tests/test_vit_sliding_window_gpu.py, with that file's models, seeds and state dicts: the
    forward of one window, the window-batch route (amx_vit_forward_windows) in both modes, and the whole-volume call
    (amx_vit_sliding_window) for features, logits and labels."""
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch
    import test_vit_sliding_window_gpu as T
    from anatomix_amd.registration.sliding_window import sliding_window_inference, sliding_window_volume

    for case in ("A", "B", "C"):
        roi, size, overlap, corners = T.CASES[case]
        model, _ = T.vit(roi, dev)
        x = T.volume(case, dev)
        z, y, xx = corners[-1]
        with torch.no_grad():
            emit(f"vit/{case}/forward", model(x[:, :, z:z + roi[0], y:y + roi[1], xx:xx + roi[2]].contiguous()))
            for mode, kw in (("gaussian", T.GAUSS), ("constant", dict(mode="constant"))):
                emit(f"vit/{case}/sliding_window_inference/{mode}", sliding_window_inference(x, roi, 4, model, overlap=overlap, **kw))
                feat = sliding_window_volume(x, roi, model, overlap=overlap, **kw)
                emit(f"vit/{case}/sliding_window_volume/features/{mode}", feat)
            head = T.centred_head(feat, 5, T.HEAD_SEED)
            for out in ("logits", "labels"):
                emit(f"vit/{case}/sliding_window_volume/{out}", sliding_window_volume(x, roi, model, overlap=overlap, head=head, out=out))


def train_section(dev, emit, size, only_step):
    """model/train.py and pretraining/step.py: outputs, taps, parameter gradients, running statistics, step records."""
    import copy
    from argparse import Namespace
    import torch
    import anatomix_amd
    from anatomix_amd.model import train as TR
    from anatomix_amd.pretraining import FusedAdamW, GraphedContrastiveStep, PatchSampleF, SupPatchNCELoss, contrastive_step
    from oracle import pretrain_inputs as PI, unet_ref as R

    def net(kw, precision, seed=3, gain=1.0):
        with contextlib.redirect_stdout(sys.stderr):
            m = anatomix_amd.Unet(**kw)
        m.load_state_dict(R.synthetic_state_dict(kw, seed, gain=gain), strict=True)
        m.precision = precision
        return m.to(dev).train()

    def emit_state(tag, m, grads=True):
        for k, p in m.named_parameters():
            if grads and p.grad is not None:
                emit(f"{tag}/grad/{k}", p.grad)
            elif not grads:
                emit(f"{tag}/param/{k}", p)
        for k, b in m.named_buffers():
            emit(f"{tag}/buffer/{k}", b)

    def dense_case(tag, m, x, layers, scale=4096.0):
        """The loss of tests/test_train_step_gpu.py::_compare: seeded cotangents on the taps + 0.1 * mean(out^2)."""
        out, feats = m(x, layers)
        g = torch.Generator().manual_seed(5)
        loss = 0.1 * out.square().mean()
        for f in feats:
            loss = loss + (f * (torch.randn(f.shape, generator=g).to(dev) / f[0].numel() ** 0.5)).sum()
        (loss * scale).backward()
        emit(f"{tag}/out", out)
        for l, f in zip(sorted(layers), feats):
            emit(f"{tag}/tap{l}", f)
        if x.grad is not None:
            emit(f"{tag}/grad/input", x.grad)
        emit_state(tag, m)

    x32 = R.synthetic_input(11, 2, (32, 32, 32)).to(dev)
    base = dict(dimension=3, input_nc=1)
    if not only_step:
        shallow = [("batch_d1", dict(output_nc=16, num_downs=1, ngf=16), [0, 3, 5, 10, 13, 17, 20]),
                   ("batch_single_lrelu", dict(output_nc=16, num_downs=2, ngf=16, doubleconv=False, activation="lrelu"), [0, 3, 7, 11, 15, 19]),
                   ("batch_ngf32", dict(output_nc=32, num_downs=2, ngf=32), [3, 13, 20, 27, 34]),
                   ("instance_avg_trilinear", dict(output_nc=32, num_downs=2, ngf=32, norm="instance", pooling="Avg", interp="trilinear", norm_eps=1e-2),
                    [3, 13, 20, 27, 34]),
                   ("instance_affine_lrelu", dict(output_nc=16, num_downs=1, ngf=16, norm="instance_affine", activation="lrelu"), [0, 3, 5, 10, 13, 17, 20]),
                   ("batch_avg_trilinear", dict(output_nc=16, num_downs=2, ngf=16, norm="batch", pooling="Avg", interp="trilinear"), [3, 13, 20, 27, 34])]
        for name, kw, layers in shallow:
            dense_case(f"train/{name}", net(dict(base, **kw), "f16"), x32, layers)
        for mode, layers in (("some_layers_frozen", [3, 13, 20, 27, 34]), ("whole_network_eval", [4, 13, 21, 34])):
            m = net(dict(base, output_nc=16, num_downs=2, ngf=16, activation="lrelu"), "f16")
            if mode == "whole_network_eval":
                m.eval()
            else:
                for i, mod in enumerate(m.model):
                    if isinstance(mod, torch.nn.BatchNorm3d) and i % 2 == 0:
                        mod.eval()
            dense_case(f"train/frozen/{mode}", m, x32, layers)
        for interp, pooling in (("nearest", "Max"), ("trilinear", "Avg")):
            m = net(dict(base, output_nc=16, num_downs=2, ngf=16, interp=interp, pooling=pooling), "f16")
            kinds = [type(mod).__name__ for mod in m.model]
            dense_case(f"train/pool_up_taps/{interp}_{pooling}", m,
                       x32, [i for i, k in enumerate(kinds) if k in ("MaxPool3d", "AvgPool3d", "Upsample")] + [len(kinds) - 1])
        dense_case("train/input_gradient", net(dict(base, output_nc=16, num_downs=1, ngf=16), "f16"), x32.clone().requires_grad_(True), [], scale=64.0)

    # ---- the 6 M variant: dense and sampled taps, each twice (the second pass replays the recorded pack plan)
    kw6 = R.VARIANTS["anatomix"]
    sizes = [(size >> s,) * 3 for s in (3, 4, 3, 2, 1, 0)]                # the tap shapes of NCE_LAYERS
    g = torch.Generator().manual_seed(77)
    ids = []
    for sz in sizes:
        flat = torch.randperm(sz[0] ** 3, generator=g)[:64]
        ids.append(torch.stack([flat // (sz[0] * sz[0]), flat // sz[0] % sz[0], flat % sz[0]], dim=1).to(dev))
    if not only_step:
        for route in ("dense", "sampled"):
            m = net(kw6, "bf16", gain=2 ** 0.5)
            for rep in (0, 1):
                for p in m.parameters():
                    p.grad = None
                tag = f"train/6m/{route}/pass{rep}"
                if route == "dense":
                    dense_case(tag, m, x32, PI.NCE_LAYERS, scale=1.0)
                    continue
                out, rows, coords, dims = TR.forward_train_sampled(m, x32, PI.NCE_LAYERS, lambda i, shape: ids[PI.NCE_LAYERS.index(i)])
                gen = torch.Generator().manual_seed(5)
                sum((r * torch.randn(r.shape, generator=gen).to(dev)).sum() for r in rows).backward()
                emit(f"{tag}/out", out)
                for l, r in zip(PI.NCE_LAYERS, rows):
                    emit(f"{tag}/rows{l}", r)
                emit_state(tag, m)

    # ---- one eager step and three graphed replays, FusedAdamW with and without clipping
    A, B, seg = [t.to(dev) for t in PI.step_inputs(size)]
    nopt = Namespace(nce_T=0.33, weigh_rarity=False, balance_denominator=False, weighting_mode="raw")
    okw = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-5)
    # (at 32^3 the bottleneck tap has 8 voxels: with 64 patches the per-layer shapes differ and the step takes the per-layer head routes,
    #  with 8 patches the batched one)
    for P, max_norm in ((64, None), (64, 1.0), (8, None)):
        netG = net(kw6, "bf16", gain=2 ** 0.5)
        torch.manual_seed(9)
        with contextlib.redirect_stdout(sys.stderr):
            netF = PatchSampleF(use_mlp=True, init_type="kaiming", nc=256, n_mlps=3)
            netF.create_mlp([torch.zeros(1, c, 1, 1, 1, device=dev) for c in (128, 256, 128, 64, 32, 16)])
        netF = netF.to(dev).train()
        crits = [SupPatchNCELoss(nopt) for _ in PI.NCE_LAYERS]
        for mode in ("eager", "graphed"):
            nG, nF = copy.deepcopy(netG), copy.deepcopy(netF)
            opts = (FusedAdamW(nG.parameters(), max_norm=max_norm, **okw), FusedAdamW(nF.parameters(), max_norm=max_norm, **okw))
            tag = f"train/step{size}/{mode}/patches_{P}/max_norm_{max_norm}"
            if mode == "eager":
                recs = [contrastive_step(nG, nF, crits, A, B, seg, PI.NCE_LAYERS, num_patches=P, optimizers=opts, sample_ids=[c[:P] for c in ids])]
            else:
                step = GraphedContrastiveStep(nG, nF, crits, PI.NCE_LAYERS, opts, num_patches=P, warmup=2, sample_ids=[c[:P] for c in ids])
                recs = [step(A, B, seg) for _ in range(3)]
            for k, r in enumerate(recs):
                emit(f"{tag}/record{k}", torch.tensor([r["loss"], r["grad_norm_G"], r["grad_norm_F"]] + list(r["per_layer"].values()), dtype=torch.float64))
            emit_state(f"{tag}/netG", nG, grads=False)
            emit_state(f"{tag}/netF", nF, grads=False)


def child(section, tree, size, dump):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from anatomix_amd import _lib, _stream
    from anatomix_amd.datagen import views as SV
    from anatomix_amd.pretraining import augment as P
    from anatomix_amd.registration import convex_adam_utils as CU, instance_optimization as IO, metrics as RM
    from anatomix_amd.segmentation import augment as G

    dev = torch.device("cuda:0")
    lib = _lib.load()
    gen = torch.Generator().manual_seed(20240607)
    count, kept = [0], {}

    def emit(name, t):
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        count[0] += 1
        if dump:
            kept[name] = t.detach().cpu()
        print(f"{name} {tuple(t.shape)} {str(t.dtype).split('.')[1]} {h}", flush=True)

    def rand(*shape, offset=0):
        """Seeded standard-normal device tensor; offset = 1 puts its base one float past an aligned allocation."""
        buf = torch.empty(int(np.prod(shape)) + offset, dtype=torch.float32, device=dev)
        buf[offset:] = torch.randn(int(np.prod(shape)), generator=gen).to(dev)
        return buf[offset:].view(*shape)

    def empty(*shape, offset=0, dtype=torch.float32):
        return torch.empty(int(np.prod(shape)) + offset, dtype=dtype, device=dev)[offset:].view(*shape)

    def done():
        torch.cuda.synchronize()
        if dump:
            torch.save(kept, dump)
        print(f"# {count[0]} tensors from {_lib.LIB_PATH}", flush=True)

    if section in ("train", "train_step"):
        train_section(dev, emit, size, section == "train_step")
        return done()
    if section in ("unet", "all"):
        unet_section(dev, emit, tree)
    if section == "unet":
        return done()
    if section == "vit":
        vit_section(dev, emit, tree)
        return done()

    # ---- amx_seg_loss_forward / _backward / amx_seg_argmax, head mode and logits mode
    LABEL = (torch.float32, torch.int64, torch.uint8)
    seg_cases = [("V1", 1, 2, (1, 1, 1), 0), ("c5_17x16x19", 3, 5, (17, 16, 19), 0), ("c5_odd_17x15x19", 3, 5, (17, 15, 19), 0),
                 ("V4096", 2, 3, (16, 16, 16), 0), ("V4096_off1", 2, 3, (16, 16, 16), 1), ("96cubed", 4, 5, (96, 96, 96), 0)]
    for ci, (tag, B, C, size, off) in enumerate(seg_cases):
        V = int(np.prod(size))
        for F in (16, 0):
            mode = "head" if F else "logits"
            ldt = LABEL[(ci + (1 if F else 0)) % 3]
            x = rand(B, F or C, V, offset=off)
            w = rand(C, F) * 0.3 if F else None
            b = rand(C) if F else None
            lab = torch.randint(0, C, (B, V), generator=gen).to(ldt).to(dev)
            loss, stats = torch.empty(3, dtype=torch.float32, device=dev), torch.empty(B, C, 3, dtype=torch.float32, device=dev)
            bad = torch.empty(1, dtype=torch.int64, device=dev)
            lt = _lib.SEG_LABEL[str(ldt).split(".")[1]]
            tail = (0, 1e-5, 1e-5, 1.0, 1.0)        # include_background, smooth_nr, smooth_dr, lambda_dice, lambda_ce
            nb = lib.amx_seg_loss_scratch_bytes(B, V, C, F)
            sc = _lib.scratch(nb, dev)
            _lib.check(lib.amx_seg_loss_forward(_lib.ptr(x), F, _lib.ptr(w), _lib.ptr(b), _lib.ptr(lab), lt, B, C, V, *tail,
                                                _lib.ptr(loss), _lib.ptr(stats), _lib.ptr(bad), _lib.ptr(sc), nb, _lib.stream(dev)))
            for n, t in (("loss", loss), ("stats", stats), ("bad", bad)):
                emit(f"seg_loss_forward/{mode}/{tag}/{n}", t)
            gout = torch.tensor([0.7, 0.0, 0.0], dtype=torch.float32, device=dev)
            dx = empty(B, F or C, V, offset=off)
            dw = torch.empty(C, F, dtype=torch.float32, device=dev) if F else None
            db = torch.empty(C, dtype=torch.float32, device=dev) if F else None
            _lib.check(lib.amx_seg_loss_backward(_lib.ptr(x), F, _lib.ptr(w), _lib.ptr(b), _lib.ptr(lab), lt, B, C, V, *tail,
                                                 _lib.ptr(stats), _lib.ptr(gout), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                                 _lib.ptr(sc) if F else None, nb, _lib.stream(dev)))
            for n, t in (("dx", dx), ("dw", dw), ("db", db)):
                if t is not None:
                    emit(f"seg_loss_backward/{mode}/{tag}/{n}", t)
            pred = torch.empty(B, V, dtype=torch.uint8, device=dev)
            _lib.check(lib.amx_seg_argmax(_lib.ptr(x), F, _lib.ptr(w), _lib.ptr(b), B, C, V, _lib.ptr(pred), _lib.stream(dev)))
            emit(f"seg_argmax/{mode}/{tag}/labels", pred)
            del x, dx, lab, pred, sc

    # ---- segaug: minmax (+ finalize), pointwise x 2, crop, gaussian x 2, affine, minmax_finalize of the affine's partials
    B = 4
    for s in (15, 16, 96):
        size, tag = (s, s, s), f"{s}cubed"
        vols = [rand(s + 3, s + 2, s + 1) for _ in range(B)]
        labs = [torch.randint(0, 5, (s + 3, s + 2, s + 1), generator=gen).to(torch.uint8).to(dev) for _ in range(B)]
        t = G._Table(B)
        for i in range(B):
            t.host["vol"][i], t.host["lab"][i] = vols[i].data_ptr(), labs[i].data_ptr()
            t.host["vol_dim"][i] = vols[i].shape
            t.host["corner"][i] = (i % 4, i % 3, i % 2)
            t.host["flags"][i] = (G.RESCALE | G.CONTRAST | G.AFFINE | (G.NOISE if i != 1 else 0) | (G.BIAS if i != 2 else 0)
                                  | (G.SMOOTH | G.SHARPEN if i != 3 else 0))
            t.host["noise_std"][i] = 0.05 + 0.01 * i
            t.host["bias"][i] = np.linspace(0.0, 0.05, 20) * (1 + i)
            t.host["gamma"][i] = 0.6 + 0.9 * i
            t.host["sharpen_alpha"][i] = 10.0 + 5.0 * i
            t.host["affine"][i] = G.affine_matrix((0.1 * i, -0.2, 0.3), (0.05, -0.1, 0.02 * i), (1.1, 0.9, 1.0 + 0.05 * i)).reshape(9)
        G._set_taps(t, 0, np.array([[0.5 + 0.1 * i, 0.6, 0.85] for i in range(B)]))
        G._set_taps(t, 1, np.array([[0.8, 0.5 + 0.1 * i, 0.7] for i in range(B)]))
        G._set_taps(t, 2, np.array([[0.5, 0.6, 0.5 + 0.05 * i] for i in range(B)]))
        t.device(dev)
        img, lab = G._crop(t, B, size, rand(B, 1, *size), torch.uint8, dev)
        emit(f"segaug_crop/{tag}/img", img)
        emit(f"segaug_crop/{tag}/lab", lab)
        mm = G._minmax(img)
        emit(f"segaug_minmax/{tag}/minmax", mm)
        emit(f"segaug_pointwise/scale/{tag}/out", G._pointwise(img, torch.empty_like(img), mm, G._OP_SCALE, t))
        pos = img.abs() + 0.1
        emit(f"segaug_pointwise/contrast/{tag}/out", G._pointwise(pos, torch.empty_like(pos), G._minmax(pos), G._OP_CONTRAST, t))
        emit(f"segaug_gaussian/smooth/{tag}/out", G._gaussian(img, G._GAUSS_SMOOTH, t))
        emit(f"segaug_gaussian/sharpen/{tag}/out", G._gaussian(img, G._GAUSS_SHARPEN, t))
        out, olab, sc, nb = G._affine(img, lab, size, t)
        emit(f"segaug_affine/{tag}/img", out)
        emit(f"segaug_affine/{tag}/lab", olab)
        mm2 = torch.empty((B, 2), dtype=torch.float32, device=dev)
        _lib.check(lib.amx_segaug_minmax_finalize(_lib.ptr(sc), nb, B, out[0].numel(), _lib.ptr(mm2), _lib.stream(dev)))
        emit(f"segaug_minmax_finalize/{tag}/minmax", mm2)
        del vols, labs, img, lab, out, olab, pos

    # ---- preaug: spatial (image and label), blur, intensity on 2 views; off = 1 puts every base one element past an allocation
    st = _lib.stream(dev)
    for tag, shape, off in (("12x10x8", (12, 10, 8), 0), ("12x10x8_off1", (12, 10, 8), 1), ("9x11x7", (9, 11, 7), 0), ("37x35x70", (37, 35, 70), 0)):
        x, noise = rand(2, *shape, offset=off), rand(2, *shape, offset=off)
        lab = empty(*shape, offset=off, dtype=torch.uint8)
        lab.copy_(torch.randint(0, 7, shape, generator=gen).to(torch.uint8))
        mm = P._minmax(x)
        for which in ("both_on", "view1_copied"):
            t = P._Table(2)
            t.host["flags"] = P.SPATIAL | P.BLUR | P.NOISE | P.BIAS | P.GAMMA
            if which == "view1_copied":
                t.host["flags"][1] = P.NOISE | P.GAMMA
            t.host["map"][0] = P.spatial_map(shape, (True, False, True), (1.2, 0.8, 1.1), (20.0, -35.0, 10.0)).reshape(12)
            t.host["map"][1] = P.spatial_map(shape, (False, True, False), (0.7, 1.3, 0.9), (-40.0, 5.0, 25.0)).reshape(12)
            P._set_taps(t, np.array([[2.0, 2.0, 2.0], [0.6, 1.3, 0.0]]))
            t.host["noise_std"], t.host["gamma"] = (0.1, 0.2), (0.7, 1.4)
            t.host["bias"] = np.linspace(-0.5, 0.5, 20)[None] * np.array([[1.0], [-0.6]])
            t.device(dev)
            with_lab = which == "both_on"
            out, tmp = empty(2, *shape, offset=off), empty(2, *shape, offset=off)
            olab = empty(*shape, offset=off, dtype=torch.uint8) if with_lab else None
            _lib.check(lib.amx_preaug_spatial(_lib.ptr(x), _lib.ptr(lab if with_lab else None), 2, *shape, _lib.ptr(mm), _lib.ptr(out),
                                              _lib.ptr(olab), *t.args, st))
            emit(f"preaug_spatial/{tag}/{which}/img", out)
            if with_lab:
                emit(f"preaug_spatial/{tag}/{which}/lab", olab)
            _lib.check(lib.amx_preaug_blur(_lib.ptr(x), _lib.ptr(out), _lib.ptr(tmp), 2, *shape, *t.args, st))
            emit(f"preaug_blur/{tag}/{which}/out", out)
            _lib.check(lib.amx_preaug_intensity(_lib.ptr(x), _lib.ptr(noise), _lib.ptr(tmp), 2, *shape, *t.args, st))
            emit(f"preaug_intensity/{tag}/{which}/out", tmp)
        del x, noise, lab, out, tmp, olab

    # ---- synth: every entry on batch 2 (4 rows); noff = 1 puts the noise one float past an allocation.  k-space is a seeded tensor.
    n = 4
    for tag, shape, scales, noff in (("16x32x48", (16, 32, 48), (4, 8, 16), 0), ("16x32x48_noise_off1", (16, 32, 48), (4, 8, 16), 1),
                                     ("9x15x21", (9, 15, 21), (1, 3), 0)):
        V = int(np.prod(shape))
        uniq = [np.arange(5), np.arange(6)]
        params = dict(unique_labels=uniq, means=[np.linspace(25, 255, 2 * u.size).reshape(2, -1) for u in uniq],
                      stds=[np.linspace(5, 20, 2 * u.size).reshape(2, -1) for u in uniq],
                      zero_background=np.array([[False, False], [True, False]]), perl_mult_factor=0.02)
        t = SV._appearance_table(params, 2)
        t.host["flags"] |= np.array([SV.SPIKE, SV.SPIKE | SV.SPIKE_FIXED | SV.LOWRES, SV.LOWRES, SV.LOWRES])
        t.host["spike_loc"] = (shape[0] // 2 + 1, shape[1] // 3, 1)
        t.host["spike_loc"][1] = (0, shape[1] - 1, shape[2] // 2)
        t.host["spike_slot"], t.host["spike_factor"], t.host["spike_intensity"] = (0, 1, 0, 0), 1.0, 3.0
        t.host["lowres"] = [SV.low_resolution_shape(shape, z) for z in (1.0, 0.5, 0.8, 0.5)]
        t.device(dev)
        lab = torch.cat([torch.randint(0, u.size, (1, V), generator=gen) for u in uniq]).to(torch.uint8).to(dev)
        noise = rand(n, V, offset=noff)
        grids = [rand(n, *[a // s for a in shape]) * (1.0 + i) for i, s in enumerate(scales)]
        sc, nb = SV._scratch(n, V, dev)
        _lib.check(lib.amx_synth_gmm_minmax(_lib.ptr(lab), _lib.ptr(noise), 2, V, *t.args, _lib.ptr(sc), nb, st))
        mm = _stream.minmax_finalize(sc, nb, n, V, dev)
        emit(f"synth_gmm_minmax/{tag}/minmax", mm)
        x = empty(n, V)
        gp = (ctypes.c_void_p * len(scales))(*[g.data_ptr() for g in grids])
        _lib.check(lib.amx_synth_appearance(_lib.ptr(lab), _lib.ptr(noise), gp, (ctypes.c_int * len(scales))(*scales), len(scales),
                                            _lib.ptr(mm), _lib.ptr(x), 2, *shape, *t.args, _lib.ptr(sc), nb, st))
        emit(f"synth_appearance/{tag}/out", x)
        emit(f"synth_appearance/{tag}/minmax", _stream.minmax_finalize(sc, nb, n, V, dev))
        k, mean = rand(2, V, 2), empty(2)
        _lib.check(lib.amx_synth_logk_mean(_lib.ptr(k), 2, V, _lib.ptr(mean), _lib.ptr(sc), nb, st))
        emit(f"synth_logk_mean/{tag}/mean", mean)
        _lib.check(lib.amx_synth_spike(_lib.ptr(x), _lib.ptr(k), 2, _lib.ptr(mean), n, *shape, *t.args, st))
        emit(f"synth_spike/{tag}/out", x)
        low = empty(n, V)
        _lib.check(lib.amx_synth_lowres(_lib.ptr(x), _lib.ptr(low), n, *shape, *t.args, st))
        emit(f"synth_lowres/{tag}/out", low)
        _lib.check(lib.amx_synth_clip_minmax(_lib.ptr(low), n, V, _lib.ptr(sc), nb, st))
        mm = _stream.minmax_finalize(sc, nb, n, V, dev)
        emit(f"synth_clip_minmax/{tag}/minmax", mm)
        for u8 in (0, 1):
            fin = empty(n, V, dtype=torch.uint8 if u8 else torch.float32)
            _lib.check(lib.amx_synth_finish(_lib.ptr(low), _lib.ptr(fin), n, V, _lib.ptr(mm), u8, st))
            emit(f"synth_finish/{tag}/{'uint8' if u8 else 'float32'}", fin)
        del lab, noise, grids, x, low, k

    # ---- registration metrics
    for shape in ((7, 9, 11), (32, 32, 32)):
        tag = "x".join(map(str, shape))
        a = torch.randint(0, 14, shape, generator=gen)
        bb = torch.where(torch.rand(shape, generator=gen) < 0.8, a, torch.randint(0, 20, shape, generator=gen))     # some >= bins: bad
        for da, db_ in ((torch.uint8, torch.int64), (torch.float32, torch.uint8)):
            counts, nbad = RM._overlap(a.to(da).to(dev), bb.to(db_).to(dev), 16)
            pair = f"{str(da).split('.')[1]}_{str(db_).split('.')[1]}"
            emit(f"label_overlap/{tag}/{pair}/counts", counts)
            emit(f"label_overlap/{tag}/{pair}/bad", nbad)
        jdet, stats = CU._jacobian_call(rand(3, *shape) * 0.3, 1, True, True)
        emit(f"jacobian_det/{tag}/jdet", jdet)
        emit(f"jacobian_det/{tag}/stats", stats)

    # ---- instance optimisation (12 x 10 x 14, c = 3, g = 1) and the stage-1 features (5 x 8 x 16; 7 channels on 6 x 9 x 11)
    h, w, d, c = 12, 10, 14, 3
    wgt, fix, mov = rand(1, 3, h, w, d) * 0.5, rand(1, c, h, w, d), rand(1, c, h, w, d)
    for n, tns in zip(("grad", "disp_sample", "loss", "reg"), IO.instance_opt_grad(wgt, fix, mov, 0.75)):
        emit(f"instance_opt_grad/{h}x{w}x{d}/{n}", tns)
    emit(f"run_instance_opt/{h}x{w}x{d}/niter5/out", IO.run_instance_opt(wgt * 2, fix, mov, 1, 0.75, (h, w, d), 5, 0))
    emit(f"run_instance_opt/{h}x{w}x{d}/niter5_smooth3/out", IO.run_instance_opt(wgt * 2, fix, mov, 1, 0.75, (h, w, d), 5, 3))
    emit("mindssc/5x8x16/r1d2/out", CU.MINDSSC(rand(1, 1, 5, 8, 16).abs(), 1, 2))
    emit("mindssc/5x8x16/r2d2/out", CU.MINDSSC(rand(1, 1, 5, 8, 16).abs(), 2, 2))
    ssd, amin = CU.correlate(rand(1, 7, 6, 9, 11), rand(1, 7, 6, 9, 11), 1, 1, (6, 9, 11), 7)
    emit("correlate_ssd/6x9x11/hw1/ssd", ssd)
    emit("correlate_ssd/6x9x11/hw1/argmin", amin)
    done()


# ---- parent: two children, one comparison -----------------------------------------------------------------------------------

def run_side(name, lib_path, timeout, section, tree=ROOT, size=32, dump=None):
    env = dict(os.environ, AMX_LIB_PATH=os.path.abspath(lib_path))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--section", section, "--tree", os.path.abspath(tree), "--size", str(size)]
    try:
        r = subprocess.run(cmd + (["--dump", dump] if dump else []), env=env, cwd=ROOT, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        print(f"{name}: no listing within {timeout} s")
        return None
    if r.returncode != 0:
        print(f"{name}: child exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("#")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", action="store_true", help="print this process's listing (AMX_LIB_PATH selects the library)")
    ap.add_argument("--old", help="the library to compare against (e.g. the parent commit's build)")
    ap.add_argument("--new", default=os.path.join(ROOT, "anatomix_amd", "csrc", "libanatomix_amd.so"))
    ap.add_argument("--old-tree", help="a directory with another commit's anatomix_amd/, oracle/ and tests/: the old side's Python")
    ap.add_argument("--tree", default=ROOT, help="(child) the tree this listing imports from")
    ap.add_argument("--dump", help="(child) also save every tensor to this file")
    ap.add_argument("--size", type=int, default=32, help="cube side of the contrastive steps of the train sections")
    ap.add_argument("--section", choices=("streams", "unet", "vit", "all", "train", "train_step"), default="all")
    ap.add_argument("--expect-different", metavar="REGEX", help="names the caller expects to differ (a repaired path): listed, not counted")
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds per child")
    ap.add_argument("--print-listings", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.section, a.tree, a.size, a.dump)
    if not (a.old or a.old_tree):
        ap.error("--old or --old-tree is required")
    if a.section in ("train", "train_step") and not a.old_tree:
        ap.error("the train sections compare two trees: --old-tree is required")
    # with --old-tree: old, old again (what is bit-stable on the old side alone), new; every side keeps its tensors for the unstable ones
    sides = [("old", a.old or a.new, a.old_tree or ROOT)] + ([("old2", a.old or a.new, a.old_tree)] if a.old_tree else []) + [("new", a.new, ROOT)]
    listings = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, path, tree in sides:
            if not os.path.exists(path):
                print(f"{name}: {path} does not exist")
                return 2
            listings[name] = run_side(name, path, a.timeout, a.section, tree, a.size, os.path.join(tmp, name + ".pt") if a.old_tree else None)
            if listings[name] is None:
                return 2
            print(f"{name}: {len(listings[name])} tensors from {tree}", flush=True)
        return compare(a, listings, tmp)


def compare(a, listings, tmp):
    old, new = listings["old"], listings["new"]
    if a.print_listings:
        print("\n".join(new))
    key = lambda ln: ln.split(" (")[0]
    do, dn = {key(ln): ln for ln in old}, {key(ln): ln for ln in new}
    diff = [k for k in do if do[k] != dn.get(k)] + [k for k in dn if k not in do]
    expected = [k for k in diff if a.expect_different and re.search(a.expect_different, k)]
    if a.expect_different:
        diff = [k for k in diff if k not in expected]
        print(f"EXPECTED to differ (--expect-different {a.expect_different}): {len(expected)} tensors do")
    d2 = {key(ln): ln for ln in listings.get("old2", old)}
    unstable = [k for k in do if do[k] != d2.get(k)]
    if unstable:
        import torch
        t = {n: torch.load(os.path.join(tmp, n + ".pt")) for n in ("old", "old2", "new")}
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm().clamp_min(1e-300))
        for k in unstable:
            e_self, e_new = rel(t["old2"][k], t["old"][k]), rel(t["new"][k], t["old"][k]) if k in t["new"] else float("inf")
            print(f"UNSTABLE on the old side alone {k}: old vs old {e_self:.3e}, new vs old {e_new:.3e} (held to 1e-4)")
            if e_new <= 1e-4 and k in diff:
                diff.remove(k)
    for k in diff:
        print(f"DIFFERENT {k}\n  old {do.get(k)}\n  new {dn.get(k)}")
    if diff or len(old) != len(new) or not old:
        print(f"ab_bitwise: {len(diff)} of {len(old)} tensors differ between {a.old_tree or a.old} and {a.new}")
        return 1
    print(f"ab_bitwise: identical, {len(old) - len(expected)} tensors ({len(unstable)} of them unstable on the old side and held to the "
          f"tolerance; {len(expected)} more expected to differ), {a.old_tree or a.old} against {a.new}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
