"""The optimizer of the contrastive step: ``torch.optim.AdamW`` as the reference builds it for netG and for netF
(pretraining/models/supcl_model.py:510-516, 584-590; stepped at :628-661), with every parameter tensor of an optimizer updated
by ONE HIP launch (``amx_adamw_step``) instead of torch's few kernels per parameter -- in the graph-replayed step the stock
capturable AdamW is ~170 launches of a few microseconds each.

Same constructor arguments, same update rule, same ``state_dict`` layout as ``torch.optim.AdamW(capturable=True)`` (per parameter:
``step`` a 0-dim fp32 device tensor, ``exp_avg``, ``exp_avg_sq``), so a checkpoint moves between the two.  GPU only: fp32
parameters on a CUDA device -- anything else raises, there is no host path.

Hyper-parameters and HIP graphs.  The reference changes ``lr`` every epoch (base_model.py: get_scheduler / update_learning_rate
set ``param_group['lr']``).  Kernel arguments passed by value are frozen into a captured graph, so the kernel reads {lr, betas, eps,
weight_decay} from a small per-group DEVICE buffer, which ``step()`` refreshes from a pinned host mirror with a copy that is part
of the stream (and of a capture): ``GraphedContrastiveStep`` calls ``refresh_hyperparameters()`` -- a host write into that mirror --
before every replay, and the replayed copy carries the current ``param_groups`` values to the kernel.

Gradient clipping (the reference's ``--clip_grad`` / ``--max_norm_G`` / ``--max_norm_F``, supcl_model.py:631-655).  ``max_norm=``
makes ``step()`` clip as ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` followed by the step would, without the pass over
the gradients: ``grad_norms`` writes the total norm of every optimizer's gradients into its ``total_norm`` (ONE call for all of
them, ``amx_grad_norms``: deterministic, no atomics) and the step kernel multiplies each gradient by
``min(max_norm / (total_norm + 1e-6), 1)`` as it reads it (``amx_adamw_step_clip_dev``).  Two deviations from torch, both
invisible to the reference's loop: ``p.grad`` is left UNCLIPPED (the step zeroes it right after), and the recorded norm is the
norm before clipping (what ``clip_grad_norm_`` returns and the reference logs).  ``total_norm`` is not part of the state_dict."""
import ctypes

import numpy as np
import torch

from .. import _lib


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=True, differentiable=False, fused=None, max_norm=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdamW: lr must be a Python number (schedulers set group['lr'] to one)")
        if amsgrad:
            raise NotImplementedError("FusedAdamW: amsgrad is not offered (the reference does not use it, supcl_model.py:510-516)")
        if differentiable:
            raise NotImplementedError("FusedAdamW: differentiable=True is not offered")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # `capturable` is what GraphedContrastiveStep looks at: the step count lives on the device, a step is graph-safe
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize, foreach=None,
                        capturable=True, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        if max_norm is not None and not float(max_norm) >= 0.0:
            raise ValueError(f"Invalid max_norm: {max_norm}")
        # max_norm lives outside param_groups: the state_dict layout stays that of torch.optim.AdamW
        self.max_norm = None if max_norm is None else float(max_norm)
        first = self.param_groups[0]["params"][0]
        self.total_norm = torch.zeros((), dtype=torch.float32, device=first.device)    # written by grad_norms()
        self._norm_written = False
        self._hyper = {}            # (group index, device) -> (pinned host mirror [5] float64, device buffer [5] float64)

    @staticmethod
    def _hyper_values(group):
        lr = group["lr"]
        if isinstance(lr, torch.Tensor):
            raise ValueError("FusedAdamW: lr must be a Python number (schedulers set group['lr'] to one)")
        beta1, beta2 = group["betas"]
        vals = (float(lr), float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"]))
        if not (vals[0] >= 0.0 and vals[3] >= 0.0 and 0.0 <= vals[1] < 1.0 and 0.0 <= vals[2] < 1.0 and vals[4] >= 0.0):
            raise ValueError(f"FusedAdamW: hyper-parameters out of range: lr {vals[0]}, betas ({vals[1]}, {vals[2]}), eps {vals[3]}, "
                             f"weight_decay {vals[4]}")
        return vals

    def refresh_hyperparameters(self):
        """Write the current ``param_groups`` values into the pinned host mirrors (host-side only; nothing is enqueued).  Called by
        ``step()``, and -- because ``step()`` does not run when a captured graph is replayed -- by ``GraphedContrastiveStep`` before
        every replay.  A CHANGED value first waits for the device: an earlier replay may not have read the mirror yet."""
        for gi, group in enumerate(self.param_groups):
            vals = self._hyper_values(group)
            for (g2, dev), (host, _) in self._hyper.items():
                if g2 == gi and tuple(host.tolist()) != vals:
                    # (not while the stream is being captured: a device-wide synchronise is illegal there and nothing can be
                    #  replaying -- hence reading the mirror -- before the capture ends)
                    if not torch.cuda.is_current_stream_capturing():
                        torch.cuda.synchronize(dev)
                    host.copy_(torch.tensor(vals, dtype=torch.float64))

    def _hyper_buffers(self, gi, group, dev):
        key = (gi, dev)
        if key not in self._hyper:
            host = torch.tensor(self._hyper_values(group), dtype=torch.float64).pin_memory()
            self._hyper[key] = (host, torch.empty(5, dtype=torch.float64, device=dev))
        return self._hyper[key]

    def _state_of(self, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        elif not (torch.is_tensor(st["step"]) and st["step"].is_cuda):
            # a state_dict written by a non-capturable torch.optim.AdamW keeps its step count on the host
            st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32).to(p.device)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        if self.max_norm is not None and not self._norm_written:
            raise RuntimeError("FusedAdamW(max_norm=...): total_norm was never written -- call grad_norms([...]) after the backward "
                               "(or write the norm into optimizer.total_norm and call mark_norm_written())")
        self.refresh_hyperparameters()
        for gi, group in enumerate(self.param_groups):
            per_device = {}
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise RuntimeError("FusedAdamW does not support sparse gradients")
                if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous()):
                    raise RuntimeError(f"FusedAdamW: contiguous fp32 parameters on a CUDA device only (got {p.dtype} on {p.device}, "
                                       f"gradient {g.dtype})")
                st = self._state_of(p)
                if not g.is_contiguous():
                    g = g.contiguous()
                rows, steps, keep = per_device.setdefault(p.device, ([], [], []))
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
                             p.numel()))
                steps.append(st["step"])
                keep.append(g)
            for dev, (rows, steps, keep) in per_device.items():
                with torch.cuda.device(dev):
                    host, dbuf = self._hyper_buffers(gi, group, dev)
                    dbuf.copy_(host, non_blocking=True)                               # captured with the step: replays re-read the mirror
                    torch._foreach_add_(steps, 1.0)                                   # t: one launch for the whole list
                    table = np.asarray(rows, dtype=np.int64)
                    if self.max_norm is None:
                        _lib.check(lib.amx_adamw_step_dev(table.ctypes.data_as(ctypes.c_void_p), len(rows), _lib.ptr(dbuf),
                                                          int(bool(group["maximize"])),
                                                          _lib.stream(dev)))
                    else:
                        if self.total_norm.device != dev:
                            raise RuntimeError("FusedAdamW(max_norm=...): every parameter must live on the device of total_norm")
                        _lib.check(lib.amx_adamw_step_clip_dev(table.ctypes.data_as(ctypes.c_void_p), len(rows), _lib.ptr(dbuf),
                                                               int(bool(group["maximize"])), _lib.ptr(self.total_norm),
                                                               self.max_norm, _lib.stream(dev)))
        return loss

    def mark_norm_written(self):
        """``total_norm`` holds the norm of the current gradients (``grad_norms`` calls this; a caller that fills it itself must)."""
        self._norm_written = True


_NORM_SCRATCH = {}              # device -> uint8 scratch of amx_grad_norms (grown on demand, reused by every call and replay)


@torch.no_grad()
def grad_norms(groups):
    """L2 norm of the gradients of each entry of ``groups`` -- a ``FusedAdamW`` (all parameters of its param_groups), an
    ``nn.Module`` or an iterable of parameters -- as ONE ``amx_grad_norms`` call: a fp32 device tensor ``[len(groups)]``; every
    ``FusedAdamW`` among them also gets its number in ``total_norm``.  Parameters without a gradient are skipped, an entry without
    gradients has norm 0.  No host synchronisation; capturable (call it once eagerly first: the scratch is allocated then)."""
    lists = []
    for entry in groups:
        if isinstance(entry, torch.optim.Optimizer):
            lists.append([p for g in entry.param_groups for p in g["params"]])
        elif isinstance(entry, torch.nn.Module):
            lists.append(list(entry.parameters()))
        else:
            lists.append(list(entry))
    rows, keep, dev = [], [], None
    for gi, params in enumerate(lists):
        for p in params:
            g = p.grad
            if g is None:
                continue
            if not (g.is_cuda and g.dtype == torch.float32) or g.is_sparse:
                raise RuntimeError(f"grad_norms: dense fp32 gradients on a CUDA device only (got {g.dtype} on {g.device})")
            if dev is None:
                dev = g.device
            elif g.device != dev:
                raise RuntimeError("grad_norms: all gradients of one call on one device")
            if not g.is_contiguous():
                g = g.contiguous()
            rows.append((g.data_ptr(), g.numel(), gi))
            keep.append(g)
    fused = [(k, e) for k, e in enumerate(groups) if isinstance(e, FusedAdamW)]
    if dev is None:
        dev = fused[0][1].total_norm.device if fused else None
        if dev is None:
            raise RuntimeError("grad_norms: no gradient and no FusedAdamW to take the device from")
    lib = _lib.load()
    table = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    tptr = table.ctypes.data_as(ctypes.c_void_p)
    need = int(lib.amx_grad_norms_scratch_bytes(tptr, len(rows), len(lists)))
    if need == 0:
        raise RuntimeError("grad_norms: too many elements for one call")
    with torch.cuda.device(dev):
        scratch = _NORM_SCRATCH.get(dev)
        if scratch is None or scratch.numel() < need:
            scratch = _NORM_SCRATCH[dev] = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=dev)
        out = torch.empty(len(lists), dtype=torch.float32, device=dev)
        _lib.check(lib.amx_grad_norms(tptr, len(rows), len(lists), _lib.ptr(out), _lib.ptr(scratch), scratch.numel(),
                                      _lib.stream(dev)))
        if fused:
            torch._foreach_copy_([e.total_norm for _, e in fused], [out[k] for k, _ in fused])
            for _, e in fused:
                e.mark_norm_written()
    return out
