"""The learning-rate policies of the pretraining loop (reference: pretraining/models/pretraining_networks.py:526-599 get_scheduler;
stepped once per epoch by base_model.py:209-218 update_learning_rate, ``plateau`` once per evaluation with the validation loss).
They are torch's own schedulers with the reference's constants; they set ``param_group['lr']`` to a Python float, which is what
``FusedAdamW`` carries to its kernel (and into a replayed graph) through its device mirror."""
from torch.optim import lr_scheduler

POLICIES = ("const_linear", "linear", "exponential", "step", "plateau", "cosine")


def get_scheduler(optimizer, opt):
    """``opt`` carries lr_policy, n_epochs, n_epochs_decay and (for ``step``) lr_decay_iters.

      const_linear  factor 1 for the first n_epochs, then down by 1 / (n_epochs_decay + 1) per epoch; counted by the scheduler's
                    own epoch (restored by its state_dict on resume), never offset by opt.epoch_count
      linear        LinearLR from 1 to 0.05 over n_epochs + n_epochs_decay epochs
      exponential   0.99 per epoch
      step          halved every lr_decay_iters epochs
      plateau       ReduceLROnPlateau(min, factor 0.5, threshold 1e-4, patience 5, min_lr 1e-7) on the validation loss
      cosine        CosineAnnealingLR(T_max = n_epochs, eta_min 0)"""
    policy = opt.lr_policy
    if policy == "const_linear":
        n_epochs, n_decay = opt.n_epochs, opt.n_epochs_decay
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda epoch: 1.0 - max(0, epoch - n_epochs) / float(n_decay + 1))
    if policy == "linear":
        return lr_scheduler.LinearLR(optimizer, start_factor=1.0, end_factor=5e-2, total_iters=opt.n_epochs + opt.n_epochs_decay)
    if policy == "exponential":
        return lr_scheduler.ExponentialLR(optimizer, 0.99)
    if policy == "step":
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.5)
    if policy == "plateau":
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.5, threshold=1e-4, patience=5, min_lr=1e-7)
    if policy == "cosine":
        return lr_scheduler.CosineAnnealingLR(optimizer, T_max=opt.n_epochs, eta_min=0)
    # (the reference RETURNS this exception instead of raising it, so an unknown policy only fails later, at the first
    #  scheduler.step(): a bug not worth mirroring)
    raise NotImplementedError(f"learning rate policy [{policy}] is not implemented (one of {', '.join(POLICIES)})")


def update_learning_rate(schedulers, policy, metric=None):
    """base_model.py:209-218: every scheduler one step (``plateau``: with the metric)."""
    for s in schedulers:
        if policy == "plateau":
            s.step(metric)
        else:
            s.step()
