"""Files of a pretraining run (reference: pretraining/models/base_model.py:245-466).

  <epoch>_net_<name>.pth     the plain state_dict of network <name> (G, F) on the CPU: ``latest``, ``best_val``, ``iter_<n>`` or the
                             iteration count as <epoch>; keys as the module reports them, so the reference loads our files and we
                             load its files -- written after torch.compile / DataParallel its keys carry ``_orig_mod.`` /
                             ``module.``, which are stripped on load
  latest_train_state.pth     {optimizers, schedulers, scaler, total_iters, epoch, best_evaluation_loss, last_eval_loss}: the state
                             that pairs with the most recent NUMBERED network files, always overwritten
  best_val_loss.txt          the best validation loss so far, one line

Unlike the reference, saving does not move the module to the CPU and back: the parameters stay where the optimizers, and a
captured graph, hold them."""
import os
from collections import OrderedDict

import torch

TRAIN_STATE = "latest_train_state.pth"
BEST_VAL_TXT = "best_val_loss.txt"


def network_path(save_dir, epoch, name):
    return os.path.join(save_dir, "%s_net_%s.pth" % (epoch, name))


def _core(net):
    net = getattr(net, "_orig_mod", net)           # torch.compile
    return getattr(net, "module", net)             # DataParallel


def strip_prefixes(state_dict):
    """Keys without ``module.`` and ``_orig_mod.`` (base_model.py:458-466); plain state_dicts pass through."""
    return OrderedDict((k.replace("module.", "").replace("_orig_mod.", ""), v) for k, v in state_dict.items())


def save_networks(save_dir, epoch, nets):
    """``nets``: {"G": netG, "F": netF}.  One file per network, tensors copied to the CPU."""
    os.makedirs(save_dir, exist_ok=True)
    for name, net in nets.items():
        sd = OrderedDict((k, v.detach().cpu()) for k, v in _core(net).state_dict().items())
        torch.save(sd, network_path(save_dir, epoch, name))


def output_head_keys(net, keys):
    """The keys a partial warm start may leave at their fresh initialisation (base_model.py:267-303): those of the network's
    output head -- ``up_projection.`` where the network has one, else the last parametrised child of its ``model`` Sequential."""
    core = _core(net)
    if hasattr(core, "up_projection"):
        head = "up_projection."
    else:
        seq = getattr(core, "model", None)
        if not isinstance(seq, torch.nn.Sequential):
            return set()
        idxs = [int(n) for n, child in seq.named_children() if any(True for _ in child.parameters(recurse=True))]
        if not idxs:
            return set()
        head = f"model.{max(idxs)}."
    return {k for k in keys if k.replace("module.", "").replace("_orig_mod.", "").startswith(head)}


def _read_state_dict(path, device):
    sd = torch.load(path, map_location=str(device))
    first = next(iter(sd.keys()))
    if "module." in first or "_orig_mod." in first:
        sd = strip_prefixes(sd)
    if hasattr(sd, "_metadata"):
        del sd._metadata
    return sd


def load_network(path, net, device="cpu"):
    """One file into ``net`` (base_model.py:336-388).  A checkpoint that differs from the network ONLY in its output head is loaded
    without it (the head keeps its fresh initialisation); any other mismatch is refused."""
    net = _core(net)
    sd = _read_state_dict(path, device)
    try:
        net.load_state_dict(sd)
        return []
    except RuntimeError as e:
        model = net.state_dict()
        ckpt_keys, model_keys = set(sd), set(model)
        mismatched = sorted(k for k in ckpt_keys & model_keys if sd[k].size() != model[k].size())
        missing, unexpected = sorted(model_keys - ckpt_keys), sorted(ckpt_keys - model_keys)
        offenders = sorted((set(mismatched) | set(missing) | set(unexpected)) - output_head_keys(net, model_keys))
        if offenders:
            raise RuntimeError(f"Refusing to partially load '{path}': the checkpoint does not fit parameters outside the output head: "
                               f"{offenders} -- usually another architecture or configuration.  Load a matching checkpoint or start "
                               f"fresh.  (shape-mismatched={mismatched}, missing_from_ckpt={missing}, unexpected_in_ckpt={unexpected})"
                               ) from e
        for k in ckpt_keys & model_keys:
            if sd[k].size() == model[k].size():
                model[k] = sd[k]
        net.load_state_dict(model)
        left = sorted(set(mismatched) | set(missing))
        print(f"Partial load from '{path}': output-head parameters {left} keep their fresh initialisation; everything else loaded.")
        return left


def load_networks(load_dir, epoch, nets, device="cpu"):
    """``<epoch>_net_<name>.pth`` of ``load_dir`` into every network of ``nets`` (this run's directory on resume, another run's
    for ``--pretrained_name``)."""
    if not nets:
        raise ValueError("found empty model list to load, please double check")
    for name, net in nets.items():
        path = network_path(load_dir, epoch, name)
        print("loading the model from %s" % path)
        load_network(path, net, device)


def load_G_only(ckpt_path, netG, device="cpu"):
    """``--pretrained_G_only_ckpt``: netG from a stand-alone file, strictly; netF keeps its initialisation (base_model.py:390-413)."""
    print("loading netG only from %s" % ckpt_path)
    _core(netG).load_state_dict(_read_state_dict(ckpt_path, device))


def save_training_state(save_dir, optimizers, schedulers, scaler, extras):
    """``extras``: total_iters, epoch, best_evaluation_loss, last_eval_loss."""
    state = {"optimizers": [o.state_dict() for o in optimizers], "schedulers": [s.state_dict() for s in schedulers],
             "scaler": scaler.state_dict() if scaler is not None else None}
    state.update(extras)
    os.makedirs(save_dir, exist_ok=True)
    torch.save(state, os.path.join(save_dir, TRAIN_STATE))


def peek_training_state(save_dir):
    """The train state on the CPU (for ``total_iters`` before any network exists), or None."""
    path = os.path.join(save_dir, TRAIN_STATE)
    return torch.load(path, map_location="cpu") if os.path.exists(path) else None


def load_training_state(save_dir, optimizers, schedulers, scaler=None, device="cpu"):
    """Restores optimizers, schedulers and (when both sides have one) the scaler; returns the extras, or None without a file."""
    path = os.path.join(save_dir, TRAIN_STATE)
    if not os.path.exists(path):
        return None
    print(f"Loading training state from {path}")
    state = torch.load(path, map_location=str(device))
    for o, sd in zip(optimizers, state.get("optimizers", [])):
        o.load_state_dict(sd)
    for s, sd in zip(schedulers, state.get("schedulers", [])):
        s.load_state_dict(sd)
    if state.get("scaler") is not None and scaler is not None:
        scaler.load_state_dict(state["scaler"])
    return {k: v for k, v in state.items() if k not in ("optimizers", "schedulers", "scaler")}


def write_best_val(save_dir, value):
    with open(os.path.join(save_dir, BEST_VAL_TXT), "w") as f:
        f.write(f"{value}")


def read_best_val(save_dir):
    path = os.path.join(save_dir, BEST_VAL_TXT)
    if not os.path.exists(path):
        return None
    with open(path) as f:
        return float(f.readline().rstrip())
