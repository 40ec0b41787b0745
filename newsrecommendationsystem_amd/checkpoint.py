"""Checkpoints in the reference's format (src/train.py:54-64,144-159,264-279;
src/evaluate.py:281-288).

A checkpoint is the dict torch.save writes at src/train.py:266-277:
  {'model_state_dict': NRMS.state_dict(), 'optimizer_state_dict':
   Adam.state_dict(), 'step': int, 'early_stop_value': -val_auc}
where early_stop_value is a numpy float64 (the negated AUC of evaluate()).
Module parameter names are the reference's (nrms.py), and HipAdam keeps
torch.optim.Adam's state keys and param_group fields, so files interchange
in both directions: a reference checkpoint resumes on the HIP path and a HIP
checkpoint resumes under the reference's train.py.

Loading never unpickles arbitrary objects: torch.load(weights_only=True) with
only numpy's scalar reconstruction allowed (the early_stop_value entry).
"""
import os

import numpy as np
import torch


def _safe_numpy_globals():
    try:
        from numpy._core.multiarray import scalar
    except ImportError:                       # numpy < 2
        from numpy.core.multiarray import scalar
    return [scalar, np.dtype, type(np.dtype(np.float64))]


def load(path, map_location="cpu"):
    """The checkpoint dict, read with torch.load(weights_only=True)."""
    with torch.serialization.safe_globals(_safe_numpy_globals()):
        return torch.load(path, map_location=map_location, weights_only=True)


def load_model(path, device="cpu"):
    """The checkpoint's model on `device`, in eval mode: an NRMS whose
    num_words and word_embedding_dim are the saved embedding table's shape
    (the other hyper-parameters are NRMSConfig's). A state dict that holds
    news_encoder.text_encoders.title.word_embedding.weight is a
    MODEL_NAME=Exp1 checkpoint and gives an Exp1, with num_words,
    num_categories and num_clicked_news_a_user from the saved shapes."""
    from .config import Exp1Config, NRMSConfig
    from .nrms import NRMS
    state = load(path)["model_state_dict"]
    pre = "news_encoder.text_encoders.title."
    if pre + "word_embedding.weight" in state:
        from .exp1 import Exp1
        V, D = state[pre + "word_embedding.weight"].shape
        C, E = state["news_encoder.element_encoders.category.embedding.weight"].shape
        n_clicked = state["user_encoder.position_embedding"].shape[0]
        cfg = type("CheckpointCfg", (Exp1Config,), dict(
            num_words=int(V), word_embedding_dim=int(D), num_categories=int(C), category_embedding_dim=int(E),
            num_clicked_news_a_user=int(n_clicked)))
        model = Exp1(cfg)
        model.load_state_dict(state)
        return model.to(torch.device(device)).eval()
    V, D = state["news_encoder.word_embedding.weight"].shape
    cfg = type("CheckpointCfg", (NRMSConfig,), dict(num_words=int(V), word_embedding_dim=int(D)))
    model = NRMS(cfg)
    model.load_state_dict(state)
    return model.to(torch.device(device)).eval()


def latest_checkpoint(directory):
    """Path of the ckpt-{step}.pth with the largest step, or None
    (src/train.py:54-64)."""
    if not os.path.isdir(directory):
        return None
    found = {}
    for name in os.listdir(directory):
        try:
            found[int(name.split(".")[-2].split("-")[-1])] = name
        except (IndexError, ValueError):
            continue
    if not found:
        return None
    return os.path.join(directory, found[max(found)])


def resume(path, model, optimizer=None):
    """Load model (and optimizer) state as src/train.py:144-159 does; returns
    (step, early_stop_value). The model keeps its device: tensors are mapped
    onto it, and the optimizer's moments follow its parameters' devices.

    The file is read onto the CPU: load_state_dict copies the parameters onto
    the model's device, and Optimizer.load_state_dict moves exp_avg /
    exp_avg_sq to each parameter's device but leaves the 'step' counters where
    they were loaded -- on the CPU, as the reference keeps them (a CUDA step
    tensor would cost HipAdam a device-to-host sync per parameter per step)."""
    ck = load(path, map_location="cpu")
    model.load_state_dict(ck["model_state_dict"])
    if optimizer is not None:
        optimizer.load_state_dict(ck["optimizer_state_dict"])
        for st in optimizer.state.values():
            step = st.get("step")
            if torch.is_tensor(step) and step.device.type != "cpu":
                st["step"] = step.cpu()
    return int(ck["step"]), ck["early_stop_value"]


def rank_path(path, rank):
    """ckpt-{t}.rank{r}.pth beside ckpt-{t}.pth: client r's own optimizer
    state of a federated fit (fit.fit(fed=...)). latest_checkpoint skips such
    names: their second-to-last dotted part is no step number."""
    root, ext = os.path.splitext(path)
    return f"{root}.rank{int(rank)}{ext}"


def save_rank(path, rank, optimizer, step):
    """Client `rank` > 0's file beside the checkpoint `path`: its optimizer
    state and the step, nothing else (the model is rank 0's file's)."""
    torch.save({"optimizer_state_dict": optimizer.state_dict(), "step": int(step)}, rank_path(path, rank))


def _load_optimizer(optimizer, state):
    optimizer.load_state_dict(state)
    for st in optimizer.state.values():
        step = st.get("step")
        if torch.is_tensor(step) and step.device.type != "cpu":
            st["step"] = step.cpu()


def resume_rank(path, rank, model, optimizer):
    """resume() for client `rank` > 0 of a federated fit: the model from
    `path`, the optimizer from rank_path(path, rank) when that file exists and
    holds the same step, else from `path` (rank 0's moments: the world size
    changed, or the file was lost). Returns (step, early_stop_value, whether
    the rank's own file was used)."""
    ck = load(path, map_location="cpu")
    model.load_state_dict(ck["model_state_dict"])
    own = None
    if os.path.exists(rank_path(path, rank)):
        own = load(rank_path(path, rank), map_location="cpu")
        if int(own["step"]) != int(ck["step"]):
            own = None
    _load_optimizer(optimizer, (own or ck)["optimizer_state_dict"])
    return int(ck["step"]), ck["early_stop_value"], own is not None


def save(path, model, optimizer, step, early_stop_value):
    """src/train.py:266-277."""
    torch.save({"model_state_dict": model.state_dict(),
                "optimizer_state_dict": optimizer.state_dict(),
                "step": int(step),
                "early_stop_value": np.float64(early_stop_value)}, path)
