"""Training on a MIND directory: the reference's train() (src/train.py:67-279)
with everything under the loop on the device.

The reference's loop assembles [B, 1+K+N, L] int64 batches on the host
(BaseDataset + DataLoader), launches torch's loss kernels and reads
loss.item() back every step. At ~3 ms per HIP training step that shape is what
the GPU would wait on, so here

  * the training set stays on the device as row indices (TrainSet: the corpus
    titles once, and per sample C + N int32 rows into them);
  * nrms_train_batch_gather assembles a batch in one launch into buffers the
    TrainSet owns (csrc/fit.hip);
  * nrms_xent_class0 computes CrossEntropyLoss against class 0 and its
    gradient in one launch and leaves the loss in a device log, read back only
    when a log line or a validation needs it;
  * the sample order of an epoch is uploaded once per epoch.

What is kept from the reference: shuffled drop_last batches, validation every
num_batches_validate steps, EarlyStopping(patience 5) on -AUC, ckpt-{step}.pth
on improvement, resume from the latest checkpoint (checkpoint.py: the
reference's file format). What differs: the order of epoch e is a pure
function of (seed, e, S) and the dropout seed one of (seed, step), so a resumed
run continues the trajectory of an uninterrupted one; and a resumed run stops
at the same total step count (the reference restarts its counter and trains
num_epochs more).
"""
import csv
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _native as N
from . import checkpoint as CK
from . import train as TR
from .data import NUM_CLICKED


class TrainSet:
    """behaviors_parsed.tsv as row indices (src/dataset.py:64-85).

    titles  int64 [n_news + 1, L]: the corpus titles and one final all-zero
            row, the padding title;
    rows    int32 [S, C + N]: per sample the C candidate rows in file order
            (positive first), then the first N history items left-padded with
            the padding row.
    Every line must list the same number of candidates (the reference's default
    collate stacks them); the `clicked` column is read and ignored
    (src/train.py:205 trains against class 0). ValueError on a ragged line or
    an unknown news id. Host copies (titles_host, rows_host) stay available
    for the host-assembled baseline route of fit()."""

    def __init__(self, behaviors_parsed_path, corpus, num_clicked=NUM_CLICKED, device="cpu"):
        n_news, L = corpus.titles.shape
        pad = n_news
        rows = []
        C = None
        with open(behaviors_parsed_path, newline="") as f:
            rd = csv.reader(f, delimiter="\t", quoting=csv.QUOTE_NONE)
            header = next(rd)
            cc, cn = header.index("clicked_news"), header.index("candidate_news")
            header.index("clicked")          # must be there; its values are not used
            for k, row in enumerate(rd):
                try:
                    cand = [corpus.index[x] for x in row[cn].split()]
                    hist = [corpus.index[x] for x in row[cc].split()[:num_clicked]]
                except KeyError as e:
                    raise ValueError(f"{behaviors_parsed_path}: line {k + 2} names unknown news id {e}") from None
                if C is None:
                    C = len(cand)
                if len(cand) != C:
                    raise ValueError(f"{behaviors_parsed_path}: line {k + 2} has {len(cand)} candidates, "
                                     f"the lines before it {C}")
                rows.append(cand + [pad] * (num_clicked - len(hist)) + hist)
        if not rows:
            raise ValueError(f"{behaviors_parsed_path}: no samples")
        if n_news + 1 > np.iinfo(np.int32).max:
            raise ValueError("more news than int32 rows address")
        self.C, self.N, self.L = C, int(num_clicked), int(L)
        self.rows_host = np.asarray(rows, dtype=np.int32).reshape(len(rows), C + self.N)
        self.titles_host = np.concatenate([corpus.titles, np.zeros((1, L), np.int64)])
        self.max_id = int(self.titles_host.max()) if self.titles_host.size else 0
        self.min_id = int(self.titles_host.min()) if self.titles_host.size else 0
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.titles = torch.from_numpy(self.titles_host).to(self.device)
        self.rows = torch.from_numpy(self.rows_host).to(self.device)
        self._out = {}

    def __len__(self):
        return self.rows_host.shape[0]

    def host_batch(self, sample_idx):
        """(cand [B, C, L], clicked [B, N, L]) int64 CPU tensors by numpy
        indexing of the host copies; an index outside [0, S) gives all-zero
        titles for that sample, as the device kernel writes them."""
        idx = np.asarray(torch.as_tensor(sample_idx).cpu(), dtype=np.int64).reshape(-1)
        S = len(self)
        ok = (idx >= 0) & (idx < S)
        r = self.rows_host[np.where(ok, idx, 0)].astype(np.int64)
        r[~ok] = self.titles_host.shape[0] - 1
        g = self.titles_host[r]
        return (torch.from_numpy(np.ascontiguousarray(g[:, :self.C])),
                torch.from_numpy(np.ascontiguousarray(g[:, self.C:])))

    def batch(self, sample_idx):
        """(cand [B, C, L], clicked [B, N, L]) int64 on the set's device. On a
        GPU: one nrms_train_batch_gather launch into two buffers this set owns
        (one pair per batch size; the next call with the same B overwrites
        them), nothing allocated, no host synchronisation when sample_idx is
        already an int64 tensor on the device."""
        if self.device.type != "cuda":
            return self.host_batch(sample_idx)
        idx = torch.as_tensor(sample_idx).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        B = idx.numel()
        out = self._out.get(B)
        if out is None:
            out = self._out[B] = (torch.empty(B, self.C, self.L, dtype=torch.int64, device=self.device),
                                  torch.empty(B, self.N, self.L, dtype=torch.int64, device=self.device))
        N.call("nrms_train_batch_gather", N.ptr(self.titles), self.titles.shape[0], self.L, N.ptr(self.rows),
               len(self), self.C, self.N, N.ptr(idx), B, N.ptr(out[0]), N.ptr(out[1]),
               N.stream_handle(self.device))
        return out


def xent_class0(logits, dlogits=None, loss_out=None):
    """nrms_xent_class0 on a contiguous fp32 CUDA [B, C]: (loss [1] device
    tensor, dlogits [B, C]). loss_out: a one-element view to write the loss to
    (the fit loop's device loss log)."""
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2):
        raise TypeError("xent_class0 needs a contiguous float32 CUDA [B, C] tensor")
    B, C = logits.shape
    if dlogits is None:
        dlogits = torch.empty_like(logits)
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=logits.device)
    N.call("nrms_xent_class0", N.ptr(logits), B, C, N.ptr(dlogits), N.ptr(loss_out), N.stream_handle(logits.device))
    return loss_out, dlogits


def epoch_order(seed, epoch, S):
    """The sample order of epoch `epoch`: a permutation of range(S) that is a
    pure function of (seed, epoch, S) (int64 CPU tensor)."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch) * 7919 + 12345) & (2 ** 62 - 1))
    return torch.randperm(int(S), generator=g)


def dropout_seed(seed, step):
    """Dropout seed of global step `step` (from 1): a function of (seed, step)
    alone, so a resumed run draws the masks the uninterrupted run would."""
    return ((int(seed) & 0x3fffffff) << 31) | (int(step) & 0x7fffffff)


def batch_of_step(step, S, batch_size):
    """(epoch, first position, one past the last) of global step `step` (from
    1) in its epoch's order; S // batch_size steps per epoch (drop_last)."""
    per = S // batch_size
    e, k = divmod(step - 1, per)
    return e, k * batch_size, (k + 1) * batch_size


class EarlyStopping:
    """src/train.py:27-51: called with -AUC; strict <."""

    def __init__(self, patience=5):
        self.patience = patience
        self.counter = 0
        self.best_loss = np.inf

    def __call__(self, val_loss):
        if val_loss < self.best_loss:
            self.counter = 0
            self.best_loss = val_loss
            return False, True
        self.counter += 1
        return self.counter >= self.patience, False


@dataclass
class FitResult:
    start_step: int = 0            # step of the checkpoint resumed from (0: fresh)
    step: int = 0                  # last global step run
    steps: int = 0                 # steps run by this call
    seconds: float = 0.0           # wall time of the loop, validation included
    losses: torch.Tensor = None    # float32 CPU [steps]: every step's loss
    aucs: list = field(default_factory=list)   # [(step, auc)] of this call's validations
    best_auc: float = None         # incl. the resumed checkpoint's
    checkpoint: str = None         # last checkpoint written, else the one resumed from
    early_stopped: bool = False
    best_loss: float = np.inf      # EarlyStopping's value (-best AUC)
    optimizer: object = None

    @property
    def last_auc(self):
        return self.aucs[-1][1] if self.aucs else None

    @property
    def steps_per_s(self):
        return self.steps / self.seconds if self.seconds > 0 else float("nan")


class _DirValidator:
    """evaluate(model, val_dir, max_count=200000)'s AUC (src/train.py:248-250)
    with the split read and indexed once (EvalPlan), scored each time."""

    def __init__(self, directory, num_clicked):
        self.directory, self.num_clicked, self.plan = directory, num_clicked, None

    def __call__(self, model):
        from .data import load_behaviors, read_news_parsed
        from .evaluate import EvalPlan, nan_sums, reduce_means, score_plan
        if self.plan is None:
            corpus = read_news_parsed(os.path.join(self.directory, "news_parsed.tsv"))
            imps = load_behaviors(os.path.join(self.directory, "behaviors.tsv"))
            self.plan = EvalPlan(corpus, imps, max_count=200000, num_clicked=self.num_clicked)
        _, metrics = score_plan(model, self.plan)
        return reduce_means(*nan_sums(metrics))[0]


def fit(model, train_set, val=None, *, checkpoint_dir=None, seed=0, steps=None, batch_size=None,
        validate=None, log=print, host_batches=False):
    """The reference's train() on `train_set` (module docstring). `validate`:
    callable model -> AUC; else `val`: a directory with news_parsed.tsv and
    behaviors.tsv; neither: no validation, no checkpoints. `steps`: how many
    steps this call runs (default: up to num_epochs * S // batch_size in
    total, counting a resumed checkpoint's). host_batches: the baseline route
    on a GPU (batches assembled on the host and uploaded, torch's loss
    kernels, loss.item() every step). Returns a FitResult."""
    cfg = model.config
    dev = next(model.parameters()).device
    B = int(batch_size if batch_size is not None else cfg.batch_size)
    S = len(train_set)
    if B <= 0 or S // B == 0:
        raise ValueError(f"batch size {B} leaves no full batch of {S} samples (drop_last)")
    if train_set.min_id < 0 or train_set.max_id >= cfg.num_words:
        raise IndexError(f"token ids {train_set.min_id}..{train_set.max_id} outside num_words = {cfg.num_words}")
    hip = dev.type == "cuda" and getattr(cfg, "hip_train", True)
    if host_batches and not hip:
        raise ValueError("host_batches is the baseline of the HIP route (a GPU model with hip_train)")
    if dev.type == "cuda" and not host_batches and train_set.device != dev:
        raise ValueError(f"train set on {train_set.device}, model on {dev}")
    if hip:
        from . import train_hip
    optimizer = TR.make_optimizer(model)
    early = EarlyStopping()
    res = FitResult(optimizer=optimizer)
    if checkpoint_dir is not None:
        os.makedirs(checkpoint_dir, exist_ok=True)
        path = CK.latest_checkpoint(checkpoint_dir)
        if path is not None:
            log(f"Load saved parameters in {path}")
            res.start_step, esv = CK.resume(path, model, optimizer)
            early(esv)                                    # src/train.py:148
            res.checkpoint = path
    if validate is None and val is not None:
        validate = _DirValidator(val, cfg.num_clicked_news_a_user)
    if steps is None:
        steps = max(0, cfg.num_epochs * S // B - res.start_step)
    model.train()

    show, every = int(cfg.num_batches_show_loss), int(cfg.num_batches_validate)
    losses = []
    loss_log = torch.zeros(max(show, 1), dtype=torch.float32, device=dev) if not host_batches else None
    pending = []                    # slots of loss_log not yet copied back, in step order

    def flush():
        if pending:
            host = loss_log.cpu()
            losses.extend(host[pending].tolist())
            pending.clear()

    epoch, order = None, None
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    t = res.start_step
    for t in range(res.start_step + 1, res.start_step + steps + 1):
        e, a, b = batch_of_step(t, S, B)
        if e != epoch:
            epoch, order = e, epoch_order(seed, e, S)
            if dev.type == "cuda" and not host_batches:
                order = order.to(dev)
        if host_batches:
            cand, clk = train_set.host_batch(order[a:b])
            logits = train_hip.forward_hip(model, cand.to(dev), clk.to(dev), seed=dropout_seed(seed, t))
            loss = TR.loss_fn(logits)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            losses.append(loss.item())
        else:
            if len(pending) == loss_log.numel():
                flush()
            slot = t % loss_log.numel()
            cand, clk = train_set.batch(order[a:b])
            if hip:
                logits = train_hip.forward_hip(model, cand, clk, seed=dropout_seed(seed, t))
                _, dlogits = xent_class0(logits.detach(), loss_out=loss_log[slot:slot + 1])
                optimizer.zero_grad()
                logits.backward(dlogits)
                optimizer.step()
            else:
                loss_log[slot].copy_(TR.train_step(model, optimizer, cand, clk))
            pending.append(slot)
        if show > 0 and t % show == 0:
            flush()
            log(f"batches {t}, current loss {losses[-1]:.4f}, average loss: {np.mean(losses):.4f}, "
                f"latest average loss: {np.mean(losses[-256:]):.4f}")        # src/train.py:241-244
        if validate is not None and every > 0 and t % every == 0:
            flush()
            model.eval()
            auc = float(validate(model))
            model.train()
            res.aucs.append((t, auc))
            log(f"batches {t}, validation AUC: {auc:.4f}")
            stop, better = early(-auc)
            if stop:
                log("Early stop.")
                res.early_stopped = True
                break
            if better and checkpoint_dir is not None:
                res.checkpoint = os.path.join(checkpoint_dir, f"ckpt-{t}.pth")
                CK.save(res.checkpoint, model, optimizer, t, -auc)
    flush()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    res.seconds = time.perf_counter() - t0
    res.steps = len(losses)
    res.step = t
    res.losses = torch.tensor(losses, dtype=torch.float32)
    res.best_loss = early.best_loss
    res.best_auc = None if not np.isfinite(early.best_loss) else float(-early.best_loss)
    return res
