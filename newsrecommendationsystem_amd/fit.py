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
  * the sample order of an epoch is uploaded once per epoch;
  * ImpressionSet keeps a raw behaviors.tsv per impression instead, and
    nrms_train_batch_sample_gather draws each sample's K negatives in the
    gather launch, as a counter-based hash of (seed, epoch, sample): new
    negatives every epoch, no per-epoch table, nothing uploaded.

What is kept from the reference: shuffled drop_last batches, validation every
num_batches_validate steps, EarlyStopping(patience 5) on -AUC, ckpt-{step}.pth
on improvement, resume from the latest checkpoint (checkpoint.py: the
reference's file format). What differs: the order of epoch e is a pure
function of (seed, e, S) and the dropout seed one of (seed, step), so a resumed
run continues the trajectory of an uninterrupted one; and a resumed run stops
at the same total step count (the reference restarts its counter and trains
num_epochs more).

fit(fed=train.FedAvg(...)) is the same loop as one client of a federation
(BASELINE config 5): each rank trains on the samples of the users it owns and
the models are averaged on a schedule that is a function of the step alone
(sync_due); validation is sharded by user, checkpoints are per rank (fit's
docstring; DESIGN §Federated fit).
"""
import csv
import ctypes
import os
import time
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.distributed as dist

from . import _native as N
from . import checkpoint as CK
from . import train as TR
from . import train_hip
from .config import NRMSConfig
from .data import NUM_CLICKED, BehaviorsTable, load_behaviors, read_news_parsed, write_behaviors_parsed
from .distributed import shard_impressions, user_rank
from .evaluate import EvalPlan, cut_impressions, evaluate_plan
from .splits import index_split


class _TitleRowSet:
    """What the two training sets share: the corpus titles with the all-zero
    padding title as their last row (titles_host, titles, min_id, max_id), the
    device (a bare "cuda" is the current device), the batch shape C, N, L, and
    batch()'s output buffers. A subclass uploads its own row tables and issues
    its gather call in _gather."""

    def __init__(self, corpus, C, num_clicked, device):
        n_news, L = corpus.titles.shape
        if n_news + 1 > np.iinfo(np.int32).max:
            raise ValueError("more news than int32 rows address")
        self.C, self.N, self.L = int(C), int(num_clicked), int(L)
        self.titles_host = np.concatenate([corpus.titles, np.zeros((1, L), np.int64)])
        self.max_id = int(self.titles_host.max()) if self.titles_host.size else 0
        self.min_id = int(self.titles_host.min()) if self.titles_host.size else 0
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._out = {}

    def _upload(self, *names):
        for name in names:
            setattr(self, name, torch.from_numpy(getattr(self, name + "_host")).to(self.device))

    def batch(self, sample_idx, *key):
        """(cand [B, C, L], clicked [B, N, L]) int64 on the set's device. On a
        GPU: one launch of the set's gather kernel into two buffers this set
        owns (one pair per batch size; the next call with the same B overwrites
        them), nothing allocated, no host synchronisation when sample_idx is
        already an int64 tensor on the device."""
        if self.device.type != "cuda":
            return self.host_batch(sample_idx, *key)
        idx = torch.as_tensor(sample_idx).to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        B = idx.numel()
        out = self._out.get(B)
        if out is None:
            out = self._out[B] = (torch.empty(B, self.C, self.L, dtype=torch.int64, device=self.device),
                                  torch.empty(B, self.N, self.L, dtype=torch.int64, device=self.device))
        self._gather(idx, B, out, *key)
        return out

    def _host_gather(self, rows):
        """(cand [B, C, L], clicked [B, N, L]) int64 CPU tensors of the title
        rows int64 [B, C + N]; -1 marks a title the device kernel writes as
        zeros."""
        g = self.titles_host[np.where(rows >= 0, rows, 0)]
        g[rows < 0] = 0
        return (torch.from_numpy(np.ascontiguousarray(g[:, :self.C])),
                torch.from_numpy(np.ascontiguousarray(g[:, self.C:])))


class TrainSet(_TitleRowSet):
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
    for the host-assembled baseline route of fit(). users: the `user` column,
    one name per sample (None when the file has no such column; only a
    federated fit, which shards by user, needs it)."""

    def __init__(self, behaviors_parsed_path, corpus, num_clicked=NUM_CLICKED, device="cpu"):
        pad = len(corpus.titles)
        rows = []
        C = None
        with open(behaviors_parsed_path, newline="") as f:
            rd = csv.reader(f, delimiter="\t", quoting=csv.QUOTE_NONE)
            header = next(rd)
            cc, cn = header.index("clicked_news"), header.index("candidate_news")
            header.index("clicked")          # must be there; its values are not used
            cu = header.index("user") if "user" in header else None
            users = [] if cu is not None else None
            for k, row in enumerate(rd):
                if users is not None:
                    users.append(row[cu])
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
        super().__init__(corpus, C, num_clicked, device)
        self.rows_host = np.asarray(rows, dtype=np.int32).reshape(len(rows), C + self.N)
        self.users = users
        self._upload("titles", "rows")

    def __len__(self):
        return self.rows_host.shape[0]

    def host_batch(self, sample_idx):
        """(cand [B, C, L], clicked [B, N, L]) int64 CPU tensors by numpy
        indexing of the host copies; an index outside [0, S) gives all-zero
        titles for that sample, as the device kernel writes them."""
        idx = np.asarray(torch.as_tensor(sample_idx).cpu(), dtype=np.int64).reshape(-1)
        ok = (idx >= 0) & (idx < len(self))
        rows = self.rows_host[np.where(ok, idx, 0)].astype(np.int64)
        rows[~ok] = -1
        return self._host_gather(rows)

    def _gather(self, idx, B, out):
        N.call("nrms_train_batch_gather", N.ptr(self.titles), self.titles.shape[0], self.L, N.ptr(self.rows),
               len(self), self.C, self.N, N.ptr(idx), B, N.ptr(out[0]), N.ptr(out[1]),
               N.stream_handle(self.device))


MAX_SAMPLED_NEGATIVES = 15          # the sampler keeps 16 hash slots per sample (16 s + j)
_U64 = (1 << 64) - 1


def _mix64(x):
    """The splitmix64 finaliser (stream.mix) on a uint64 array, wrapping."""
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mix64(x):
    """_mix64 of one Python int, mod 2^64."""
    return int(_mix64(np.array([int(x) & _U64], dtype=np.uint64))[0])


def sampler_base(seed, epoch):
    """mix(mix(uint64(seed)) + uint64(epoch)): the key of one epoch's draws."""
    return mix64((mix64(int(seed) & _U64) + (int(epoch) & _U64)) & _U64)


def draw_positions(seed, epoch, s, n, k):
    """The sampler of nrms_train_batch_sample_gather on the host (numpy, all
    arithmetic uint64 and wrapping): int64 [B, k], row b the positions, among
    n[b] negatives, of the k draws of sample s[b] in epoch `epoch`: a uniform
    ordered k-subset without replacement, a function of (seed, epoch, s) alone.

        base = mix(mix(seed) + epoch)
        r    = ((mix(base + 16 s + j) >> 32) * (n - j)) >> 32     in [0, n - j)
        for p in ascending order of the positions chosen before: r += (r >= p)

    -1 where the kernel writes zeros: draws j >= n (and a position that n >=
    2^32 would let wrap past n)."""
    s = np.asarray(s, dtype=np.int64).reshape(-1)
    n = np.broadcast_to(np.asarray(n, dtype=np.int64), s.shape)
    B, k = s.size, int(k)
    if not 0 <= k <= MAX_SAMPLED_NEGATIVES:
        raise ValueError(f"K = {k} outside 0..{MAX_SAMPLED_NEGATIVES}")
    out = np.full((B, k), -1, dtype=np.int64)
    su, nu = s.astype(np.uint64), n.astype(np.uint64)
    key = np.uint64(sampler_base(seed, epoch)) + np.uint64(16) * su
    chosen = np.zeros((B, k), dtype=np.uint64)            # columns [0, j): ascending
    for j in range(k):
        h = _mix64(key + np.uint64(j))
        r = ((h >> np.uint64(32)) * (nu - np.uint64(j))) >> np.uint64(32)
        for c in range(j):
            r = r + (r >= chosen[:, c]).astype(np.uint64)
        ok = (n > j) & (r < nu)
        out[ok, j] = r[ok].astype(np.int64)
        chosen[:, j] = r
        chosen[:, :j + 1].sort(axis=1)
    return out


class ImpressionSet(_TitleRowSet):
    """A labelled raw behaviors.tsv as a training set whose negatives are drawn
    anew for every (seed, epoch): what TrainSet holds per sample, kept per
    impression.

    A sample is one positive click; samples are ordered by impression, then by
    candidate position.
      titles    int64 [n_news + 1, L]  corpus titles + the all-zero padding title
      pos_row   int32 [S]              corpus row of sample s's clicked article
      pos_imp   int32 [S]              its impression
      neg_off   int64 [I + 1], neg_rows int32 [T]
                                       CSR of each impression's label-0
                                       candidates, in file order
      imp_hist  int32 [I]              impression -> distinct history string
      hist_rows int32 [H, N]           first N history items, left-padded with
                                       the padding row (as TrainSet)
    (each also as *_host numpy copies). The positives of an impression with
    fewer than K negatives are not samples (the reference's balancing drops
    incomplete groups, src/data_preprocess.py:55-68); n_dropped counts them.
    ValueError: K outside 0..15, an unknown news id, a label other than 0/1, no
    sample left.

    On purpose not the reference: every positive draws its own K of ALL the
    impression's negatives (draw_positions), so two positives of one impression
    may share a negative, and no positive is dropped because the negatives ran
    out; the reference deals one shuffled negative list out across the
    positives, once, offline."""

    _TABLES = ("titles", "pos_row", "pos_imp", "neg_off", "neg_rows", "imp_hist", "hist_rows")

    def __init__(self, behaviors_path, corpus, k=None, num_clicked=NUM_CLICKED, device="cpu"):
        K = int(NRMSConfig.negative_sampling_ratio if k is None else k)
        if not 0 <= K <= MAX_SAMPLED_NEGATIVES:
            raise ValueError(f"K = {K} outside 0..{MAX_SAMPLED_NEGATIVES}")
        try:
            split = index_split(corpus, load_behaviors(behaviors_path), num_clicked)
        except KeyError as e:
            raise ValueError(f"{behaviors_path}: unknown news id {e}") from None
        cand = split.cand
        labels = np.asarray(split.labels, dtype=np.int64)
        counts = np.asarray(split.counts, dtype=np.int64)
        if ((labels != 0) & (labels != 1)).any():
            bad = int(labels[(labels != 0) & (labels != 1)][0])
            raise ValueError(f"{behaviors_path}: label {bad}, a training split needs 0/1 labels")
        I = counts.size
        imp_of = np.repeat(np.arange(I, dtype=np.int64), counts)
        neg = labels == 0
        n_neg = np.bincount(imp_of[neg], minlength=I).astype(np.int64)
        keep = ~neg & (n_neg[imp_of] >= K)
        self.n_dropped = int((~neg).sum() - keep.sum())
        if not keep.any():
            raise ValueError(f"{behaviors_path}: no samples (no positive in an impression with >= {K} negatives)")
        if cand.size > np.iinfo(np.int32).max or I > np.iinfo(np.int32).max:
            raise ValueError("more candidates or impressions than int32 addresses")
        super().__init__(corpus, 1 + K, num_clicked, device)
        self.K = K
        self.pos_row_host = cand[keep].astype(np.int32)
        self.pos_imp_host = imp_of[keep].astype(np.int32)
        self.neg_off_host = np.concatenate([[0], np.cumsum(n_neg)]).astype(np.int64)
        self.neg_rows_host = cand[neg].astype(np.int32)
        self.imp_hist_host = np.asarray(split.imp_user, dtype=np.int32)
        self.hist_rows_host = np.ascontiguousarray(split.hist_rows, dtype=np.int32).reshape(-1, self.N)
        self._upload(*self._TABLES)
        self._ids, self._imps = corpus.ids, split.impressions           # names, for export_epoch
        self._seed = self._epoch = None

    @property
    def users(self):
        """Each sample's user: its impression's."""
        u = self._imps.users() if isinstance(self._imps, BehaviorsTable) else [im.user for im in self._imps]
        return [u[i] for i in self.pos_imp_host.tolist()]

    def __len__(self):
        return self.pos_row_host.shape[0]

    @property
    def device_bytes(self):
        return sum(getattr(self, n).numel() * getattr(self, n).element_size() for n in self._TABLES)

    def begin_epoch(self, seed, epoch):
        """The (seed, epoch) that batch / host_batch draw with when a call
        names none: fit() calls this when an epoch begins."""
        self._seed, self._epoch = int(seed), int(epoch)

    def _key(self, seed, epoch):
        seed = self._seed if seed is None else seed
        epoch = self._epoch if epoch is None else epoch
        if seed is None or epoch is None:
            raise ValueError("ImpressionSet draws per (seed, epoch): pass them or call begin_epoch first")
        return int(seed), int(epoch)

    def _sample_tables(self, sample_idx):
        """Per sample of the batch, with the kernel's checks: (sample valid,
        clamped sample, impression valid, clamped impression, negatives'
        offset, negatives' count (0 where neg_off is unusable))."""
        idx = np.asarray(torch.as_tensor(sample_idx).cpu(), dtype=np.int64).reshape(-1)
        ok_s = (idx >= 0) & (idx < len(self))
        s = np.where(ok_s, idx, 0)
        i = self.pos_imp_host[s].astype(np.int64)
        ok_i = ok_s & (i >= 0) & (i < self.imp_hist_host.shape[0])
        i = np.where(ok_i, i, 0)
        o0, o1 = self.neg_off_host[i], self.neg_off_host[i + 1]
        ok_o = ok_i & (o0 >= 0) & (o0 <= o1) & (o1 <= self.neg_rows_host.shape[0])
        return idx, ok_s, s, ok_i, i, np.where(ok_o, o0, 0), np.where(ok_o, o1 - o0, 0)

    def draws(self, seed, epoch, sample_idx):
        """int64 [B, K]: the positions, within the negative list of each
        sample's impression, that (seed, epoch) draws (draw_positions); -1
        where the batch gets zeros instead."""
        idx, _, _, _, _, _, n = self._sample_tables(sample_idx)
        return draw_positions(seed, epoch, idx, n, self.K)

    def _rows(self, sample_idx, seed, epoch):
        """int64 [B, C + N] title rows of the batch, -1 where the kernel
        writes zeros."""
        idx, ok_s, s, ok_i, i, o0, n = self._sample_tables(sample_idx)
        rows = np.full((idx.size, self.C + self.N), -1, dtype=np.int64)
        rows[:, 0] = np.where(ok_s, self.pos_row_host[s], -1)
        if self.K:
            pos = draw_positions(seed, epoch, idx, n, self.K)
            got = pos >= 0
            at = np.where(got, o0[:, None] + pos, 0)
            rows[:, 1:self.C] = np.where(got, self.neg_rows_host[at] if self.neg_rows_host.size else -1, -1)
        h = self.imp_hist_host[i].astype(np.int64)
        ok_h = ok_i & (h >= 0) & (h < self.hist_rows_host.shape[0])
        if self.N and self.hist_rows_host.shape[0]:
            rows[:, self.C:] = np.where(ok_h[:, None], self.hist_rows_host[np.where(ok_h, h, 0)], -1)
        rows[(rows < 0) | (rows >= self.titles_host.shape[0])] = -1
        return rows

    def host_batch(self, sample_idx, seed=None, epoch=None):
        """(cand [B, C, L], clicked [B, N, L]) int64 CPU tensors: the numpy
        mirror of nrms_train_batch_sample_gather, its zeros included."""
        return self._host_gather(self._rows(sample_idx, *self._key(seed, epoch)))

    def batch(self, sample_idx, seed=None, epoch=None):
        """_TitleRowSet.batch with this set's (seed, epoch), or begin_epoch's: on
        a GPU one nrms_train_batch_sample_gather launch (draw + gather)."""
        return super().batch(sample_idx, *self._key(seed, epoch))

    def _gather(self, idx, B, out, seed, epoch):
        N.call("nrms_train_batch_sample_gather", N.ptr(self.titles), self.titles.shape[0], self.L,
               N.ptr(self.pos_row), N.ptr(self.pos_imp), self.pos_row.shape[0], N.ptr(self.neg_off),
               self.imp_hist.shape[0], N.ptr(self.neg_rows), self.neg_rows.shape[0], N.ptr(self.imp_hist),
               N.ptr(self.hist_rows), self.hist_rows.shape[0], self.K, self.N, N.ptr(idx), B,
               ctypes.c_uint64(seed & _U64), epoch, N.ptr(out[0]), N.ptr(out[1]), N.stream_handle(self.device))

    def materialize(self, seed, epoch):
        """int32 [S, C + N]: the row table a TrainSet would hold for this
        epoch's draw (the padding row where the kernel writes zeros)."""
        rows = self._rows(np.arange(len(self)), seed, epoch)
        rows[rows < 0] = self.titles_host.shape[0] - 1
        return rows.astype(np.int32)

    def export_epoch(self, path, seed, epoch):
        """Write the epoch's samples as a behaviors_parsed.tsv
        (data.write_behaviors_parsed): what TrainSet and the reference's
        BaseDataset read."""
        rows = self.materialize(seed, epoch)
        pad = self.titles_host.shape[0] - 1
        ids = self._ids
        write_behaviors_parsed(path, self.users,
                               [[ids[r] for r in h if r != pad] for h in rows[:, self.C:].tolist()],
                               [[ids[r] for r in c] for c in rows[:, :self.C].tolist()],
                               [[1] + [0] * self.K] * len(self))


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


def client_seed(seed, rank):
    """Seed of federated client `rank`: `seed` itself for rank 0 (a federation
    of one is the plain fit), else mix64(mix64(seed) + rank) mod 2^62: the
    client's epoch orders and dropout masks are epoch_order(client_seed, e,
    S_r) and dropout_seed(client_seed, t)."""
    if int(rank) == 0:
        return int(seed)
    return mix64((mix64(int(seed) & _U64) + int(rank)) & _U64) & (2 ** 62 - 1)


def sample_owners(train_set, world):
    """int64 [S]: the client that owns each sample of `train_set`, its user's
    distributed.user_rank. ValueError when the set carries no users (a
    behaviors_parsed.tsv without the `user` column)."""
    users = train_set.users
    if users is None:
        raise ValueError("a federated fit shards the samples by user: behaviors_parsed.tsv has no `user` column")
    owner = {}
    return np.fromiter((owner[u] if u in owner else owner.setdefault(u, user_rank(u, world)) for u in users),
                       dtype=np.int64, count=len(users))


def _client(train_set, seed=0, rank=0, world=None):
    """What client `rank` of `world` trains on: (rank, world, its samples
    int64 [S_r] ascending, [S_0, .., S_{world-1}], client_seed(seed, rank),
    the set's sample count); every rank computes all of it from the users it
    loaded, no collective. world None: the one client of a plain fit (no
    users needed; samples and sizes None)."""
    if world is None:
        return 0, 1, None, None, client_seed(seed, 0), len(train_set)
    owners = sample_owners(train_set, world)
    return (rank, world, np.flatnonzero(owners == rank).astype(np.int64),
            np.bincount(owners, minlength=world).tolist(), client_seed(seed, rank), len(owners))


def client_shard(train_set, rank, world):
    """int64 [S_r]: the samples of `train_set`, ascending, that client `rank`
    of `world` owns."""
    return _client(train_set, 0, rank, world)[2]


def shard_sizes(train_set, world):
    """[S_0, .., S_{world-1}]: every client's sample count."""
    return _client(train_set, 0, 0, world)[3]


def federated_total_steps(num_epochs, S_total, world, batch_size):
    """Global steps of a federated fit: num_epochs epochs of an average shard
    (S_total // world samples), the same number on every rank; each client
    wraps its own epochs (batch_of_step on its S_r)."""
    return num_epochs * (S_total // world) // batch_size


def sync_due(t, every, validate_every, last):
    """Whether the clients average their models after global step t: every
    `every` steps, before a validation (t % validate_every == 0; 0: none) and
    after the last step. A function of t alone, so a resumed run syncs where
    the uninterrupted one does."""
    return (every > 0 and t % every == 0) or (validate_every > 0 and t % validate_every == 0) or t == last


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
    syncs: int = 0                 # federated fit: model averagings of this call (the start broadcast not counted)
    shard_sizes: list = None       # federated fit: every client's sample count

    @property
    def last_auc(self):
        return self.aucs[-1][1] if self.aucs else None

    @property
    def steps_per_s(self):
        return self.steps / self.seconds if self.seconds > 0 else float("nan")


class _DirValidator:
    """evaluate(model, val_dir, max_count=200000)'s AUC (src/train.py:248-250)
    with the split read and indexed once (EvalPlan), scored each time
    (evaluate.evaluate_plan, where evaluate() ends too).

    sharded (a federated fit; `group` its process group, None: the default
    one): max_count cuts the global impression list first, the plan holds the
    impressions of the users this rank owns (distributed.shard_impressions)
    and evaluate_plan all-reduces the metric sums, so every rank returns the
    same AUC from the same reduced buffer."""

    def __init__(self, directory, num_clicked, group=None, sharded=False, max_count=200000):
        self.directory, self.num_clicked, self.plan = directory, num_clicked, None
        self.group, self.sharded, self.max_count = group, sharded, max_count

    def __call__(self, model):
        if self.plan is None:
            corpus = read_news_parsed(os.path.join(self.directory, "news_parsed.tsv"))
            imps = cut_impressions(load_behaviors(os.path.join(self.directory, "behaviors.tsv")), self.max_count)
            if self.sharded:
                self.group = dist.group.WORLD if self.group is None else self.group
                imps = shard_impressions(imps, dist.get_rank(self.group), dist.get_world_size(self.group))
            self.plan = EvalPlan(corpus, imps, num_clicked=self.num_clicked)
        return evaluate_plan(model, self.plan, self.group if self.sharded else None)[0]


def _resume(checkpoint_dir, model, optimizer, early, fed, rank, say, log):
    """Continue from the latest checkpoint of `checkpoint_dir`, if it has one:
    (its step, its path), else (0, None). Rank r > 0 takes its own optimizer
    file, or logs that it has none; EarlyStopping is primed with the
    checkpoint's value (src/train.py:148)."""
    os.makedirs(checkpoint_dir, exist_ok=True)
    if fed is not None and fed.world > 1:
        fed.dist.barrier(group=fed.group)             # files an earlier call of another rank still writes
    path = CK.latest_checkpoint(checkpoint_dir)
    if path is None:
        return 0, None
    say(f"Load saved parameters in {path}")
    if rank == 0:
        start, esv = CK.resume(path, model, optimizer)
    else:
        start, esv, own = CK.resume_rank(path, rank, model, optimizer)
        if not own:
            log(f"rank {rank}: no {os.path.basename(CK.rank_path(path, rank))}, taking rank 0's optimizer state")
    early(esv)
    return start, path


class _LossRing:
    """Every step's loss without a read-back per step: a device route writes
    step t's loss to slot(t) = t % size of the device log `log` (flushing
    first when every slot is marked) and marks the slot; flush() appends the
    marked slots to the host list `losses` with one copy. The host_batches
    route appends to `losses` itself (size 0)."""

    def __init__(self, size, device):
        self.losses = []
        self.log = torch.zeros(size, dtype=torch.float32, device=device)
        self.pending = []               # slots of log not yet copied back, in step order

    def slot(self, t):
        if len(self.pending) == self.log.numel():
            self.flush()
        return t % self.log.numel()

    def mark(self, slot):
        self.pending.append(slot)

    def flush(self):
        if self.pending:
            host = self.log.cpu()
            self.losses.extend(host[self.pending].tolist())
            self.pending.clear()


# The three routes of a step. Each returns step(t, idx): global step t on the
# samples idx of train_set, its loss recorded in `ring`.
def _hip_step(model, optimizer, train_set, ring, cseed):
    """Device batch, HIP forward, loss + gradient in one launch into the ring."""
    def step(t, idx):
        slot = ring.slot(t)
        cand, clk = train_set.batch(idx)
        logits = train_hip.forward_hip(model, cand, clk, seed=dropout_seed(cseed, t))
        _, dlogits = xent_class0(logits.detach(), loss_out=ring.log[slot:slot + 1])
        TR.backward_step(optimizer, logits, dlogits)
        ring.mark(slot)
    return step


def _aten_step(model, optimizer, train_set, ring, cseed):
    """train.train_step (the CPU, or a GPU model without hip_train; torch's dropout)."""
    def step(t, idx):
        slot = ring.slot(t)
        ring.log[slot].copy_(TR.train_step(model, optimizer, *train_set.batch(idx)))
        ring.mark(slot)
    return step


def _host_batches_step(model, optimizer, train_set, ring, cseed):
    """_hip_step's baseline: host-assembled batch, torch's loss kernels, loss.item()."""
    dev = next(model.parameters()).device

    def step(t, idx):
        cand, clk = train_set.host_batch(idx)
        logits = train_hip.forward_hip(model, cand.to(dev), clk.to(dev), seed=dropout_seed(cseed, t))
        loss = TR.loss_fn(logits)
        TR.backward_step(optimizer, loss)
        ring.losses.append(loss.item())
    return step


def _epoch_samples(train_set, cseed, seed, e, S, owned, device):
    """Epoch e's samples in training order: epoch_order(cseed, e, S) on
    `device` (None: the host), through `owned` for a federated client. An
    ImpressionSet is told the (seed, e) it draws with."""
    order = epoch_order(cseed, e, S)
    if hasattr(train_set, "begin_epoch"):
        train_set.begin_epoch(seed, e)
    if device is not None:
        order = order.to(device)
    return order if owned is None else owned[order]           # local -> global sample, on the device


def _validated(t, model, validate, early, res, checkpoint_dir, rank, say):
    """Validation after step t, early stopping (True: stop), and the
    checkpoint on improvement."""
    model.eval()
    auc = float(validate(model))
    model.train()
    res.aucs.append((t, auc))
    say(f"batches {t}, validation AUC: {auc:.4f}")
    stop, better = early(-auc)
    if stop:
        say("Early stop.")
        res.early_stopped = True
    elif better and checkpoint_dir is not None:
        res.checkpoint = os.path.join(checkpoint_dir, f"ckpt-{t}.pth")
        if rank == 0:
            CK.save(res.checkpoint, model, res.optimizer, t, -auc)
        else:
            CK.save_rank(res.checkpoint, rank, res.optimizer, t)
    return stop


def fit(model, train_set, val=None, *, checkpoint_dir=None, seed=0, steps=None, batch_size=None,
        validate=None, log=print, host_batches=False, fed=None):
    """The reference's train() on `train_set` (module docstring): a TrainSet
    (the file's static negatives), or an ImpressionSet, whose negatives epoch
    e draws with the loop's (seed, e) -- told through begin_epoch. `validate`:
    callable model -> AUC; else `val`: a directory with news_parsed.tsv and
    behaviors.tsv; neither: no validation, no checkpoints. `steps`: how many
    steps this call runs (default: up to num_epochs * S // batch_size in
    total, counting a resumed checkpoint's). host_batches: the baseline route
    on a GPU (batches assembled on the host and uploaded, torch's loss
    kernels, loss.item() every step). Returns a FitResult.

    fed (a train.FedAvg over this model): the call is one client of a
    federation, made by every rank of fed's group with the same arguments.
    The client trains on the samples whose user it owns (client_shard: a
    device table of global sample indices, applied to the epoch's order on the
    device; an ImpressionSet still draws with (seed, epoch, global sample)),
    with client_seed(seed, rank) for its epoch orders and dropout masks; t is
    global, the default total federated_total_steps(...) - start step. The
    clients start from rank 0's model (fed.broadcast after an optional resume)
    and average theirs where sync_due says; Adam moments stay local. A `val`
    directory is scored sharded by user with the metric sums all-reduced (a
    `validate` callable must return the same value on every rank), so every
    rank takes the same early-stopping decisions. Rank 0 writes ckpt-{t}.pth
    (the averaged model, its own optimizer state), rank r > 0 its optimizer
    state to ckpt-{t}.rank{r}.pth; a resuming rank without its file takes rank
    0's moments and logs that. Log lines come from rank 0. ValueError: a set
    without users, a shard smaller than the batch (the rank is named),
    host_batches."""
    cfg = model.config
    dev = next(model.parameters()).device
    B = int(batch_size if batch_size is not None else cfg.batch_size)
    if fed is not None and host_batches:
        raise ValueError("host_batches is the single-client baseline route: not with fed")
    rank, world, owned, sizes, cseed, S_total = (                                      # raises without users
        _client(train_set, seed) if fed is None else _client(train_set, seed, fed.dist.get_rank(fed.group), fed.world))
    S = S_total if fed is None else int(owned.size)
    for r, n in enumerate(sizes or ()):                       # every rank raises, naming the short one
        if B > 0 and n < B:
            raise ValueError(f"rank {r}: its shard of {n} samples (of {S_total}, world {world}) is smaller than "
                             f"the batch size {B}")
    if B <= 0 or S // B == 0:
        raise ValueError(f"batch size {B} leaves no full batch of {S} samples (drop_last)")
    if train_set.min_id < 0 or train_set.max_id >= cfg.num_words:
        raise IndexError(f"token ids {train_set.min_id}..{train_set.max_id} outside num_words = {cfg.num_words}")
    hip = dev.type == "cuda" and getattr(cfg, "hip_train", True)
    if host_batches and not hip:
        raise ValueError("host_batches is the baseline of the HIP route (a GPU model with hip_train)")
    if dev.type == "cuda" and not host_batches and train_set.device != dev:
        raise ValueError(f"train set on {train_set.device}, model on {dev}")

    optimizer = TR.make_optimizer(model)
    early = EarlyStopping()
    res = FitResult(optimizer=optimizer, shard_sizes=sizes)
    say = log if rank == 0 else (lambda *_: None)
    if checkpoint_dir is not None:
        res.start_step, res.checkpoint = _resume(checkpoint_dir, model, optimizer, early, fed, rank, say, log)
    if validate is None and val is not None:
        validate = _DirValidator(val, cfg.num_clicked_news_a_user, group=fed.group if fed is not None else None,
                                 sharded=fed is not None)
    if steps is None:
        steps = max(0, federated_total_steps(cfg.num_epochs, S_total, world, B) - res.start_step)
    if fed is not None:
        fed.broadcast(0)                                  # one model, whatever each rank was seeded with
        owned = torch.from_numpy(owned).to(dev)
    model.train()
    show, every = int(cfg.num_batches_show_loss), int(cfg.num_batches_validate)
    ring = _LossRing(0 if host_batches else max(show, 1), dev)
    step = (_host_batches_step if host_batches else _hip_step if hip else _aten_step)(
        model, optimizer, train_set, ring, cseed)

    epoch, order = None, None
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    t = res.start_step
    last = res.start_step + steps
    for t in range(res.start_step + 1, last + 1):
        e, a, b = batch_of_step(t, S, B)
        if e != epoch:
            epoch, order = e, _epoch_samples(train_set, cseed, seed, e, S, owned, None if host_batches else dev)
        step(t, order[a:b])
        if fed is not None and sync_due(t, fed.every, every if validate is not None else 0, last):
            fed.sync()
            res.syncs += 1
        if show > 0 and t % show == 0:
            ring.flush()
            say(f"batches {t}, current loss {ring.losses[-1]:.4f}, average loss: {np.mean(ring.losses):.4f}, "
                f"latest average loss: {np.mean(ring.losses[-256:]):.4f}")        # src/train.py:241-244
        if validate is not None and every > 0 and t % every == 0:
            ring.flush()
            if _validated(t, model, validate, early, res, checkpoint_dir, rank, say):
                break
    ring.flush()
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    res.seconds = time.perf_counter() - t0
    res.steps, res.step = len(ring.losses), t
    res.losses = torch.tensor(ring.losses, dtype=torch.float32)
    res.best_loss = early.best_loss
    res.best_auc = None if not np.isfinite(early.best_loss) else float(-early.best_loss)
    return res
