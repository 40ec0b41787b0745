"""Training step of src/train.py and the federated-averaging loop of
BASELINE config 5 (one process per GPU, local Adam steps, parameter
all-reduce over RCCL every E steps).

On a GPU the training step runs the HIP training kernels (train_hip.py:
train-mode forward with dropout, backward, Adam). The functions below are the
reference's own op sequence on ATen autograd: the CPU path, and the GPU
tests' reference for the HIP gradients (tests/test_gpu_train.py). Config 5's
FedAvg exchange: `FedAvg.sync()` averages the 21,955,400 fp32 parameters
(87.8 MB) with one all-reduce. The reference has no federated averaging at all
(SURVEY §0 finding 2), so there is no oracle for the averaged trajectory; the
tests check the exchange itself (every rank ends with the exact mean) and the
single-process step against the CPU restatement's autograd. The loop around
the step (src/train.py:67-279: batches of a MIND directory, validation, early
stopping, checkpoints) is fit.py. The command line `python -m
newsrecommendationsystem_amd.train` is train_cli.py: `DIR` runs fit, and `DIR
--gpus N` runs it federated: one client per rank, FedAvg's exchange (two HIP
launches around the all-reduce, csrc/fedavg.hip) on fit's schedule.

Semantics kept from the reference:
  * dropout p = config.dropout_probability on the embedding output and on the
    MHSA output (src/model/NRMS/news_encoder.py:38-45), identity in eval;
  * raw-exp attention normalisation (multihead_self.py:15-23);
  * CrossEntropyLoss against class 0 = the positive candidate first
    (src/train.py:126,205-206); Adam(lr = config.learning_rate) (:127);
  * nn.Embedding(padding_idx=0): row 0 receives no gradient.
"""
import ctypes
import math

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import _native as N
from .distributed import all_reduce_, broadcast_
from .train_hip import HipAdam


def _mhsa(x, m):
    # src/model/general/attention/multihead_self.py:46-75 (+ :15-23)
    b = x.size(0)
    h, dk = m.num_attention_heads, m.d_k
    q = m.W_Q(x).view(b, -1, h, dk).transpose(1, 2)
    k = m.W_K(x).view(b, -1, h, dk).transpose(1, 2)
    v = m.W_V(x).view(b, -1, h, dk).transpose(1, 2)
    e = torch.exp(torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dk))
    a = e / (e.sum(dim=-1, keepdim=True) + 1e-8)
    return torch.matmul(a, v).transpose(1, 2).contiguous().view(b, -1, h * dk)


def _additive(x, m):
    # src/model/general/attention/additive.py:27-53
    t = torch.tanh(m.linear(x))
    w = F.softmax(torch.matmul(t, m.attention_query_vector), dim=1)
    return torch.bmm(w.unsqueeze(1), x).squeeze(1)


def news_encode_autograd(ne, ids, training=True, masks=None):
    """NewsEncoder.forward (news_encoder.py:27-48) with autograd. masks (m1,
    m2): the two dropouts (news_encoder.py:38-45) are these multiplications
    instead of torch's draw, m1 on the embedding output, m2 on the MHSA
    output, each with ids.numel() rows."""
    if masks is None:
        p = ne.config.dropout_probability
        x = F.dropout(ne.word_embedding(ids), p=p, training=training)
        h = F.dropout(_mhsa(x, ne.multihead_self_attention), p=p, training=training)
    else:
        n, L = ids.shape
        x = ne.word_embedding(ids) * masks[0].view(n, L, -1)
        h = _mhsa(x, ne.multihead_self_attention) * masks[1].view(n, L, -1)
    return _additive(h, ne.additive_attention)


def user_encode_autograd(ue, clicked_vec):
    """UserEncoder.forward (user_encoder.py:15-26) with autograd."""
    return _additive(_mhsa(clicked_vec, ue.multihead_self_attention), ue.additive_attention)


def forward_autograd(model, cand_ids, clicked_ids, training=True, masks=None):
    """NRMS.forward (src/model/NRMS/__init__.py:19-48) with autograd: all
    B*(C+N) titles go through the encoder in one call (the reference encodes the
    55 slots one by one; per-title results and the dropout distribution are the
    same). masks (m1, m2): dropout as explicit multiplicative masks over the
    titles in the HIP step's order [candidates B*C | clicked B*N]
    (train_hip.hip_dropout_masks), whatever `training` says."""
    ne, ue = model.news_encoder, model.user_encoder
    dev = ne.word_embedding.weight.device
    cand = cand_ids.to(dev)
    clk = clicked_ids.to(dev)
    B, C, L = cand.shape
    n_clicked = clk.shape[1]
    vec = news_encode_autograd(ne, torch.cat([cand.reshape(B * C, L), clk.reshape(B * n_clicked, L)]),
                               training, masks)
    D = vec.shape[-1]
    cand_vec = vec[:B * C].view(B, C, D)
    clk_vec = vec[B * C:].view(B, n_clicked, D)
    user = user_encode_autograd(ue, clk_vec)
    return torch.bmm(cand_vec, user.unsqueeze(-1)).squeeze(-1)


def loss_fn(logits):
    """CrossEntropyLoss vs class 0 (src/train.py:205-206)."""
    return F.cross_entropy(logits, torch.zeros(logits.shape[0], dtype=torch.long,
                                               device=logits.device))


def backward_step(optimizer, out, grad=None):
    """zero_grad, out.backward(grad), optimizer.step (src/train.py:230-236):
    `out` the loss, or the logits with the loss's gradient `grad`."""
    optimizer.zero_grad()
    out.backward(grad)
    optimizer.step()


def train_step(model, optimizer, cand_ids, clicked_ids):
    """One iteration of the loop body of src/train.py:202-236. On a GPU the
    forward/backward are the HIP training kernels (model.forward_ids in train
    mode -> train_hip.NRMSTrain); on the CPU, ATen autograd."""
    model.train()
    loss = loss_fn(model.forward_ids(cand_ids, clicked_ids))
    backward_step(optimizer, loss)
    return loss.detach()


# FedAvg(native=None) on a GPU: the HIP pack / unpack kernels. Decided by the
# alternated measurement in profiles/fedfit_sync_bench.txt (DESIGN §Federated fit).
NATIVE_SYNC_DEFAULT = True


class FedAvg:
    """Federated averaging of the model parameters over a process group: every
    `every` local steps, one all-reduce of the flattened parameters (RCCL
    over xGMI when the group's backend is "nccl", gloo on CPU), divided by
    the world size. Adam moments stay local (each client keeps its own
    optimizer state, as in FedAvg with client-side adaptive optimisers).

    `flat` holds the parameters in model.parameters() order, contiguous.
    native: True moves them with two HIP launches (nrms_params_pack before the
    all-reduce, nrms_params_unpack_div after it: the division is the correctly
    rounded fp32 one, numpy.float32(sum) / numpy.float32(world)); False is one
    torch copy_ per parameter each way and div_ (the only route on the CPU,
    and the baseline of profiles/fedfit_sync_bench.txt); None: native when the
    parameters are on a GPU (NATIVE_SYNC_DEFAULT; a library that does not load
    is then an error at the first sync, not a fall-back). After a native sync `flat`
    holds the sum, after a torch one the mean; at world size 1 both are the
    parameters themselves. The descriptor table stays on the host and is
    rebuilt only when a parameter's data_ptr changes. ValueError: native with
    a parameter that is not a contiguous float32 tensor on flat's device."""

    def __init__(self, model, every, group=None, native=None):
        self.dist = dist
        self.group = group
        self.every = int(every)
        self.params = [p for p in model.parameters()]
        n = sum(p.numel() for p in self.params)
        self.flat = torch.empty(n, dtype=torch.float32, device=self.params[0].device)
        self.world = dist.get_world_size(group)
        self.steps = 0
        if native is None:
            native = self.flat.is_cuda and NATIVE_SYNC_DEFAULT
        elif native and not self.flat.is_cuda:
            raise ValueError("FedAvg(native=True) needs the parameters on a GPU")
        self.native = bool(native)
        self._table = self._table_key = None

    def _descriptors(self):
        """(host array of nrms_flat_tensor_t, n) for the parameters as they lie now."""
        key = tuple(p.data_ptr() for p in self.params)
        if key != self._table_key:
            for p in self.params:
                if not (p.is_contiguous() and p.dtype == torch.float32 and p.device == self.flat.device):
                    raise ValueError("FedAvg's kernels need contiguous float32 parameters on "
                                     f"{self.flat.device} (got {p.dtype}, {p.device}, "
                                     f"contiguous={p.is_contiguous()}, shape {tuple(p.shape)})")
            off, rows = 0, []
            for p in self.params:
                rows.append(N.FlatTensor(p.data_ptr(), p.numel(), off))
                off += p.numel()
            arr = (N.FlatTensor * len(rows))(*rows)
            self._table, self._table_key = (arr, ctypes.cast(arr, ctypes.c_void_p), len(rows)), key
        return self._table[1], self._table[2]

    def _pack(self):
        if self.native:
            tab, n = self._descriptors()
            N.call("nrms_params_pack", tab, n, N.ptr(self.flat), N.stream_handle(self.flat.device))
            return
        off = 0
        for p in self.params:
            k = p.numel()
            self.flat[off:off + k].copy_(p.detach().reshape(-1))
            off += k

    def _unpack(self, divisor):
        if self.native:
            tab, n = self._descriptors()
            N.call("nrms_params_unpack_div", tab, n, N.ptr(self.flat), ctypes.c_float(divisor),
                   N.stream_handle(self.flat.device))
            # written through raw pointers: bump the version counters, as HipAdam does
            torch.autograd.graph.increment_version(self.params)
            return
        if divisor is not None:
            self.flat.div_(divisor)
        off = 0
        for p in self.params:
            k = p.numel()
            p.copy_(self.flat[off:off + k].view_as(p))
            off += k

    @torch.no_grad()
    def sync(self):
        """pack -> all-reduce -> unpack / world: three device operations on
        the native route, 19 + 1 + 1 + 19 on the torch one."""
        self._pack()
        all_reduce_(self.flat, self.group)
        self._unpack(self.world)

    @torch.no_grad()
    def broadcast(self, src=0):
        """Every rank takes rank `src`'s parameters (bitwise): pack, broadcast
        of `flat`, unpack with divisor 1. A CUDA `flat` under gloo goes through
        host memory, as distributed.all_reduce_ does."""
        self._pack()
        broadcast_(self.flat, src, self.group)
        self._unpack(1 if self.native else None)

    def step(self):
        """Call after each local optimizer step; syncs every `every` steps."""
        self.steps += 1
        if self.every > 0 and self.steps % self.every == 0:
            self.sync()
            return True
        return False


def make_optimizer(model):
    """Adam(lr = config.learning_rate) (src/train.py:127): the HIP update
    (train_hip.HipAdam, same state keys) on a GPU, torch.optim.Adam on CPU."""
    if next(model.parameters()).is_cuda:
        return HipAdam(model.parameters(), lr=model.config.learning_rate)
    return torch.optim.Adam(model.parameters(), lr=model.config.learning_rate)


def synthetic_train_batches(seed, n_batches, B, V, C=3, N=50, L=20, device="cpu"):
    """MIND-shaped training batches (src/dataset.py:64-85 contract): 1 positive
    + K negatives per row (positive first), history left-padded with zero
    titles."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n_batches):
        ids = torch.randint(1, V, (B, C + N, L), generator=g)
        lens = torch.randint(5, L + 1, (B, C + N, 1), generator=g)
        ids = torch.where(torch.arange(L)[None, None] < lens, ids, torch.zeros_like(ids))
        hist = torch.randint(1, N + 1, (B, 1), generator=g)
        pad = torch.arange(N)[None] < (N - hist)
        clk = torch.where(pad[:, :, None], torch.zeros_like(ids[:, C:]), ids[:, C:])
        out.append((ids[:, :C].contiguous().to(device), clk.contiguous().to(device)))
    return out


if __name__ == "__main__":
    from .train_cli import _main
    _main()
