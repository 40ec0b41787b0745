"""Case tables and fp64 references of the per-kernel training tests
(tests/test_gpu_train_kernels.py on the GPU, tests/test_train_kernel_cases_cpu.py
for the references and tables themselves). Pure torch / numpy on the CPU.

Every input is drawn from a seeded CPU generator in fp64 and rounded to fp32;
a reference is the plain formula of one entry point of include/nrms_hip.h
("Training kernels"), evaluated in fp64 on those rounded values. The same
function evaluated in fp32 gives o_32, the fp32 error level the tolerance rule
below is built on. Inputs a kernel receives from an earlier stage (y_tanh,
scores, qkv) are the fp64 reference of that stage rounded to fp32, never the
output of another HIP kernel.
"""
import math

import numpy as np
import torch

D, H, DK, Q = 300, 15, 20, 200

# ---------------------------------------------------------------------------
# The tolerance rule (one place): for an output o,
#   e_hip = |o_hip - o_64|, e_32 = |o_32 - o_64|, n = |o_64|   (Frobenius)
#   e_hip <= max(4 e_32, 1e-6 n, floor_abs)
# 4: margin for another reduction order and the split-bf16 x6 arithmetic over
# the fp32 reference's own error; 1e-6 n: keeps a lucky fp32 reference from
# making the bound vanish; floor_abs: only for outputs that are analytically
# zero or at rounding level, stated per case.
FACTOR_32 = 4.0
REL_FLOOR = 1e-6
ERR_PREFIX = "train-kernel-error"


def _norm(t):
    return float(torch.linalg.vector_norm(t.detach().double().reshape(-1)))


CAP_GRAD, CAP_FORWARD = 1e-4, 1e-5   # the end-to-end bounds of tests/test_gpu_train.py: never looser than these


def errors(o_hip, o_64, o_32, floor_abs=0.0, cap_rel=CAP_GRAD):
    """(e_hip, e_32, n, bound, which term sets the bound)."""
    o_64 = o_64.double()
    e_hip = _norm(o_hip.double().cpu() - o_64)
    e_32 = _norm(o_32.double() - o_64)
    n = _norm(o_64)
    terms = {"4e32": min(FACTOR_32 * e_32, cap_rel * n), "1e-6n": REL_FLOOR * n, "floor": float(floor_abs)}
    which = max(terms, key=terms.get)
    return e_hip, e_32, n, terms[which], which


def report(kernel, case, name, o_hip, o_64, o_32, floor_abs=0.0, cap_rel=CAP_GRAD):
    """Print the one line per output the error file is made of; return whether
    the output meets the rule (callers assert after printing all outputs)."""
    e_hip, e_32, n, bound, which = errors(o_hip, o_64, o_32, floor_abs, cap_rel)
    d = n if n > 0 else 1.0
    ratio = e_hip / e_32 if e_32 > 0 else (0.0 if e_hip == 0 else float("inf"))
    finite = bool(torch.isfinite(o_hip).all())
    print(f"{ERR_PREFIX}: {kernel} {case} {name} e_hip/n={e_hip / d:.3e} e_32/n={e_32 / d:.3e} "
          f"ratio={ratio:.2f} bound={which}")
    return finite and e_hip <= bound


def g0_pattern(*shape):
    """The non-zero fp32 prefill of accumulated (d_*) outputs: exact multiples
    of 2^-10 in [-3, 3] x 2^-10, small against the gradients so the rule stays
    tight, far above the bound so an overwrite instead of an add is caught."""
    n = int(np.prod(shape))
    return (((torch.arange(n) % 7) - 3).float() * 2.0 ** -10).reshape(shape)


def f32(t):
    return t.to(torch.float32)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return f32(torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


def uniform(g, *shape, lo=0.0, hi=1.0):
    return f32(torch.rand(*shape, generator=g, dtype=torch.float64) * (hi - lo) + lo)


def encoder_weights(seed):
    """fp32 parameters of one encoder at nn.Linear's scale (D = 300, H = 15,
    Q = 200), in the field order of nrms_encoder_weights_t."""
    g = gen(seed)
    a = 1.0 / math.sqrt(D)
    w = {}
    for k in ("q", "k", "v"):
        w["w_" + k] = uniform(g, D, D, lo=-a, hi=a)
        w["b_" + k] = uniform(g, D, lo=-a, hi=a)
    w["w_add"] = uniform(g, Q, D, lo=-a, hi=a)
    w["b_add"] = uniform(g, Q, lo=-a, hi=a)
    w["q_add"] = uniform(g, Q, lo=-0.1, hi=0.1)
    return w


WEIGHT_FIELDS = ("w_q", "b_q", "w_k", "b_k", "w_v", "b_v", "w_add", "b_add", "q_add")

# ---------------------------------------------------------------------------
# 1. nrms_dropout: y[i] = x[i] / (1 - p) if u(seed, i) >= p else 0, u the top
# 24 bits of the splitmix64 finaliser of (seed, i) times 2^-24.
DROPOUT_N = (1, 255, 256, 257, 300 * 20 * 3 + 1)
DROPOUT_P = (0.0, 0.2, 0.999)
DROPOUT_SEEDS = (0, 11, 2 ** 64 - 1)
DROPOUT_BAD_P = (-0.1, 1.0, 1.5, float("nan"))

_M64 = (1 << 64) - 1
_GOLD, _C1, _C2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def splitmix64_int(seed, i):
    """The hash on Python integers (the header's words, one index at a time)."""
    z = (seed + _GOLD * (i + 1)) & _M64
    z = ((z ^ (z >> 30)) * _C1) & _M64
    z = ((z ^ (z >> 27)) * _C2) & _M64
    return z ^ (z >> 31)


def dropout_uniform_np(seed, n):
    i = np.arange(n, dtype=np.uint64)
    z = np.uint64(seed) + np.uint64(_GOLD) * (i + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_C1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_C2)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_np(x, p, seed):
    """x: float32 array. Bitwise the kernel's result."""
    x = np.asarray(x, dtype=np.float32)
    p32 = np.float32(p)
    keep = dropout_uniform_np(seed, x.size).reshape(x.shape) >= p32
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return np.where(keep, x * scale, np.float32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------
# 2. nrms_score_backward
SCORE_SHAPES = ((1, 1, 300), (3, 5, 300), (5, 1, 300), (9, 4, 7))


def score_inputs(B, C, Dd, seed=201):
    g = gen(seed + 1000 * B + 10 * C + Dd)
    return randn(g, B, C, Dd), randn(g, B, Dd), randn(g, B, C)


def score_backward_ref(news, user, dl):
    """dnews[b, c, :] = dl[b, c] user[b, :]; duser[b, :] = sum_c dl[b, c] news[b, c, :]."""
    dnews = dl.unsqueeze(-1) * user.unsqueeze(1)
    duser = (dl.unsqueeze(-1) * news).sum(dim=1)
    return dnews, duser


# ---------------------------------------------------------------------------
# 3 / 4. additive attention, train-mode forward and backward
ADDITIVE_FWD_SHAPES = ((1, 1), (3, 17), (5, 13), (4, 20), (2, 64), (65, 1))   # (n_seq, L)
ADDITIVE_FWD_ROWS = (1, 51, 65, 80, 128, 65)                                  # on and off the 64-row tile
ADDITIVE_BWD_SHAPES = ADDITIVE_FWD_SHAPES + ((64, 2), (65, 2), (129, 2))      # reduce_rows_add: 1 pass, 2, last chunk of 1
RED_CHUNK = 64


def reduce_passes(rows):
    """(passes, rows of the last chunk) of reduce_rows_add (train.hip)."""
    if rows <= RED_CHUNK:
        return 1, rows
    return 2, rows - (rows - 1) // RED_CHUNK * RED_CHUNK


def additive_inputs(n_seq, L, seed=301):
    g = gen(seed + 100 * n_seq + L)
    return randn(g, n_seq, L, D, scale=0.5), randn(g, n_seq, D)   # x, dout


def additive_forward_ref(x, w_add, b_add, q_add):
    """y_tanh [n_seq, L, Q] = tanh(x W^T + b), scores [n_seq, L] = y . q,
    out [n_seq, D] = sum_l softmax_l(scores) x_l."""
    y = torch.tanh(x @ w_add.t() + b_add)
    s = y @ q_add
    return y, s, (torch.softmax(s, dim=1).unsqueeze(-1) * x).sum(dim=1)


def additive_backward_ref(x, w_add, q_add, y, s, dout):
    """(dx, d_w_add, d_b_add, d_q_add) of additive_forward_ref's `out`, with
    y_tanh and scores as given inputs (the formulas of train.hip's header)."""
    w = torch.softmax(s, dim=1)
    dw = (x * dout.unsqueeze(1)).sum(-1)
    ds = w * (dw - (w * dw).sum(dim=1, keepdim=True))
    dz = ds.unsqueeze(-1) * q_add * (1 - y * y)
    dx = w.unsqueeze(-1) * dout.unsqueeze(1) + dz @ w_add
    dz2, x2 = dz.reshape(-1, dz.shape[-1]), x.reshape(-1, x.shape[-1])
    return dx, dz2.t() @ x2, dz2.sum(0), (ds.unsqueeze(-1) * y).sum((0, 1))


def additive_floor(L, x, dout, numel):
    """L = 1: softmax of one score is 1, so d_w / d_b / d_q are analytically 0."""
    if L != 1:
        return 0.0
    return 1e-6 * float(dout.abs().max()) * float(x.abs().max()) * math.sqrt(numel)


# ---------------------------------------------------------------------------
# 5. nrms_self_attention_backward
MHSA_L = (1, 2, 19, 20, 21, 50, 64)
MHSA_NSEQ = (1, 3)
MHSA_REGIMES = ("normal", "wide", "vanishing")
MHSA_CASES = tuple((L, n, "normal") for L in MHSA_L for n in MHSA_NSEQ) + tuple(
    (L, n, r) for L in (20, 21) for n in MHSA_NSEQ for r in ("wide", "vanishing"))
MHSA_UNSUPPORTED_L = 65


def mhsa_scores(qkv, n_seq, L):
    """S[n_seq, H, L, L] = q k^T / sqrt(d_k) of qkv[n_seq * L, 3 D]."""
    q, k, _ = _split_heads(qkv, n_seq, L)
    return q @ k.transpose(-1, -2) / math.sqrt(DK)


def _split_heads(qkv, n_seq, L):
    t = qkv.reshape(n_seq, L, 3, H, DK).permute(2, 0, 3, 1, 4)   # [3, n_seq, H, L, DK]
    return t[0], t[1], t[2]


def mhsa_inputs(L, n_seq, regime, seed=506):
    """qkv [n_seq * L, 3 D], dctx [n_seq * L, D] (fp32). normal: |S| <= 5;
    wide: max |S| = 21 (within +-22); vanishing: q in [0.5, 1.5], k = -4 [0.5,
    1.5], every S in [-25, -11] and min Z about 2e-8, so the 1e-8 added to Z
    matters (the seed is one for which all four vanishing cases keep that
    range; test_mhsa_score_regimes checks it)."""
    g = gen(seed + 1000 * L + 10 * n_seq + MHSA_REGIMES.index(regime))
    R = n_seq * L
    v, dctx = randn(g, R, D), randn(g, R, D)
    if regime == "vanishing":
        q = uniform(g, R, D, lo=0.5, hi=1.5)
        k = -4.0 * uniform(g, R, D, lo=0.5, hi=1.5)
    else:
        q, k = randn(g, R, D, scale=0.8), randn(g, R, D, scale=0.8)
        if regime == "wide":
            s = mhsa_scores(torch.cat([q, k, v], dim=1).double(), n_seq, L)
            q = f32(q.double() * (21.0 / float(s.abs().max())))
    return torch.cat([q, k, v], dim=1).contiguous(), dctx


def mhsa_backward_ref(qkv, dctx, n_seq, L):
    """dqkv [n_seq * L, 3 D]: A = E / (Z + 1e-8), E = exp(S) without a maximum
    subtracted; dA = dO V^T; dS = A (dA - rowsum(dA A)) (exact with the 1e-8);
    dV = A^T dO, dQ = dS K / sqrt(dk), dK = dS^T Q / sqrt(dk)."""
    q, k, v = _split_heads(qkv, n_seq, L)
    do = dctx.reshape(n_seq, L, H, DK).permute(0, 2, 1, 3)
    rs = 1.0 / math.sqrt(DK)
    e = torch.exp(q @ k.transpose(-1, -2) * rs)
    a = e / (e.sum(-1, keepdim=True) + 1e-8)
    da = do @ v.transpose(-1, -2)
    dsc = a * (da - (da * a).sum(-1, keepdim=True)) * rs
    parts = (dsc @ k, dsc.transpose(-1, -2) @ q, a.transpose(-1, -2) @ do)   # dq, dk, dv: [n_seq, H, L, DK]
    return torch.stack(parts, 0).permute(1, 3, 0, 2, 4).reshape(n_seq * L, 3 * D)


def mhsa_floor(L, qkv, dctx):
    """L = 1: dq, dk are dA A (1 - A) = O(1e-8 / e), which fp32 rounds to 0."""
    if L != 1:
        return 0.0
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    return (1e-6 * float(dctx.abs().max()) * float(v.abs().max()) *
            max(float(q.abs().max()), float(k.abs().max())) * math.sqrt(q.numel()))


# ---------------------------------------------------------------------------
# 6. nrms_qkv_project_backward
PROJECT_ROWS = (1, 33, 100, 1760, 1761)
TN_TILE, TN_BK, TN_BLOCKS, TN_MAX_SLICES = 64, 32, 4096, 64
PROJECT_SLICES = {1: (1, 1), 33: (2, 1), 100: (4, 4), 1760: (55, 32), 1761: (28, 33)}   # rows: (slices, rows of the last)


def tn_max_slices(N, K):
    """gemm_tn_slices (train.hip)."""
    tiles = ((N + TN_TILE - 1) // TN_TILE) * ((K + TN_TILE - 1) // TN_TILE)
    return max(1, min(TN_MAX_SLICES, (TN_BLOCKS + tiles - 1) // tiles))


def tn_slicing(R, N, K):
    """(rows per slice, slices) of launch_gemm_tn for R rows."""
    z = tn_max_slices(N, K)
    sl = (R + z - 1) // z
    sl = (sl + TN_BK - 1) // TN_BK * TN_BK
    return sl, (R + sl - 1) // sl


def project_inputs(rows, seed=601):
    g = gen(seed + rows)
    return randn(g, rows, D, scale=0.5), randn(g, rows, 3 * D)   # x, dqkv


def project_backward_ref(x, dqkv, w_q, w_k, w_v):
    """dx = dqkv [W_Q; W_K; W_V], d_w_qkv [3D, D] = dqkv^T x, d_b_qkv = column sums."""
    return dqkv @ torch.cat([w_q, w_k, w_v], 0), dqkv.t() @ x, dqkv.sum(0)


# ---------------------------------------------------------------------------
# 7. nrms_embedding_backward(_ws)
EMBED_RUNS = {1: 1, 2: 8, 3: 9, 4: 255, 5: 256, 6: 257, 7: 320, 8: 321, 9: 1024, 10: 1025}   # id: tokens
EMBED_V = (63, 64, 65)
EMBED_D = (300, 4, 324)
EMB_LONG, EMB_SEG, EMB_SW, EMB_PASS_COLS = 256, 64, 16, 320


def embed_ids(V, seed=701):
    """One shuffled batch: the run-length table, 30 % padding (id 0), the
    skipped ids -1, V and 2^40, and id V - 1 once."""
    ids = [i for i, c in EMBED_RUNS.items() for _ in range(c)]
    ids += [-1, V, 2 ** 40, V - 1]
    n_pad = int(round(0.3 / 0.7 * len(ids)))
    ids = np.array(ids + [0] * n_pad, dtype=np.int64)
    return torch.from_numpy(np.random.default_rng(seed).permutation(ids))


def embed_ref(ids, dx, V, table0, padding_idx=0):
    """table0 + index_add of the valid, non-padding tokens in token order, in
    table0's dtype (fp32: the CPU reference's order, bitwise the short runs')."""
    keep = (ids != padding_idx) & (ids >= 0) & (ids < V)
    out = table0.clone()
    out.index_add_(0, ids[keep], dx[keep].to(table0.dtype))
    return out


# ---------------------------------------------------------------------------
# 8. nrms_adam_step(_multi). The C entry points take lr / betas / eps as fp32;
# those rounded values are the hyperparameters of all three computations.
ADAM_N = (1, 255, 256, 257, 1025)
ADAM_STEPS = (1, 2, 1000, 10 ** 6)
ADAM_COUNTS = (1, 32, 33, 65)
ADAM_SIZES = (1, 257, 300, 90000)
ADAM_CHUNK = 32
ADAM_HYPER = tuple(float(np.float32(h)) for h in (1e-3, 0.9, 0.999, 1e-8))   # lr, beta1, beta2, eps


def adam_state(n, seed):
    """(p, g, m, v) fp32. The gradient cycles through order-1 values, exact
    zeros, 1e-20 (g^2 underflows) and order-1e4 values; the first quarter of
    the state is zero (with a zero gradient there the parameter must not move)."""
    g_ = gen(seed)
    p = randn(g_, n)
    grad = randn(g_, n)
    kind = torch.arange(n) % 4
    grad[kind == 1] = 0.0
    grad[kind == 2] = 1e-20
    grad[kind == 3] *= 1e4
    m, v = randn(g_, n, scale=0.1), f32(randn(g_, n).double() ** 2)
    z = torch.arange(n) < max(1, n // 4)
    m[z], v[z] = 0.0, 0.0
    return p, grad, m, v


def adam_ref64(p, g, m, v, step, hyper=ADAM_HYPER):
    """(delta p, exp_avg, exp_avg_sq) in fp64 from fp32 state."""
    lr, b1, b2, eps = hyper
    g, m, v = g.double(), m.double(), v.double()
    m1 = m + (1 - b1) * (g - m)
    v1 = b2 * v + (1 - b2) * g * g
    denom = v1.sqrt() / math.sqrt(1 - b2 ** step) + eps
    return -(lr / (1 - b1 ** step)) * (m1 / denom), m1, v1


def adam_torch(ps, gs, ms, vs, step, dtype, hyper=ADAM_HYPER):
    """torch.optim.Adam(foreach=False) in `dtype` on the CPU from the given
    state; returns lists (delta p, exp_avg, exp_avg_sq)."""
    lr, b1, b2, eps = hyper
    params = [p.to(dtype).clone().requires_grad_(True) for p in ps]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    for q, g, m, v in zip(params, gs, ms, vs):
        q.grad = g.to(dtype).clone()
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.to(dtype).clone(),
                        "exp_avg_sq": v.to(dtype).clone()}
    opt.step()
    return ([q.detach().double() - p.double() for q, p in zip(params, ps)],
            [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params])


def adam_multi_sizes(count, with_empty):
    """Descriptor sizes of one nrms_adam_step_multi call: `count` tensors
    cycling through ADAM_SIZES; with_empty adds a numel == 0 descriptor in the
    middle and one at the end."""
    sizes = [ADAM_SIZES[i % len(ADAM_SIZES)] for i in range(count)]
    if with_empty:
        sizes = sizes[:count // 2] + [0] + sizes[count // 2:] + [0]
    return sizes
