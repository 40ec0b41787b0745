"""Case tables and fp64 / fp32 references of the per-kernel inference tests
(tests/test_gpu_infer_kernels.py on the GPU, tests/test_infer_kernel_cases_cpu.py
for the references and tables themselves). Pure torch / numpy on the CPU.

The stage and eval entry points of include/nrms_hip.h, one at a time: the dot
scorers, the per-impression metrics, the raw-exp self-attention, the additive
scores / pooling, the staged Q|K|V projection and the embedding gather. Every
input is drawn from a seeded CPU generator in fp64 and rounded to fp32; a
reference is the plain formula on those rounded values, in fp64 (o_64) and in
fp32 (o_32). What a kernel would receive from an earlier stage (qkv rows,
scores) is drawn directly or is that stage's fp64 reference rounded to fp32,
never another HIP kernel's output.

The tolerance is train_kernel_cases.errors with cap_rel = CAP_FORWARD:
e_hip <= max(4 e_32, 1e-6 n, floor_abs). Two project numbers stand in for the
1e-6 n term, both passed as floor_abs:
  - GEMM outputs under the split-f16 x3 arithmetic (22-bit operands by
    design): 2e-6 n, the per-row bound of tests/test_gpu_parity.py;
  - mixed-sign dot products: |(D + 16) 2^-24 sum_i |a_i b_i||, which is
    tests/topk_cases.tolerance.
"""
import math

import numpy as np
import torch

from tests.train_kernel_cases import (CAP_FORWARD, D, DK, H, Q, _split_heads, encoder_weights, errors, f32, gen,
                                      mhsa_inputs, mhsa_scores, randn, uniform)

ERR_PREFIX = "infer-kernel-error"
F16X3_REL = 2e-6   # tests/test_gpu_parity.py: the split-f16 x3 GEMM rows against fp64


def report(kernel, case, name, o_hip, o_64, o_32, floor_abs=0.0):
    """One printed line per output (the format of train_kernel_cases.report);
    returns whether the output meets the rule. Callers assert after printing
    every output of a case."""
    e_hip, e_32, n, bound, which = errors(o_hip, o_64, o_32, floor_abs, CAP_FORWARD)
    d = n if n > 0 else 1.0
    ratio = e_hip / e_32 if e_32 > 0 else (0.0 if e_hip == 0 else float("inf"))
    finite = bool(torch.isfinite(o_hip).all())
    print(f"{ERR_PREFIX}: {kernel} {case} {name} e_hip/n={e_hip / d:.3e} e_32/n={e_32 / d:.3e} "
          f"ratio={ratio:.2f} bound={which}")
    return finite and e_hip <= bound


def f16x3_floor(o_64):
    return F16X3_REL * float(torch.linalg.vector_norm(o_64.double().reshape(-1)))


# ---------------------------------------------------------------------------
# 1. Dot scorers: nrms_score (score.hip), nrms_score_pairs and the scores of
# nrms_rank_impressions (wave_dot, nrms_common.hpp:97-119).
DOT_D_SCALAR = (1, 3, 7, 301)                  # D % 4 != 0: the scalar lanes (nrms_common.hpp:116, score.hip:33)
DOT_D_LANES = (4, 252, 256, 260, 300)          # D / 4 = 1, 63, 64, 65, 75 against the 64 lanes (nrms_common.hpp:108,114)
DOT_D_CACHE = (1020, 1024, 1028, 1280, 2052)   # kDotUserRegs = 4 float4 per lane, D <= 1024 cached (nrms_common.hpp:76):
#   1020 the last cached float4 short of full, 1024 the cache exactly, 1028 the first float4 read from memory
#   (nrms_common.hpp:114), 1280 a whole fifth pass, 2052 two memory passes and a one-lane tail
DOT_D = DOT_D_SCALAR + DOT_D_LANES + DOT_D_CACHE
DOT_NEWS, DOT_USERS = 12, 3
DOT_COUNTS = (1, 3, 4, 5, 9)                   # pairs per call / candidates per impression: 4 waves per block (eval.hip:31,114)
DOT_KINDS = ("same_sign", "randn")
SCORE_B, SCORE_C = 3, 4                        # nrms_score's [B, C, D] view of the 12 news rows
SCORE_LAYOUT_D = (300, 7)
SCORE_LAYOUTS = ("contiguous", "stride_c+4", "stride_c+1", "base+1", "stride_u0", "C1", "B1")


def dot_inputs(Dd, kind, seed=1101):
    """news [12, D], user [3, D]. same_sign: uniform [0.5, 1.5], a well
    conditioned dot; randn: mixed signs."""
    g = gen(seed + 10 * Dd + DOT_KINDS.index(kind))
    if kind == "same_sign":
        return uniform(g, DOT_NEWS, Dd, lo=0.5, hi=1.5), uniform(g, DOT_USERS, Dd, lo=0.5, hi=1.5)
    return randn(g, DOT_NEWS, Dd), randn(g, DOT_USERS, Dd)


def dot_pairs():
    """The impressions of lengths DOT_COUNTS as one pair list: (news_idx [22],
    user_idx [22], offsets [6], imp_user [5])."""
    offsets = np.concatenate([[0], np.cumsum(DOT_COUNTS)]).astype(np.int64)
    n = int(offsets[-1])
    news_idx = (np.arange(n, dtype=np.int64) * 5 + 3) % DOT_NEWS   # 5 is coprime to 12: every row appears
    imp_user = (np.arange(len(DOT_COUNTS), dtype=np.int64) + 1) % DOT_USERS
    user_idx = np.repeat(imp_user, DOT_COUNTS)
    return (torch.from_numpy(news_idx), torch.from_numpy(user_idx), torch.from_numpy(offsets),
            torch.from_numpy(imp_user))


def dot_ref(a, b):
    """Row-wise <a, b> in the dtype of the arguments ([..., D] broadcastable)."""
    return (a * b).sum(-1)


def dot_floor_rows(a, b):
    """(D + 16) 2^-24 sum_i |a_i b_i| per dot, in fp64 (tests/topk_cases.tolerance)."""
    return (a.shape[-1] + 16) * 2.0 ** -24 * (a.double().abs() * b.double().abs()).sum(-1)


def dot_floor(a, b, kind):
    """floor_abs of one case: the norm of the per-dot bounds for mixed signs, none for same-sign inputs."""
    return float(torch.linalg.vector_norm(dot_floor_rows(a, b).reshape(-1))) if kind == "randn" else 0.0


def wave_dot_emulated(nv, uv):
    """wave_dot's summation order on the CPU in fp32 (numpy): lane l takes the
    float4s (D % 4 == 0) or the floats l, l + 64, ... in one FMA chain, then the
    xor tree. fmaf(a, b, c) is round32(a b + c) with the product exact in fp64."""
    nv, uv = np.asarray(nv, np.float32), np.asarray(uv, np.float32)
    Dd = nv.shape[0]
    acc = np.zeros(64, np.float32)
    if Dd % 4 == 0:
        for i in range(Dd // 4):
            for t in range(4):
                k = 4 * i + t
                acc[i % 64] = np.float32(np.float64(nv[k]) * np.float64(uv[k]) + np.float64(acc[i % 64]))
    else:
        for k in range(Dd):
            acc[k % 64] = np.float32(np.float64(nv[k]) * np.float64(uv[k]) + np.float64(acc[k % 64]))
    o = 32
    while o:
        acc = (acc + acc[np.arange(64) ^ o]).astype(np.float32)
        o >>= 1
    return float(acc[0])


# ---------------------------------------------------------------------------
# 2. nrms_impression_metrics (impression_metrics_kernel, eval.hip:154-216)
METRIC_N = (1, 2, 5, 6, 10, 11, 63, 64, 65, 129)   # one wave per impression: n on both sides of 64 lanes and of 2 x 64
#   (eval.hip:167,180); 5|6 and 10|11: the nDCG cut-offs (eval.hip:194-195, 204-207)
METRIC_RANKS = (1, 5, 6, 10, 11)                   # and n: the single positive's rank
METRIC_NIMP = (1, 4, 5)                            # 4 waves per block (eval.hip:158)
METRIC_OFFSET0 = 7
NONFINITE_N, NONFINITE_POS = 129, (0, 63, 64, 128)   # beyond lane 63: the second and third trip of eval.hip:167


def ranks_ref(s):
    """1-based rank of every candidate: its position in np.argsort(s, kind="stable")[::-1]."""
    order = np.argsort(np.asarray(s), kind="stable")[::-1]
    r = np.empty(len(order), np.int64)
    r[order] = np.arange(1, len(order) + 1)
    return r


def metrics_ref(y, s):
    """[AUC, MRR, nDCG@5, nDCG@10] in fp64 from the stable ranks (ties: larger
    index first); AUC is oracle.metrics.auc_score. Header contract: non-finite
    score or empty: four NaN; no positive: four NaN; no negative: AUC NaN, MRR
    = mean(1 / rank), nDCG = 1."""
    from oracle.metrics import auc_score
    y, s = np.asarray(y), np.asarray(s, np.float32)
    nan4 = [float("nan")] * 4
    if len(s) == 0 or not np.isfinite(s).all():
        return nan4
    pos = y == 1
    npos = int(pos.sum())
    if npos == 0:
        return nan4
    r = ranks_ref(s)[pos].astype(np.float64)
    out = [float("nan") if npos == len(s) else auc_score(y, s), float(np.sum(1.0 / r) / npos)]
    for k in (5, 10):
        dcg = float(np.sum(1.0 / np.log2(r[r <= k] + 1.0)))
        idcg = float(np.sum(1.0 / np.log2(np.arange(1, min(npos, k) + 1) + 1.0)))
        out.append(dcg / idcg)
    return out


def _distinct_scores(rng, n):
    """n distinct fp32 scores in random order."""
    return rng.permutation(np.linspace(-2.0, 3.0, n).astype(np.float32) if n > 1 else np.float32([0.25]))


def metric_cases(seed=1201):
    """[(name, labels int32 [n], scores float32 [n])]: every n of METRIC_N with
    one positive at rank 1, 5, 6, 10, 11, n; positive counts 0, 1, 5, 6, 10, 11,
    n - 1, n; and the tie cases (a positive tied with a negative on either
    side of it, all scores equal, +0 against -0, ties among positives across
    the rank-5 and rank-10 cut-offs)."""
    rng = np.random.default_rng(seed)
    out = []
    for n in METRIC_N:
        for rank in sorted({r for r in METRIC_RANKS + (n,) if r <= n}):
            s = _distinct_scores(rng, n)
            y = (ranks_ref(s) == rank).astype(np.int32)
            out.append((f"n{n}-pos@{rank}", y, s))
        for p in sorted({c for c in (0, 1, 5, 6, 10, 11, n - 1, n) if 0 <= c <= n}):
            s = _distinct_scores(rng, n)
            y = np.zeros(n, np.int32)
            y[rng.permutation(n)[:p]] = 1
            out.append((f"n{n}-npos{p}", y, s))
        if n < 2:
            continue
        # a positive tied with a negative: the larger index ranks first
        for first in (1, 0):
            s = _distinct_scores(rng, n)
            i, j = sorted(rng.permutation(n)[:2].tolist())
            s[j] = s[i]
            y = (rng.random(n) < 0.3).astype(np.int32)
            y[i], y[j] = first, 1 - first
            out.append((f"n{n}-tie-pos{'lo' if first else 'hi'}", y, s))
        y = (np.arange(n) % 3 == 1).astype(np.int32)
        out.append((f"n{n}-all-equal", y, np.full(n, 0.75, np.float32)))
        z = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        out.append((f"n{n}-zeros", rng.permutation(y), z))
        if n >= 11:
            # ranks 4..7 share one score and ranks 9..12 another; positives and negatives in both groups
            s = _distinct_scores(rng, n)
            order = np.argsort(s, kind="stable")[::-1]
            s[order[3:7]] = s[order[3]]
            s[order[8:12]] = s[order[8]]
            y = np.zeros(n, np.int32)
            y[order[[0, 3, 5, 6, 8, 10]]] = 1
            if n > 12:
                y[order[11]] = 1
            out.append((f"n{n}-ties-across-cuts", y, s))
    return out


def nonfinite_cases(seed=1202):
    rng = np.random.default_rng(seed)
    out = []
    for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for pos in NONFINITE_POS:
            s = _distinct_scores(rng, NONFINITE_N)
            s[pos] = v
            out.append((f"{name}@{pos}", (rng.random(NONFINITE_N) < 0.3).astype(np.int32), s))
    return out


def pack_impressions(cases, offset0=0, empty_every=0):
    """Concatenate cases into (scores [offset0 + sum n], labels, offsets
    [n_imp + 1], rows): scores / labels before offset0 are NaN / 1 (never
    owned by an impression); with empty_every > 0 an empty impression follows
    every empty_every-th case. rows[i]: index of case i's impression."""
    scores, labels = [np.full(offset0, np.nan, np.float32)], [np.ones(offset0, np.int32)]
    offsets, rows, at = [offset0], [], offset0
    for i, (_, y, s) in enumerate(cases):
        rows.append(len(offsets) - 1)
        scores.append(np.asarray(s, np.float32))
        labels.append(np.asarray(y, np.int32))
        at += len(s)
        offsets.append(at)
        if empty_every and (i + 1) % empty_every == 0:
            offsets.append(at)
    return (np.concatenate(scores), np.concatenate(labels), np.asarray(offsets, np.int64), np.asarray(rows))


# ---------------------------------------------------------------------------
# 3. nrms_self_attention (attention.hip): four LDS instances and the long kernel
ATT_L = (1, 19, 20, 21, 32, 33, 50, 51, 64, 65, 66, 130)   # launch_mhsa's splits L <= 20 | 32 | 50 | 64 (attention.hip:297-300)
#   and the long kernel past 64 (attention.hip:292); 19 | 20 | 21 ... each side of every split; 130: tasks = 1950 over 256
#   threads and more than two 64-key runs
ATT_NSEQ = (1, 3)
ATT_REGIMES = ("wide", "vanishing", "recheck")
ATT_REGIME_L = (20, 32, 50, 64, 65)            # the last length of each instance and the first of the long kernel
ATT_REGIME_NSEQ = 3
ATT_ADDRESS_L = (20, 65)
# Seeds of train_kernel_cases.mhsa_inputs whose vanishing scores stay in [-25, -11] at these lengths
# (test_attention_regimes checks every one).
ATT_SEEDS = {(32, "vanishing"): 507, (50, "vanishing"): 507, (64, "vanishing"): 533, (65, "vanishing"): 529}
RECHECK_HEAD = 7
RECHECK_LOG2 = 123.0                           # the fp64 row sum aimed at: inside [2^121, 2^125], past kExpRecheck = 2^120
#   (nrms_common.hpp:55) and finite in fp32


def attention_seed(L, regime):
    return ATT_SEEDS.get((L, regime), 506)


def recheck_constant(L):
    """c with L exp(DK c^2 / sqrt(DK)) = 2^123, rounded to fp32: every score of
    the head is sqrt(DK) c^2 (about 82 at L = 20)."""
    return float(np.float32(math.sqrt((RECHECK_LOG2 * math.log(2.0) - math.log(L)) / math.sqrt(DK))))


def attention_inputs(L, n_seq, regime):
    """qkv [n_seq * L, 3 D] (fp32). normal / wide / vanishing: mhsa_inputs.
    recheck: the normal rows with head RECHECK_HEAD's q and k slices set to
    recheck_constant(L), so every row sum of that head is about 2^123: finite
    in fp32, and past kExpRecheck, where the kernels redo the row with ref_exp."""
    if regime != "recheck":
        return mhsa_inputs(L, n_seq, regime, seed=attention_seed(L, regime))[0]
    qkv = mhsa_inputs(L, n_seq, "normal", seed=attention_seed(L, regime))[0].clone()
    c = recheck_constant(L)
    for part in (0, 1):
        qkv[:, part * D + RECHECK_HEAD * DK:part * D + (RECHECK_HEAD + 1) * DK] = c
    return qkv


def attention_ref(qkv, n_seq, L):
    """ctx [n_seq * L, D]: per head e = exp(q k^T / sqrt(d_k)) with no maximum
    subtracted, a = e / (sum e + 1e-8), ctx = a v, heads concatenated."""
    q, k, v = _split_heads(qkv, n_seq, L)
    e = torch.exp(q @ k.transpose(-1, -2) / math.sqrt(DK))
    a = e / (e.sum(-1, keepdim=True) + 1e-8)
    return (a @ v).permute(0, 2, 1, 3).reshape(n_seq * L, D)


def attention_row_sums(qkv, n_seq, L):
    """fp64 row sums Z [n_seq, H, L] of exp(S)."""
    return torch.exp(mhsa_scores(qkv.double(), n_seq, L)).sum(-1)


# ---------------------------------------------------------------------------
# 4. nrms_additive_scores / nrms_additive_pool / nrms_additive_attention
ADD_ROWS = (1, 63, 64, 65, 127, 128, 129, 257)   # the f32 GEMM's 128-row tile (BM, gemm_f32.hip:533) and its 32-row
#   waves: one short tile, one tile + 1, two tiles + 1
ADD_SETS = ("normal", "saturating", "tiny")
ADD_SET_ROWS = 129
ADD_SCALE = {"normal": 0.5, "saturating": 30.0, "tiny": 1e-4}
POOL_L = (1, 2, 63, 64, 65, 130)                 # L > kWave switches the kernel's form (attention.hip:220)
POOL_D = (4, 252, 256, 260, 300)                 # D / 4 against 64 lanes: the column loop's second trip (attention.hip:248, 227)
POOL_NSEQ = (1, 4, 5)                            # 4 waves per block (attention.hip:214)
POOL_SETS = ("normal", "spread", "equal", "neg_inf")
ADD_ATTENTION_SHAPES = ((1, 1), (5, 20), (3, 65), (2, 130))   # (n_seq, L)


def additive_score_inputs(rows, kind="normal", seed=1401):
    return randn(gen(seed + 10 * rows + ADD_SETS.index(kind)), rows, D, scale=ADD_SCALE[kind])


def additive_scores_ref(x, w_add, b_add, q_add):
    """scores [rows] = tanh(x W^T + b) . q."""
    return torch.tanh(x @ w_add.t() + b_add) @ q_add


def pool_inputs(n_seq, L, Dd, kind, seed=1402):
    """x [n_seq, L, D], scores [n_seq, L]."""
    g = gen(seed + 100000 * n_seq + 1000 * L + 10 * Dd + POOL_SETS.index(kind))
    x = randn(g, n_seq, L, Dd)
    if kind == "normal":
        s = randn(g, n_seq, L)
    elif kind == "spread":
        s = uniform(g, n_seq, L, lo=-80.0, hi=80.0)
    elif kind == "equal":
        s = torch.full((n_seq, L), 1.25)
    else:
        s = randn(g, n_seq, L)
        if L > 1:
            s[:, L // 2] = float("-inf")
    return x, s


def pool_ref(x, s):
    """out [n_seq, D] = sum_l softmax_l(s) x_l."""
    return (torch.softmax(s, dim=1).unsqueeze(-1) * x).sum(dim=1)


# ---------------------------------------------------------------------------
# 5. nrms_qkv_project / nrms_qkv_project_ws
PROJ_M = (1, 63, 64, 65, 127, 128, 129, 193)   # 128-row tiles of the f32 GEMM (BM, gemm_f32.hip:464), 64-row tiles of the
#   split-bf16 GEMM (XBM, gemm_f32.hip:227,456) and of the workspace kernel: 193 = 3 x 64 + 1 = 128 + 65
PROJ_IDS_M, PROJ_IDS_ROWS = 129, 40
PROJ_LD_PADDED = 928                           # rows padded to whole 128-B lines (nrms_hip.h: nrms_qkv_row_stride)


def project_inputs(rows, seed=1501):
    return randn(gen(seed + rows), rows, D, scale=0.5)


def project_row_ids(seed=1502):
    """129 ids into 40 rows of x: every row at least twice, and one -1 and one
    V (= 40), both of which give NaN rows."""
    ids = np.random.default_rng(seed).permutation(np.arange(PROJ_IDS_M, dtype=np.int64) % PROJ_IDS_ROWS)
    ids[17], ids[100] = -1, PROJ_IDS_ROWS
    return torch.from_numpy(ids)


def project_ref(x, w):
    """qkv [rows, 3 D] = x [W_Q; W_K; W_V]^T + [b_Q; b_K; b_V] in x's dtype."""
    wcat = torch.cat([w["w_q"], w["w_k"], w["w_v"]], 0).to(x.dtype)
    bcat = torch.cat([w["b_q"], w["b_k"], w["b_v"]], 0).to(x.dtype)
    return x @ wcat.t() + bcat


# ---------------------------------------------------------------------------
# 6. nrms_embedding_gather (gather.hip)
GATHER_D = (1, 4, 7, 299, 301, 304)            # any D != 300: the scalar kernel (gather.hip:61); 299 / 301: more than one
#   trip of its 256-thread column loop (gather.hip:51)
GATHER_TOK = (1, 63, 64, 65, 129)              # kRowsPerBlock = 64 of the float4 kernel (gather.hip:10,19-20)
GATHER_V = 50
GATHER_BAD = (-1, GATHER_V, 2 ** 40)


def gather_inputs(n_tok, Dd, seed=1601):
    """table [V, D] and ids [n_tok]: row 0 and row V - 1 appear whenever there is room, and from 63 tokens on
    three ids are out of range (NaN rows)."""
    g = gen(seed + 1000 * n_tok + Dd)
    table = randn(g, GATHER_V, Dd)
    ids = torch.randint(0, GATHER_V, (n_tok,), generator=g, dtype=torch.int64)
    if n_tok >= 2:
        ids[0], ids[-1] = GATHER_V - 1, 0
    if n_tok >= 63:
        for k, bad in enumerate(GATHER_BAD):
            ids[5 + 20 * k] = bad
    return table, ids


def gather_ref(table, ids):
    """(rows [n_tok, D] with zeros where the id is out of range, valid [n_tok])."""
    valid = (ids >= 0) & (ids < table.shape[0])
    out = torch.zeros(ids.numel(), table.shape[1], dtype=table.dtype)
    out[valid] = table[ids[valid]]
    return out, valid
