"""Catalogue-wide recommendation on the HIP path (the end use of the
reference's src/recommend.py:352-386).

The reference ranks 20 randomly drawn news ids per user on the CPU
(create_candidate, src/utils.py:114-123; its comment leaves open how to query
the full set and remove the history). Here every user is ranked against the
whole corpus, with the already-clicked articles removed:

  1. news vectors of the corpus and user vectors of each user's history, as
     evaluate() builds them (evaluate.news_vectors / user_vectors);
  2. one nrms_recommend_topk call: a fused users x news scoring kernel that
     keeps a running top-K per user (csrc/topk.hip) -- the [users, news] score
     matrix is never written.

Entry points: topk (the C call on tensors), recommend_split (every distinct
user of a behaviors split), recommend (one user of a split directory, the
reference's recommend()), and a CLI:

    python -m newsrecommendationsystem_amd.recommend DIR --checkpoint CKPT
        [--k 10] [--user U123] [--out rec.tsv] [--bench]

The web demo around the reference's function (Flask, Elasticsearch) is out of
scope; so is sharding over ranks (users shard exactly as evaluate() shards
them).
"""
import os
import sys

import numpy as np
import torch

from . import _native as N
from .data import BehaviorsTable, load_behaviors, read_news_parsed
from .evaluate import category_args, news_vectors, user_vectors
from .splits import history_rows_of as history_rows   # (corpus, hists, num_clicked): EvalPlan's hist_rows

MAX_K = 256
MAX_EXCLUDE = 256


def topk(news_tab, users, k, exclude=None, n_news=None):
    """(rows int64 [U, k], scores float32 [U, k]) on the vectors' device: for
    each user vector the k best rows of news_tab[:n_news] by (score
    descending, row ascending), rows of exclude[u, :] left out; entries of
    `exclude` outside [0, n_news) are ignored. Fewer than k eligible rows: the
    tail is row -1, score NaN. The contract is nrms_recommend_topk's
    (include/nrms_hip.h).

    n_news defaults to news_tab.shape[0]; pass len(corpus) to leave out the
    PADDED_NEWS row evaluate.news_vectors appends."""
    dev = news_tab.device
    n_news = news_tab.shape[0] if n_news is None else int(n_news)
    if not 0 <= n_news <= news_tab.shape[0]:
        raise ValueError(f"n_news {n_news} outside the table's {news_tab.shape[0]} rows")
    if news_tab.dtype != torch.float32 or users.dtype != torch.float32:
        raise TypeError("topk takes float32 vectors")
    if users.dim() != 2 or news_tab.dim() != 2 or users.shape[1] != news_tab.shape[1]:
        raise ValueError(f"vector shapes {tuple(news_tab.shape)} / {tuple(users.shape)} do not match")
    news_tab, users = news_tab.contiguous(), users.contiguous().to(dev)
    U, D = users.shape
    n_excl = 0
    if exclude is not None:
        exclude = torch.as_tensor(exclude, dtype=torch.int64).to(dev).contiguous()
        if exclude.dim() != 2 or exclude.shape[0] != U:
            raise ValueError(f"exclude must be [{U}, n_excl], got {tuple(exclude.shape)}")
        n_excl = exclude.shape[1]
        if n_excl == 0:
            exclude = None
    k = int(k)
    rows = torch.empty(U, k, dtype=torch.int64, device=dev)
    scores = torch.empty(U, k, dtype=torch.float32, device=dev)
    lib = N.load()
    ws_bytes = lib.nrms_recommend_topk_workspace_size(U, n_news, D, k, n_excl)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    N.call("nrms_recommend_topk", N.ptr(news_tab), n_news, N.ptr(users), U, D, N.ptr(exclude), n_excl, k,
           N.ptr(rows), N.ptr(scores), N.ptr(ws), ws_bytes, N.stream_handle(dev))
    return rows, scores


def _host(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


class Recommendations:
    """recommend_split's result, one entry per distinct user in first-seen
    order: users (ids), rows int64 [U, k] (corpus rows, -1 past the eligible
    ones), news_ids (per user the ranked id list, padding dropped), scores
    float32 [U, k] (the raw click scores, NaN padding) and degrees float64
    [U, k] = (score + 1) / 2, the reference's "recommendation degree"
    (src/recommend.py:339)."""

    def __init__(self, users, rows, scores, corpus_ids):
        self.users = users
        self.rows = rows
        self.scores = scores
        self.degrees = (scores.astype(np.float64) + 1.0) / 2.0
        self.news_ids = [[corpus_ids[r] for r in row if r >= 0] for row in rows.tolist()]

    def __len__(self):
        return len(self.users)

    def above(self, thr=0.5):
        """Per user the ids whose degree exceeds thr (src/recommend.py:385)."""
        return [[nid for nid, d in zip(ids, deg) if d > thr] for ids, deg in zip(self.news_ids, self.degrees)]


def first_lines(impressions):
    """(user ids, history strings) of the split's distinct users in first-seen
    order; a user's history is the one on their first line (the reference's
    .iloc[[0]], src/recommend.py:101,160)."""
    if isinstance(impressions, BehaviorsTable):
        names = impressions.users()
        seen, first = {}, []
        for k, u in enumerate(names):
            if u not in seen:
                seen[u] = len(first)
                first.append(k)
        return [names[k] for k in first], [impressions[k].clicked_news for k in first]
    seen, users, hists = set(), [], []
    for im in impressions:
        if im.user not in seen:
            seen.add(im.user)
            users.append(im.user)
            hists.append(im.clicked_news)
    return users, hists


@torch.no_grad()
def recommend_split(model, corpus, impressions, k=10, exclude_history=True):
    """The k best news of the corpus for every distinct user of the split
    (Recommendations). The user vector is built from the first
    num_clicked_news_a_user ids of the user's first line, as evaluate() builds
    it; with exclude_history those clicked rows are never recommended."""
    users, hists = first_lines(impressions)
    hrows = history_rows(corpus, hists, model.config.num_clicked_news_a_user)
    k = int(k)
    if not users:
        return Recommendations([], np.zeros((0, k), np.int64), np.zeros((0, k), np.float32), corpus.ids)
    news_tab = news_vectors(model, corpus.titles, **category_args(model, corpus))
    uvec = user_vectors(model, news_tab, hrows)
    rows, scores = topk(news_tab, uvec, k, exclude=hrows if exclude_history else None, n_news=len(corpus))
    return Recommendations(users, _host(rows).astype(np.int64), _host(scores).astype(np.float32), corpus.ids)


@torch.no_grad()
def recommend(model, directory, user_id, k=20, thr=0.5):
    """The reference's recommend() for one user of the split in `directory`
    (news_parsed.tsv + behaviors.tsv), ranked over the whole corpus instead of
    20 drawn candidates: (ranked news ids, their degrees (score + 1) / 2 in
    fp64, the ids with degree > thr). An unknown user raises KeyError."""
    corpus = read_news_parsed(os.path.join(directory, "news_parsed.tsv"))
    imps = load_behaviors(os.path.join(directory, "behaviors.tsv"))
    names = imps.users() if isinstance(imps, BehaviorsTable) else [im.user for im in imps]
    if user_id not in names:
        raise KeyError(user_id)
    res = recommend_split(model, corpus, [imps[names.index(user_id)]], k)
    ids = res.news_ids[0]
    return ids, res.degrees[0, :len(ids)], res.above(thr)[0]


# ------------------------------------------------------------------ benchmark
BENCH_NEWS, BENCH_USERS, BENCH_K, BENCH_EXCL, BENCH_D = 42416, 50000, 10, 50, 300
# dense peaks of one MI355X used for the floor (TFLOP/s): f32 MFMA, bf16 MFMA
PEAK_F32_TF, PEAK_BF16_TF = 157.3, 2516.8


def torch_route(news, users, k, exclude, chunk=4096):
    """The route without the fused kernel: torch.topk(users[a:b] @ news.T,
    k + n_excl) in user chunks, the excluded rows masked out, re-cut to k.
    (Ties come out in torch.topk's order, not by row.)"""
    n_excl = exclude.shape[1]
    rows = torch.empty(users.shape[0], k, dtype=torch.int64, device=users.device)
    scores = torch.empty(users.shape[0], k, dtype=torch.float32, device=users.device)
    for a in range(0, users.shape[0], chunk):
        s, r = torch.topk(users[a:a + chunk] @ news.T, k + n_excl, dim=1)
        hit = (r.unsqueeze(2) == exclude[a:a + chunk].unsqueeze(1)).any(2)
        s = s.masked_fill(hit, float("-inf"))
        s2, j = torch.topk(s, k, dim=1)
        rows[a:a + chunk] = r.gather(1, j)
        scores[a:a + chunk] = s2
    return rows, scores


def check_rule_d(news, users, exclude, rows, scores, sample=64):
    """Rule (d) of tests/test_gpu_topk.py on a sample of users, in fp64 on the
    host: every row not returned (and not excluded) scores at most the k-th
    returned score + 2 tol, and each returned score is within tol of its
    row's fp64 dot, tol = (D + 16) 2^-24 sum |n_i u_i|. Returns the worst
    (score error / tol, margin violation / tol)."""
    idx = np.linspace(0, users.shape[0] - 1, sample).astype(np.int64)
    nw = news.double().cpu().numpy()
    worst_e = worst_v = 0.0
    for u in idx:
        uv = users[u].double().cpu().numpy()
        y = nw @ uv
        tol = (nw.shape[1] + 16) * 2.0 ** -24 * (np.abs(nw) @ np.abs(uv))
        r, s = _host(rows[u]), _host(scores[u]).astype(np.float64)
        worst_e = max(worst_e, float(np.max(np.abs(s - y[r]) / tol[r])))
        rest = np.ones(nw.shape[0], bool)
        rest[r] = False
        ex = _host(exclude[u])
        rest[ex[(ex >= 0) & (ex < nw.shape[0])]] = False
        worst_v = max(worst_v, float(np.max((y[rest] - s[-1]) / tol[rest])))
    return worst_e, worst_v


def bench(reps=20, warmup=3, out=sys.stdout):
    """Time topk at the MIND-small-dev shape bench.py uses for evaluate()
    (42,416 news, 50,000 users, K = 10, 50 excluded per user, seeded random
    vectors) under each arithmetic, alternating with torch_route in the same
    process; device events, median and min..max over `reps` runs."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    news = torch.randn(BENCH_NEWS, BENCH_D, generator=g).to(dev)
    users = torch.randn(BENCH_USERS, BENCH_D, generator=g).to(dev)
    exclude = torch.randint(0, BENCH_NEWS, (BENCH_USERS, BENCH_EXCL), generator=g).to(dev)
    pairs = BENCH_NEWS * BENCH_USERS
    flop = 2.0 * pairs * BENCH_D

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    def stats(v):
        v = np.sort(np.asarray(v))
        return float(np.median(v)), float(v[0]), float(v[-1])

    print(f"topk bench: {BENCH_NEWS} news x {BENCH_USERS} users, D {BENCH_D}, K {BENCH_K}, "
          f"{BENCH_EXCL} excluded per user; {reps} reps after {warmup} warm-up, alternating", file=out)
    modes = [("split-f16x3 (default)", N.NRMS_GEMM_SPLIT_F16X3, 6 * flop / (PEAK_BF16_TF * 1e9)),
             ("split-bf16x6", N.NRMS_GEMM_SPLIT_BF16X6, 6 * flop / (PEAK_BF16_TF * 1e9)),
             ("f32", N.NRMS_GEMM_F32, flop / (PEAK_F32_TF * 1e9))]
    result = {}
    for name, mode, floor_ms in modes:
        with N.gemm_arith(mode):
            fused = lambda: topk(news, users, BENCH_K, exclude)
            ref = lambda: torch_route(news, users, BENCH_K, exclude)
            for _ in range(warmup):
                fused()
                ref()
            tf, tr = [], []
            for _ in range(reps):
                t, got = timed(fused)
                tf.append(t)
                t, want = timed(ref)
                tr.append(t)
            e, v = check_rule_d(news, users, exclude, got[0], got[1])
            e2, v2 = check_rule_d(news, users, exclude, want[0], want[1])
        mf, lf, hf = stats(tf)
        mr, lr, hr = stats(tr)
        ok = e <= 1.0 and v <= 2.0 and e2 <= 1.0 and v2 <= 2.0
        print(f"  {name:22s} fused {mf:8.3f} ms [{lf:.3f} .. {hf:.3f}]  {pairs / mf / 1e6:8.2f} G pairs/s  "
              f"floor {floor_ms:.2f} ms (at {100 * floor_ms / mf:.1f} % of its rate)  | torch {mr:8.3f} ms "
              f"[{lr:.3f} .. {hr:.3f}]  ratio {mr / mf:.2f}x  | rule (d): fused err/tol {e:.4f} "
              f"margin/tol {v:.3f}, torch {e2:.4f} / {v2:.3f} -> {'agree' if ok else 'DISAGREE'}", file=out)
        result[name] = dict(fused_ms=mf, fused_min=lf, fused_max=hf, torch_ms=mr, torch_min=lr, torch_max=hr,
                            agree=ok)
    return result


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Rank the whole corpus for the users of a behaviors split")
    ap.add_argument("directory", nargs="?", help="split directory: news_parsed.tsv + behaviors.tsv")
    ap.add_argument("--checkpoint", help="ckpt-*.pth in the reference's format")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--user", help="one user id (default: every user of the split)")
    ap.add_argument("--out", help="write `user<TAB>N1 N2 ...` lines here (default: stdout)")
    ap.add_argument("--bench", action="store_true", help="time the fused kernel against the torch route")
    a = ap.parse_args(argv)
    if a.bench:
        bench()
        return 0
    if not a.directory or not a.checkpoint:
        ap.error("DIR and --checkpoint are required")
    from .checkpoint import load_model
    model = load_model(a.checkpoint, "cuda:0")
    corpus = read_news_parsed(os.path.join(a.directory, "news_parsed.tsv"))
    imps = load_behaviors(os.path.join(a.directory, "behaviors.tsv"))
    if a.user is not None:
        names = imps.users() if isinstance(imps, BehaviorsTable) else [im.user for im in imps]
        if a.user not in names:
            raise KeyError(a.user)
        imps = [imps[names.index(a.user)]]
    res = recommend_split(model, corpus, imps, a.k)
    f = open(a.out, "w") if a.out else sys.stdout
    try:
        for u, ids in zip(res.users, res.news_ids):
            f.write(f"{u}\t{' '.join(ids)}\n")
    finally:
        if a.out:
            f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
