"""nrms_rank_impressions and the prediction pipeline on the GPU: scores bitwise
nrms_score_pairs', both rank orders exactly at the edge lengths (LDS limit and
chunked path included), isolation of an impression from its call, agreement
with the metrics kernel's ranks, the CLI end to end and graph capture."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from newsrecommendationsystem_amd import _native as N
from newsrecommendationsystem_amd import data as Dt
from newsrecommendationsystem_amd import predict as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIM = N.NRMS_RANK_LDS_CANDIDATES


def bits(x):
    return np.ascontiguousarray(x).view(np.int32)


def score_pairs(news, users, cand, pair_user):
    out = torch.empty(cand.shape[0], dtype=torch.float32, device=news.device)
    N.call("nrms_score_pairs", N.ptr(news), news.shape[0], N.ptr(users), users.shape[0], N.ptr(cand),
           N.ptr(pair_user), cand.shape[0], news.shape[1], N.ptr(out), N.stream_handle(news.device))
    return out


def ragged(D, device, seed=1):
    """50 news, 7 users, 40 ragged impressions (some empty); candidate rows
    reach outside [0, 50) and two impressions name a user row out of range."""
    g = torch.Generator().manual_seed(seed)
    news = torch.randn(50, D, generator=g).to(device)
    users = torch.randn(7, D, generator=g).to(device)
    counts = torch.randint(0, 31, (40,), generator=g)
    counts[3], counts[17], counts[5], counts[29] = 0, 1, 4, 9
    off = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])
    cand = torch.randint(-2, 53, (int(off[-1]),), generator=g)
    imp_user = torch.randint(0, 7, (40,), generator=g)
    imp_user[5], imp_user[29] = 7, -1
    return news, users, cand.to(device), imp_user.to(device), off.to(device), counts.to(device)


@pytest.mark.parametrize("D", [300, 64, 7])
def test_scores_bitwise_equal_score_pairs(device, D):
    news, users, cand, imp_user, off, counts = ragged(D, device)
    pair_user = torch.repeat_interleave(imp_user, counts)
    want = score_pairs(news, users, cand, pair_user).cpu().numpy()
    for ties in ("order", "shared"):
        got, ranks = P.rank_impressions(news, users, cand, imp_user, off, ties)
        got = got.cpu().numpy()
        assert np.array_equal(bits(got), bits(want)), (D, ties)
        assert np.array_equal(ranks.cpu().numpy(), P.numpy_ranks(got, off.cpu().numpy(), ties)), (D, ties)
    # NaN exactly where a candidate row or the impression's user row is out of range
    c, u = cand.cpu().numpy(), pair_user.cpu().numpy()
    bad = (c < 0) | (c >= 50) | (u < 0) | (u >= 7)
    assert bad.any() and not bad.all()
    assert np.array_equal(np.isnan(want), bad) and np.array_equal(np.isnan(got), bad)


# ---------------------------------------------------------------- ranks at the edge lengths
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, LIM - 1, LIM, LIM + 1, 3 * LIM + 5]


def reference_ranks(s, ties):
    """The issue's definitions on one impression's fp32 scores."""
    n = s.shape[0]
    if ties == "order":
        order = np.argsort(s, kind="stable")[::-1]
        r = np.empty(n, np.int64)
        r[order] = np.arange(1, n + 1)
        return r
    nan = np.isnan(s)
    r = np.empty(n, np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(n):          # key_j > key_c: by value, NaN above +inf, all NaNs equal
            r[c] = 1 + ((s > s[c]) | (nan & ~nan[c])).sum()
    return r


@pytest.fixture(scope="module")
def edge():
    """One call per tie mode over impressions of every edge length, twice:
    first drawing finite rows only, then all rows (inf, -inf, NaN, zeros of
    both signs). 16 news rows of small integers and integer user vectors, so
    scores are small integers and ties are plentiful and exact."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    device = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    D = 8
    news = rng.integers(-2, 3, (16, D)).astype(np.float32)
    news[11] = [0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0]
    news[12, 2] = np.inf
    news[13, 2] = -np.inf
    news[14, 5] = np.nan
    news[15] = -0.0
    users = rng.integers(0, 3, (3, D)).astype(np.float32)
    users[:, 2] = [1.0, 2.0, 0.0]                             # (user 2: inf * 0 = NaN as well)
    counts = np.array(EDGE_LENGTHS * 2, np.int64)
    n_imp = counts.shape[0]
    finite_only = np.arange(n_imp) < len(EDGE_LENGTHS)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cand = np.concatenate([rng.integers(0, 12 if f else 16, c) for c, f in zip(counts, finite_only)]).astype(np.int64)
    imp_user = (np.arange(n_imp) % 3).astype(np.int64)
    d = dict(news=torch.from_numpy(news).to(device), users=torch.from_numpy(users).to(device), cand=cand,
             imp_user=imp_user, off=off, counts=counts, finite_only=finite_only, device=device)
    for ties in ("order", "shared"):
        s, r = P.rank_impressions(d["news"], d["users"], cand, imp_user, off, ties)
        d[ties] = (s.cpu().numpy(), r.cpu().numpy())
    return d


def test_ranks_exact_at_edge_lengths(edge):
    off = edge["off"]
    s = edge["order"][0]
    assert np.array_equal(bits(s), bits(edge["shared"][0]))
    assert np.isinf(s).any() and np.isnan(s).any() and (s == 0).any()
    assert np.array_equal(s[np.isfinite(s)], np.round(s[np.isfinite(s)]))      # small integers: exact ties
    for i, (a, b) in enumerate(zip(off[:-1], off[1:])):
        si = s[a:b]
        if edge["finite_only"][i]:
            assert np.isfinite(si).all()
        for ties in ("order", "shared"):
            got = edge[ties][1][a:b]
            assert np.array_equal(got, reference_ranks(si, ties)), (i, b - a, ties)
        assert np.array_equal(np.sort(edge["order"][1][a:b]), np.arange(1, b - a + 1)), i   # a permutation
        if edge["finite_only"][i]:
            # the reference's value2rank, literally (src/evaluate.py:45-48)
            vals = si.tolist()
            ordered = sorted(vals, reverse=True)
            assert edge["shared"][1][a:b].tolist() == [ordered.index(x) + 1 for x in vals], i
    # ties did occur on both sides of the LDS limit
    for i in (len(EDGE_LENGTHS) - 4, len(EDGE_LENGTHS) - 1):
        a, b = off[i], off[i + 1]
        assert len(np.unique(s[a:b])) < (b - a) // 4


def test_impression_is_isolated_from_its_call(edge):
    """Each impression alone in a call, and the whole batch in reversed order,
    give bitwise the scores and ranks of the batched call."""
    off, cand, imp_user, counts = edge["off"], edge["cand"], edge["imp_user"], edge["counts"]
    n_imp = counts.shape[0]
    rev = np.arange(n_imp)[::-1]
    rev_cand = np.concatenate([cand[off[i]:off[i + 1]] for i in rev]).astype(np.int64)
    rev_off = np.concatenate([[0], np.cumsum(counts[rev])]).astype(np.int64)
    for ties in ("order", "shared"):
        want_s, want_r = edge[ties]
        for i in range(n_imp):
            a, b = off[i], off[i + 1]
            s, r = P.rank_impressions(edge["news"], edge["users"], cand[a:b], imp_user[i:i + 1],
                                      np.array([0, b - a], np.int64), ties)
            assert np.array_equal(bits(s.cpu().numpy()), bits(want_s[a:b])), (ties, i)
            assert np.array_equal(r.cpu().numpy(), want_r[a:b]), (ties, i)
        s, r = P.rank_impressions(edge["news"], edge["users"], rev_cand, imp_user[rev].copy(), rev_off, ties)
        s, r = s.cpu().numpy(), r.cpu().numpy()
        for k, i in enumerate(rev):
            a, b = off[i], off[i + 1]
            assert np.array_equal(bits(s[rev_off[k]:rev_off[k + 1]]), bits(want_s[a:b])), (ties, i)
            assert np.array_equal(r[rev_off[k]:rev_off[k + 1]], want_r[a:b]), (ties, i)


# ---------------------------------------------------------------- the pipeline
V = 2048


@pytest.fixture(scope="module")
def labelled(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from newsrecommendationsystem_amd import NRMS, NRMSConfig
    d = str(tmp_path_factory.mktemp("predict_gpu"))
    corpus, imps = Dt.synthetic_split(d, seed=11, n_news=500, n_users=60, n_impressions=300, V=V)
    torch.manual_seed(7)
    cfg = type("Cfg", (NRMSConfig,), dict(num_words=V))
    model = NRMS(cfg, torch.randn(V, 300) * 0.5).to(torch.device("cuda:0")).eval()
    pred = P.predict_split(model, corpus, Dt.load_behaviors(d + "/behaviors.tsv"))
    return dict(dir=d, corpus=corpus, imps=imps, model=model, pred=pred)


def test_ranks_agree_with_the_metrics_kernel(labelled):
    """MRR recomputed in fp64 from predict_split's "order" ranks and the labels
    equals nrms_impression_metrics' column 1 (same rank definition; only the
    summation order differs), except where that kernel returns NaN by its own
    rule: no positive label, or a non-finite score."""
    from newsrecommendationsystem_amd.evaluate import EvalPlan, score_plan
    plan = EvalPlan(labelled["corpus"], Dt.load_behaviors(labelled["dir"] + "/behaviors.tsv"))
    scores, metrics = score_plan(labelled["model"], plan)
    scores, metrics = scores.cpu().numpy(), metrics.cpu().numpy()
    pred = labelled["pred"]
    assert np.array_equal(pred.offsets, plan.offsets) and len(pred) == 300
    assert np.array_equal(bits(pred.scores), bits(scores))
    mrr = np.full(len(pred), np.nan)
    excluded = np.zeros(len(pred), bool)
    for i, (a, b) in enumerate(zip(plan.offsets[:-1], plan.offsets[1:])):
        pos = plan.labels[a:b] == 1
        excluded[i] = not pos.any() or not np.isfinite(scores[a:b]).all()
        if not excluded[i]:
            mrr[i] = (1.0 / pred.ranks[a:b][pos].astype(np.float64)).sum() / pos.sum()
    assert 0 < excluded.sum() < len(pred) // 2
    assert np.isnan(metrics[excluded, 1]).all()
    keep = ~excluded
    assert np.allclose(mrr[keep], metrics[keep, 1], rtol=0, atol=1e-12, equal_nan=True)
    assert not np.isnan(metrics[keep, 1]).any()


def test_cli_end_to_end_on_an_unlabelled_split(labelled, tmp_path):
    """behaviors.tsv with the labels stripped through the CLI in a child
    process: prediction.txt has one line per impression in file order, each a
    permutation, equal to predict_split in this process."""
    from tests.predict_cases import strip_labels
    d = str(tmp_path)
    strip_labels(labelled["dir"] + "/behaviors.tsv", d + "/behaviors.tsv")
    with open(labelled["dir"] + "/news_parsed.tsv") as f, open(d + "/news_parsed.tsv", "w") as g:
        g.write(f.read())
    with open(d + "/behaviors.tsv") as f:
        assert all("-" not in line.split("\t")[4] for line in f)
    ckpt, out = d + "/ckpt-1.pth", d + "/prediction.txt"
    torch.save({"model_state_dict": labelled["model"].state_dict()}, ckpt)
    p = subprocess.run([sys.executable, "-m", "newsrecommendationsystem_amd.predict", d, "--checkpoint", ckpt,
                        "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    got = P.read_prediction(out)
    bare = Dt.load_behaviors_any(d + "/behaviors.tsv")
    assert isinstance(bare, Dt.BehaviorsTable) and (bare.labels == -1).all()
    want = P.predict_split(labelled["model"], labelled["corpus"], bare)
    with open(out) as f:
        lines = f.read().split("\n")
    assert lines[-1] == "" and len(lines) == 301 and " [" in lines[0] and ", " not in lines[0]
    assert got.impression_ids == want.impression_ids == [str(k + 1) for k in range(300)]
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.ranks, want.ranks)
    for i in range(len(got)):
        assert np.array_equal(np.sort(got.ranks_of(i)), np.arange(1, len(labelled["imps"][i].candidates) + 1)), i
    # ... and to the labelled split's prediction: the labels play no part
    assert np.array_equal(want.ranks, labelled["pred"].ranks)
    assert np.array_equal(bits(want.scores), bits(labelled["pred"].scores))


def test_graph_capture(device):
    """One call captured in torch.cuda.graph and replayed equals the eager
    result bitwise (no allocation, no synchronisation in the call)."""
    news, users, cand, imp_user, off, _ = ragged(300, device, seed=2)
    eager_s, eager_r = P.rank_impressions(news, users, cand, imp_user, off)
    sc = torch.full_like(eager_s, -7.0)
    rk = torch.full_like(eager_r, -7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        N.call("nrms_rank_impressions", N.ptr(news), news.shape[0], N.ptr(users), users.shape[0], N.ptr(cand),
               N.ptr(imp_user), N.ptr(off), imp_user.shape[0], 300, N.NRMS_RANK_ORDER, N.ptr(sc), N.ptr(rk),
               N.stream_handle(device))
    sc.fill_(-7.0)
    rk.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(sc.cpu().numpy()), bits(eager_s.cpu().numpy()))
    assert np.array_equal(rk.cpu().numpy(), eager_r.cpu().numpy())
