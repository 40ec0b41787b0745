"""MIND prediction files on the HIP path: for every impression of a split,
labelled or not, the rank of each candidate (what a MIND user submits for the
test split, whose impressions cells read "N1 N2 N3" without labels).

The reference defines value2rank for this (src/evaluate.py:45-48) and never
calls it. Here:

  1. the split is read with or without labels (data.load_behaviors_any) and
     planned once on the host (PredictPlan: candidate rows, offsets, one user
     row per impression, history rows -- EvalPlan without labels and without
     the per-pair user array);
  2. news and user vectors as evaluate() builds them (evaluate.news_vectors /
     user_vectors);
  3. one nrms_rank_impressions call: a workgroup per impression scores its
     candidates against the impression's user vector (bitwise
     nrms_score_pairs' scores) and ranks them (csrc/eval.hip);
  4. write_prediction: `<impression id> [r1,r2,...]` lines, optionally zipped
     as prediction.txt.

CLI:

    python -m newsrecommendationsystem_amd.predict DIR --checkpoint CKPT
        [--out prediction.txt] [--zip] [--ties order|shared] [--bench]

Sharding over ranks is out of scope (users shard as in evaluate(); a caller
concatenates the shards' lines), and so is a native formatter for the file.
"""
import io
import os
import sys
import time
import zipfile

import numpy as np
import torch

from . import _native as N
from .data import BehaviorsTable, load_behaviors_any, read_news_parsed
from .evaluate import category_args, news_vectors, user_vectors
from .splits import index_split

TIES = {"order": N.NRMS_RANK_ORDER, "shared": N.NRMS_RANK_SHARED}
PREDICTION_NAME = "prediction.txt"


def rank_impressions(news_tab, users, cand_rows, imp_user, offsets, ties="order"):
    """(scores float32 [P], ranks int32 [P]) on the vectors' device, P =
    offsets[-1]: impression i owns the candidates cand_rows[offsets[i] :
    offsets[i + 1]] (rows of news_tab) and the user vector users[imp_user[i]].
    ties="order": the 1-based position in np.argsort(s, kind="stable")[::-1]
    (a permutation per impression); "shared": 1 + the number of strictly
    larger scores (the reference's value2rank). The contract is
    nrms_rank_impressions' (include/nrms_hip.h)."""
    if ties not in TIES:
        raise ValueError(f"ties must be one of {sorted(TIES)}, got {ties!r}")
    dev = news_tab.device
    if news_tab.dtype != torch.float32 or users.dtype != torch.float32:
        raise TypeError("rank_impressions takes float32 vectors")
    if users.dim() != 2 or news_tab.dim() != 2 or users.shape[1] != news_tab.shape[1]:
        raise ValueError(f"vector shapes {tuple(news_tab.shape)} / {tuple(users.shape)} do not match")
    news_tab, users = news_tab.contiguous(), users.contiguous().to(dev)
    cand_rows, imp_user, offsets = (torch.as_tensor(x, dtype=torch.int64).to(dev).contiguous()
                                    for x in (cand_rows, imp_user, offsets))
    if cand_rows.dim() != 1 or imp_user.dim() != 1 or offsets.dim() != 1:
        raise ValueError("cand_rows, imp_user and offsets are one-dimensional")
    n_imp = imp_user.shape[0]
    if offsets.shape[0] != n_imp + 1:
        raise ValueError(f"offsets must hold {n_imp + 1} entries, got {offsets.shape[0]}")
    P = cand_rows.shape[0]
    scores = torch.empty(P, dtype=torch.float32, device=dev)
    ranks = torch.empty(P, dtype=torch.int32, device=dev)
    if n_imp and P:   # (nothing to write otherwise; an empty tensor's pointer is null)
        N.call("nrms_rank_impressions", N.ptr(news_tab), news_tab.shape[0], N.ptr(users), users.shape[0],
               N.ptr(cand_rows), N.ptr(imp_user), N.ptr(offsets), n_imp, users.shape[1], TIES[ties],
               N.ptr(scores), N.ptr(ranks), N.stream_handle(dev))
    return scores, ranks


class PredictPlan:
    """Host-side index arrays of one split for prediction: `cand` (corpus row
    of every candidate), `offsets` [n + 1], `imp_user` [n] (row of hist_rows)
    and `hist_rows` [users, num_clicked]: splits.index_split's arrays without
    labels, and the impression ids. Takes a BehaviorsTable or a list of
    Impression, labelled or not (labels are ignored); an unknown id raises
    KeyError."""

    def __init__(self, corpus, impressions, num_clicked=50):
        split = index_split(corpus, impressions, num_clicked, labelled=False)
        self.corpus = corpus
        self.num_clicked = num_clicked
        self.impressions = impressions
        self.cand, self.offsets = split.cand, split.offsets
        self.imp_user, self.hist_rows = split.imp_user, split.hist_rows
        self.impression_ids = split.impression_ids()

    @property
    def n_impressions(self):
        return len(self.offsets) - 1


class Predictions:
    """predict_split's result: impression_ids (file order), offsets int64
    [n + 1], ranks int32 [P] and scores float32 [P] (None when read back from
    a prediction file); impression i owns [offsets[i], offsets[i + 1])."""

    def __init__(self, impression_ids, offsets, ranks, scores=None):
        self.impression_ids = list(impression_ids)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self.ranks = np.asarray(ranks, dtype=np.int32)
        self.scores = None if scores is None else np.asarray(scores, dtype=np.float32)

    def __len__(self):
        return len(self.impression_ids)

    def ranks_of(self, i):
        return self.ranks[self.offsets[i]:self.offsets[i + 1]]


@torch.no_grad()
def predict_plan(model, plan, ties="order"):
    """Predictions of a PredictPlan: the vectors, then one
    nrms_rank_impressions call."""
    if not plan.n_impressions:
        return Predictions([], [0], np.zeros(0, np.int32), np.zeros(0, np.float32))
    news_tab = news_vectors(model, plan.corpus.titles, **category_args(model, plan.corpus))
    users = user_vectors(model, news_tab, plan.hist_rows)
    scores, ranks = rank_impressions(news_tab, users, plan.cand, plan.imp_user, plan.offsets, ties)
    return Predictions(plan.impression_ids, plan.offsets, ranks.cpu().numpy(), scores.cpu().numpy())


@torch.no_grad()
def predict_split(model, corpus, impressions, ties="order"):
    """Scores and ranks of every candidate of every impression of the split
    (Predictions), labelled or not."""
    return predict_plan(model, PredictPlan(corpus, impressions, model.config.num_clicked_news_a_user), ties)


def format_prediction(predictions):
    """The MIND submission text: one `<impression id> [r1,r2,...]` line per
    impression in file order, no spaces inside the brackets."""
    toks = predictions.ranks.astype(str).tolist()
    off = predictions.offsets.tolist()
    return "".join(f"{iid} [{','.join(toks[a:b])}]\n"
                   for iid, a, b in zip(predictions.impression_ids, off[:-1], off[1:]))


def write_prediction(path, predictions, zip=False):
    """Write format_prediction's text at `path`, or with zip=True a zip archive
    at `path` holding it as prediction.txt."""
    text = format_prediction(predictions)
    if zip:
        with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
            z.writestr(PREDICTION_NAME, text)
    else:
        with open(path, "w", newline="") as f:
            f.write(text)


def read_prediction(path):
    """A prediction file (plain, or a zip holding prediction.txt) as
    Predictions without scores."""
    if zipfile.is_zipfile(path):
        with zipfile.ZipFile(path) as z:
            text = io.TextIOWrapper(z.open(PREDICTION_NAME), newline="").read()
    else:
        with open(path, newline="") as f:
            text = f.read()
    ids, counts, ranks = [], [], []
    for line in text.split("\n"):
        if not line:
            continue
        iid, cell = line.split(" ", 1)
        if not (cell.startswith("[") and cell.endswith("]")):
            raise ValueError(f"malformed prediction line {line!r}")
        body = cell[1:-1]
        vals = [int(x) for x in body.split(",")] if body else []
        ids.append(iid)
        counts.append(len(vals))
        ranks += vals
    return Predictions(ids, np.concatenate([[0], np.cumsum(counts)]), np.array(ranks, dtype=np.int32))


# ------------------------------------------------------------------ benchmark
# the shape of bench.py's eval_throughput leg (MIND-small dev)
BENCH_NEWS, BENCH_USERS, BENCH_IMPS, BENCH_D = 42416, 50000, 73152, 300
BENCH_MIN_CANDS, BENCH_MAX_CANDS = 2, 73


def numpy_ranks(scores, offsets, ties="order"):
    """The numpy definition of the two rank orders, per impression (host;
    tests and the benchmark's check)."""
    out = np.empty(scores.shape[0], np.int32)
    for a, b in zip(offsets[:-1], offsets[1:]):
        s = scores[a:b]
        if ties == "order":
            order = np.argsort(s, kind="stable")[::-1]
            r = np.empty(b - a, np.int32)
            r[order] = np.arange(1, b - a + 1)
        else:
            nan = np.isnan(s)
            with np.errstate(invalid="ignore"):
                gt = (s[None, :] > s[:, None]) | (nan[None, :] & ~nan[:, None])
            r = 1 + gt.sum(1)
        out[a:b] = r
    return out


def torch_route(news, users, cand, pair_user_host, offsets, counts):
    """The route without the fused kernel: upload the per-pair user array,
    nrms_score_pairs, then a segmented rank in torch -- a stable sort by score
    followed by a stable sort by impression puts every impression's pairs in
    ascending stable order, whose reverse is the "order" ranking."""
    dev = news.device
    P = cand.shape[0]
    pu = torch.from_numpy(pair_user_host).to(dev)
    scores = torch.empty(P, dtype=torch.float32, device=dev)
    N.call("nrms_score_pairs", N.ptr(news), news.shape[0], N.ptr(users), users.shape[0], N.ptr(cand),
           N.ptr(pu), P, news.shape[1], N.ptr(scores), N.stream_handle(dev))
    seg = torch.repeat_interleave(torch.arange(counts.shape[0], device=dev), counts, output_size=P)
    by_score = torch.sort(scores, stable=True).indices
    idx = by_score[torch.sort(seg[by_score], stable=True).indices]
    ranks = torch.empty(P, dtype=torch.int32, device=dev)
    ranks[idx] = (offsets[1:][seg] - torch.arange(P, device=dev)).to(torch.int32)
    return scores, ranks


def bench(reps=20, warmup=3, out=sys.stdout):
    """Time rank_impressions against torch_route at the MIND-small-dev shape
    (seeded random vectors and impressions), alternating in one process; wall
    time around a device synchronisation, since route (b)'s upload is part of
    it. Median and min..max over `reps` runs, and pairs/s."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    news = torch.randn(BENCH_NEWS, BENCH_D, generator=g).to(dev)
    users = torch.randn(BENCH_USERS, BENCH_D, generator=g).to(dev)
    counts_h = torch.randint(BENCH_MIN_CANDS, BENCH_MAX_CANDS + 1, (BENCH_IMPS,), generator=g).numpy()
    offsets_h = np.concatenate([[0], np.cumsum(counts_h)]).astype(np.int64)
    P = int(offsets_h[-1])
    cand = torch.randint(0, BENCH_NEWS, (P,), generator=g).to(dev)
    imp_user_h = torch.randint(0, BENCH_USERS, (BENCH_IMPS,), generator=g).numpy()
    pair_user_h = np.repeat(imp_user_h, counts_h)
    offsets, counts = torch.from_numpy(offsets_h).to(dev), torch.from_numpy(counts_h).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(v):
        v = np.sort(np.asarray(v))
        return float(np.median(v)), float(v[0]), float(v[-1])

    fused = lambda: rank_impressions(news, users, cand, torch.from_numpy(imp_user_h), offsets)
    ref = lambda: torch_route(news, users, cand, pair_user_h, offsets, counts)
    for _ in range(warmup):
        fused()
        ref()
    tf, tr, wins = [], [], 0
    for _ in range(reps):
        a, got = timed(fused)
        b, want = timed(ref)
        tf.append(a)
        tr.append(b)
        wins += a < b
    same_scores = bool((got[0].view(torch.int32) == want[0].view(torch.int32)).all())
    same_ranks = bool((got[1] == want[1]).all())
    host = numpy_ranks(got[0].cpu().numpy(), offsets_h)
    agree = same_scores and same_ranks and bool((got[1].cpu().numpy() == host).all())
    mf, lf, hf = stats(tf)
    mr, lr, hr = stats(tr)
    print(f"predict bench: {BENCH_NEWS} news, {BENCH_USERS} users, {BENCH_IMPS} impressions of "
          f"{BENCH_MIN_CANDS}..{BENCH_MAX_CANDS} candidates ({P} pairs), D {BENCH_D}; {reps} reps after "
          f"{warmup} warm-up, alternating, wall time incl. the user-index upload", file=out)
    print(f"  (a) nrms_rank_impressions          {mf:8.3f} ms [{lf:.3f} .. {hf:.3f}]  {P / mf / 1e3:8.2f} M pairs/s",
          file=out)
    print(f"  (b) nrms_score_pairs + torch rank  {mr:8.3f} ms [{lr:.3f} .. {hr:.3f}]  {P / mr / 1e3:8.2f} M pairs/s",
          file=out)
    print(f"  ratio (b) / (a) {mr / mf:.2f}x; (a) faster in {wins} of {reps} alternated pairs; scores bitwise "
          f"{'equal' if same_scores else 'DIFFERENT'}, ranks {'equal' if same_ranks else 'DIFFERENT'}, numpy "
          f"definition {'agrees' if agree else 'DISAGREES'}", file=out)
    return dict(fused_ms=mf, fused_min=lf, fused_max=hf, torch_ms=mr, torch_min=lr, torch_max=hr, wins=wins,
                reps=reps, agree=agree)


def bench_end_to_end(directory, out=sys.stdout, V=4096):
    """Wall-time split of one predict_split + write_prediction at the same
    shape: an unlabelled behaviors.tsv and a news_parsed.tsv written under
    `directory`, a seeded model; read, plan, GPU (vectors + rank + copy
    back), format + write."""
    from .config import NRMSConfig
    from .data import NUM_WORDS_TITLE, write_news_parsed
    from .nrms import NRMS
    rng = np.random.default_rng(0)
    os.makedirs(directory, exist_ok=True)
    titles = rng.integers(1, V, (BENCH_NEWS, NUM_WORDS_TITLE))
    titles[np.arange(NUM_WORDS_TITLE)[None, :] >= rng.integers(5, NUM_WORDS_TITLE + 1, BENCH_NEWS)[:, None]] = 0
    write_news_parsed(os.path.join(directory, "news_parsed.tsv"), [f"N{i}" for i in range(BENCH_NEWS)], titles)
    hists = [" ".join(f"N{x}" for x in rng.integers(0, BENCH_NEWS, rng.integers(0, 71))) for _ in range(BENCH_USERS)]
    with open(os.path.join(directory, "behaviors.tsv"), "w") as f:
        for k in range(BENCH_IMPS):
            u = int(rng.integers(0, BENCH_USERS))
            c = rng.integers(0, BENCH_NEWS, rng.integers(BENCH_MIN_CANDS, BENCH_MAX_CANDS + 1))
            f.write(f"{k + 1}\tU{u}\t11/15/2019 10:00:00 AM\t{hists[u]}\t{' '.join(f'N{x}' for x in c)}\n")
    torch.manual_seed(0)
    cfg = type("BenchCfg", (NRMSConfig,), dict(num_words=V))
    model = NRMS(cfg, torch.randn(V, BENCH_D) * 0.5).to(torch.device("cuda:0")).eval()
    path = os.path.join(directory, PREDICTION_NAME)
    rows = []
    for rep in range(2):   # (the first pass warms the kernels and the allocator)
        t = [time.perf_counter()]
        corpus = read_news_parsed(os.path.join(directory, "news_parsed.tsv"))
        imps = load_behaviors_any(os.path.join(directory, "behaviors.tsv"))
        t.append(time.perf_counter())
        plan = PredictPlan(corpus, imps, model.config.num_clicked_news_a_user)
        t.append(time.perf_counter())
        pred = predict_plan(model, plan)
        torch.cuda.synchronize()
        t.append(time.perf_counter())
        write_prediction(path, pred)
        t.append(time.perf_counter())
        rows.append(np.diff(t) * 1e3)
    r = rows[-1]
    print(f"end to end, {len(pred)} impressions / {pred.ranks.shape[0]} pairs, native reader "
          f"{'yes' if isinstance(imps, BehaviorsTable) else 'no'} (second of two passes): read {r[0]:.1f} ms, "
          f"plan {r[1]:.1f} ms, GPU (news + user vectors, rank, copy back) {r[2]:.1f} ms, format + write "
          f"{r[3]:.1f} ms, total {r.sum():.1f} ms", file=out)
    return dict(read_ms=r[0], plan_ms=r[1], gpu_ms=r[2], format_ms=r[3])


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Write a MIND prediction file for a behaviors split")
    ap.add_argument("directory", nargs="?", help="split directory: news_parsed.tsv + behaviors.tsv")
    ap.add_argument("--checkpoint", help="ckpt-*.pth in the reference's format")
    ap.add_argument("--out", default=PREDICTION_NAME, help="the prediction file (default: prediction.txt)")
    ap.add_argument("--zip", action="store_true", help="write a zip archive holding prediction.txt")
    ap.add_argument("--ties", choices=sorted(TIES), default="order")
    ap.add_argument("--bench", action="store_true",
                    help="time the fused kernel against score_pairs + a torch rank, and one end-to-end run")
    a = ap.parse_args(argv)
    if a.bench:
        import tempfile
        bench()
        with tempfile.TemporaryDirectory() as d:
            bench_end_to_end(d)
        return 0
    if not a.directory or not a.checkpoint:
        ap.error("DIR and --checkpoint are required")
    from .checkpoint import load_model
    model = load_model(a.checkpoint, "cuda:0")
    corpus = read_news_parsed(os.path.join(a.directory, "news_parsed.tsv"))
    imps = load_behaviors_any(os.path.join(a.directory, "behaviors.tsv"))
    write_prediction(a.out, predict_split(model, corpus, imps, a.ties), zip=a.zip)
    return 0


if __name__ == "__main__":
    sys.exit(main())
