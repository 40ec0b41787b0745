"""Eval-semantics scoring pipeline on the HIP path (drop-in for
src/evaluate.py:171-272).

The reference scores a split in three host-driven passes: news vectors cached
in a dict, user vectors cached per history string, then a Python loop with
batch size 1 over impressions (one get_prediction and one device->host sync
each), and finally per-impression AUC/MRR/nDCG in a process pool. Here every
pass is one (or a few) launches over flat index arrays built once on the
host:

  1. news vectors of the whole corpus: NRMS.get_news_vector (HIP NewsEncoder),
     plus one all-zero row for PADDED_NEWS (evaluate.py:203-204);
  2. user vectors of every distinct history string: the clicked-news rows are
     gathered from the news-vector table by nrms_embedding_gather and encoded
     by NRMS.get_user_vector (HIP UserEncoder);
  3. all impressions' candidate logits in one nrms_score_pairs launch;
  4. per-impression metrics in one nrms_impression_metrics launch, then the
     nanmean (evaluate.py:270-272) — or, across ranks, an all-reduce of
     (sum, count) per metric.
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

from . import _native as N
from .data import load_behaviors, read_news_parsed
from .distributed import all_reduce_sums, shard_impressions
from .splits import index_split


def cut_impressions(impressions, max_count=sys.maxsize):
    """The impressions the reference scores under max_count: it counts from 1
    and breaks when count == max_count before scoring that one
    (src/evaluate.py:245-249), so impressions 1..max_count-1; all of them when
    the count never reaches max_count (above their number, or below 1). The
    list itself when nothing is cut."""
    return impressions if not 1 <= max_count <= len(impressions) else impressions[:max_count - 1]


class EvalPlan:
    """Host-side index arrays for one split (built once, reused per model):
    splits.index_split's arrays of the impressions max_count leaves, and the
    user row of every (impression, candidate) pair. An unknown id raises
    KeyError as news2vector[...] does."""

    def __init__(self, corpus, impressions, max_count=sys.maxsize, num_clicked=50):
        split = index_split(corpus, cut_impressions(impressions, max_count), num_clicked)
        self.corpus = corpus
        self.num_clicked = num_clicked
        self.impressions = split.impressions
        self.cand, self.labels = split.cand, split.labels
        self.offsets, self.hist_rows = split.offsets, split.hist_rows
        self.pair_user = np.repeat(split.imp_user, split.counts)

    @property
    def n_impressions(self):
        return len(self.offsets) - 1


def has_category_views(model):
    """The model's news encoder reads category and subcategory besides the title (exp1.Exp1)."""
    return hasattr(getattr(model, "news_encoder", None), "element_encoders")


def category_args(model, corpus):
    """news_vectors' keyword arguments besides the titles: none for an NRMS
    model (its call is unchanged); for a model with category views the
    corpus's (category, subcategory) columns, read on first need."""
    return {"categories": corpus.categories()} if has_category_views(model) else {}


@torch.no_grad()
def news_vectors(model, titles, chunk=65536, categories=None):
    """[n + 1, D] news-vector table on the model's device; last row = PADDED_NEWS.
    categories: (category [n], subcategory [n]) for a model with category
    views (category_args), passed along in every chunk."""
    ne = model.news_encoder
    dev = ne.word_embedding.weight.device
    D = ne.word_embedding.embedding_dim
    n = titles.shape[0]
    out = torch.zeros(n + 1, D, dtype=torch.float32, device=dev)
    t = torch.from_numpy(titles) if isinstance(titles, np.ndarray) else titles
    if has_category_views(model):
        if categories is None:
            raise ValueError("a model with category views needs the corpus's categories (category_args)")
        cat, sub = (torch.as_tensor(c) for c in categories)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        news = {"title": t[a:b]}
        if has_category_views(model):
            news.update(category=cat[a:b], subcategory=sub[a:b])
        out[a:b] = model.get_news_vector(news)
    return out


@torch.no_grad()
def user_vectors(model, news_tab, hist_rows, chunk=16384):
    """User vectors of every history: gather clicked rows (PADDED -> zero row)
    then the HIP UserEncoder. A user encoder with a position embedding
    (exp1.UserEncoder) adds it in the gather's pass."""
    dev = news_tab.device
    U, Nc = hist_rows.shape
    D = news_tab.shape[1]
    out = torch.empty(U, D, dtype=torch.float32, device=dev)
    rows = torch.from_numpy(hist_rows).to(dev)
    ue = model.user_encoder
    for a in range(0, U, chunk):
        r = rows[a:a + chunk].contiguous()
        b = r.shape[0]
        if hasattr(ue, "add_position_rows"):
            out[a:a + b] = ue.encode_positioned(ue.add_position_rows(news_tab, r))
            continue
        x = torch.empty(b * Nc, D, dtype=torch.float32, device=dev)
        N.call("nrms_embedding_gather", N.ptr(r), b * Nc, N.ptr(news_tab), news_tab.shape[0], D,
               N.ptr(x), N.stream_handle(dev))
        out[a:a + b] = model.get_user_vector(x.view(b, Nc, D))
    return out


@torch.no_grad()
def score_plan(model, plan):
    """Logits of every (impression, candidate) pair and the per-impression
    metric table [n_imp, 4] (AUC, MRR, nDCG@5, nDCG@10; fp64) on the device."""
    news_tab = news_vectors(model, plan.corpus.titles, **category_args(model, plan.corpus))
    dev = news_tab.device
    D = news_tab.shape[1]
    users = user_vectors(model, news_tab, plan.hist_rows)
    K = plan.cand.shape[0]
    scores = torch.empty(K, dtype=torch.float32, device=dev)
    cand = torch.from_numpy(plan.cand).to(dev)
    pu = torch.from_numpy(plan.pair_user).to(dev)
    st = N.stream_handle(dev)
    N.call("nrms_score_pairs", N.ptr(news_tab), news_tab.shape[0], N.ptr(users), users.shape[0],
           N.ptr(cand), N.ptr(pu), K, D, N.ptr(scores), st)
    labels = torch.from_numpy(plan.labels).to(dev)
    offsets = torch.from_numpy(plan.offsets).to(dev)
    metrics = torch.empty(plan.n_impressions, 4, dtype=torch.float64, device=dev)
    N.call("nrms_impression_metrics", N.ptr(scores), N.ptr(labels), N.ptr(offsets),
           plan.n_impressions, N.ptr(metrics), st)
    return scores, metrics


def nan_sums(metrics):
    """(sum, count) per metric column over non-NaN rows (fp64)."""
    ok = ~torch.isnan(metrics)
    return torch.where(ok, metrics, torch.zeros_like(metrics)).sum(0), ok.sum(0).to(torch.float64)


def reduce_means(sums, counts):
    with np.errstate(invalid="ignore"):
        return tuple(float(x) for x in (sums / counts).cpu().numpy())


@torch.no_grad()
def evaluate_plan(model, plan, process_group=None):
    """(AUC, MRR, nDCG@5, nDCG@10) of `plan`: the nanmean of score_plan's
    metric table (src/evaluate.py:270-272). With a `process_group`, `plan` is
    this rank's shard (it may be empty) and the (sum, count) per metric are
    all-reduced: every rank returns the same means."""
    if plan.n_impressions:
        sums, counts = nan_sums(score_plan(model, plan)[1])
    else:
        dev = model.news_encoder.word_embedding.weight.device
        sums, counts = (torch.zeros(4, dtype=torch.float64, device=dev) for _ in range(2))
    if process_group is not None:
        sums, counts = all_reduce_sums(sums, counts, process_group)
    return reduce_means(sums, counts)


@torch.no_grad()
def evaluate(model, directory, num_workers=4, max_count=sys.maxsize, process_group=None):
    """Same signature and return value as the reference's evaluate()
    (src/evaluate.py:171-184): (AUC, MRR, nDCG@5, nDCG@10) of the split in
    `directory` (news_parsed.tsv + behaviors.tsv). `num_workers` is accepted
    for compatibility (there is no process pool). With a torch.distributed
    `process_group`, each rank scores the impressions of its users
    (distributed.user_rank: user_id % world) and the metric sums are all-reduced."""
    corpus = read_news_parsed(os.path.join(directory, "news_parsed.tsv"))
    imps = load_behaviors(os.path.join(directory, "behaviors.tsv"))
    return evaluate_split(model, corpus, imps, max_count, process_group)


@torch.no_grad()
def evaluate_split(model, corpus, impressions, max_count=sys.maxsize, process_group=None):
    imps = cut_impressions(impressions, max_count)
    if process_group is not None:
        imps = shard_impressions(imps, dist.get_rank(process_group), dist.get_world_size(process_group))
    return evaluate_plan(model, EvalPlan(corpus, imps, num_clicked=model.config.num_clicked_news_a_user), process_group)
