"""The host-side index of one behaviors.tsv split (numpy only): what
evaluation, prediction files and fitting from raw impressions all read.

index_split maps every candidate and every history id of a split to its corpus
row in flat passes (the reference looks them up inside its per-impression
loop, src/evaluate.py:115-124,251-255) and numbers the users by history
string, as the reference caches user vectors. EvalPlan, PredictPlan and
ImpressionSet are views of its result.
"""
from dataclasses import dataclass
from typing import Callable

import numpy as np

from .data import (PADDED_NEWS, BehaviorsTable, _index_rows, candidate_rows_numeric, history_ids,
                   history_rows_numeric, news_numbers, numeric_news_index, parse_candidate_cells,
                   parse_impression_cells)


@dataclass
class SplitIndex:
    cand: np.ndarray             # int64 [P]: corpus row of every candidate, file order
    labels: np.ndarray           # int32 [P], or None (labelled=False)
    counts: np.ndarray           # int64 [I]: candidates per impression
    offsets: np.ndarray          # int64 [I + 1]
    imp_user: np.ndarray         # int64 [I]: row of hist_rows
    hist_rows: np.ndarray        # int64 [H, num_clicked]: distinct histories, first-seen order
    impressions: object          # the table or list the arrays were built from
    impression_ids: Callable     # () -> the impression id column (str), file order


def index_split(corpus, impressions, num_clicked, labelled=True):
    """The SplitIndex of a BehaviorsTable or a list of Impression.

    A table over a corpus of MIND-form ids (data.numeric_news_index) is indexed
    from its arrays. Anything else goes by the raw cells: one numeric parse
    when the ids allow, the per-name corpus.index lookup otherwise.
    labelled=False takes `<id>-<label>` and bare `<id>` tokens alike and
    gives no labels; labelled=True on a bare token raises what
    data.parse_impression_cells raises. An unknown id raises KeyError naming
    it, as news2vector[...] does."""
    nindex = numeric_news_index(corpus)
    labels = None
    if isinstance(impressions, BehaviorsTable) and nindex is not None:
        tab = impressions
        cand, counts, imp_user = _index_rows(nindex, tab.cand_num), tab.cand_count, tab.hist_user
        if labelled:
            labels = tab.labels
        hist_rows = table_history_rows(tab, nindex, num_clicked, len(corpus))
        ids = lambda: [tab.text[a:b] for a, b in tab.fields[:, 0].tolist()]
    else:
        imps = impressions = list(impressions)
        imp_user, hists = users_by_history(imps)
        if labelled:
            fast = candidate_rows_numeric(imps, nindex)
            if fast is not None:
                cand, labels, counts = fast
            else:
                names, labels, counts = parse_impression_cells(imps)
                cand = lookup_rows(corpus, names)
        else:
            names, counts = parse_candidate_cells(imps)
            nums = news_numbers(names) if nindex is not None else None
            cand = _index_rows(nindex, nums) if nums is not None else lookup_rows(corpus, names)
        hist_rows = history_rows_of(corpus, hists, num_clicked, nindex)
        ids = lambda: [im.impression_id for im in imps]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return SplitIndex(cand, labels, counts, offsets, imp_user, hist_rows, impressions, ids)


def users_by_history(impressions):
    """(user index int64 per impression, the distinct history strings): users
    are keyed by history string, numbered in first-seen order."""
    hist_of = {}
    hists = []
    imp_user = np.empty(len(impressions), dtype=np.int64)
    for k, im in enumerate(impressions):
        u = hist_of.get(im.clicked_news)
        if u is None:
            u = hist_of[im.clicked_news] = len(hists)
            hists.append(im.clicked_news)
        imp_user[k] = u
    return imp_user, hists


def lookup_rows(corpus, names):
    """corpus rows of news ids by name: id -> first row (news2vector[...],
    evaluate.py:255); an unknown id raises KeyError."""
    return np.fromiter(map(corpus.index.__getitem__, names), dtype=np.int64, count=len(names))


def history_rows_of(corpus, hists, num_clicked, nindex=None):
    """[len(hists), num_clicked] corpus rows of each history string's first
    num_clicked ids, left-padded with len(corpus) (the PADDED_NEWS row): the
    numeric pass when the ids allow, the per-name lookup otherwise. `nindex`:
    numeric_news_index(corpus) when the caller already holds it. An unknown
    id raises KeyError."""
    pad = len(corpus)
    if nindex is None:
        nindex = numeric_news_index(corpus)
    hrows = history_rows_numeric(hists, nindex, num_clicked, pad)
    if hrows is None:
        hist_names = [x for h in hists for x in history_ids(h, num_clicked)]
        real = np.array([x != PADDED_NEWS for x in hist_names], dtype=bool)
        rows = np.full(len(hist_names), pad, dtype=np.int64)
        if real.any():
            rows[real] = lookup_rows(corpus, [x for x, r in zip(hist_names, real) if r])
        hrows = rows.reshape(len(hists), num_clicked)
    return hrows


def table_history_rows(tab, nindex, num_clicked, pad):
    """The same rows from a BehaviorsTable: each distinct history's first
    line, its first num_clicked ids, left-padded."""
    imp_user = tab.hist_user
    _, first = np.unique(imp_user, return_index=True) if len(tab) else (None, np.zeros(0, np.int64))
    U = first.size
    hc, ho = tab.hist_count[first], tab.hist_off[first]
    m = np.minimum(hc, num_clicked)
    rows = np.full((U, num_clicked), pad, dtype=np.int64)
    if int(m.sum()):
        u = np.repeat(np.arange(U), m)
        k = np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m)
        rows[u, num_clicked - np.repeat(m, m) + k] = _index_rows(nindex, tab.hist_num[np.repeat(ho, m) + k])
    return rows
