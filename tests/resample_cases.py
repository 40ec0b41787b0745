"""Small raw splits (news_parsed.tsv + a labelled behaviors.tsv) and helpers
shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py."""
import os

import numpy as np
import torch

from newsrecommendationsystem_amd import data as Dt
from tests import fit_cases as FC

F = FC.F


def distinct_titles(n_news, L, V, seed=0):
    """[n_news, L] titles whose first word is row + 1, so a title identifies
    its row (needs n_news < V); the other words random, lengths 2 .. L."""
    assert n_news < V
    rng = np.random.default_rng(seed)
    t = rng.integers(1, V, (n_news, L))
    t[np.arange(L)[None, :] >= rng.integers(min(2, L), L + 1, n_news)[:, None]] = 0
    t[:, 0] = np.arange(n_news) + 1
    return t.astype(np.int64)


def write_raw_split(directory, shape, *, L=20, N=50, n_news=None, V=512, seed=0):
    """Write news_parsed.tsv + behaviors.tsv under `directory` and return
    (corpus, impressions). shape: [(n_pos, n_neg)] per impression; candidates
    are distinct news with the positives at random positions; histories of
    0 .. N + 3 items (some empty, some truncated), a few shared between
    impressions."""
    rng = np.random.default_rng(seed)
    os.makedirs(str(directory), exist_ok=True)
    if n_news is None:
        n_news = max(p + n for p, n in shape) + 8
    titles = distinct_titles(n_news, L, V, seed)
    ids = [f"N{i + 1}" for i in range(n_news)]
    users = [" ".join(f"N{x + 1}" for x in rng.integers(0, n_news, int(rng.integers(0, N + 4))))
             for _ in range(max(1, (len(shape) * 2) // 3))]
    imps = []
    for k, (p, n) in enumerate(shape):
        u = int(rng.integers(0, len(users)))
        cand = rng.choice(n_news, size=p + n, replace=False)
        labels = np.zeros(p + n, np.int64)
        labels[rng.choice(p + n, size=p, replace=False)] = 1
        imps.append(Dt.Impression(str(k + 1), f"U{u}", "11/15/2019 10:00:00 AM", users[u] or " ",
                                  [ids[c] for c in cand], labels.tolist()))
    Dt.write_news_parsed(os.path.join(str(directory), "news_parsed.tsv"), ids, titles)
    Dt.write_behaviors(os.path.join(str(directory), "behaviors.tsv"), imps)
    corpus = Dt.read_news_parsed(os.path.join(str(directory), "news_parsed.tsv"), num_words_title=L)
    assert np.array_equal(corpus.titles, titles)
    return corpus, imps


def raw_set(directory, shape, *, K, device="cpu", L=20, N=50, **kw):
    corpus, _ = write_raw_split(directory, shape, L=L, N=N, **kw)
    return F.ImpressionSet(os.path.join(str(directory), "behaviors.tsv"), corpus, k=K, num_clicked=N, device=device)


def exported_train_set(iset, directory, seed, epoch, device="cpu"):
    """The TrainSet of `iset`'s epoch as a behaviors_parsed.tsv written by
    export_epoch under `directory` (which holds the split's news_parsed.tsv)."""
    path = os.path.join(str(directory), f"behaviors_parsed_e{epoch}.tsv")
    iset.export_epoch(path, seed, epoch)
    corpus = Dt.read_news_parsed(os.path.join(str(directory), "news_parsed.tsv"), num_words_title=iset.L)
    return F.TrainSet(path, corpus, num_clicked=iset.N, device=device)


def set_table(iset, name, values):
    """Replace one table of the set, host copy and device copy alike (the
    deliberately broken sets of the index checks)."""
    host = np.ascontiguousarray(values, dtype=getattr(iset, name + "_host").dtype)
    setattr(iset, name + "_host", host)
    setattr(iset, name, torch.from_numpy(host).to(iset.device))
