"""The seams of the training host path, on the CPU: forward_autograd's
explicit dropout masks, the one max_count cut (evaluate.cut_impressions), the
host gather that TrainSet.host_batch and ImpressionSet.host_batch share, and
the command line's dispatch (train_cli._main)."""
import os
import sys

import numpy as np
import pytest
import torch

from newsrecommendationsystem_amd import NRMS, NRMSConfig
from newsrecommendationsystem_amd import data as Dt
from newsrecommendationsystem_amd import train as TR
from newsrecommendationsystem_amd import train_cli
from newsrecommendationsystem_amd.evaluate import cut_impressions
from tests import fit_cases as FC
from tests import resample_cases as RC

B, C, N, L, V = 2, 2, 3, 4, 50


def _model_and_batch():
    torch.manual_seed(5)
    m = NRMS(type("Cfg", (NRMSConfig,), dict(num_words=V)), torch.randn(V, 300) * 0.5).train()
    g = torch.Generator().manual_seed(6)
    cand = torch.randint(1, V, (B, C, L), generator=g)
    clk = torch.randint(0, V, (B, N, L), generator=g)
    clk[0, 0] = 0                                     # a padding title
    return m, cand, clk


def _grads(model, logits):
    model.zero_grad()
    TR.loss_fn(logits).backward()
    return {n: p.grad.clone() for n, p in model.named_parameters()}


def _assert_same(model, got, ref):
    assert torch.equal(got, ref)
    g, r = _grads(model, got), _grads(model, ref)
    assert list(g) == [n for n, _ in model.named_parameters()]
    for n in g:
        assert torch.equal(g[n], r[n]), n


def test_forward_autograd_masks_of_ones_is_eval_forward():
    m, cand, clk = _model_and_batch()
    ones = [torch.ones(B * (C + N) * L, 300) for _ in range(2)]
    _assert_same(m, TR.forward_autograd(m, cand, clk, masks=ones),
                 TR.forward_autograd(m, cand, clk, training=False))


def test_forward_autograd_masks_are_the_two_dropouts():
    """masks = (m1, m2) drawn as 0 or 1/(1-p): the op sequence written out."""
    m, cand, clk = _model_and_batch()
    p = m.config.dropout_probability
    assert 0 < p < 1
    g = torch.Generator().manual_seed(7)
    m1, m2 = ((torch.rand(B * (C + N) * L, 300, generator=g) >= p).float() / (1 - p) for _ in range(2))
    assert 0 < int((m1 == 0).sum()) < m1.numel()
    got = TR.forward_autograd(m, cand, clk, masks=(m1, m2))

    ne, ue = m.news_encoder, m.user_encoder
    ids = torch.cat([cand.reshape(B * C, L), clk.reshape(B * N, L)])
    x = ne.word_embedding(ids) * m1.view(B * (C + N), L, 300)
    h = TR._mhsa(x, ne.multihead_self_attention) * m2.view(B * (C + N), L, 300)
    vec = TR._additive(h, ne.additive_attention)
    user = TR.user_encode_autograd(ue, vec[B * C:].view(B, N, -1))
    ref = torch.bmm(vec[:B * C].view(B, C, -1), user.unsqueeze(-1)).squeeze(-1)
    _assert_same(m, got, ref)


def _reference_scored(impressions, max_count):
    """src/evaluate.py:241-249: count from 1, break before scoring when
    count == max_count."""
    scored, count = [], 0
    for im in impressions:
        count += 1
        if count == max_count:
            break
        scored.append(im)
    return scored


def test_cut_impressions_is_the_references_break():
    imps = list("abcde")
    n = len(imps)
    for max_count in (0, 1, 2, n - 1, n, n + 1, sys.maxsize):
        assert list(cut_impressions(imps, max_count)) == _reference_scored(imps, max_count), max_count
    assert cut_impressions(imps) is imps


def _check_host_batch(ts, rows, *key):
    """host_batch of valid indices mixed with -1 and S against titles_host
    indexed by the set's row table `rows` [S, C + N]."""
    S = len(ts)
    idx = np.array([-1, 3, S, 0, S - 1, 3])
    cand, clk = ts.host_batch(torch.from_numpy(idx), *key)
    assert cand.shape == (idx.size, ts.C, ts.L) and clk.shape == (idx.size, ts.N, ts.L)
    assert cand.dtype == clk.dtype == torch.int64
    got = np.concatenate([cand.numpy(), clk.numpy()], axis=1)
    ok = (idx >= 0) & (idx < S)
    assert not got[~ok].any()
    assert np.array_equal(got[ok], ts.titles_host[rows[idx[ok]]])
    assert got[ok].any()


def test_train_set_host_batch_is_the_row_table_gather(tmp_path):
    ts = FC.generated_train_set(tmp_path, S=30, C=3, N=5, L=6)
    _check_host_batch(ts, ts.rows_host)


def test_impression_set_host_batch_is_the_row_table_gather(tmp_path):
    shape = [(2, 4), (1, 3), (3, 5), (1, 1), (2, 6), (4, 4), (1, 7), (2, 2), (3, 3), (1, 5), (2, 3), (2, 4)]
    iset = RC.raw_set(tmp_path, shape, K=2, L=6, N=5)
    assert 20 <= len(iset) <= 40
    _check_host_batch(iset, iset.materialize(3, 1), 3, 1)


def _no_model(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(train_cli, "NRMS", boom)


def test_cli_bench_with_bench_resample_runs_the_bench(monkeypatch):
    """--bench wins over --bench-resample, with the bench defaults filled in;
    the dispatch itself builds nothing."""
    _no_model(monkeypatch)
    seen = []
    monkeypatch.setattr(train_cli, "_bench_main", lambda a: seen.append(("bench", a.steps, a.batch, a.pairs)))
    monkeypatch.setattr(train_cli, "_bench_resample_main", lambda a: seen.append(("resample",)))
    train_cli._main(["--bench", "--bench-resample"])
    assert seen == [("bench", 300, 64, 5)]
    train_cli._main(["--bench-resample", "--steps", "7"])
    assert seen[1:] == [("resample",)]


def test_cli_export_epoch_needs_negatives_resample(monkeypatch, tmp_path):
    _no_model(monkeypatch)
    Dt.synthetic_train_split(str(tmp_path / "train"), seed=0, n_samples=8, n_news=20, V=V, K=2)
    monkeypatch.chdir(tmp_path)
    for extra in (["--export-epoch", "0", str(tmp_path / "out.tsv")], ["--k", "2"]):
        with pytest.raises(SystemExit) as e:
            train_cli._main([str(tmp_path), *extra])
        assert e.value.code == "--export-epoch and --k go with --negatives resample"
    assert not os.path.exists(tmp_path / "out.tsv") and not os.path.exists(tmp_path / "checkpoint")
