"""Fit from a raw behaviors.tsv on the GPU (fit.ImpressionSet, csrc/fit.hip):
nrms_train_batch_sample_gather bitwise against the host mirror at its edge
shapes, its index checks on deliberately broken sets, the sampler's properties
read from the kernel's own output, and fit() on an ImpressionSet against fit()
on the TrainSet of the exported epoch, bitwise, with resume."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

from newsrecommendationsystem_amd import _native as N
from oracle import weights as W
from tests import fit_cases as FC
from tests import resample_cases as RC

pytestmark = pytest.mark.gpu
F = FC.F
quiet = lambda *_: None   # noqa: E731


def _check(s, idx, seed, epoch):
    want_c, want_k = s.host_batch(idx, seed, epoch)
    cand, clk = s.batch(torch.as_tensor(idx), seed, epoch)
    assert cand.is_cuda and cand.dtype == torch.int64 and tuple(cand.shape) == tuple(want_c.shape)
    assert clk.is_cuda and clk.dtype == torch.int64 and tuple(clk.shape) == tuple(want_k.shape)
    assert torch.equal(cand.cpu(), want_c) and torch.equal(clk.cpu(), want_k)
    return cand.cpu().clone(), clk.cpu().clone()


# ------------------------------------------------------------------ kernel vs host mirror
# impressions (positives, negatives): one with n = K for every K below, one with n = 300
SHAPE = [(2, 15), (1, 300), (3, 2), (1, 1), (2, 4), (2, 40)]


@pytest.fixture(scope="module")
def split_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("resample_gpu")
    RC.write_raw_split(d, SHAPE, n_news=340, V=512, seed=2)
    return d


@pytest.mark.parametrize("K", [0, 1, 2, 15])
def test_sample_gather_matches_host_mirror(device, split_dir, K):
    corpus = RC.Dt.read_news_parsed(str(split_dir / "news_parsed.tsv"))
    s = F.ImpressionSet(str(split_dir / "behaviors.tsv"), corpus, k=K, device=device)
    S = len(s)
    assert S == {0: 11, 1: 11, 2: 10, 15: 5}[K] and s.C == 1 + K
    n = np.diff(s.neg_off_host)[s.pos_imp_host]
    if K:
        assert (n == K).any() and (n == 300).any()
    _check(s, [S - 1], 0, 0)                                                    # B = 1
    idx = [0, S - 1, 0, 1, 1, 2, 0]                                             # repeated samples
    cand, clk = _check(s, idx, 9, 3)
    assert torch.equal(cand[0], cand[2]) and torch.equal(cand[0], cand[6]) and torch.equal(clk[3], clk[4])
    first = s.batch(torch.as_tensor(idx), 9, 3)
    again = s.batch(torch.as_tensor(idx, device=device), 9, 3)
    assert again[0].data_ptr() == first[0].data_ptr() and again[1].data_ptr() == first[1].data_ptr()   # the set's own
    assert torch.equal(again[0].cpu(), cand) and torch.equal(again[1].cpu(), clk)                       # two calls
    # a sample's titles are the same alone and inside a larger batch
    alone = _check(s, [1], 9, 3)
    assert torch.equal(alone[0][0], cand[3]) and torch.equal(alone[1][0], clk[3])
    # all samples, large seed and epoch
    _check(s, np.arange(S), -1, 2 ** 40 + 5)


@pytest.mark.parametrize("K,N,L,B", [(2, 1, 7, 3), (4, 50, 20, 65)], ids=["odd-L7", "ragged-last-workgroup"])
def test_sample_gather_generated(device, tmp_path, K, N, L, B):
    """L = 7 with N = 1: rows only 8-byte aligned. S = 70, K = 4, N = 50,
    L = 20, B = 65: 71,500 words, 280 workgroups, the last one ragged."""
    rng = np.random.default_rng(5)
    shape, S = [], 0
    while S < 70:
        p = min(int(rng.integers(1, 5)), 70 - S)
        shape.append((p, int(rng.integers(K, K + 20))))
        S += p
    s = RC.raw_set(tmp_path, shape, K=K, N=N, L=L, device=device, n_news=90, V=512, seed=6)
    assert len(s) == 70 and (B * (1 + K + N) * L) % 256 != 0
    _check(s, F.epoch_order(1, 0, 70)[:B], 1, 0)


def test_sampler_properties_from_the_kernel_output(device, split_dir):
    """Read from the kernel's output alone (titles are distinct: the first
    word is row + 1): slot 0 is the positive, every other slot one of the
    impression's negatives, no negative position repeats, and epochs 0 and 1
    draw differently."""
    corpus = RC.Dt.read_news_parsed(str(split_dir / "news_parsed.tsv"))
    s = F.ImpressionSet(str(split_dir / "behaviors.tsv"), corpus, k=2, device=device)
    S = len(s)
    out = {}
    for e in (0, 1):
        cand, clk = s.batch(torch.arange(S), 12, e)
        out[e] = cand.cpu().numpy().copy()
        rows = out[e][:, :, 0] - 1
        assert np.array_equal(out[e], s.titles_host[rows])                        # whole titles, not only word 0
        assert np.array_equal(rows[:, 0], s.pos_row_host)
        for b in range(S):
            i = int(s.pos_imp_host[b])
            negs = s.neg_rows_host[s.neg_off_host[i]:s.neg_off_host[i + 1]].tolist()
            assert len(set(negs)) == len(negs)                                      # so a row names one position
            got = rows[b, 1:].tolist()
            assert set(got) <= set(negs) and len(set(got)) == len(got)
        hist = s.hist_rows_host[s.imp_hist_host[s.pos_imp_host]]
        assert np.array_equal(clk.cpu().numpy(), s.titles_host[hist])
    assert (out[0] != out[1]).any(axis=(1, 2)).sum() >= 1
    assert np.array_equal(out[0][:, 0], out[1][:, 0])                              # the positives stay


# ------------------------------------------------------------------ index checks
def test_out_of_range_sample_index_gives_zero_titles(device, split_dir):
    """An input check, not a fault: nothing is read at an index outside the
    set; that sample's titles are zeros and the others stay correct."""
    corpus = RC.Dt.read_news_parsed(str(split_dir / "news_parsed.tsv"))
    s = F.ImpressionSet(str(split_dir / "behaviors.tsv"), corpus, k=2, device=device)
    S = len(s)
    cand, clk = _check(s, [2, -1, 0, S, 1], 3, 1)
    for b in (1, 3):
        assert not cand[b].any() and not clk[b].any()
    good = _check(s, [2, 0, 1], 3, 1)
    assert torch.equal(cand[[0, 2, 4]], good[0]) and torch.equal(clk[[0, 2, 4]], good[1])
    assert cand[[0, 2, 4], 0].any(dim=1).all()


def _broken(device, split_dir):
    corpus = RC.Dt.read_news_parsed(str(split_dir / "news_parsed.tsv"))
    return F.ImpressionSet(str(split_dir / "behaviors.tsv"), corpus, k=2, device=device)


def _break_pos_imp(s):
    v = s.pos_imp_host.copy()
    v[1] = s.imp_hist_host.shape[0]                     # = I
    RC.set_table(s, "pos_imp", v)
    return lambda c, k: not c[1, 1:].any() and not k[1].any() and c[1, 0].any()     # the positive needs no impression


def _break_neg_rows(s):
    v = s.neg_rows_host.copy()
    v[:] = s.titles_host.shape[0]                       # = n_title_rows, every entry
    RC.set_table(s, "neg_rows", v)
    return lambda c, k: not c[:, 1:].any() and c[:, 0].any(dim=1).all() and k.any()


def _break_imp_hist(s):
    v = s.imp_hist_host.copy()
    v[int(s.pos_imp_host[1])] = s.hist_rows_host.shape[0]                            # = H
    RC.set_table(s, "imp_hist", v)
    return lambda c, k: not k[1].any() and c[1].any(dim=1).all()


def _break_neg_off_past_end(s):
    v = s.neg_off_host.copy()
    v[-1] = s.neg_rows_host.shape[0] + 5                # the last impression's range runs past T
    RC.set_table(s, "neg_off", v)
    return lambda c, k: not c[-1, 1:].any() and c[-1, 0].any() and c[0, 1:].any(dim=1).all()


def _break_neg_off_decreasing(s):
    v = s.neg_off_host.copy()
    i = int(s.pos_imp_host[1])
    v[i + 1] = v[i] - 1
    RC.set_table(s, "neg_off", v)
    return lambda c, k: not c[1, 1:].any() and c[1, 0].any()


def _break_too_few_negatives(s):
    i = int(s.pos_imp_host[1])                          # an impression with n = 1 < K = 2, placed by hand
    v = s.neg_off_host.copy()
    v[i + 1] = v[i] + 1
    RC.set_table(s, "neg_off", v)
    return lambda c, k: c[1, 1].any() and not c[1, 2].any() and c[1, 0].any()


@pytest.mark.parametrize("breaker", [_break_pos_imp, _break_neg_rows, _break_imp_hist, _break_neg_off_past_end,
                                     _break_neg_off_decreasing, _break_too_few_negatives],
                         ids=lambda f: f.__name__[7:])
def test_broken_set_gives_zeros(device, split_dir, breaker):
    """Input checks that complete normally: an index that falls outside its
    table is compared with the table's size and never dereferenced; the titles
    that depend on it are zeros (host mirror: the same rule)."""
    s = _broken(device, split_dir)
    zeros_where_expected = breaker(s)
    cand, clk = _check(s, np.arange(len(s)), 4, 0)
    assert zeros_where_expected(cand, clk)


def test_unsupported_k_is_refused_without_a_launch(device, split_dir):
    s = _broken(device, split_dir)
    idx = torch.zeros(1, dtype=torch.int64, device=device)
    cand = torch.full((1, 17, s.L), -7, dtype=torch.int64, device=device)
    clk = torch.full((1, s.N, s.L), -7, dtype=torch.int64, device=device)
    for K in (16, -1):
        st = N.load().nrms_train_batch_sample_gather(
            N.ptr(s.titles), s.titles.shape[0], s.L, N.ptr(s.pos_row), N.ptr(s.pos_imp), len(s), N.ptr(s.neg_off),
            s.imp_hist.shape[0], N.ptr(s.neg_rows), s.neg_rows.shape[0], N.ptr(s.imp_hist), N.ptr(s.hist_rows),
            s.hist_rows.shape[0], K, s.N, N.ptr(idx), 1, ctypes.c_uint64(0), 0, N.ptr(cand), N.ptr(clk),
            N.stream_handle(device))
        assert st == N.NRMS_ERR_UNSUPPORTED
    torch.cuda.synchronize(device)
    assert (cand == -7).all() and (clk == -7).all()                 # nothing was written


# ------------------------------------------------------------------ the loop
V_FIT = 512


@pytest.fixture(scope="module")
def fit_sets(device, tmp_path_factory):
    """S = 14 samples of 5 impressions, K = 2, N = 50, L = 20 over V = 512: B = 4
    gives three steps per epoch."""
    d = tmp_path_factory.mktemp("resample_fit")
    s = RC.raw_set(d, [(3, 7), (2, 3), (4, 11), (3, 2), (2, 25)], K=2, device=device, n_news=60, V=V_FIT, seed=4)
    assert len(s) == 14
    return s, d


def _gpu_model(device, p, seed=51, **fields):
    from newsrecommendationsystem_amd import NRMS, NRMSConfig
    m = NRMS(FC.with_cfg(NRMSConfig, num_words=V_FIT, dropout_probability=p, **fields))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.nrms_state(seed, V_FIT).items()})
    return m.to(device).train()


def test_fit_equals_fit_on_the_exported_epoch(device, fit_sets):
    """Three steps inside epoch 0: the same batches as the TrainSet read from
    the epoch's exported file, so the same parameters and Adam state, bitwise."""
    s, d = fit_sets
    ts = RC.exported_train_set(s, d, 7, 0, device)
    base = _gpu_model(device, 0.2)
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    ra = F.fit(ma, s, steps=3, batch_size=4, seed=7, log=quiet)
    rb = F.fit(mb, ts, steps=3, batch_size=4, seed=7, log=quiet)
    assert torch.equal(ra.losses, rb.losses) and torch.isfinite(ra.losses).all()
    FC.assert_same_training_state(ma, ra.optimizer, mb, rb.optimizer)


def test_fit_across_an_epoch_boundary_is_bitwise_repeatable(device, fit_sets):
    s, d = fit_sets
    base = _gpu_model(device, 0.2)
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    ra = F.fit(ma, s, steps=5, batch_size=4, seed=5, log=quiet)
    rb = F.fit(mb, s, steps=5, batch_size=4, seed=5, log=quiet)
    assert torch.equal(ra.losses, rb.losses) and torch.isfinite(ra.losses).all()
    FC.assert_same_training_state(ma, ra.optimizer, mb, rb.optimizer)
    # epoch 1 (steps 4, 5) trains on another draw than the epoch-0 file holds
    mc = copy.deepcopy(base)
    rc = F.fit(mc, RC.exported_train_set(s, d, 5, 0, device), steps=5, batch_size=4, seed=5, log=quiet)
    assert torch.equal(ra.losses[:3], rc.losses[:3]) and not torch.equal(ra.losses[3:], rc.losses[3:])


def test_fit_resume_is_bitwise_with_dropout(device, fit_sets, tmp_path):
    """As test_gpu_fit's: interrupted after step 3 (the end of epoch 0) and
    resumed from its checkpoint, the run is the uninterrupted one; holds only
    if the negatives are a function of (seed, epoch, sample)."""
    s, _ = fit_sets
    rising = [0.51, 0.52, 0.53]
    base = _gpu_model(device, 0.2, num_batches_validate=2)
    ma = copy.deepcopy(base)
    ra = F.fit(ma, s, checkpoint_dir=str(tmp_path / "a"), seed=1, steps=6, batch_size=4,
               validate=FC.scripted(rising), log=quiet)
    mb = copy.deepcopy(base)
    F.fit(mb, s, checkpoint_dir=str(tmp_path / "b"), seed=1, steps=4, batch_size=4,
          validate=FC.scripted(rising), log=quiet)
    assert sorted(os.listdir(tmp_path / "b")) == ["ckpt-2.pth", "ckpt-4.pth"]
    fresh = _gpu_model(device, 0.2, seed=52, num_batches_validate=2)
    rb = F.fit(fresh, s, checkpoint_dir=str(tmp_path / "b"), seed=1, steps=2, batch_size=4,
               validate=FC.scripted(rising[2:]), log=quiet)
    assert rb.start_step == 4 and rb.step == 6                      # resumed inside epoch 1
    assert torch.equal(ra.losses[4:], rb.losses)
    FC.assert_same_training_state(ma, ra.optimizer, fresh, rb.optimizer)


def test_fit_host_batches_route_gives_the_same_losses(device, fit_sets):
    s, _ = fit_sets
    base = _gpu_model(device, 0.0)
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    ra = F.fit(ma, s, steps=4, batch_size=4, seed=2, log=quiet)
    rb = F.fit(mb, s, steps=4, batch_size=4, seed=2, log=quiet, host_batches=True)
    print("device", ra.losses.tolist(), "host_batches", rb.losses.tolist())
    assert (ra.losses - rb.losses).abs().max() <= 1e-6
