"""The references and case tables of the per-kernel inference tests
(tests/infer_kernel_cases.py) checked on the CPU: each fp64 reference equals
the oracle's restatement of the reference model (oracle.nrms_oracle) taken in
fp64, the metric restatement equals oracle.metrics.single_impression wherever
the scores have no ties and predict.numpy_ranks("order") everywhere, every
table holds both sides of each threshold it names, the attention regimes keep
their score ranges, and the references that have to stay inside a bound on
their own do."""
import math

import numpy as np
import pytest
import torch

from oracle import metrics as OM
from oracle import nrms_oracle as O
from tests import infer_kernel_cases as C
from tests import topk_cases as T
from tests import train_kernel_cases as K


def _close(a, b, rel=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape
    assert float((a - b).norm()) <= rel * max(float(b.norm()), 1e-300), float((a - b).norm() / b.norm())


# -- the rule ---------------------------------------------------------------------

def test_report_is_the_forward_rule(capsys):
    o64 = torch.tensor([3.0, 4.0], dtype=torch.float64)
    o32 = o64 + torch.tensor([1e-6, 0.0], dtype=torch.float64)
    assert C.report("k", "c", "o", o64 + 2e-6, o64, o32) and not C.report("k", "c", "o", o64 + 4e-6, o64, o32)
    # 4 e_32 never beyond CAP_FORWARD n; the substituted floors enter as floor_abs
    assert not C.report("k", "c", "o", o64 + 1e-4, o64, o64 + 1.0)
    assert C.report("k", "c", "o", o64 + 6e-6, o64, o64, floor_abs=C.f16x3_floor(o64))
    assert not C.report("k", "c", "o", o64 + 6e-6, o64, o64)
    assert not C.report("k", "c", "o", torch.tensor([3.0, float("nan")]), o64, o32)
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 6 and all(ln.startswith(C.ERR_PREFIX + ": k c o e_hip/n=") for ln in lines)
    assert C.ERR_PREFIX != K.ERR_PREFIX and C.F16X3_REL == 2e-6 and K.CAP_FORWARD == 1e-5


# -- 1. dot scorers ---------------------------------------------------------------------

def test_dot_tables():
    assert set(C.DOT_D) == set(C.DOT_D_SCALAR + C.DOT_D_LANES + C.DOT_D_CACHE) and len(set(C.DOT_D)) == len(C.DOT_D)
    assert all(d % 4 for d in C.DOT_D_SCALAR) and not any(d % 4 for d in C.DOT_D_LANES + C.DOT_D_CACHE)
    assert {1, 63, 64, 65} <= {d // 4 for d in C.DOT_D_LANES}           # one lane, one short of, at and past a wave
    assert max(C.DOT_D_SCALAR) > 4 * 64 and min(C.DOT_D_SCALAR) == 1       # the scalar loop's fifth trip; one lane live
    cached = 4 * 64 * 4                                                  # kDotUserRegs float4 x 64 lanes
    assert {cached - 4, cached, cached + 4} <= set(C.DOT_D_CACHE)
    assert cached + 64 * 4 in C.DOT_D_CACHE                              # a whole pass from memory
    assert any(d > cached + 2 * 64 * 4 and (d // 4) % 64 == 1 for d in C.DOT_D_CACHE)   # two passes and a one-lane tail
    ni, ui, off, iu = C.dot_pairs()
    assert tuple(np.diff(off.numpy())) == C.DOT_COUNTS and off[0] == 0
    assert {c % 4 for c in C.DOT_COUNTS} == {0, 1, 3} and int(off[-1]) % 4 != 0   # partial last blocks
    assert set(ni.tolist()) == set(range(C.DOT_NEWS)) and set(iu.tolist()) == set(range(C.DOT_USERS))
    assert ui.tolist() == np.repeat(iu.numpy(), C.DOT_COUNTS).tolist()
    assert C.SCORE_B * C.SCORE_C == C.DOT_NEWS and C.SCORE_B == C.DOT_USERS
    assert set(C.SCORE_LAYOUT_D) == {300, 7} and len(C.SCORE_LAYOUTS) == 7


@pytest.mark.parametrize("kind", C.DOT_KINDS)
@pytest.mark.parametrize("Dd", C.DOT_D)
def test_dot_refs(Dd, kind):
    news, user = C.dot_inputs(Dd, kind)
    assert news.dtype == torch.float32 and news.shape == (C.DOT_NEWS, Dd) and user.shape == (C.DOT_USERS, Dd)
    nb = news.view(C.SCORE_B, C.SCORE_C, Dd)
    o64 = C.dot_ref(nb.double(), user.double().unsqueeze(1))
    _close(o64, O.click_score(nb.numpy(), user.numpy(), dt=np.float64))
    ni, ui, _, _ = C.dot_pairs()
    a, b = news[ni], user[ui]
    p64, p32 = C.dot_ref(a.double(), b.double()), C.dot_ref(a, b)
    _close(p64, torch.einsum("kd,kd->k", a.double(), b.double()))
    assert p32.dtype == torch.float32
    floor = C.dot_floor(a, b, kind)
    if kind == "same_sign":
        assert floor == 0.0 and float(a.min()) >= 0.5 and float(b.max()) <= 1.5
        # the kernel's own summation order in fp32, emulated: inside the rule with no floor, so the rule alone
        # bounds a correct wave_dot on these inputs
        emu = torch.tensor([C.wave_dot_emulated(a[k].numpy(), b[k].numpy()) for k in range(len(ni))],
                           dtype=torch.float64)
        e_hip, e_32, n, bound, which = K.errors(emu, p64, p32, 0.0, K.CAP_FORWARD)
        assert e_hip <= bound and e_hip <= 1.6 * max(e_32, 1e-7 * n)
        assert K.errors(p32, p64, p32, 0.0, K.CAP_FORWARD)[0] <= K.REL_FLOOR * n   # o_32 itself: under the 1e-6 n term
    else:
        rows = C.dot_floor_rows(a, b)
        assert floor == pytest.approx(float(rows.norm())) and bool((rows > 0).all())
        assert bool(((p32.double() - p64).abs() <= rows).all())             # the bound holds for the fp32 reference
        if Dd == T.D:   # the top-K tests' tolerance, one (user, row) at a time
            tol = T.tolerance(news.numpy(), user.numpy())                   # [users, news]
            assert np.allclose(rows.numpy(), tol[ui.numpy(), ni.numpy()], rtol=1e-14, atol=0)


def test_wave_dot_emulation_order():
    # exactly representable products: the emulation is the exact sum, whatever the order
    for Dd in (3, 8, 260):
        a = np.arange(1, Dd + 1, dtype=np.float32)
        b = np.where(np.arange(Dd) % 2 == 0, 0.5, -0.25).astype(np.float32)
        assert C.wave_dot_emulated(a, b) == float(np.dot(a.astype(np.float64), b.astype(np.float64)))


# -- 2. metrics -------------------------------------------------------------------------------

def _has_ties(s):
    return len(np.unique(np.asarray(s) + np.float32(0.0))) < len(s)


def test_metric_tables():
    cases = C.metric_cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    assert {5, 6, 10, 11, 63, 64, 65, 129} <= set(C.METRIC_N) and {1, 2} <= set(C.METRIC_N)
    for n in C.METRIC_N:
        for r in (1, 5, 6, 10, 11, n):
            assert (f"n{n}-pos@{r}" in names) == (r <= n)
        for p in (0, 1, 5, 6, 10, 11, n - 1, n):
            assert (f"n{n}-npos{p}" in names) == (0 <= p <= n)
        for kind in ("tie-poslo", "tie-poshi", "all-equal", "zeros"):
            assert (f"n{n}-{kind}" in names) == (n >= 2)
        assert (f"n{n}-ties-across-cuts" in names) == (n >= 11)
    by = {c[0]: c for c in cases}
    for name, y, s in cases:
        assert y.dtype == np.int32 and s.dtype == np.float32 and len(y) == len(s) and np.isfinite(s).all()
        n = len(s)
        if "-pos@" in name:
            r = int(name.split("@")[1])
            assert int(y.sum()) == 1 and int(C.ranks_ref(s)[y == 1][0]) == r and not _has_ties(s)
        if "-npos" in name:
            assert int(y.sum()) == int(name.split("npos")[1]) and not _has_ties(s)
        if "-tie-pos" in name:
            v, cnt = np.unique(s, return_counts=True)
            tied = np.flatnonzero(s == v[cnt == 2][0])
            assert sorted(cnt.tolist())[-2:] == ([1, 2] if n > 2 else [2]) and y[tied].sum() == 1
            # poslo: the positive has the smaller index and ranks after the negative it ties with
            r = C.ranks_ref(s)[tied]
            assert r[1] + 1 == r[0] and (y[tied[0]] == 1) == name.endswith("poslo")
        if name.endswith("zeros"):
            assert np.signbit(s).any() and (~np.signbit(s)).any() and (s == 0).all() and 0 < y.sum() < n
        if name.endswith("ties-across-cuts"):
            r, pos = C.ranks_ref(s), y == 1
            for lo, hi in ((4, 7), (9, 12)):   # one score over ranks lo..hi, positives on both sides of the cut-off
                grp = (r >= lo) & (r <= hi)
                assert len(np.unique(s[grp])) == 1 and (pos & grp & (r <= lo + 1)).any() and (pos & grp & (r > lo + 1)).any()
                assert (~pos & grp).any()
    # more than 10 positives, and rank 5 | 6 and 10 | 11 hit by a single positive
    assert int(by["n129-npos11"][1].sum()) == 11 and "n11-pos@11" in by and "n6-pos@5" in by
    bad = C.nonfinite_cases()
    assert len(bad) == 3 * len(C.NONFINITE_POS) and C.NONFINITE_POS == (0, 63, 64, C.NONFINITE_N - 1)
    for name, y, s in bad:
        assert len(s) == C.NONFINITE_N and int((~np.isfinite(s)).sum()) == 1 and 0 < y.sum() < len(y)
        assert not np.isfinite(s[int(name.split("@")[1])])
    assert C.METRIC_NIMP == (1, 4, 5) and C.METRIC_OFFSET0 == 7


def test_metrics_ref_is_the_oracle_without_ties_and_numpy_ranks_everywhere():
    from newsrecommendationsystem_amd import predict as P
    n_plain = 0
    for name, y, s in C.metric_cases() + C.nonfinite_cases():
        mine = np.array(C.metrics_ref(y, s))
        if not _has_ties(s):
            n_plain += 1
            want = np.array(OM.single_impression(y, s), dtype=np.float64)
            assert np.allclose(mine, want, rtol=1e-12, atol=1e-12, equal_nan=True), (name, mine, want)
        if np.isfinite(s).all():
            off = np.array([0, len(s)])
            assert P.numpy_ranks(s, off, "order").tolist() == C.ranks_ref(s).tolist(), name
            if 0 < y.sum() < len(y):   # AUC is oracle.metrics.auc_score, ties counted 1/2
                assert mine[0] == OM.auc_score(y, s)
    assert n_plain > 100
    assert np.isnan(C.metrics_ref(np.zeros(0, np.int32), np.zeros(0, np.float32))).all()


def test_metrics_ref_tie_order_by_hand():
    # scores 1 1 1, the positive first: it ranks last of the three (larger index first)
    assert C.ranks_ref(np.float32([1, 1, 1])).tolist() == [3, 2, 1]
    auc, mrr, n5, n10 = C.metrics_ref(np.int32([1, 0, 0]), np.float32([1, 1, 1]))
    assert (auc, mrr) == (0.5, 1 / 3) and n5 == n10 == pytest.approx(1 / math.log2(4))
    auc, mrr, n5, n10 = C.metrics_ref(np.int32([0, 0, 1]), np.float32([1, 1, 1]))
    assert (auc, mrr, n5, n10) == (0.5, 1.0, 1.0, 1.0)
    assert C.ranks_ref(np.float32([0.0, -0.0, 0.0])).tolist() == [3, 2, 1]
    # six tied positives and a negative below: ranks 1..6, five of them inside the first cut-off
    y, s = np.int32([1] * 6 + [0]), np.float32([2] * 6 + [1])
    d = 1 / np.log2(np.arange(1, 7) + 1.0)
    assert C.metrics_ref(y, s)[2] == pytest.approx(1.0) and C.metrics_ref(y, s)[3] == pytest.approx(1.0)
    y[5] = 0   # index 5 ranks first among the ties: the positives hold ranks 2..6
    assert C.metrics_ref(y, s)[2] == pytest.approx(d[1:5].sum() / d[:5].sum(), rel=1e-14)


def test_pack_impressions():
    cases = C.metric_cases()[:25]
    s, y, off, rows = C.pack_impressions(cases, 7, empty_every=10)
    assert off[0] == 7 and np.isnan(s[:7]).all() and len(off) - 1 == 25 + 2 and len(s) == off[-1] == len(y)
    for i, r in enumerate(rows):
        assert s[off[r]:off[r + 1]].tobytes() == cases[i][2].tobytes()
        assert y[off[r]:off[r + 1]].tobytes() == cases[i][1].tobytes()
    empty = np.setdiff1d(np.arange(27), rows)
    assert empty.tolist() == [10, 21] and all(off[e] == off[e + 1] for e in empty)


# -- 3. self-attention ------------------------------------------------------------------------

def test_attention_tables():
    for edge in (20, 32, 50, 64):   # launch_mhsa's instances, and the long kernel past 64
        assert {edge, edge + 1} <= set(C.ATT_L)
    assert {1, 19, 66, 130} <= set(C.ATT_L) and max(C.ATT_L) * K.H > 256 * 7
    assert C.ATT_REGIME_L == (20, 32, 50, 64, 65) and set(C.ATT_ADDRESS_L) == {20, 65}
    assert set(C.ATT_REGIMES) == {"wide", "vanishing", "recheck"} and C.ATT_NSEQ == (1, 3)
    assert 0 <= C.RECHECK_HEAD < K.H


@pytest.mark.parametrize("n_seq", C.ATT_NSEQ)
@pytest.mark.parametrize("L", C.ATT_L)
def test_attention_ref_is_the_oracle(L, n_seq):
    qkv = C.attention_inputs(L, n_seq, "normal")
    assert qkv.dtype == torch.float32 and qkv.shape == (n_seq * L, 3 * K.D)
    assert float(K.mhsa_scores(qkv.double(), n_seq, L).abs().max()) <= 5.0
    q, k, v = (t.double().numpy() for t in K._split_heads(qkv, n_seq, L))
    want = O.raw_exp_attention(q, k, v, K.DK, dt=np.float64)                 # [n_seq, H, L, DK]
    want = torch.from_numpy(want).permute(0, 2, 1, 3).reshape(n_seq * L, K.D)
    _close(C.attention_ref(qkv.double(), n_seq, L), want)
    assert C.attention_ref(qkv, n_seq, L).dtype == torch.float32


@pytest.mark.parametrize("regime", C.ATT_REGIMES)
@pytest.mark.parametrize("L", C.ATT_REGIME_L)
def test_attention_regimes(L, regime):
    n_seq = C.ATT_REGIME_NSEQ
    qkv = C.attention_inputs(L, n_seq, regime)
    s = K.mhsa_scores(qkv.double(), n_seq, L)
    z = C.attention_row_sums(qkv, n_seq, L)
    o32 = C.attention_ref(qkv, n_seq, L)
    assert bool(torch.isfinite(o32).all())
    if regime == "wide":
        assert 20.0 < float(s.abs().max()) <= 22.0
    elif regime == "vanishing":
        assert -25.0 <= float(s.min()) and float(s.max()) <= -11.0
        assert float(z.min()) < 1e-7   # the + 1e-8 changes a weight by more than 10 % in some row
    else:
        hot = z[:, C.RECHECK_HEAD]
        assert 2.0 ** 121 <= float(hot.min()) and float(hot.max()) <= 2.0 ** 125
        # past kExpRecheck = 2^120 with a margin the fast exp cannot eat; the other heads stay far below it
        rest = torch.cat([z[:, :C.RECHECK_HEAD], z[:, C.RECHECK_HEAD + 1:]], 1)
        assert float(rest.max()) < 2.0 ** 20
        # finite in fp32: the largest single exp and the fp32 row sum
        e32 = torch.exp(K.mhsa_scores(qkv, n_seq, L))
        assert float(e32.max()) < float("inf") and float(e32.sum(-1).max()) < float("inf")
        # equal scores: the head's context is the mean of its value rows
        v = K._split_heads(qkv.double(), n_seq, L)[2][:, C.RECHECK_HEAD]     # [n_seq, L, DK]
        got = C.attention_ref(qkv.double(), n_seq, L).view(n_seq, L, K.H, K.DK)[:, :, C.RECHECK_HEAD]
        _close(got, v.mean(1, keepdim=True).expand(-1, L, -1), rel=1e-9)


# -- 4. additive ----------------------------------------------------------------------------------

def _params(w):
    return {"a.linear.weight": w["w_add"].numpy(), "a.linear.bias": w["b_add"].numpy(),
            "a.attention_query_vector": w["q_add"].numpy()}


def test_additive_tables():
    assert {63, 64, 65, 127, 128, 129} <= set(C.ADD_ROWS) and 1 in C.ADD_ROWS and max(C.ADD_ROWS) > 2 * 128
    assert {63, 64, 65} <= set(C.POOL_L) and {1, 2, 130} <= set(C.POOL_L)
    assert {63, 64, 65} <= {d // 4 for d in C.POOL_D} and not any(d % 4 for d in C.POOL_D) and 300 in C.POOL_D
    assert C.POOL_NSEQ == (1, 4, 5) and C.ADD_SET_ROWS in C.ADD_ROWS
    assert {(n * L) for n, L in C.ADD_ATTENTION_SHAPES} >= {1, 100, 195, 260}
    assert {L > 64 for _, L in C.ADD_ATTENTION_SHAPES} == {True, False}


def test_additive_refs_are_the_oracle_and_the_sets_hold():
    w = K.encoder_weights(7)
    wa, ba, qa = (w[k].double() for k in ("w_add", "b_add", "q_add"))
    for n_seq, L in C.ADD_ATTENTION_SHAPES:
        x = C.additive_score_inputs(n_seq * L, "normal", seed=1403).view(n_seq, L, K.D)
        s64 = C.additive_scores_ref(x.double(), wa, ba, qa)
        want = O.additive_attention(x.numpy(), _params(w), "a", dt=np.float64)
        _close(C.pool_ref(x.double(), s64), want)
        _close(s64, torch.tanh(torch.from_numpy(O.linear(x.reshape(-1, K.D).numpy(), w["w_add"].numpy(),
                                                         w["b_add"].numpy(), dt=np.float64))).reshape(n_seq, L, K.Q) @ qa)
    z = {k: (C.additive_score_inputs(C.ADD_SET_ROWS, k).double() @ wa.t() + ba).abs() for k in C.ADD_SETS}
    assert float(z["saturating"].median()) > 5.0 and float((z["saturating"] > 1).double().mean()) > 0.9
    assert float((z["tiny"] - ba.abs()).abs().max()) < 1e-3          # the bias alone
    assert 0.1 < float(z["normal"].median()) < 1.0


@pytest.mark.parametrize("kind", C.POOL_SETS)
def test_pool_sets(kind):
    for L in C.POOL_L:
        x, s = C.pool_inputs(5, L, 300, kind)
        assert x.shape == (5, L, 300) and s.shape == (5, L) and s.dtype == torch.float32
        o64, o32 = C.pool_ref(x.double(), s.double()), C.pool_ref(x, s)
        assert bool(torch.isfinite(o64).all()) and bool(torch.isfinite(o32).all())
        if kind == "spread" and L > 2:
            assert float(s.max() - s.min()) > 80.0       # weights that underflow in fp32 next to the maximum
        if kind == "equal":
            _close(o64, x.double().mean(1), rel=1e-14)
        if kind == "neg_inf" and L > 1:
            assert bool(torch.isinf(s[:, L // 2]).all()) and int(torch.isinf(s).sum()) == 5
            keep = [l for l in range(L) if l != L // 2]
            _close(o64, C.pool_ref(x[:, keep].double(), s[:, keep].double()), rel=1e-14)


def test_pool_softmax_sum_absorbs_1e_8():
    """additive_pool_kernel divides by the max-subtracted sum, which holds an
    exp(0) = 1 term: sum >= 1, and fp32 rounds sum + 1e-8 back to sum (half an
    ulp of 1 is 6e-8). `e / (sum + 1e-8f)` there is the same kernel bit for bit,
    so no case of these tables (or any other) can tell the two apart; the
    raw-exp attention, whose sums reach 1e-8, is where the term counts."""
    for kind in C.POOL_SETS:
        for L in C.POOL_L:
            _, s = C.pool_inputs(5, L, 4, kind)
            sums = torch.exp(s - s.max(dim=1, keepdim=True).values).sum(1)
            assert sums.dtype == torch.float32 and float(sums.min()) >= 1.0
            assert torch.equal(sums + torch.tensor(1e-8, dtype=torch.float32), sums)
    assert np.float32(1.0) + np.float32(1e-8) == np.float32(1.0)


# -- 5. projection -----------------------------------------------------------------------------------

def test_project_tables_and_ref():
    for tile in (64, 128):
        assert {tile - 1, tile, tile + 1} <= set(C.PROJ_M)
    assert 193 in C.PROJ_M and 1 in C.PROJ_M and C.PROJ_LD_PADDED % 32 == 0 and C.PROJ_LD_PADDED > 3 * K.D
    w = K.encoder_weights(7)
    x = C.project_inputs(65)
    o64 = C.project_ref(x.double(), w)
    for i, n in enumerate("qkv"):
        _close(o64[:, i * K.D:(i + 1) * K.D], O.linear(x.numpy(), w["w_" + n].numpy(), w["b_" + n].numpy(), dt=np.float64))
    assert C.project_ref(x, w).dtype == torch.float32 and o64.shape == (65, 3 * K.D)
    ids = C.project_row_ids()
    assert ids.numel() == C.PROJ_IDS_M and int((ids == -1).sum()) == 1 and int((ids == C.PROJ_IDS_ROWS).sum()) == 1
    counts = np.bincount(ids[(ids >= 0) & (ids < C.PROJ_IDS_ROWS)].numpy(), minlength=C.PROJ_IDS_ROWS)
    assert counts.min() >= 2 and C.PROJ_IDS_M > 128


# -- 6. gather -----------------------------------------------------------------------------------------

def test_gather_tables_and_ref():
    assert 300 not in C.GATHER_D and {299, 301} <= set(C.GATHER_D) and {1, 4, 7, 304} <= set(C.GATHER_D)
    assert {63, 64, 65} <= set(C.GATHER_TOK) and max(C.GATHER_TOK) > 2 * 64
    for n_tok in C.GATHER_TOK:
        table, ids = C.gather_inputs(n_tok, 7)
        want, valid = C.gather_ref(table, ids)
        assert int((~valid).sum()) == (3 if n_tok >= 63 else 0)
        assert sorted(ids[~valid].tolist()) == (sorted(C.GATHER_BAD) if n_tok >= 63 else [])
        assert want[valid].numpy().tobytes() == O.embedding_gather(table.numpy(), ids[valid].numpy()).tobytes()
        if n_tok >= 2:
            assert int(ids[0]) == C.GATHER_V - 1 and int(ids[-1]) == 0
