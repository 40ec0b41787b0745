"""Exp1 on the GPU: the three new entry points of include/nrms_hip.h alone
against fp64 / fp32 references (tests/exp1_cases.py), then the module against
the reference's outputs (tests/golden/exp1_golden.npz), evaluate(), predict
and recommend on tests/golden/exp1/eval.

Tolerance of the kernel tests: tests/infer_kernel_cases.py's rule, e_hip <=
max(4 e_32, 1e-6 n, floor_abs) through train_kernel_cases.errors with
CAP_FORWARD. floor_abs is 0 except for the prepared logits, which are
mixed-sign dots q . tanh(.) of length Q: there it is that file's dot floor,
(Q + 16) 2^-24 sum_q |q_q tanh_q| per logit. No split-arithmetic floor: the
title-logit GEMM is the exact-f32 one in every mode. Copies, NaN patterns,
in-place against out-of-place and the position add are bitwise. The module
tests hold every output vector to TOL = 1e-5 (normwise, as
tests/test_gpu_parity.py).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import nrms_oracle as O
from tests import exp1_cases as X
from tests import infer_kernel_cases as C
from tests import topk_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exp1_golden.npz")
SPLIT = os.path.join(ROOT, "tests", "golden", "exp1", "eval")
D, Q, E = X.D, X.Q, X.E


def _N():
    from newsrecommendationsystem_amd import _native
    return _native


def _same_bits(a, b):
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def _device_views(w, device):
    """(nrms_views_weights_t, the device tensors it points into)."""
    N = _N()
    k = {n: t.to(device).contiguous() for n, t in w.items()}
    P = lambda n: k[n].data_ptr()
    s = N.ViewsWeights(P("emb"), P("emb"), w["emb"].shape[0], E, P("w_cat"), P("b_cat"), P("w_sub"), P("b_sub"),
                       P("w_fin"), P("b_fin"), P("q_fin"), D, Q)
    return s, k


def _prepare(w, device):
    N = _N()
    s, keep = _device_views(w, device)
    Cn = w["emb"].shape[0]
    nb = N.load().nrms_views_state_size(Cn, D)
    assert nb == Cn * (2 * D + 2) * 4
    state = torch.full((nb // 4 + 8,), float("nan"), device=device)   # 8 guard floats behind the state
    N.call("nrms_views_prepare", ctypes.byref(s), N.ptr(state), nb, N.stream_handle(device))
    torch.cuda.synchronize()
    assert bool(torch.isnan(state[nb // 4:]).all())
    return s, keep, state


def _fuse(s, state, title, cat, sub, out=None):
    N = _N()
    n = title.shape[0]
    out = torch.full_like(title, float("nan")) if out is None else out
    nb = N.load().nrms_news_views_fuse_workspace_size(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=title.device)
    N.call("nrms_news_views_fuse", N.ptr(title), n, N.ptr(cat), N.ptr(sub), ctypes.byref(s), N.ptr(state),
           N.ptr(out), N.ptr(ws), nb, N.stream_handle(title.device))
    torch.cuda.synchronize()
    return out


# -- 1. nrms_views_prepare ------------------------------------------------------
@pytest.mark.parametrize("Cn", X.PREPARE_C)
def test_views_prepare(device, Cn):
    w = X.views_weights(Cn)
    cv64, sv64, cl64, sl64, pre = X.prepare_ref(w, torch.float64)
    cv32, sv32, cl32, sl32, _ = X.prepare_ref(w, torch.float32)
    assert all(bool((z < 0).any()) and bool((z > 0).any()) for z in pre)   # pre-activations of both signs
    _, _, state = _prepare(w, device)
    st = state.cpu()
    got_cv, got_sv = st[:Cn * D].view(Cn, D), st[Cn * D:2 * Cn * D].view(Cn, D)
    got_cl, got_sl = st[2 * Cn * D:2 * Cn * D + Cn], st[2 * Cn * D + Cn:2 * Cn * D + 2 * Cn]
    ok = True
    for name, got, r64, r32, z in (("cat_vec", got_cv, cv64, cv32, pre[0]), ("sub_vec", got_sv, sv64, sv32, pre[1])):
        ok &= C.report("views_prepare", f"C{Cn}", name, got, r64, r32)
        # the ReLU's zeros are exact zeros (away from a pre-activation at rounding level)
        clear = z < -1e-5
        assert bool((got[clear] == 0).all()) and bool((got >= 0).all()), name
    p64 = {k: v.double() for k, v in w.items()}
    for name, got, r64, r32, v64 in (("cat_logit", got_cl, cl64, cl32, cv64), ("sub_logit", got_sl, sl64, sl32, sv64)):
        t = torch.tanh(v64 @ p64["w_fin"].t() + p64["b_fin"])
        floor = float(torch.linalg.vector_norm(C.dot_floor_rows(t, p64["q_fin"].expand_as(t))))
        ok &= C.report("views_prepare", f"C{Cn}", name, got, r64, r32, floor_abs=floor)
    assert ok


# -- 2. nrms_news_views_fuse ----------------------------------------------------
@pytest.mark.parametrize("n", X.FUSE_N)
def test_news_views_fuse(device, n):
    """Against fp64 on states prepared by the kernel above; ids 0 and C - 1;
    in place bitwise the out-of-place call; ids -1 and C give NaN rows and
    leave the others' bits; a NaN title row stays in its row."""
    w = X.views_weights(X.FUSE_C)
    s, keep, state = _prepare(w, device)
    title, cat, sub = X.fuse_inputs(n)
    r64, wts = X.fuse_ref(title, cat, sub, w, torch.float64)
    r32, _ = X.fuse_ref(title, cat, sub, w, torch.float32)
    assert 0.02 < float(wts.min()) and float(wts.max()) < 0.95     # every view matters
    dt, dc, ds = title.to(device), cat.to(device), sub.to(device)
    out = _fuse(s, state, dt, dc, ds)
    assert C.report("news_views_fuse", f"n{n}", "out", out, r64, r32)
    inplace = dt.clone()
    assert _fuse(s, state, inplace, dc, ds, out=inplace) is inplace
    assert _same_bits(inplace, out)
    if n >= 127:
        bad_c, bad_s = dc.clone(), ds.clone()
        bad_c[3], bad_s[70], bad_c[n - 2] = -1, X.FUSE_C, X.FUSE_C
        got = _fuse(s, state, dt, bad_c, bad_s)
        rows = torch.zeros(n, dtype=torch.bool)
        rows[[3, 70, n - 2]] = True
        assert bool(torch.isnan(got.cpu()[rows]).all())
        assert _same_bits(got.cpu()[~rows], out.cpu()[~rows])
        nan_t = dt.clone()
        nan_t[65, 17] = float("nan")
        got = _fuse(s, state, nan_t, dc, ds)
        rows = torch.zeros(n, dtype=torch.bool)
        rows[65] = True
        assert bool(torch.isnan(got.cpu()[65]).all())
        assert _same_bits(got.cpu()[~rows], out.cpu()[~rows])


def test_news_views_fuse_dominant_view(device):
    """q_fin scaled by 1000: the logits reach hundreds, where a softmax without
    the maximum subtracted overflows. Every output is finite; rows whose
    largest fp64 weight is within 1e-6 of 1 (there the output's sensitivity
    to the logits' own rounding, (1 - w_max) |dl|, is below the rule's floor)
    meet the rule."""
    n = 129
    w = X.views_weights(X.FUSE_C, q_scale=1000.0)
    s, keep, state = _prepare(w, device)
    title, cat, sub = X.fuse_inputs(n)
    r64, wts = X.fuse_ref(title, cat, sub, w, torch.float64)
    r32, _ = X.fuse_ref(title, cat, sub, w, torch.float32)
    logit = state.cpu()[2 * X.FUSE_C * D:2 * X.FUSE_C * (D + 1)]
    assert float(logit.abs().max()) > 100.0
    top = wts.max(dim=1).values
    assert bool((top > 0.999).any())
    out = _fuse(s, state, title.to(device), cat.to(device), sub.to(device)).cpu()
    assert bool(torch.isfinite(out).all())
    sure = top >= 1 - 1e-6
    assert int(sure.sum()) >= 8
    assert C.report("news_views_fuse", "dominant", "out", out[sure], r64[sure], r32[sure])


# -- 3. nrms_rows_add_position --------------------------------------------------
def _add_position(src, n_src, rows, B, Nn, sb, sn, pos, Dd, device):
    N = _N()
    out = torch.full((B * Nn * Dd + 8,), float("nan"), device=device)
    N.call("nrms_rows_add_position", N.ptr(src), n_src, N.ptr(rows), B, Nn, sb, sn, N.ptr(pos), Dd, N.ptr(out),
           N.stream_handle(device))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[B * Nn * Dd:]).all())
    return out[:B * Nn * Dd].view(B, Nn, Dd)


@pytest.mark.parametrize("Dd", X.POSITION_D)
@pytest.mark.parametrize("B,Nn", X.POSITION_GATHER_BN)
def test_rows_add_position_gather(device, B, Nn, Dd):
    table, rows, pos = X.position_inputs(B, Nn, Dd)
    want = table[rows] + pos
    out = _add_position(table.to(device), table.shape[0], rows.to(device), B, Nn, 0, 0, pos.to(device), Dd, device)
    assert _same_bits(out, want)
    bad = rows.clone()
    bad.view(-1)[-1] = table.shape[0]
    bad.view(-1)[B * Nn // 2] = -1
    out = _add_position(table.to(device), table.shape[0], bad.to(device), B, Nn, 0, 0, pos.to(device), Dd, device)
    hit = (bad < 0) | (bad >= table.shape[0])
    assert bool(torch.isnan(out.cpu()[hit]).all())
    assert _same_bits(out.cpu()[~hit], want[~hit])


@pytest.mark.parametrize("Dd", X.POSITION_D)
@pytest.mark.parametrize("view", X.POSITION_VIEWS)
def test_rows_add_position_view(device, view, Dd):
    B, Nn = 3, 50
    g = X.gen(2401 + Dd)
    pos = X.uniform(g, Nn, Dd, lo=-0.1, hi=0.1)
    if view == "contiguous":
        base = X.randn(g, B, Nn, Dd).to(device)
        x = base
    elif view == "transposed":     # torch.stack(..., dim=0).transpose(0, 1), src/evaluate.py:220-224
        base = X.randn(g, Nn, B, Dd).to(device)
        x = base.transpose(0, 1)
    else:                          # a slice of a wider tensor: row stride Dd + 4
        base = X.randn(g, B, Nn, Dd + 4).to(device)
        x = base[:, :, :Dd]
    assert x.shape == (B, Nn, Dd) and x.stride(2) == 1
    want = x.cpu() + pos
    out = _add_position(x, 0, None, B, Nn, x.stride(0), x.stride(1), pos.to(device), Dd, device)
    assert _same_bits(out, want)


# -- 4. the module against the reference ---------------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def state(golden):
    return X.exp1_state(int(golden["seed"]), int(golden["V"]), int(golden["C"]))


@pytest.fixture(scope="module")
def inputs(golden):
    return X.golden_inputs(int(golden["seed"]), int(golden["V"]), int(golden["C"]))


def _model(state, device):
    from newsrecommendationsystem_amd import Exp1, Exp1Config
    V = state[f"{X.TITLE}.word_embedding.weight"].shape[0]
    Cn = state[f"{X.ELEMENT}.category.embedding.weight"].shape[0]
    m = Exp1(type("Cfg", (Exp1Config,), dict(num_words=V, num_categories=Cn)))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    return m.to(device).eval()


@pytest.fixture(scope="module")
def model(state, device):
    return _model(state, device)


def _np(t):
    return t.detach().cpu().numpy()


def test_get_news_vector(model, golden, inputs, gemm_mode):
    with torch.no_grad():
        out = _np(model.get_news_vector({k: torch.from_numpy(v) for k, v in inputs["news"].items()}))
    err = O.normwise_rel_err(out, golden["news_out"])
    print("exp1-module news", gemm_mode, err.max())
    assert err.max() < X.TOL


def test_get_user_vector(model, golden, inputs, device, gemm_mode):
    x = torch.from_numpy(inputs["user_in"]).to(device)
    with torch.no_grad():
        out = _np(model.get_user_vector(x))
        xt = x.transpose(0, 1).contiguous().transpose(0, 1)      # the reference caller's strided view
        assert not xt.is_contiguous()
        out_t = _np(model.get_user_vector(xt))
    print("exp1-module user", gemm_mode, O.normwise_rel_err(out, golden["user_out"]).max())
    assert O.normwise_rel_err(out, golden["user_out"]).max() < X.TOL
    assert O.normwise_rel_err(out_t, golden["user_out"]).max() < X.TOL


def test_forward(model, golden, inputs, gemm_mode):
    with torch.no_grad():
        y = _np(model(X.as_module_batch(inputs["fwd_cand"]), X.as_module_batch(inputs["fwd_clicked"])))
    ref = golden["fwd_out"]
    assert y.shape == ref.shape == (4, 5)
    print("exp1-module forward", gemm_mode, O.normwise_rel_err(y, ref).max())
    assert O.normwise_rel_err(y, ref).max() < X.TOL


def test_get_prediction(model, golden, inputs, device, gemm_mode):
    with torch.no_grad():
        out = _np(model.get_prediction(torch.from_numpy(inputs["pred_news"]).to(device),
                                       torch.from_numpy(inputs["pred_user"]).to(device)))
    assert O.normwise_rel_err(out.reshape(1, -1), golden["pred_out"].reshape(1, -1)).max() < X.TOL


def test_prepared_state_follows_the_weights(state, inputs, device):
    """final_attention.linear.weight changed in place: the prepared per-id
    table is stale, and get_news_vector must move as the restatement does."""
    m = _model(state, device)
    news = {k: torch.from_numpy(v) for k, v in inputs["news"].items()}
    n = inputs["news"]
    with torch.no_grad():
        before = _np(m.get_news_vector(news))
        m.news_encoder.final_attention.linear.weight.mul_(3.0)
        after = _np(m.get_news_vector(news))
    sd2 = dict(state)
    sd2[f"{X.FINAL}.linear.weight"] = state[f"{X.FINAL}.linear.weight"] * np.float32(3.0)
    want = X.news_encode(n["category"], n["subcategory"], n["title"], sd2)
    assert O.normwise_rel_err(after, want).max() < X.TOL
    assert np.median(O.normwise_rel_err(before, want)) > 100 * X.TOL


# -- 5. evaluate / predict / recommend on the golden split ------------------------
def test_evaluate_matches_the_reference(model, golden):
    from newsrecommendationsystem_amd import data as Dt
    from newsrecommendationsystem_amd.evaluate import EvalPlan, evaluate, score_plan
    got = evaluate(model, SPLIT)
    print("exp1-evaluate", got, golden["eval_tuple"])
    np.testing.assert_allclose(got, golden["eval_tuple"], rtol=0, atol=1e-6)
    corpus = Dt.read_news_parsed(os.path.join(SPLIT, "news_parsed.tsv"))
    imps = Dt.load_behaviors(os.path.join(SPLIT, "behaviors.tsv"))
    scores, metrics = score_plan(model, EvalPlan(corpus, imps))
    np.testing.assert_allclose(_np(metrics), golden["eval_metrics"], rtol=0, atol=1e-6, equal_nan=True)
    ref = golden["eval_y_pred"]
    assert np.abs(_np(scores) - ref).max() <= X.TOL * np.abs(ref).max()


def test_predict_scores_are_score_plans(model):
    from newsrecommendationsystem_amd import data as Dt
    from newsrecommendationsystem_amd import predict as P
    from newsrecommendationsystem_amd.evaluate import EvalPlan, score_plan
    corpus = Dt.read_news_parsed(os.path.join(SPLIT, "news_parsed.tsv"))
    imps = Dt.load_behaviors_any(os.path.join(SPLIT, "behaviors.tsv"))
    pred = P.predict_split(model, corpus, imps)
    scores, _ = score_plan(model, EvalPlan(corpus, Dt.load_behaviors(os.path.join(SPLIT, "behaviors.tsv"))))
    assert pred.scores.shape == tuple(scores.shape) and len(pred) == 12
    assert _same_bits(torch.from_numpy(pred.scores), scores)


def test_recommend_split(model, gemm_mode):
    """Rows whose scores are the fp64 dots of the module's own vectors within
    topk_cases.tolerance, none of them from the user's history."""
    from newsrecommendationsystem_amd import data as Dt
    from newsrecommendationsystem_amd import recommend as R
    from newsrecommendationsystem_amd.evaluate import category_args, news_vectors, user_vectors
    corpus = Dt.read_news_parsed(os.path.join(SPLIT, "news_parsed.tsv"))
    imps = Dt.load_behaviors(os.path.join(SPLIT, "behaviors.tsv"))
    k = 5
    res = R.recommend_split(model, corpus, imps, k=k)
    users, hists = R.first_lines(imps)
    assert res.users == users and len(users) > 1
    hrows = R.history_rows(corpus, hists, 50)
    tab = news_vectors(model, corpus.titles, **category_args(model, corpus))
    nv = _np(tab[:len(corpus)])
    uv = _np(user_vectors(model, tab, hrows))
    y, tol = T.scores64(nv, uv), T.tolerance(nv, uv)
    for u in range(len(users)):
        rows = res.rows[u]
        rows = rows[rows >= 0]
        assert len(rows) == min(k, len(corpus) - len({r for r in hrows[u].tolist() if 0 <= r < len(corpus)}))
        assert not set(hists[u].split()[:50]) & set(res.news_ids[u])
        assert (np.abs(res.scores[u, :len(rows)] - y[u, rows]) <= tol[u, rows]).all()
        assert (np.diff(res.scores[u, :len(rows)]) <= 0).all()
