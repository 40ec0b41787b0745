"""Exp1 without a GPU: the module tree, the fp64 restatement against the
reference's outputs (tests/golden/exp1_golden.npz), checkpoint loading, the
category columns of news_parsed.tsv, the limits that raise, and the argument
checks of the three new C entry points."""
import csv
import ctypes
import hashlib
import os

import numpy as np
import pytest
import torch

from newsrecommendationsystem_amd import _native as N
from oracle import nrms_oracle as O
from tests import exp1_cases as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "exp1_golden.npz")
SPLIT = os.path.join(ROOT, "tests", "golden", "exp1", "eval")


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


def small_config(V=64, C=9):
    from newsrecommendationsystem_amd import Exp1Config
    return type("Cfg", (Exp1Config,), dict(num_words=V, num_categories=C))


def test_state_dict_has_the_references_keys_and_shapes(golden, state):
    from newsrecommendationsystem_amd import Exp1
    want = {k: tuple(int(x) for x in s if x) for k, s in zip(golden["state_keys"].tolist(), golden["state_shapes"])}
    assert len(want) == 29
    m = Exp1(small_config(int(golden["V"]), int(golden["C"])))
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want
    assert X.state_shapes(state) == want
    enc = m.news_encoder.element_encoders
    assert enc["category"].embedding is enc["subcategory"].embedding
    p = m.user_encoder.position_embedding
    assert isinstance(p, torch.nn.Parameter) and float(p.detach().abs().max()) <= 0.1
    # the generated state is the one the golden was made from
    h = hashlib.sha256()
    for k in sorted(state):
        h.update(k.encode())
        h.update(np.ascontiguousarray(state[k], dtype=np.float32).tobytes())
    assert h.hexdigest() == str(golden["state_sha256"])


def test_plugin_path_and_exports():
    import newsrecommendationsystem_amd as P
    from newsrecommendationsystem_amd.model.Exp1 import Exp1
    assert Exp1 is P.Exp1 and P.Exp1Config.dataset_attributes["news"] == ["category", "subcategory", "title"]
    assert N.load().nrms_abi_version() == 9


def test_restatement_reproduces_the_reference(golden, state, inputs):
    n = inputs["news"]
    news = X.news_encode(n["category"], n["subcategory"], n["title"], state)
    err = O.normwise_rel_err(news, golden["news_out"])
    print("exp1-restatement news", err.max())
    assert err.max() < X.TOL
    user = X.user_encode(inputs["user_in"], state)
    err = O.normwise_rel_err(user, golden["user_out"])
    print("exp1-restatement user", err.max())
    assert err.max() < X.TOL
    y = X.forward(inputs["fwd_cand"], inputs["fwd_clicked"], state)
    err = O.normwise_rel_err(y, golden["fwd_out"])
    print("exp1-restatement forward", err.max())
    assert err.max() < X.TOL
    p = O.get_prediction(inputs["pred_news"], inputs["pred_user"], np.float64)
    err = O.normwise_rel_err(p.reshape(1, -1), golden["pred_out"].reshape(1, -1))
    print("exp1-restatement prediction", err.max())
    assert err.max() < X.TOL


def test_golden_discriminates(golden, state, inputs):
    """The conditions the generator asserts, checked on the committed file's
    inputs: a dropped or swapped view, or a missing position, moves the
    outputs by far more than TOL."""
    n = inputs["news"]
    views = X.news_views(n["category"], n["subcategory"], n["title"], state)
    w = X.view_weights(views, state)
    assert 0.05 <= w.min() and w.max() <= 0.9
    assert (n["category"] != n["subcategory"]).mean() >= 0.5
    assert (np.abs(state["user_encoder.position_embedding"]).max(axis=1) > 0).all()
    swapped = np.einsum("nk,nkd->nd", w, views[:, [0, 2, 1]])
    assert np.median(O.normwise_rel_err(swapped, golden["news_out"])) > 1e-2
    no_pos = O.user_encode(inputs["user_in"], state, np.float64)
    assert O.normwise_rel_err(no_pos, golden["user_out"]).min() > 1e-3


def test_load_model_round_trip(tmp_path, state):
    from newsrecommendationsystem_amd import NRMS, Exp1, NRMSConfig
    from newsrecommendationsystem_amd.checkpoint import load, load_model
    sd = {k: torch.from_numpy(v) for k, v in state.items()}
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(3))], lr=1e-4)
    path = str(tmp_path / "ckpt-7.pth")
    torch.save({"model_state_dict": sd, "optimizer_state_dict": opt.state_dict(), "step": 7,
                "early_stop_value": np.float64(-0.61)}, path)     # src/train.py:266-277
    assert load(path)["step"] == 7                                 # weights_only=True inside
    m = load_model(path)
    assert isinstance(m, Exp1) and not m.training
    assert (m.config.num_words, m.config.num_categories, m.config.num_clicked_news_a_user) == (256, 9, 50)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # an NRMS file still gives an NRMS
    base = NRMS(type("Cfg", (NRMSConfig,), dict(num_words=32)))
    path_n = str(tmp_path / "ckpt-1.pth")
    torch.save({"model_state_dict": base.state_dict(), "optimizer_state_dict": opt.state_dict(), "step": 1,
                "early_stop_value": np.float64(-0.5)}, path_n)
    mn = load_model(path_n)
    assert type(mn) is NRMS and mn.config.num_words == 32
    # unequal shared embeddings: refused
    bad = dict(sd)
    bad["news_encoder.element_encoders.subcategory.embedding.weight"] = sd[
        "news_encoder.element_encoders.subcategory.embedding.weight"] + 1.0
    path_b = str(tmp_path / "ckpt-2.pth")
    torch.save({"model_state_dict": bad, "optimizer_state_dict": opt.state_dict(), "step": 2,
                "early_stop_value": np.float64(-0.5)}, path_b)
    with pytest.raises(ValueError, match="embeddings differ"):
        load_model(path_b)


def _old_write_news_parsed(path, ids, titles):
    """The writer as it was before it took category columns."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", quoting=csv.QUOTE_NONE, escapechar="\\", lineterminator="\n")
        w.writerow(["id", "category", "subcategory", "title", "abstract", "title_entities", "abstract_entities"])
        zero_a = str([0] * 50)
        for nid, t in zip(ids, titles):
            w.writerow([nid, 0, 0, "[" + ", ".join(str(int(x)) for x in t) + "]", zero_a, str([0] * len(t)), zero_a])


def test_news_categories_round_trip(tmp_path):
    from newsrecommendationsystem_amd import data as Dt
    rng = np.random.default_rng(5)
    ids = [f"N{i}" for i in range(17)]
    titles = rng.integers(0, 99, (17, 20))
    cat, sub = rng.integers(0, 275, 17), rng.integers(0, 275, 17)
    p = str(tmp_path / "news_parsed.tsv")
    Dt.write_news_parsed(p, ids, titles, cat, sub)
    c2, s2 = Dt.read_news_categories(p)
    assert c2.dtype == np.int64 and s2.dtype == np.int64
    np.testing.assert_array_equal(c2, cat)
    np.testing.assert_array_equal(s2, sub)
    for read in (Dt.read_news_parsed, Dt.read_news_parsed_py):
        corpus = read(p)
        assert corpus.ids == ids
        np.testing.assert_array_equal(corpus.titles, titles)
    corpus = Dt.read_news_parsed(p)
    np.testing.assert_array_equal(corpus.categories()[0], cat)
    np.testing.assert_array_equal(corpus.categories()[1], sub)
    with pytest.raises(ValueError):
        Dt.NewsCorpus(ids, titles).categories()
    # without categories: byte for byte the old writer's file
    q, r = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    Dt.write_news_parsed(q, ids, titles)
    _old_write_news_parsed(r, ids, titles)
    with open(q, "rb") as f, open(r, "rb") as g:
        assert f.read() == g.read()
    c0, s0 = Dt.read_news_categories(q)
    assert not c0.any() and not s0.any()


def test_golden_split_has_category_columns(golden):
    from newsrecommendationsystem_amd import data as Dt
    corpus = Dt.read_news_parsed(os.path.join(SPLIT, "news_parsed.tsv"))
    cat, sub = corpus.categories()
    assert len(corpus) == 40 and cat.min() >= 1 and max(cat.max(), sub.max()) < int(golden["C"])
    assert (cat != sub).any()
    assert len(Dt.load_behaviors(os.path.join(SPLIT, "behaviors.tsv"))) == len(golden["eval_metrics"]) == 12


def test_limits_raise():
    from newsrecommendationsystem_amd import Exp1, Exp1Config
    for attrs in (["title"], ["category", "title"], ["category", "subcategory", "title", "abstract"]):
        cfg = type("Cfg", (Exp1Config,), dict(num_words=16, num_categories=4,
                                              dataset_attributes={"news": attrs, "record": []}))
        with pytest.raises(ValueError, match="attributes"):
            Exp1(cfg)
    m = Exp1(small_config(16, 4))
    assert m.training
    news = [{"category": torch.zeros(2, dtype=torch.int64), "subcategory": torch.zeros(2, dtype=torch.int64),
             "title": torch.zeros(2, 20, dtype=torch.int64)}]
    with pytest.raises(NotImplementedError, match="training"):
        m(news, news)
    with pytest.raises(NotImplementedError, match="training"):
        m.get_news_vector(news[0])
    with pytest.raises(NotImplementedError, match="training"):
        m.get_user_vector(torch.zeros(1, 50, 300))


# ---------------------------------------------------------------- C entry points, no device
P = ctypes.c_void_p
A16, A4 = 4096, 4100     # stand-in addresses: never dereferenced, every call below is rejected first


def _views(**kw):
    f = dict(emb_cat=A16, emb_sub=A16, n_cat=9, emb_dim=100, w_cat=A16, b_cat=A16, w_sub=A16, b_sub=A16, w_fin=A16,
             b_fin=A16, q_fin=A16, d_model=300, query_dim=200)
    f.update(kw)
    return N.ViewsWeights(**f)


POINTERS = ("emb_cat", "emb_sub", "w_cat", "b_cat", "w_sub", "b_sub", "w_fin", "b_fin", "q_fin")


def test_views_prepare_rejects_bad_arguments():
    lib = N.load()
    size = lib.nrms_views_state_size(9, 300)
    assert size == 9 * (2 * 300 + 2) * 4
    assert lib.nrms_views_state_size(-1, 300) == 0 and lib.nrms_views_state_size(9, 0) == 0
    call = lambda w, state=P(A16), nb=size: lib.nrms_views_prepare(ctypes.byref(w) if w else None, state, nb, None)
    assert call(None) == N.NRMS_ERR_INVALID_ARG
    for name in POINTERS:
        assert call(_views(**{name: None})) == N.NRMS_ERR_INVALID_ARG, name
    for name in ("emb_dim", "d_model", "query_dim"):
        assert call(_views(**{name: 0})) == N.NRMS_ERR_INVALID_ARG, name
    assert call(_views(n_cat=-1)) == N.NRMS_ERR_INVALID_ARG
    assert call(_views(), state=None) == N.NRMS_ERR_INVALID_ARG
    assert call(_views(), nb=size - 1) == N.NRMS_ERR_WORKSPACE
    assert call(_views(query_dim=209)) == N.NRMS_ERR_UNSUPPORTED
    assert call(_views(emb_dim=12000)) == N.NRMS_ERR_UNSUPPORTED
    assert call(_views(n_cat=0)) == N.NRMS_OK          # nothing to prepare, nothing launched


def test_news_views_fuse_rejects_bad_arguments():
    lib = N.load()
    assert lib.nrms_news_views_fuse_workspace_size(0) == 0 and lib.nrms_news_views_fuse_workspace_size(-3) == 0
    nb = lib.nrms_news_views_fuse_workspace_size(129)
    assert nb >= 129 * 4

    def call(w=None, **kw):
        a = dict(title=P(A16), n=129, cat=P(A16), sub=P(A16), state=P(A16), out=P(A16), ws=P(A16), nb=nb)
        a.update(kw)
        w = _views() if w is None else w
        return lib.nrms_news_views_fuse(a["title"], a["n"], a["cat"], a["sub"], ctypes.byref(w), a["state"],
                                        a["out"], a["ws"], a["nb"], None)
    for name in ("title", "cat", "sub", "state", "out"):
        assert call(**{name: None}) == N.NRMS_ERR_INVALID_ARG, name
    for name in POINTERS:
        assert call(_views(**{name: None})) == N.NRMS_ERR_INVALID_ARG, name
    assert call(n=-1) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_news_views_fuse(P(A16), 1, P(A16), P(A16), None, P(A16), P(A16), P(A16), nb, None) \
        == N.NRMS_ERR_INVALID_ARG
    assert call(ws=None) == N.NRMS_ERR_WORKSPACE
    assert call(nb=129 * 4 - 1) == N.NRMS_ERR_WORKSPACE
    assert call(title=P(A4)) == N.NRMS_ERR_UNSUPPORTED
    assert call(out=P(A4)) == N.NRMS_ERR_UNSUPPORTED
    assert call(state=P(A4)) == N.NRMS_ERR_UNSUPPORTED
    assert call(_views(d_model=302)) == N.NRMS_ERR_UNSUPPORTED
    assert call(n=0, title=None, cat=None, sub=None, out=None, ws=None, nb=0) == N.NRMS_OK


def test_rows_add_position_rejects_bad_arguments():
    lib = N.load()

    def call(**kw):
        a = dict(src=P(A16), n_src=41, rows=P(A16), B=3, N=50, sb=0, sn=0, pos=P(A16), D=300, out=P(A16))
        a.update(kw)
        return lib.nrms_rows_add_position(a["src"], a["n_src"], a["rows"], a["B"], a["N"], a["sb"], a["sn"],
                                          a["pos"], a["D"], a["out"], None)
    for name in ("src", "pos", "out"):
        assert call(**{name: None}) == N.NRMS_ERR_INVALID_ARG, name
    for name in ("B", "n_src", "sb", "sn"):
        assert call(**{name: -1}) == N.NRMS_ERR_INVALID_ARG, name
    for name in ("N", "D"):
        assert call(**{name: 0}) == N.NRMS_ERR_INVALID_ARG, name
    assert call(N=2 ** 20, D=2 ** 20) == N.NRMS_ERR_UNSUPPORTED
    assert call(B=2 ** 40) == N.NRMS_ERR_UNSUPPORTED
    assert call(B=0, src=None, pos=None, out=None) == N.NRMS_OK
