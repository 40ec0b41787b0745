"""Host side of prediction, no GPU: the label-optional native reader
(nrms_behaviors_scan_any / _parse_any), the Python readers, PredictPlan, the
prediction file, and nrms_rank_impressions' argument checks (nothing is
launched)."""
import ctypes
import zipfile

import numpy as np
import pytest

from newsrecommendationsystem_amd import _native as N
from newsrecommendationsystem_amd import data as Dt
from newsrecommendationsystem_amd import predict as P
from newsrecommendationsystem_amd.evaluate import EvalPlan
from tests.predict_cases import strip_labels

LABELLED = ("1\tU1\tt\t\tN3-1 N0-0\n"
            "2\tU2\tt\t N1 N2 \tN5-01 N6-0\n\n"
            "3\tU1\tt\t\tN7-1\n"
            "4\tU9\tt\tN1 N2\tN11-0 N10-1 N9-0\textra\n")
UNLABELLED = ("1\tU1\tt\t\tN3 N0\n"
              "2\tU2\tt\t N1 N2 \tN5 N6\n\n"
              "3\tU1\tt\t\tN7\n"
              "4\tU9\tt\tN1 N2\tN11 N10 N9\textra\n")
MIXED = ("1\tU1\tt\t\tN3-1 N0\n"
         "2\tU2\tt\t N1 N2 \tN5 N6-0\n\n"
         "3\tU1\tt\t\tN7\n"
         "4\tU9\tt\tN1 N2\tN11-0 N10 N9-0\textra\n")
# the rejection cases of tests/test_eval_cpu.py::test_native_behaviors_edge_forms
REJECTED = ("1\tU1\tt\tN1\tN3-1\r\n", "1\tU1\tt\tN1  N2\tN3-1\n", "1\tU1\tt\tN01\tN3-1\n",
            "1\tU1\tt\tN1\tN3-1  N4-0\n", "1\tU1\tt\tN1\n", "1\tU1\tt\tN1\tN3-1 \n", "1\tU\xe9\tt\tN1\tN3-1\n",
            "1\tU1\tt\tN1\tN3-\n", "1\tU1\tt\tN1\tN03-1\n")
# ... and their label-less counterparts
REJECTED_BARE = ("1\tU1\tt\tN1\tN3\r\n", "1\tU1\tt\tN1\tN3  N4\n", "1\tU1\tt\tN1\tN3 \n", "1\tU1\tt\tN1\tN03\n",
                 "1\tU1\tt\tN1\tN3x\n", "1\tU1\tt\tN1\t3\n", "1\tU1\tt\tN1\t\n", "1\tU1\tt\tN1\tN3 N4-\n")


def _native(text, any_form, capacity=None):
    """(status of scan, status of parse, arrays) of the native pair on `text`."""
    lib = N.load()
    scan = lib.nrms_behaviors_scan_any if any_form else lib.nrms_behaviors_scan
    parse = lib.nrms_behaviors_parse_any if any_form else lib.nrms_behaviors_parse
    buf = text.encode("utf-8")
    A = lambda a: a.ctypes.data
    cap = np.zeros(3, np.int64)
    st_scan = scan(buf, len(buf), A(cap))
    if capacity is not None:
        cap = np.array(capacity, np.int64)
    elif st_scan != N.NRMS_OK:
        cap = np.array([8, 64, 64], np.int64)
    n, nc, nh = (int(x) for x in cap)
    out = dict(fields=np.zeros((n, 5, 2), np.int64), cand_num=np.zeros(nc, np.int64), labels=np.zeros(nc, np.int32),
               cand_count=np.zeros(n, np.int64), hist_num=np.zeros(nh, np.int64), hist_count=np.zeros(n, np.int64),
               hist_user=np.zeros(n, np.int64), counts=np.zeros(4, np.int64), cap=cap)
    st = parse(buf, len(buf), A(cap), A(out["counts"]), A(out["fields"]), A(out["cand_num"]), A(out["labels"]),
               A(out["cand_count"]), A(out["hist_num"]), A(out["hist_count"]), A(out["hist_user"]))
    return st_scan, st, out


def _trim(o):
    n, nc, nh = (int(x) for x in o["counts"][:3])
    return dict(cand_num=o["cand_num"][:nc], labels=o["labels"][:nc], cand_count=o["cand_count"][:n],
                hist_num=o["hist_num"][:nh], hist_count=o["hist_count"][:n], hist_user=o["hist_user"][:n],
                counts=o["counts"])


def test_native_any_reader_on_labelled_unlabelled_and_mixed_cells():
    s0, st0, old = _native(LABELLED, any_form=False)
    assert (s0, st0) == (N.NRMS_OK, N.NRMS_OK)
    ref = _trim(old)
    assert ref["labels"].tolist() == [1, 0, 1, 0, 1, 0, 1, 0]
    want_labels = {"labelled": ref["labels"].tolist(), "unlabelled": [-1] * 8,
                   "mixed": [1, -1, -1, 0, -1, 0, -1, 0]}
    for name, text in (("labelled", LABELLED), ("unlabelled", UNLABELLED), ("mixed", MIXED)):
        s, st, got = _native(text, any_form=True)
        assert (s, st) == (N.NRMS_OK, N.NRMS_OK), name
        # the scan's bounds hold: lines, candidate tokens (no '-' to count), history ids
        assert (got["cap"] >= got["counts"][:3]).all(), name
        assert got["cap"][1] == 8, name                       # the token count of the impressions columns
        g = _trim(got)
        for k in ("cand_num", "cand_count", "hist_num", "hist_count", "hist_user", "counts"):
            assert np.array_equal(g[k], ref[k]), (name, k)
        assert g["labels"].tolist() == want_labels[name] and g["labels"].dtype == np.int32, name
    # the byte spans of the columns are those of the text itself
    _, _, got = _native(UNLABELLED, any_form=True)
    a, b = got["fields"][3, 4]
    assert UNLABELLED[a:b] == "N11 N10 N9"


def test_old_pair_still_declines_unlabelled_cells():
    for text in (UNLABELLED, MIXED, "1\tU1\tt\tN1\tN3\n"):
        _, st, _ = _native(text, any_form=False, capacity=[8, 64, 64])
        assert st == N.NRMS_ERR_UNSUPPORTED


@pytest.mark.parametrize("text", REJECTED + REJECTED_BARE)
def test_native_any_reader_rejections(text):
    s, st, _ = _native(text, any_form=True)
    assert st == N.NRMS_ERR_UNSUPPORTED, repr(text)
    assert s in (N.NRMS_OK, N.NRMS_ERR_UNSUPPORTED)
    if "\r" in text or "\xe9" in text:
        assert s == N.NRMS_ERR_UNSUPPORTED                    # the byte check is the scan's as well


def test_native_any_reader_short_capacity():
    _, _, full = _native(UNLABELLED, any_form=True)
    n, nc, nh = (int(x) for x in full["counts"][:3])
    for cap in ([n - 1, nc, nh], [n, nc - 1, nh], [n, nc, nh - 1], [n, 0, nh]):
        _, st, _ = _native(UNLABELLED, any_form=True, capacity=cap)
        assert st == N.NRMS_ERR_WORKSPACE, cap
    _, st, _ = _native(UNLABELLED, any_form=True, capacity=[n, nc, nh])
    assert st == N.NRMS_OK
    lib = N.load()
    assert lib.nrms_behaviors_scan_any(b"x", 1, None) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_behaviors_scan_any(None, 1, np.zeros(3, np.int64).ctypes.data) == N.NRMS_ERR_INVALID_ARG


def _raw(cell):
    return Dt.Impression("1", "U1", "t", " ", raw=cell)


def test_parse_candidate_cells_takes_both_token_forms():
    cells = ["N1-0 N2-1", "N3 N4", "N5-1 N6", " N7  N8-10 ", "N-1-0 X9"]
    names, counts = Dt.parse_candidate_cells([_raw(c) for c in cells])
    assert names == ["N1", "N2", "N3", "N4", "N5", "N6", "N7", "N8", "N", "X9"]
    assert counts.tolist() == [2, 2, 2, 2, 2] and counts.dtype == np.int64
    # an impression built from lists, without a raw cell
    names, counts = Dt.parse_candidate_cells([Dt.Impression("1", "U", "t", " ", ["N4", "N2"], [0, 1])])
    assert names == ["N4", "N2"] and counts.tolist() == [2]
    names, counts = Dt.parse_candidate_cells([])
    assert names == [] and counts.shape == (0,)
    # the labelled parser keeps the reference's error on such a cell
    with pytest.raises(IndexError):
        Dt.parse_impression_cells([_raw("N3 N4")])


def _write(path, text):
    with open(path, "w", newline="") as f:
        f.write(text)


def _plan_arrays(plan):
    return {k: getattr(plan, k) for k in ("cand", "offsets", "imp_user", "hist_rows")}


def test_load_behaviors_any_native_and_fallback_agree(tmp_path):
    corpus = Dt.NewsCorpus([f"N{i}" for i in range(12)], np.arange(240).reshape(12, 20))
    p = str(tmp_path / "b.tsv")
    _write(p, UNLABELLED)
    tab = Dt.load_behaviors_any(p)
    assert isinstance(tab, Dt.BehaviorsTable) and (tab.labels == -1).all()
    _write(p, UNLABELLED.replace("\n", "\r\n"))               # CRLF: the native reader declines
    assert Dt.read_behaviors_native(p, any_form=True) is None
    _write(p, UNLABELLED.replace("N3 N0", "N3  N0"))          # a double space: declined too
    imps = Dt.load_behaviors_any(p)
    assert isinstance(imps, list) and len(imps) == len(tab) == 4
    for a, b in zip(tab, imps):
        assert (a.impression_id, a.user, a.time, a.clicked_news) == (b.impression_id, b.user, b.time, b.clicked_news)
    p1, p2 = P.PredictPlan(corpus, tab, num_clicked=3), P.PredictPlan(corpus, imps, num_clicked=3)
    for k, a in _plan_arrays(p1).items():
        b = getattr(p2, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert p1.impression_ids == p2.impression_ids == ["1", "2", "3", "4"]
    assert p1.cand.tolist() == [3, 0, 5, 6, 7, 11, 10, 9] and p1.offsets.tolist() == [0, 2, 4, 5, 8]
    assert p1.imp_user.tolist() == [0, 1, 0, 2]
    assert p1.hist_rows.tolist() == [[12, 12, 12], [12, 1, 2], [12, 1, 2]]
    # a labelled file reads the same through load_behaviors_any
    _write(p, LABELLED)
    p3 = P.PredictPlan(corpus, Dt.load_behaviors_any(p), num_clicked=3)
    for k, a in _plan_arrays(p1).items():
        assert np.array_equal(a, getattr(p3, k)), k


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict_split")
    corpus, imps = Dt.synthetic_split(str(d), seed=3, n_news=300, n_users=40, n_impressions=120, V=512)
    return str(d), corpus, imps


@pytest.mark.parametrize("reader", ["table", "list", "names"])
def test_predict_plan_equals_eval_plan_without_labels(split, tmp_path, reader):
    d, corpus, _ = split
    bare = str(tmp_path / "behaviors.tsv")
    strip_labels(d + "/behaviors.tsv", bare)
    want = EvalPlan(corpus, Dt.read_behaviors(d + "/behaviors.tsv"))
    if reader == "table":
        imps = Dt.load_behaviors_any(bare)
        assert isinstance(imps, Dt.BehaviorsTable)
    else:
        imps = Dt.read_behaviors(bare)
    if reader == "names":                                     # ids outside the numeric form: corpus.index
        corpus = Dt.NewsCorpus(corpus.ids + ["PADDING-LIKE"], np.vstack([corpus.titles, corpus.titles[:1]]))
        assert Dt.numeric_news_index(corpus) is None
        want = EvalPlan(corpus, Dt.read_behaviors(d + "/behaviors.tsv"))
    plan = P.PredictPlan(corpus, imps)
    assert plan.n_impressions == want.n_impressions == 120
    for k in ("cand", "offsets", "hist_rows"):
        a, b = getattr(plan, k), getattr(want, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert np.array_equal(np.repeat(plan.imp_user, np.diff(plan.offsets)), want.pair_user)
    assert plan.impression_ids == [str(k + 1) for k in range(120)]
    # a labelled split gives the same plan: the labels are ignored
    lab = P.PredictPlan(corpus, Dt.read_behaviors(d + "/behaviors.tsv"))
    for k, a in _plan_arrays(plan).items():
        assert np.array_equal(a, getattr(lab, k)), k


def test_predict_plan_unknown_id_raises(split):
    _, corpus, _ = split
    with pytest.raises(KeyError):
        P.PredictPlan(corpus, [Dt.Impression("x", "U1", "t", " ", raw="N1 N99999")])
    with pytest.raises(KeyError):
        P.PredictPlan(corpus, [Dt.Impression("x", "U1", "t", "N1 N99999", raw="N1")])
    with pytest.raises(KeyError):
        P.PredictPlan(corpus, [Dt.Impression("x", "U1", "t", " ", raw="N1 NOPE")])


def test_prediction_file_exact_bytes_and_round_trip(tmp_path):
    pred = P.Predictions(["7", "8", "imp-9"], [0, 3, 3, 5], np.array([2, 1, 3, 1, 2], np.int32),
                         np.zeros(5, np.float32))
    want = b"7 [2,1,3]\n8 []\nimp-9 [1,2]\n"
    plain, zipped = str(tmp_path / "prediction.txt"), str(tmp_path / "prediction.zip")
    P.write_prediction(plain, pred)
    with open(plain, "rb") as f:
        assert f.read() == want
    P.write_prediction(zipped, pred, zip=True)
    with zipfile.ZipFile(zipped) as z:
        assert z.namelist() == ["prediction.txt"] and z.read("prediction.txt") == want
    for path in (plain, zipped):
        back = P.read_prediction(path)
        assert back.impression_ids == pred.impression_ids and back.scores is None
        assert np.array_equal(back.offsets, pred.offsets) and np.array_equal(back.ranks, pred.ranks)
        assert back.ranks.dtype == np.int32 and len(back) == 3
        assert back.ranks_of(2).tolist() == [1, 2]
    # a larger ragged round trip
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 40, 200)
    off = np.concatenate([[0], np.cumsum(counts)])
    ranks = np.concatenate([rng.permutation(c) + 1 for c in counts]).astype(np.int32)
    big = P.Predictions([str(i) for i in range(200)], off, ranks)
    P.write_prediction(plain, big)
    back = P.read_prediction(plain)
    assert back.impression_ids == big.impression_ids
    assert np.array_equal(back.offsets, off) and np.array_equal(back.ranks, ranks)


def test_numpy_ranks_definition():
    s = np.array([0.5, np.nan, 0.5, -0.0, 0.0, np.inf, np.nan, -np.inf], np.float32)
    off = np.array([0, 8])
    order = P.numpy_ranks(s, off, "order")
    assert (np.argsort(order) == [6, 1, 5, 2, 0, 4, 3, 7]).all()       # the order the issue states
    assert P.numpy_ranks(s, off, "shared").tolist() == [4, 1, 4, 6, 6, 3, 1, 8]


def test_rank_impressions_rejects_bad_arguments_without_launch():
    lib = N.load()
    p = ctypes.c_void_p(4096)            # never dereferenced: every call below returns before a launch
    call = lib.nrms_rank_impressions
    ok = dict(news=p, n_news=100, user=p, n_users=8, news_idx=p, imp_user=p, offsets=p, n_imp=4, D=300,
              tie_mode=0, out_score=p, out_rank=p, stream=None)

    def status(**kw):
        a = dict(ok, **kw)
        return call(a["news"], a["n_news"], a["user"], a["n_users"], a["news_idx"], a["imp_user"], a["offsets"],
                    a["n_imp"], a["D"], a["tie_mode"], a["out_score"], a["out_rank"], a["stream"])

    for name in ("news", "user", "news_idx", "imp_user", "offsets", "out_score", "out_rank"):
        assert status(**{name: None}) == N.NRMS_ERR_INVALID_ARG, name
    for tm in (-1, 2, 7):
        assert status(tie_mode=tm) == N.NRMS_ERR_INVALID_ARG, tm
        assert status(tie_mode=tm, n_imp=0) == N.NRMS_ERR_INVALID_ARG, tm
    assert status(n_imp=-1) == N.NRMS_ERR_INVALID_ARG
    assert status(n_news=-1) == N.NRMS_ERR_INVALID_ARG
    assert status(n_users=-1) == N.NRMS_ERR_INVALID_ARG
    assert status(D=0) == N.NRMS_ERR_INVALID_ARG
    assert status(n_imp=2 ** 31) == N.NRMS_ERR_UNSUPPORTED
    # no impressions: success, nothing launched, no pointer and no stream needed
    for tm in (N.NRMS_RANK_ORDER, N.NRMS_RANK_SHARED):
        assert status(n_imp=0, tie_mode=tm) == N.NRMS_OK
        assert status(n_imp=0, tie_mode=tm, news=None, user=None, news_idx=None, imp_user=None, offsets=None,
                      out_score=None, out_rank=None) == N.NRMS_OK
    assert N.ABI_VERSION == 9 and lib.nrms_abi_version() == 9           # additive: no bump
    assert N.NRMS_RANK_LDS_CANDIDATES == 2048
