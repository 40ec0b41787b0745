"""Exp1 on MI355X: NRMS with category views and a position embedding.

Drop-in for ``model.Exp1.Exp1`` (src/model/Exp1/__init__.py:7-80), inference
only: same constructor ``Exp1(config, pretrained_word_embedding=None)``, same
``forward`` / ``get_news_vector`` / ``get_user_vector`` / ``get_prediction``
signatures and the reference's module tree, so ``state_dict()`` has its 29
keys and a ``MODEL_NAME=Exp1`` checkpoint loads unchanged.

What Exp1 adds to NRMS (src/model/Exp1/news_encoder.py, user_encoder.py):
  * the title goes through the NRMS news encoder
    (``news_encoder.text_encoders.title`` is an nrms.NewsEncoder, its HIP
    forward reused whole);
  * category and subcategory go through Embedding -> Linear -> ReLU, both
    over one shared nn.Embedding(num_categories, 100, padding_idx=0);
  * a second additive attention (``final_attention``) pools the three views;
  * the user encoder adds ``position_embedding[50, 300]`` to the history
    before its self-attention.
The element encoders depend on the id alone, so they are folded once per
parameter version into a per-id table with each row's attention logit
(nrms_views_prepare); per article the library computes the title's logit,
the three-way softmax and the weighted sum (nrms_news_views_fuse), and the
position add is one pass fused with the eval path's row gather
(nrms_rows_add_position). Everything else is the NRMS kernels.

View order. The reference builds its ModuleDicts from set intersections, so
the order in which it stacks (title, category, subcategory) changes with
Python's string hash seed. Pooling over views does not depend on the order up
to fp32 rounding; here the sum is always (w_t title + w_c category) + w_s
subcategory. Results therefore agree with the reference at a tolerance, never
bitwise.

Limits: a call in training mode raises NotImplementedError (the reference
trains Exp1 as an ensemble under NLLLoss, src/train.py:100-104,192-200: not
built here), and the only attribute set is Exp1Config's
['category', 'subcategory', 'title'].
"""
import ctypes
import sys

import torch
import torch.nn as nn

from . import _native as N
from . import nrms
from .config import Exp1Config

ATTRIBUTES = ["category", "subcategory", "title"]


def _no_training(what):
    raise NotImplementedError(f"Exp1.{what} in training mode: this build runs Exp1 for inference only "
                              "(call model.eval()); training Exp1 is not implemented")


class ElementEncoder(nn.Module):
    """Parameter holder for src/model/Exp1/news_encoder.py:36-43."""

    def __init__(self, embedding, linear_input_dim, linear_output_dim):
        super().__init__()
        self.embedding = embedding
        self.linear = nn.Linear(linear_input_dim, linear_output_dim)


class NewsEncoder(nn.Module):
    """src/model/Exp1/news_encoder.py:46-111, forward on the HIP path."""

    def __init__(self, config, pretrained_word_embedding=None):
        super().__init__()
        self.config = config
        self.text_encoders = nn.ModuleDict({"title": nrms.NewsEncoder(config, pretrained_word_embedding)})
        category_embedding = nn.Embedding(config.num_categories, config.category_embedding_dim, padding_idx=0)
        self.element_encoders = nn.ModuleDict({
            name: ElementEncoder(category_embedding, config.category_embedding_dim, config.word_embedding_dim)
            for name in ("category", "subcategory")})
        self.final_attention = nrms.AdditiveAttention(config.query_vector_dim, config.word_embedding_dim)
        self._ws = nrms._Workspace()
        self._views = None   # (key, ViewsWeights, tensors it points into, state buffer)

    @property
    def word_embedding(self):
        """The title encoder's table (the eval passes read its device and width)."""
        return self.text_encoders["title"].word_embedding

    def _view_params(self):
        cat, sub = self.element_encoders["category"], self.element_encoders["subcategory"]
        fin = self.final_attention
        return [cat.embedding.weight, sub.embedding.weight, cat.linear.weight, cat.linear.bias, sub.linear.weight,
                sub.linear.bias, fin.linear.weight, fin.linear.bias, fin.attention_query_vector]

    def _views_key(self):
        return tuple((p.data_ptr(), p._version) for p in self._view_params())

    def views_state(self):
        """(nrms_views_weights_t, prepared state) for the current parameters:
        the per-id view vectors and logits, prepared again when the storage or
        the version of any parameter they are made from changes (the cache-key
        style of nrms.NewsEncoder._fold_key)."""
        key = self._views_key()
        if self._views is not None and self._views[0] == key:
            return self._views[1], self._views[3]
        keep = [nrms._f32(p.detach()) for p in self._view_params()]
        emb_c, emb_s, w_c, b_c, w_s, b_s, w_f, b_f, q_f = keep
        C, E = emb_c.shape
        D, Q = w_c.shape[0], w_f.shape[0]
        P = lambda t: t.data_ptr()
        w = N.ViewsWeights(P(emb_c), P(emb_s), C, E, P(w_c), P(b_c), P(w_s), P(b_s), P(w_f), P(b_f), P(q_f), D, Q)
        nb = N.load().nrms_views_state_size(C, D)
        dev = emb_c.device
        state = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
        N.call("nrms_views_prepare", ctypes.byref(w), N.ptr(state), state.numel(), N.stream_handle(dev))
        if not torch.cuda.is_current_stream_capturing():   # other streams may read the state next
            torch.cuda.current_stream(dev).synchronize()
        self._views = (key, w, keep, state)
        return w, state

    def _element_ids(self, ids, name):
        dev = self.final_attention.attention_query_vector.device
        ids = torch.as_tensor(ids)
        if getattr(self.config, "hip_check_ids", True) and ids.numel():
            lo, hi = torch.aminmax(ids)
            if int(lo) < 0 or int(hi) >= self.element_encoders[name].embedding.num_embeddings:
                raise IndexError("index out of range in self")
        return ids.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous().reshape(-1)

    def forward(self, news):
        if self.training:
            _no_training("news_encoder")
        cat = self._element_ids(news["category"], "category")
        sub = self._element_ids(news["subcategory"], "subcategory")
        out = self.text_encoders["title"]({"title": news["title"]})
        n, D = out.shape
        if cat.numel() != n or sub.numel() != n:
            raise ValueError(f"{n} titles with {cat.numel()} categories and {sub.numel()} subcategories")
        if n == 0:
            return out
        w, state = self.views_state()
        ws = self._ws.get(N.load().nrms_news_views_fuse_workspace_size(n), out.device)
        N.call("nrms_news_views_fuse", N.ptr(out), n, N.ptr(cat), N.ptr(sub), ctypes.byref(w), N.ptr(state),
               N.ptr(out), N.ptr(ws), ws.numel(), N.stream_handle(out.device))
        return out


class UserEncoder(nrms.UserEncoder):
    """src/model/Exp1/user_encoder.py:7-31, forward on the HIP path."""

    def __init__(self, config):
        nn.Module.__init__(self)
        self.config = config
        self.multihead_self_attention = nrms.MultiHeadSelfAttention(config.word_embedding_dim,
                                                                    config.num_attention_heads)
        self.position_embedding = nn.Parameter(
            torch.empty(config.num_clicked_news_a_user, config.word_embedding_dim).uniform_(-0.1, 0.1))
        self.additive_attention = nrms.AdditiveAttention(config.query_vector_dim, config.word_embedding_dim)
        self._ws = nrms._Workspace()

    def _position(self, n_clicked, D):
        pos = nrms._f32(self.position_embedding.detach())
        if tuple(pos.shape) != (n_clicked, D):
            raise ValueError(f"history of shape [*, {n_clicked}, {D}] against position_embedding "
                             f"{tuple(pos.shape)}")
        return pos

    def add_position(self, user_vector):
        """user_vector + position_embedding as a contiguous [B, N, D]; strided
        views (the transpose(0, 1) of src/evaluate.py:220-224) are read in place."""
        pos = self.position_embedding
        x = user_vector.to(pos.device)
        if x.dtype != torch.float32 or x.stride(2) != 1:
            x = nrms._f32(x)
        B, n_clicked, D = x.shape
        pos = self._position(n_clicked, D)
        out = torch.empty(B, n_clicked, D, dtype=torch.float32, device=pos.device)
        if B:
            N.call("nrms_rows_add_position", N.ptr(x), 0, None, B, n_clicked, x.stride(0), x.stride(1), N.ptr(pos), D,
                   N.ptr(out), N.stream_handle(pos.device))
        return out

    def add_position_rows(self, table, rows):
        """table[rows] + position_embedding in one pass: rows int64 [B, N] on
        the device index the [n, D] table (the eval path's gather)."""
        B, n_clicked = rows.shape
        D = table.shape[1]
        pos = self._position(n_clicked, D)
        out = torch.empty(B, n_clicked, D, dtype=torch.float32, device=table.device)
        if B:
            N.call("nrms_rows_add_position", N.ptr(table), table.shape[0], N.ptr(rows), B, n_clicked, 0, 0,
                   N.ptr(pos), D, N.ptr(out), N.stream_handle(table.device))
        return out

    def encode_positioned(self, x):
        """The NRMS user encoder over a history that already carries its position."""
        return nrms.UserEncoder.forward(self, x)

    def forward(self, user_vector):
        if self.training:
            _no_training("user_encoder")
        return self.encode_positioned(self.add_position(user_vector))


class Exp1(nn.Module):
    """Exp1 network (src/model/Exp1/__init__.py:7-80), eval mode."""

    def __init__(self, config=Exp1Config, pretrained_word_embedding=None):
        super().__init__()
        attrs = list(config.dataset_attributes["news"])
        if sorted(attrs) != ATTRIBUTES:
            raise ValueError(f"Exp1 is built for the news attributes {ATTRIBUTES}, not {attrs}")
        self.config = config
        self.news_encoder = NewsEncoder(config, pretrained_word_embedding)
        self.user_encoder = UserEncoder(config)
        self.click_predictor = nrms.DotProductClickPredictor()

    def load_state_dict(self, state_dict, *args, **kwargs):
        """nn.Module.load_state_dict; the two element encoders share one
        embedding (the reference cannot save them unequal), so a state whose
        two entries differ is refused instead of keeping one of them."""
        a = state_dict.get("news_encoder.element_encoders.category.embedding.weight")
        b = state_dict.get("news_encoder.element_encoders.subcategory.embedding.weight")
        if a is not None and b is not None and (a.shape != b.shape or not torch.equal(a.cpu(), b.cpu())):
            raise ValueError("Exp1 state dict: the category and subcategory embeddings differ, "
                             "but the model shares one table between them")
        return super().load_state_dict(state_dict, *args, **kwargs)

    def forward(self, candidate_news, clicked_news):
        """candidate_news: list (1+K) of {"category": [B], "subcategory": [B],
        "title": [B, L]}; clicked_news: list (N) of the same -> logits
        [B, 1+K]. All B (1+K+N) articles go through the title encoder and the
        view attention in one call each (src/model/Exp1/__init__.py:15-44)."""
        if self.training:
            _no_training("forward")
        C, n_clicked = len(candidate_news), len(clicked_news)
        B = candidate_news[0]["title"].shape[0]

        def stacked(key):   # [B (C + N), ...]: the candidates of every sample, then the histories
            cand = torch.stack([torch.as_tensor(x[key]) for x in candidate_news], dim=1)
            clk = torch.stack([torch.as_tensor(x[key]) for x in clicked_news], dim=1)
            return torch.cat([cand.reshape(B * C, *cand.shape[2:]), clk.reshape(B * n_clicked, *clk.shape[2:])])

        vec = self.news_encoder({k: stacked(k) for k in ATTRIBUTES})
        D = vec.shape[1]
        user = self.user_encoder(vec[B * C:].view(B, n_clicked, D))
        return self.click_predictor(vec[:B * C].view(B, C, D), user)

    def get_news_vector(self, news):
        if self.training:
            _no_training("get_news_vector")
        return self.news_encoder(news)

    def get_user_vector(self, clicked_news_vector):
        if self.training:
            _no_training("get_user_vector")
        return self.user_encoder(clicked_news_vector)

    def get_prediction(self, news_vector, user_vector):
        if self.training:
            _no_training("get_prediction")
        return self.click_predictor(news_vector.unsqueeze(dim=0), user_vector.unsqueeze(dim=0)).squeeze(dim=0)


# ------------------------------------------------------------------ benchmark
BENCH_NEWS, BENCH_CATEGORIES, BENCH_USERS, BENCH_CLICKED, BENCH_D = 42416, 275, 16384, 50, 300
HBM_PEAK_GBS = 8000.0   # one MI355X, HBM3E


def views_torch_route(title, cat, sub, ne):
    """nrms_news_views_fuse in torch ops (the reference's own sequence)."""
    enc = ne.element_encoders
    fin = ne.final_attention
    views = torch.stack([title] + [torch.relu(enc[k].linear(enc[k].embedding(i)))
                                   for k, i in (("category", cat), ("subcategory", sub))], dim=1)
    w = torch.softmax(torch.tanh(fin.linear(views)) @ fin.attention_query_vector, dim=1)
    return torch.bmm(w.unsqueeze(1), views).squeeze(1)


def bench(reps=20, warmup=3, out=sys.stdout):
    """Time the two new passes against the same computation in torch ops, and
    evaluate()'s GPU passes for an Exp1 and an NRMS model of equal sizes:
    device events, `warmup` runs then `reps` timed runs, alternating with the
    comparison in one process; median and min..max."""
    import tempfile

    import numpy as np

    from . import data as Dt
    from .evaluate import EvalPlan, score_plan
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    def alternate(first, second):
        for _ in range(warmup):
            first()
            second()
        t1, t2 = [], []
        for _ in range(reps):
            t1.append(timed(first)[0])
            t2.append(timed(second)[0])
        wins = sum(a < b for a, b in zip(t1, t2))
        return np.sort(t1), np.sort(t2), wins

    def line(name, t):
        return f"{name} {float(np.median(t)):8.3f} ms [{t[0]:.3f} .. {t[-1]:.3f}]"

    class Cfg(Exp1Config):
        num_words = 4096
        num_categories = BENCH_CATEGORIES

    print(f"exp1 bench: {reps} reps after {warmup} warm-up, alternating, device events", file=out)
    with torch.no_grad():
        model = Exp1(Cfg).to(dev).eval()
        ne, ue = model.news_encoder, model.user_encoder
        # (a) the view attention over a catalogue of title vectors
        title = torch.randn(BENCH_NEWS, BENCH_D, generator=g).to(dev)
        cat = torch.randint(0, BENCH_CATEGORIES, (BENCH_NEWS,), generator=g).to(dev)
        sub = torch.randint(0, BENCH_CATEGORIES, (BENCH_NEWS,), generator=g).to(dev)
        w, state = ne.views_state()
        res = torch.empty_like(title)
        ws = torch.empty(N.load().nrms_news_views_fuse_workspace_size(BENCH_NEWS), dtype=torch.uint8, device=dev)
        st = N.stream_handle(dev)

        def fuse():
            N.call("nrms_news_views_fuse", N.ptr(title), BENCH_NEWS, N.ptr(cat), N.ptr(sub), ctypes.byref(w),
                   N.ptr(state), N.ptr(res), N.ptr(ws), ws.numel(), st)
            return res
        tf, tt, wins = alternate(fuse, lambda: views_torch_route(title, cat, sub, ne))
        err = float((fuse() - views_torch_route(title, cat, sub, ne)).abs().max())
        # title read twice (GEMM, combine), two view rows read, out written, ids and logits
        moved = BENCH_NEWS * (5 * BENCH_D * 4 + 2 * 8 + 2 * 4)
        gbs = moved / (float(np.median(tf)) * 1e-3) / 1e9
        print(f"  (a) nrms_news_views_fuse, {BENCH_NEWS} articles, C = {BENCH_CATEGORIES}: {line('hip', tf)} | "
              f"{line('torch', tt)} | hip faster in {wins}/{reps} pairs | {moved / 1e6:.1f} MB moved, "
              f"{gbs:.0f} GB/s = {100 * gbs / HBM_PEAK_GBS:.1f} % of HBM peak | max |diff| {err:.2e}", file=out)

        # (b) the gathering position add against gather + torch add
        table = torch.randn(BENCH_NEWS + 1, BENCH_D, generator=g).to(dev)
        rows = torch.randint(0, BENCH_NEWS + 1, (BENCH_USERS, BENCH_CLICKED), generator=g).to(dev)
        pos = ue.position_embedding

        def two_pass():
            x = torch.empty(BENCH_USERS * BENCH_CLICKED, BENCH_D, dtype=torch.float32, device=dev)
            N.call("nrms_embedding_gather", N.ptr(rows), BENCH_USERS * BENCH_CLICKED, N.ptr(table), table.shape[0],
                   BENCH_D, N.ptr(x), st)
            return x.view(BENCH_USERS, BENCH_CLICKED, BENCH_D) + pos
        tf, tt, wins = alternate(lambda: ue.add_position_rows(table, rows), two_pass)
        same = bool(torch.equal(ue.add_position_rows(table, rows), two_pass()))
        moved = BENCH_USERS * BENCH_CLICKED * (2 * BENCH_D * 4 + 8)
        gbs = moved / (float(np.median(tf)) * 1e-3) / 1e9
        print(f"  (b) nrms_rows_add_position, {BENCH_USERS} x {BENCH_CLICKED} rows from {table.shape[0]}: "
              f"{line('hip', tf)} | {line('gather + torch add', tt)} | hip faster in {wins}/{reps} pairs | "
              f"{gbs:.0f} GB/s = {100 * gbs / HBM_PEAK_GBS:.1f} % of HBM peak | bitwise equal: {same}", file=out)
        del title, table, rows, res

        # (c) evaluate()'s GPU passes, Exp1 against NRMS
        with tempfile.TemporaryDirectory() as tmp:
            corpus, imps = Dt.synthetic_split(tmp, seed=0, V=Cfg.num_words)
            rng = np.random.default_rng(0)
            cats = rng.integers(0, BENCH_CATEGORIES, (2, len(corpus)))
            Dt.write_news_parsed(tmp + "/news_parsed.tsv", corpus.ids, corpus.titles, cats[0], cats[1])
            corpus = Dt.read_news_parsed(tmp + "/news_parsed.tsv")
            corpus.categories()
        plan = EvalPlan(corpus, imps)

        class CfgN(nrms.NRMSConfig):
            num_words = Cfg.num_words
        base = nrms.NRMS(CfgN).to(dev).eval()
        te, tn, wins = alternate(lambda: score_plan(model, plan), lambda: score_plan(base, plan))
        print(f"  (c) evaluate() GPU passes, {len(corpus)} news, {plan.hist_rows.shape[0]} histories, "
              f"{plan.n_impressions} impressions: {line('Exp1', te)} | {line('NRMS', tn)} | "
              f"Exp1 / NRMS {float(np.median(te)) / float(np.median(tn)):.2f}x", file=out)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Exp1 on the HIP path")
    ap.add_argument("--bench", action="store_true", help="time the view and position kernels against torch")
    a = ap.parse_args(argv)
    if not a.bench:
        ap.error("nothing to do (--bench)")
    bench()
    return 0


if __name__ == "__main__":
    sys.exit(main())
