"""Weights, fp64 restatement and case tables of the Exp1 tests
(tests/test_exp1_cpu.py, tests/test_gpu_exp1.py, tests/golden/gen_golden_exp1.py).
Pure numpy / torch on the CPU.

exp1_state draws a full Exp1 state dict with the reference's 29 key names from
oracle.weights' splitmix64 primitives, at the reference's initialisers' scales.
The restatement (news_encode, user_encode, forward) is written from the
formulas of src/model/Exp1/: the NRMS title encoder (oracle.nrms_oracle's
attention primitives under Exp1's parameter names), relu(emb[id] W^T + b) per
element, an additive attention over the stacked views [title, category,
subcategory], and position_embedding added to the history before the user
encoder. tests/test_exp1_cpu.py pins it to the reference's own outputs.
"""
import numpy as np
import torch

from oracle import nrms_oracle as O
from oracle import weights as W
from tests.train_kernel_cases import D, Q, gen, randn, uniform

TOL = 1e-5               # tests/test_gpu_parity.py's bound, per output vector
E = 100                  # category_embedding_dim
N_CLICKED = 50
GOLDEN_SEED, GOLDEN_V, GOLDEN_C = 20261021, 256, 9
TITLE = "news_encoder.text_encoders.title"
ELEMENT = "news_encoder.element_encoders"
FINAL = "news_encoder.final_attention"


def exp1_state(seed, V=256, C=9):
    """Full Exp1 state_dict (numpy float32) with the reference's key names
    (src/model/Exp1/). The category embedding is one table under both element
    encoders; its row 0 is drawn like the others (padding_idx only affects
    gradients, and an all-zero row would hide a kernel that skips id 0)."""
    sd = {f"{TITLE}.word_embedding.weight": W.normal(seed, 1, (V, D))}
    for k, v in W.encoder_params(seed, 100, D, Q).items():
        sd[f"{TITLE}.{k}"] = v
    emb = W.normal(seed, 300, (C, E))
    eb = float(1.0 / np.sqrt(E))
    for i, name in enumerate(("category", "subcategory")):
        sd[f"{ELEMENT}.{name}.embedding.weight"] = emb
        sd[f"{ELEMENT}.{name}.linear.weight"] = W.uniform(seed, 310 + 2 * i, (D, E), -eb, eb)
        sd[f"{ELEMENT}.{name}.linear.bias"] = W.uniform(seed, 311 + 2 * i, (D,), -eb, eb)
    lb = float(1.0 / np.sqrt(D))
    sd[f"{FINAL}.attention_query_vector"] = W.uniform(seed, 320, (Q,), -0.1, 0.1)
    sd[f"{FINAL}.linear.weight"] = W.uniform(seed, 321, (Q, D), -lb, lb)
    sd[f"{FINAL}.linear.bias"] = W.uniform(seed, 322, (Q,), -lb, lb)
    for k, v in W.encoder_params(seed, 200, D, Q).items():
        sd["user_encoder." + k] = v
    sd["user_encoder.position_embedding"] = W.uniform(seed, 330, (N_CLICKED, D), -0.1, 0.1)
    return sd


def state_shapes(sd):
    return {k: tuple(v.shape) for k, v in sd.items()}


# ---------------------------------------------------------------- restatement
def title_encode(ids, sd, dt=np.float64):
    x = O.embedding_gather(sd[f"{TITLE}.word_embedding.weight"], ids).astype(dt)
    h = O.multihead_self_attention(x, sd, f"{TITLE}.multihead_self_attention", dt=dt)
    return O.additive_attention(h, sd, f"{TITLE}.additive_attention", dt)


def element_encode(ids, sd, name, dt=np.float64):
    """relu(emb[id] W^T + b): [n] -> [n, D]."""
    emb = sd[f"{ELEMENT}.{name}.embedding.weight"][np.asarray(ids)]
    return np.maximum(O.linear(emb, sd[f"{ELEMENT}.{name}.linear.weight"], sd[f"{ELEMENT}.{name}.linear.bias"], dt),
                      dt(0))


def view_weights(views, sd, dt=np.float64):
    """Softmax weights [n, 3] of the final attention over views [n, 3, D]."""
    n, k, d = views.shape
    t = np.tanh(O.linear(views.reshape(n * k, d), sd[f"{FINAL}.linear.weight"], sd[f"{FINAL}.linear.bias"], dt))
    s = (t @ sd[f"{FINAL}.attention_query_vector"].astype(dt)).reshape(n, k)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def news_views(category, subcategory, title_ids, sd, dt=np.float64):
    """[n, 3, D]: the title, category and subcategory views."""
    return np.stack([title_encode(title_ids, sd, dt), element_encode(category, sd, "category", dt),
                     element_encode(subcategory, sd, "subcategory", dt)], axis=1)


def news_encode(category, subcategory, title_ids, sd, dt=np.float64):
    views = news_views(category, subcategory, title_ids, sd, dt)
    return np.einsum("nk,nkd->nd", view_weights(views, sd, dt), views).astype(dt)


def user_encode(clicked_vec, sd, dt=np.float64):
    x = np.asarray(clicked_vec, dtype=dt) + sd["user_encoder.position_embedding"].astype(dt)[None]
    return O.user_encode(x, sd, dt)


def forward(cand, clicked, sd, dt=np.float64):
    """cand / clicked: dicts of category [B, C], subcategory [B, C], title
    [B, C, L] (and [B, N, ...]) -> logits [B, C]."""
    def enc(x):
        B, C, L = x["title"].shape
        return news_encode(x["category"].reshape(-1), x["subcategory"].reshape(-1), x["title"].reshape(B * C, L),
                           sd, dt).reshape(B, C, -1)
    return O.click_score(enc(cand), user_encode(enc(clicked), sd, dt), dt)


# ---------------------------------------------------------------- golden inputs
def golden_inputs(seed=GOLDEN_SEED, V=GOLDEN_V, C=GOLDEN_C):
    """The inputs of tests/golden/exp1_golden.npz, regenerable anywhere (the
    fixture holds the reference's outputs only)."""
    d = {}
    t = W.titles(seed, 20, 64, V)
    t[0, :] = 0                                        # an all-padding title
    t[1, :] = W.randint(seed, 21, (20,), 1, V)          # a full-length title
    cat, sub = W.randint(seed, 22, (64,), 0, C), W.randint(seed, 23, (64,), 0, C)
    cat[2], sub[2] = 0, 0
    cat[3], sub[4] = C - 1, C - 1
    d["news"] = dict(category=cat, subcategory=sub, title=t)
    u = W.normal(seed, 30, (8, N_CLICKED, D), 0.3)
    u_len = W.randint(seed, 31, (8,), 1, N_CLICKED + 1)
    u_len[0], u_len[1] = N_CLICKED, 1
    for b in range(8):
        u[b, :N_CLICKED - u_len[b]] = 0.0              # left-padded with PADDED_NEWS vectors
    d["user_in"], d["user_len"] = u, u_len
    cand, clk, hist = W.impressions(seed, 40, 4, V)
    B, Cn, N = cand.shape[0], cand.shape[1], clk.shape[1]
    pad = np.arange(N)[None, :] < (N - hist)[:, None]
    d["fwd_cand"] = dict(category=W.randint(seed, 44, (B, Cn), 1, C), subcategory=W.randint(seed, 45, (B, Cn), 1, C),
                         title=cand)
    d["fwd_clicked"] = dict(category=np.where(pad, 0, W.randint(seed, 46, (B, N), 1, C)),
                            subcategory=np.where(pad, 0, W.randint(seed, 47, (B, N), 1, C)), title=clk)
    d["pred_news"], d["pred_user"] = W.normal(seed, 50, (7, D), 0.5), W.normal(seed, 51, (D,), 0.5)
    return d


def as_module_batch(x):
    """{key: [B, C, ...]} -> the reference's list of C dicts of [B, ...] tensors."""
    return [{k: torch.from_numpy(np.ascontiguousarray(v[:, i])) for k, v in x.items()}
            for i in range(x["title"].shape[1])]


# ---------------------------------------------------------------- kernel cases
PREPARE_C = (1, 2, 9, 275)
FUSE_N = (1, 127, 128, 129, 257)      # the score GEMM's 128-row tile (BM, gemm_f32.hip) and the combine's 64 rows
FUSE_C = 9
POSITION_GATHER_BN = ((1, 50), (2, 50), (3, 50), (5, 1), (70, 3))   # 50 / 100 / 150 rows: the 64-row block cuts a user
POSITION_TABLE_ROWS = 41
POSITION_D = (300, 7)
POSITION_VIEWS = ("contiguous", "transposed", "slice")


def views_weights(C, seed=2101, q_scale=1.0):
    """fp32 parameters of nrms_views_weights_t at the initialisers' scales; the
    element linears' biases are spread so that pre-activations take both signs."""
    g = gen(seed + C)
    a, b = 1.0 / np.sqrt(E), 1.0 / np.sqrt(D)
    w = dict(emb=randn(g, C, E), w_cat=uniform(g, D, E, lo=-a, hi=a), b_cat=uniform(g, D, lo=-0.5, hi=0.5),
             w_sub=uniform(g, D, E, lo=-a, hi=a), b_sub=uniform(g, D, lo=-0.5, hi=0.5),
             w_fin=uniform(g, Q, D, lo=-b, hi=b), b_fin=uniform(g, Q, lo=-b, hi=b),
             q_fin=uniform(g, Q, lo=-0.1, hi=0.1) * q_scale)
    return w


def prepare_ref(w, dtype):
    """(cat_vec [C, D], sub_vec [C, D], cat_logit [C], sub_logit [C]) in `dtype`, plus the pre-activations."""
    p = {k: v.to(dtype) for k, v in w.items()}
    out, pre = [], []
    for n in ("cat", "sub"):
        z = p["emb"] @ p["w_" + n].t() + p["b_" + n]
        pre.append(z)
        out.append(torch.relu(z))
    logit = [torch.tanh(v @ p["w_fin"].t() + p["b_fin"]) @ p["q_fin"] for v in out]
    return out[0], out[1], logit[0], logit[1], pre


def fuse_inputs(n, C=FUSE_C, seed=2201):
    """title vectors [n, D] at the title encoder's scale, ids covering 0 and C - 1."""
    g = gen(seed + n)
    title = randn(g, n, D, scale=0.3)
    cat = torch.randint(0, C, (n,), generator=g, dtype=torch.int64)
    sub = torch.randint(0, C, (n,), generator=g, dtype=torch.int64)
    cat[0], sub[0] = 0, C - 1
    cat[-1], sub[-1] = C - 1, 0
    return title, cat, sub


def fuse_ref(title, cat, sub, w, dtype):
    """out [n, D] and the softmax weights [n, 3], ids assumed in range."""
    cv, sv, _, _, _ = prepare_ref(w, dtype)
    p = {k: v.to(dtype) for k, v in w.items()}
    views = torch.stack([title.to(dtype), cv[cat], sv[sub]], dim=1)
    wts = torch.softmax(torch.tanh(views @ p["w_fin"].t() + p["b_fin"]) @ p["q_fin"], dim=1)
    return (wts.unsqueeze(-1) * views).sum(1), wts


def position_inputs(B, N, Dd, seed=2301):
    g = gen(seed + 1000 * B + 10 * N + Dd)
    table = randn(g, POSITION_TABLE_ROWS, Dd)
    table[-1] = 0.0                                    # the PADDED_NEWS row
    rows = torch.randint(0, POSITION_TABLE_ROWS, (B, N), generator=g, dtype=torch.int64)
    rows[0, 0] = POSITION_TABLE_ROWS - 1
    pos = uniform(g, N, Dd, lo=-0.1, hi=0.1)
    return table, rows, pos
