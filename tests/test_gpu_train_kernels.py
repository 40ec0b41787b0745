"""Each training kernel of include/nrms_hip.h alone against its fp64 reference
(tests/train_kernel_cases.py), at the tile and dispatch edges of its launch
code: one entry point per test, inputs drawn on the CPU in fp64 and rounded to
fp32, what an earlier stage would hand over (y_tanh, scores, qkv) taken from
the fp64 reference, never from another HIP kernel.

One tolerance rule for every floating-point output (train_kernel_cases.errors):
e_hip <= max(4 e_32, 1e-6 n, floor_abs), e_32 the error of the same reference
evaluated in fp32 on the CPU. Every output prints one line under -s; the
MI355X printout is profiles/train_kernel_errors.txt.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import train_kernel_cases as K

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3


class AdamTensor(ctypes.Structure):
    """nrms_adam_tensor_t."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_int64), ("first_block", ctypes.c_int64)]


def _N():
    from newsrecommendationsystem_amd import _native
    return _native


def _status(name, *args):
    return getattr(_N().load(), name)(*args)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _nan(device, *shape):
    return torch.full(shape, float("nan"), device=device)


@functools.lru_cache(maxsize=None)
def _host_weights():
    return K.encoder_weights(7)


def _weights(device):
    """nrms_encoder_weights_t over device copies, as nrms.py's weights()."""
    N = _N()
    keep = [_host_weights()[f].to(device).contiguous() for f in K.WEIGHT_FIELDS]
    return N.EncoderWeights(*[t.data_ptr() for t in keep], K.D, K.H, K.Q), keep


def _guarded(nbytes, device):
    """A workspace of exactly nbytes at the head of a buffer 4 KiB larger,
    and the byte pattern of that tail."""
    buf = torch.zeros(nbytes + 4096, dtype=torch.uint8, device=device)
    tail = (torch.arange(4096, device=device) % 251).to(torch.uint8)
    buf[nbytes:] = tail
    return buf, tail


# -- 1. nrms_dropout ----------------------------------------------------------

@pytest.mark.parametrize("seed", K.DROPOUT_SEEDS)
@pytest.mark.parametrize("p", K.DROPOUT_P)
def test_dropout_bitwise(device, p, seed):
    N = _N()
    st = N.stream_handle(device)
    for n in K.DROPOUT_N:
        x = K.randn(K.gen(100 + n), n)
        want = torch.from_numpy(K.dropout_np(x.numpy(), p, seed))
        xd = x.to(device)
        y = _nan(device, n + 8)
        N.call("nrms_dropout", N.ptr(xd), N.ptr(y), n, ctypes.c_float(p), ctypes.c_uint64(seed), st)
        assert _same_bits(y[:n], want), (n, p, seed)
        assert bool(torch.isnan(y[n:]).all())
        assert _same_bits(xd, x)
        N.call("nrms_dropout", N.ptr(xd), N.ptr(xd), n, ctypes.c_float(p), ctypes.c_uint64(seed), st)   # in place
        assert _same_bits(xd, want), (n, p, seed, "in place")
        if p == 0:
            assert _same_bits(xd, x)


def test_dropout_empty_and_rejected_p(device):
    N = _N()
    st = N.stream_handle(device)
    x = K.randn(K.gen(1), 300).to(device)
    y0 = K.randn(K.gen(2), 300).to(device)
    y = y0.clone()
    assert _status("nrms_dropout", N.ptr(x), N.ptr(y), 0, ctypes.c_float(0.2), ctypes.c_uint64(1), st) == OK
    assert _status("nrms_dropout", None, None, 0, ctypes.c_float(0.2), ctypes.c_uint64(1), st) == OK
    for p in K.DROPOUT_BAD_P:   # rejected in capi.hip before any launch
        assert _status("nrms_dropout", N.ptr(x), N.ptr(y), 300, ctypes.c_float(p), ctypes.c_uint64(1), st) == INVALID
    assert _same_bits(y, y0)


# -- 2. nrms_score_backward -----------------------------------------------------

@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,C,Dd", K.SCORE_SHAPES)
def test_score_backward(device, B, C, Dd, strided):
    N = _N()
    news, user, dl = K.score_inputs(B, C, Dd)
    r64 = K.score_backward_ref(news.double(), user.double(), dl.double())
    r32 = K.score_backward_ref(news, user, dl)
    if strided:   # news a view into [B, C + 2, D + 4], user rows at stride D + 4
        nb0 = K.randn(K.gen(9), B, C + 2, Dd + 4)
        ub0 = K.randn(K.gen(10), B, Dd + 4)
        nb0[:, 1:C + 1, 2:Dd + 2] = news
        ub0[:, 1:Dd + 1] = user
        nb, ub = nb0.to(device), ub0.to(device)
        nv, uv = nb[:, 1:C + 1, 2:Dd + 2], ub[:, 1:Dd + 1]
        assert nv.stride() == ((C + 2) * (Dd + 4), Dd + 4, 1) and uv.stride() == (Dd + 4, 1)
    else:
        nb0, ub0 = news, user
        nb, ub = news.to(device), user.to(device)
        nv, uv = nb, ub
    dnews, duser, dld = _nan(device, B * C * Dd + 16), _nan(device, B * Dd + 16), dl.to(device)
    N.call("nrms_score_backward", N.ptr(nv), B, C, nv.stride(0), nv.stride(1), N.ptr(uv), uv.stride(0), Dd,
           N.ptr(dld), N.ptr(dnews), N.ptr(duser), N.stream_handle(device))
    case = f"B{B}C{C}D{Dd}{'-strided' if strided else ''}"
    ok = [K.report("score_backward", case, "dnews", dnews[:B * C * Dd].view(B, C, Dd), r64[0], r32[0]),
          K.report("score_backward", case, "duser", duser[:B * Dd].view(B, Dd), r64[1], r32[1])]
    assert all(ok)
    # every element written, nothing past the end, the inputs (and what surrounds the views) untouched
    assert bool(torch.isnan(dnews[B * C * Dd:]).all()) and bool(torch.isnan(duser[B * Dd:]).all())
    assert _same_bits(nb, nb0) and _same_bits(ub, ub0)


# -- 3 / 4. additive attention ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def _additive_case(n_seq, L):
    """Inputs and fp64 / fp32 references of one (n_seq, L), computed once."""
    w = _host_weights()
    x, dout = K.additive_inputs(n_seq, L)
    wa, ba, qa = w["w_add"], w["b_add"], w["q_add"]
    f64 = K.additive_forward_ref(x.double(), wa.double(), ba.double(), qa.double())
    f32 = K.additive_forward_ref(x, wa, ba, qa)
    y, s = K.f32(f64[0]), K.f32(f64[1])   # what the backward receives: the fp64 forward, rounded
    b64 = K.additive_backward_ref(x.double(), wa.double(), qa.double(), y.double(), s.double(), dout.double())
    b32 = K.additive_backward_ref(x, wa, qa, y, s, dout)
    return x, dout, y, s, f64, f32, b64, b32


@pytest.mark.parametrize("n_seq,L", K.ADDITIVE_FWD_SHAPES)
def test_additive_forward_train(device, gemm_mode, n_seq, L):
    N = _N()
    x, _, _, _, f64, f32, _, _ = _additive_case(n_seq, L)
    w, keep = _weights(device)
    xd = x.to(device)
    y, s, out = _nan(device, n_seq, L, K.Q), _nan(device, n_seq, L), _nan(device, n_seq, K.D)
    N.call("nrms_additive_forward_train", N.ptr(xd), n_seq, L, ctypes.byref(w), N.ptr(y), N.ptr(s), N.ptr(out),
           N.stream_handle(device))
    case = f"{gemm_mode}-n{n_seq}L{L}"
    ok = [K.report("additive_forward_train", case, name, o, a, b, cap_rel=K.CAP_FORWARD)
          for name, o, a, b in zip(("y_tanh", "scores", "out"), (y, s, out), f64, f32)]
    assert all(ok)
    assert _same_bits(xd, x)


@pytest.mark.parametrize("n_seq,L", K.ADDITIVE_BWD_SHAPES)
def test_additive_backward(device, gemm_mode, n_seq, L):
    N = _N()
    lib = N.load()
    x, dout, y, s, _, _, b64, b32 = _additive_case(n_seq, L)
    w, keep = _weights(device)
    st = N.stream_handle(device)
    shapes = ((K.Q, K.D), (K.Q,), (K.Q,))
    g0 = [K.g0_pattern(*sh) for sh in shapes]
    ins = [t.to(device) for t in (x, y, s, dout)]
    nbytes = lib.nrms_additive_backward_workspace_size(n_seq, L, K.D, K.Q)
    assert nbytes > 0
    ws, tail = _guarded(nbytes, device)

    def run(ws_bytes):
        outs = [_nan(device, n_seq, L, K.D)] + [g.to(device) for g in g0]
        status = _status("nrms_additive_backward", N.ptr(ins[0]), n_seq, L, ctypes.byref(w), N.ptr(ins[1]),
                         N.ptr(ins[2]), N.ptr(ins[3]), *[N.ptr(o) for o in outs], N.ptr(ws), ws_bytes, st)
        return status, outs

    # one byte short: rejected in capi.hip before any launch, every output bitwise as it was
    status, outs = run(nbytes - 1)
    assert status == WORKSPACE
    assert bool(torch.isnan(outs[0]).all()) and all(_same_bits(o, g) for o, g in zip(outs[1:], g0))
    status, outs = run(nbytes)
    assert status == OK
    case = f"{gemm_mode}-n{n_seq}L{L}"
    ok = [K.report("additive_backward", case, "dx", outs[0], b64[0], b32[0])]
    for name, o, g, a, b in zip(("d_w_add", "d_b_add", "d_q_add"), outs[1:], g0, b64[1:], b32[1:]):
        floor = K.additive_floor(L, x, dout, g.numel())
        ok.append(K.report("additive_backward", case, name, o, g.double() + a, g + b, floor_abs=floor))
    assert all(ok), case
    assert torch.equal(ws[nbytes:], tail)
    assert all(_same_bits(a, b) for a, b in zip(ins, (x, y, s, dout)))


# -- 5. nrms_self_attention_backward ------------------------------------------------

@pytest.mark.parametrize("L,n_seq,regime", K.MHSA_CASES)
def test_self_attention_backward(device, L, n_seq, regime):
    N = _N()
    qkv, dctx = K.mhsa_inputs(L, n_seq, regime)
    r64 = K.mhsa_backward_ref(qkv.double(), dctx.double(), n_seq, L)
    r32 = K.mhsa_backward_ref(qkv, dctx, n_seq, L)
    w, keep = _weights(device)
    qd, dd = qkv.to(device), dctx.to(device)
    dqkv = _nan(device, n_seq * L * 3 * K.D + 64)
    N.call("nrms_self_attention_backward", N.ptr(qd), N.ptr(dd), n_seq, L, ctypes.byref(w), N.ptr(dqkv),
           N.stream_handle(device))
    out = dqkv[:n_seq * L * 3 * K.D].view(n_seq * L, 3 * K.D)
    assert bool(torch.isfinite(out).all())            # all 900 columns of every row written
    assert bool(torch.isnan(dqkv[n_seq * L * 3 * K.D:]).all())
    floor = K.mhsa_floor(L, qkv, dctx)
    case = f"L{L}n{n_seq}-{regime}"
    ok = [K.report("self_attention_backward", case, name, out[:, i * K.D:(i + 1) * K.D],
                   r64[:, i * K.D:(i + 1) * K.D], r32[:, i * K.D:(i + 1) * K.D], floor_abs=floor if i < 2 else 0.0)
          for i, name in enumerate(("dq", "dk", "dv"))]
    assert all(ok), case
    assert _same_bits(qd, qkv) and _same_bits(dd, dctx)


def test_self_attention_backward_rejects_long_sequences(device):
    N = _N()
    L, n_seq = K.MHSA_UNSUPPORTED_L, 1
    qkv, dctx = K.mhsa_inputs(L, n_seq, "normal")
    w, keep = _weights(device)
    dqkv, qd, dd = _nan(device, n_seq * L, 3 * K.D), qkv.to(device), dctx.to(device)
    # L > 64: launch_mhsa_backward returns before its launch
    status = _status("nrms_self_attention_backward", N.ptr(qd), N.ptr(dd), n_seq, L,
                     ctypes.byref(w), N.ptr(dqkv), N.stream_handle(device))
    assert status == UNSUPPORTED
    assert bool(torch.isnan(dqkv).all())


# -- 6. nrms_qkv_project_backward ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def _project_case(rows):
    w = _host_weights()
    x, dqkv = K.project_inputs(rows)
    r64 = K.project_backward_ref(x.double(), dqkv.double(), w["w_q"].double(), w["w_k"].double(), w["w_v"].double())
    r32 = K.project_backward_ref(x, dqkv, w["w_q"], w["w_k"], w["w_v"])
    return x, dqkv, r64, r32


@pytest.mark.parametrize("rows", K.PROJECT_ROWS)
def test_qkv_project_backward(device, gemm_mode, rows):
    N = _N()
    lib = N.load()
    x, dqkv, r64, r32 = _project_case(rows)
    w, keep = _weights(device)
    st = N.stream_handle(device)
    g0w, g0b = K.g0_pattern(3 * K.D, K.D), K.g0_pattern(3 * K.D)
    xd, dd = x.to(device), dqkv.to(device)
    xoff = torch.zeros(rows * K.D + 4, device=device)   # the same x one float into its buffer
    xoff[1:rows * K.D + 1] = xd.reshape(-1)
    assert xoff[1:].data_ptr() % 16 == 4
    nbytes = lib.nrms_qkv_project_backward_workspace_size(K.D)
    assert nbytes > 0
    ws, tail = _guarded(nbytes, device)

    def run(xin, with_dx, ws_bytes=nbytes):
        dx = _nan(device, rows, K.D) if with_dx else None
        dw, db = g0w.to(device), g0b.to(device)
        status = _status("nrms_qkv_project_backward", N.ptr(xin), rows, ctypes.byref(w), N.ptr(dd), N.ptr(dx),
                         N.ptr(dw), N.ptr(db), N.ptr(ws), ws_bytes, st)
        return status, dx, dw, db

    status, dx, dw, db = run(xd, True, nbytes - 1)   # rejected in capi.hip before any launch
    assert status == WORKSPACE
    assert bool(torch.isnan(dx).all()) and _same_bits(dw, g0w) and _same_bits(db, g0b)

    case = f"{gemm_mode}-rows{rows}"
    status, dx, dw, db = run(xd, True)
    assert status == OK
    ok = [K.report("qkv_project_backward", case, "dx", dx, r64[0], r32[0]),
          K.report("qkv_project_backward", case, "d_w_qkv", dw, g0w.double() + r64[1], g0w + r32[1]),
          K.report("qkv_project_backward", case, "d_b_qkv", db, g0b.double() + r64[2], g0b + r32[2])]
    status, none, dw2, db2 = run(xd, False)          # dx == NULL: the same gradients, bitwise
    assert status == OK and none is None
    same = _same_bits(dw2, dw) and _same_bits(db2, db)
    status, none, dw3, db3 = run(xoff[1:], False)    # misaligned x: the f32 kernel under the split modes
    assert status == OK
    ok += [K.report("qkv_project_backward", case + "-xoff", "d_w_qkv", dw3, g0w.double() + r64[1], g0w + r32[1]),
           K.report("qkv_project_backward", case + "-xoff", "d_b_qkv", db3, g0b.double() + r64[2], g0b + r32[2])]
    assert all(ok), case
    assert same
    assert torch.equal(ws[nbytes:], tail)
    assert _same_bits(xd, x) and _same_bits(dd, dqkv)


# -- 7. nrms_embedding_backward(_ws) --------------------------------------------------

def _embed_ws(N, ids, dx, V, Dd, table, device):
    lib = N.load()
    nb = lib.nrms_embedding_backward_workspace_size(ids.numel(), V)
    ws, tail = _guarded(nb, device)
    N.call("nrms_embedding_backward_ws", N.ptr(ids), ids.numel(), N.ptr(dx), V, Dd, 0, N.ptr(table), N.ptr(ws), nb,
           N.stream_handle(device))
    assert torch.equal(ws[nb:], tail)
    return table


@pytest.mark.parametrize("Dd", K.EMBED_D)
@pytest.mark.parametrize("V", K.EMBED_V)
def test_embedding_backward(device, V, Dd):
    N = _N()
    ids = K.embed_ids(V)
    n_tok = ids.numel()
    dx = K.randn(K.gen(710 + Dd), n_tok, Dd)
    g0 = K.g0_pattern(V, Dd)
    r32, r64 = K.embed_ref(ids, dx, V, g0), K.embed_ref(ids, dx, V, g0.double())
    idd, dxd = ids.to(device), dx.to(device)
    got = _embed_ws(N, idd, dxd, V, Dd, g0.to(device), device).cpu()
    again = _embed_ws(N, idd, dxd, V, Dd, g0.to(device), device).cpu()
    long_ = torch.tensor([i for i, c in K.EMBED_RUNS.items() if c > K.EMB_LONG])
    short = torch.ones(V, dtype=torch.bool)
    short[long_] = False
    case = f"V{V}D{Dd}"
    ok = [K.report("embedding_backward_ws", case, "long_rows", got[long_], r64[long_], r32[long_])]
    # runs of at most 256 tokens: the CPU index_add in token order, bitwise; row 0 and unused rows: g0
    assert _same_bits(got[short], r32[short])
    assert _same_bits(got[0], g0[0]) and _same_bits(got[11:V - 1], g0[11:V - 1])
    assert _same_bits(got, again)
    atom = g0.to(device)
    N.call("nrms_embedding_backward", N.ptr(idd), n_tok, N.ptr(dxd), V, Dd, 0, N.ptr(atom), N.stream_handle(device))
    atom = atom.cpu()
    ok.append(K.report("embedding_backward", case, "dtable", atom, r64, r32))
    assert all(ok), case
    assert _same_bits(atom[0], g0[0]) and _same_bits(atom[11:V - 1], g0[11:V - 1])
    assert _same_bits(idd, ids) and _same_bits(dxd, dx)


def test_embedding_backward_one_token_and_all_padding(device):
    N = _N()
    V, Dd = 64, 300
    g0 = K.g0_pattern(V, Dd)
    dx = K.randn(K.gen(720), 40, Dd)
    dxd = dx.to(device)
    one = torch.tensor([V - 1])
    want = g0.clone()
    want[V - 1] += dx[0]
    pad = torch.zeros(40, dtype=torch.int64)
    for form in ("ws", "atomic"):
        for ids, ref in ((one, want), (pad, g0)):
            table, idd = g0.to(device), ids.to(device)
            if form == "ws":
                _embed_ws(N, idd, dxd, V, Dd, table, device)
            else:
                N.call("nrms_embedding_backward", N.ptr(idd), ids.numel(), N.ptr(dxd), V, Dd, 0,
                       N.ptr(table), N.stream_handle(device))
            assert _same_bits(table, ref), (form, ids.numel())


# -- 8. nrms_adam_step(_multi) ---------------------------------------------------------

def _hyper():
    return [ctypes.c_float(h) for h in K.ADAM_HYPER]


def _adam_refs(states, step):
    """Concatenated (delta p, exp_avg, exp_avg_sq): fp64 and torch's fp32 Adam."""
    r64 = [K.adam_ref64(*s, step) for s in states]
    t32 = K.adam_torch(*zip(*states), step, torch.float32) if states else ([], [], [])
    cat = lambda ts: torch.cat([t.double().reshape(-1) for t in ts]) if ts else torch.zeros(0, dtype=torch.float64)
    return [cat([r[i] for r in r64]) for i in range(3)], [cat(t32[i]) for i in range(3)]


@pytest.mark.parametrize("step", K.ADAM_STEPS)
@pytest.mark.parametrize("n", K.ADAM_N)
def test_adam_step(device, n, step):
    N = _N()
    p, g, m, v = K.adam_state(n, 800 + n)
    r64, r32 = _adam_refs([(p, g, m, v)], step)
    pd, gd, md, vd = (t.to(device) for t in (p, g, m, v))
    N.call("nrms_adam_step", N.ptr(pd), N.ptr(gd), N.ptr(md), N.ptr(vd), n, *_hyper(), step, N.stream_handle(device))
    dp = pd.cpu().double() - p.double()
    case = f"n{n}-step{step}"
    ok = [K.report("adam_step", case, name, o, a, b)
          for name, o, a, b in zip(("delta_p", "exp_avg", "exp_avg_sq"), (dp, md.cpu(), vd.cpu()), r64, r32)]
    assert all(ok), case
    still = (g == 0) & (m == 0) & (v == 0)   # zero gradient on zero state: the parameter keeps its bits
    assert _same_bits(pd.cpu()[still], p[still])
    assert _same_bits(gd, g)


@pytest.mark.parametrize("with_empty", [False, True])
@pytest.mark.parametrize("count", K.ADAM_COUNTS)
def test_adam_step_multi(device, count, with_empty):
    N = _N()
    step = 2
    st = N.stream_handle(device)
    sizes = K.adam_multi_sizes(count, with_empty)
    states = [K.adam_state(n, 900 + i) if n else None for i, n in enumerate(sizes)]
    live = [s for s in states if s is not None]
    r64, r32 = _adam_refs(live, step)
    multi = [[t.to(device) for t in s] if s else None for s in states]
    single = [[t.to(device) for t in s] for s in live]
    arr = (AdamTensor * len(sizes))()
    for d, s, n in zip(arr, multi, sizes):
        if s:   # an empty descriptor keeps its null pointers
            d.param, d.grad, d.exp_avg, d.exp_avg_sq = (t.data_ptr() for t in s)
        d.numel = n
    N.call("nrms_adam_step_multi", ctypes.cast(arr, ctypes.c_void_p), len(sizes), *_hyper(), step, st)
    for s in single:
        N.call("nrms_adam_step", *[N.ptr(t) for t in s], s[0].numel(), *_hyper(), step, st)
    got = [s for s in multi if s]
    for a, b in zip(got, single):   # the two forms: bitwise the same
        assert all(_same_bits(x, y) for x, y in zip(a, b))
    cat = lambda ts: torch.cat([t.cpu().double().reshape(-1) for t in ts])
    outs = (cat([s[0] for s in got]) - cat([s[0] for s in live]), cat([s[2] for s in got]), cat([s[3] for s in got]))
    case = f"tensors{count}{'-empty' if with_empty else ''}"
    ok = [K.report("adam_step_multi", case, name, o, a, b)
          for name, o, a, b in zip(("delta_p", "exp_avg", "exp_avg_sq"), outs, r64, r32)]
    assert all(ok), case
    for a, s in zip(got, live):
        still = (s[1] == 0) & (s[2] == 0) & (s[3] == 0)
        assert _same_bits(a[0].cpu()[still], s[0][still])


def test_adam_empty_calls(device):
    N = _N()
    st = N.stream_handle(device)
    assert _status("nrms_adam_step", None, None, None, None, 0, *_hyper(), 1, st) == OK
    assert _status("nrms_adam_step_multi", None, 0, *_hyper(), 1, st) == OK
    arr = (AdamTensor * 2)()   # only empty descriptors: nothing to launch
    assert _status("nrms_adam_step_multi", ctypes.cast(arr, ctypes.c_void_p), 2, *_hyper(), 1, st) == OK
