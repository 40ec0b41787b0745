"""The forward over a prepared weight state (nrms_forward_prepare /
nrms_forward_prepared, include/nrms_hip.h) against nrms_forward: bitwise the
same logits at every shape, projection mode, arithmetic and dedupe /
compaction setting; the state is invalidated by every parameter it reads, is
only read by a step (shared between forwards on two streams), stays valid
inside a captured graph across an in-place re-prepare, and the misuse cases
return their error codes without touching the logits."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import weights as W

pytestmark = pytest.mark.gpu

V, C, NC, L, D = 3000, 5, 50, 20, 300
SENTINEL = -12345.0


def _module(seed, device, **knobs):
    from newsrecommendationsystem_amd import NRMS, NRMSConfig

    class Cfg(NRMSConfig):
        num_words = V
    for k, v in knobs.items():
        setattr(Cfg, k, v)
    m = NRMS(Cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.nrms_state(seed, V).items()})
    return m.to(device).eval()


@pytest.fixture(scope="module")
def model(device):
    return _module(61, device)


def _batch(seed, B, device, zero_frac=0.3):
    """Left-padded histories (oracle.weights.impressions) with about 30 % of
    the clicked titles zeroed on top, as test_forward_graph_replay_recomputes_bitwise."""
    cand, clk, _ = W.impressions(seed, 5, B, V)
    clk = clk.copy()
    if zero_frac:
        clk[np.random.default_rng(seed).random(clk.shape[:2]) < zero_frac] = 0
    return torch.from_numpy(cand).to(device), torch.from_numpy(clk).to(device)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _reference(m, cand, clk, mode):
    """nrms_forward itself: everything recomputed in the call."""
    from newsrecommendationsystem_amd import _native as N
    lib = N.load()
    B = cand.shape[0]
    tab = m.news_encoder.table()
    wn, kn = m.news_encoder.weights()
    wu, ku = m.user_encoder.weights()
    nb = lib.nrms_forward_workspace_size(B, C, NC, L, V, D, mode)
    ws = torch.empty(nb, dtype=torch.uint8, device=tab.device)
    out = torch.full((B, C), SENTINEL, device=tab.device)
    N.call("nrms_forward", N.ptr(cand), N.ptr(clk), B, C, NC, L, N.ptr(tab), V, ctypes.byref(wn), ctypes.byref(wu),
           mode, N.ptr(out), N.ptr(ws), nb, N.stream_handle(tab.device))
    torch.cuda.synchronize()
    return out


def _prepared_call(m, cand, clk, mode, state, ws=None, ws_bytes=None):
    """nrms_forward_prepared over `state` (a ctypes reference or None); returns
    (status, logits pre-filled with the sentinel)."""
    from newsrecommendationsystem_amd import _native as N
    lib = N.load()
    B = cand.shape[0]
    tab = m.news_encoder.table()
    wn, kn = m.news_encoder.weights()
    wu, ku = m.user_encoder.weights()
    if ws is None:
        ws = torch.empty(lib.nrms_forward_prepared_workspace_size(B, C, NC, L, D), dtype=torch.uint8,
                         device=tab.device)
    out = torch.full((B, C), SENTINEL, device=tab.device)
    st = lib.nrms_forward_prepared(N.ptr(cand), N.ptr(clk), B, C, NC, L, N.ptr(tab), V, ctypes.byref(wn),
                                   ctypes.byref(wu), mode, N.ptr(out), N.ptr(ws),
                                   ws.numel() if ws_bytes is None else ws_bytes, N.stream_handle(tab.device), state)
    torch.cuda.synchronize()
    return st, out


def _folded(mode, B):
    from newsrecommendationsystem_amd import _native as N
    return mode == N.NRMS_PROJ_FOLDED or (mode == N.NRMS_PROJ_AUTO and B * (C + NC) * L > V)


class _switches:
    """Title dedupe / token compaction for the enclosed calls."""

    def __init__(self, dedupe, compact):
        self.want = (dedupe, compact)

    def __enter__(self):
        from newsrecommendationsystem_amd import _native as N
        lib = N.load()
        self.prev = (lib.nrms_set_title_dedupe(self.want[0]), lib.nrms_set_token_compaction(self.want[1]))

    def __exit__(self, *exc):
        from newsrecommendationsystem_amd import _native as N
        lib = N.load()
        lib.nrms_set_title_dedupe(self.prev[0])
        lib.nrms_set_token_compaction(self.prev[1])
        return False


# B = 70: 3,850 titles, the last classification block partial; B = 1: one
# partial block, fewer groups than CUs (and under auto: 1,100 tokens < V, the
# direct mode); B = 256: 14,080 = 55 x 256 titles, whole blocks
@pytest.mark.parametrize("B", [70, 1, 256])
@pytest.mark.parametrize("proj", ["folded", "direct", "auto"])
def test_prepared_bitwise_equals_forward(model, device, gemm_mode, proj, B):
    from newsrecommendationsystem_amd import _native as N
    mode = {"folded": N.NRMS_PROJ_FOLDED, "direct": N.NRMS_PROJ_DIRECT, "auto": N.NRMS_PROJ_AUTO}[proj]
    cand, clk = _batch(100 + B, B, device)
    with torch.no_grad():
        state = model.forward_state(_folded(mode, B))
        assert state.st.gemm_arith == N.load().nrms_get_gemm_arith()
        assert bool(state.st.flags & N.NRMS_STATE_QKV_PACKS) == (gemm_mode != "f32")
        for dedupe in (1, 0):
            for compact in (1, 0):
                with _switches(dedupe, compact):
                    ref = _reference(model, cand, clk, mode)
                    st, got = _prepared_call(model, cand, clk, mode, state.ref())
                assert st == N.NRMS_OK
                assert torch.isfinite(ref).all()
                assert _same(got, ref), (dedupe, compact)


@pytest.mark.parametrize("case", ["no_padding_title", "all_padding_user", "bad_ids"])
def test_prepared_bitwise_edge_batches(model, device, gemm_mode, case):
    """rep = none (no all-padding title in the batch); one user whose 50
    clicked titles are all padding; out-of-range and negative ids (what
    hip_check_ids = False lets through): the ids take the NaN-row path, the
    same NaN pattern as nrms_forward."""
    from newsrecommendationsystem_amd import _native as N
    B = 70
    cand, clk = _batch(300, B, device)
    if case == "no_padding_title":
        t = torch.from_numpy(W.titles(301, 7, B * NC, V)).to(device).view(B, NC, L)
        clk = torch.where((clk == 0).all(-1, keepdim=True), t, clk)
        assert not (clk == 0).all(-1).any() and not (cand == 0).all(-1).any()
    elif case == "all_padding_user":
        clk[3] = 0
    else:
        cand[2, 1, 0], cand[5, 0, 3], clk[7, 49, 1], clk[9, 48, 0] = V, -1, V + 12345, -(1 << 40)
    modes = (N.NRMS_PROJ_FOLDED, N.NRMS_PROJ_DIRECT)
    with torch.no_grad():
        for mode in modes:
            ref = _reference(model, cand, clk, mode)
            st, got = _prepared_call(model, cand, clk, mode, model.forward_state(_folded(mode, B)).ref())
            assert st == N.NRMS_OK and _same(got, ref), mode
            if case == "bad_ids":
                # a bad candidate id: that logit; a bad clicked id: the user's row
                nan = torch.isnan(ref)
                assert nan[7].all() and nan[9].all() and nan[2, 1] and nan[5, 0]
                assert int(nan.sum()) == 2 * C + 2
            else:
                assert torch.isfinite(ref).all()


def _check_fresh(m, fwds, batch, old):
    """TimedForward.run and forward_ids equal a fresh nrms_forward and differ from `old`."""
    from newsrecommendationsystem_amd import _native as N
    cand, clk = batch
    ref = _reference(m, cand, clk, N.NRMS_PROJ_FOLDED)
    assert not _same(ref, old)
    y = fwds.run(cand, clk).clone()
    z = m.forward_ids(cand, clk, proj_mode=N.NRMS_PROJ_FOLDED)
    torch.cuda.synchronize()
    assert _same(y, ref) and _same(z, ref)
    return ref


def test_state_goes_stale_with_every_parameter_change(device):
    """p.add_() on W_Q and on the news W_add, load_state_dict, one HipAdam
    step and nrms_set_gemm_arith: each time the prepared paths give the new
    parameters' (arithmetic's) logits, through the same state buffer."""
    from newsrecommendationsystem_amd import _native as N
    from newsrecommendationsystem_amd import train_hip as H
    from newsrecommendationsystem_amd.pipeline import TimedForward
    m = _module(62, device)
    B = 70
    batch = _batch(400, B, device)
    fwd = TimedForward(m, B, C, NC, L)
    assert fwd.prepared
    buf = fwd.state.buf.data_ptr()
    with torch.no_grad():
        old = _check_fresh(m, fwd, batch, torch.zeros(B, C, device=device))
        m.news_encoder.multihead_self_attention.W_Q.weight.add_(0.01)
        old = _check_fresh(m, fwd, batch, old)
        m.news_encoder.additive_attention.linear.weight.add_(0.01)
        old = _check_fresh(m, fwd, batch, old)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.nrms_state(63, V).items()})
        old = _check_fresh(m, fwd, batch, old)
    params = [p for p in m.parameters()]
    for p in params:
        p.grad = torch.full_like(p, 0.5)
    H.HipAdam(params, lr=1e-2).step()
    for p in params:
        p.grad = None
    with torch.no_grad():
        old = _check_fresh(m, fwd, batch, old)
        assert fwd.state.buf.data_ptr() == buf          # prepared again in place
        with N.gemm_arith(N.NRMS_GEMM_SPLIT_BF16X6):
            _check_fresh(m, fwd, batch, old)
            assert fwd.state.buf.data_ptr() != buf      # (an entry of its own per arithmetic)
        assert _same(fwd.run(*batch), old) and fwd.state.buf.data_ptr() == buf


def test_graph_replays_prepared_state_and_survives_refresh(device):
    """The prepared step captured in a HIP graph: replays give the eager
    logits of whatever the id buffers hold; after an in-place weight update
    and refresh() the same capture gives the new weights' eager logits."""
    from newsrecommendationsystem_amd import _native as N
    from newsrecommendationsystem_amd.pipeline import TimedForward
    m = _module(64, device)
    B = 64
    batches = [_batch(s, B, device) for s in (500, 501)]
    fwd = TimedForward(m, B, C, NC, L)
    assert fwd.prepared
    c, k = batches[0][0].clone(), batches[0][1].clone()
    with torch.no_grad():
        eager = [_reference(m, *b, N.NRMS_PROJ_FOLDED) for b in batches]
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            fwd.run(c, k)
        torch.cuda.current_stream(device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fwd.run(c, k)

        def replay(i):
            c.copy_(batches[i][0])
            k.copy_(batches[i][1])
            fwd.logits.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            return fwd.logits

        for i in (0, 1, 0):
            assert _same(replay(i), eager[i]), i
        m.user_encoder.multihead_self_attention.W_K.weight.mul_(1.5)
        m.news_encoder.word_embedding.weight.add_(0.05)
        fwd.refresh()
        torch.cuda.synchronize()
        fresh = [_reference(m, *b, N.NRMS_PROJ_FOLDED) for b in batches]
        for i in (1, 0):
            assert not _same(fresh[i], eager[i])
            assert _same(replay(i), fresh[i]), i


def test_two_forwards_share_one_state_on_two_streams(device):
    """Two TimedForward (B = 64 and B = 70) over one model, so one state, on
    two streams with their steps interleaved: each equals its solo result.
    Nothing a step writes lives in the state."""
    from newsrecommendationsystem_amd.pipeline import TimedForward
    m = _module(65, device)
    fa, fb = TimedForward(m, 64, C, NC, L), TimedForward(m, 70, C, NC, L)
    assert fa.state is fb.state
    ba, bb = _batch(600, 64, device), _batch(601, 70, device)
    with torch.no_grad():
        solo_a, solo_b = fa.run(*ba).clone(), fb.run(*bb).clone()
        torch.cuda.synchronize()
        table = fa.state.buf.clone()
        sa, sb = torch.cuda.Stream(device), torch.cuda.Stream(device)
        for _ in range(4):
            fa.logits.fill_(float("nan"))
            fb.logits.fill_(float("nan"))
            torch.cuda.synchronize()
            with torch.cuda.stream(sa):
                fa.run(*ba)
            with torch.cuda.stream(sb):
                fb.run(*bb)
            with torch.cuda.stream(sa):
                fa.run(*ba)
            torch.cuda.synchronize()
            assert _same(fa.logits, solo_a) and _same(fb.logits, solo_b)
        assert torch.equal(fa.state.buf, table)


def test_misuse_returns_error_codes_and_leaves_logits(model, device):
    from newsrecommendationsystem_amd import _native as N
    lib = N.load()
    B = 8
    cand, clk = _batch(700, B, device)
    FOLDED = N.NRMS_PROJ_FOLDED

    def untouched(out):
        return bool((out == SENTINEL).all())

    with torch.no_grad():
        good = model.forward_state(True)
        st, out = _prepared_call(model, cand, clk, FOLDED, good.ref())
        assert st == N.NRMS_OK and not untouched(out)
        # a null state
        st, out = _prepared_call(model, cand, clk, FOLDED, None)
        assert st == N.NRMS_ERR_INVALID_ARG and untouched(out)
        # a state for another V
        other = N.ForwardState.from_buffer_copy(good.st)
        other.V = V + 1
        st, out = _prepared_call(model, cand, clk, FOLDED, ctypes.byref(other))
        assert st == N.NRMS_ERR_INVALID_ARG and untouched(out)
        # a state prepared under another arithmetic
        with N.gemm_arith(N.NRMS_GEMM_F32 if lib.nrms_get_gemm_arith() != N.NRMS_GEMM_F32
                          else N.NRMS_GEMM_SPLIT_BF16X6):
            st, out = _prepared_call(model, cand, clk, FOLDED, good.ref())
        assert st == N.NRMS_ERR_INVALID_ARG and untouched(out)
        # a state without a folded table on a folded call (fine on a direct one)
        packs = model.forward_state(False)
        st, out = _prepared_call(model, cand, clk, FOLDED, packs.ref())
        assert st == N.NRMS_ERR_INVALID_ARG and untouched(out)
        st, out = _prepared_call(model, cand, clk, N.NRMS_PROJ_DIRECT, packs.ref())
        assert st == N.NRMS_OK and _same(out, _reference(model, cand, clk, N.NRMS_PROJ_DIRECT))
        # a short state buffer: at the prepare, and a state that claims fewer bytes
        tab = model.news_encoder.table()
        wn, kn = model.news_encoder.weights()
        wu, ku = model.user_encoder.weights()
        need = lib.nrms_forward_state_size(V, D, 1)
        buf = torch.empty(need, dtype=torch.uint8, device=device)
        fresh = N.ForwardState()
        assert lib.nrms_forward_prepare(N.ptr(tab), V, ctypes.byref(wn), ctypes.byref(wu), 1, N.ptr(buf), need - 256,
                                        ctypes.byref(fresh), N.stream_handle(device)) == N.NRMS_ERR_WORKSPACE
        st, out = _prepared_call(model, cand, clk, FOLDED, ctypes.byref(fresh))
        assert st == N.NRMS_ERR_INVALID_ARG and untouched(out)      # (never prepared)
        short = N.ForwardState.from_buffer_copy(good.st)
        short.bytes = need - 256
        st, out = _prepared_call(model, cand, clk, FOLDED, ctypes.byref(short))
        assert st == N.NRMS_ERR_WORKSPACE and untouched(out)
        # a short workspace
        nb = lib.nrms_forward_prepared_folded_workspace_size(B, C, NC, L, D)
        ws = torch.empty(nb, dtype=torch.uint8, device=device)
        st, out = _prepared_call(model, cand, clk, FOLDED, good.ref(), ws=ws, ws_bytes=nb - 256)
        assert st == N.NRMS_ERR_WORKSPACE and untouched(out)
        st, out = _prepared_call(model, cand, clk, FOLDED, good.ref(), ws=ws)
        assert st == N.NRMS_OK and _same(out, _reference(model, cand, clk, FOLDED))
