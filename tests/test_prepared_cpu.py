"""CPU-only checks of the prepared forward's host arithmetic
(nrms_forward_state_size, nrms_forward_prepared_workspace_size) and of the
argument checks that return before anything touches the device."""
import ctypes

from newsrecommendationsystem_amd import _native as N


def test_abi_version_unchanged():
    assert N.load().nrms_abi_version() == 9 == N.ABI_VERSION


def test_size_functions_reject_invalid_shapes():
    lib = N.load()
    assert lib.nrms_forward_state_size(-1, 300, 1) == 0
    assert lib.nrms_forward_state_size(1000, 0, 1) == 0
    assert lib.nrms_forward_state_size(1000, -300, 0) == 0
    for bad in ((-1, 5, 50, 20, 300), (4, -1, 50, 20, 300), (4, 5, 0, 20, 300), (4, 5, 50, 0, 300),
                (4, 5, 50, 20, 0)):
        assert lib.nrms_forward_prepared_workspace_size(*bad) == 0, bad
        assert lib.nrms_forward_prepared_folded_workspace_size(*bad) == 0, bad


def test_state_size_grows_with_vocabulary_only_with_the_table():
    lib = N.load()
    ld = lib.nrms_qkv_row_stride(300)
    packs = lib.nrms_forward_state_size(1000, 300, 0)
    assert packs > 0
    assert lib.nrms_forward_state_size(70976, 300, 0) == packs == lib.nrms_forward_state_size(0, 300, 0)
    small, large = lib.nrms_forward_state_size(1000, 300, 1), lib.nrms_forward_state_size(70976, 300, 1)
    assert small >= packs + 1000 * ld * 4 and large >= packs + 70976 * ld * 4
    assert large - small >= (70976 - 1000) * ld * 4 - 256   # (256-B alignment of the table)


def test_prepared_workspace_has_no_vocabulary_term():
    """The folded table lives in the state: the step's workspace is smaller
    than nrms_forward's by the table, whatever V."""
    lib = N.load()
    B, C, Nc, L, D = 64, 5, 50, 20, 300
    ld = lib.nrms_qkv_row_stride(D)
    folded = lib.nrms_forward_prepared_folded_workspace_size(B, C, Nc, L, D)
    every = lib.nrms_forward_prepared_workspace_size(B, C, Nc, L, D)
    assert 0 < folded < every
    assert every - folded >= B * (C + Nc) * L * ld * 4          # the direct mode's per-token rows
    for V in (1000, 70976):
        full = lib.nrms_forward_workspace_size(B, C, Nc, L, V, D, N.NRMS_PROJ_FOLDED)
        assert full - folded >= V * ld * 4
        assert lib.nrms_forward_workspace_size(B, C, Nc, L, V, D, N.NRMS_PROJ_DIRECT) == every


def test_prepare_and_prepared_reject_bad_arguments_without_launch():
    lib = N.load()
    dummy = ctypes.c_void_p(256)
    w = N.EncoderWeights(*([dummy.value] * 9), 300, 15, 200)
    st = N.ForwardState()
    null_w = N.EncoderWeights()
    # null state struct, null weights, no buffer, short buffer: nothing is enqueued
    assert lib.nrms_forward_prepare(dummy, 1000, w, w, 1, dummy, 1 << 30, None, None) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_forward_prepare(dummy, 1000, null_w, w, 1, dummy, 1 << 30, st, None) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_forward_prepare(dummy, 0, w, w, 1, dummy, 1 << 30, st, None) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_forward_prepare(dummy, 1000, w, w, 1, None, 1 << 30, st, None) == N.NRMS_ERR_WORKSPACE
    need = lib.nrms_forward_state_size(1000, 300, 1)
    assert lib.nrms_forward_prepare(dummy, 1000, w, w, 1, dummy, need - 1, st, None) == N.NRMS_ERR_WORKSPACE
    assert st.buffer is None and st.flags == 0
    # a step without a state, or with one that was never prepared
    args = (dummy, dummy, 4, 5, 50, 20, dummy, 1000, w, w, N.NRMS_PROJ_FOLDED, dummy, dummy, 1 << 30, None)
    assert lib.nrms_forward_prepared(*args, None) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_forward_prepared(*args, st) == N.NRMS_ERR_INVALID_ARG
    assert lib.nrms_forward_prepared_timed(*args, st, None, 3) == N.NRMS_ERR_INVALID_ARG
