"""GPU: the sampler spread over many workgroups (iq_sample_permutations_ws, csrc/iq_sample.hip) against NumPy's legacy generator and
against the one-workgroup entry point it must equal bit for bit: permutations, the 625 state words handed back, and what a
poisoned state does.  The size of the workspace never changes a result: the one-workgroup kernel runs last and draws the rest."""
import ctypes

import numpy as np
import pytest
import torch

from interpret_quality_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

STARTS = {"fresh": 624, "zero": 0, "last": 623, "mid": 311}     # position word of the state a draw starts from


def _state(seed, pos):
    """A legacy generator state at position ``pos`` of its 624-word block (624: a fresh seed's, nothing generated yet)."""
    np.random.seed(seed)
    st = np.random.get_state()
    return ("MT19937", st[1], pos, 0, 0.0)


def _numpy(state, s, r):
    np.random.set_state(state)
    orders = np.stack([np.random.permutation(np.arange(r)) for _ in range(s)])
    after = np.random.get_state()
    return orders, np.concatenate([after[1], [after[2]]]).astype(np.uint32)


def _old_entry(state, s, r):
    """iq_sample_permutations itself (hip_ops goes through the workspace entry) -> (orders, 625 state words)."""
    lib = _lib.load()
    words = hip_ops.mt_state_to_device(DEV, state)
    orders = torch.empty((s, r), dtype=torch.int32, device=DEV)
    _lib.check(lib.iq_sample_permutations(hip_ops._p(words), hip_ops._p(orders), s, r, hip_ops._stream()), "iq_sample_permutations")
    return orders.cpu().numpy(), words.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("start", sorted(STARTS))
@pytest.mark.parametrize("s", [1, 7, 1000])
@pytest.mark.parametrize("r", [2, 3, 32, 64])
def test_the_wide_path_equals_numpy_and_the_one_workgroup_kernel(r, s, start):
    state = _state(100 * r + s, STARTS[start])
    want, want_words = _numpy(state, s, r)
    words = hip_ops.mt_state_to_device(DEV, state)
    got = hip_ops.sample_permutations(words, s, r).cpu().numpy()
    got_words = words.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)
    assert np.array_equal(got_words, want_words)
    old, old_words = _old_entry(state, s, r)
    assert np.array_equal(got, old) and np.array_equal(got_words, old_words)


@pytest.mark.parametrize("start", sorted(STARTS))
@pytest.mark.parametrize("s,r", [(1000, 32), (20000, 2), (9000, 3), (5000, 64), (100, 64)])
def test_the_wide_kernels_draw_the_whole_call_at_the_size_the_query_gives(s, r, start):
    """A call that one batch of the one-workgroup kernel covers stays on it, so the small cases above never reach the wide kernels;
    these do, from every start position, with up to 4096 permutations in a segment (R = 2: a word each).  Nothing else shows who
    drew: the first word of the workspace counts the permutations the wide kernels wrote (csrc/iq_sample.hip, ctl[0]); what is
    missing from S is left to the one-workgroup kernel.  At the queried size that is nothing."""
    state = _state(s + r, STARTS[start])
    want, want_words = _numpy(state, s, r)
    words = hip_ops.mt_state_to_device(DEV, state)
    got = hip_ops.sample_permutations(words, s, r)
    assert int(hip_ops._sample_ws[DEV][:4].view(torch.int32).item()) == s
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(words.cpu().numpy().view(np.uint32), want_words)
    old, old_words = _old_entry(state, s, r)
    assert np.array_equal(got.cpu().numpy(), old) and np.array_equal(words.cpu().numpy().view(np.uint32), old_words)


def test_half_a_workspace_leaves_half_of_the_call_to_the_finishing_kernel():
    words = hip_ops.mt_state_to_device(DEV, _state(1, 624))
    hip_ops.sample_permutations(words, 1000, 32, workspace_bytes=300000)      # 30 blocks: about 444 permutations of 40.7 words
    assert 300 < int(hip_ops._sample_ws[DEV][:4].view(torch.int32).item()) < 600


def test_several_calls_equal_one_call():
    state = _state(4, 624)
    want, want_words = _numpy(state, 700, 32)
    words = hip_ops.mt_state_to_device(DEV, state)
    parts = [hip_ops.sample_permutations(words, n, 32) for n in (1, 99, 250, 350)]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), want)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want_words)


@pytest.mark.parametrize("nbytes", [0, 8, 20048, 40000, 300000])
def test_a_workspace_that_is_far_too_small_gives_the_same_result(nbytes):
    """20048 bytes hold two 624-word blocks, about 20 of the 1000 permutations: the finishing kernel draws the other 980.  Below
    that the wide kernels do not run at all; 300 000 bytes hold under half of what the call asks for."""
    lib = _lib.load()
    assert lib.iq_sample_workspace_bytes(1000, 32) > 2 * 300000
    state = _state(8, 100)
    want, want_words = _numpy(state, 1000, 32)
    words = hip_ops.mt_state_to_device(DEV, state)
    got = hip_ops.sample_permutations(words, 1000, 32, workspace_bytes=nbytes)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want_words)


def test_a_malformed_state_gives_rows_of_minus_one_and_the_marked_position():
    words = hip_ops.mt_state_to_device(DEV, _state(5, 624))
    words[624] = 1000
    key = words[:624].cpu().numpy().copy()
    orders = hip_ops.sample_permutations(words, 7, 32)
    assert bool((orders == -1).all())
    after = words.cpu().numpy().view(np.uint32)
    assert int(after[624]) == 0x7fffffff and np.array_equal(after[:624].view(np.int32), key)
    with pytest.raises(_lib.IqError, match="did not complete"):
        hip_ops.mt_state_to_host(words, set_global=False)
    again = hip_ops.sample_permutations(words, 3, 8)         # a poisoned state stays poisoned
    assert bool((again == -1).all()) and int(words.cpu().numpy().view(np.uint32)[624]) == 0x7fffffff


@pytest.mark.parametrize("nbytes", [None, 40000])
@pytest.mark.parametrize("position", [625, 1000, 0x7fffffff, 0xffffffff])
def test_a_malformed_state_on_the_wide_route(position, nbytes):
    """The same at a shape that takes the wide kernels (1000 permutations of 32 regions; at the queried size and with a workspace of
    three blocks): none of them may draw, and the finishing kernel must not take over the count and the offset that the call
    before - a complete one, on the same workspace - left in the control words."""
    assert _lib.load().iq_sample_workspace_bytes(1000, 32) > 40000
    good = hip_ops.mt_state_to_device(DEV, _state(6, 311))
    hip_ops.sample_permutations(good, 1000, 32, workspace_bytes=nbytes)
    assert int(hip_ops._sample_ws[DEV][:4].view(torch.int32).item()) in ((1000,) if nbytes is None else range(20, 60))   # what that call left
    words = hip_ops.mt_state_to_device(DEV, _state(5, 624))
    key = words[:624].cpu().numpy().copy()
    words[624] = int(np.uint32(position).view(np.int32))
    for _ in range(2):                                       # malformed, then already poisoned
        orders = hip_ops.sample_permutations(words, 1000, 32, workspace_bytes=nbytes)
        assert bool((orders == -1).all())
        after = words.cpu().numpy().view(np.uint32)
        assert int(after[624]) == 0x7fffffff and np.array_equal(after[:624].view(np.int32), key)
    with pytest.raises(_lib.IqError, match="did not complete"):
        hip_ops.mt_state_to_host(words, set_global=False)
    old = hip_ops.mt_state_to_device(DEV, _state(5, 624))    # the one-workgroup entry on the same state: the same rows and state
    old[624] = int(np.uint32(position).view(np.int32))
    rows = torch.zeros((1000, 32), dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().iq_sample_permutations(hip_ops._p(old), hip_ops._p(rows), 1000, 32, hip_ops._stream()), "iq_sample_permutations")
    assert torch.equal(rows, orders) and torch.equal(old, words)


def test_the_size_query_answers_zero_where_nothing_is_drawn():
    lib = _lib.load()
    assert lib.iq_sample_workspace_bytes(0, 32) == 0 and lib.iq_sample_workspace_bytes(10, 1) == 0
    assert lib.iq_sample_workspace_bytes(1000, 32) % 8 == 0
    assert isinstance(ctypes.c_size_t(lib.iq_sample_workspace_bytes(1000, 64)).value, int)
