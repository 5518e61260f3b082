"""GPU: the device sampler for wide games (iq_sample_permutations_wide, csrc/iq_sample.hip) against NumPy's legacy generator -
permutations of up to 1024 regions and all 625 state words handed back, exact equality throughout - and the properties the narrow
sampler has (tests/test_sampling_ws_gpu.py): the spread kernels draw a whole call at the queried workspace size, the result
depends neither on the workspace nor on how a draw is cut into calls, a poisoned state stays poisoned.  New here: ``head`` (only
the first entries of every permutation are written) and the skip mode (the state advances, nothing is written)."""
import ctypes

import numpy as np
import pytest
import torch

from interpret_quality_amd import _lib, hip_ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

STARTS = {"fresh": 624, "zero": 0, "last": 623, "mid": 311}     # position word of the state a draw starts from
# the rejection mask changes at i = 2^k: both sides of every power of two from 64 on, and the smallest games
REGIONS = [2, 3, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1022, 1023, 1024]
_numpy_cache = {}


def _state(seed, pos):
    """A legacy generator state at position ``pos`` of its 624-word block (624: a fresh seed's, nothing generated yet)."""
    np.random.seed(seed)
    st = np.random.get_state()
    return ("MT19937", st[1], pos, 0, 0.0)


def _numpy(seed, pos, s, r):
    """NumPy's own draw, once per (state, S, R): (orders (S,R), the 625 state words afterwards); shared, never written to."""
    key = (seed, pos, s, r)
    if key not in _numpy_cache:
        np.random.set_state(_state(seed, pos))
        orders = np.stack([np.random.permutation(np.arange(r)) for _ in range(s)])
        after = np.random.get_state()
        words = np.concatenate([after[1], [after[2]]]).astype(np.uint32)
        orders.setflags(write=False)
        words.setflags(write=False)
        _numpy_cache[key] = (orders, words)
    return _numpy_cache[key]


def _wide(seed, pos, s, r, **kw):
    words = hip_ops.mt_state_to_device(DEV, _state(seed, pos))
    got = hip_ops.sample_permutations_wide(words, s, r, **kw)
    return (None if got is None else got.cpu().numpy()), words.cpu().numpy().view(np.uint32)


def _ctl():
    """Control words 0, 1 of the workspace the last call used: permutations the spread kernels wrote, word offset behind them."""
    return hip_ops._sample_ws[DEV][:8].view(torch.int32).tolist()


@pytest.mark.parametrize("start", sorted(STARTS))
@pytest.mark.parametrize("s", [1, 7, 300])
@pytest.mark.parametrize("r", REGIONS)
def test_permutations_and_state_equal_numpy(r, s, start):
    seed = 100 * r + s
    want, want_words = _numpy(seed, STARTS[start], s, r)
    got, got_words = _wide(seed, STARTS[start], s, r)
    assert got.dtype == np.int32 and got.shape == (s, r)
    assert np.array_equal(got, want)
    assert np.array_equal(got_words, want_words)
    if r <= 64:                                  # the narrow entry on the same state: the same rows and state
        lib = _lib.load()
        words = hip_ops.mt_state_to_device(DEV, _state(seed, STARTS[start]))
        old = torch.empty((s, r), dtype=torch.int32, device=DEV)
        _lib.check(lib.iq_sample_permutations(hip_ops._p(words), hip_ops._p(old), s, r, hip_ops._stream()), "iq_sample_permutations")
        assert np.array_equal(old.cpu().numpy(), got) and np.array_equal(words.cpu().numpy().view(np.uint32), got_words)


@pytest.mark.parametrize("start", sorted(STARTS))
def test_the_spread_kernels_draw_the_whole_call_at_the_size_the_query_gives(start):
    """3000 permutations of 1022 regions: 4.2 M words, about 6.8 k twists and a thousand segments of 4096 offsets, one call (68 MB
    of scratch, under the wrapper's cap).  The first control word of the workspace counts the permutations the spread kernels
    wrote; what is missing from S is left to the one-workgroup kernel.  At the queried size that is nothing."""
    s, r = 3000, 1022
    lib = _lib.load()
    nbytes = lib.iq_sample_wide_workspace_bytes(s, r)
    assert 60 << 20 < nbytes < hip_ops.SAMPLE_WIDE_WS_CAP and nbytes % 8 == 0
    want, want_words = _numpy(7, STARTS[start], s, r)
    got, got_words = _wide(7, STARTS[start], s, r)
    assert _ctl()[0] == s
    assert np.array_equal(got, want) and np.array_equal(got_words, want_words)


@pytest.mark.parametrize("r,m", [(128, 63), (1024, 511), (1022, 1022), (65, 1), (2, 1)])
def test_head_writes_the_first_entries_of_every_permutation(r, m):
    s = 300 if r > 2 else 5000
    want, want_words = _numpy(11, 311, s, r)
    for head in sorted({0, 1, m, r}):
        got, got_words = _wide(11, 311, s, r, head=head)
        assert got.shape == (s, head) and np.array_equal(got, want[:, :head]), head
        assert np.array_equal(got_words, want_words), head
    assert _ctl()[0] == s                        # the spread kernels' copy with a row stride of `head`, not only the finishing one's


def test_head_through_the_finishing_kernel_alone():
    want, want_words = _numpy(12, 100, 9, 1024)
    for head in (0, 3, 511, 1024):
        got, got_words = _wide(12, 100, 9, 1024, head=head, workspace_bytes=0)
        assert np.array_equal(got, want[:, :head]) and np.array_equal(got_words, want_words)


@pytest.mark.parametrize("s,r,nbytes", [(300, 1024, None), (9, 1024, 0), (300, 128, None), (2, 700, None)])
def test_skip_mode_leaves_the_state_of_the_full_draw_and_touches_no_output(s, r, nbytes):
    _, want_words = _numpy(13, 623, s, r)
    got, got_words = _wide(13, 623, s, r, skip=True, workspace_bytes=nbytes)
    assert got is None and np.array_equal(got_words, want_words)
    # the entry itself with a buffer it must not touch: head = 0, and a NULL `orders` with head > 0
    lib = _lib.load()
    ws_bytes = lib.iq_sample_wide_workspace_bytes(s, r) if nbytes is None else nbytes
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=DEV)
    guard = torch.full((s * r,), 77, dtype=torch.int32, device=DEV)
    for orders, head in ((hip_ops._p(guard), 0), (ctypes.c_void_p(0), r // 2)):
        words = hip_ops.mt_state_to_device(DEV, _state(13, 623))
        _lib.check(lib.iq_sample_permutations_wide(hip_ops._p(words), orders, s, r, head, hip_ops._p(ws), ws_bytes, hip_ops._stream()),
                   "iq_sample_permutations_wide")
        assert np.array_equal(words.cpu().numpy().view(np.uint32), want_words)
        assert bool((guard == 77).all())


def test_several_calls_equal_one_call():
    want, want_words = _numpy(14, 624, 340, 1024)
    words = hip_ops.mt_state_to_device(DEV, _state(14, 624))
    parts = [hip_ops.sample_permutations_wide(words, n, 1024) for n in (1, 9, 30, 300)]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), want)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), want_words)


def test_the_wrapper_cuts_a_large_draw_into_calls_under_its_cap(monkeypatch):
    """With the cap at 1 MiB (65 536 estimated words, about 43 permutations of 1024 regions) the wrapper draws 300 permutations in
    five calls or more, each into its slice of one output; the rows, with and without ``head``, and the state are the one call's."""
    lib = _lib.load()
    monkeypatch.setattr(hip_ops, "SAMPLE_WIDE_WS_CAP", 1 << 20)
    per_call = hip_ops._wide_sample_call_size(lib, 300, 1024, 1 << 20)
    assert 10 <= per_call <= 60
    assert lib.iq_sample_wide_workspace_bytes(per_call, 1024) <= 1 << 20 < lib.iq_sample_wide_workspace_bytes(per_call + 1, 1024)
    want, want_words = _numpy(15, 0, 300, 1024)
    for head in (None, 511):
        got, got_words = _wide(15, 0, 300, 1024, head=head)
        assert np.array_equal(got, want[:, :head]) and np.array_equal(got_words, want_words)
    _, got_words = _wide(15, 0, 300, 1024, skip=True)
    assert np.array_equal(got_words, want_words)


@pytest.mark.parametrize("which", ["none", "eight", "two_blocks", "half"])
def test_a_workspace_that_is_too_small_gives_the_same_result(which):
    """R = 1024, 40 permutations (56 k words).  0 and 8 bytes: the one-workgroup kernel alone; 20048 bytes hold two 624-word blocks,
    not one permutation: the spread kernels run and write nothing; half the queried size: they write about half of the rows."""
    s, r = 40, 1024
    full = _lib.load().iq_sample_wide_workspace_bytes(s, r)
    assert full > 4 * 20048
    nbytes = {"none": 0, "eight": 8, "two_blocks": 20048, "half": full // 2 // 8 * 8}[which]
    want, want_words = _numpy(16, 100, s, r)
    got, got_words = _wide(16, 100, s, r, workspace_bytes=nbytes)
    assert np.array_equal(got, want) and np.array_equal(got_words, want_words)
    if which == "two_blocks":
        assert _ctl()[0] == 0
    if which == "half":
        assert 10 <= _ctl()[0] <= 25


@pytest.mark.parametrize("s,r,head,nbytes", [(7, 128, 5, None), (300, 1024, 1024, None), (300, 1024, 511, 40000), (9, 1024, 2, 0)])
@pytest.mark.parametrize("position", [625, 1000, 0x7fffffff, 0xffffffff])
def test_a_malformed_or_poisoned_state_gives_rows_of_minus_one_and_stays_poisoned(position, s, r, head, nbytes):
    words = hip_ops.mt_state_to_device(DEV, _state(5, 624))
    key = words[:624].cpu().numpy().copy()
    words[624] = int(np.uint32(position).view(np.int32))
    for _ in range(2):                           # malformed, then already poisoned
        orders = hip_ops.sample_permutations_wide(words, s, r, head=head, workspace_bytes=nbytes)
        assert tuple(orders.shape) == (s, head) and bool((orders == -1).all())
        after = words.cpu().numpy().view(np.uint32)
        assert int(after[624]) == 0x7fffffff and np.array_equal(after[:624].view(np.int32), key)
    assert hip_ops.sample_permutations_wide(words, s, r, skip=True, workspace_bytes=nbytes) is None
    assert int(words.cpu().numpy().view(np.uint32)[624]) == 0x7fffffff
    with pytest.raises(_lib.IqError, match="did not complete"):
        hip_ops.mt_state_to_host(words, set_global=False)


def test_refused_arguments():
    lib = _lib.load()
    words = hip_ops.mt_state_to_device(DEV, _state(1, 624))
    before = words.clone()
    orders = torch.empty((4, 1025), dtype=torch.int32, device=DEV)
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device=DEV)
    for s, r, head in ((4, 0, 0), (4, 1025, 1025), (4, 1025, 3), (4, 128, 129), (4, 128, -1), (-1, 128, 128)):
        rc = lib.iq_sample_permutations_wide(hip_ops._p(words), hip_ops._p(orders), s, r, head, hip_ops._p(ws), ws.numel(), hip_ops._stream())
        assert rc == -1, (s, r, head, rc)        # IQ_EINVAL
        assert b"iq_sample_permutations_wide" in lib.iq_last_error()
    with pytest.raises(_lib.IqError):
        hip_ops.sample_permutations_wide(words, 4, 1025)
    with pytest.raises(_lib.IqError):
        hip_ops.sample_permutations_wide(words, 4, 128, head=129)
    rc = lib.iq_sample_permutations_wide(hip_ops._p(words), hip_ops._p(orders), 4, 128, 128, ctypes.c_void_p(ws.data_ptr() + 4), 1 << 15,
                                         hip_ops._stream())
    assert rc == -1 and b"aligned" in lib.iq_last_error()
    assert torch.equal(words, before)            # a refused call draws nothing
    assert tuple(hip_ops.sample_permutations_wide(words, 0, 128).shape) == (0, 128) and torch.equal(words, before)


def test_one_region_draws_nothing():
    words = hip_ops.mt_state_to_device(DEV, _state(2, 311))
    before = words.clone()
    assert bool((hip_ops.sample_permutations_wide(words, 5, 1) == 0).all()) and torch.equal(words, before)
