"""torch-tensor front end of the C ABI (include/iq.h).  PyTorch only owns the device memory and
the stream; all arithmetic happens in libiq_hip.so.  Every function raises if a tensor is not on
a GPU - there is no CPU fallback."""
import ctypes

import numpy as np
import torch

from . import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.IqError("%s must be a CUDA/HIP tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise _lib.IqError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise _lib.IqError("%s must be contiguous" % name)
    return ctypes.c_void_p(t.data_ptr())


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def as_i32(x, device):
    """int64 ndarray/tensor -> int32 device tensor (indices are int32 at the ABI)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    return x.to(device=device, dtype=torch.int32).contiguous()


def check_index_range(t, lo, hi, what):
    """Raise IqError unless every entry of the int32 device tensor ``t`` lies in [lo, hi) (iq_check_index_range; the one
    call that synchronises the stream).  The kernels never fault on a bad id, but their results are then meaningless."""
    lib = _lib.load()
    if t.numel() == 0:
        return
    scratch = torch.empty((1,), dtype=torch.int32, device=t.device)
    rc = lib.iq_check_index_range(_dev(t, torch.int32, what), t.numel(), int(lo), int(hi), _p(scratch), _stream())
    if rc != 0:
        msg = lib.iq_last_error()
        raise _lib.IqError("%s: %s" % (what, msg.decode() if msg else "index out of range"))


def check_host_indices(arr, lo, hi, what):
    """The same check for indices that are still on the host (region_id.npy, all_orders.npy, pair lists): free."""
    a = np.asarray(arr)
    if a.size and (a.min() < lo or a.max() >= hi):
        bad = int(np.flatnonzero((a.reshape(-1) < lo) | (a.reshape(-1) >= hi))[0])
        raise _lib.IqError("%s: index at position %d is outside [%d, %d)" % (what, bad, lo, hi))


def region_ids(region_id, device, num_regions):
    """Region ids of one cloud (ndarray from region_id.npy, or a tensor) -> validated int32 device tensor."""
    if isinstance(region_id, np.ndarray):
        check_host_indices(region_id, 0, num_regions, "region_id")
        return as_i32(region_id, device)
    t = as_i32(region_id, device)
    check_index_range(t, 0, num_regions, "region_id")
    return t


def region_bitmask(regions):
    """Iterable of region ids -> python int bit mask."""
    m = 0
    for r in regions:
        m |= 1 << int(r)
    return m


def masks_to_tensor(masks, device):
    """uint64 bit masks as an int64-typed device tensor (same bits)."""
    arr = np.asarray(masks, dtype=np.uint64).view(np.int64)
    return torch.from_numpy(np.ascontiguousarray(arr)).to(device)


def mt_state_to_device(device, state=None):
    """NumPy legacy generator state (np.random.get_state(); default: the GLOBAL generator's) -> (625,) int32 device tensor
    holding the 624 key words and the position, the form iq_sample_permutations advances."""
    st = np.random.get_state() if state is None else state
    if st[0] != "MT19937":
        raise _lib.IqError("the reference's sampling stream is NumPy's legacy MT19937 generator, got %r" % (st[0],))
    if not 0 <= int(st[2]) <= 624:     # np.random.set_state accepts any position; the generator itself never leaves 0..624
        raise _lib.IqError("MT19937 state with position %d outside 0..624" % int(st[2]))
    words = np.empty(625, dtype=np.uint32)
    words[:624], words[624] = st[1], st[2]
    return torch.from_numpy(words.view(np.int32)).to(device)


def mt_state_to_host(mt_state, set_global=True):
    """The advanced state back on the host (one device->host copy); ``set_global`` installs it as NumPy's global generator
    so that whatever the host draws next continues the reference's stream."""
    words = mt_state.cpu().numpy().view(np.uint32)
    if int(words[624]) > 624:          # iq_sample_permutations marks a state it could not draw all permutations from
        raise _lib.IqError("the device sampler did not complete (state position word %#x): the permutations of the last "
                           "sample_permutations call on this state are not valid" % int(words[624]))
    cur = np.random.get_state()          # the device drew 32-bit words only: a cached Gaussian of the host generator stays as it is
    st = ("MT19937", words[:624].copy(), int(words[624]), cur[3], cur[4])
    if set_global:
        np.random.set_state(st)
    return st


_sample_ws = {}       # device -> uint8 scratch tensor of the sampler, grown on demand
SAMPLE_WS_CAP = 32 << 20    # bytes kept per device at most (16 per estimated word: 50 000 permutations of 32 regions); beyond it
#                             the library's finishing kernel draws what the wide kernels could not


def sample_permutations(mt_state, num_samples, num_regions, workspace_bytes=None):
    """iq_sample_permutations_ws: (S,R) int32 permutations continuing the generator ``mt_state`` (advanced in place, no sync).
    ``workspace_bytes``: lend the library that much scratch instead of what iq_sample_workspace_bytes asks for (the result does
    not depend on it; 0 = the one-workgroup kernel alone).  The scratch tensor is one per device: calls on one device are
    expected on one stream, like the engines' workspaces."""
    lib = _lib.load()
    s, r = int(num_samples), int(num_regions)
    orders = torch.empty((s, r), dtype=torch.int32, device=mt_state.device)
    state = _dev(mt_state, torch.int32, "mt_state")
    nbytes = min(lib.iq_sample_workspace_bytes(s, r), SAMPLE_WS_CAP) if workspace_bytes is None else int(workspace_bytes)
    ws = _sample_ws.get(mt_state.device)
    if nbytes and (ws is None or ws.numel() < nbytes):
        ws = _sample_ws[mt_state.device] = torch.empty((nbytes,), dtype=torch.uint8, device=mt_state.device)
    _lib.check(lib.iq_sample_permutations_ws(state, _p(orders), s, r, _p(ws) if nbytes else ctypes.c_void_p(0), nbytes, _stream()),
               "iq_sample_permutations_ws")
    return orders


def prefix_keep_masks(orders):
    """orders (S,R) i32 -> (S*(R+1),) int64-typed keep masks of the prefix coalitions (tools/final_common.py:56-60)."""
    lib = _lib.load()
    s, r = orders.shape
    keep = torch.empty((s * (r + 1),), dtype=torch.int64, device=orders.device)
    _lib.check(lib.iq_prefix_keep_masks(_dev(orders, torch.int32, "orders"), _p(keep), s, r, _stream()), "iq_prefix_keep_masks")
    return keep


def context_keep_masks(pairs, contexts):
    """pairs (P,2) i32, contexts (P,C,m) i32 -> (4*P*C,) int64-typed keep masks, rows S+{i,j}, S+{i}, S+{j}, S per context
    (final_point_binary_interaction_logits.py:45-52)."""
    lib = _lib.load()
    p, c, m = contexts.shape
    keep = torch.empty((4 * p * c,), dtype=torch.int64, device=pairs.device)
    _lib.check(lib.iq_context_keep_masks(_dev(pairs, torch.int32, "pairs"), _dev(contexts, torch.int32, "contexts") if m else ctypes.c_void_p(0),
                                         _p(keep), p, c, m, _stream()), "iq_context_keep_masks")
    return keep


def mask_shapley(cloud, region_id, orders, center, channel_first=False):
    """cloud (N,3) f32, region_id (N,) i32, orders (bs,R) i32, center (3,) f32 ->
    (bs*(R+1), N, 3) or (bs*(R+1), 3, N)."""
    lib = _lib.load()
    n = cloud.shape[0]
    bs, r = orders.shape
    shape = (bs * (r + 1), 3, n) if channel_first else (bs * (r + 1), n, 3)
    out = torch.empty(shape, dtype=torch.float32, device=cloud.device)
    _lib.check(lib.iq_mask_shapley(_dev(cloud, torch.float32, "cloud"), _dev(region_id, torch.int32, "region_id"),
                                   _dev(orders, torch.int32, "orders"), _dev(center, torch.float32, "center"),
                                   _p(out), n, r, bs, int(channel_first), _stream()), "iq_mask_shapley")
    return out


def mask_interaction(cloud, region_id, pairs, ctx_mask, center, num_regions):
    """pairs (nb,2) i32, ctx_mask (nb,) i64 (bit masks) -> (4*nb, 3, N)."""
    lib = _lib.load()
    n = cloud.shape[0]
    nb = pairs.shape[0]
    out = torch.empty((4 * nb, 3, n), dtype=torch.float32, device=cloud.device)
    _lib.check(lib.iq_mask_interaction(_dev(cloud, torch.float32, "cloud"), _dev(region_id, torch.int32, "region_id"),
                                       _dev(pairs, torch.int32, "pairs"), _dev(ctx_mask, torch.int64, "ctx_mask"),
                                       _dev(center, torch.float32, "center"), _p(out), n, num_regions, nb,
                                       _stream()), "iq_mask_interaction")
    return out


def mask_coalitions(cloud, region_id, keep, center, channel_first=False):
    lib = _lib.load()
    n = cloud.shape[0]
    b = keep.shape[0]
    shape = (b, 3, n) if channel_first else (b, n, 3)
    out = torch.empty(shape, dtype=torch.float32, device=cloud.device)
    _lib.check(lib.iq_mask_coalitions(_dev(cloud, torch.float32, "cloud"), _dev(region_id, torch.int32, "region_id"),
                                      _dev(keep, torch.int64, "keep"), _dev(center, torch.float32, "center"),
                                      _p(out), n, b, int(channel_first), _stream()), "iq_mask_coalitions")
    return out


def reward(logits, label, modified=True):
    lib = _lib.load()
    b, c = logits.shape
    v = torch.empty((b,), dtype=torch.float32, device=logits.device)
    _lib.check(lib.iq_reward(_dev(logits, torch.float32, "logits"), int(label), int(modified), _p(v), b, c,
                             _stream()), "iq_reward")
    return v


def reward_classes(logits, labels=None, modified=True, out=None, first=0):
    """iq_reward_classes: logits (B,C) f32, ``labels`` a sequence of labels in [0, C) (any order, repeats allowed; None = every
    class) -> (G,B) f32 whose row g carries ``reward(logits, labels[g], modified)``'s bits.  With ``out`` ((G,M) f32, contiguous)
    the rewards go to out[:, first:first+B] and nothing else of ``out`` is touched: a table filled one chunk of coalitions at a
    time."""
    lib = _lib.load()
    b, c = _shape(logits, "logits", None, None)
    lab = None if labels is None else [int(x) for x in labels]
    g = c if lab is None else len(lab)
    if out is None:
        out, first = torch.empty((g, b), dtype=torch.float32, device=logits.device), 0
    first = int(first)
    _, m = _shape(out, "out", g, None)
    if first < 0 or first + b > m:
        raise _lib.IqError("out has %d columns: rows %d .. %d do not fit" % (m, first, first + b))
    host = None if lab is None else (ctypes.c_int32 * max(g, 1))(*lab)
    base = _dev(out, torch.float32, "out").value or 0
    _lib.check(lib.iq_reward_classes(_dev(logits, torch.float32, "logits"), host, g, int(bool(modified)),
                                     ctypes.c_void_p(base + 4 * first), m, b, c, _stream()), "iq_reward_classes")
    return out


def _shapley_accum(entry, v, orders, snap_counts, exact=True):
    """The body of shapley_accum and shapley_accum_wide: ``entry`` names the library call.  The kernel reads the first S*(R+1)
    rewards: a shorter ``v`` is always refused, a longer one unless ``exact`` is False."""
    lib = _lib.load()
    s, r = orders.shape
    dev = v.device
    if v.numel() < s * (r + 1) or (exact and v.numel() != s * (r + 1)):
        raise _lib.IqError("v holds %d rewards for %d permutations of %d regions" % (v.numel(), s, r))
    sv_rows = torch.zeros((max(s, 1), r), dtype=torch.float64, device=dev)
    phi = torch.empty((r,), dtype=torch.float64, device=dev)
    snaps = counts = None
    n_snap = 0
    if snap_counts is not None and len(snap_counts) > 0:
        counts = torch.tensor(list(snap_counts), dtype=torch.int32, device=dev)
        n_snap = counts.numel()
        snaps = torch.zeros((n_snap, r), dtype=torch.float64, device=dev)
    _lib.check(getattr(lib, entry)(_dev(v, torch.float32, "v"), _dev(orders, torch.int32, "orders"), _p(sv_rows), _p(phi), _p(counts),
                                   n_snap, _p(snaps), r, s, _stream()), entry)
    return phi, sv_rows[:s], snaps


def shapley_accum(v, orders, snap_counts=None):
    """v (S*(R+1),) f32, orders (S,R) i32 -> (phi_sum (R,) f64, sv_rows (S,R) f64, snaps or None).  A longer ``v`` is let through as
    before (pose_sweep.shapley_over_poses passes one when all_orders.npy holds fewer than num_samples permutations)."""
    return _shapley_accum("iq_shapley_accum", v, orders, snap_counts, exact=False)


def shapley_snapshots(v, orders, counts, accum=shapley_accum):
    """The tail of every sampling loop: ``accum`` (shapley_accum or shapley_accum_wide) with running sums at the ``counts`` that
    do not exceed S, everything moved to the host -> ({count: (R,) float64 running sum}, rows (S,R) float64, total (R,))."""
    s, r = orders.shape
    counts = [int(c) for c in (counts or []) if c <= s]
    total, rows, snaps = accum(v, orders, snap_counts=counts)
    snaps = snaps.cpu().numpy() if snaps is not None else np.zeros((0, r))
    return {c: snaps[k] for k, c in enumerate(counts)}, rows.cpu().numpy(), total.cpu().numpy()


def interaction_reduce(v):
    lib = _lib.load()
    n = v.numel() // 4
    out = torch.empty((n,), dtype=torch.float32, device=v.device)
    _lib.check(lib.iq_interaction_reduce(_dev(v, torch.float32, "v"), _p(out), n, _stream()), "iq_interaction_reduce")
    return out


MAX_EXACT_PLAYERS = 24      # IQ_MAX_EXACT_PLAYERS of include/iq.h (tests/test_exact_cpu.py compares the two)


def enum_keep_masks(first, count, n, device, players=None, base=0):
    """iq_enum_keep_masks: (count,) int64-typed keep masks of the coalitions first .. first + count - 1 of an n-player game;
    player k is region players[k] (None: region k), the regions of the bit mask ``base`` are kept in every coalition."""
    lib = _lib.load()
    if torch.device(device).type != "cuda":
        raise _lib.IqError("enum_keep_masks needs a GPU device (the HIP path has no CPU fallback)")
    keep = torch.empty((int(count),), dtype=torch.int64, device=device)
    pl = None
    if players is not None:
        pl = np.ascontiguousarray(np.asarray(players, dtype=np.int64).reshape(-1).clip(-1, 64), dtype=np.int32)
        if pl.size != int(n):
            raise _lib.IqError("players names %d regions for n=%d players" % (pl.size, int(n)))
    _lib.check(lib.iq_enum_keep_masks(_p(keep), int(first) & (2 ** 64 - 1), int(count), ctypes.c_void_p(pl.ctypes.data if pl is not None else 0),
                                      int(n), int(base) & (2 ** 64 - 1), _stream()), "iq_enum_keep_masks")
    return keep


def _value_table(v):
    """The number of players of a (2^n,) float32 table of coalition rewards."""
    _dev(v, torch.float32, "v")
    n = int(v.numel()).bit_length() - 1
    if v.dim() != 1 or v.numel() != 1 << max(n, 0) or not 1 <= n <= MAX_EXACT_PLAYERS:
        raise _lib.IqError("v must be a (2^n,) table with 1 <= n <= %d, got shape %s" % (MAX_EXACT_PLAYERS, tuple(v.shape)))
    return n


def _exact_scratch(lib, n, p, device):
    return torch.empty((lib.iq_exact_scratch_bytes(n, p) // 8,), dtype=torch.float64, device=device)


def exact_shapley(v):
    """v (2^n,) f32 rewards of all coalitions (bit k of the index = player k present) -> (n,) f64 Shapley values
    (iq_exact_shapley: float64, fixed order, bitwise repeatable)."""
    lib = _lib.load()
    n = _value_table(v)
    phi = torch.empty((n,), dtype=torch.float64, device=v.device)
    scratch = _exact_scratch(lib, n, 0, v.device)
    _lib.check(lib.iq_exact_shapley(_p(v), n, _p(phi), _p(scratch), scratch.numel() * 8, _stream()), "iq_exact_shapley")
    return phi


def all_pairs(n):
    """The n(n-1)/2 pairs (i, j), i < j, of player positions, in lexicographic order: (P,2) int32 ndarray."""
    return np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int32).reshape(-1, 2)


def exact_interactions(v, pairs=None):
    """v (2^n,) f32, pairs (P,2) player positions (None: all_pairs(n)) -> (P, n-1) f64: out[p][m] = the mean of
    ((v[c|i|j] + v[c]) - v[c|i]) - v[c|j] over ALL contexts c of m players (iq_exact_interactions)."""
    lib = _lib.load()
    n = _value_table(v)
    if isinstance(pairs, torch.Tensor):
        pr = pairs.to(device=v.device, dtype=torch.int32).contiguous()
        if pr.dim() != 2 or pr.shape[1] != 2:
            raise _lib.IqError("pairs must be (P,2), got %s" % (tuple(pr.shape),))
        check_index_range(pr, 0, n, "pairs")
        if bool((pr[:, 0] == pr[:, 1]).any()):
            raise _lib.IqError("pairs: a pair names the same player twice")
    else:
        host = all_pairs(n) if pairs is None else np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        check_host_indices(host, 0, n, "pairs")
        if host.size and (host[:, 0] == host[:, 1]).any():
            raise _lib.IqError("pairs: pair %d names the same player twice" % int(np.flatnonzero(host[:, 0] == host[:, 1])[0]))
        pr = as_i32(host, v.device)
    p = pr.shape[0]
    out = torch.empty((p, n - 1), dtype=torch.float64, device=v.device)
    if p:
        scratch = _exact_scratch(lib, n, p, v.device)
        _lib.check(lib.iq_exact_interactions(_p(v), n, _p(pr), p, _p(out), _p(scratch), scratch.numel() * 8, _stream()),
                   "iq_exact_interactions")
    return out


def moebius(v):
    """v (2^n,) f32 -> (2^n,) f64 Harsanyi dividends a[c] = sum over subsets t of c of (-1)^(|c|-|t|) v[t] (iq_moebius)."""
    lib = _lib.load()
    n = _value_table(v)
    a = torch.empty((1 << n,), dtype=torch.float64, device=v.device)
    _lib.check(lib.iq_moebius(_p(v), n, _p(a), _stream()), "iq_moebius")
    return a


MAX_KSHAP_REGIONS = 64      # IQ_MAX_REGIONS: the regression estimator's rows are one uint64 each


class KshapSingular(_lib.IqError):
    """kshap_solve: the rows behind A do not determine the regression."""


def kshap_regions(n):
    """The region count of a game the regression estimator takes, as an int (IqError outside 2 .. 64)."""
    n = int(n)
    if not 2 <= n <= MAX_KSHAP_REGIONS:
        raise _lib.IqError("the regression estimator takes 2 .. %d regions, got %d" % (MAX_KSHAP_REGIONS, n))
    return n


def _kshap_keep_masks(entry, regions, words, orders, sizes, paired):
    """The body of kshap_keep_masks and kshap_keep_masks_wide: ``entry`` names the library call, ``regions`` checks the region
    count, ``words(n)`` is the shape of one keep row."""
    lib = _lib.load()
    _dev(orders, torch.int32, "orders")
    s, n = _shape(orders, "orders", None, None)
    n = regions(n)
    _shape(sizes, "sizes", s)
    keep = torch.empty((2 * s if paired else s,) + words(n), dtype=torch.int64, device=orders.device)
    status = torch.zeros((1,), dtype=torch.int32, device=orders.device)
    _lib.check(getattr(lib, entry)(_p(orders), _dev(sizes, torch.int32, "sizes"), _p(keep), s, n, int(bool(paired)), _p(status),
                                   _stream()), entry)
    verdict = int(status.item()) if s else 0
    if verdict:
        raise _lib.IqError(entry[3:] + ": " + ("a size lies outside 1 .. %d" % (n - 1) if verdict == 1
                                               else "an order entry lies outside [0, %d)" % n))
    return keep


def kshap_keep_masks(orders, sizes, paired=True):
    """orders (S,n) i32 permutations, sizes (S,) i32 in 1 .. n-1 -> int64-typed keep masks (iq_kshap_keep_masks): the first
    sizes[m] entries of permutation m; ``paired``: (2S,) with every set followed by its complement within the n bits, else (S,).
    A size outside 1 .. n-1 or an order entry outside [0, n) raises IqError (one 4-byte read back)."""
    return _kshap_keep_masks("iq_kshap_keep_masks", kshap_regions, lambda n: (), orders, sizes, paired)


def _opt(t, dtype, name):
    """The pointer of an optional tensor argument: NULL for None."""
    return _dev(t, dtype, name) if t is not None else ctypes.c_void_p(0)


def _kshap_scratch_words(what, nbytes, m, r, g, regions="R"):
    """The answer of a regression entry's ``*_scratch_bytes`` -> the float64 words of its scratch; 0 bytes refuses the shape."""
    if nbytes == 0:
        raise _lib.IqError("%s: M=%d rows, %s=%d regions, G=%d games is out of range" % (what, m, regions, r, g))
    return nbytes // 8


def _kshap_scratch(what, nbytes, m, r, g, dev, regions="R"):
    """The scratch of a regression entry, uninitialised.  (The control-variate wrappers lend zeroed memory on purpose and allocate
    their own: the note above ``kshap_pairs_terms``.)"""
    return torch.empty((_kshap_scratch_words(what, nbytes, m, r, g, regions),), dtype=torch.float64, device=dev)


def _pair_coef(r, dev):
    """The (r+1, 3) float64 table (alpha, beta, gamma) of the all-pairs entries, on the device."""
    from . import kernelshap
    return torch.from_numpy(kernelshap.pair_coefficients(r)).to(dev)


def kshap_accum(keep, v, v0, n, weights=None):
    """keep (M,) int64-typed rows, v (G,M) f32 rewards of G games on those rows, v0 (G,) f64, weights (M,) f64 or None (all 1) ->
    (A (n,n) f64, b (G,n) f64, wsum (1,) f64): the RAW sums A = sum w z z^T, b[g] = sum w z (v[g] - v0[g]), wsum = sum w
    (iq_kshap_accum: float64 in a fixed order, bitwise repeatable; without weights A holds exact counts and wsum = M)."""
    lib = _lib.load()
    n = kshap_regions(n)
    m, = _shape(keep, "keep", None)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    if weights is not None:
        _shape(weights, "weights", m)
    dev = keep.device
    nbytes = lib.iq_kshap_scratch_bytes(m, n, g)
    scratch = _kshap_scratch("kshap_accum", nbytes, m, n, g, dev, regions="n")
    a = torch.empty((n, n), dtype=torch.float64, device=dev)
    b = torch.empty((g, n), dtype=torch.float64, device=dev)
    wsum = torch.empty((1,), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_accum(_dev(keep, torch.int64, "keep"), _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"),
                                  _opt(weights, torch.float64, "weights"), m, n, g, _p(a), _p(b), _p(wsum), _p(scratch), nbytes, _stream()), "iq_kshap_accum")
    return a, b, wsum


def kshap_solve(a, b, delta):
    """a (n,n) f64 symmetric positive definite, b (G,n) f64, delta (G,) f64 -> phi (G,n) f64 with a phi[g] + lambda 1 = b[g] and
    sum(phi[g]) = delta[g] (iq_kshap_solve: one workgroup, Cholesky in LDS).  IqError when the rows behind ``a`` do not
    determine the regression (a status word read back, not a fault)."""
    lib = _lib.load()
    n = kshap_regions(_shape(a, "a", None, None)[0])
    _shape(a, "a", n, n)
    g, _ = _shape(b, "b", None, n)
    _shape(delta, "delta", g)
    phi = torch.empty((g, n), dtype=torch.float64, device=a.device)
    status = torch.zeros((1,), dtype=torch.int32, device=a.device)
    _lib.check(lib.iq_kshap_solve(_dev(a, torch.float64, "a"), _dev(b, torch.float64, "b"), _dev(delta, torch.float64, "delta"),
                                  _p(phi), _p(status), n, g, _stream()), "iq_kshap_solve")
    if int(status.item()):
        raise KshapSingular("the sampled coalitions do not determine the regression: draw more samples or use gram='analytic'")
    return phi


def region_assign(cloud, fps_idx):
    lib = _lib.load()
    n = cloud.shape[0]
    r = fps_idx.shape[0]
    out = torch.empty((n,), dtype=torch.int32, device=cloud.device)
    _lib.check(lib.iq_region_assign(_dev(cloud, torch.float32, "cloud"), _dev(fps_idx, torch.int32, "fps_idx"),
                                    _p(out), n, r, _stream()), "iq_region_assign")
    return out


# ---- wide coalitions: more than 64 regions, up to one region per point (include/iq.h, "Wide coalitions") ----------------------

MAX_WIDE_REGIONS = 1024     # IQ_MAX_WIDE_REGIONS of include/iq.h (tests/test_wide_cpu.py compares the two)


def wide_words(num_regions):
    """Words per wide keep row: ceil(R / 64), after the range check every wide wrapper makes."""
    r = int(num_regions)
    if not 1 <= r <= MAX_WIDE_REGIONS:
        raise _lib.IqError("num_regions=%d is outside [1, %d]" % (r, MAX_WIDE_REGIONS))
    return (r + 63) // 64


def wide_keep(keep, num_regions):
    """The one check of wide keep rows: (B, wide_words(R)) int64, contiguous, on the GPU -> their pointer."""
    w = wide_words(num_regions)
    if keep.dim() != 2 or keep.shape[1] != w:
        raise _lib.IqError("keep must be (B, %d) for %d regions, got %s" % (w, int(num_regions), tuple(keep.shape)))
    return _dev(keep, torch.int64, "keep")


def region_words(ids, num_regions, prefixes=False):
    """Host: region ids (..., k) -> (..., W) uint64 words of the set they name, bit (r & 63) of word (r >> 6) = region r; an
    entry outside [0, R) is ignored, as the device builders ignore it.  ``prefixes``: (..., k + 1, W), row i the set of the
    first i ids (OR-accumulated).  The one builder behind the four host *_keep_masks; one pass over the ids per word."""
    r = int(num_regions)
    w = wide_words(r)
    ids = np.asarray(ids, dtype=np.int64)
    k = ids.shape[-1]
    out = np.zeros(ids.shape[:-1] + ((k + 1, w) if prefixes else (w,)), dtype=np.uint64)
    if k:
        for j in range(w):
            # NumPy shifts by a count outside 0..63 to 0: an id of another word, or a negative one (huge as uint64), sets nothing
            bits = np.left_shift(np.uint64(1), (ids - 64 * j if j else ids).astype(np.uint64))
            if prefixes:
                np.bitwise_or.accumulate(bits, axis=-1, out=out[..., 1:, j])
            else:
                out[..., j] = np.bitwise_or.reduce(bits, axis=-1)
        if r & 63:
            out[..., w - 1] &= np.uint64((1 << (r & 63)) - 1)      # ids in [R, 64 W)
    return out


def wide_masks_to_tensor(masks, device):
    """(B,W) uint64 keep rows as an int64-typed device tensor (same bits)."""
    arr = np.ascontiguousarray(np.asarray(masks, dtype=np.uint64))
    if arr.ndim != 2:
        raise _lib.IqError("wide masks must be (B,W), got %s" % (arr.shape,))
    return torch.from_numpy(arr.view(np.int64)).to(device)


def prefix_keep_masks_wide(orders):
    """orders (S,R) i32 -> (S*(R+1), W) int64-typed keep rows of the prefix coalitions (iq_prefix_keep_masks_wide)."""
    lib = _lib.load()
    s, r = orders.shape
    keep = torch.empty((s * (r + 1), wide_words(r)), dtype=torch.int64, device=orders.device)
    _lib.check(lib.iq_prefix_keep_masks_wide(_dev(orders, torch.int32, "orders"), _p(keep), s, r, _stream()),
               "iq_prefix_keep_masks_wide")
    return keep


def context_keep_masks_wide(pairs, contexts, num_regions):
    """pairs (P,2) i32, contexts (P,C,m) i32, 0 <= m <= R -> (4*P*C, W) int64-typed keep rows S+{i,j}, S+{i}, S+{j}, S per context
    (iq_context_keep_masks_wide; final_point_binary_interaction_logits.py:45-52).  An entry outside [0, R) is ignored."""
    lib = _lib.load()
    r = int(num_regions)
    w = wide_words(r)
    _shape(pairs, "pairs", None, 2)
    p, c, m = _shape(contexts, "contexts", pairs.shape[0], None, None)
    if m > r:
        raise _lib.IqError("contexts name %d regions each, the game has %d" % (m, r))
    keep = torch.empty((4 * p * c, w), dtype=torch.int64, device=pairs.device)
    _lib.check(lib.iq_context_keep_masks_wide(_dev(pairs, torch.int32, "pairs"),
                                              _dev(contexts, torch.int32, "contexts") if contexts.numel() else ctypes.c_void_p(0),
                                              _p(keep), p, c, m, r, _stream()), "iq_context_keep_masks_wide")
    return keep


SAMPLE_WIDE_WS_CAP = 128 << 20   # bytes of sampler scratch per device that sample_permutations_wide asks for at most


def _wide_sample_call_size(lib, s, r, cap):
    """The most permutations of ``r`` regions, at most ``s``, whose queried workspace stays within ``cap`` bytes (at least 1)."""
    if lib.iq_sample_wide_workspace_bytes(s, r) <= cap:
        return s
    lo, hi = 1, s                      # the query never shrinks as S grows: lo fits (or is 1), hi does not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.iq_sample_wide_workspace_bytes(mid, r) <= cap else (lo, mid)
    return lo


def sample_permutations_wide(mt_state, num_samples, num_regions, head=None, skip=False, workspace_bytes=None):
    """iq_sample_permutations_wide: the first ``head`` entries (None: all R) of S permutations of 1 <= R <= MAX_WIDE_REGIONS regions
    continuing the generator ``mt_state`` (advanced in place, no sync) -> (S, head) int32.  ``skip``: draw, advance the state, write
    and return nothing.  The scratch is iq_sample_wide_workspace_bytes's 16 bytes per estimated word (the key, next[] and an 8-byte
    hop per word offset; about 1413 words per permutation of 1024 regions), and a large draw is cut into calls so that the scratch
    tensor - one per device, shared with ``sample_permutations`` - stays under SAMPLE_WIDE_WS_CAP = 128 MiB: about 5900 permutations
    of 1024 regions per call.  Rows and state do not depend on the cut.  ``workspace_bytes``: one call that lends the library
    exactly that much instead (0 = the one-workgroup kernel alone; the result does not depend on it either)."""
    lib = _lib.load()
    s, r = int(num_samples), int(num_regions)
    h = 0 if skip else r if head is None else int(head)
    state = _dev(mt_state, torch.int32, "mt_state")
    dev = mt_state.device
    orders = None if skip else torch.empty((max(s, 0), max(h, 0)), dtype=torch.int32, device=dev)
    per_call = s if workspace_bytes is not None or s <= 0 else _wide_sample_call_size(lib, s, r, SAMPLE_WIDE_WS_CAP)
    done = 0
    while True:
        n = min(per_call, s - done)
        nbytes = lib.iq_sample_wide_workspace_bytes(n, r) if workspace_bytes is None else int(workspace_bytes)
        ws = _sample_ws.get(dev)
        if nbytes and (ws is None or ws.numel() < nbytes):
            ws = _sample_ws[dev] = None        # release the old tensor before the larger one is made
            ws = _sample_ws[dev] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        out = ctypes.c_void_p(0) if orders is None or orders.numel() == 0 else ctypes.c_void_p(orders.data_ptr() + 4 * done * h)
        _lib.check(lib.iq_sample_permutations_wide(state, out, n, r, h, _p(ws) if nbytes else ctypes.c_void_p(0), nbytes, _stream()),
                   "iq_sample_permutations_wide")
        done += n
        if done >= s:
            return orders


def context_regions_wide(pairs, heads, num_regions):
    """iq_context_regions_wide: ``heads`` (P,C,m) i32 device tensor, heads of permutations of R - 2, becomes IN PLACE the context
    regions rest[heads] - rest the ascending regions outside the pair (final_gen_pair.py:25-29) - and is returned.  ``pairs``
    (P,2): a host array (checked here: i != j, both in [0, R)) ."""
    lib = _lib.load()
    r = int(num_regions)
    wide_words(r)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    check_host_indices(pairs, 0, r, "pairs")
    if (pairs[:, 0] == pairs[:, 1]).any():
        raise _lib.IqError("pairs: pair %d names one region twice" % int(np.flatnonzero(pairs[:, 0] == pairs[:, 1])[0]))
    p, c, m = _shape(heads, "heads", pairs.shape[0], None, None)
    if m > r - 2:
        raise _lib.IqError("a context of %d regions does not fit beside a pair in %d" % (m, r))
    _lib.check(lib.iq_context_regions_wide(_p(as_i32(pairs, heads.device)), _dev(heads, torch.int32, "heads"), p, c, m, r, _stream()),
               "iq_context_regions_wide")
    return heads


def mask_coalitions_wide(cloud, region_id, keep, center, num_regions, channel_first=False):
    """cloud (N,3) f32, region_id (N,) i32, keep (B,W) i64, center (3,) f32 -> (B,N,3) or (B,3,N) (iq_mask_coalitions_wide)."""
    lib = _lib.load()
    n = cloud.shape[0]
    kp = wide_keep(keep, num_regions)
    b = keep.shape[0]
    out = torch.empty((b, 3, n) if channel_first else (b, n, 3), dtype=torch.float32, device=cloud.device)
    _lib.check(lib.iq_mask_coalitions_wide(_dev(cloud, torch.float32, "cloud"), _dev(region_id, torch.int32, "region_id"), kp,
                                           _dev(center, torch.float32, "center"), _p(out), n, int(num_regions), b,
                                           int(channel_first), _stream()), "iq_mask_coalitions_wide")
    return out


def region_assign_wide(cloud, fps_idx):
    """cloud (N,3) f32, fps_idx (R,) i32 with R <= MAX_WIDE_REGIONS -> (N,) i32 region ids (iq_region_assign_wide)."""
    lib = _lib.load()
    n = cloud.shape[0]
    r = fps_idx.shape[0]
    wide_words(r)
    out = torch.empty((n,), dtype=torch.int32, device=cloud.device)
    _lib.check(lib.iq_region_assign_wide(_dev(cloud, torch.float32, "cloud"), _dev(fps_idx, torch.int32, "fps_idx"),
                                         _p(out), n, r, _stream()), "iq_region_assign_wide")
    return out


def shapley_accum_wide(v, orders, snap_counts=None):
    """shapley_accum for R <= MAX_WIDE_REGIONS: v (S*(R+1),) f32, orders (S,R) i32 -> (phi_sum (R,) f64, sv_rows (S,R) f64,
    snaps or None)."""
    wide_words(orders.shape[1])
    return _shapley_accum("iq_shapley_accum_wide", v, orders, snap_counts)


def shapley_games_scratch_bytes(num_regions, num_samples, num_games):
    """iq_shapley_games_scratch_bytes: the 16-bit (S,R) position table of shapley_accum_games; it does not depend on the game count."""
    return int(_lib.load().iq_shapley_games_scratch_bytes(int(num_regions), int(num_samples), int(num_games)))


def shapley_accum_games(v, orders, snap_counts=None, validate=True, entry="iq_shapley_accum_games"):
    """iq_shapley_accum_games: v (G,M) f32 with M >= S*(R+1) - row g the rewards of game g on the prefix coalitions of ``orders``,
    the table reward_classes fills - and orders (S,R), 1 <= R <= MAX_WIDE_REGIONS -> (phi_sum (G,R) f64, snaps (G,n_snap,R) f64 or
    None): per game the bits of shapley_accum_wide (for R <= 64 also shapley_accum's), without any per-game (S,R) row table.
    ``orders``: an ndarray (validated on the host, free) or an int32 device tensor (validated by check_index_range, one 4-byte
    read back, unless ``validate`` is False: the caller has checked them)."""
    lib = _lib.load()
    g, m = _shape(v, "v", None, None)
    dev = v.device
    if isinstance(orders, np.ndarray):
        if orders.ndim != 2:
            raise _lib.IqError("orders must be (S, R), got %s" % (orders.shape,))
        check_host_indices(orders, 0, orders.shape[1], "orders")
        orders = as_i32(orders, dev)
    else:
        _shape(orders, "orders", None, None)
        if validate:
            check_index_range(orders, 0, orders.shape[1], "orders")
    s, r = orders.shape
    wide_words(r)
    if g < 1 or m < s * (r + 1):
        raise _lib.IqError("v is (%d, %d): at least one game of %d rewards is needed for %d permutations of %d regions"
                           % (g, m, s * (r + 1), s, r))
    nbytes = lib.iq_shapley_games_scratch_bytes(r, s, g)
    scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    phi = torch.empty((g, r), dtype=torch.float64, device=dev)
    snaps = counts = None
    n_snap = 0
    if snap_counts is not None and len(snap_counts) > 0:
        counts = torch.tensor(list(snap_counts), dtype=torch.int32, device=dev)
        n_snap = counts.numel()
        snaps = torch.zeros((g, n_snap, r), dtype=torch.float64, device=dev)
    _lib.check(getattr(lib, entry)(_dev(v, torch.float32, "v"), m, _p(orders), _p(phi), _p(counts), n_snap, _p(snaps), r, s, g,
                                   _p(scratch), nbytes, _stream()), entry)
    return phi, snaps


def shapley_sq_accum_games(v, orders, snap_counts=None, validate=True):
    """iq_shapley_sq_accum_games: ``shapley_accum_games`` with every widened float32 difference squared before it is added ->
    (sq_sum (G,R) f64, sq_snaps (G,n_snap,R) f64 or None), strictly in permutation order: with the sums of ``shapley_accum_games``
    the second moment a standard error needs (``shapley_se``)."""
    return shapley_accum_games(v, orders, snap_counts, validate, "iq_shapley_sq_accum_games")


def shapley_se(total, sq, count):
    """The standard error of the permutation estimator's mean at ``count`` >= 2 permutations from the running sum ``total`` and
    sum of squares ``sq`` (ndarrays or tensors of one shape): sqrt(max(sq - total^2 / n, 0) / (n (n - 1))) -> float64 ndarray.
    Formed in extended precision where NumPy has it and rounded once: the difference cancels where the mean is large beside the
    spread, and the two float64 sums should be all that is rounded before it."""
    n = int(count)
    if n < 2:
        raise _lib.IqError("a standard error needs at least 2 permutations, got %d" % n)
    t, q = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64).astype(np.longdouble) for x in (total, sq))
    return np.sqrt(np.maximum(q - t * t / n, 0) / (n * (n - 1))).astype(np.float64)


def kshap_regions_wide(r):
    """The region count of a game the wide regression estimator's entry points take, as an int (IqError outside 2 .. 1024)."""
    r = int(r)
    if not 2 <= r <= MAX_WIDE_REGIONS:
        raise _lib.IqError("the wide regression estimator takes 2 .. %d regions, got %d" % (MAX_WIDE_REGIONS, r))
    return r


def kshap_keep_masks_wide(orders, sizes, paired=True):
    """``kshap_keep_masks`` for wide rows: orders (S,R) i32 permutations, sizes (S,) i32 in 1 .. R-1 -> (2S or S, W) int64-typed
    keep rows (iq_kshap_keep_masks_wide), every set followed by its complement within the R bits when ``paired``.  A size outside
    1 .. R-1 or an order entry outside [0, R) raises IqError (one 4-byte read back)."""
    return _kshap_keep_masks("iq_kshap_keep_masks_wide", kshap_regions_wide, lambda r: (wide_words(r),), orders, sizes, paired)


def kshap_moment_wide(keep, v, v0, num_regions, weights=None):
    """keep (M,W) int64-typed wide rows, v (G,M) f32 rewards of G games on those rows, v0 (G,) f64, weights (M,) f64 or None (all 1)
    -> (b (G,R) f64, wsum (1,) f64): the RAW sums b[g] = sum w z (v[g] - v0[g]) and wsum = sum w (iq_kshap_moment_wide: float64 in
    ``kshap_accum``'s order, for R <= 64 its bits; bitwise repeatable)."""
    lib = _lib.load()
    r = kshap_regions_wide(num_regions)
    kp = wide_keep(keep, r)
    m = keep.shape[0]
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    if weights is not None:
        _shape(weights, "weights", m)
    dev = keep.device
    nbytes = lib.iq_kshap_scratch_bytes_wide(m, r, g)
    scratch = _kshap_scratch("kshap_moment_wide", nbytes, m, r, g, dev)
    b = torch.empty((g, r), dtype=torch.float64, device=dev)
    wsum = torch.empty((1,), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_moment_wide(kp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"),
                                        _opt(weights, torch.float64, "weights"), m, r, g, _p(b), _p(wsum), _p(scratch), nbytes, _stream()), "iq_kshap_moment_wide")
    return b, wsum


def kshap_phi_analytic(b, wsum, delta):
    """b (G,R) f64 and wsum (1,) f64 RAW as ``kshap_moment_wide`` returns them, delta (G,) f64 -> phi (G,R) f64 =
    2 H_{R-1} (b / wsum - mean(b / wsum)) + delta / R, the regression under the analytic Gram matrix in closed form
    (iq_kshap_phi_analytic: sum(phi[g]) = delta[g]; no singular case, nothing is read back)."""
    lib = _lib.load()
    g, r = _shape(b, "b", None, None)
    r = kshap_regions_wide(r)
    _shape(wsum, "wsum", 1)
    _shape(delta, "delta", g)
    phi = torch.empty((g, r), dtype=torch.float64, device=b.device)
    _lib.check(lib.iq_kshap_phi_analytic(_dev(b, torch.float64, "b"), _dev(wsum, torch.float64, "wsum"),
                                         _dev(delta, torch.float64, "delta"), _p(phi), r, g, _stream()), "iq_kshap_phi_analytic")
    return phi


def kshap_pairs(keep, v, v0, delta, r, weights=None):
    """keep (M,) int64-typed narrow rows (r <= 64) or (M,W) wide rows, v (G,M) f32 rewards of G games on those rows, v0 and delta
    (G,) f64, weights (M,) f64 or None (all 1) -> (G,r,r) f64: the SHAP-IQ estimate of the pairwise Shapley interaction index of
    every pair of regions (iq_kshap_pairs: float64, the product on the f64 matrix pipe, a fixed order, bitwise repeatable; the
    diagonal is 0, the matrix symmetric bit for bit).  One entry for both row formats: a narrow row is a wide row of one word."""
    lib = _lib.load()
    r = kshap_regions_wide(r)
    kp, m = _sampled_rows(keep, r)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    _shape(delta, "delta", g)
    if weights is not None:
        _shape(weights, "weights", m)
    dev = keep.device
    nbytes = lib.iq_kshap_pairs_scratch_bytes(m, r, g)
    scratch = _kshap_scratch("kshap_pairs", nbytes, m, r, g, dev)
    coef = _pair_coef(r, dev)
    out = torch.empty((g, r, r), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_pairs(kp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"), _dev(delta, torch.float64, "delta"),
                                  _opt(weights, torch.float64, "weights"), _p(coef), m, r, g, _p(out), _p(scratch), nbytes, _stream()),
               "iq_kshap_pairs")
    return out


def _sampled_rows(keep, r):
    """The keep rows of an entry that takes both row formats -> (pointer argument, M): narrow (M,) rows for r <= 64, or (M,W) wide
    rows."""
    if isinstance(keep, torch.Tensor) and keep.dim() == 1:
        if r > 64:
            raise _lib.IqError("keep must be (M, %d) for %d regions, got %s" % (wide_words(r), r, tuple(keep.shape)))
        return _dev(keep, torch.int64, "keep"), keep.shape[0]
    return wide_keep(keep, r), keep.shape[0]


def _units(what, m, paired):
    """The iid units of M sampled rows (a row, or a row and its complement); IqError below two whole units."""
    if paired and m % 2:
        raise _lib.IqError("%s: %d paired rows are not whole pairs" % (what, m))
    u = m // 2 if paired else m
    if u < 2:
        raise _lib.IqError("%s: a standard error needs at least 2 units, %d rows %s give %d" % (what, m, "paired" if paired else "unpaired", u))
    return u


SE_NEEDS_SAMPLES = "a standard error is the sampling error of drawn rows: enumerated or weighted rows have none"


def kshap_pairs_se(keep, v, v0, delta, r, paired=True, weights=None):
    """``kshap_pairs`` of SAMPLED rows (no weights) with the standard error of every entry -> (out (G,r,r) f64, the bits of
    ``kshap_pairs``; se (G,r,r) f64, symmetric bit for bit with a zero diagonal).  iq_kshap_pairs_se: the second moment of the
    same rows, its product on the f64 matrix pipe over the iid units - a row, or ``paired`` a row and its complement (M even) -
    of which at least 2 are needed.  No further model evaluation.  ``weights`` other than None are refused."""
    if weights is not None:
        raise _lib.IqError("kshap_pairs_se: " + SE_NEEDS_SAMPLES)
    lib = _lib.load()
    r = kshap_regions_wide(r)
    kp, m = _sampled_rows(keep, r)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    _shape(delta, "delta", g)
    _units("kshap_pairs_se", m, paired)
    dev = keep.device
    nbytes = lib.iq_kshap_pairs_se_scratch_bytes(m, r, g, int(bool(paired)))
    scratch = _kshap_scratch("kshap_pairs_se", nbytes, m, r, g, dev)
    coef = _pair_coef(r, dev)
    out = torch.empty((g, r, r), dtype=torch.float64, device=dev)
    se = torch.empty((g, r, r), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_pairs_se(kp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"), _dev(delta, torch.float64, "delta"),
                                     _p(coef), m, r, g, int(bool(paired)), _p(out), _p(se), _p(scratch), nbytes, _stream()),
               "iq_kshap_pairs_se")
    return out, se


def kshap_moment_se(keep, v, v0, r, paired=True, weights=None):
    """SAMPLED rows (no weights), narrow (M,) or wide (M,W) -> (b (G,r) f64, the RAW moment with the bits of ``kshap_moment_wide``;
    var (G,r) f64, the variance of phi under the analytic Gram matrix, phi_i = 2 H (b_i - mean(b)) / M + delta / r, from the second
    moment of the same rows over the iid units (iq_kshap_moment_se_wide).  The standard error is sqrt(max(var, 0)).  ``weights``
    other than None are refused."""
    if weights is not None:
        raise _lib.IqError("kshap_moment_se: " + SE_NEEDS_SAMPLES)
    lib = _lib.load()
    r = kshap_regions_wide(r)
    kp, m = _sampled_rows(keep, r)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    _units("kshap_moment_se", m, paired)
    dev = keep.device
    nbytes = lib.iq_kshap_moment_se_scratch_bytes_wide(m, r, g, int(bool(paired)))
    scratch = _kshap_scratch("kshap_moment_se", nbytes, m, r, g, dev)
    b = torch.empty((g, r), dtype=torch.float64, device=dev)
    var = torch.empty((g, r), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_moment_se_wide(kp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"), m, r, g, int(bool(paired)),
                                           _p(b), _p(var), _p(scratch), nbytes, _stream()), "iq_kshap_moment_se_wide")
    return b, var


# The wrappers of the control-variate entries (below, to ``kshap_pair_shift_terms``) lend the library ZEROED memory: what a call
# returns then cannot depend on an earlier call's bytes whatever a kernel reads, at the price of a memset of at most the 35 MB
# factor beside a fit of milliseconds.  The library itself does not rely on it: tests/test_kshap_paircv_gpu.py hands the same
# calls memory with hostile contents between guard zones and asks for the same bits.
def _terms(t, m, what):
    """The float64 per-row terms of a terms entry, (G,M) -> G."""
    g, _ = _shape(t, what, None, m)
    return g


def kshap_pairs_terms(keep, t, r, weights=None):
    """``kshap_pairs`` on float64 per-row terms t (G,M) in place of (v, v0, delta) -> (G,r,r) f64: (((A + L_i) + L_j) + Q_ij) / W_sum,
    the estimator without its delta / (r-1) term (iq_kshap_pairs_terms; include/iq.h, "Control variates for the all-pairs map").
    Narrow (M,) or wide (M,W) rows; ``weights`` as ``kshap_pairs`` takes them."""
    lib = _lib.load()
    r = kshap_regions_wide(r)
    kp, m = _sampled_rows(keep, r)
    g = _terms(t, m, "t")
    if weights is not None:
        _shape(weights, "weights", m)
    dev = keep.device
    nbytes = lib.iq_kshap_pairs_scratch_bytes(m, r, g)
    scratch = torch.zeros((_kshap_scratch_words("kshap_pairs_terms", nbytes, m, r, g),), dtype=torch.float64, device=dev)
    coef = _pair_coef(r, dev)
    out = torch.zeros((g, r, r), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_pairs_terms(kp, _dev(t, torch.float64, "t"), _opt(weights, torch.float64, "weights"), _p(coef), m, r, g, _p(out), _p(scratch), nbytes, _stream()), "iq_kshap_pairs_terms")
    return out


def kshap_pairs_terms_se(keep, t, r, paired=True, weights=None):
    """``kshap_pairs_se`` on float64 per-row terms t (G,M) of SAMPLED rows -> (out, se), both (G,r,r) f64: out the bits of
    ``kshap_pairs_terms``, se its standard error over the iid units (iq_kshap_pairs_terms_se).  ``weights`` other than None are
    refused."""
    if weights is not None:
        raise _lib.IqError("kshap_pairs_terms_se: " + SE_NEEDS_SAMPLES)
    lib = _lib.load()
    r = kshap_regions_wide(r)
    kp, m = _sampled_rows(keep, r)
    g = _terms(t, m, "t")
    _units("kshap_pairs_terms_se", m, paired)
    dev = keep.device
    nbytes = lib.iq_kshap_pairs_se_scratch_bytes(m, r, g, int(bool(paired)))
    scratch = torch.zeros((_kshap_scratch_words("kshap_pairs_terms_se", nbytes, m, r, g),), dtype=torch.float64, device=dev)
    coef = _pair_coef(r, dev)
    out = torch.zeros((g, r, r), dtype=torch.float64, device=dev)
    se = torch.zeros((g, r, r), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_pairs_terms_se(kp, _dev(t, torch.float64, "t"), _p(coef), m, r, g, int(bool(paired)), _p(out), _p(se),
                                           _p(scratch), nbytes, _stream()), "iq_kshap_pairs_terms_se")
    return out, se


SURROGATE_NEEDS_SHIFT = ("the regression surrogate has R + R (R-1) / 2 unknowns and takes 2 .. %d regions: use control='shift' or "
                         "control='sparse' above" % MAX_KSHAP_REGIONS)


def kshap_pair_features(r):
    """d = r + r (r-1) / 2, the features of the 2-additive surrogate: the singles, then the pairs (i < j) row-major.  IqError
    that names ``shift`` above 64 regions."""
    r = int(r)
    if r > MAX_KSHAP_REGIONS:
        raise _lib.IqError(SURROGATE_NEEDS_SHIFT + ", got %d" % r)
    r = kshap_regions(r)
    return r + r * (r - 1) // 2


def _narrow_rows(keep, what):
    if not isinstance(keep, torch.Tensor) or keep.dim() != 1:
        raise _lib.IqError("%s: keep must be (M,) narrow rows" % what)
    return _dev(keep, torch.int64, "keep"), keep.shape[0]


def kshap_pair_gram(keep, r):
    """keep (M,) int64-typed narrow rows -> (d,d) f64: Gram[a][b] = the number of rows that hold feature a and feature b, exact
    counts (iq_kshap_pair_gram: the d x d x M product on the f64 matrix pipe; bits at or above r are ignored)."""
    lib = _lib.load()
    d = kshap_pair_features(r)
    kp, m = _narrow_rows(keep, "kshap_pair_gram")
    if not 1 <= m <= 1 << 30:
        raise _lib.IqError("kshap_pair_gram: M=%d rows is out of range" % m)
    gram = torch.zeros((d, d), dtype=torch.float64, device=keep.device)
    _lib.check(lib.iq_kshap_pair_gram(kp, m, int(r), _p(gram), _stream()), "iq_kshap_pair_gram")
    return gram


def kshap_pair_fit(gram, keep, v, v0, delta, r, ridge, solves=False):
    """gram (d,d) of ``kshap_pair_gram`` on the same rows, keep (M,), v (G,M) f32, v0 and delta (G,) f64, ridge >= 0 -> beta (G,d)
    f64: the ridge regression of the rewards on the features under sum(beta[g]) = delta[g] (iq_kshap_pair_fit: blocked float64
    Cholesky of gram + ridge I, one factor for all games).  ``solves``: -> (beta, (G+1,d) f64: rows 0 .. G-1 the unconstrained
    solutions beta_u, row G the solution w for the ones vector).  KshapSingular when a pivot fails (a status word read back)."""
    lib = _lib.load()
    d = kshap_pair_features(r)
    kp, m = _narrow_rows(keep, "kshap_pair_fit")
    _shape(gram, "gram", d, d)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    _shape(delta, "delta", g)
    ridge = float(ridge)
    if not ridge >= 0.0:
        raise _lib.IqError("kshap_pair_fit: ridge must be a number >= 0, got %r" % ridge)
    dev = keep.device
    nbytes = lib.iq_kshap_pair_fit_scratch_bytes(m, int(r), g)
    scratch = torch.zeros((_kshap_scratch_words("kshap_pair_fit", nbytes, m, int(r), g),), dtype=torch.float64, device=dev)
    beta = torch.zeros((g, d), dtype=torch.float64, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    both = torch.zeros((g + 1, d), dtype=torch.float64, device=dev) if solves else None
    _lib.check(lib.iq_kshap_pair_fit(_dev(gram, torch.float64, "gram"), kp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"),
                                     _dev(delta, torch.float64, "delta"), ridge, m, int(r), g, _p(beta), _p(both), _p(status), _p(scratch),
                                     nbytes, _stream()), "iq_kshap_pair_fit")
    if int(status.item()):
        raise KshapSingular("the rows do not determine the 2-additive surrogate (%d rows, %d unknowns, ridge %g): draw more samples "
                            "or use a ridge > 0" % (m, d, ridge))
    return (beta, both) if solves else beta


def kshap_pair_surrogate(keep, beta, r, v=None, v0=None):
    """keep (M,), beta (G,d) f64 -> g (G,M) f64, g[g][m] = the sum of beta[g] over the features row m holds, in index order
    (iq_kshap_pair_surrogate).  With v (G,M) f32 and v0 (G,) f64: -> (g, t), t = ((double)v - v0) - g, the residual terms."""
    lib = _lib.load()
    d = kshap_pair_features(r)
    kp, m = _narrow_rows(keep, "kshap_pair_surrogate")
    g, _ = _shape(beta, "beta", None, d)
    if not 1 <= m <= 1 << 30:
        raise _lib.IqError("kshap_pair_surrogate: M=%d rows is out of range" % m)
    dev = keep.device
    out = torch.zeros((g, m), dtype=torch.float64, device=dev)
    t = None
    if v is not None:
        _shape(v, "v", g, m)
        _shape(v0, "v0", g)
        t = torch.zeros((g, m), dtype=torch.float64, device=dev)
    _lib.check(lib.iq_kshap_pair_surrogate(kp, _dev(beta, torch.float64, "beta"), _opt(v if t is not None else None, torch.float32, "v"),
                                           _opt(v0 if t is not None else None, torch.float64, "v0"), m, int(r), g, _p(out), _p(t),
                                           _stream()), "iq_kshap_pair_surrogate")
    return out if t is None else (out, t)


def kshap_pair_shift_terms(keep, v, v0, delta, r):
    """Narrow (M,) or wide (M,W) rows, v (G,M) f32, v0 and delta (G,) f64 -> t (G,M) f64 = ((double)v - v0) - delta s / r, s the
    row's size: the rewards less the additive game that spreads delta evenly (iq_kshap_pair_shift_terms)."""
    lib = _lib.load()
    r = kshap_regions_wide(r)
    kp, m = _sampled_rows(keep, r)
    g, _ = _shape(v, "v", None, m)
    _shape(v0, "v0", g)
    _shape(delta, "delta", g)
    if not 1 <= m <= 1 << 30:
        raise _lib.IqError("kshap_pair_shift_terms: M=%d rows is out of range" % m)
    t = torch.zeros((g, m), dtype=torch.float64, device=keep.device)
    _lib.check(lib.iq_kshap_pair_shift_terms(kp, _dev(v, torch.float32, "v"), _dev(v0, torch.float64, "v0"),
                                             _dev(delta, torch.float64, "delta"), m, r, g, _p(t), _stream()), "iq_kshap_pair_shift_terms")
    return t


def kshap_draw_counter(seed, stream, first, count, r, cdf=None, paired=True, device="cuda"):
    """The counter-based draw of samples ``first .. first + count - 1`` of one cloud (iq_kshap_draw_counter: Philox4x32-10 keyed by
    (seed, stream), each sample a pure function of (seed, stream, index, r)) -> (keep (2 count or count, W) int64-typed wide rows,
    every set followed by its complement within the R bits when ``paired``; sizes (count,) int32), both on ``device``.  ``cdf``:
    (r-1,) float64 table of P(size <= k + 1), ndarray or device tensor; None: ``kernelshap._size_cdf(r)``.  One launch."""
    lib = _lib.load()
    r = kshap_regions_wide(r)
    first, count = int(first), int(count)
    if count < 0 or count > 1 << 29 or first < 0 or first + count > 1 << 62:
        raise _lib.IqError("kshap_draw_counter: first=%d, count=%d (0 <= count <= 2^29, 0 <= first, first + count <= 2^62)" % (first, count))
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.IqError("kshap_draw_counter: device must be a CUDA/HIP device (the HIP path has no CPU fallback)")
    if cdf is None:
        from . import kernelshap
        cdf = kernelshap._size_cdf(r)
    if isinstance(cdf, np.ndarray):
        cdf = torch.from_numpy(np.ascontiguousarray(cdf, dtype=np.float64)).to(device)
    _shape(cdf, "cdf", r - 1)
    keep = torch.empty((2 * count if paired else count, wide_words(r)), dtype=torch.int64, device=cdf.device)
    sizes = torch.empty((count,), dtype=torch.int32, device=cdf.device)
    _lib.check(lib.iq_kshap_draw_counter(int(seed) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF, first, count, r, _dev(cdf, torch.float64, "cdf"),
                                         int(bool(paired)), _p(keep), _p(sizes), _stream()), "iq_kshap_draw_counter")
    return keep, sizes


def fps(xyz, npoint):
    """xyz (B,N,3) f32 -> (B,npoint) i32."""
    lib = _lib.load()
    b, n, _ = xyz.shape
    out = torch.empty((b, npoint), dtype=torch.int32, device=xyz.device)
    _lib.check(lib.iq_fps(_dev(xyz, torch.float32, "xyz"), _p(out), b, n, npoint, _stream()), "iq_fps")
    return out


def ball_query(xyz, new_xyz, radius, nsample):
    """xyz (B,N,3), new_xyz (B,S,3) f32 -> (B,S,nsample) i32 (models/pointnet2.py:70-91)."""
    lib = _lib.load()
    b, n, _ = xyz.shape
    s = new_xyz.shape[1]
    out = torch.empty((b, s, nsample), dtype=torch.int32, device=xyz.device)
    _lib.check(lib.iq_ball_query(_dev(xyz, torch.float32, "xyz"), _dev(new_xyz, torch.float32, "new_xyz"),
                                 ctypes.c_float(radius), nsample, _p(out), b, n, s, _stream()), "iq_ball_query")
    return out


def knn(x, k=20):
    """x (B,N,C) row-major f32, C in {3,64,128} -> (B,N,k) i32 neighbour sets (models/dgcnn.py:12-18)."""
    lib = _lib.load()
    b, n, c = x.shape
    out = torch.empty((b, n, k), dtype=torch.int32, device=x.device)
    # The size formula restates iq_knn's own (csrc/iq_dgcnn.hip: the arrays it carves from tmp, B*N*84 + 16*B + 8192 bytes, and
    # B*N*C*6 more for the bf16x3 operand image of C = 64 / 128, which it builds only when that room is there); the slack is 16384
    # here so that the 256-byte rounding in front of the image cannot cost it.  tests/test_workspace_contents_gpu.py runs the call
    # in exactly this many bytes between guard zones, so the two formulas cannot drift apart unnoticed.
    tmp = torch.empty((b * n * (84 + (6 * c if c in (64, 128) else 0)) + 16 * b + 16384,), dtype=torch.uint8, device=x.device)
    _lib.check(lib.iq_knn(_dev(x, torch.float32, "x"), _p(out), _p(tmp), tmp.numel(), b, n, c, k, _stream()), "iq_knn")
    return out


def _shape(t, what, *dims):
    """The shape of tensor ``t``; IqError unless it has len(dims) dimensions and matches every dims entry that is not None."""
    if not isinstance(t, torch.Tensor) or t.dim() != len(dims) or any(d is not None and t.shape[i] != d for i, d in enumerate(dims)):
        want = "(%s)" % ",".join("*" if d is None else str(d) for d in dims)
        raise _lib.IqError("%s must be %s, got %s" % (what, want, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
    return tuple(t.shape)


_INDEX_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def _valid_idx(idx, n, what):
    """Caller indices -> int32 device tensor, validated to lie in [0, n) (IqError otherwise) before any kernel reads them.
    A wider index is clamped to [-1, n] before the cast, so a value outside the int32 range cannot wrap into [0, n)."""
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda:
        raise _lib.IqError("%s must be a CUDA/HIP tensor (the HIP path has no CPU fallback)" % what)
    if idx.dtype not in _INDEX_DTYPES:
        raise _lib.IqError("%s must be an integer tensor, got %s" % (what, idx.dtype))
    t = (idx.clamp(-1, n) if idx.dtype == torch.int64 else idx).to(dtype=torch.int32).contiguous()
    check_index_range(t, 0, n, what)
    return t


def index_points(points, idx):
    """points (B,N,C) f32, idx (B,...) integer -> (B,...,C) f32: points[b, idx[b,...], :] (models/pointnet2.py:27-43)."""
    lib = _lib.load()
    b, n, c = _shape(points, "points", None, None, None)
    if not isinstance(idx, torch.Tensor) or idx.dim() < 1 or idx.shape[0] != b:
        raise _lib.IqError("idx must be (%d,...), got %s" % (b, tuple(idx.shape) if isinstance(idx, torch.Tensor) else type(idx).__name__))
    t = _valid_idx(idx, n, "idx")
    out = torch.empty(tuple(t.shape) + (c,), dtype=torch.float32, device=points.device)
    m = t[0].numel() if b else 0
    _lib.check(lib.iq_index_points(_dev(points, torch.float32, "points"), _p(t), _p(out), b, n, m, c, _stream()), "iq_index_points")
    return out


def group_points(xyz, points=None, new_xyz=None, idx=None, xyz_first=True):
    """xyz (B,N,3), points (B,N,D) or None, new_xyz (B,S,3) or None, idx (B,S,K) integer or None -> (B,S,K,3+D) f32 rows
    [xyz[idx] - new_xyz, points[idx]] (xyz_first) or [points[idx], xyz[idx] - new_xyz]; new_xyz None: nothing subtracted;
    idx None: all N points (S = 1, K = N) (models/pointnet2.py:93-137, 222-230; models/pointconv.py:117-197)."""
    lib = _lib.load()
    b, n, _ = _shape(xyz, "xyz", None, None, 3)
    d = _shape(points, "points", b, n, None)[2] if points is not None else 0
    if idx is not None:
        _, s, k = _shape(idx, "idx", b, None, None)
    else:
        s, k = 1, n
    if new_xyz is not None:
        _shape(new_xyz, "new_xyz", b, s, 3)
    t = _valid_idx(idx, n, "idx") if idx is not None else None
    out = torch.empty((b, s, k, 3 + d), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.iq_group_points(_dev(xyz, torch.float32, "xyz"),
                                   _dev(points, torch.float32, "points") if points is not None else ctypes.c_void_p(0),
                                   _dev(new_xyz, torch.float32, "new_xyz") if new_xyz is not None else ctypes.c_void_p(0),
                                   _p(t), _p(out), int(bool(xyz_first)), b, n, s, k, d, _stream()), "iq_group_points")
    return out


def edgeconv_gather(x, idx, channel_first=True):
    """x (B,C,N) (channel_first) or (B,N,C) f32, idx (B,N,k) integer -> (B,2C,N,k) f32 [x_j - x_i ; x_i]
    (models/dgcnn.py:21-47 with idx given)."""
    lib = _lib.load()
    if channel_first:
        b, c, n = _shape(x, "x", None, None, None)
    else:
        b, n, c = _shape(x, "x", None, None, None)
    k = _shape(idx, "idx", b, n, None)[2]
    t = _valid_idx(idx, n, "idx")
    out = torch.empty((b, 2 * c, n, k), dtype=torch.float32, device=x.device)
    _lib.check(lib.iq_edgeconv_gather(_dev(x, torch.float32, "x"), _p(t), _p(out), int(bool(channel_first)), b, n, c, k, _stream()),
               "iq_edgeconv_gather")
    return out


def knn_point(xyz, new_xyz, k):
    """xyz (B,N,3), new_xyz (B,S,3) f32 -> (B,S,k) i32: the k nearest points by square_distance, nearest first, ties to the
    lower index (models/pointconv.py:103-114); N <= 4096, k <= min(N, 128)."""
    lib = _lib.load()
    b, n, _ = _shape(xyz, "xyz", None, None, 3)
    s = _shape(new_xyz, "new_xyz", b, None, 3)[1]
    out = torch.empty((b, s, k), dtype=torch.int32, device=xyz.device)
    _lib.check(lib.iq_knn_point(_dev(xyz, torch.float32, "xyz"), _dev(new_xyz, torch.float32, "new_xyz"), int(k), _p(out),
                                ctypes.c_void_p(0), 0, b, n, s, _stream()), "iq_knn_point")
    return out


def sort_neighbours(q, keys, idx):
    """q (B,S,C), keys (B,N,C) f32, idx (B,S,k) i32 -> idx reordered in place nearest first by the distance of
    models/dgcnn.py:13-15 in float32 (ties to the lower index): the order of knn's topk(sorted=True).  Returns idx."""
    lib = _lib.load()
    b, n, c = _shape(keys, "keys", None, None, None)
    s = _shape(q, "q", b, None, c)[1]
    k = _shape(idx, "idx", b, s, None)[2]
    _dev(idx, torch.int32, "idx")
    check_index_range(idx, 0, n, "idx")
    _lib.check(lib.iq_sort_neighbours(_dev(q, torch.float32, "q"), _dev(keys, torch.float32, "keys"), _p(idx), b, n, s, c, k,
                                      _stream()), "iq_sort_neighbours")
    return idx


def density(xyz, bandwidth):
    """xyz (B,N,3) f32 -> (B,N) f32 Gaussian kernel density (models/pointconv.py:199-209, compute_density)."""
    lib = _lib.load()
    b, n, _ = _shape(xyz, "xyz", None, None, 3)
    out = torch.empty((b, n), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.iq_density(_dev(xyz, torch.float32, "xyz"), float(bandwidth), _p(out), b, n, _stream()), "iq_density")
    return out


def pointconv_inverse_density(xyz, bandwidth):
    """xyz (B,N,3) f32, N <= 3072 -> (B,N) f32: the inverse density as the fused PointConv path computes it in front of its
    DensityNets (iq_pointconv_inverse_density); 1 / ``density`` up to that kernel's rounding."""
    lib = _lib.load()
    b, n, _ = _shape(xyz, "xyz", None, None, 3)
    out = torch.empty((b, n), dtype=torch.float32, device=xyz.device)
    _lib.check(lib.iq_pointconv_inverse_density(_dev(xyz, torch.float32, "xyz"), float(bandwidth), _p(out), b, n, _stream()),
               "iq_pointconv_inverse_density")
    return out


SMOOTHNESS_MODES = ("linearity", "planarity", "scattering")


def smoothness_enum(cloud, region_id, num_regions, mode, objective, step=1e-3, enum_step=0.05, var_threshold=0.003,
                    dist_threshold=0.03, stop_ratio=0.5, epochs=50, max_iteration=100, origin=None, project_to_bound=False,
                    entry="iq_smoothness_enum"):
    """final_smoothness_center_enum_all.py:183-242,303-335 for all regions and epochs in one launch.
    cloud (N,3) f32, region_id (N,) i32 -> dict(data (E,N,3) f32, smoothness (E,R) f32, var (E,R,3) f32,
    orig (R,4) f32, stop_epoch (R,) i32); see include/iq.h.  ``origin`` (N,3): restart from a deformed ``cloud``.
    Every region id must lie in [0, num_regions): an IqError otherwise (check_index_range), before anything is launched."""
    lib = _lib.load()
    n, r, e = cloud.shape[0], int(num_regions), int(epochs)
    dev = cloud.device
    _dev(region_id, torch.int32, "region_id")
    check_index_range(region_id, 0, r, "region_id")
    out = {"data": torch.empty((e, n, 3), dtype=torch.float32, device=dev),
           "smoothness": torch.empty((e, r), dtype=torch.float32, device=dev),
           "var": torch.empty((e, r, 3), dtype=torch.float32, device=dev),
           "orig": torch.empty((r, 4), dtype=torch.float32, device=dev),
           "stop_epoch": torch.empty((r,), dtype=torch.int32, device=dev)}
    prm = _lib.SmoothnessParams(step, enum_step, var_threshold, dist_threshold, stop_ratio, e, int(max_iteration), int(bool(project_to_bound)), 0)
    if mode not in SMOOTHNESS_MODES or objective not in ("inc", "dec"):
        raise _lib.IqError("smoothness_enum: mode %r / objective %r" % (mode, objective))
    org = _dev(origin, torch.float32, "origin") if origin is not None else ctypes.c_void_p(0)
    _lib.check(getattr(lib, entry)(_dev(cloud, torch.float32, "cloud"), org, _dev(region_id, torch.int32, "region_id"), n, r,
                                   SMOOTHNESS_MODES.index(mode), 1 if objective == "inc" else -1, ctypes.byref(prm),
                                   _p(out["data"]), _p(out["smoothness"]), _p(out["var"]), _p(out["orig"]),
                                   _p(out["stop_epoch"]), _stream()), entry)
    return out


MAX_SMOOTHNESS_POINTS = 1024    # iq_smoothness_enum, iq_smoothness_enum_wide: a region's points live in the kernel's LDS arrays


def smoothness_enum_wide(cloud, region_id, num_regions, mode, objective, **kw):
    """``smoothness_enum`` for a wide game, 1 <= num_regions <= MAX_WIDE_REGIONS (iq_smoothness_enum_wide: the same kernel, one
    wave per region; for num_regions <= 64 the same bits).  The cloud keeps the narrow limit of MAX_SMOOTHNESS_POINTS points.
    A region without points leaves no trace in ``data``: every point of the cloud belongs to a region that writes it."""
    wide_words(num_regions)
    if not 1 <= cloud.shape[0] <= MAX_SMOOTHNESS_POINTS:
        raise _lib.IqError("smoothness_enum_wide: N=%d points, the enumeration takes 1 .. %d" % (cloud.shape[0], MAX_SMOOTHNESS_POINTS))
    return smoothness_enum(cloud, region_id, num_regions, mode, objective, entry="iq_smoothness_enum_wide", **kw)


class PackedLinear:
    """A (cout,cin) weight + bias in the library's MFMA fragment order (iq_pack_weight) on the device.  bf3: also as three bf16
    terms (iq_pack_weight_bf3) - a layer with cout % 256 == 0 (or 64: all but the last 64 columns) and cin >= 32 then takes its products on the bf16 matrix pipe,
    float32-exact (include/iq.h: iq_dense_layer.w_bf3)."""

    def __init__(self, weight, bias, device, bf3=False):
        from .engine import Packer      # engine.py imports this module
        self.cout, self.cin = np.shape(weight)
        self._packer = Packer(device)   # keeps the device tensors alive
        self.struct = self._packer.dense(np.asarray(weight), bias, bf3=bf3)


def linear(x, layer, act=0):
    """x (M,cin) f32 -> act(x W^T + b) (M,cout); act 0 none, 1 ReLU, 2 LeakyReLU(0.2)."""
    lib = _lib.load()
    m = x.shape[0]
    out = torch.empty((m, layer.cout), dtype=torch.float32, device=x.device)
    _lib.check(lib.iq_linear(_dev(x, torch.float32, "x"), x.shape[1], ctypes.byref(layer.struct), _p(out), layer.cout, m, int(act),
                             _stream()), "iq_linear")
    return out


def pointnet_reps(keep, cloud_of=None, num_regions=64, nclouds=1, scratch_bytes=None):
    """Diagnostic (iq_debug_pointnet_reps; no product path calls it): keep (B,) int64-typed masks, cloud_of (B,) int32 or None
    -> (B,) int32, for every coalition the lowest item of the batch on the same cloud with the same kept regions - the items the
    PointNet chains compute; the others copy their rows.  ``scratch_bytes``: lend the table that much instead of what it needs."""
    lib = _lib.load()
    b = keep.shape[0]
    rep = torch.empty((b,), dtype=torch.int32, device=keep.device)
    nbytes = 16 * max(b, 1) if scratch_bytes is None else int(scratch_bytes)
    scratch = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=keep.device)
    _lib.check(lib.iq_debug_pointnet_reps(_dev(keep, torch.int64, "keep"), _dev(cloud_of, torch.int32, "cloud_of") if cloud_of is not None
                                          else ctypes.c_void_p(0), b, int(nclouds), int(num_regions), _p(rep), _p(scratch), nbytes,
                                          _stream()), "iq_debug_pointnet_reps")
    return rep


def pointnet_slots(keep, cloud_of=None, num_regions=64, nclouds=1):
    """Diagnostic (iq_debug_pointnet_slots; no product path calls it): the slots the PointNet forward gives the distinct coalitions
    of a batch.  keep (B,) int64-typed masks, cloud_of (B,) int32 or None -> (slot_of (B,), item_u (U,), cloud_u (U,) or None, U):
    slot_of[i] = the rank of item i's representative among the representatives, item_u / cloud_u = the item and the cloud in
    every slot."""
    lib = _lib.load()
    b = keep.shape[0]
    out = torch.full((3 * b + 1,), -1, dtype=torch.int32, device=keep.device)
    nbytes = 24 * max(b, 1) + 8
    scratch = torch.empty((nbytes,), dtype=torch.uint8, device=keep.device)
    _lib.check(lib.iq_debug_pointnet_slots(_dev(keep, torch.int64, "keep"), _dev(cloud_of, torch.int32, "cloud_of") if cloud_of is not None
                                           else ctypes.c_void_p(0), b, int(nclouds), int(num_regions), _p(out), _p(scratch), nbytes,
                                           _stream()), "iq_debug_pointnet_slots")
    u = int(out[3 * b].item()) if b else 0
    return out[:b], out[b:b + u], (out[2 * b:2 * b + u] if cloud_of is not None else None), u
