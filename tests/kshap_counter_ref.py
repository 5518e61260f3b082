"""NumPy restatement of the counter-based draw of a wide game's rows (include/iq.h, "The COUNTER-BASED draw"), written
from the contract and sharing no code with the kernel or with interpret_quality_amd/wide_kernelshap.py:

* Philox4x32-10, vectorised over blocks in uint64 arithmetic;
* the size of sample m from the block with counter (m_lo, m_hi, 0, 1) by NumPy's random_sample construction and searchsorted;
* the members of sample m as the s smallest composite keys (key << 10) | region by argsort.

It is the reference of tests/test_kshap_counter_cpu.py and tests/test_kshap_counter_gpu.py."""
import numpy as np

import kernelshap_ref as narrow

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter (..., 4) and key (..., 2) of 32-bit words (broadcast against each other) -> (..., 4) uint64 holding 32-bit words."""
    counter, key = np.asarray(counter, dtype=np.uint64) & MASK, np.asarray(key, dtype=np.uint64) & MASK
    shape = np.broadcast_shapes(counter.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(counter[..., i], shape) for i in range(4)]
    k0, k1 = np.broadcast_to(key[..., 0], shape), np.broadcast_to(key[..., 1], shape)
    for rnd in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                              # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _32) ^ c[1] ^ k0, p1 & MASK, (p0 >> _32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=-1)


def _key(seed, stream):
    return np.array([int(seed) & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF], dtype=np.uint64)


def _index_words(first, count):
    """Sample indices first .. first + count - 1 as (m_lo, m_hi) uint64 columns (Python integers: no overflow on the way)."""
    m = [int(first) + j for j in range(int(count))]
    return (np.array([x & 0xFFFFFFFF for x in m], dtype=np.uint64).reshape(-1), np.array([x >> 32 for x in m], dtype=np.uint64).reshape(-1))


def uniforms(seed, stream, first, count):
    """u of samples first .. first + count - 1 -> (count,) float64 in [0, 1)."""
    lo, hi = _index_words(first, count)
    w = philox4x32_10(np.stack([lo, hi, np.zeros_like(lo), np.ones_like(lo)], axis=-1), _key(seed, stream))
    return ((w[:, 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[:, 1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def sizes(seed, stream, first, count, r, cdf=None):
    """-> (count,) int32 sizes in 1 .. r-1."""
    cdf = narrow.size_cdf(r) if cdf is None else np.asarray(cdf, dtype=np.float64)
    assert cdf.shape == (r - 1,)
    u = uniforms(seed, stream, first, count)
    return np.minimum(r - 1, 1 + np.searchsorted(cdf, u, side="right")).astype(np.int32)


def region_keys(seed, stream, first, count, r):
    """-> (count, r) uint64: the 32-bit key of every region of every sample."""
    lo, hi = _index_words(first, count)
    nblocks = (r + 3) // 4
    blk = np.arange(nblocks, dtype=np.uint64)
    counter = np.stack([np.broadcast_to(lo[:, None], (len(lo), nblocks)), np.broadcast_to(hi[:, None], (len(lo), nblocks)),
                        np.broadcast_to(blk[None], (len(lo), nblocks)), np.zeros((len(lo), nblocks), dtype=np.uint64)], axis=-1)
    return philox4x32_10(counter, _key(seed, stream)).reshape(len(lo), 4 * nblocks)[:, :r]


def composite_keys(seed, stream, first, count, r):
    """-> (count, r) uint64: (key << 10) | region."""
    return (region_keys(seed, stream, first, count, r) << np.uint64(10)) | np.arange(r, dtype=np.uint64)[None]


def pack(z):
    """(M, R) 0/1 -> (M, W) uint64 rows, bit (i & 63) of word (i >> 6) = column i."""
    z = np.asarray(z, dtype=np.uint8)
    m, r = z.shape
    w = (r + 63) // 64
    padded = np.zeros((m, 64 * w), dtype=np.uint8)
    padded[:, :r] = z
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u8").astype(np.uint64).reshape(m, w)


def rows(seed, stream, first, count, r, paired=True, cdf=None):
    """-> ((count or 2 count, W) uint64 rows, (count,) int32 sizes): sample m's set, paired: followed by its complement."""
    s = sizes(seed, stream, first, count, r, cdf)
    order = np.argsort(composite_keys(seed, stream, first, count, r), axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(r)[None], order.shape), axis=1)
    z = (rank < s[:, None]).astype(np.uint8)
    if not paired:
        return pack(z), s
    both = np.empty((2 * int(count), r), dtype=np.uint8)
    both[0::2], both[1::2] = z, 1 - z
    return pack(both), s
