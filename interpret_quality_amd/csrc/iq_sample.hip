// Coalition sampling on the device (SURVEY.md §8 a4 / K1-K2 inputs; north star: "coalition sampling").
//
// * mt_permutations_kernel: the reference draws its region permutations from NumPy's GLOBAL legacy generator
//   (final_shapley_value.py:59-72: np.random.permutation per sample after tools/final_util.py:113-120 seeded it).  That
//   stream is MT19937 + Fisher-Yates from the back with masked rejection sampling (numpy/random: RandomState.shuffle ->
//   _shuffle_raw -> random_interval).  The kernel continues it ON THE DEVICE from a given generator state (624 key words +
//   position) and hands the advanced state back, so the permutations - and everything the host draws afterwards - are
//   bit-identical to the reference's for the same seed.
//   The stream looks sequential - a rejected draw shifts every later one - but where a permutation STARTS in the word stream
//   is all that couples two permutations, and how many words a permutation consumes is a function of its start offset alone.
//   One workgroup of 1024 lanes therefore works in batches of 8 x 624 words: (1) regenerate and temper the words (three
//   element-parallel thirds per 624-word block); (2) every lane simulates the draws of a permutation starting at EVERY word
//   offset of the batch (no swaps, just the rejection loop) -> next[o] = offset behind it; (3) one lane follows
//   next[] from the current position: the start offsets of the real permutations; (4) one lane per real permutation replays
//   its draws with the swaps and writes the row.  1000 permutations of 32 regions take 0.40 ms (profiles/serial_kernels_profile.txt)
//   instead of the 4 ms of a draw-by-draw scalar loop (which is what the first version of this kernel was).  By instruction count
//   step (2) dominates, and it and step (4) are parallel over the whole call, not only over a batch: iq_sample_permutations_ws
//   (below) spreads them over the GPU and takes 0.075 ms for the same draw; this kernel then only finishes what is left.
// * prefix_keep_kernel / context_keep_kernel: permutations -> the R+1 prefix coalitions of each
//   (tools/final_common.py:56-60), (pair, context) -> the 4 coalitions of each context
//   (final_point_binary_interaction_logits.py:45-52), as uint64 region bit masks, the form every coalition entry point
//   of this library takes.
#include "iq_common.h"

namespace {

constexpr int kMtN = 624, kMtM = 397;
constexpr int kMtBlocks = 8;                      // 624-word blocks per batch
constexpr int kMtWords = kMtBlocks * kMtN;        // 4992 words per batch
constexpr int kMtThreads = 1024;
constexpr int kMtMaxStarts = kMtWords + 1;        // (R = 2 draws at least one word per permutation)
constexpr unsigned kMtInvalid = 0xffffu;
constexpr unsigned kMtPoison = 0x7fffffffu;        // position word of a state no draw may continue from (a failed / refused call)

__device__ inline uint32_t mt_mix(uint32_t hi, uint32_t lo, uint32_t far) {
    const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

__device__ inline uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// smallest 2^b - 1 >= i (i >= 1): random_interval's mask
__device__ inline uint32_t interval_mask(int i) { return (2u << (31 - __clz(i))) - 1u; }

// Offset behind a permutation of R regions whose draws start at word offset o of a stream of `limit` words (no swaps, just the
// rejection loop), -1 if it runs out of the stream.  word(k): tempered word k, k < limit.  The words a simulation consumes are
// consecutive whatever it accepts, so four are read ahead per trip and the four decisions run branch-free: one flat loop
// (nested accept / reject loops diverge lane by lane and wait on every read: 5x slower)
template <class Word>
__device__ inline int perm_end(Word word, int limit, int R, int o) {
    int i = R - 1, p = o;
    bool fail = false;
    while (i >= 1) {
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = word(min(p + u, limit - 1));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool active = i >= 1, inb = p < limit;
            fail = fail || (active && !inb);
            const bool acc = active && inb && (w[u] & interval_mask(max(i, 1))) <= (uint32_t)i;
            p += (active && inb) ? 1 : 0;
            i -= acc ? 1 : 0;
        }
        if (fail) i = 0;
    }
    return fail ? -1 : p;
}

// What depends on the region count, as parameters of ONE body per kernel below.  Row: the element of a permutation row in LDS
// (a byte cannot hold an id above 255).  kNextTail: words behind its 256 offsets that a workgroup of mt_next_kernel keeps in LDS,
// kReplayTail: words behind a segment that mt_replay_kernel keeps - a permutation of 1024 regions draws about 1413 words, one of
// 64 about 90; beyond the tail the words come from memory, so the tails are a matter of speed only.  The 16-bit offsets of the
// narrow kernels (nxt[] and start[] of a batch of 4992 words, start[] relative to a segment of 4096) count words, not regions:
// they fit at any R.
struct MtNarrow {
    using Row = uint8_t;
    static constexpr int kNextTail = 256, kReplayTail = 1024;
    static int next_tail(int) { return kNextTail; }
};
struct MtWide {
    using Row = uint16_t;
    static constexpr int kNextTail = 2048, kReplayTail = 2048;
    // 1.39 R words on average at worst (R = 2^k), sigma about sqrt(R): 1.5 R + 64 covers all but a rare lane
    static int next_tail(int R) { const int t = ((3 * R / 2 + 64) + 255) / 256 * 256; return t < kNextTail ? t : kNextTail; }
};

// The same draws with the swaps: row (R entries) becomes the permutation that starts at offset p; its words all lie below `limit`
template <class Word, class Row>
__device__ inline void perm_replay(Word word, int limit, int R, int p, Row* row) {
    for (int j = 0; j < R; ++j) row[j] = (Row)j;
    int i = R - 1;
    while (i >= 1) {
        uint32_t w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = word(min(p + u, limit - 1));
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i >= 1) {
                const uint32_t v = w[u] & interval_mask(i);
                ++p;
                if (v <= (uint32_t)i) {
                    const Row a_i = row[i], a_v = row[v];
                    row[i] = a_v;
                    row[v] = a_i;
                    --i;
                }
            }
        }
    }
}

// The whole draw on one workgroup.  iq_sample_permutations launches it alone (keys == nullptr: the state comes from `state`).  The
// workspace route launches it LAST: keys / reached are what the wide kernels below left - reached[0] permutations written,
// reached[1] the word offset behind them in keys[] - and it draws whatever is missing (normally nothing) and hands the state back.
// Of every permutation the first `head` entries are written, rows of `head` (head = R: the whole permutation; 0: the draw only
// advances the state and `orders` is never touched).
template <class Cfg>
__global__ __launch_bounds__(kMtThreads) void mt_permutations_kernel(uint32_t* __restrict__ state, int32_t* __restrict__ orders, int S, int R,
                                                                     int head, const uint32_t* __restrict__ keys,
                                                                     const int* __restrict__ reached, int nblk) {
    using Row = typename Cfg::Row;
    __shared__ uint32_t key[kMtBlocks][kMtN];      // block 0: the carried generator state; block k = twist of block k - 1
    __shared__ uint32_t word[kMtWords];            // tempered outputs of the batch
    __shared__ uint16_t nxt[kMtWords + 1];         // offset behind a permutation that starts at offset o (kMtInvalid: runs out of the batch)
    __shared__ uint16_t start[kMtMaxStarts];       // start offsets of the real permutations of this batch
    __shared__ int ctl[3];                         // permutations found in this batch, position behind the last of them, no-progress flag
    const int tid = threadIdx.x;
    const uint32_t* from = state;
    int pos = (int)state[kMtN];                    // 0..624
    int done = 0;                                  // permutations written so far (uniform)
    if (keys && (unsigned)pos <= (unsigned)kMtN) { // continue behind the wide kernels: the block that holds their offset, as below
        done = reached[0];
        const int cur = reached[1], kb = cur == 0 ? 0 : min((cur - 1) / kMtN, nblk - 1);
        from = keys + (size_t)kb * kMtN;
        pos = cur - kb * kMtN;
    }
    for (int k = tid; k < kMtN; k += kMtThreads) key[0][k] = from[k];
    __syncthreads();
    if ((unsigned)pos > (unsigned)kMtN) {
        // a malformed state (np.random.set_state accepts any position) or one a failed call poisoned: draw nothing, write rows
        // that every range check rejects, keep the state poisoned so that the host sees it (hip_ops.mt_state_to_host raises)
        for (size_t e = tid; e < (size_t)S * head; e += kMtThreads) orders[e] = -1;
        if (tid == 0) state[kMtN] = kMtPoison;
        return;
    }
    while (done < S) {
        // (1) blocks 1..7 by twisting (three dependent thirds, each element-parallel); temper all
        for (int blk = 1; blk < kMtBlocks; ++blk) {
            const uint32_t* o = key[blk - 1];
            uint32_t* n = key[blk];
            if (tid < kMtN - kMtM) n[tid] = mt_mix(o[tid], o[tid + 1], o[tid + kMtM]);
            __syncthreads();
            if (tid < kMtN - kMtM) { const int k = kMtN - kMtM + tid; n[k] = mt_mix(o[k], o[k + 1], n[tid]); }
            __syncthreads();
            if (tid < kMtM - (kMtN - kMtM)) {
                const int k = 2 * (kMtN - kMtM) + tid;
                n[k] = mt_mix(o[k], k + 1 < kMtN ? o[k + 1] : n[0], n[k - (kMtN - kMtM)]);
            }
            __syncthreads();
        }
        for (int k = tid; k < kMtWords; k += kMtThreads) word[k] = mt_temper(key[k / kMtN][k % kMtN]);
        __syncthreads();
        // (2) length of a permutation that would start at offset o, for every o
        const auto lds_word = [&](int k) { return word[k]; };
        for (int o = pos + tid; o <= kMtWords; o += kMtThreads) {
            const int p = perm_end(lds_word, kMtWords, R, o);
            nxt[o] = p < 0 ? (uint16_t)kMtInvalid : (uint16_t)p;
        }
        __syncthreads();
        // (3) the chain of real starts
        if (tid == 0) {
            int cur = pos, n = 0;
            while (done + n < S) {
                const unsigned nx = nxt[cur];
                if (nx == kMtInvalid) break;
                start[n++] = (uint16_t)cur;
                cur = (int)nx;
            }
            ctl[0] = n;
            ctl[1] = cur;
        }
        __syncthreads();
        const int n = ctl[0], cur = ctl[1];
        // (4) replay with the swaps: one lane per permutation, its row in nxt[]'s storage (free once the chain is known), then
        // one coalesced copy to global memory.  n rows of R bytes never exceed that storage (n <= 4992 / (R - 1) + 1); rows of
        // 16-bit entries can, and are then replayed as many at a time as it holds (four of 1024 regions)
        if (head > 0) {
            Row* rows = reinterpret_cast<Row*>(nxt);
            const int cap = (int)(sizeof(nxt) / (R * sizeof(Row)));
            for (int r0 = 0; r0 < n; r0 += cap) {
                const int nr = min(cap, n - r0);
                for (int s = tid; s < nr; s += kMtThreads) perm_replay(lds_word, kMtWords, R, start[r0 + s], rows + s * R);
                __syncthreads();
                int32_t* out = orders + (size_t)(done + r0) * head;
                if (head == R) {
                    for (int e = tid; e < nr * R; e += kMtThreads) out[e] = rows[e];
                } else {
                    for (int e = tid; e < nr * head; e += kMtThreads) { const int s = e / head; out[e] = rows[s * R + (e - s * head)]; }
                }
                if (r0 + cap < n) __syncthreads();
            }
        }
        // carry the state: the block that holds `cur` becomes block 0 (cur == 624 k stays at the END of block k - 1, as NumPy
        // leaves its position at 624 until the next draw)
        const int kb = cur == 0 ? 0 : min((cur - 1) / kMtN, kMtBlocks - 1);
        __syncthreads();
        if (kb > 0) {
            uint32_t carry = tid < kMtN ? key[kb][tid] : 0u;
            __syncthreads();
            if (tid < kMtN) key[0][tid] = carry;
        }
        pos = cur - kb * kMtN;
        done += n;
        __syncthreads();
        if (n == 0 && kb == 0) break;   // no progress is only possible if one permutation needs more than 4368 words (p < 2^-4000)
    }
    for (int k = tid; k < kMtN; k += kMtThreads) state[k] = key[0][k];
    if (done < S) {                     // gave up: the rows not drawn are marked, and so is the state (see the entry check)
        for (size_t e = (size_t)done * head + tid; e < (size_t)S * head; e += kMtThreads) orders[e] = -1;
        pos = (int)kMtPoison;
    }
    if (tid == 0) state[kMtN] = (uint32_t)pos;
}

// ---- the same draw over many workgroups (iq_sample_permutations_ws) ------------------------------------------------------------
// Only the twist is serial.  mt_words_kernel (one workgroup) twists nblk blocks ahead into the workspace; mt_next_kernel (wide)
// simulates a permutation from every word offset; mt_jump_kernel cuts the offsets into segments of kMtSeg and, by pointer jumping
// inside a segment, finds for every offset where the chain of permutations that starts there leaves the segment and after how many
// permutations, so that the chain of REAL starts is one hop per segment instead of one per permutation; mt_replay_kernel (one
// workgroup per segment) takes those hops to its own segment, walks it, replays its permutations with the swaps and writes their
// rows.  How many words S permutations draw is only known afterwards: nblk is an estimate, and mt_permutations_kernel runs last
// and draws what the estimate missed.  iq_sample_permutations_wide (up to 1024 regions, `head` entries of a permutation, skip mode)
// is the same kernels with MtWide for MtNarrow; mt_words_kernel and mt_jump_kernel do not depend on R.
constexpr int kMtSeg = 4096;                       // word offsets per segment
constexpr int kMtSegThreads = 1024;
constexpr int kMtSegPer = kMtSeg / kMtSegThreads + 1;   // offsets per lane (the last segment also holds offset W)
constexpr int kMtCtl = 16;                         // control words in front of the workspace
constexpr uint32_t kMtNone = 0xffffffffu;          // next[]: the permutation runs out of the words

// ctl[0] permutations written, ctl[1] word offset behind them (what mt_permutations_kernel continues from), ctl[2] the offset the
// call starts at, or kMtPoison
__global__ __launch_bounds__(256) void mt_words_kernel(const uint32_t* __restrict__ state, uint32_t* __restrict__ keys,
                                                       int* __restrict__ ctl, int nblk) {
    __shared__ uint32_t key[2][kMtN];
    const int tid = threadIdx.x;
    const int pos = (int)state[kMtN];
    const bool bad = (unsigned)pos > (unsigned)kMtN;   // mt_permutations_kernel marks the rows and the state
    if (tid == 0) { ctl[0] = 0; ctl[1] = bad ? 0 : pos; ctl[2] = bad ? (int)kMtPoison : pos; }
    if (bad) return;
    for (int k = tid; k < kMtN; k += 256) keys[k] = key[0][k] = state[k];
    __syncthreads();
    for (int blk = 1; blk < nblk; ++blk) {
        const uint32_t* o = key[(blk - 1) & 1];
        uint32_t* n = key[blk & 1];
        uint32_t* out = keys + (size_t)blk * kMtN;
        if (tid < kMtN - kMtM) out[tid] = n[tid] = mt_mix(o[tid], o[tid + 1], o[tid + kMtM]);
        __syncthreads();
        if (tid < kMtN - kMtM) { const int k = kMtN - kMtM + tid; out[k] = n[k] = mt_mix(o[k], o[k + 1], n[tid]); }
        __syncthreads();
        if (tid < kMtM - (kMtN - kMtM)) {
            const int k = 2 * (kMtN - kMtM) + tid;
            out[k] = n[k] = mt_mix(o[k], k + 1 < kMtN ? o[k + 1] : n[0], n[k - (kMtN - kMtM)]);
        }
        __syncthreads();
    }
}

// next[o], o = 0..W: the offset behind a permutation that starts at offset o.  A workgroup keeps its 256 offsets' words and the
// `tail` (<= Cfg::kNextTail, a multiple of 256) behind them in LDS - the lanes of a wave start at consecutive offsets and read
// nearly the same words; a permutation that draws more reads the rest from memory.
template <class Cfg>
__global__ __launch_bounds__(256) void mt_next_kernel(const uint32_t* __restrict__ keys, const int* __restrict__ ctl,
                                                      uint32_t* __restrict__ next, int W, int R, int tail) {
    __shared__ uint32_t win[256 + Cfg::kNextTail];
    if (ctl[2] == (int)kMtPoison) return;
    const int base = blockIdx.x * 256, tid = threadIdx.x, held = 256 + tail;
    for (int k = tid; k < held; k += 256) win[k] = base + k < W ? mt_temper(keys[base + k]) : 0u;
    __syncthreads();
    const int o = base + tid;
    if (o > W) return;
    const int p = perm_end([&](int k) { return k >= base && k < base + held ? win[k - base] : mt_temper(keys[k]); }, W, R, o);   // (k < base: o == W)
    next[o] = p < 0 ? kMtNone : (uint32_t)p;
}

__device__ inline int mt_seg_end(int seg, int nseg, int W) { return seg == nseg - 1 ? W + 1 : (seg + 1) * kMtSeg; }

// hop[o] = (x, c): following next[] from o for c permutations reaches x, the first offset outside o's segment - or, with
// x still inside, the offset whose permutation runs out of the words.  Pointer jumping: a round doubles the permutations covered.
__global__ __launch_bounds__(kMtSegThreads) void mt_jump_kernel(const uint32_t* __restrict__ next, const int* __restrict__ ctl,
                                                                uint2* __restrict__ hop, int W, int nseg) {
    __shared__ uint32_t to[kMtSeg + 1], cnt[kMtSeg + 1];
    if (ctl[2] == (int)kMtPoison) return;
    const int tid = threadIdx.x, lo = blockIdx.x * kMtSeg, hi = mt_seg_end(blockIdx.x, nseg, W), n = hi - lo;
    for (int k = tid; k < n; k += kMtSegThreads) {
        const uint32_t nx = next[lo + k];
        to[k] = nx == kMtNone ? (uint32_t)(lo + k) : nx;     // an offset that cannot go on points at itself
        cnt[k] = nx == kMtNone ? 0u : 1u;
    }
    __syncthreads();
    for (;;) {
        uint32_t nto[kMtSegPer], ncnt[kMtSegPer];
        int changed = 0;
#pragma unroll
        for (int j = 0; j < kMtSegPer; ++j) {
            const int k = tid + j * kMtSegThreads;
            if (k >= n) continue;
            const uint32_t x = nto[j] = to[k];
            ncnt[j] = cnt[k];
            if (x < (uint32_t)hi && to[x - lo] != x) {
                nto[j] = to[x - lo];
                ncnt[j] += cnt[x - lo];
                changed = 1;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kMtSegPer; ++j) {
            const int k = tid + j * kMtSegThreads;
            if (k < n) { to[k] = nto[j]; cnt[k] = ncnt[j]; }
        }
        if (!__syncthreads_or(changed)) break;
    }
    for (int k = tid; k < n; k += kMtSegThreads) hop[lo + k] = make_uint2(to[k], cnt[k]);
}

template <class Cfg>
__global__ __launch_bounds__(kMtSegThreads) void mt_replay_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ next,
                                                                  const uint2* __restrict__ hop, int* __restrict__ ctl,
                                                                  int32_t* __restrict__ orders, int S, int R, int head, int W, int nseg) {
    using Row = typename Cfg::Row;
    constexpr int kHeld = kMtSeg + Cfg::kReplayTail;   // words of the segment and behind it in LDS (beyond: global reads)
    __shared__ uint32_t nx[kMtSeg + 1];            // next[] of the segment, later the rows
    __shared__ uint32_t word[kHeld];
    __shared__ uint16_t start[kMtSeg + 1];         // real starts, relative to the segment
    __shared__ int sh[3];                          // first real start of the segment (-1: none), permutations before it, found here
    const int start_pos = ctl[2];
    if (start_pos == (int)kMtPoison) return;
    const int tid = threadIdx.x, seg = blockIdx.x, lo = seg * kMtSeg, hi = mt_seg_end(seg, nseg, W), n_off = hi - lo;
    if (tid == 0) {
        // the chain of real starts, one hop per segment.  Every workgroup takes the hops to its own segment itself: nseg^2 / 2
        // dependent reads over the grid, but at most nseg (0.3 us each) in a row on any one lane - 11 segments for the 1000
        // permutations of a step, 300 for 30 000 contexts (about 0.1 ms, still under the twist of that many words).  A call of
        // millions of permutations would want one prefix pass over the segments instead.
        int cur = start_pos, before = 0;
        while (cur < lo && before < S) {
            const uint2 h = hop[cur];
            if ((int)h.x < mt_seg_end(min(cur / kMtSeg, nseg - 1), nseg, W)) break;   // runs out of the words before this segment
            cur = (int)h.x;
            before += (int)h.y;
        }
        sh[0] = (cur >= lo && cur < hi && before < S) ? cur : -1;
        sh[1] = before;
    }
    __syncthreads();
    const int entry = sh[0], before = sh[1];
    if (entry < 0) return;
    for (int k = tid; k < n_off; k += kMtSegThreads) nx[k] = next[lo + k];
    if (head > 0)
        for (int k = tid; k < kHeld; k += kMtSegThreads) word[k] = lo + k < W ? mt_temper(keys[lo + k]) : 0u;
    __syncthreads();
    if (tid == 0) {
        int x = entry, n = 0;
        while (before + n < S && x < hi && nx[x - lo] != kMtNone) {
            start[n++] = (uint16_t)(x - lo);
            x = (int)nx[x - lo];
        }
        sh[2] = n;
        if (before + n >= S || x < hi) { ctl[0] = before + n; ctl[1] = x; }   // the call ends here: all drawn, or out of words
    }
    __syncthreads();
    const int n = sh[2];
    if (head == 0) return;                         // the draw only advances the state
    // n rows fit next[]'s storage: n <= (kMtSeg - 1) / (R - 1) + 1 starts in a segment, of R bytes or R 16-bit entries each
    // (R = 2: 4096 rows of 4 bytes; from there the product falls)
    Row* rows = reinterpret_cast<Row*>(nx);
    const auto lds_word = [&](int k) { return k < lo + kHeld ? word[k - lo] : mt_temper(keys[k]); };
    for (int s = tid; s < n; s += kMtSegThreads) perm_replay(lds_word, W, R, lo + start[s], rows + s * R);
    __syncthreads();
    int32_t* out = orders + (size_t)before * head;
    if (head == R) {
        for (int e = tid; e < n * R; e += kMtSegThreads) out[e] = rows[e];
    } else {
        for (int e = tid; e < n * head; e += kMtSegThreads) { const int s = e / head; out[e] = rows[s * R + (e - s * head)]; }
    }
}

// Blocks to twist ahead for S permutations of R regions: the words they draw - mean + 8 standard deviations - the 624 a start
// position can lie in, and a few more.  Draw i = R-1..1 is accepted with p = (i + 1) / (mask + 1): 1 / p draws on average,
// variance (1 - p) / p^2.  0: the mean fits what one batch of mt_permutations_kernel holds behind any start position, and the call
// stays on that kernel - five launches take longer than its one batch (100 permutations of 32 regions: 51 us against 44).
int mt_blocks_estimate(int S, int R) {
    double mean = 0, var = 0;
    for (int i = 1; i < R; ++i) {
        uint32_t mask = 1;
        while (mask < (uint32_t)i) mask = 2 * mask + 1;
        const double p = (i + 1.0) / (mask + 1.0);
        mean += 1 / p;
        var += (1 - p) / (p * p);
    }
    if (S * mean <= kMtWords - kMtN) return 0;
    const double words = kMtN + S * mean + 8 * sqrt(S * var) + 256;
    return (int)fmin(words / kMtN + 2, 3.0e6);     // (int offsets: under 2^31 words)
}

size_t mt_workspace_bytes(int nblk) {              // ctl, keys[W], next[W + 1] (+ 1: 8-byte alignment), hop[W + 1]
    const size_t W = (size_t)nblk * kMtN;
    return sizeof(uint32_t) * (kMtCtl + W + (W + 2) + 2 * (W + 1));
}

// R == 1: a permutation of one region draws nothing
__global__ void zero_orders_kernel(int32_t* __restrict__ orders, int n) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) orders[t] = 0;
}

// one lane per permutation: running OR over its entries; R + 1 coalesced-enough 8-byte stores per lane
__global__ __launch_bounds__(256) void prefix_keep_kernel(const int32_t* __restrict__ orders, uint64_t* __restrict__ keep, int S, int R) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    uint64_t m = 0;
    uint64_t* out = keep + (size_t)s * (R + 1);
    out[0] = 0;
    for (int j = 0; j < R; ++j) {
        const int r = orders[(size_t)s * R + j];
        if ((unsigned)r < 64u) m |= 1ull << r;  // an out-of-range entry is ignored (iq_check_index_range names it)
        out[j + 1] = m;
    }
}

// one lane per (pair, context)
__global__ __launch_bounds__(256) void context_keep_kernel(const int32_t* __restrict__ pairs, const int32_t* __restrict__ ctx,
                                                           uint64_t* __restrict__ keep, int P, int C, int m) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)P * C) return;
    const int p = (int)(t / C);
    uint64_t sset = 0;
    for (int j = 0; j < m; ++j) {
        const int r = ctx[t * m + j];
        if ((unsigned)r < 64u) sset |= 1ull << r;
    }
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    const uint64_t bi = (unsigned)i < 64u ? 1ull << i : 0ull, bj = (unsigned)j < 64u ? 1ull << j : 0ull;
    uint64_t* out = keep + 4 * t;  // rows 4k: S+{i,j}, 4k+1: S+{i}, 4k+2: S+{j}, 4k+3: S
    out[0] = sset | bi | bj;
    out[1] = sset | bi;
    out[2] = sset | bj;
    out[3] = sset;
}

// The one-workgroup kernel alone.  `what`: the entry point's name for messages
template <class Cfg>
int mt_sample_one(const char* what, uint32_t* mt_state, int32_t* orders, int S, int R, int head, hipStream_t st) {
    if (S == 0) return IQ_OK;
    IQ_REQUIRE(mt_state && (orders || head == 0), "%s: null pointer", what);
    if (R == 1) {                                  // nothing is drawn; a row is the one region
        if (head == 0) return IQ_OK;
        IQ_LAUNCH(zero_orders_kernel, dim3((S + 255) / 256), dim3(256), 0, st, orders, S);
        return IQ_OK;
    }
    IQ_LAUNCH(mt_permutations_kernel<Cfg>, dim3(1), dim3(kMtThreads), 0, st, mt_state, orders, S, R, head, nullptr, nullptr, 0);
    return IQ_OK;
}

// The spread kernels over as many blocks as the workspace holds, then the one-workgroup kernel for what is left
template <class Cfg>
int mt_sample_ws(const char* what, uint32_t* mt_state, int32_t* orders, int S, int R, int head, void* workspace, size_t workspace_bytes,
                 hipStream_t st) {
    IQ_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", what);
    // as many blocks ahead as the workspace holds, at most the estimate; under two there is nothing to spread
    int nblk = 0;
    if (workspace && S > 0 && R >= 2) {
        nblk = mt_blocks_estimate(S, R);
        while (nblk >= 2 && mt_workspace_bytes(nblk) > workspace_bytes)
            nblk = (int)fmin(nblk - 1, (double)(workspace_bytes / (16 * kMtN)));
    }
    if (nblk < 2) return mt_sample_one<Cfg>(what, mt_state, orders, S, R, head, st);
    IQ_REQUIRE(mt_state && (orders || head == 0), "%s: null pointer", what);
    const int W = nblk * kMtN, nseg = (W + kMtSeg - 1) / kMtSeg;
    int* ctl = static_cast<int*>(workspace);
    uint32_t* keys = static_cast<uint32_t*>(workspace) + kMtCtl;
    uint32_t* next = keys + W;
    uint2* hop = reinterpret_cast<uint2*>(next + W + 2);
    IQ_LAUNCH(mt_words_kernel, dim3(1), dim3(256), 0, st, mt_state, keys, ctl, nblk);
    IQ_LAUNCH(mt_next_kernel<Cfg>, dim3(W / 256 + 1), dim3(256), 0, st, keys, ctl, next, W, R, Cfg::next_tail(R));
    IQ_LAUNCH(mt_jump_kernel, dim3(nseg), dim3(kMtSegThreads), 0, st, next, ctl, hop, W, nseg);
    IQ_LAUNCH(mt_replay_kernel<Cfg>, dim3(nseg), dim3(kMtSegThreads), 0, st, keys, next, hop, ctl, orders, S, R, head, W, nseg);
    IQ_LAUNCH(mt_permutations_kernel<Cfg>, dim3(1), dim3(kMtThreads), 0, st, mt_state, orders, S, R, head, keys, ctl, nblk);
    return IQ_OK;
}

// heads (P,C,m) of permutations of R - 2 -> region ids: entry k of the ascending list of the regions outside the pair
__global__ __launch_bounds__(256) void context_regions_kernel(const int32_t* __restrict__ pairs, int32_t* __restrict__ heads, size_t total,
                                                              int per_pair) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int p = (int)(t / (size_t)per_pair);
    const int a = pairs[2 * p], b = pairs[2 * p + 1], lo = min(a, b), hi = max(a, b);
    const int k = heads[t];
    heads[t] = k + (k >= lo ? 1 : 0) + (k + 1 >= hi ? 1 : 0);
}

}  // namespace

extern "C" int iq_sample_permutations(uint32_t* mt_state, int32_t* orders, int S, int R, iq_stream_t stream) {
    IQ_REQUIRE(S >= 0 && R >= 1 && R <= IQ_MAX_REGIONS, "iq_sample_permutations: S=%d R=%d", S, R);
    return mt_sample_one<MtNarrow>("iq_sample_permutations", mt_state, orders, S, R, R, iq::as_stream(stream));
}

extern "C" size_t iq_sample_workspace_bytes(int S, int R) {
    if (S <= 0 || R < 2 || R > IQ_MAX_REGIONS || mt_blocks_estimate(S, R) == 0) return 0;
    return mt_workspace_bytes(mt_blocks_estimate(S, R));
}

extern "C" int iq_sample_permutations_ws(uint32_t* mt_state, int32_t* orders, int S, int R, void* workspace, size_t workspace_bytes,
                                         iq_stream_t stream) {
    IQ_REQUIRE(S >= 0 && R >= 1 && R <= IQ_MAX_REGIONS, "iq_sample_permutations_ws: S=%d R=%d", S, R);
    return mt_sample_ws<MtNarrow>("iq_sample_permutations_ws", mt_state, orders, S, R, R, workspace, workspace_bytes, iq::as_stream(stream));
}

extern "C" size_t iq_sample_wide_workspace_bytes(int S, int R) {
    if (S <= 0 || R < 2 || R > IQ_MAX_WIDE_REGIONS || mt_blocks_estimate(S, R) == 0) return 0;
    return mt_workspace_bytes(mt_blocks_estimate(S, R));
}

extern "C" int iq_sample_permutations_wide(uint32_t* mt_state, int32_t* orders, int S, int R, int head, void* workspace,
                                           size_t workspace_bytes, iq_stream_t stream) {
    IQ_REQUIRE(S >= 0 && R >= 1 && R <= IQ_MAX_WIDE_REGIONS && head >= 0 && head <= R, "iq_sample_permutations_wide: S=%d R=%d head=%d", S,
               R, head);
    if (!orders) head = 0;                         // skip mode: the draw advances the state and writes nothing
    return mt_sample_ws<MtWide>("iq_sample_permutations_wide", mt_state, orders, S, R, head, workspace, workspace_bytes,
                                iq::as_stream(stream));
}

extern "C" int iq_context_regions_wide(const int32_t* pairs, int32_t* heads, int P, int C, int m, int R, iq_stream_t stream) {
    IQ_REQUIRE(P >= 0 && C >= 0 && R >= 2 && R <= IQ_MAX_WIDE_REGIONS && m >= 0 && m <= R - 2, "iq_context_regions_wide: P=%d C=%d m=%d R=%d",
               P, C, m, R);
    const size_t total = (size_t)P * C * m;
    if (total == 0) return IQ_OK;
    IQ_REQUIRE(pairs && heads, "iq_context_regions_wide: null pointer");
    IQ_LAUNCH(context_regions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, iq::as_stream(stream), pairs, heads, total,
              C * m);
    return IQ_OK;
}

extern "C" int iq_prefix_keep_masks(const int32_t* orders, uint64_t* keep, int S, int R, iq_stream_t stream) {
    IQ_REQUIRE(S >= 0 && R >= 1 && R <= IQ_MAX_REGIONS, "iq_prefix_keep_masks: S=%d R=%d", S, R);
    if (S == 0) return IQ_OK;
    IQ_REQUIRE(orders && keep, "iq_prefix_keep_masks: null pointer");
    IQ_LAUNCH(prefix_keep_kernel, dim3((S + 255) / 256), dim3(256), 0, iq::as_stream(stream), orders, keep, S, R);
    return IQ_OK;
}

extern "C" int iq_context_keep_masks(const int32_t* pairs, const int32_t* contexts, uint64_t* keep, int P, int C, int m,
                                     iq_stream_t stream) {
    IQ_REQUIRE(P >= 0 && C >= 0 && m >= 0 && m <= IQ_MAX_REGIONS, "iq_context_keep_masks: P=%d C=%d m=%d", P, C, m);
    if ((size_t)P * C == 0) return IQ_OK;
    IQ_REQUIRE(pairs && keep && (contexts || m == 0), "iq_context_keep_masks: null pointer");
    const size_t n = (size_t)P * C;
    IQ_LAUNCH(context_keep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, iq::as_stream(stream), pairs, contexts, keep,
              P, C, m);
    return IQ_OK;
}
