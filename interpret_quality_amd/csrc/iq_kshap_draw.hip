// The counter-based draw of a wide game's coalition rows (include/iq.h, "The COUNTER-BASED draw"): sample m of a cloud is a pure
// function of (seed, stream, m, R).  Philox4x32-10 gives the sample its size (one block, inverse CDF over the host's table) and
// every region a 32-bit key (block i >> 2, word i & 3); the members are the s regions of the smallest composite keys
// (key << 10) | region.  Integer work and one float64 comparison chain: nothing here rounds.
//
// One wave per sample, four per workgroup, as kshap_keep_wide_kernel.  Two layouts, joined through the wave's 4 KB of LDS:
//   * generation: lane l computes blocks l, l + 64, .. (four consecutive regions each) and stores the four words as one 16-byte
//     LDS write, so no block is computed twice;
//   * selection: lane l holds the composite keys of regions l, l + 64, .. in K <= 16 registers (K = the words of a row rounded up
//     to a power of two), so the ballot of "key k of every lane is below the pivot" is a 64-bit mask whose population count is
//     a scalar, and the ballot of "key k is at or below the threshold" IS word k of the row: no shuffles, no LDS for the row.
// The s-th smallest composite key is built from bit 41 down: the pivot keeps a bit when fewer than s keys lie below it.
#include "iq_common.h"

namespace {

constexpr int kMaxR = IQ_MAX_WIDE_REGIONS;
constexpr int kSamplesPerWg = 4;   // waves of a workgroup, one sample each
constexpr int kKeyBits = 42;       // 32 bits of Philox over 10 bits of region index
constexpr unsigned kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned long long p0 = (unsigned long long)kM0 * c.x, p1 = (unsigned long long)kM1 * c.z;
        c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
        k0 += kW0;
        k1 += kW1;
    }
    return c;
}

// 1 + #{k : cdf[k] <= u} over the R - 1 ascending entries, capped at R - 1: every lane runs the same search on the same addresses
__device__ __forceinline__ int size_of(const double* __restrict__ cdf, int R, double u) {
    int lo = 0, hi = R - 1;                                     // the first k with cdf[k] > u lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid + 1;
        else hi = mid;
    }
    return min(R - 1, 1 + lo);
}

template <int K>
__global__ __launch_bounds__(64 * kSamplesPerWg) void kshap_draw_counter_kernel(unsigned k0, unsigned k1, long long first, int S, int R, int W,
                                                                                const double* __restrict__ cdf, int paired,
                                                                                unsigned long long* __restrict__ keep,
                                                                                int32_t* __restrict__ sizes) {
    __shared__ uint4 block_s[kSamplesPerWg][16 * K];            // the wave's Philox words, region order
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * kSamplesPerWg + wave;
    const bool live = j < S;                                    // no early return: every wave reaches the barrier
    const unsigned long long m = (unsigned long long)(first + j);
    const unsigned m_lo = (unsigned)m, m_hi = (unsigned)(m >> 32);
    const int nblocks = (R + 3) >> 2;
    if (live) {
#pragma unroll
        for (int g = 0; g < (K + 3) / 4; ++g) {
            const int b = 64 * g + lane;
            if (b < nblocks && b < 16 * K) block_s[wave][b] = philox4x32_10(make_uint4(m_lo, m_hi, (unsigned)b, 0u), k0, k1);
        }
    }
    __syncthreads();
    if (!live) return;
    const uint4 head = philox4x32_10(make_uint4(m_lo, m_hi, 0u, 1u), k0, k1);
    const double u = ((double)(head.x >> 5) * 67108864.0 + (double)(head.y >> 6)) / 9007199254740992.0;   // exact: 53 bits
    const int s = size_of(cdf, R, u);

    const unsigned* words = reinterpret_cast<const unsigned*>(block_s[wave]);
    unsigned long long key[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = 64 * k + lane;
        key[k] = i < R ? ((unsigned long long)words[i] << 10) | (unsigned long long)i : ~0ull;   // past the game: above every pivot
    }
    unsigned long long t = 0ull;                                // the s-th smallest key: the largest t with fewer than s keys below it
    for (int bit = kKeyBits - 1; bit >= 0; --bit) {
        const unsigned long long pivot = t | (1ull << bit);
        int below = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) below += __popcll(__ballot(key[k] < pivot));
        if (below < s) t = pivot;
    }
    const int rows = paired ? 2 : 1;
    const int q = lane >= W ? 1 : 0, w = lane - q * W;          // row q of the pair, word w of the row
    unsigned long long set = 0ull;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long word = __ballot(key[k] <= t);
        if (w == k) set = word;
    }
    if (lane < rows * W) {
        const unsigned long long all = (w == W - 1 && (R & 63)) ? (1ull << (R & 63)) - 1ull : ~0ull;   // bits at or above R stay 0
        keep[(size_t)j * rows * W + lane] = q ? ~set & all : set;
    }
    if (sizes && lane == 0) sizes[j] = s;
}

template <int K>
int launch(unsigned k0, unsigned k1, long long first, int S, int R, const double* cdf, int paired, uint64_t* keep, int32_t* sizes,
            hipStream_t st) {
    IQ_LAUNCH(kshap_draw_counter_kernel<K>, dim3((unsigned)((S + kSamplesPerWg - 1) / kSamplesPerWg)), dim3(64 * kSamplesPerWg), 0,
              st, k0, k1, first, S, R, iq::keep_words(R), cdf, paired ? 1 : 0, reinterpret_cast<unsigned long long*>(keep), sizes);
    return IQ_OK;
}

}  // namespace

extern "C" int iq_kshap_draw_counter(uint64_t seed, uint64_t stream, int64_t first, int S, int R, const double* cdf, int paired,
                                     uint64_t* keep, int32_t* sizes, iq_stream_t queue) {
    IQ_REQUIRE(R >= 2 && R <= kMaxR, "iq_kshap_draw_counter: R=%d is outside 2..%d", R, kMaxR);
    IQ_REQUIRE(S >= 0 && S <= (1 << 29), "iq_kshap_draw_counter: S=%d", S);
    IQ_REQUIRE(first >= 0 && first <= (1ll << 62) - S, "iq_kshap_draw_counter: first=%lld, S=%d (0 <= first, first + S <= 2^62)",
               (long long)first, S);
    if (S == 0) return IQ_OK;
    IQ_REQUIRE(cdf && keep, "iq_kshap_draw_counter: null pointer");
    const unsigned k0 = (unsigned)(seed & 0xffffffffull), k1 = (unsigned)(stream & 0xffffffffull);
    hipStream_t st = iq::as_stream(queue);
    const int W = iq::keep_words(R);
    if (W <= 1) return launch<1>(k0, k1, first, S, R, cdf, paired, keep, sizes, st);
    else if (W <= 2) return launch<2>(k0, k1, first, S, R, cdf, paired, keep, sizes, st);
    else if (W <= 4) return launch<4>(k0, k1, first, S, R, cdf, paired, keep, sizes, st);
    else if (W <= 8) return launch<8>(k0, k1, first, S, R, cdf, paired, keep, sizes, st);
    else return launch<16>(k0, k1, first, S, R, cdf, paired, keep, sizes, st);
}
