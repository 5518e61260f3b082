// Exact games by full enumeration: coalition masks of a 2^n lattice, and three reductions over the table v[c] of its rewards -
// Shapley values, pairwise interactions of every order, Harsanyi dividends (Moebius transform).  include/iq.h has the definitions.
//
// All sums are float64 in an order that depends on (n, P) only: no floating-point atomics, two calls give the same bits.
//
// Shapley values and interactions are the same reduction: for a set of Q fixed players (Q = 1: player k; Q = 2: the pair i, j)
// walk the 2^(n-Q) contexts x (coalitions of the other players, found by inserting zero bits at the fixed positions), take the
// float32 difference d(x) the reference takes, and sum it per STRATUM popcount(x).  The strata sums are divided by their exact
// integer weights at the very end, so every output is (a sum of float32 values widened to float64) / integer - one rounding
// beyond the additions, which for rewards of similar magnitude are themselves exact in float64.
//
// Access pattern (strata_kernel): a workgroup takes 16384 consecutive contexts, thread t the contexts t, t + 256, ...: the four
// (two) addresses of consecutive lanes are consecutive floats when the fixed bits are above bit 7 - full 256-byte rows per wave
// load.  A fixed bit 0 makes v[c], v[c | 1] one aligned float2 per lane (contiguous again); a fixed bit in 1 .. 7 leaves loads
// that interleave to full cache lines across the two or four of them (the second touch of a line hits L1).
// The table is read once per pair (64 MB at n = 24: it stays in the 256 MiB last-level cache between pairs).
// The stratum of context x = chunk * 16384 + jj * 256 + t is popcount(chunk) + popcount(jj) + popcount(t): jj is a compile-time
// constant of the unrolled loop, so a thread keeps 7 register accumulators; the workgroup folds them by popcount(t) through LDS
// in a fixed two-level order into 15 bins, and the gather kernel shifts each chunk's bins by popcount(chunk).
#include "iq_common.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 64;                    // contexts per thread, unrolled: popcount(jj) <= 6
constexpr int kChunk = kThreads * kPerThread;     // contexts per workgroup
constexpr int kLocal = 7;                         // accumulators per thread
constexpr int kBins = 16;                         // popcount(jj) + popcount(t) <= 14; bin 15 stays zero
constexpr int kMaxPairs = 65535;                  // pairs per call: the grid's y dimension

struct PlayerTable { unsigned char region[IQ_MAX_EXACT_PLAYERS]; };
struct Denominators { double d[IQ_MAX_EXACT_PLAYERS]; };

__host__ __device__ inline int chunks_of(int bits) { return bits <= 14 ? 1 : 1 << (bits - 14); }

// x with a zero bit inserted at position b
__device__ inline uint32_t insert_zero(uint32_t x, int b) { return ((x >> b) << (b + 1)) | (x & ((1u << b) - 1u)); }

__global__ void enum_keep_kernel(unsigned long long* __restrict__ keep, unsigned long long first, size_t count, PlayerTable pl, int n,
                                 unsigned long long base) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    const unsigned long long c = first + b;
    unsigned long long m = base;
    for (int k = 0; k < n; ++k)
        if ((c >> k) & 1ull) m |= 1ull << pl.region[k];
    keep[b] = m;
}

// part[(p * nchunk + chunk) * kBins + r] = sum of d(x) over the chunk's contexts with popcount(jj) + popcount(t) = r.
// Q = 1: p is the player, d = v[c | k] - v[c] (tools/final_common.py:93).  Q = 2: pairs[p] = (i, j),
// d = ((v[c|i|j] + v[c]) - v[c|i]) - v[c|j] (final_cal_interactions.py:33).  A pair outside [0, n) or with i = j reads nothing
// and gives NaN.
template <int Q>
__global__ __launch_bounds__(kThreads) void strata_kernel(const float* __restrict__ v, const int32_t* __restrict__ pairs, int n,
                                                          int nchunk, double* __restrict__ part) {
    __shared__ double sh[kLocal][kThreads];
    __shared__ double fold[16][kBins];
    const int p = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    double* out = part + ((size_t)p * nchunk + chunk) * kBins;
    int i = p, j = -1;
    if (Q == 2) {
        i = pairs[2 * p];
        j = pairs[2 * p + 1];
        if ((unsigned)i >= (unsigned)n || (unsigned)j >= (unsigned)n || i == j) {
            if (t < kBins) out[t] = NAN;
            return;
        }
    }
    const int lo = Q == 2 && j < i ? j : i, hi = Q == 2 && j < i ? i : j;
    const uint32_t bi = 1u << i, bj = Q == 2 ? 1u << j : 0u;
    const uint32_t total = 1u << (n - Q);
    double acc[kLocal];
#pragma unroll
    for (int q = 0; q < kLocal; ++q) acc[q] = 0.0;
#pragma unroll
    for (int jj = 0; jj < kPerThread; ++jj) {
        const uint32_t x = (uint32_t)chunk * kChunk + jj * kThreads + t;
        if (x < total) {
            uint32_t c = insert_zero(x, lo);
            if (Q == 2) c = insert_zero(c, hi);
            float d;
            if (lo == 0) {   // (workgroup-uniform) v[c] and v[c | 1] are one aligned float2: lanes read 8 contiguous bytes each
                const float2 a = *reinterpret_cast<const float2*>(v + c);
                if (Q == 1) {
                    d = __fsub_rn(a.y, a.x);
                } else {
                    const float2 b = *reinterpret_cast<const float2*>(v + (c | (1u << hi)));
                    const float vi = i == 0 ? a.y : b.x, vj = i == 0 ? b.x : a.y;   // v[c | i], v[c | j]
                    d = __fsub_rn(__fsub_rn(__fadd_rn(b.y, a.x), vi), vj);
                }
            } else if (Q == 1) {
                d = __fsub_rn(v[c | bi], v[c]);
            } else {
                d = __fsub_rn(__fsub_rn(__fadd_rn(v[c | bi | bj], v[c]), v[c | bi]), v[c | bj]);
            }
            acc[__builtin_popcount(jj)] += (double)d;
        }
    }
#pragma unroll
    for (int q = 0; q < kLocal; ++q) sh[q][t] = acc[q];
    __syncthreads();
    {   // 16 groups of 16 threads, then the 16 groups: a fixed order
        const int r = t & 15, g = t >> 4;
        double s = 0.0;
        for (int u = 0; u < 16; ++u) {
            const int tt = g * 16 + u, q = r - __builtin_popcount(tt);
            if (q >= 0 && q < kLocal) s += sh[q][tt];
        }
        fold[g][r] = s;
    }
    __syncthreads();
    if (t < kBins) {
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += fold[g][t];
        out[t] = s;
    }
}

// One workgroup per row p, thread s per stratum: term(s) = (sum over the chunks, in chunk order, of the bin of stratum s) / den[s].
// sum_strata = 0: out[p * S + s] = term(s) (interactions).  sum_strata = 1: out[p] = the terms added in stratum order (Shapley).
__global__ __launch_bounds__(32) void strata_gather_kernel(const double* __restrict__ part, int nchunk, int S, Denominators den,
                                                          int sum_strata, double* __restrict__ out) {
    __shared__ double term[32];
    const int p = blockIdx.x, s = threadIdx.x;
    const double* row = part + (size_t)p * nchunk * kBins;
    double acc = 0.0;
    if (s < S) {
#pragma unroll 8
        for (int ch = 0; ch < nchunk; ++ch) {
            const int r = s - __builtin_popcount(ch);
            const double x = row[(size_t)ch * kBins + (r & (kBins - 1))];
            if (r >= 0 && r < kBins) acc += x;
        }
        acc /= den.d[s];
        if (!sum_strata) out[(size_t)p * S + s] = acc;
    }
    if (!sum_strata) return;
    term[s] = acc;
    __syncthreads();
    if (s == 0) {
        double phi = 0.0;
        for (int q = 0; q < S; ++q) phi += term[q];
        out[p] = phi;
    }
}

// Moebius transform: a[c] -= a[c without bit b] for every bit b in turn.  The low bits of a 2048-entry tile in LDS ...
constexpr int kMoebiusLow = 11;
__global__ __launch_bounds__(kThreads) void moebius_low_kernel(const float* __restrict__ v, double* __restrict__ a, int L) {
    __shared__ double sh[1 << kMoebiusLow];
    const int size = 1 << L, t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x << L;
    for (int e = t; e < size; e += kThreads) sh[e] = (double)v[base + e];
    __syncthreads();
    for (int b = 0; b < L; ++b) {
        for (int x = t; x < size / 2; x += kThreads) {
            const uint32_t c = insert_zero((uint32_t)x, b);
            sh[c | (1u << b)] -= sh[c];
        }
        __syncthreads();
    }
    for (int e = t; e < size; e += kThreads) a[base + e] = sh[e];
}

// ... the bits above them NB at a time in registers: a thread owns the 2^NB entries that differ in bits b0 .. b0 + NB - 1.
template <int NB>
__global__ __launch_bounds__(kThreads) void moebius_high_kernel(double* __restrict__ a, int n, int b0) {
    const size_t x = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (x >= ((size_t)1 << (n - NB))) return;
    const size_t base = ((x >> b0) << (b0 + NB)) | (x & (((size_t)1 << b0) - 1));
    double r[1 << NB];
#pragma unroll
    for (int u = 0; u < (1 << NB); ++u) r[u] = a[base + ((size_t)u << b0)];
#pragma unroll
    for (int bit = 0; bit < NB; ++bit)
#pragma unroll
        for (int u = 0; u < (1 << NB); ++u)
            if (u & (1 << bit)) r[u] -= r[u ^ (1 << bit)];
#pragma unroll
    for (int u = 0; u < (1 << NB); ++u) a[base + ((size_t)u << b0)] = r[u];
}

double binomial(int n, int k) {
    double c = 1.0;   // exact: every intermediate is an integer below 2^53 for n <= 24
    for (int i = 1; i <= k; ++i) c = c * (n - k + i) / i;
    return c;
}

size_t part_doubles(int rows, int n) { return (size_t)rows * chunks_of(n - 1) * kBins; }

}  // namespace

extern "C" size_t iq_exact_scratch_bytes(int n, int P) {
    if (n < 1 || n > IQ_MAX_EXACT_PLAYERS || P < 0 || P > kMaxPairs) return 0;
    return part_doubles(P > n ? P : n, n) * sizeof(double);
}

extern "C" int iq_enum_keep_masks(uint64_t* keep, uint64_t first, size_t count, const int32_t* players, int n, uint64_t base,
                                  iq_stream_t stream) {
    IQ_REQUIRE(n >= 1 && n <= IQ_MAX_EXACT_PLAYERS, "iq_enum_keep_masks: n=%d is outside 1..%d", n, IQ_MAX_EXACT_PLAYERS);
    IQ_REQUIRE(count <= ((size_t)1 << 30), "iq_enum_keep_masks: count=%zu", count);
    PlayerTable pl;
    uint64_t seen = 0;
    for (int k = 0; k < n; ++k) {
        const int r = players ? players[k] : k;
        IQ_REQUIRE(r >= 0 && r < IQ_MAX_REGIONS, "iq_enum_keep_masks: players[%d]=%d is outside [0,%d)", k, r, IQ_MAX_REGIONS);
        IQ_REQUIRE(!((seen >> r) & 1), "iq_enum_keep_masks: region %d is named by two players (second: players[%d])", r, k);
        IQ_REQUIRE(!((base >> r) & 1), "iq_enum_keep_masks: players[%d]=%d is also in base (always kept)", k, r);
        seen |= 1ull << r;
        pl.region[k] = (unsigned char)r;
    }
    if (count == 0) return IQ_OK;
    IQ_REQUIRE(keep, "iq_enum_keep_masks: null pointer");
    IQ_LAUNCH(enum_keep_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, iq::as_stream(stream),
              reinterpret_cast<unsigned long long*>(keep), (unsigned long long)first, count, pl, n, (unsigned long long)base);
    return IQ_OK;
}

extern "C" int iq_exact_shapley(const float* v, int n, double* phi, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(n >= 1 && n <= IQ_MAX_EXACT_PLAYERS, "iq_exact_shapley: n=%d is outside 1..%d", n, IQ_MAX_EXACT_PLAYERS);
    IQ_REQUIRE(v && phi && scratch, "iq_exact_shapley: null pointer");
    IQ_REQUIRE(((uintptr_t)v & 7) == 0, "iq_exact_shapley: v must be 8-byte aligned");
    const int nchunk = chunks_of(n - 1);
    const size_t np = (size_t)n * nchunk * kBins;
    if (scratch_bytes < np * sizeof(double) || ((uintptr_t)scratch & 7))
        return iq::fail(IQ_EWORKSPACE, "iq_exact_shapley: scratch of %zu bytes (8-byte aligned) needed, got %zu", np * sizeof(double), scratch_bytes);
    double* part = static_cast<double*>(scratch);
    Denominators den;
    for (int s = 0; s < n; ++s) den.d[s] = n * binomial(n - 1, s);   // 1 / w(s), an integer
    hipStream_t st = iq::as_stream(stream);
    IQ_LAUNCH(strata_kernel<1>, dim3(nchunk, n), dim3(kThreads), 0, st, v, nullptr, n, nchunk, part);
    IQ_LAUNCH(strata_gather_kernel, dim3(n), dim3(32), 0, st, part, nchunk, n, den, 1, phi);
    return IQ_OK;
}

extern "C" int iq_exact_interactions(const float* v, int n, const int32_t* pairs, int P, double* out, void* scratch,
                                     size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(n >= 1 && n <= IQ_MAX_EXACT_PLAYERS, "iq_exact_interactions: n=%d is outside 1..%d", n, IQ_MAX_EXACT_PLAYERS);
    IQ_REQUIRE(P >= 0 && P <= kMaxPairs, "iq_exact_interactions: P=%d is outside 0..%d", P, kMaxPairs);
    if (P == 0) return IQ_OK;
    IQ_REQUIRE(n >= 2, "iq_exact_interactions: a pair needs n >= 2 players, got n=%d", n);
    IQ_REQUIRE(v && pairs && out && scratch, "iq_exact_interactions: null pointer");
    IQ_REQUIRE(((uintptr_t)v & 7) == 0, "iq_exact_interactions: v must be 8-byte aligned");
    const int nchunk = chunks_of(n - 2);
    const size_t np = (size_t)P * nchunk * kBins;
    if (scratch_bytes < np * sizeof(double) || ((uintptr_t)scratch & 7))
        return iq::fail(IQ_EWORKSPACE, "iq_exact_interactions: scratch of %zu bytes (8-byte aligned) needed, got %zu", np * sizeof(double), scratch_bytes);
    double* part = static_cast<double*>(scratch);
    Denominators den;
    for (int m = 0; m < n - 1; ++m) den.d[m] = binomial(n - 2, m);   // the number of contexts of order m
    hipStream_t st = iq::as_stream(stream);
    IQ_LAUNCH(strata_kernel<2>, dim3(nchunk, P), dim3(kThreads), 0, st, v, pairs, n, nchunk, part);
    IQ_LAUNCH(strata_gather_kernel, dim3(P), dim3(32), 0, st, part, nchunk, n - 1, den, 0, out);
    return IQ_OK;
}

extern "C" int iq_moebius(const float* v, int n, double* a, iq_stream_t stream) {
    IQ_REQUIRE(n >= 1 && n <= IQ_MAX_EXACT_PLAYERS, "iq_moebius: n=%d is outside 1..%d", n, IQ_MAX_EXACT_PLAYERS);
    IQ_REQUIRE(v && a, "iq_moebius: null pointer");
    hipStream_t st = iq::as_stream(stream);
    const int L = n < kMoebiusLow ? n : kMoebiusLow;
    IQ_LAUNCH(moebius_low_kernel, dim3(1u << (n - L)), dim3(kThreads), 0, st, v, a, L);
    for (int b = L; b < n;) {
        const int nb = n - b >= 3 ? 3 : n - b;
        const unsigned blocks = (unsigned)((((size_t)1 << (n - nb)) + kThreads - 1) / kThreads);
        if (nb == 3) IQ_LAUNCH(moebius_high_kernel<3>, dim3(blocks), dim3(kThreads), 0, st, a, n, b);
        else if (nb == 2) IQ_LAUNCH(moebius_high_kernel<2>, dim3(blocks), dim3(kThreads), 0, st, a, n, b);
        else IQ_LAUNCH(moebius_high_kernel<1>, dim3(blocks), dim3(kThreads), 0, st, a, n, b);
        b += nb;
    }
    return IQ_OK;
}
