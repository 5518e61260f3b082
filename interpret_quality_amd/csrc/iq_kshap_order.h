// The summation order of the regression estimator's moments, written once for the narrow kernels (iq_kshap.hip: a row is one
// uint64) and the wide ones (iq_kshap_wide.hip: a row is W words): the cut of the rows into chunks, the moment b of one chunk,
// a chunk's sum of weights and the fold of the chunks; then what the estimators built on them (iq_kshap_pairs.hip, iq_kshap_paircv.hip
// and the standard errors) share: a row's size, a chunk's scalar sum, the kernels over the iid units, the fold of the moments and
// the host's checks.  include/iq.h, "The regression (KernelSHAP) estimator", has the contract.
#pragma once
#include "iq_common.h"

#include <cstdint>

namespace iq {
namespace kshap {

constexpr int kThreads = 256;
constexpr int kTile = 256;          // rows staged per step: one per thread
constexpr int kMaxChunks = 256;

struct Chunks { int count, tiles_per; };

// A chunk is a whole number of 256-row tiles, at most kMaxChunks chunks: a function of M alone.
__host__ __device__ inline Chunks chunks_of(long long M) {
    const long long tiles = (M + kTile - 1) / kTile;
    const long long per = (tiles + kMaxChunks - 1) / kMaxChunks;
    return {(int)((tiles + per - 1) / per), (int)per};
}

// The cut of the pairwise product Q (iq_kshap_pairs.hip), whose partials are R x R per chunk: chunks_of(M) with the count capped so
// that one game's partials, counted as count * R * R float64, stay within kPairPartialBytes (8 chunks at R = 1024) - a function
// of (M, R) alone.  Where the cap does not bind it is chunks_of(M).
constexpr long long kPairPartialBytes = 64ll << 20;

__host__ __device__ inline Chunks pair_chunks_of(long long M, int R) {
    const Chunks ch = chunks_of(M);
    const long long cap = kPairPartialBytes / (8ll * R * R);      // >= 8 for R <= 1024
    if (ch.count <= cap) return ch;
    const long long tiles = (M + kTile - 1) / kTile;
    const long long per = (tiles + cap - 1) / cap;
    return {(int)((tiles + per - 1) / per), (int)per};
}

// the bits of word `word` of a row that exist: all 64, or the low R - 64 word of the last word
__device__ __forceinline__ unsigned long long live_mask(int word, int R) {
    const int bits = R - 64 * word;
    return bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
}

// the number of regions below R that a row of W words keeps
__device__ __forceinline__ int row_size(const unsigned long long* __restrict__ row, int W, int R) {
    int s = 0;
    for (int w = 0; w < W; ++w) s += __popcll(row[w] & live_mask(w, R));
    return s;
}

// The workgroup's values x, one per thread, added in thread order through the kThreads words of `sh` (free to be overwritten:
// every thread is past its last read of them); the sum is thread 0's return value.
template <typename T>
__device__ __forceinline__ T sum_threads_in_order(T* sh, T x) {
    sh[threadIdx.x] = x;
    __syncthreads();
    T s = T(0);
    if (threadIdx.x == 0)
        for (int u = 0; u < kThreads; ++u) s += sh[u];
    return s;
}

// One chunk's sum of d_m z_mi for the 64 regions of word `word` of rows of W words (narrow: W = 1, word 0), d_m = value(m, w_m) of a
// live row, on a workgroup of kThreads: lane i of wave q adds rows 64 q .. 64 q + 63 of every tile in row order, then the four
// waves are added as ((0 + 1) + 2) + 3.  Every LDS read of the inner loop is a broadcast.  Threads t < 64 write out[t] when
// t < live_bits (the regions of this word that exist).  With wpart the workgroup also leaves the chunk's sum of weights there: per
// thread over its rows t, t + 256, ... of the chunk, then the 256 threads in index order.  What lane i sums over is member(word, i):
// bit i of the word, or whatever else a lane stands for (iq_kshap_paircv.hip: a feature of the surrogate).
struct BitOfLane {
    __device__ __forceinline__ bool operator()(unsigned long long word, int lane) const { return (word >> lane) & 1ull; }
};

template <typename RowValue, typename Member = BitOfLane>
__device__ __forceinline__ void moment_chunk_of(const unsigned long long* __restrict__ keep, int W, int word, RowValue value,
                                                const double* __restrict__ weights, long long M, int tiles_per, int chunk,
                                                double* __restrict__ out, int live_bits, double* __restrict__ wpart,
                                                Member member = Member()) {
    __shared__ unsigned long long sh_keep[kTile];
    __shared__ double sh_d[kTile];
    __shared__ double sh_fold[4][64];
    const int t = threadIdx.x, lane = t & 63, q = t >> 6;
    const long long row0 = (long long)chunk * tiles_per * kTile;
    double acc = 0.0, wacc = 0.0;
    for (int tile = 0; tile < tiles_per; ++tile) {
        const long long m = row0 + (long long)tile * kTile + t;
        const bool live = m < M;
        const double w = live ? (weights ? weights[m] : 1.0) : 0.0;
        sh_keep[t] = live ? keep[(size_t)m * W + word] : 0ull;
        sh_d[t] = live ? value(m, w) : 0.0;
        wacc += w;
        __syncthreads();
#pragma unroll 8
        for (int r = q * 64; r < q * 64 + 64; ++r) acc += member(sh_keep[r], lane) ? sh_d[r] : 0.0;
        __syncthreads();
    }
    sh_fold[q][lane] = acc;
    __syncthreads();
    if (t < live_bits) out[t] = ((sh_fold[0][t] + sh_fold[1][t]) + sh_fold[2][t]) + sh_fold[3][t];
    if (wpart) {
        const double s = sum_threads_in_order(sh_d, wacc);      // sh_d: the barrier above is past its last read
        if (t == 0) *wpart = s;
    }
}

// moment_chunk_of with d_m = w_m ((double)vg[m] - base): the moment b of the regression estimator.
__device__ __forceinline__ void moment_chunk(const unsigned long long* __restrict__ keep, int W, int word, const float* __restrict__ vg,
                                             double base, const double* __restrict__ weights, long long M, int tiles_per, int chunk,
                                             double* __restrict__ out, int live_bits, double* __restrict__ wpart) {
    moment_chunk_of(keep, W, word, [vg, base](long long m, double w) { return w * ((double)vg[m] - base); }, weights, M, tiles_per,
                    chunk, out, live_bits, wpart);
}

// The chunks' partials p[0], p[stride], ... added in chunk order.
__device__ __forceinline__ double fold_chunks(const double* __restrict__ p, size_t stride, int nchunk) {
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += p[(size_t)c * stride];
    return s;
}

// wsum: the chunks' sums of weights in chunk order; without weights it is M.
__device__ __forceinline__ double fold_wsum(const double* __restrict__ partW, int weighted, long long M, int nchunk) {
    return weighted ? fold_chunks(partW, 1, nchunk) : (double)M;
}

// One chunk's sum of value(m) over its rows m < M, on a workgroup of kThreads: per thread over its rows t, t + 256, ... of the chunk,
// then the 256 threads in index order (the rule of a chunk's sum of weights); the sum is thread 0's return value.
template <typename RowValue>
__device__ __forceinline__ double scalar_chunk_of(RowValue value, long long M, int tiles_per, int chunk) {
    __shared__ double sh[kThreads];
    const long long row0 = (long long)chunk * tiles_per * kTile;
    double acc = 0.0;
    for (int tile = 0; tile < tiles_per; ++tile) {
        const long long m = row0 + (long long)tile * kTile + threadIdx.x;
        if (m < M) acc += value(m);
    }
    return sum_threads_in_order(sh, acc);
}

// The two kernels over the iid units u of a standard error (a unit's first row starts at keep + u * stride words).  `unit` holds
// kArrays arrays of U values per game; x0 is game 0's array of the value summed, game g's is x0 + kArrays g U.
// Grid (chunk of chunks_of(U), word, game): part[(g * nchunk + chunk) * R + 64 word + i] = the chunk's sum of x_u z_ui in
// moment_chunk_of's order.
template <int kArrays>
__global__ __launch_bounds__(kThreads) void unit_moment_kernel(const unsigned long long* __restrict__ keep, const double* __restrict__ x0,
                                                               long long U, int R, int stride, int tiles_per, double* __restrict__ part) {
    const int chunk = blockIdx.x, word = blockIdx.y, g = blockIdx.z;
    const double* x = x0 + (size_t)kArrays * g * U;
    moment_chunk_of(
        keep, stride, word, [=](long long u, double) { return x[u]; }, nullptr, U, tiles_per, chunk,
        part + ((size_t)g * gridDim.x + chunk) * R + 64 * word, min(64, R - 64 * word), nullptr);
}

// Grid (chunk of chunks_of(U), game): part[g * nchunk + chunk] = the chunk's sum of x_u by scalar_chunk_of.
template <int kArrays>
__global__ __launch_bounds__(kThreads) void unit_scalar_kernel(const double* __restrict__ x0, long long U, int tiles_per,
                                                               double* __restrict__ part) {
    const int chunk = blockIdx.x, g = blockIdx.y;
    const double* x = x0 + (size_t)kArrays * g * U;
    const double s = scalar_chunk_of([=](long long u) { return x[u]; }, U, tiles_per, chunk);
    if (threadIdx.x == 0) part[(size_t)g * gridDim.x + chunk] = s;
}

// One thread per output: the chunks' partials added in chunk order.  Entries [0, G R): L; with kScalars then G of A; the last one wsum.
template <bool kScalars>
__global__ __launch_bounds__(kThreads) void fold_moments_kernel(const double* __restrict__ partL, const double* __restrict__ partA,
                                                                const double* __restrict__ partW, int weighted, long long M, int R, int G,
                                                                int nchunk, double* __restrict__ L, double* __restrict__ A,
                                                                double* __restrict__ wsum) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x, nl = (long long)G * R, na = kScalars ? G : 0;
    if (e < nl) {
        const long long g = e / R, i = e % R;
        L[e] = fold_chunks(partL + (size_t)g * nchunk * R + i, R, nchunk);
    } else if (e < nl + na) {
        const long long g = e - nl;
        A[g] = fold_chunks(partA + (size_t)g * nchunk, 1, nchunk);
    } else if (e == nl + na) {
        *wsum = fold_wsum(partW, weighted, M, nchunk);
    }
}

// The variance of an estimate (1 / M) sum_u x_u from S1 = sum_u x_u and S2 = sum_u x_u^2 over the U iid units of M rows, every
// operation rounded on its own.
__device__ __forceinline__ double unit_variance(double s1, double s2, long long U, long long M) {
#pragma clang fp contract(off)
    const double units = (double)U, rows = (double)M;
    return ((units / (units - 1.0)) * (s2 - s1 * s1 / units)) / (rows * rows);
}

// ---- the host's side ------------------------------------------------------------------------------------------------------------

// the units of M rows; 0 where the rows do not make at least two whole units
inline long long units_of(long long M, int paired) {
    if (paired && (M & 1)) return 0;
    const long long U = paired ? M / 2 : M;
    return U >= 2 ? U : 0;
}

// 2 H_{R-1}, float64, the harmonic sum ascending: summed on the host, passed to the kernels by value
inline double two_harmonic(int R) {
    double h = 0.0;
    for (int k = 1; k < R; ++k) h += 1.0 / (double)k;
    return 2.0 * h;
}

// the rows, regions and games an entry of the family takes; max_r: IQ_MAX_REGIONS or IQ_MAX_WIDE_REGIONS
inline bool rows_ok(long long M, int R, int G, int max_r) {
    return M >= 1 && M <= (1ll << 30) && R >= 2 && R <= max_r && G >= 1 && G <= 65535;
}

// IQ_OK when the caller's scratch holds `need` bytes and is 8-byte aligned
inline int scratch_ok(const char* name, const void* scratch, size_t got, size_t need) {
    if (got < need || ((uintptr_t)scratch & 7))
        return fail(IQ_EWORKSPACE, "%s: scratch of %zu bytes (8-byte aligned) needed, got %zu", name, need, got);
    return IQ_OK;
}

}  // namespace kshap
}  // namespace iq
