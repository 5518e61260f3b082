// The summation order of the regression estimator's moments, written once for the narrow kernels (iq_kshap.hip: a row is one
// uint64) and the wide ones (iq_kshap_wide.hip: a row is W words): the cut of the rows into chunks, the moment b of one chunk,
// a chunk's sum of weights and the fold of the chunks.  include/iq.h, "The regression (KernelSHAP) estimator", has the contract.
#pragma once
#include "iq_common.h"

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
// thread over its rows t, t + 256, ... of the chunk, then the 256 threads in index order.
template <typename RowValue>
__device__ __forceinline__ void moment_chunk_of(const unsigned long long* __restrict__ keep, int W, int word, RowValue value,
                                                const double* __restrict__ weights, long long M, int tiles_per, int chunk,
                                                double* __restrict__ out, int live_bits, double* __restrict__ wpart) {
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
        for (int r = q * 64; r < q * 64 + 64; ++r) acc += (sh_keep[r] >> lane) & 1ull ? sh_d[r] : 0.0;
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

}  // namespace kshap
}  // namespace iq
