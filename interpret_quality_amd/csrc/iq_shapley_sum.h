// The sum kernel body shared by iq_reward.hip (shapley_sum_kernel, shapley_sum_games_kernel) and iq_wide.hip (shapley_sum_wide_kernel).
#pragma once
#include "iq_common.h"

namespace iq {

// ---- the sum of iq_shapley_accum[_wide|_games]: 64 regions (r0 .. r0 + 63) of (S,R) float64 rows on one workgroup of kSumThreads -
// One lane per region adds strictly in permutation order: the float64 sequence of the reference's host loop, hence its bits.  A
// lane that loads its own rows pays a memory latency every few adds (50 us for 1000 permutations); here the whole workgroup
// brings kSumRows rows at a time into LDS, the next piece on its way while the 64 lanes add the present one.
// ``value(o, r)`` is the float64 entry of permutation o < S and region r < R: a load from the row table (shapley_sum_rows) or the
// float32 difference behind an inverted permutation (iq_shapley_accum_games) - the staging and the adds do not know which.
constexpr int kSumThreads = 256, kSumRows = 64;

template <class Value>
__device__ __forceinline__ void shapley_sum_values(Value value, double* __restrict__ phi_sum, const int32_t* __restrict__ snap_counts,
                                                   int n_snap, double* __restrict__ snaps, int R, int S, int r0) {
    __shared__ double tile[kSumRows * 64];
    constexpr int kPer = kSumRows * 64 / kSumThreads, kStep = kSumThreads / 64;   // rows a lane loads per piece, rows per pass
    const int tid = threadIdx.x, col = tid & 63, sub = tid >> 6, r = r0 + col;
    const bool live = r < R;
    double reg[kPer];
    const auto fetch = [&](int o0) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int o = o0 + sub + kStep * j;
            reg[j] = (live && o < S) ? value(o, r) : 0.0;
        }
    };
    double acc = 0.0;
    int k = 0, next = n_snap > 0 ? snap_counts[0] : -1;      // the count the next snapshot waits for
    fetch(0);
    for (int o0 = 0; o0 < S; o0 += kSumRows) {
#pragma unroll
        for (int j = 0; j < kPer; ++j) tile[(sub + kStep * j) * 64 + col] = reg[j];
        __syncthreads();
        if (o0 + kSumRows < S) fetch(o0 + kSumRows);
        if (tid < 64 && live) {
            const int n = min(kSumRows, S - o0);
            if (next > o0 && next <= o0 + n) {     // a snapshot falls into this piece: add row by row
                for (int row = 0; row < n; ++row) {
                    acc += tile[row * 64 + col];
                    while (next == o0 + row + 1) {
                        snaps[(size_t)k * R + r] = acc;
                        ++k;
                        next = k < n_snap ? snap_counts[k] : -1;
                    }
                }
            } else if (n == kSumRows) {            // a whole piece: all its LDS reads in flight, the adds follow them in order
                double t[kSumRows];
#pragma unroll
                for (int u = 0; u < kSumRows; ++u) t[u] = tile[u * 64 + col];
#pragma unroll
                for (int u = 0; u < kSumRows; ++u) acc += t[u];
            } else {
                for (int row = 0; row < n; ++row) acc += tile[row * 64 + col];
            }
        }
        __syncthreads();
    }
    if (tid < 64 && live) phi_sum[r] = acc;
}

__device__ __forceinline__ void shapley_sum_rows(const double* __restrict__ sv_rows, double* __restrict__ phi_sum,
                                                 const int32_t* __restrict__ snap_counts, int n_snap, double* __restrict__ snaps,
                                                 int R, int S, int r0) {
    shapley_sum_values([&](int o, int r) { return sv_rows[(size_t)o * R + r]; }, phi_sum, snap_counts, n_snap, snaps, R, S, r0);
}

}  // namespace iq
