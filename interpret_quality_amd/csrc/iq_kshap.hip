// The regression (KernelSHAP) estimator of a region game of 2 <= n <= 64 regions: coalition rows from permutations and sizes, the
// moments A = sum w z z^T and b = sum w z (v - v0) of those rows, and the constrained solve.  include/iq.h has the definitions.
//
// Every float64 sum is taken in an order that depends on (M, n, G) only - the rule of strata_kernel (iq_lattice.hip): a workgroup
// sums a CHUNK of rows in row order, a second small kernel folds the chunks in chunk order; no atomics, and the grid is a
// function of M alone.  A chunk is a whole number of 256-row TILES (the rows a workgroup stages in LDS at a time); at most
// kMaxChunks chunks, so the scratch stays bounded when M is the 2^24 rows of an enumerated game.  Without weights A holds
// co-occurrence counts: the same kernel with integer accumulators, exact and order-free.
#include "iq_common.h"
#include "iq_kshap_order.h"

namespace {

// iq_kshap_order.h: the cut into chunks, the moment of a chunk and the folds, shared with the wide form (iq_kshap_wide.hip)
using iq::kshap::Chunks;
using iq::kshap::chunks_of;
using iq::kshap::kThreads;
using iq::kshap::kTile;

constexpr int kMaxN = IQ_MAX_REGIONS;
constexpr int kCols = 16;           // entries of a row of A per thread: 256 threads x 16 = 64 x 64

// One thread per sample: the first sizes[m] entries of permutation m as a bit mask; paired: its complement within n bits beside it.
// status: 1 = a size outside 1 .. n-1, 2 = an order entry outside [0, n) (the row is written as 0 either way).
__global__ void kshap_keep_kernel(const int32_t* __restrict__ orders, const int32_t* __restrict__ sizes,
                                  unsigned long long* __restrict__ keep, int S, int n, int paired, int32_t* __restrict__ status) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= S) return;
    const int s = sizes[m];
    unsigned long long mask = 0;
    int bad = (s < 1 || s > n - 1) ? 1 : 0;
    if (!bad) {
        const int32_t* row = orders + (size_t)m * n;
        for (int i = 0; i < s; ++i) {
            const int r = row[i];
            if ((unsigned)r >= (unsigned)n) bad = 2;
            else mask |= 1ull << r;
        }
    }
    if (bad) {
        atomicMax(status, bad);
        mask = 0;
    }
    const unsigned long long all = n == 64 ? ~0ull : (1ull << n) - 1ull;
    if (paired) {
        keep[2 * (size_t)m] = mask;
        keep[2 * (size_t)m + 1] = bad ? 0ull : ~mask & all;
    } else {
        keep[m] = mask;
    }
}

// partA[(chunk * n + i) * n + j] = the chunk's sum of w_m z_mi z_mj in row order; T = double (weights given; partW[chunk] = the
// chunk's sum of w_m: per thread over its rows t, t + 256, ..., then the 256 threads in index order) or T = unsigned long long
// (w = 1: counts).  Thread t owns row i = t / 4 of A and the 16 columns from 16 (t % 4).
template <typename T>
__global__ __launch_bounds__(kThreads) void kshap_gram_kernel(const unsigned long long* __restrict__ keep,
                                                              const double* __restrict__ weights, long long M, int n, int tiles_per,
                                                              T* __restrict__ partA, double* __restrict__ partW) {
    __shared__ unsigned long long sh_keep[kTile];
    __shared__ T sh_w[kTile];
    const int t = threadIdx.x, i = t >> 2, j0 = (t & 3) * kCols;
    const long long row0 = (long long)blockIdx.x * tiles_per * kTile;
    T acc[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) acc[c] = T(0);
    T wacc = T(0);
    for (int tile = 0; tile < tiles_per; ++tile) {
        const long long m = row0 + (long long)tile * kTile + t;
        const bool live = m < M;
        const T w = live ? (weights ? (T)weights[m] : T(1)) : T(0);
        sh_keep[t] = live ? keep[m] : 0ull;
        sh_w[t] = w;
        wacc += w;
        __syncthreads();
        if (i < n) {
            for (int r = 0; r < kTile; ++r) {
                const unsigned long long k = sh_keep[r];
                const T wi = (k >> i) & 1ull ? sh_w[r] : T(0);
                const unsigned cols = (unsigned)(k >> j0);
#pragma unroll
                for (int c = 0; c < kCols; ++c) acc[c] += (cols >> c) & 1u ? wi : T(0);
            }
        }
        __syncthreads();
    }
    if (i < n) {
#pragma unroll
        for (int c = 0; c < kCols; ++c)
            if (j0 + c < n) partA[((size_t)blockIdx.x * n + i) * n + j0 + c] = acc[c];
    }
    if (partW) {
        const T s = iq::kshap::sum_threads_in_order(sh_w, wacc);
        if (t == 0) partW[blockIdx.x] = (double)s;
    }
}

// partB[(g * nchunk + chunk) * n + i] = the chunk's sum of w_m z_mi ((double)v[g][m] - v0[g]): lane i of wave q adds rows
// 64 q .. 64 q + 63 of every tile in row order, then the four waves are added in wave order (iq::kshap::moment_chunk).
__global__ __launch_bounds__(kThreads) void kshap_moment_kernel(const unsigned long long* __restrict__ keep, const float* __restrict__ v,
                                                                const double* __restrict__ v0, const double* __restrict__ weights,
                                                                long long M, int n, int tiles_per, double* __restrict__ partB) {
    const int g = blockIdx.y;
    iq::kshap::moment_chunk(keep, 1, 0, v + (size_t)g * M, v0[g], weights, M, tiles_per, blockIdx.x,
                            partB + ((size_t)g * gridDim.x + blockIdx.x) * n, n, nullptr);
}

// One thread per output: the chunks' partials added in chunk order.  Entries [0, n^2): A; then G n of b; the last one wsum.
__global__ __launch_bounds__(kThreads) void kshap_fold_kernel(const void* __restrict__ partA, const double* __restrict__ partB,
                                                              const double* __restrict__ partW, int weighted, long long M, int n, int G,
                                                              int nchunk, double* __restrict__ A, double* __restrict__ b,
                                                              double* __restrict__ wsum) {
    const int e = blockIdx.x * kThreads + threadIdx.x, nn = n * n;
    if (e < nn) {
        if (weighted) {
            A[e] = iq::kshap::fold_chunks(static_cast<const double*>(partA) + e, nn, nchunk);
        } else {
            const unsigned long long* p = static_cast<const unsigned long long*>(partA);
            unsigned long long s = 0;
            for (int c = 0; c < nchunk; ++c) s += p[(size_t)c * nn + e];
            A[e] = (double)s;          // a count below 2^53: exact
        }
    } else if (e < nn + G * n) {
        const int g = (e - nn) / n, i = (e - nn) % n;
        b[e - nn] = iq::kshap::fold_chunks(partB + (size_t)g * nchunk * n + i, n, nchunk);
    } else if (e == nn + G * n) {
        *wsum = iq::kshap::fold_wsum(partW, weighted, M, nchunk);
    }
}

// One workgroup.  Cholesky A = L L^T in LDS (rows padded to 65 doubles: a column walk touches every bank), then right-hand side
// 0 = the ones vector and 1 .. G = the rows of b, 32 at a time, one lane each: L y = rhs, L^T x = y in the lane's column of xs.
constexpr int kLd = kMaxN + 1;
constexpr int kRhs = 32;

__global__ __launch_bounds__(kThreads) void kshap_solve_kernel(const double* __restrict__ A, const double* __restrict__ b,
                                                               const double* __restrict__ delta, double* __restrict__ phi,
                                                               int32_t* __restrict__ status, int n, int G) {
    __shared__ double L[kMaxN * kLd];
    __shared__ double xs[kMaxN][kRhs];
    __shared__ double yv[kMaxN];
    __shared__ double sh_tol, sh_sy;
    const int t = threadIdx.x;
    for (int e = t; e < n * n; e += kThreads) L[(e / n) * kLd + e % n] = A[e];
    __syncthreads();
    if (t == 0) {
        double mx = 0.0;
        for (int i = 0; i < n; ++i) mx = L[i * kLd + i] > mx ? L[i * kLd + i] : mx;
        sh_tol = (double)n * 0x1p-52 * mx;
    }
    __syncthreads();
    const double tol = sh_tol;
    for (int k = 0; k < n; ++k) {
        const double pivot = L[k * kLd + k];      // the same LDS word for every thread: the exit below is uniform
        if (!(pivot > tol)) {                     // a NaN pivot leaves too
            if (t == 0) *status = 1;
            return;
        }
        const double d = sqrt(pivot);
        __syncthreads();
        if (t == 0) L[k * kLd + k] = d;
        for (int i = k + 1 + t; i < n; i += kThreads) L[i * kLd + k] /= d;
        __syncthreads();
        const int w = n - k - 1;
        for (int e = t; e < w * w; e += kThreads) {
            const int i = k + 1 + e / w, j = k + 1 + e % w;
            if (j <= i) L[i * kLd + j] -= L[i * kLd + k] * L[j * kLd + k];
        }
        __syncthreads();
    }
    if (t == 0) *status = 0;
    for (int first = 0; first < G + 1; first += kRhs) {
        const int r = first + t;                  // right-hand side of this lane
        const bool live = t < kRhs && r < G + 1;
        if (live) {
            const double* rhs = r ? b + (size_t)(r - 1) * n : nullptr;
            for (int i = 0; i < n; ++i) {
                double s = rhs ? rhs[i] : 1.0;
                for (int j = 0; j < i; ++j) s -= L[i * kLd + j] * xs[j][t];
                xs[i][t] = s / L[i * kLd + i];
            }
            for (int i = n - 1; i >= 0; --i) {
                double s = xs[i][t];
                for (int j = i + 1; j < n; ++j) s -= L[j * kLd + i] * xs[j][t];
                xs[i][t] = s / L[i * kLd + i];
            }
        }
        if (first == 0) {
            if (t == 0) {
                double sy = 0.0;
                for (int i = 0; i < n; ++i) {
                    yv[i] = xs[i][0];
                    sy += xs[i][0];
                }
                sh_sy = sy;
            }
            __syncthreads();
        }
        if (live && r) {
            double sx = 0.0;
            for (int i = 0; i < n; ++i) sx += xs[i][t];
            const double c = (sx - delta[r - 1]) / sh_sy;
            for (int i = 0; i < n; ++i) phi[(size_t)(r - 1) * n + i] = xs[i][t] - yv[i] * c;
        }
    }
}

struct Scratch {
    void* partA;
    double *partB, *partW;
    size_t bytes;
};

Scratch carve(void* base, long long M, int n, int G) {
    const Chunks ch = chunks_of(M);
    iq::Carver c(base);
    Scratch s;
    s.partA = c.take<double>((size_t)ch.count * n * n);
    s.partB = c.take<double>((size_t)G * ch.count * n);
    s.partW = c.take<double>((size_t)ch.count);
    s.bytes = c.bytes();
    return s;
}

}  // namespace

extern "C" size_t iq_kshap_scratch_bytes(int M, int n, int G) {
    return iq::kshap::rows_ok(M, n, G, kMaxN) ? carve(nullptr, M, n, G).bytes : 0;
}

extern "C" int iq_kshap_keep_masks(const int32_t* orders, const int32_t* sizes, uint64_t* keep, int S, int n, int paired,
                                   int32_t* status, iq_stream_t stream) {
    IQ_REQUIRE(n >= 2 && n <= kMaxN, "iq_kshap_keep_masks: n=%d is outside 2..%d", n, kMaxN);
    IQ_REQUIRE(S >= 0 && S <= (1 << 29), "iq_kshap_keep_masks: S=%d", S);
    if (S == 0) return IQ_OK;
    IQ_REQUIRE(orders && sizes && keep && status, "iq_kshap_keep_masks: null pointer");
    IQ_LAUNCH(kshap_keep_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, iq::as_stream(stream), orders, sizes,
              reinterpret_cast<unsigned long long*>(keep), S, n, paired ? 1 : 0, status);
    return IQ_OK;
}

extern "C" int iq_kshap_accum(const uint64_t* keep, const float* v, const double* v0, const double* weights, int M, int n, int G,
                              double* A, double* b, double* wsum, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(iq::kshap::rows_ok(M, n, G, kMaxN), "iq_kshap_accum: M=%d, n=%d, G=%d (1 <= M <= 2^30, 2 <= n <= %d, 1 <= G <= 65535)", M, n, G, kMaxN);
    IQ_REQUIRE(keep && v && v0 && A && b && wsum && scratch, "iq_kshap_accum: null pointer");
    const Scratch s = carve(scratch, M, n, G);
    IQ_TRY(iq::kshap::scratch_ok("iq_kshap_accum", scratch, scratch_bytes, s.bytes));
    const Chunks ch = chunks_of(M);
    hipStream_t st = iq::as_stream(stream);
    const unsigned long long* k = reinterpret_cast<const unsigned long long*>(keep);
    if (weights)
        IQ_LAUNCH(kshap_gram_kernel<double>, dim3(ch.count), dim3(kThreads), 0, st, k, weights, M, n, ch.tiles_per,
                  static_cast<double*>(s.partA), s.partW);
    else
        IQ_LAUNCH(kshap_gram_kernel<unsigned long long>, dim3(ch.count), dim3(kThreads), 0, st, k, nullptr, M, n,
                  ch.tiles_per, static_cast<unsigned long long*>(s.partA), nullptr);
    IQ_LAUNCH(kshap_moment_kernel, dim3(ch.count, G), dim3(kThreads), 0, st, k, v, v0, weights, M, n, ch.tiles_per, s.partB);
    const int outputs = n * n + G * n + 1;
    IQ_LAUNCH(kshap_fold_kernel, dim3((outputs + kThreads - 1) / kThreads), dim3(kThreads), 0, st, (const void*)s.partA,
              (const double*)s.partB, (const double*)s.partW, weights ? 1 : 0, M, n, G, ch.count, A, b, wsum);
    return IQ_OK;
}

extern "C" int iq_kshap_solve(const double* A, const double* b, const double* delta, double* phi, int32_t* status, int n, int G,
                              iq_stream_t stream) {
    IQ_REQUIRE(n >= 2 && n <= kMaxN && G >= 1 && G <= 65535, "iq_kshap_solve: n=%d, G=%d (2 <= n <= %d, 1 <= G <= 65535)", n, G, kMaxN);
    IQ_REQUIRE(A && b && delta && phi && status, "iq_kshap_solve: null pointer");
    IQ_LAUNCH(kshap_solve_kernel, dim3(1), dim3(kThreads), 0, iq::as_stream(stream), A, b, delta, phi, status, n, G);
    return IQ_OK;
}
