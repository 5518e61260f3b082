// Control variates for the all-pairs interaction map (include/iq.h, "Control variates for the all-pairs map"): the
// 2-additive regression surrogate of a game on narrow rows, 2 <= R <= 64, and the per-row terms the residual SHAP-IQ pass
// (iq_kshap_pairs_terms[_se], csrc/iq_kshap_pairs.hip) is run on.
//
//     features  a = 0 .. d-1, d = R + R (R-1) / 2: the R singles, then the pairs (i < j) in row-major order; fm_a the feature's mask,
//               f_a(S) = [fm_a is a subset of S];
//     Gram      Gram[a][b] = #{m : fm_a | fm_b subset of S_m}: a d x d x M product over 0/1 features on v_mfma_f64_16x16x4_f64, one
//               workgroup per 64 x 64 block on or above the diagonal, mirrored when written; every entry an exact count;
//     rhs       c_g[a] = sum_m f_a(S_m) ((double)v_m - v0_g), float64 in the order of the regression estimator's moments
//               (chunks_of(M); lane = feature, rows in row order, the four waves ((0 + 1) + 2) + 3, chunks in chunk order);
//     fit       A = Gram + ridge I = L L^T, blocked (panels of 32 columns: the diagonal block in one workgroup's LDS, the panel
//               below it a row per thread, the trailing update a 32 x 32 tile per workgroup) in HBM; beta_u = A^-1 c_g and
//               w = A^-1 1 from the one factor; beta = beta_u - w (1 beta_u - delta) / (1 w);
//     surrogate g_beta(S_m) = sum_a f_a(S_m) beta_a, one thread per row, the features in index order in one chain of additions.
//
// One stream, every launch in a fixed order, every element owned by one thread, no floating-point atomics, no grid that depends on
// the data: two calls give the same bits, a game's bits depend neither on G nor on a neighbouring game's rewards.
#include "iq_common.h"
#include "iq_kshap_block.h"
#include "iq_kshap_fit.h"

// every sum is a chain of individually rounded operations: no fused multiply-add
#pragma clang fp contract(off)

namespace {

using iq::kshap::carve_fit;
using iq::kshap::Chunks;
using iq::kshap::chunks_of;
using iq::kshap::FitScratch;
using iq::kshap::kBlockElems;
using iq::kshap::kThreads;
using iq::kshap::kTile;
using iq::kshap::live_mask;
using iq::kshap::rows_ok;

constexpr int kMaxR = IQ_MAX_REGIONS;
constexpr int kMaxD = kMaxR + kMaxR * (kMaxR - 1) / 2;      // 2080
static_assert(kMaxD == iq::kshap::kFitMaxFeatures, "the solve keeps a right-hand side of the largest fit in LDS");
constexpr int kPanel = 32;                                  // columns of a Cholesky panel
constexpr int kPanelLd = kPanel + 1;
constexpr int kTrsmThreads = 128;

__host__ __device__ inline int features_of(int R) { return R + R * (R - 1) / 2; }

// fm_a: bit a for a single; bits i and j of the pair (i < j) number a - R in row-major order.  a < d.
__device__ __forceinline__ unsigned long long feature_mask(int a, int R) {
    if (a < R) return 1ull << a;
    int p = a - R, i = 0;
    while (p >= R - 1 - i) {
        p -= R - 1 - i;
        ++i;
    }
    return (1ull << i) | (1ull << (i + 1 + p));
}

// The rows of block_product for a block of the Gram matrix: a staged row is its word, bits at or above R masked, a row at or above
// M the empty set, which holds no feature; an operand is a select, (word & fm) == fm ? 1.0 : 0.0, on this lane's features.
struct GramRows {
    unsigned long long* sh_k;
    const unsigned long long* keep;
    long long M;
    unsigned long long live;
    unsigned long long ma[4], mb[4];             // this lane's features: row 16 a + col of the block, column 16 a + col
    __device__ __forceinline__ void stage(int t, long long m) const { sh_k[t] = m < M ? keep[m] & live : 0ull; }
    __device__ __forceinline__ void operands(int r, int, double (&fa)[4], double (&fb)[4]) const {
        const unsigned long long w = sh_k[r];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            fa[a] = (w & ma[a]) == ma[a] ? 1.0 : 0.0;                    // A[i = 16 a + col][k]
            fb[a] = (w & mb[a]) == mb[a] ? 1.0 : 0.0;                    // B[k][j = 16 a + col]
        }
    }
};

// Grid (block): the workgroup owns block (bi, bj), bi <= bj, blk = bj (bj + 1) / 2 + bi, of the Gram matrix and walks every row
// (iq_kshap_block.h: block_product, shared with the pairwise product Q).  Features at or above d get the mask 0 and are never
// written; a skipped tile of a diagonal block is written by its mirror image.  Sums of ones: exact in any order.
__global__ __launch_bounds__(kThreads, 2) void kshap_paircv_gram_kernel(const unsigned long long* __restrict__ keep, long long M, int R,
                                                                        int d, double* __restrict__ gram) {
    __shared__ unsigned long long sh_k[kTile];
    __shared__ double sh_acc[kBlockElems];
    const int t = threadIdx.x, col = t & 15;
    const auto [bi, bj] = iq::kshap::block_of(blockIdx.x);
    GramRows rows{sh_k, keep, M, live_mask(0, R)};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int fa = 64 * bi + 16 * a + col, fb = 64 * bj + 16 * a + col;
        rows.ma[a] = fa < d ? feature_mask(fa, R) : 0ull;
        rows.mb[a] = fb < d ? feature_mask(fb, R) : 0ull;
    }
    iq::kshap::block_product(rows, bi, bj, d, 0, (int)((M + kTile - 1) / kTile), sh_acc);
    for (int e = t; e < kBlockElems; e += kThreads) {
        const int r = e >> 6, c = e & 63, gi = 64 * bi + r, gj = 64 * bj + c;
        if (gi >= d || gj >= d) continue;
        if (bi == bj && (c >> 4) < (r >> 4)) continue;          // a skipped tile: its mirror image writes this entry
        const double x = sh_acc[e];
        gram[(size_t)gi * d + gj] = x;
        if (bi != bj || (c >> 4) > (r >> 4)) gram[(size_t)gj * d + gi] = x;
    }
}

// Grid (chunk of chunks_of(M), block of 64 features, game): part[(g * nchunk + chunk) * d + a] = the chunk's sum of
// f_a(S_m) ((double)v_m - v0): moment_chunk_of on the one word of a narrow row, lane a standing for feature a - the row is a member
// when it holds fm_a (a feature mask has no bit at or above R, so the row's own are not masked).  Lanes at or above d sum every row
// (their mask is 0) and are not written.
__global__ __launch_bounds__(kThreads) void kshap_paircv_rhs_kernel(const unsigned long long* __restrict__ keep, const float* __restrict__ v,
                                                                    const double* __restrict__ v0, long long M, int R, int d,
                                                                    int tiles_per, double* __restrict__ part) {
    const int chunk = blockIdx.x, a0 = 64 * blockIdx.y, a = a0 + (threadIdx.x & 63), g = blockIdx.z;
    const float* vg = v + (size_t)g * M;
    const double base = v0[g];
    const unsigned long long fm = a < d ? feature_mask(a, R) : 0ull;
    iq::kshap::moment_chunk_of(
        keep, 1, 0, [=](long long m, double) { return (double)vg[m] - base; }, nullptr, M, tiles_per, chunk,
        part + ((size_t)g * gridDim.x + chunk) * d + a0, min(64, d - a0), nullptr,
        [fm](unsigned long long word, int) { return (word & fm) == fm; });
}

// One thread per entry of X ((G + 1, d)): rows 0 .. G-1 the chunks' partials added in chunk order, row G the ones vector.
__global__ __launch_bounds__(kThreads) void kshap_paircv_rhs_fold_kernel(const double* __restrict__ part, int d, int G, int nchunk,
                                                                         double* __restrict__ X) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long long)(G + 1) * d) return;
    const long long g = e / d, a = e % d;
    X[e] = g < G ? iq::kshap::fold_chunks(part + (size_t)g * nchunk * d + a, d, nchunk) : 1.0;
}

// One thread per entry: A = Gram + ridge I.
__global__ __launch_bounds__(kThreads) void kshap_paircv_ridge_kernel(const double* __restrict__ gram, double ridge, int d,
                                                                      double* __restrict__ A) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long long)d * d) return;
    A[e] = e / d == e % d ? gram[e] + ridge : gram[e];
}

// One workgroup: the Cholesky factor of the diagonal block A[k0 .. k0 + nb)^2 in LDS, right-looking, a column at a time; only the
// lower triangle is read and written.  The panel at k0 = 0 first leaves *tol = d 2^-52 max_i A_ii (iq_kshap_solve's threshold; a
// maximum, whatever the order: thread t over entries t, t + 256, ..., then the 256 threads); a pivot that is not above it sets
// *status = 1 and is replaced by 1 (the caller discards the result).
__global__ __launch_bounds__(kThreads) void kshap_paircv_potrf_kernel(double* __restrict__ A, int d, int k0, int nb,
                                                                      double* __restrict__ tol, int32_t* __restrict__ status) {
    __shared__ double sh[kPanel * kPanelLd];
    __shared__ double sh_max[kThreads];
    __shared__ double sh_tol;
    const int t = threadIdx.x;
    for (int e = t; e < nb * nb; e += kThreads) {
        const int r = e / nb, c = e % nb;
        sh[r * kPanelLd + c] = c <= r ? A[(size_t)(k0 + r) * d + k0 + c] : 0.0;
    }
    if (k0 == 0) {                                // uniform: the launch's argument
        double mx = 0.0;
        for (int i = t; i < d; i += kThreads) {
            const double x = A[(size_t)i * d + i];
            mx = x > mx ? x : mx;
        }
        sh_max[t] = mx;
        __syncthreads();
        if (t == 0) {
            for (int u = 1; u < kThreads; ++u) mx = sh_max[u] > mx ? sh_max[u] : mx;
            *tol = (double)d * 0x1p-52 * mx;
        }
    }
    if (t == 0) sh_tol = *tol;
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        if (t == 0) {
            double p = sh[j * kPanelLd + j];
            if (!(p > sh_tol)) {                  // a NaN pivot too
                *status = 1;
                p = 1.0;
            }
            sh[j * kPanelLd + j] = sqrt(p);
        }
        __syncthreads();
        if (t > j && t < nb) sh[t * kPanelLd + j] = sh[t * kPanelLd + j] / sh[j * kPanelLd + j];
        __syncthreads();
        for (int e = t; e < nb * nb; e += kThreads) {
            const int r = e / nb, c = e % nb;
            if (c > j && r >= c) sh[r * kPanelLd + c] = sh[r * kPanelLd + c] - sh[r * kPanelLd + j] * sh[c * kPanelLd + j];
        }
        __syncthreads();
    }
    for (int e = t; e < nb * nb; e += kThreads) {
        const int r = e / nb, c = e % nb;
        if (c <= r) A[(size_t)(k0 + r) * d + k0 + c] = sh[r * kPanelLd + c];
    }
}

// The panel below a factored diagonal block of kPanel columns: one thread per row i >= k0 + kPanel solves x L11^T = A[i][k0 ..] for
// its row in registers, column by column, the earlier columns subtracted in column order.
__global__ __launch_bounds__(kTrsmThreads) void kshap_paircv_trsm_kernel(double* __restrict__ A, int d, int k0) {
    __shared__ double sh[kPanel * kPanelLd];
    const int t = threadIdx.x;
    for (int e = t; e < kPanel * kPanel; e += kTrsmThreads) {
        const int r = e / kPanel, c = e % kPanel;
        sh[r * kPanelLd + c] = A[(size_t)(k0 + r) * d + k0 + c];
    }
    __syncthreads();
    const int i = k0 + kPanel + blockIdx.x * kTrsmThreads + t;
    if (i >= d) return;
    double* row = A + (size_t)i * d + k0;
    double x[kPanel];
#pragma unroll
    for (int c = 0; c < kPanel; ++c) x[c] = row[c];
#pragma unroll
    for (int c = 0; c < kPanel; ++c) {
        double s = x[c];
#pragma unroll
        for (int p = 0; p < c; ++p) s = s - x[p] * sh[c * kPanelLd + p];
        x[c] = s / sh[c * kPanelLd + c];
    }
#pragma unroll
    for (int c = 0; c < kPanel; ++c) row[c] = x[c];
}

// The trailing update behind a panel of kPanel columns at k0: A[i][j] -= sum_p L[i][k0 + p] L[j][k0 + p], p in order, for
// k1 = k0 + kPanel <= j <= i < d.  Grid (tile row, tile column) of 32 x 32 tiles; tiles above the diagonal leave at once.  Thread
// (ty, tx) owns rows ty, ty + 8, ty + 16, ty + 24 of column tx.
__global__ __launch_bounds__(kThreads) void kshap_paircv_syrk_kernel(double* __restrict__ A, int d, int k0) {
    __shared__ double sh_i[kPanel * kPanelLd], sh_j[kPanel * kPanelLd];
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5, k1 = k0 + kPanel;
    for (int e = t; e < kPanel * kPanel; e += kThreads) {
        const int r = e / kPanel, p = e % kPanel, gi = k1 + 32 * bi + r, gj = k1 + 32 * bj + r;
        sh_i[r * kPanelLd + p] = gi < d ? A[(size_t)gi * d + k0 + p] : 0.0;
        sh_j[r * kPanelLd + p] = gj < d ? A[(size_t)gj * d + k0 + p] : 0.0;
    }
    __syncthreads();
    const int j = k1 + 32 * bj + tx;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = ty + 8 * k, i = k1 + 32 * bi + r;
        if (i >= d || j > i) continue;
        double s = A[(size_t)i * d + j];
#pragma unroll 8
        for (int p = 0; p < kPanel; ++p) s = s - sh_i[r * kPanelLd + p] * sh_j[tx * kPanelLd + p];
        A[(size_t)i * d + j] = s;
    }
}

// Grid (right-hand side): one workgroup solves L y = x, then L^T x = y for row blockIdx.x of X, the vector in LDS, panel by panel:
// the diagonal block a column at a time, then the rest of the vector, a thread per entry, the panel's columns in order.
__global__ __launch_bounds__(kThreads) void kshap_paircv_solve_kernel(const double* __restrict__ A, int d, double* __restrict__ X) {
    __shared__ double y[kMaxD];
    __shared__ double sh[kPanel * kPanelLd];
    const int t = threadIdx.x;
    double* x = X + (size_t)blockIdx.x * d;
    for (int a = t; a < d; a += kThreads) y[a] = x[a];
    __syncthreads();
    for (int k0 = 0; k0 < d; k0 += kPanel) {
        const int nb = min(kPanel, d - k0);
        for (int e = t; e < nb * nb; e += kThreads) {
            const int r = e / nb, c = e % nb;
            sh[r * kPanelLd + c] = c <= r ? A[(size_t)(k0 + r) * d + k0 + c] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < nb; ++c) {
            if (t == c) y[k0 + c] = y[k0 + c] / sh[c * kPanelLd + c];
            __syncthreads();
            if (t > c && t < nb) y[k0 + t] = y[k0 + t] - sh[t * kPanelLd + c] * y[k0 + c];
            __syncthreads();
        }
        for (int i = k0 + nb + t; i < d; i += kThreads) {
            const double* row = A + (size_t)i * d + k0;
            double s = y[i];
            for (int p = 0; p < nb; ++p) s = s - row[p] * y[k0 + p];
            y[i] = s;
        }
        __syncthreads();
    }
    for (int k0 = (d - 1) / kPanel * kPanel; k0 >= 0; k0 -= kPanel) {
        const int nb = min(kPanel, d - k0);
        for (int e = t; e < nb * nb; e += kThreads) {
            const int r = e / nb, c = e % nb;
            sh[r * kPanelLd + c] = c <= r ? A[(size_t)(k0 + r) * d + k0 + c] : 0.0;
        }
        __syncthreads();
        for (int c = nb - 1; c >= 0; --c) {
            if (t == c) y[k0 + c] = y[k0 + c] / sh[c * kPanelLd + c];
            __syncthreads();
            if (t < c) y[k0 + t] = y[k0 + t] - sh[c * kPanelLd + t] * y[k0 + c];
            __syncthreads();
        }
        for (int i = t; i < k0; i += kThreads) {
            double s = y[i];
            for (int p = 0; p < nb; ++p) s = s - A[(size_t)(k0 + p) * d + i] * y[k0 + p];
            y[i] = s;
        }
        __syncthreads();
    }
    for (int a = t; a < d; a += kThreads) x[a] = y[a];
}

// Grid (game): beta = beta_u - w ((1 beta_u - delta) / (1 w)), beta_u row g and w row G of X.  Both sums: per thread over its
// entries t, t + 256, ... in order, then the 256 threads in index order.
__global__ __launch_bounds__(kThreads) void kshap_paircv_constrain_kernel(const double* __restrict__ X, const double* __restrict__ delta,
                                                                          int d, int G, double* __restrict__ beta) {
    __shared__ double sh[kThreads];
    __shared__ double sh_lambda;
    const int t = threadIdx.x, g = blockIdx.x;
    const double *bu = X + (size_t)g * d, *w = X + (size_t)G * d;
    double sb = 0.0, sw = 0.0;
    for (int a = t; a < d; a += kThreads) {
        sb += bu[a];
        sw += w[a];
    }
    const double tb = iq::kshap::sum_threads_in_order(sh, sb);
    __syncthreads();
    const double tw = iq::kshap::sum_threads_in_order(sh, sw);
    if (t == 0) sh_lambda = (tb - delta[g]) / tw;
    __syncthreads();
    const double lambda = sh_lambda;
    for (int a = t; a < d; a += kThreads) beta[(size_t)g * d + a] = bu[a] - w[a] * lambda;
}

// Grid (M / 256, game), one thread per row: g_beta(S_m) = the betas of the features the row holds, added in index order in one
// chain starting from 0 (singles, then the pairs (i < j) row-major); beta of the game in LDS.  out_g[g][m] = g_beta(S_m); with v,
// out_t[g][m] = ((double)v_m - v0) - g_beta(S_m).  Either output may be null.
__global__ __launch_bounds__(kThreads) void kshap_paircv_surrogate_kernel(const unsigned long long* __restrict__ keep,
                                                                          const double* __restrict__ beta, const float* __restrict__ v,
                                                                          const double* __restrict__ v0, long long M, int R, int d,
                                                                          double* __restrict__ out_g, double* __restrict__ out_t) {
    __shared__ double sh_beta[kMaxD];
    const int t = threadIdx.x, g = blockIdx.y;
    for (int a = t; a < d; a += kThreads) sh_beta[a] = beta[(size_t)g * d + a];
    __syncthreads();
    const long long m = (long long)blockIdx.x * kThreads + t;
    if (m >= M) return;
    const unsigned long long k = keep[m] & live_mask(0, R);
    double acc = 0.0;
    for (int i = 0; i < R; ++i)
        if ((k >> i) & 1ull) acc += sh_beta[i];
    int a = R;
    for (int i = 0; i < R; ++i) {
        if ((k >> i) & 1ull)
            for (int j = i + 1; j < R; ++j)
                if ((k >> j) & 1ull) acc += sh_beta[a + j - i - 1];
        a += R - 1 - i;
    }
    if (out_g) out_g[(size_t)g * M + m] = acc;
    if (out_t) out_t[(size_t)g * M + m] = ((double)v[(size_t)g * M + m] - v0[g]) - acc;
}

// Grid (M / 256, game), one thread per row of W words: t[g][m] = ((double)v_m - v0) - (delta (double)s_m) / (double)R, s_m the
// regions below R the row keeps.
__global__ __launch_bounds__(kThreads) void kshap_paircv_shift_kernel(const unsigned long long* __restrict__ keep, const float* __restrict__ v,
                                                                      const double* __restrict__ v0, const double* __restrict__ delta,
                                                                      long long M, int R, int W, double* __restrict__ out) {
    const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int g = blockIdx.y;
    if (m >= M) return;
    const int s = iq::kshap::row_size(keep + (size_t)m * W, W, R);
    out[(size_t)g * M + m] = ((double)v[(size_t)g * M + m] - v0[g]) - (delta[g] * (double)s) / (double)R;
}

unsigned blocks_for(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

int iq::kshap::fit_from_partials(const char* copy_what, const double* gram, const double* delta, double ridge, int d, int G, int nchunk,
                                 const FitScratch& s, double* beta, double* solves, int32_t* status, hipStream_t st) {
    IQ_LAUNCH(kshap_paircv_rhs_fold_kernel, dim3(blocks_for((long long)(G + 1) * d)), dim3(kThreads), 0, st, (const double*)s.part, d, G,
              nchunk, s.X);
    IQ_LAUNCH(kshap_paircv_ridge_kernel, dim3(blocks_for((long long)d * d)), dim3(kThreads), 0, st, gram, ridge, d, s.A);
    for (int k0 = 0; k0 < d; k0 += kPanel) {
        const int nb = d - k0 < kPanel ? d - k0 : kPanel, rest = d - k0 - nb;
        IQ_LAUNCH(kshap_paircv_potrf_kernel, dim3(1), dim3(kThreads), 0, st, s.A, d, k0, nb, s.tol, status);
        if (rest > 0) {                           // nb == kPanel here
            const int tiles = (rest + kPanel - 1) / kPanel;
            IQ_LAUNCH(kshap_paircv_trsm_kernel, dim3((rest + kTrsmThreads - 1) / kTrsmThreads), dim3(kTrsmThreads), 0, st, s.A, d, k0);
            IQ_LAUNCH(kshap_paircv_syrk_kernel, dim3(tiles, tiles), dim3(kThreads), 0, st, s.A, d, k0);
        }
    }
    IQ_LAUNCH(kshap_paircv_solve_kernel, dim3(G + 1), dim3(kThreads), 0, st, (const double*)s.A, d, s.X);
    if (solves)
        IQ_TRY(iq::hip_ok(hipMemcpyAsync(solves, s.X, (size_t)(G + 1) * d * sizeof(double), hipMemcpyDeviceToDevice, st), copy_what));
    IQ_LAUNCH(kshap_paircv_constrain_kernel, dim3(G), dim3(kThreads), 0, st, (const double*)s.X, delta, d, G, beta);
    return IQ_OK;
}

extern "C" int iq_kshap_pair_features(int R) { return R >= 2 && R <= kMaxR ? features_of(R) : 0; }

extern "C" int iq_kshap_pair_gram(const uint64_t* keep, int M, int R, double* gram, iq_stream_t stream) {
    IQ_REQUIRE(rows_ok(M, R, 1, kMaxR), "iq_kshap_pair_gram: M=%d, R=%d (1 <= M <= 2^30, 2 <= R <= %d)", M, R, kMaxR);
    IQ_REQUIRE(keep && gram, "iq_kshap_pair_gram: null pointer");
    const int d = features_of(R);
    IQ_LAUNCH(kshap_paircv_gram_kernel, dim3(iq::kshap::blocks_of(d)), dim3(kThreads), 0, iq::as_stream(stream),
              reinterpret_cast<const unsigned long long*>(keep), (long long)M, R, d, gram);
    return IQ_OK;
}

extern "C" size_t iq_kshap_pair_fit_scratch_bytes(int M, int R, int G) { return rows_ok(M, R, G, kMaxR) ? carve_fit(nullptr, M, features_of(R), G).bytes : 0; }

extern "C" int iq_kshap_pair_fit(const double* gram, const uint64_t* keep, const float* v, const double* v0, const double* delta,
                                 double ridge, int M, int R, int G, double* beta, double* solves, int32_t* status, void* scratch,
                                 size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(rows_ok(M, R, G, kMaxR), "iq_kshap_pair_fit: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G, kMaxR);
    IQ_REQUIRE(ridge >= 0.0, "iq_kshap_pair_fit: ridge must be a number >= 0");
    IQ_REQUIRE(gram && keep && v && v0 && delta && beta && status && scratch, "iq_kshap_pair_fit: null pointer");
    const FitScratch s = carve_fit(scratch, M, features_of(R), G);
    IQ_TRY(iq::kshap::scratch_ok("iq_kshap_pair_fit", scratch, scratch_bytes, s.bytes));
    hipStream_t st = iq::as_stream(stream);
    const unsigned long long* k = reinterpret_cast<const unsigned long long*>(keep);
    const int d = features_of(R);
    const Chunks ch = chunks_of(M);
    IQ_TRY(iq::hip_ok(hipMemsetAsync(status, 0, sizeof(int32_t), st), "iq_kshap_pair_fit: clearing the status word"));
    IQ_LAUNCH(kshap_paircv_rhs_kernel, dim3(ch.count, (d + 63) / 64, G), dim3(kThreads), 0, st, k, v, v0, (long long)M, R, d, ch.tiles_per,
              s.part);
    IQ_TRY(iq::kshap::fit_from_partials("iq_kshap_pair_fit: copying the solves", gram, delta, ridge, d, G, ch.count, s, beta, solves, status, st));
    return IQ_OK;
}

extern "C" int iq_kshap_pair_surrogate(const uint64_t* keep, const double* beta, const float* v, const double* v0, int M, int R, int G,
                                       double* out_g, double* out_t, iq_stream_t stream) {
    IQ_REQUIRE(rows_ok(M, R, G, kMaxR), "iq_kshap_pair_surrogate: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G,
               kMaxR);
    IQ_REQUIRE(keep && beta && (out_g || out_t) && (!out_t || (v && v0)), "iq_kshap_pair_surrogate: null pointer");
    IQ_LAUNCH(kshap_paircv_surrogate_kernel, dim3(blocks_for(M), G), dim3(kThreads), 0, iq::as_stream(stream),
              reinterpret_cast<const unsigned long long*>(keep), beta, v, v0, (long long)M, R, features_of(R), out_g, out_t);
    return IQ_OK;
}

extern "C" int iq_kshap_pair_shift_terms(const uint64_t* keep, const float* v, const double* v0, const double* delta, int M, int R, int G,
                                         double* t, iq_stream_t stream) {
    IQ_REQUIRE(rows_ok(M, R, G, IQ_MAX_WIDE_REGIONS),
               "iq_kshap_pair_shift_terms: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G, IQ_MAX_WIDE_REGIONS);
    IQ_REQUIRE(keep && v && v0 && delta && t, "iq_kshap_pair_shift_terms: null pointer");
    IQ_LAUNCH(kshap_paircv_shift_kernel, dim3(blocks_for(M), G), dim3(kThreads), 0, iq::as_stream(stream),
              reinterpret_cast<const unsigned long long*>(keep), v, v0, delta, (long long)M, R, iq::keep_words(R), t);
    return IQ_OK;
}
