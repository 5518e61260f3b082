// The sparse regression control variate of the all-pairs map (include/iq.h, "Sparse regression control variate"): a
// 2-additive surrogate with all R singles and a caller-chosen list of K pairs, d = R + K <= 2080, on narrow or wide rows of
// 2 .. 1024 regions.  Everything works on FEATURE ROWS: row m expanded into its d feature bits, ceil(d / 64) words.
//
//     expand    bit a of feat[m] = f_a(S_m): a single's own bit, a listed pair's two bits; one thread per (row, word of the feature row);
//     Gram      Gram[a][b] = #{m : bits a and b of feat[m]}: block_product (iq_kshap_block.h) on v_mfma_f64_16x16x4_f64, one workgroup
//               per 64 x 64 block on or above the diagonal walking every row, mirrored when written; every entry an exact count;
//     rhs       c_g[a] = sum_m f_a(S_m) ((double)v_m - v0_g): moment_chunk_of on word a / 64 of the feature rows, lane = feature,
//               chunks_of(M) - the order of kshap_paircv_rhs_kernel; then fit_from_partials (iq_kshap_fit.h): the fold, ridge,
//               factor, solves and constraint of iq_kshap_pair_fit, the same instances;
//     surrogate g_beta(S_m) = the betas of the set bits of feat[m], added in index order in one chain starting from 0.
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

constexpr int kMaxD = IQ_KSHAP_SPARSE_MAX_FEATURES;
static_assert(kMaxD == iq::kshap::kFitMaxFeatures, "the fit is built for at most this many features");

inline int feat_words(int d) { return (d + 63) >> 6; }

inline bool feat_ok(long long M, int d, int G) { return M >= 1 && M <= (1ll << 30) && d >= 2 && d <= kMaxD && G >= 1 && G <= 65535; }

// Grid (M / 256, word of the feature row), one thread per (row, word): bit b of the word is feature a = 64 word + b - below R the
// row's own bit a, then pair a - R of the list when 0 <= i < j < R (any other entry is a feature that no row holds: no index is
// formed from it), at or above d nothing.  The 64 list entries of the word are staged in LDS once.
__global__ __launch_bounds__(kThreads) void kshap_sparsecv_expand_kernel(const unsigned long long* __restrict__ keep,
                                                                         const int32_t* __restrict__ pairs, long long M, int R, int K,
                                                                         int W, int Wd, unsigned long long* __restrict__ feat) {
    __shared__ int sh_i[64], sh_j[64];
    const int t = threadIdx.x, word = blockIdx.y, a0 = 64 * word, d = R + K;
    if (t < 64) {
        const int k = a0 + t - R;
        int i = -1, j = -1;
        if (k >= 0 && k < K) {
            i = pairs[2 * (size_t)k];
            j = pairs[2 * (size_t)k + 1];
            if (!(i >= 0 && i < j && j < R)) i = j = -1;
        }
        sh_i[t] = i;
        sh_j[t] = j;
    }
    __syncthreads();
    const long long m = (long long)blockIdx.x * kThreads + t;
    if (m >= M) return;
    const unsigned long long* row = keep + (size_t)m * W;
    unsigned long long out = 0ull;
    if (a0 < R) out = row[word] & live_mask(word, R);             // the singles of this word: word < W here
    const int b0 = a0 < R ? min(64, R - a0) : 0, b1 = min(64, d - a0);
    for (int b = b0; b < b1; ++b) {
        const int i = sh_i[b], j = sh_j[b];
        if (i < 0) continue;
        const unsigned long long both = (row[i >> 6] >> (i & 63)) & (row[j >> 6] >> (j & 63)) & 1ull;
        out |= both << b;
    }
    feat[(size_t)m * Wd + word] = out;
}

// The rows of block_product for block (bi, bj) of the Gram matrix of feature rows: a staged row is its words bi and bj, bits at or
// above d masked, a row at or above M one that holds nothing (PairRows of iq_kshap_pairs.hip with e = 1); an operand is a select.
struct FeatRows {
    unsigned long long *sh_a, *sh_b;
    const unsigned long long* feat;
    long long M;
    int Wd, bi, bj;
    unsigned long long mask_a, mask_b;
    __device__ __forceinline__ void stage(int t, long long m) const {
        unsigned long long ka = 0ull, kb = 0ull;
        if (m < M) {
            ka = feat[(size_t)m * Wd + bi] & mask_a;
            kb = feat[(size_t)m * Wd + bj] & mask_b;
        }
        sh_a[t] = ka;
        sh_b[t] = kb;
    }
    __device__ __forceinline__ void operands(int r, int col, double (&fa)[4], double (&fb)[4]) const {
        const unsigned long long wa = sh_a[r] >> col, wb = sh_b[r] >> col;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            fa[a] = (wa >> (16 * a)) & 1ull ? 1.0 : 0.0;          // A[i = 16 a + col][k]
            fb[a] = (wb >> (16 * a)) & 1ull ? 1.0 : 0.0;          // B[k][j = 16 a + col]
        }
    }
};

// Grid (block): the workgroup owns block (bi, bj), bi <= bj, blk = bj (bj + 1) / 2 + bi, and walks every row; a skipped tile of a
// diagonal block is written by its mirror image.  Sums of ones: exact in any order.
__global__ __launch_bounds__(kThreads, 2) void kshap_sparsecv_gram_kernel(const unsigned long long* __restrict__ feat, long long M, int d,
                                                                          int Wd, double* __restrict__ gram) {
    __shared__ unsigned long long sh_a[kTile], sh_b[kTile];
    __shared__ double sh_acc[kBlockElems];
    const int t = threadIdx.x;
    const auto [bi, bj] = iq::kshap::block_of(blockIdx.x);
    const FeatRows rows{sh_a, sh_b, feat, M, Wd, bi, bj, live_mask(bi, d), live_mask(bj, d)};
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
// f_a(S_m) ((double)v_m - v0): moment_chunk_of on word blockIdx.y of the feature rows, lane b standing for feature 64 word + b.
__global__ __launch_bounds__(kThreads) void kshap_sparsecv_rhs_kernel(const unsigned long long* __restrict__ feat, const float* __restrict__ v,
                                                                      const double* __restrict__ v0, long long M, int d, int Wd,
                                                                      int tiles_per, double* __restrict__ part) {
    const int chunk = blockIdx.x, word = blockIdx.y, g = blockIdx.z;
    const float* vg = v + (size_t)g * M;
    const double base = v0[g];
    iq::kshap::moment_chunk_of(
        feat, Wd, word, [=](long long m, double) { return (double)vg[m] - base; }, nullptr, M, tiles_per, chunk,
        part + ((size_t)g * gridDim.x + chunk) * d + 64 * word, min(64, d - 64 * word), nullptr);
}

// Grid (M / 256, game), one thread per row: the betas of the row's set feature bits below d, added in index order in one chain
// starting from 0; beta of the game in LDS.  out_g[g][m] = g_beta(S_m); with v, out_t[g][m] = ((double)v_m - v0) - g_beta(S_m).
__global__ __launch_bounds__(kThreads) void kshap_sparsecv_surrogate_kernel(const unsigned long long* __restrict__ feat,
                                                                            const double* __restrict__ beta, const float* __restrict__ v,
                                                                            const double* __restrict__ v0, long long M, int d, int Wd,
                                                                            double* __restrict__ out_g, double* __restrict__ out_t) {
    __shared__ double sh_beta[kMaxD];
    const int t = threadIdx.x, g = blockIdx.y;
    for (int a = t; a < d; a += kThreads) sh_beta[a] = beta[(size_t)g * d + a];
    __syncthreads();
    const long long m = (long long)blockIdx.x * kThreads + t;
    if (m >= M) return;
    double acc = 0.0;
    for (int w = 0; w < Wd; ++w) {
        unsigned long long bits = feat[(size_t)m * Wd + w] & live_mask(w, d);
        while (bits) {
            acc += sh_beta[64 * w + __builtin_ctzll(bits)];
            bits &= bits - 1ull;
        }
    }
    if (out_g) out_g[(size_t)g * M + m] = acc;
    if (out_t) out_t[(size_t)g * M + m] = ((double)v[(size_t)g * M + m] - v0[g]) - acc;
}

unsigned blocks_for(long long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" int iq_kshap_sparse_expand(const uint64_t* keep, const int32_t* pairs, int M, int R, int K, uint64_t* feat, iq_stream_t stream) {
    IQ_REQUIRE(iq::kshap::rows_ok(M, R, 1, IQ_MAX_WIDE_REGIONS) && K >= 0 && K <= kMaxD - R,
               "iq_kshap_sparse_expand: M=%d, R=%d, K=%d (1 <= M <= 2^30, 2 <= R <= %d, 0 <= K, R + K <= %d)", M, R, K, IQ_MAX_WIDE_REGIONS,
               kMaxD);
    IQ_REQUIRE(keep && feat && (pairs || K == 0), "iq_kshap_sparse_expand: null pointer");
    const int Wd = feat_words(R + K);
    IQ_LAUNCH(kshap_sparsecv_expand_kernel, dim3(blocks_for(M), Wd), dim3(kThreads), 0, iq::as_stream(stream),
              reinterpret_cast<const unsigned long long*>(keep), pairs, (long long)M, R, K, iq::keep_words(R), Wd,
              reinterpret_cast<unsigned long long*>(feat));
    return IQ_OK;
}

extern "C" int iq_kshap_feat_gram(const uint64_t* feat, int M, int d, double* gram, iq_stream_t stream) {
    IQ_REQUIRE(feat_ok(M, d, 1), "iq_kshap_feat_gram: M=%d, d=%d (1 <= M <= 2^30, 2 <= d <= %d)", M, d, kMaxD);
    IQ_REQUIRE(feat && gram, "iq_kshap_feat_gram: null pointer");
    IQ_LAUNCH(kshap_sparsecv_gram_kernel, dim3(iq::kshap::blocks_of(d)), dim3(kThreads), 0, iq::as_stream(stream),
              reinterpret_cast<const unsigned long long*>(feat), (long long)M, d, feat_words(d), gram);
    return IQ_OK;
}

extern "C" size_t iq_kshap_feat_fit_scratch_bytes(int M, int d, int G) { return feat_ok(M, d, G) ? carve_fit(nullptr, M, d, G).bytes : 0; }

extern "C" int iq_kshap_feat_fit(const double* gram, const uint64_t* feat, const float* v, const double* v0, const double* delta,
                                 double ridge, int M, int d, int G, double* beta, double* solves, int32_t* status, void* scratch,
                                 size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(feat_ok(M, d, G), "iq_kshap_feat_fit: M=%d, d=%d, G=%d (1 <= M <= 2^30, 2 <= d <= %d, 1 <= G <= 65535)", M, d, G, kMaxD);
    IQ_REQUIRE(ridge >= 0.0, "iq_kshap_feat_fit: ridge must be a number >= 0");
    IQ_REQUIRE(gram && feat && v && v0 && delta && beta && status && scratch, "iq_kshap_feat_fit: null pointer");
    const FitScratch s = carve_fit(scratch, M, d, G);
    IQ_TRY(iq::kshap::scratch_ok("iq_kshap_feat_fit", scratch, scratch_bytes, s.bytes));
    hipStream_t st = iq::as_stream(stream);
    const Chunks ch = chunks_of(M);
    const int Wd = feat_words(d);
    IQ_TRY(iq::hip_ok(hipMemsetAsync(status, 0, sizeof(int32_t), st), "iq_kshap_feat_fit: clearing the status word"));
    IQ_LAUNCH(kshap_sparsecv_rhs_kernel, dim3(ch.count, Wd, G), dim3(kThreads), 0, st, reinterpret_cast<const unsigned long long*>(feat), v,
              v0, (long long)M, d, Wd, ch.tiles_per, s.part);
    IQ_TRY(iq::kshap::fit_from_partials("iq_kshap_feat_fit: copying the solves", gram, delta, ridge, d, G, ch.count, s, beta, solves, status, st));
    return IQ_OK;
}

extern "C" int iq_kshap_feat_surrogate(const uint64_t* feat, const double* beta, const float* v, const double* v0, int M, int d, int G,
                                       double* out_g, double* out_t, iq_stream_t stream) {
    IQ_REQUIRE(feat_ok(M, d, G), "iq_kshap_feat_surrogate: M=%d, d=%d, G=%d (1 <= M <= 2^30, 2 <= d <= %d, 1 <= G <= 65535)", M, d, G,
               kMaxD);
    IQ_REQUIRE(feat && beta && (out_g || out_t) && (!out_t || (v && v0)), "iq_kshap_feat_surrogate: null pointer");
    IQ_LAUNCH(kshap_sparsecv_surrogate_kernel, dim3(blocks_for(M), G), dim3(kThreads), 0, iq::as_stream(stream),
              reinterpret_cast<const unsigned long long*>(feat), beta, v, v0, (long long)M, d, feat_words(d), out_g, out_t);
    return IQ_OK;
}
