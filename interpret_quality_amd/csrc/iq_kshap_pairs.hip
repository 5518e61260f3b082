// The pairwise Shapley interaction index (SII) of ALL pairs of regions from the rows of the regression estimator (SHAP-IQ), for
// narrow rows (W = 1) and wide rows alike, 2 <= R <= IQ_MAX_WIDE_REGIONS.  include/iq.h, "All-pairs interactions from the
// regression rows", has the estimator; DESIGN.md 5h the reasoning.
//
//     I_ij = delta / (R - 1) + (A + L_i + L_j + Q_ij) / W_sum,
//     A = sum d_m alpha_s,   L_i = sum (d_m beta_s) z_mi,   Q_ij = sum (d_m gamma_s) z_mi z_mj,   s = popcount(z_m),
// d_m = w_m ((double)v_m - v0) and (alpha, beta, gamma) the (R+1, 3) table of the host (kernelshap.pair_coefficients).
//
// Q is the hot part, an R x R x M product over 0/1 rows, on v_mfma_f64_16x16x4_f64.  A workgroup owns one 64 x 64 block of Q on or
// above the diagonal (word bi of the rows against word bj), one chunk of rows and one game; its four waves take rows
// 64 q .. 64 q + 63 of every 256-row tile (iq_kshap_block.h: block_product, shared with the surrogate's Gram matrix).  Operands are
// made in registers from the staged words: A = bit ? e_m : 0.0 with e_m = d_m gamma_s, B = bit ? 1.0 : 0.0 - selects, never a
// product, so a row's e_m reaches only the pairs the row holds.  Ragged R and ragged M are zero operands (bits at or above R are
// masked when the tile is staged, rows at or above M are staged as 0).  The rows' sizes are counted once, by a kernel of their own,
// into scratch: 136 blocks at R = 1024 would otherwise each re-read every word of every row.
//
// Order: block_product's within a chunk, the chunks - pair_chunks_of(M, R), a function of (M, R) alone - in chunk order by the
// assemble kernel.  L, A and W_sum take the order of the regression estimator's moments (iq_kshap_order.h: moment_chunk_of,
// scalar_chunk_of, fold_moments_kernel) on chunks_of(M).  No floating-point atomics; a game's sums never meet another's.
//
// iq_kshap_pairs_se (below the assemble kernel; include/iq.h, "Standard errors of the sampled estimates") adds the
// standard error of every entry from the second moment of the same rows: the same product body once more, over the iid units.
#include "iq_common.h"
#include "iq_kshap_block.h"

// every sum and the assembly of I_ij are chains of individually rounded operations: no fused multiply-add
#pragma clang fp contract(off)

namespace {

using iq::kshap::blocks_of;
using iq::kshap::Chunks;
using iq::kshap::chunks_of;
using iq::kshap::kBlock;
using iq::kshap::kBlockElems;
using iq::kshap::kThreads;
using iq::kshap::kTile;
using iq::kshap::live_mask;
using iq::kshap::pair_chunks_of;
using iq::kshap::rows_ok;

constexpr int kMaxR = IQ_MAX_WIDE_REGIONS;

// d times column k of the coefficient table at size s; a row of size 0 or R contributes 0 whatever its reward
__device__ __forceinline__ double row_term(double d, int s, int R, const double* __restrict__ coef, int k) {
    return (s <= 0 || s >= R) ? 0.0 : d * coef[3 * s + k];
}

// What a row contributes before its weight, d_m of game g: the reward's difference (double)v_m - v0 of the estimator's own entries, or
// a float64 term t_m the caller made (iq_kshap_pairs_terms: include/iq.h, "Control variates for the all-pairs map").  of(g, M) is
// game g's view of the (G, M) array; the kernels below are written once over either.
struct RewardDiff {
    const float* v;
    const double* v0;
    struct Game {
        const float* vg;
        double base;
        __device__ __forceinline__ double operator()(long long m) const { return (double)vg[m] - base; }
    };
    __device__ __forceinline__ Game of(int g, long long M) const { return {v + (size_t)g * M, v0[g]}; }
};

struct TermDiff {
    const double* t;
    struct Game {
        const double* tg;
        __device__ __forceinline__ double operator()(long long m) const { return tg[m]; }
    };
    __device__ __forceinline__ Game of(int g, long long M) const { return {t + (size_t)g * M}; }
};

// One thread per row: sizes[m] = the number of regions below R that row m keeps.
__global__ __launch_bounds__(kThreads) void kshap_pairs_sizes_kernel(const unsigned long long* __restrict__ keep, long long M, int R,
                                                                     int W, unsigned short* __restrict__ sizes) {
    const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (m >= M) return;
    sizes[m] = (unsigned short)iq::kshap::row_size(keep + (size_t)m * W, W, R);
}

// The rows of block_product for block (bi, bj) of Q: a staged row is its words bi and bj and its scalar e_m; A = bit ? e_m : 0.0,
// B = bit ? 1.0 : 0.0.
template <typename RowScalar>
struct PairRows {
    unsigned long long *sh_a, *sh_b;             // the tile's words bi and bj, bits at or above R masked
    double* sh_e;                                // the tile's e_m
    const unsigned long long* keep;
    size_t stride;
    RowScalar scalar;
    long long rows;
    int bi, bj;
    unsigned long long mask_a, mask_b;
    __device__ __forceinline__ void stage(int t, long long m) const {
        double e = 0.0;
        unsigned long long ka = 0ull, kb = 0ull;
        if (m < rows) {
            e = scalar(m);
            ka = keep[(size_t)m * stride + bi] & mask_a;
            kb = keep[(size_t)m * stride + bj] & mask_b;
        }
        sh_a[t] = ka;
        sh_b[t] = kb;
        sh_e[t] = e;
    }
    __device__ __forceinline__ void operands(int r, int col, double (&fa)[4], double (&fb)[4]) const {
        const unsigned long long wa = sh_a[r] >> col, wb = sh_b[r] >> col;
        const double er = sh_e[r];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            fa[a] = (wa >> (16 * a)) & 1ull ? er : 0.0;          // A[i = 16 a + col][k]
            fb[a] = (wb >> (16 * a)) & 1ull ? 1.0 : 0.0;         // B[k][j = 16 a + col]
        }
    }
};

// The body of both pairwise products: part[((g * nchunk + chunk) * nblk + blk) * 4096 + 64 r + c] = the chunk's sum of
// e_m z_m(64 bi + r) z_m(64 bj + c) over the rows m < rows of the workgroup's chunk, blk = bj (bj + 1) / 2 + bi, bi <= bj, on the
// grid (block, chunk, game).  Row m's words start at keep + m * stride (stride = W: every row; 2 W: the first row of every pair of
// rows), and e_m = scalar(m) is its per-row scalar.  Entries of skipped tiles are written as 0.
template <typename RowScalar>
__device__ __forceinline__ void pair_product_chunk(const unsigned long long* __restrict__ keep, size_t stride, RowScalar scalar,
                                                   long long rows, int R, int tiles_per, double* __restrict__ part) {
    __shared__ unsigned long long sh_a[kTile], sh_b[kTile];
    __shared__ double sh_e[kTile];
    __shared__ double sh_acc[kBlockElems];
    const int t = threadIdx.x, blk = blockIdx.x, chunk = blockIdx.y, g = blockIdx.z;
    const auto [bi, bj] = iq::kshap::block_of(blk);
    const PairRows<RowScalar> staged{sh_a, sh_b, sh_e, keep, stride, scalar, rows, bi, bj, live_mask(bi, R), live_mask(bj, R)};
    iq::kshap::block_product(staged, bi, bj, R, (long long)chunk * tiles_per * kTile, tiles_per, sh_acc);
    double* dst = part + (((size_t)g * gridDim.y + chunk) * gridDim.x + blk) * kBlockElems;
    for (int e = t; e < kBlockElems; e += kThreads) dst[e] = sh_acc[e];
}

// Grid (block of Q, chunk, game): pair_product_chunk over every row with e_m = d_m gamma_s.
// Two workgroups per CU by registers: 160 VGPRs, no scratch (left to itself the compiler takes 288 and one).
template <typename Diff>
__global__ __launch_bounds__(kThreads, 2) void kshap_pairs_q_kernel(const unsigned long long* __restrict__ keep,
                                                                    const unsigned short* __restrict__ sizes, Diff diff,
                                                                    const double* __restrict__ weights,
                                                                    const double* __restrict__ coef, long long M, int R, int W,
                                                                    int tiles_per, double* __restrict__ part) {
    const auto d = diff.of(blockIdx.z, M);
    pair_product_chunk(
        keep, (size_t)W, [=](long long m) { return row_term((weights ? weights[m] : 1.0) * d(m), sizes[m], R, coef, 2); }, M, R,
        tiles_per, part);
}

// Grid (chunk of chunks_of(M), word, game): partL[(g * nchunk + chunk) * R + 64 word + i] = the chunk's sum of (d_m beta_s) z_mi in
// moment_chunk's order; with weights, the workgroups of word 0 and game 0 also leave partW[chunk].
template <typename Diff>
__global__ __launch_bounds__(kThreads) void kshap_pairs_moment_kernel(const unsigned long long* __restrict__ keep,
                                                                      const unsigned short* __restrict__ sizes, Diff diff,
                                                                      const double* __restrict__ weights, const double* __restrict__ coef,
                                                                      long long M, int R, int W, int tiles_per,
                                                                      double* __restrict__ partL, double* __restrict__ partW) {
    const int chunk = blockIdx.x, word = blockIdx.y, g = blockIdx.z;
    const auto d = diff.of(g, M);
    iq::kshap::moment_chunk_of(
        keep, W, word, [=](long long m, double w) { return row_term(w * d(m), sizes[m], R, coef, 1); }, weights, M, tiles_per, chunk,
        partL + ((size_t)g * gridDim.x + chunk) * R + 64 * word, min(64, R - 64 * word),
        weights && word == 0 && g == 0 ? partW + chunk : nullptr);
}

// Grid (chunk of chunks_of(M), game): partA[g * nchunk + chunk] = the chunk's sum of d_m alpha_s by scalar_chunk_of.
template <typename Diff>
__global__ __launch_bounds__(kThreads) void kshap_pairs_alpha_kernel(const unsigned short* __restrict__ sizes, Diff diff,
                                                                     const double* __restrict__ weights,
                                                                     const double* __restrict__ coef, long long M, int R, int tiles_per,
                                                                     double* __restrict__ partA) {
    const int chunk = blockIdx.x, g = blockIdx.y;
    const auto d = diff.of(g, M);
    const double s = iq::kshap::scalar_chunk_of(
        [=](long long m) { return row_term((weights ? weights[m] : 1.0) * d(m), sizes[m], R, coef, 0); }, M, tiles_per, chunk);
    if (threadIdx.x == 0) partA[(size_t)g * gridDim.x + chunk] = s;
}

// Grid (R^2 / 256, game), one thread per (i, j): the thread of i < j folds Q_ij over the chunks in chunk order and writes
// out[i][j] = out[j][i] = delta / (R - 1) + (((A + L_i) + L_j) + Q_ij) / wsum, the same bits on both sides; i = j writes 0.
// delta == nullptr (the terms entries): the quotient alone.
__global__ __launch_bounds__(kThreads) void kshap_pairs_assemble_kernel(const double* __restrict__ part, const double* __restrict__ L,
                                                                        const double* __restrict__ A, const double* __restrict__ wsum,
                                                                        const double* __restrict__ delta, int R, int nchunk, int nblk,
                                                                        double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int g = blockIdx.y;
    if (e >= (long long)R * R) return;
    const int i = (int)(e / R), j = (int)(e % R);
    double* o = out + (size_t)g * R * R;
    if (i == j) o[e] = 0.0;
    if (i >= j) return;
    const int bi = i >> 6, bj = j >> 6, blk = bj * (bj + 1) / 2 + bi;
    const double qij = iq::kshap::fold_chunks(part + ((size_t)g * nchunk * nblk + blk) * kBlockElems + (i & 63) * kBlock + (j & 63),
                                              (size_t)nblk * kBlockElems, nchunk);
    const double y = (((A[g] + L[(size_t)g * R + i]) + L[(size_t)g * R + j]) + qij) / *wsum;
    const double x = delta ? delta[g] / (double)(R - 1) + y : y;
    o[(size_t)i * R + j] = x;
    o[(size_t)j * R + i] = x;
}

// ---- iq_kshap_pairs_se: the standard error of every I_ij from the second moment of the same rows (include/iq.h, "Standard errors") --
// A unit u is the iid draw: row u, or (paired) rows 2u and 2u + 1, a set and its complement.  x_u(k) is the unit's term of I_ij for a
// pair with k members in the unit's first row; its square is P_u + B_u k + G_u [k = 2], so the sum of squares is one scalar, one
// moment and one pairwise product over the units' first rows - the shape of A, L and Q above, in their order, on chunks of units.

// mu(s, k) in closed form from 2 H, each entry two roundings (not from the differences alpha, beta, gamma of `coef`, which cancel
// near s = R - 2); 0 where the case cannot occur and for rows of size 0 or R.
__device__ __forceinline__ double mu_of(int s, int k, int R, double two_h) {
    if (s <= 0 || s >= R) return 0.0;
    if (k == 1) return -two_h;
    if (k == 0) return s <= R - 2 ? two_h * (double)s / (double)(R - s - 1) : 0.0;
    return s >= 2 ? two_h * (double)(R - s) / (double)(s - 1) : 0.0;
}

// Grid (U / 256, game), one thread per unit: P_u, B_u, G_u of game g once into unit[(3 g + {0, 1, 2}) * U + u].
// x_u(k) = d_{cu} mu(s, k) [+ d_{cu+1} mu(R - s, 2 - k)], s the size of the unit's first row; 0 when that size is 0 or R.
template <typename Diff>
__global__ __launch_bounds__(kThreads) void kshap_pairs_unit_kernel(const unsigned short* __restrict__ sizes, Diff diff, long long M,
                                                                    long long U, int R, int paired, double two_h,
                                                                    double* __restrict__ unit) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int g = blockIdx.y;
    if (u >= U) return;
    const auto d = diff.of(g, M);
    const long long m = paired ? 2 * u : u;
    const int s = sizes[m];
    double x[3] = {0.0, 0.0, 0.0};
    if (s > 0 && s < R) {
        const double d0 = d(m);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = d0 * mu_of(s, k, R, two_h);
        if (paired) {
            const double d1 = d(m + 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) x[k] = x[k] + d1 * mu_of(R - s, 2 - k, R, two_h);
        }
    }
    const double p = x[0] * x[0], x1 = x[1] * x[1], x2 = x[2] * x[2];
    double* dst = unit + (size_t)3 * g * U + u;
    dst[0] = p;
    dst[(size_t)U] = x1 - p;
    dst[(size_t)2 * U] = (x2 - 2.0 * x1) + p;
}

// Grid (block, chunk of pair_chunks_of(U, R), game): pair_product_chunk over the units' first rows with e_u = G_u.
__global__ __launch_bounds__(kThreads, 2) void kshap_pairs_se_q_kernel(const unsigned long long* __restrict__ keep,
                                                                       const double* __restrict__ unit, long long U, int R, int stride,
                                                                       int tiles_per, double* __restrict__ part) {
    const double* gu = unit + ((size_t)3 * blockIdx.z + 2) * U;
    pair_product_chunk(keep, (size_t)stride, [=](long long u) { return gu[u]; }, U, R, tiles_per, part);
}

// The sums of B_u z_ui and of P_u over the units are iq_kshap_order.h's unit_moment_kernel<3> and unit_scalar_kernel<3>.

// Grid (R^2 / 256, game), one thread per (i, j); the thread of i < j folds both products over their chunks in chunk order,
//     S1 = ((A + L_i) + L_j) + Q_ij  (the sum the estimate is made of),   S2 = ((A2 + L2_i) + L2_j) + Q2_ij,
//     var = unit_variance(S1, S2, U, M),   se = sqrt(var), 0 where var < 0,
// every operation rounded on its own, and writes se[i][j] = se[j][i], the same bits on both sides; i = j writes 0.
__global__ __launch_bounds__(kThreads) void kshap_pairs_se_assemble_kernel(const double* __restrict__ part, const double* __restrict__ L,
                                                                           const double* __restrict__ A, int nchunk,
                                                                           const double* __restrict__ part2, const double* __restrict__ L2,
                                                                           const double* __restrict__ A2, int nchunk2, long long M,
                                                                           long long U, int R, int nblk, double* __restrict__ se) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int g = blockIdx.y;
    if (e >= (long long)R * R) return;
    const int i = (int)(e / R), j = (int)(e % R);
    double* o = se + (size_t)g * R * R;
    if (i == j) o[e] = 0.0;
    if (i >= j) return;
    const int bi = i >> 6, bj = j >> 6, blk = bj * (bj + 1) / 2 + bi;
    const size_t at = (size_t)blk * kBlockElems + (i & 63) * kBlock + (j & 63), step = (size_t)nblk * kBlockElems;
    const double q1 = iq::kshap::fold_chunks(part + (size_t)g * nchunk * step + at, step, nchunk);
    const double q2 = iq::kshap::fold_chunks(part2 + (size_t)g * nchunk2 * step + at, step, nchunk2);
    const double s1 = ((A[g] + L[(size_t)g * R + i]) + L[(size_t)g * R + j]) + q1;
    const double s2 = ((A2[g] + L2[(size_t)g * R + i]) + L2[(size_t)g * R + j]) + q2;
    const double var = iq::kshap::unit_variance(s1, s2, U, M);
    const double x = var < 0.0 ? 0.0 : sqrt(var);
    o[(size_t)i * R + j] = x;
    o[(size_t)j * R + i] = x;
}

struct Scratch {
    unsigned short* sizes;
    double *partQ, *partL, *partA, *partW, *L, *A, *wsum;
    size_t bytes;
};

Scratch carve(void* base, long long M, int R, int G) {
    const Chunks ch = chunks_of(M), qc = pair_chunks_of(M, R);
    iq::Carver c(base);
    Scratch s;
    s.sizes = c.take<unsigned short>((size_t)M);
    s.partQ = c.take<double>((size_t)G * qc.count * blocks_of(R) * kBlockElems);
    s.partL = c.take<double>((size_t)G * ch.count * R);
    s.partA = c.take<double>((size_t)G * ch.count);
    s.partW = c.take<double>((size_t)ch.count);
    s.L = c.take<double>((size_t)G * R);
    s.A = c.take<double>((size_t)G);
    s.wsum = c.take<double>(1);
    s.bytes = c.bytes();
    return s;
}

// The launches of iq_kshap_pairs on a carved scratch: sizes, Q, L, A, the folds and the assembly of `out`.
template <typename Diff>
int launch_pairs(const Scratch& s, const unsigned long long* k, Diff diff, const double* delta, const double* weights,
                 const double* coef, int M, int R, int G, double* out, hipStream_t st) {
    const Chunks ch = chunks_of(M), qc = pair_chunks_of(M, R);
    const int W = iq::keep_words(R), nblk = blocks_of(R);
    const long long rows = M;
    IQ_LAUNCH(kshap_pairs_sizes_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, k, rows, R, W, s.sizes);
    IQ_LAUNCH((kshap_pairs_q_kernel<Diff>), dim3(nblk, qc.count, G), dim3(kThreads), 0, st, k, (const unsigned short*)s.sizes, diff,
              weights, coef, rows, R, W, qc.tiles_per, s.partQ);
    IQ_LAUNCH((kshap_pairs_moment_kernel<Diff>), dim3(ch.count, W, G), dim3(kThreads), 0, st, k, (const unsigned short*)s.sizes, diff,
              weights, coef, rows, R, W, ch.tiles_per, s.partL, s.partW);
    IQ_LAUNCH((kshap_pairs_alpha_kernel<Diff>), dim3(ch.count, G), dim3(kThreads), 0, st, (const unsigned short*)s.sizes, diff, weights,
              coef, rows, R, ch.tiles_per, s.partA);
    const long long folds = (long long)G * R + G + 1;
    IQ_LAUNCH(iq::kshap::fold_moments_kernel<true>, dim3((unsigned)((folds + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
              (const double*)s.partL, (const double*)s.partA, (const double*)s.partW, weights ? 1 : 0, rows, R, G, ch.count, s.L, s.A,
              s.wsum);
    IQ_LAUNCH(kshap_pairs_assemble_kernel, dim3((unsigned)(((long long)R * R + kThreads - 1) / kThreads), G), dim3(kThreads), 0, st,
              (const double*)s.partQ, (const double*)s.L, (const double*)s.A, (const double*)s.wsum, delta, R, qc.count, nblk, out);
    return IQ_OK;
}

// iq_kshap_pairs_se: the scratch of iq_kshap_pairs first, then the units' (P, B, G), the second product's partials on
// pair_chunks_of(U, R), the second moment's and scalar's partials on chunks_of(U), and their folds (wsum2: the fold kernel's U).
struct SeScratch {
    Scratch first;
    double *unit, *partQ, *partL, *partA, *L, *A, *wsum;
    size_t bytes;
};

SeScratch carve_se(void* base, long long M, int R, int G, long long U) {
    const Chunks ch = chunks_of(U), qc = pair_chunks_of(U, R);
    SeScratch s;
    s.first = carve(base, M, R, G);
    iq::Carver c(base);
    c.off = s.first.bytes;
    s.unit = c.take<double>((size_t)3 * G * U);
    s.partQ = c.take<double>((size_t)G * qc.count * blocks_of(R) * kBlockElems);
    s.partL = c.take<double>((size_t)G * ch.count * R);
    s.partA = c.take<double>((size_t)G * ch.count);
    s.L = c.take<double>((size_t)G * R);
    s.A = c.take<double>((size_t)G);
    s.wsum = c.take<double>(1);
    s.bytes = c.bytes();
    return s;
}

// The launches of iq_kshap_pairs_se on a carved scratch: launch_pairs, then the units, the second product, moment and scalar, their
// folds and the assembly of `se`.
template <typename Diff>
int launch_pairs_se(const SeScratch& s, const unsigned long long* k, Diff diff, const double* delta, const double* coef, int M, int R,
                    int G, int paired, long long U, double* out, double* se, hipStream_t st) {
    IQ_TRY(launch_pairs(s.first, k, diff, delta, nullptr, coef, M, R, G, out, st));
    const Chunks qc1 = pair_chunks_of(M, R), ch = chunks_of(U), qc = pair_chunks_of(U, R);
    const int W = iq::keep_words(R), nblk = blocks_of(R), stride = paired ? 2 * W : W;
    IQ_LAUNCH((kshap_pairs_unit_kernel<Diff>), dim3((unsigned)((U + kThreads - 1) / kThreads), G), dim3(kThreads), 0, st,
              (const unsigned short*)s.first.sizes, diff, (long long)M, U, R, paired ? 1 : 0, iq::kshap::two_harmonic(R), s.unit);
    IQ_LAUNCH(kshap_pairs_se_q_kernel, dim3(nblk, qc.count, G), dim3(kThreads), 0, st, k, (const double*)s.unit, U, R, stride,
              qc.tiles_per, s.partQ);
    IQ_LAUNCH(iq::kshap::unit_moment_kernel<3>, dim3(ch.count, W, G), dim3(kThreads), 0, st, k, (const double*)s.unit + U, U, R, stride,
              ch.tiles_per, s.partL);                 // B_u: the second of a game's three arrays
    IQ_LAUNCH(iq::kshap::unit_scalar_kernel<3>, dim3(ch.count, G), dim3(kThreads), 0, st, (const double*)s.unit, U, ch.tiles_per,
              s.partA);                               // P_u: the first
    const long long folds = (long long)G * R + G + 1;
    IQ_LAUNCH(iq::kshap::fold_moments_kernel<true>, dim3((unsigned)((folds + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
              (const double*)s.partL, (const double*)s.partA, (const double*)nullptr, 0, U, R, G, ch.count, s.L, s.A, s.wsum);
    IQ_LAUNCH(kshap_pairs_se_assemble_kernel, dim3((unsigned)(((long long)R * R + kThreads - 1) / kThreads), G), dim3(kThreads), 0, st,
              (const double*)s.first.partQ, (const double*)s.first.L, (const double*)s.first.A, qc1.count, (const double*)s.partQ,
              (const double*)s.L, (const double*)s.A, qc.count, (long long)M, U, R, nblk, se);
    return IQ_OK;
}

// The checks and the carving of the four entries (`name`: the entry, for the message; `pointers`: whether all of its pointer
// arguments are there) -> a status; with IQ_OK, *carved is set.  The _se entries: *units too, after the shape and before the pointers.
int check_shape(const char* name, int M, int R, int G) {
    IQ_REQUIRE(rows_ok(M, R, G, kMaxR), "%s: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", name, M, R, G, kMaxR);
    return IQ_OK;
}

int check_call(const char* name, bool pointers, int M, int R, int G, void* scratch, size_t scratch_bytes, Scratch* carved) {
    IQ_TRY(check_shape(name, M, R, G));
    IQ_REQUIRE(pointers, "%s: null pointer", name);
    *carved = carve(scratch, M, R, G);
    return iq::kshap::scratch_ok(name, scratch, scratch_bytes, carved->bytes);
}

int check_se_call(const char* name, bool pointers, int M, int R, int G, int paired, void* scratch, size_t scratch_bytes,
                  long long* units, SeScratch* carved) {
    IQ_TRY(check_shape(name, M, R, G));
    *units = iq::kshap::units_of(M, paired);
    IQ_REQUIRE(*units, "%s: M=%d %s rows are not two or more whole units", name, M, paired ? "paired" : "unpaired");
    IQ_REQUIRE(pointers, "%s: null pointer", name);
    *carved = carve_se(scratch, M, R, G, *units);
    return iq::kshap::scratch_ok(name, scratch, scratch_bytes, carved->bytes);
}

}  // namespace

extern "C" size_t iq_kshap_pairs_se_scratch_bytes(int M, int R, int G, int paired) {
    const long long U = iq::kshap::units_of(M, paired);
    return rows_ok(M, R, G, kMaxR) && U ? carve_se(nullptr, M, R, G, U).bytes : 0;
}

extern "C" int iq_kshap_pairs_se(const uint64_t* keep, const float* v, const double* v0, const double* delta, const double* coef, int M,
                                 int R, int G, int paired, double* out, double* se, void* scratch, size_t scratch_bytes,
                                 iq_stream_t stream) {
    long long U;
    SeScratch s;
    IQ_TRY(check_se_call("iq_kshap_pairs_se", keep && v && v0 && delta && coef && out && se && scratch, M, R, G, paired, scratch,
                         scratch_bytes, &U, &s));
    return launch_pairs_se(s, reinterpret_cast<const unsigned long long*>(keep), RewardDiff{v, v0}, delta, coef, M, R, G, paired, U, out,
                           se, iq::as_stream(stream));
}

// The same machinery on float64 per-row terms t in place of (v, v0, delta): out = (((A + L_i) + L_j) + Q_ij) / M, no delta term.
extern "C" int iq_kshap_pairs_terms_se(const uint64_t* keep, const double* t, const double* coef, int M, int R, int G, int paired,
                                       double* out, double* se, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    long long U;
    SeScratch s;
    IQ_TRY(check_se_call("iq_kshap_pairs_terms_se", keep && t && coef && out && se && scratch, M, R, G, paired, scratch, scratch_bytes, &U,
                         &s));
    return launch_pairs_se(s, reinterpret_cast<const unsigned long long*>(keep), TermDiff{t}, nullptr, coef, M, R, G, paired, U, out, se,
                           iq::as_stream(stream));
}

extern "C" size_t iq_kshap_pairs_scratch_bytes(int M, int R, int G) {
    return rows_ok(M, R, G, kMaxR) ? carve(nullptr, M, R, G).bytes : 0;
}

extern "C" int iq_kshap_pairs(const uint64_t* keep, const float* v, const double* v0, const double* delta, const double* weights,
                              const double* coef, int M, int R, int G, double* out, void* scratch, size_t scratch_bytes,
                              iq_stream_t stream) {
    Scratch s;
    IQ_TRY(check_call("iq_kshap_pairs", keep && v && v0 && delta && coef && out && scratch, M, R, G, scratch, scratch_bytes, &s));
    return launch_pairs(s, reinterpret_cast<const unsigned long long*>(keep), RewardDiff{v, v0}, delta, weights, coef, M, R, G, out,
                        iq::as_stream(stream));
}

// iq_kshap_pairs on float64 per-row terms t in place of (v, v0, delta): out = (((A + L_i) + L_j) + Q_ij) / W_sum, no delta term.
// The scratch is iq_kshap_pairs_scratch_bytes.
extern "C" int iq_kshap_pairs_terms(const uint64_t* keep, const double* t, const double* weights, const double* coef, int M, int R,
                                    int G, double* out, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    Scratch s;
    IQ_TRY(check_call("iq_kshap_pairs_terms", keep && t && coef && out && scratch, M, R, G, scratch, scratch_bytes, &s));
    return launch_pairs(s, reinterpret_cast<const unsigned long long*>(keep), TermDiff{t}, nullptr, weights, coef, M, R, G, out,
                        iq::as_stream(stream));
}
