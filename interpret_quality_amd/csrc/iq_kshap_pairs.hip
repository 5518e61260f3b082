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
// 64 q .. 64 q + 63 of every 256-row tile, each wave 4 x 4 tiles of 16 x 16 in 128 accumulator registers.  Operands are made in
// registers from the staged words: A = bit ? e_m : 0.0 with e_m = d_m gamma_s, B = bit ? 1.0 : 0.0 - selects, never a product, so
// a row's e_m reaches only the pairs the row holds.  Ragged R and ragged M are zero operands (bits at or above R are masked when
// the tile is staged, rows at or above M are staged as 0); tiles of a block that lie past R, or below the diagonal of a diagonal
// block, are skipped.  The rows' sizes are counted once, by a kernel of their own, into scratch: 136 blocks at R = 1024 would
// otherwise each re-read every word of every row.
//
// Order: rows in row order within a wave (four rows per MFMA, the instruction's own fixed order within them), the four waves as
// ((0 + 1) + 2) + 3 through LDS, the chunks - pair_chunks_of(M, R), a function of (M, R) alone - in chunk order by the assemble
// kernel.  L, A and W_sum take the order of the regression estimator's moments (iq_kshap_order.h: moment_chunk_of,
// sum_threads_in_order, fold_chunks, fold_wsum) on chunks_of(M).  No floating-point atomics; a game's sums never meet another's.
//
// iq_kshap_pairs_se (below the assemble kernel; include/iq.h, "Standard errors of the sampled estimates") adds the
// standard error of every entry from the second moment of the same rows: the same product body once more, over the iid units.
#include "iq_common.h"
#include "iq_kshap_order.h"

// every sum and the assembly of I_ij are chains of individually rounded operations: no fused multiply-add
#pragma clang fp contract(off)

namespace {

using iq::kshap::Chunks;
using iq::kshap::chunks_of;
using iq::kshap::kThreads;
using iq::kshap::kTile;
using iq::kshap::pair_chunks_of;

constexpr int kMaxR = IQ_MAX_WIDE_REGIONS;
constexpr int kBlock = 64;                       // a block of Q: one word of the rows against one word
constexpr int kBlockElems = kBlock * kBlock;

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the words of a row's bits that exist: all 64, or the low R - 64 word of the last word
__device__ __forceinline__ unsigned long long live_mask(int word, int R) {
    const int bits = R - 64 * word;
    return bits >= 64 ? ~0ull : (1ull << bits) - 1ull;
}

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
    int s = 0;
    for (int w = 0; w < W; ++w) s += __popcll(keep[(size_t)m * W + w] & live_mask(w, R));
    sizes[m] = (unsigned short)s;
}

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
    const int t = threadIdx.x, lane = t & 63, q = t >> 6, col = lane & 15, kk = lane >> 4;
    const int blk = blockIdx.x, chunk = blockIdx.y, g = blockIdx.z;
    int bj = 0;
    while ((bj + 1) * (bj + 2) / 2 <= blk) ++bj;
    const int bi = blk - bj * (bj + 1) / 2;
    const unsigned long long mask_a = live_mask(bi, R), mask_b = live_mask(bj, R);
    const int na = min(4, (R - 64 * bi + 15) >> 4), nb = min(4, (R - 64 * bj + 15) >> 4);
    unsigned tiles_live = 0;                     // bit 4 a + b: tile (a, b) of the block is computed
    for (int a = 0; a < na; ++a)
        for (int b = 0; b < nb; ++b)
            if (bi != bj || b >= a) tiles_live |= 1u << (4 * a + b);
    const long long row0 = (long long)chunk * tiles_per * kTile;

    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int tile = 0; tile < tiles_per; ++tile) {
        const long long m = row0 + (long long)tile * kTile + t;
        const bool live = m < rows;
        double e = 0.0;
        unsigned long long ka = 0ull, kb = 0ull;
        if (live) {
            e = scalar(m);
            ka = keep[(size_t)m * stride + bi] & mask_a;
            kb = keep[(size_t)m * stride + bj] & mask_b;
        }
        sh_a[t] = ka;
        sh_b[t] = kb;
        sh_e[t] = e;
        __syncthreads();
#pragma unroll 2
        for (int step = 0; step < 16; ++step) {
            const int r = q * 64 + step * 4 + kk;                   // this lane's row of the four: k = lane >> 4
            const unsigned long long wa = sh_a[r] >> col, wb = sh_b[r] >> col;
            const double er = sh_e[r];
            double fa[4], fb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                fa[a] = (wa >> (16 * a)) & 1ull ? er : 0.0;          // A[i = 16 a + col][k]
                fb[a] = (wb >> (16 * a)) & 1ull ? 1.0 : 0.0;         // B[k][j = 16 a + col]
            }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if ((tiles_live >> (4 * a + b)) & 1u)
                        acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();
    }
    // the four waves in wave order; C/D of the f64 form: column = lane & 15, row = (lane >> 4) + 4 reg
    for (int turn = 0; turn < 4; ++turn) {
        if (q == turn) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int at = (16 * a + kk + 4 * reg) * kBlock + 16 * b + col;
                        sh_acc[at] = turn == 0 ? acc[a][b][reg] : sh_acc[at] + acc[a][b][reg];
                    }
        }
        __syncthreads();
    }
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

// Grid (chunk of chunks_of(M), game): partA[g * nchunk + chunk] = the chunk's sum of d_m alpha_s: per thread over its rows
// t, t + 256, ... of the chunk, then the 256 threads in index order (the rule of a chunk's sum of weights).
template <typename Diff>
__global__ __launch_bounds__(kThreads) void kshap_pairs_alpha_kernel(const unsigned short* __restrict__ sizes, Diff diff,
                                                                     const double* __restrict__ weights,
                                                                     const double* __restrict__ coef, long long M, int R, int tiles_per,
                                                                     double* __restrict__ partA) {
    __shared__ double sh[kThreads];
    const int chunk = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const auto d = diff.of(g, M);
    const long long row0 = (long long)chunk * tiles_per * kTile;
    double acc = 0.0;
    for (int tile = 0; tile < tiles_per; ++tile) {
        const long long m = row0 + (long long)tile * kTile + t;
        if (m < M) acc += row_term((weights ? weights[m] : 1.0) * d(m), sizes[m], R, coef, 0);
    }
    const double s = iq::kshap::sum_threads_in_order(sh, acc);
    if (t == 0) partA[(size_t)g * gridDim.x + chunk] = s;
}

// One thread per output: the chunks' partials added in chunk order.  Entries [0, G R): L; then G of A; the last one wsum.
__global__ __launch_bounds__(kThreads) void kshap_pairs_fold_kernel(const double* __restrict__ partL, const double* __restrict__ partA,
                                                                    const double* __restrict__ partW, int weighted, long long M, int R,
                                                                    int G, int nchunk, double* __restrict__ L, double* __restrict__ A,
                                                                    double* __restrict__ wsum) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x, nl = (long long)G * R;
    if (e < nl) {
        const long long g = e / R, i = e % R;
        L[e] = iq::kshap::fold_chunks(partL + (size_t)g * nchunk * R + i, R, nchunk);
    } else if (e < nl + G) {
        const long long g = e - nl;
        A[g] = iq::kshap::fold_chunks(partA + (size_t)g * nchunk, 1, nchunk);
    } else if (e == nl + G) {
        *wsum = iq::kshap::fold_wsum(partW, weighted, M, nchunk);
    }
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

// Grid (chunk of chunks_of(U), word, game): partL[(g * nchunk + chunk) * R + 64 word + i] = the chunk's sum of B_u z_ui in
// moment_chunk's order over the units' first rows.
__global__ __launch_bounds__(kThreads) void kshap_pairs_se_moment_kernel(const unsigned long long* __restrict__ keep,
                                                                         const double* __restrict__ unit, long long U, int R, int stride,
                                                                         int tiles_per, double* __restrict__ partL) {
    const int chunk = blockIdx.x, word = blockIdx.y, g = blockIdx.z;
    const double* bu = unit + ((size_t)3 * g + 1) * U;
    iq::kshap::moment_chunk_of(
        keep, stride, word, [=](long long u, double) { return bu[u]; }, nullptr, U, tiles_per, chunk,
        partL + ((size_t)g * gridDim.x + chunk) * R + 64 * word, min(64, R - 64 * word), nullptr);
}

// Grid (chunk of chunks_of(U), game): partA[g * nchunk + chunk] = the chunk's sum of P_u, by the rule of kshap_pairs_alpha_kernel.
__global__ __launch_bounds__(kThreads) void kshap_pairs_se_scalar_kernel(const double* __restrict__ unit, long long U, int tiles_per,
                                                                         double* __restrict__ partA) {
    __shared__ double sh[kThreads];
    const int chunk = blockIdx.x, g = blockIdx.y, t = threadIdx.x;
    const double* pu = unit + (size_t)3 * g * U;
    const long long row0 = (long long)chunk * tiles_per * kTile;
    double acc = 0.0;
    for (int tile = 0; tile < tiles_per; ++tile) {
        const long long u = row0 + (long long)tile * kTile + t;
        if (u < U) acc += pu[u];
    }
    const double s = iq::kshap::sum_threads_in_order(sh, acc);
    if (t == 0) partA[(size_t)g * gridDim.x + chunk] = s;
}

// Grid (R^2 / 256, game), one thread per (i, j); the thread of i < j folds both products over their chunks in chunk order,
//     S1 = ((A + L_i) + L_j) + Q_ij  (the sum the estimate is made of),   S2 = ((A2 + L2_i) + L2_j) + Q2_ij,
//     var = ((U / (U - 1)) (S2 - S1 S1 / U)) / (M M),   se = sqrt(var), 0 where var < 0,
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
    const double units = (double)U, rows = (double)M;
    const double var = ((units / (units - 1.0)) * (s2 - s1 * s1 / units)) / (rows * rows);
    const double x = var < 0.0 ? 0.0 : sqrt(var);
    o[(size_t)i * R + j] = x;
    o[(size_t)j * R + i] = x;
}

struct Scratch {
    unsigned short* sizes;
    double *partQ, *partL, *partA, *partW, *L, *A, *wsum;
    size_t bytes;
};

int blocks_of(int R) {
    const int nb = (R + kBlock - 1) / kBlock;
    return nb * (nb + 1) / 2;
}

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

bool shape_ok(long long M, int R, int G) { return M >= 1 && M <= (1ll << 30) && R >= 2 && R <= kMaxR && G >= 1 && G <= 65535; }

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
    IQ_LAUNCH(kshap_pairs_fold_kernel, dim3((unsigned)((folds + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const double*)s.partL,
              (const double*)s.partA, (const double*)s.partW, weights ? 1 : 0, rows, R, G, ch.count, s.L, s.A, s.wsum);
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

// the units of M rows; 0 where the rows do not make at least two whole units
long long units_of(long long M, int paired) {
    if (paired && (M & 1)) return 0;
    const long long U = paired ? M / 2 : M;
    return U >= 2 ? U : 0;
}

// The launches of iq_kshap_pairs_se on a carved scratch: launch_pairs, then the units, the second product, moment and scalar, their
// folds and the assembly of `se`.
template <typename Diff>
int launch_pairs_se(const SeScratch& s, const unsigned long long* k, Diff diff, const double* delta, const double* coef, int M, int R,
                    int G, int paired, long long U, double* out, double* se, hipStream_t st) {
    IQ_TRY(launch_pairs(s.first, k, diff, delta, nullptr, coef, M, R, G, out, st));
    double h = 0.0;                                   // H_{R-1} as iq_kshap_phi_analytic sums it
    for (int i = 1; i < R; ++i) h += 1.0 / (double)i;
    const Chunks qc1 = pair_chunks_of(M, R), ch = chunks_of(U), qc = pair_chunks_of(U, R);
    const int W = iq::keep_words(R), nblk = blocks_of(R), stride = paired ? 2 * W : W;
    IQ_LAUNCH((kshap_pairs_unit_kernel<Diff>), dim3((unsigned)((U + kThreads - 1) / kThreads), G), dim3(kThreads), 0, st,
              (const unsigned short*)s.first.sizes, diff, (long long)M, U, R, paired ? 1 : 0, 2.0 * h, s.unit);
    IQ_LAUNCH(kshap_pairs_se_q_kernel, dim3(nblk, qc.count, G), dim3(kThreads), 0, st, k, (const double*)s.unit, U, R, stride,
              qc.tiles_per, s.partQ);
    IQ_LAUNCH(kshap_pairs_se_moment_kernel, dim3(ch.count, W, G), dim3(kThreads), 0, st, k, (const double*)s.unit, U, R, stride,
              ch.tiles_per, s.partL);
    IQ_LAUNCH(kshap_pairs_se_scalar_kernel, dim3(ch.count, G), dim3(kThreads), 0, st, (const double*)s.unit, U, ch.tiles_per, s.partA);
    const long long folds = (long long)G * R + G + 1;
    IQ_LAUNCH(kshap_pairs_fold_kernel, dim3((unsigned)((folds + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const double*)s.partL,
              (const double*)s.partA, (const double*)nullptr, 0, U, R, G, ch.count, s.L, s.A, s.wsum);
    IQ_LAUNCH(kshap_pairs_se_assemble_kernel, dim3((unsigned)(((long long)R * R + kThreads - 1) / kThreads), G), dim3(kThreads), 0, st,
              (const double*)s.first.partQ, (const double*)s.first.L, (const double*)s.first.A, qc1.count, (const double*)s.partQ,
              (const double*)s.L, (const double*)s.A, qc.count, (long long)M, U, R, nblk, se);
    return IQ_OK;
}

// The checks and the carving shared by iq_kshap_pairs_se and iq_kshap_pairs_terms_se (`name`: the entry, for the message; `pointers`:
// whether all of its pointer arguments are there) -> a status; with IQ_OK, *units and *carved are set.
int check_se_call(const char* name, bool pointers, int M, int R, int G, int paired, void* scratch, size_t scratch_bytes,
                  long long* units, SeScratch* carved) {
    IQ_REQUIRE(shape_ok(M, R, G), "%s: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", name, M, R, G, kMaxR);
    *units = units_of(M, paired);
    IQ_REQUIRE(*units, "%s: M=%d %s rows are not two or more whole units", name, M, paired ? "paired" : "unpaired");
    IQ_REQUIRE(pointers, "%s: null pointer", name);
    *carved = carve_se(scratch, M, R, G, *units);
    if (scratch_bytes < carved->bytes || ((uintptr_t)scratch & 7))
        return iq::fail(IQ_EWORKSPACE, "%s: scratch of %zu bytes (8-byte aligned) needed, got %zu", name, carved->bytes, scratch_bytes);
    return IQ_OK;
}

}  // namespace

extern "C" size_t iq_kshap_pairs_se_scratch_bytes(int M, int R, int G, int paired) {
    const long long U = units_of(M, paired);
    return shape_ok(M, R, G) && U ? carve_se(nullptr, M, R, G, U).bytes : 0;
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
    return shape_ok(M, R, G) ? carve(nullptr, M, R, G).bytes : 0;
}

extern "C" int iq_kshap_pairs(const uint64_t* keep, const float* v, const double* v0, const double* delta, const double* weights,
                              const double* coef, int M, int R, int G, double* out, void* scratch, size_t scratch_bytes,
                              iq_stream_t stream) {
    IQ_REQUIRE(shape_ok(M, R, G), "iq_kshap_pairs: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G, kMaxR);
    IQ_REQUIRE(keep && v && v0 && delta && coef && out && scratch, "iq_kshap_pairs: null pointer");
    const Scratch s = carve(scratch, M, R, G);
    if (scratch_bytes < s.bytes || ((uintptr_t)scratch & 7))
        return iq::fail(IQ_EWORKSPACE, "iq_kshap_pairs: scratch of %zu bytes (8-byte aligned) needed, got %zu", s.bytes, scratch_bytes);
    return launch_pairs(s, reinterpret_cast<const unsigned long long*>(keep), RewardDiff{v, v0}, delta, weights, coef, M, R, G, out,
                        iq::as_stream(stream));
}

// iq_kshap_pairs on float64 per-row terms t in place of (v, v0, delta): out = (((A + L_i) + L_j) + Q_ij) / W_sum, no delta term.
// The scratch is iq_kshap_pairs_scratch_bytes.
extern "C" int iq_kshap_pairs_terms(const uint64_t* keep, const double* t, const double* weights, const double* coef, int M, int R,
                                    int G, double* out, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(shape_ok(M, R, G), "iq_kshap_pairs_terms: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G, kMaxR);
    IQ_REQUIRE(keep && t && coef && out && scratch, "iq_kshap_pairs_terms: null pointer");
    const Scratch s = carve(scratch, M, R, G);
    if (scratch_bytes < s.bytes || ((uintptr_t)scratch & 7))
        return iq::fail(IQ_EWORKSPACE, "iq_kshap_pairs_terms: scratch of %zu bytes (8-byte aligned) needed, got %zu", s.bytes, scratch_bytes);
    return launch_pairs(s, reinterpret_cast<const unsigned long long*>(keep), TermDiff{t}, nullptr, weights, coef, M, R, G, out,
                        iq::as_stream(stream));
}
