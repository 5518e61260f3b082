// The float64 matrix-pipe block product of the regression family, written once for the pairwise product Q (iq_kshap_pairs.hip)
// and the surrogate's Gram matrix (iq_kshap_paircv.hip): a workgroup of kThreads owns one 64 x 64 block on or above the diagonal
// of a symmetric extent x extent product over 0/1 rows, on v_mfma_f64_16x16x4_f64.  Its four waves take rows 64 q .. 64 q + 63 of
// every 256-row tile, each wave 4 x 4 tiles of 16 x 16 in 128 accumulator registers; tiles of a block that lie past the extent, or
// below the diagonal of a diagonal block, are skipped.
//
// Order: rows in row order within a wave (four rows per MFMA, the instruction's own fixed order within them), the four waves as
// ((0 + 1) + 2) + 3 through LDS.  The callers differ only in how a row is staged and how the two operands are selected from it.
#pragma once
#include "iq_kshap_order.h"

namespace iq {
namespace kshap {

constexpr int kBlock = 64;                       // a block: 64 rows of the product against 64 columns
constexpr int kBlockElems = kBlock * kBlock;

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the blocks on or above the diagonal of an extent x extent product, numbered blk = bj (bj + 1) / 2 + bi, bi <= bj
__host__ __device__ inline int blocks_of(int extent) {
    const int nb = (extent + kBlock - 1) / kBlock;
    return nb * (nb + 1) / 2;
}

struct BlockIndex { int bi, bj; };

__device__ __forceinline__ BlockIndex block_of(int blk) {
    int bj = 0;
    while ((bj + 1) * (bj + 2) / 2 <= blk) ++bj;
    return {blk - bj * (bj + 1) / 2, bj};
}

// sh_acc[64 r + c] = the sum over rows row0 .. row0 + 256 tiles - 1 of A[64 bi + r] B[64 bj + c]; entries of skipped tiles are 0.
// `rows` holds pointers to the caller's own __shared__ arrays: rows.stage(t, m) stages row m as row t of the tile (a row the caller
// does not have as one that holds nothing), rows.operands(r, col, fa, fb) gives, for staged row r, fa[a] = A[16 a + col] and
// fb[a] = B[16 a + col] of the block - selects, never products.  Every thread of the workgroup must call it; it ends on a barrier.
template <typename Rows>
__device__ __forceinline__ void block_product(const Rows& rows, int bi, int bj, int extent, long long row0, int tiles,
                                              double* __restrict__ sh_acc) {
    const int t = threadIdx.x, lane = t & 63, q = t >> 6, col = lane & 15, kk = lane >> 4;
    const int na = min(4, (extent - 64 * bi + 15) >> 4), nb = min(4, (extent - 64 * bj + 15) >> 4);
    unsigned tiles_live = 0;                     // bit 4 a + b: tile (a, b) of the block is computed
    for (int a = 0; a < na; ++a)
        for (int b = 0; b < nb; ++b)
            if (bi != bj || b >= a) tiles_live |= 1u << (4 * a + b);

    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int tile = 0; tile < tiles; ++tile) {
        rows.stage(t, row0 + (long long)tile * kTile + t);
        __syncthreads();
#pragma unroll 2
        for (int step = 0; step < 16; ++step) {
            double fa[4], fb[4];
            rows.operands(q * 64 + step * 4 + kk, col, fa, fb);      // this lane's row of the four: k = lane >> 4
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
}

}  // namespace kshap
}  // namespace iq
