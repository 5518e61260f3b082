// The dense layer's dispatch as a value: which kernel instantiation, which rows and columns, which grid every launch of
// iq::launch_linear / launch_linear_splitk / launch_linear_pool (iq_linear.hip) gets.  Host-only and pure - no HIP header, no
// runtime call, no global: the planners are functions of plain numbers, so a CPU program can enumerate them
// (tests/cpp/linear_plan_check.cpp holds the promises written below); the launchers execute the plan segment by segment.
#pragma once

#include "iq_twin.h"

namespace iq {

// One enumerator per kernel instantiation the launchers launch.
enum LinearKernel {
    kLinBf3Rows128,         // pn_gemm_bf3_kernel<false>
    kLinBf3Rows128Ragged,   // pn_gemm_bf3_kernel<false, 4, true>
    kLinBf3Rows64,          // pn_gemm_bf3_short_kernel<2, false>
    kLinBf3Rows64Ragged,    // pn_gemm_bf3_short_kernel<2, true>
    kLinBf3Rows32,          // pn_gemm_bf3_short_kernel<1, false>
    kLinBf3Rows32Ragged,    // pn_gemm_bf3_short_kernel<1, true>
    kLinLdsCols320,         // pn_gemm_lds_kernel<5, false>
    kLinLdsRows256Cols64,   // pn_gemm_lds_kernel<2, false, 1>
    kLinLdsRows256Cols128,  // pn_gemm_lds_kernel<4, false, 1>
    kLinLdsCols256,         // pn_gemm_lds_kernel<4, false>
    kLinLdsCols128,         // pn_gemm_lds_kernel<2, false>
    kLinDirectCols128,      // pn_linear_kernel<2, 2, 2, 2>
    kLinDirectRows256,      // pn_linear_kernel<2, 1, 4, 1>
    kLinSplitkBf3,          // pn_gemm_bf3_kernel<false, 4, false, true>
    kLinSplitkDirect,       // pn_linear_kernel<2, 2, 2, 2> with kb_per_split > 0
    kLinPoolBf3,            // pn_gemm_bf3_kernel<true>
    kLinPoolLds,            // pn_gemm_lds_kernel<4, true>
    kLinKernels
};

// rows / columns of one workgroup's tile, and whether the products run on the bf16 matrix pipe (three-term) or the fp32 MFMA
constexpr int linear_tile_rows(LinearKernel k) {
    switch (k) {
        case kLinBf3Rows32: case kLinBf3Rows32Ragged: return 32;
        case kLinBf3Rows64: case kLinBf3Rows64Ragged: return 64;
        case kLinLdsRows256Cols64: case kLinLdsRows256Cols128: case kLinDirectRows256: return 256;
        default: return 128;
    }
}
constexpr int linear_tile_cols(LinearKernel k) {
    switch (k) {
        case kLinDirectRows256: return 32;
        case kLinLdsRows256Cols64: return 64;
        case kLinLdsRows256Cols128: case kLinLdsCols128: case kLinDirectCols128: case kLinSplitkDirect: return 128;
        case kLinLdsCols320: return 320;
        default: return 256;
    }
}
constexpr bool linear_is_bf3(LinearKernel k) { return k <= kLinBf3Rows32Ragged || k == kLinSplitkBf3 || k == kLinPoolBf3; }

// Everything a launch needs that is not a pointer.
struct LinearSegment {
    LinearKernel kernel;
    int row0, rows;           // rows [row0, row0 + rows) of A and out (row0: the kernels' m_base)
    int col0, cols;           // columns [col0, col0 + cols) of the layer
    unsigned gx, gy, gz;      // the grid
    int col_blocks;           // > 0: a flat grid, the column blocks of a row tile side by side on one XCD; 0: a (tiles, blocks) grid
    bool tile_nu;             // the caller's tile_nu is passed on (false: dropped, or the kernel takes none)
    int Kp, Kreal;            // bf16x3 kernels: the image's k range (cin rounded up to 32) and the columns A really has
    int chunks_per_split;     // split-K on bf16x3: 32-k chunks per split
    int kbs;                  // split-K on the fp32 MFMA: 8-k blocks per split
};

// Today's longest plan: whole-round grid, tail grid, fp32 rest.
constexpr int kLinearMaxSegments = 3;
struct LinearPlan {
    int n;                    // segments, in launch order
    int splits;               // > 0: the segments write raw partial sums of `splits` k ranges; the reduce kernel follows
    LinearSegment seg[kLinearMaxSegments];
};

// What a plan is a function of.  (No device-side row count: with m_dev the scheme is chosen from M, the host's bound, and every
// grid clamps its rows to *m_dev - workgroups past it leave, the heights stay those measured for M rows.)
struct LinearQuery {
    int M, cin, cout;
    int rows_per_cloud;       // launch_linear only
    int twin;                 // iq::twin()
    int cus;                  // multiprocessors of the device; read only where linear_plan_reads_cus says so
    bool has_bf3;             // the layer carries a bf16x3 image
    bool has_tile_nu;         // launch_linear only
    bool fit_tiles;           // launch_linear only
    bool no_lds_gemm;         // iq::no_lds_gemm()
};

// ---- which columns run as bf16x3 on the bf16 matrix pipe: the three launchers' predicates, side by side ----------------------
// All three: float32-exact, for EVERY M, so that a row's result does not depend on the launch it is in; which columns take which
// arithmetic depends on the layer (and the twin) only.  Twin kTwinDenseFp32 = everything on the fp32 MFMA (A/B and tests).
//
// launch_linear: column blocks of 256, any cin >= 32 (the image pads k to a multiple of 32 with zero columns; a ragged cin has its
// own instantiations).  320 outputs would leave the second block a quarter full, and lose to the NT = 5 fp32 tiling - so for
// 256 n + 64 outputs (n >= 1) the whole blocks go to the bf16 pipe and the last 64 columns to the fp32 MFMA.
constexpr int linear_bf3_cols(int cin, int cout, bool has_bf3, int twin) {
    return !has_bf3 || twin == kTwinDenseFp32 || cin < 32 ? 0
           : cout > 256 && cout % 256 == 64               ? cout - 64
           : cout % 256 == 0                              ? cout
                                                          : 0;
}
// split-K: whole layers of 256 n outputs only - differs from launch_linear in two ways.  cin % 32 == 0, not cin >= 32: a split is
// sixteen whole 32-k chunks and no ragged split-K instantiation exists (the one caller has cin = 16384).  No 256 n + 64 rule: it
// came with PointNet++'s 320-output layer, which is no split-K layer; nothing records a decision beyond that.
constexpr bool linear_splitk_bf3(int cin, int cout, bool has_bf3, int twin) {
    return has_bf3 && cout % 256 == 0 && cin % 32 == 0 && twin != kTwinDenseFp32;
}
// pool: the image is the caller's argument (DGCNN's conv5_bf3), not the layer's; cin % 32 == 0 is the launcher's own
// requirement for either kernel.  The twin is NOT read - differs from the other two: kTwinDenseFp32 leaves conv5 on the bf16
// pipe.  The history shows no reason; the twin came with PointNet's heads and its tests compare launch_linear only.
constexpr bool linear_pool_bf3(int cout, bool has_bf3) { return has_bf3 && cout % 256 == 0; }

namespace plan_detail {

constexpr unsigned ceil_div(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

constexpr LinearSegment segment(LinearKernel k, int row0, int rows, int col0, int cols, int cin) {
    LinearSegment s{};
    s.kernel = k;
    s.row0 = row0, s.rows = rows, s.col0 = col0, s.cols = cols;
    s.gx = ceil_div(rows, linear_tile_rows(k)), s.gy = ceil_div(cols, linear_tile_cols(k)), s.gz = 1;
    s.Kp = (cin + 31) & ~31, s.Kreal = cin;
    return s;
}
// the flat form: ids ((tile / 8) col_blocks + column block) 8 + tile % 8, row tiles rounded up to a multiple of 8
constexpr void flatten(LinearSegment& s) {
    s.col_blocks = (int)s.gy;
    s.gx = (s.gx + 7) / 8 * 8 * s.gy;
    s.gy = 1;
}
constexpr void push(LinearPlan& p, const LinearSegment& s) { p.seg[p.n++] = s; }

// one flat grid of bf16x3 tiles of `tile_rows` rows over rows [row0, row0 + rows) and the first `cols` columns
constexpr void push_bf3_rows(LinearPlan& p, int tile_rows, int row0, int rows, int cols, int cin, bool tile_nu) {
    const bool ragged = (cin & 31) != 0;
    LinearSegment s = segment(tile_rows == 128  ? (ragged ? kLinBf3Rows128Ragged : kLinBf3Rows128)
                              : tile_rows == 64 ? (ragged ? kLinBf3Rows64Ragged : kLinBf3Rows64)
                                                : (ragged ? kLinBf3Rows32Ragged : kLinBf3Rows32),
                              row0, rows, 0, cols, cin);
    flatten(s);
    s.tile_nu = tile_nu;
    push(p, s);
}

// `cols` columns from col0 on the fp32 MFMA.  Two kernel families with bit-identical results (same MFMA order over k): the
// LDS-staged GEMM for launches of at least 2048 rows and 2048 workgroup tiles' worth of work, else operands straight from L1/L2.
constexpr void push_fp32(LinearPlan& p, const LinearQuery& q, int col0, int cols, bool tile_nu) {
    const int M = q.M, ntiles = (cols + 31) / 32;
    const long long t128 = (M + 127) / 128, t256 = (M + 255) / 256;
    LinearKernel k = ntiles >= 4 ? kLinDirectCols128 : kLinDirectRows256;
    if (M >= 2048 && (ntiles >= 4 || (ntiles == 2 && t256 >= 2048)) && q.cin % 32 == 0 && !q.no_lds_gemm) {
        if (ntiles % 10 == 0 && t128 * (ntiles / 10) >= 2048) k = kLinLdsCols320;   // 320 / 640 ... outputs: blocks of exactly 10 tiles
        else if (ntiles == 2 && t256 >= 2048) k = kLinLdsRows256Cols64;              // 64 outputs (the fp32 rest of a 320-output layer)
        else if (ntiles == 4 && t256 >= 2048) k = kLinLdsRows256Cols128;             // 128 outputs: every wave all four column tiles
        else if (ntiles >= 8 && t128 * ((ntiles + 7) / 8) >= 2048) k = kLinLdsCols256;
        else k = kLinLdsCols128;
    }
    LinearSegment s = segment(k, 0, M, col0, cols, q.cin);
    if (k == kLinLdsCols256 && s.gy > 1) flatten(s);
    if (k == kLinDirectCols128 || k == kLinDirectRows256) tile_nu = false;           // these kernels take none
    else if (linear_tile_rows(k) == 256 && q.rows_per_cloud % 256 != 0) tile_nu = false;   // tiles must not straddle clouds
    s.tile_nu = tile_nu;
    push(p, s);
}

}  // namespace plan_detail

// launch_linear's tile_nu survives only where 128-row tiles cannot straddle clouds
constexpr bool linear_keeps_tile_nu(const LinearQuery& q) {
    return q.has_tile_nu && q.rows_per_cloud > 0 && q.rows_per_cloud % 128 == 0;
}

// plan_linear reads q.cus for exactly these launches: the caller has to supply the device's count then (> 0), and need not else
constexpr bool linear_plan_reads_cus(const LinearQuery& q) {
    return q.M > 0 && linear_bf3_cols(q.cin, q.cout, q.has_bf3, q.twin) > 0 && q.fit_tiles && !linear_keeps_tile_nu(q) &&
           q.twin != kTwinDenseTile128;
}

// The plain bf16x3 dense layer.  128-row workgroups sit two to a CU, in rounds of 2 x CUs; 64-row ones three, 32-row ones four to
// a CU.  A grid of fewer than 2 x CUs workgroups leaves every SIMD a single wave, which does not feed the matrix pipe, and a grid a
// few workgroups over a whole number of rounds pays nearly a round for them.  Measured at 33 000 rows on 256 CUs
// (profiles/heads_profile.txt; 128-row tiles -> the choice below):
//   * fewer than one round at 128 rows: 32-row tiles throughout           (512 -> 256: 258 workgroups, 80 -> 60 us; 64-row tiles 64)
//   * fewer than two rounds: 64-row tiles throughout                      (1024 -> 512: 516 workgroups, 221 -> 188 us; 128-row
//     tiles for the whole round and 32-row ones for the 232 rows left: 195; 32-row tiles throughout: 196)
//   * from two rounds on: 128-row tiles, and where the last round is at most a quarter / a half full its rows go to a second grid
//     of 32- / 64-row tiles behind the whole rounds                       (256 -> 4096: 8.06 rounds, 447 -> 445 us, nothing; 64-row
//     tiles throughout 433, 32-row ones 509 - the short tiles' weight stream is 2 x / 4 x per row)
//   * without fit_tiles (the other families' launches, not re-measured), with tile_nu and under twin kTwinDenseTile128: 128-row
//     tiles only, the former launch.
// Which tile a row falls in changes nothing in its result (gemm_bf3_tile: MT), so the result stays independent of M.
// A plan that needs the CU count and is given none (linear_plan_reads_cus, q.cus <= 0) is empty.
constexpr LinearPlan plan_linear(const LinearQuery& q) {
    using namespace plan_detail;
    LinearPlan p{};
    if (q.M <= 0) return p;
    const bool tile_nu = linear_keeps_tile_nu(q);
    const int M = q.M, bf3_cols = linear_bf3_cols(q.cin, q.cout, q.has_bf3, q.twin), gy = bf3_cols / 256;
    if (bf3_cols > 0 && !linear_plan_reads_cus(q)) {
        push_bf3_rows(p, 128, 0, M, bf3_cols, q.cin, tile_nu);
    } else if (bf3_cols > 0) {
        if (q.cus <= 0) return p;
        const long long round = 2LL * q.cus, tiles = (M + 127) / 128, wgs = tiles * gy, last = wgs % round;
        const int m_full = (int)(wgs / round * round / gy) * 128;     // rows of the whole rounds
        if (wgs < round) {
            push_bf3_rows(p, 32, 0, M, bf3_cols, q.cin, false);
        } else if (wgs < 2 * round) {
            push_bf3_rows(p, 64, 0, M, bf3_cols, q.cin, false);
        } else if (last == 0 || last > round / 2 || m_full <= 0 || m_full >= M) {
            push_bf3_rows(p, 128, 0, M, bf3_cols, q.cin, false);
        } else {
            push_bf3_rows(p, 128, 0, m_full, bf3_cols, q.cin, false);
            push_bf3_rows(p, last <= round / 4 ? 32 : 64, m_full, M - m_full, bf3_cols, q.cin, false);
        }
    }
    if (bf3_cols < q.cout) push_fp32(p, q, bf3_cols, q.cout - bf3_cols, tile_nu);
    return p;
}

// Few rows, very long K: K is split over workgroups in slices of 512 k, whatever M is - the summation order must not depend on
// how many rows share the launch, or a coalition's logits would change with the batch it travels in (found by the two-rank
// artefact comparison).  A layer of at most 512 inputs or fewer than 128 outputs is the plain launch_linear layer (no m_dev, no
// tile_nu, no fit_tiles).  Reads M, cin, cout, has_bf3, twin and no_lds_gemm.
constexpr int kLinearSplitKbs = 64;    // 8-k blocks per split
constexpr LinearPlan plan_linear_splitk(const LinearQuery& q) {
    using namespace plan_detail;
    const int ntiles = (q.cout + 31) / 32, splits = (q.cin / 8 + kLinearSplitKbs - 1) / kLinearSplitKbs;
    if (q.M <= 0 || splits <= 1 || ntiles < 4) return plan_linear({q.M, q.cin, q.cout, 0, q.twin, 0, q.has_bf3, false, false, q.no_lds_gemm});
    LinearPlan p{};
    p.splits = splits;
    const bool bf3 = linear_splitk_bf3(q.cin, q.cout, q.has_bf3, q.twin);
    LinearSegment s = segment(bf3 ? kLinSplitkBf3 : kLinSplitkDirect, 0, q.M, 0, q.cout, q.cin);
    if (bf3) {
        flatten(s);
        s.gy = (unsigned)splits;
        s.chunks_per_split = kLinearSplitKbs * 8 / 32;     // the same 512-k splits: 16 chunks of 32 k per workgroup row
    } else {
        s.gz = (unsigned)splits;
        s.kbs = kLinearSplitKbs;
    }
    push(p, s);
    return p;
}

// Dense layer + first pooling stage: 128-row x 256-column tiles in a flat grid on either pipe.  Reads M, cout and has_bf3 (the
// caller's w_bf3 argument); cin % 32 == 0, cout % 32 == 0 and cout >= 256 are the launcher's requirements.
constexpr LinearPlan plan_linear_pool(const LinearQuery& q) {
    using namespace plan_detail;
    LinearPlan p{};
    if (q.M <= 0) return p;
    LinearSegment s = segment(linear_pool_bf3(q.cout, q.has_bf3) ? kLinPoolBf3 : kLinPoolLds, 0, q.M, 0, q.cout, q.cin);
    flatten(s);
    push(p, s);
    return p;
}

}  // namespace iq
