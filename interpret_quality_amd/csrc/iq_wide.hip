// Wide games: coalitions over more than 64 regions, up to one region per point (include/iq.h, "Wide coalitions").
//
// A wide coalition is a row of W = ceil(R / 64) uint64 words; bit (r & 63) of word (r >> 6) set = region r kept, bits at or above
// R are ignored.  The four small kernels of the Shapley path in their wide form: prefix masks, masking, region assignment and the
// per-region accumulation.  Each repeats the arithmetic of its narrow twin (iq_sample.hip, iq_mask.hip, iq_geom.hip,
// iq_reward.hip) operation by operation - the twins' tables and grids are sized for 64 regions, nothing else differs - so for
// R <= 64 the results are the twins' bits.  The (pair, context) masks of the interaction stage have the twin's rows and another
// kernel shape: one wave per context.  The fused PointNet path for wide masks is in iq_pointnet.hip.
#include "iq_common.h"
#include "iq_shapley_sum.h"
#include "iq_sqdist.h"

// iq_region_assign_wide is index-valued: individually rounded operations, as in iq_geom.hip
#pragma clang fp contract(off)

namespace {

constexpr int kMaxW = iq::kMaxKeepWords;

__host__ __device__ inline int words_of(int R) { return iq::keep_words(R); }

using iq::keep_bit_wide;   // iq_common.h: shared with the compact coalition paths' wide forms

// ---- prefix masks: one lane per (permutation, word), running OR over the entries that fall into its word ----------------------
__global__ __launch_bounds__(256) void prefix_keep_wide_kernel(const int32_t* __restrict__ orders, uint64_t* __restrict__ keep,
                                                               int S, int R, int W) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)S * W) return;
    const int s = (int)(t / W), w = (int)(t - (size_t)s * W);
    const int32_t* ord = orders + (size_t)s * R;
    uint64_t* out = keep + (size_t)s * (R + 1) * W + w;     // the W lanes of a permutation store one 8 W-byte row together
    uint64_t m = 0;
    out[0] = 0;
    for (int j = 0; j < R; ++j) {
        const int r = ord[j];
        if ((unsigned)r < (unsigned)R && (r >> 6) == w) m |= 1ull << (r & 63);   // an out-of-range entry is ignored
        out[(size_t)(j + 1) * W] = m;
    }
}

// ---- (pair, context) masks: one wave per context ------------------------------------------------------------------------------
// The narrow kernel gives a lane a whole context; at m up to R - 2 = 1022 that is a thousand dependent loads per lane, each lane on
// a row of its own.  Here the 64 lanes of a wave stride over the m entries of ONE context (`contexts` is row-contiguous: coalesced),
// OR their bits into the wave's W words in LDS (OR is order-independent: the words do not depend on the schedule), and lanes
// 0 .. 4W-1 then store the four rows S+{i,j}, S+{i}, S+{j}, S as one contiguous run of 32 W <= 512 bytes.
constexpr int kCtxPerWg = 4;   // waves of a workgroup, one context each

__global__ __launch_bounds__(64 * kCtxPerWg) void context_keep_wide_kernel(const int32_t* __restrict__ pairs,
                                                                           const int32_t* __restrict__ ctx,
                                                                           uint64_t* __restrict__ keep, size_t PC, int C, int m, int R,
                                                                           int W) {
    __shared__ unsigned long long set_s[kCtxPerWg][kMaxW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t t = (size_t)blockIdx.x * kCtxPerWg + wave;     // (pair, context) index p*C + c
    const bool live = t < PC;                                   // no early return: every wave reaches both barriers
    if (lane < W) set_s[wave][lane] = 0ull;
    __syncthreads();
    if (live) iq::wave_or_regions(ctx + t * m, m, R, lane, set_s[wave]);   // an out-of-range entry is ignored
    __syncthreads();
    if (live && lane < 4 * W) {
        const int q = lane / W, w = lane - q * W;               // row q of the four, word w of the row
        const size_t p = t / C;
        const int i = pairs[2 * p], j = pairs[2 * p + 1];
        uint64_t v = set_s[wave][w];
        if (q <= 1 && (unsigned)i < (unsigned)R && (i >> 6) == w) v |= 1ull << (i & 63);          // rows 0, 1 hold region i
        if ((q & 1) == 0 && (unsigned)j < (unsigned)R && (j >> 6) == w) v |= 1ull << (j & 63);    // rows 0, 2 hold region j
        keep[t * 4 * W + lane] = v;
    }
}

// ---- masking: mask_rows_kernel (iq_mask.hip) with the keep rows of its four output clouds in LDS ----------------------------------
constexpr int kRowsPerWg = 4;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void mask_rows_wide_kernel(const float* __restrict__ cloud, const int32_t* __restrict__ region_id,
                                                                  const uint64_t* __restrict__ keep, const float* __restrict__ center,
                                                                  float* __restrict__ out, int N, int R, int W, int rows,
                                                                  int channel_first) {
    __shared__ uint64_t keep_s[kRowsPerWg][kMaxW];
    const int g0 = blockIdx.x * kRowsPerWg;
    for (int i = threadIdx.x; i < kRowsPerWg * W; i += kThreads) {
        const int r = i / W, w = i - r * W;
        keep_s[r][w] = g0 + r < rows ? keep[(size_t)(g0 + r) * W + w] : 0ull;
    }
    __syncthreads();
    const size_t cloud_floats = (size_t)N * 3;
    if (N & 3) {   // output clouds are not 16-byte aligned: element by element
        for (int e = threadIdx.x; e < N * 3; e += kThreads) {
            int p, ch;
            if (channel_first) { ch = e / N; p = e - ch * N; }
            else               { p = e / 3;  ch = e - p * 3; }
            const float x = cloud[p * 3 + ch], c = center[ch];
            const int rid = region_id[p];
            for (int r = 0; r < kRowsPerWg && g0 + r < rows; ++r)
                out[(size_t)(g0 + r) * cloud_floats + e] = keep_bit_wide(keep_s[r], rid, R) ? x : c;
        }
        return;
    }
    const int nvec = N * 3 / 4;
    for (int e4 = threadIdx.x; e4 < nvec; e4 += kThreads) {
        float x[4], c[4];
        int rid[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = e4 * 4 + q;
            int p, ch;
            if (channel_first) { ch = e / N; p = e - ch * N; }
            else               { p = e / 3;  ch = e - p * 3; }
            x[q] = cloud[p * 3 + ch];
            c[q] = center[ch];
            rid[q] = region_id[p];
        }
#pragma unroll
        for (int r = 0; r < kRowsPerWg; ++r) {
            const int g = g0 + r;
            if (g >= rows) break;
            float4 o;
            o.x = keep_bit_wide(keep_s[r], rid[0], R) ? x[0] : c[0];
            o.y = keep_bit_wide(keep_s[r], rid[1], R) ? x[1] : c[1];
            o.z = keep_bit_wide(keep_s[r], rid[2], R) ? x[2] : c[2];
            o.w = keep_bit_wide(keep_s[r], rid[3], R) ? x[3] : c[3];
            reinterpret_cast<float4*>(out + (size_t)g * cloud_floats)[e4] = o;
        }
    }
}

// ---- region assignment: region_assign_kernel (iq_geom.hip) with a centre table for IQ_MAX_WIDE_REGIONS -------------------------
using iq::norm3;      // iq_sqdist.h: the one expression iq_region_assign ranks by
using iq::sqdist3;

__global__ __launch_bounds__(256) void region_assign_wide_kernel(const float* __restrict__ cloud, const int32_t* __restrict__ fps_idx,
                                                                 int32_t* __restrict__ region_id, int N, int R) {
    __shared__ float cs[IQ_MAX_WIDE_REGIONS * 4];
    for (int r = threadIdx.x; r < R; r += blockDim.x) {
        const int c = min(max(fps_idx[r], 0), N - 1);  // out-of-range indices: iq_check_index_range
        const float x = cloud[c * 3], y = cloud[c * 3 + 1], z = cloud[c * 3 + 2];
        cs[r * 4 + 0] = x;
        cs[r * 4 + 1] = y;
        cs[r * 4 + 2] = z;
        cs[r * 4 + 3] = norm3(x, y, z);
    }
    __syncthreads();
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N) return;
    const float x = cloud[p * 3], y = cloud[p * 3 + 1], z = cloud[p * 3 + 2];
    const float sx = norm3(x, y, z);
    float best = INFINITY;
    int arg = 0;
    for (int r = 0; r < R; ++r) {
        const float d = sqdist3(x, y, z, sx, cs[r * 4], cs[r * 4 + 1], cs[r * 4 + 2], cs[r * 4 + 3]);
        if (d < best) { best = d; arg = r; }
    }
    region_id[p] = arg;
}

// ---- accumulation: the two kernels of iq_shapley_accum, the sum over a grid of 64-region workgroups -----------------------------
__global__ void shapley_scatter_wide_kernel(const float* __restrict__ v, const int32_t* __restrict__ orders,
                                            double* __restrict__ sv_rows, int R, int S) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)S * R) return;
    const size_t o = t / R;
    const int j = (int)(t - o * R);
    const float* vo = v + o * (R + 1);
    const float dv = vo[j + 1] - vo[j];
    const int r = orders[t];
    if ((unsigned)r < (unsigned)R) sv_rows[o * R + r] = (double)dv;
}

// shapley_sum_kernel's body (iq_shapley_sum.h) on one workgroup per 64 regions
__global__ __launch_bounds__(iq::kSumThreads) void shapley_sum_wide_kernel(const double* __restrict__ sv_rows, double* __restrict__ phi_sum,
                                                                           const int32_t* __restrict__ snap_counts, int n_snap,
                                                                           double* __restrict__ snaps, int R, int S) {
    iq::shapley_sum_rows(sv_rows, phi_sum, snap_counts, n_snap, snaps, R, S, blockIdx.x * 64);
}

}  // namespace

extern "C" int iq_prefix_keep_masks_wide(const int32_t* orders, uint64_t* keep, int S, int R, iq_stream_t stream) {
    IQ_REQUIRE(S >= 0 && R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_prefix_keep_masks_wide: S=%d R=%d", S, R);
    if (S == 0) return IQ_OK;
    IQ_REQUIRE(orders && keep, "iq_prefix_keep_masks_wide: null pointer");
    const int W = words_of(R);
    const size_t n = (size_t)S * W;
    IQ_REQUIRE((n + 255) / 256 <= 0x7fffffffu, "iq_prefix_keep_masks_wide: S=%d is too large", S);
    IQ_LAUNCH(prefix_keep_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, iq::as_stream(stream), orders, keep,
              S, R, W);
    return IQ_OK;
}

extern "C" int iq_context_keep_masks_wide(const int32_t* pairs, const int32_t* contexts, uint64_t* keep, int P, int C, int m, int R,
                                          iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_context_keep_masks_wide: R=%d not in [1,%d]", R, IQ_MAX_WIDE_REGIONS);
    IQ_REQUIRE(P >= 0 && C >= 0 && m >= 0 && m <= R, "iq_context_keep_masks_wide: P=%d C=%d m=%d R=%d", P, C, m, R);
    const size_t n = (size_t)P * C;
    if (n == 0) return IQ_OK;
    IQ_REQUIRE(pairs && keep && (contexts || m == 0), "iq_context_keep_masks_wide: null pointer");
    const size_t grid = (n + kCtxPerWg - 1) / kCtxPerWg;
    IQ_REQUIRE(grid <= 0x7fffffffu, "iq_context_keep_masks_wide: P=%d C=%d is too large", P, C);
    IQ_LAUNCH(context_keep_wide_kernel, dim3((unsigned)grid), dim3(64 * kCtxPerWg), 0, iq::as_stream(stream), pairs, contexts,
              keep, n, C, m, R, words_of(R));
    return IQ_OK;
}

extern "C" int iq_mask_coalitions_wide(const float* cloud, const int32_t* region_id, const uint64_t* keep, const float* center,
                                       float* out, int N, int R, int B, int channel_first, iq_stream_t stream) {
    IQ_REQUIRE(B >= 0, "iq_mask_coalitions_wide: B=%d", B);
    IQ_REQUIRE(N > 0 && N <= IQ_MAX_POINTS, "iq_mask_coalitions_wide: N=%d not in (0,%d]", N, IQ_MAX_POINTS);
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_mask_coalitions_wide: R=%d not in [1,%d]", R, IQ_MAX_WIDE_REGIONS);
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(cloud && region_id && keep && center && out, "iq_mask_coalitions_wide: null pointer");
    const int grid = (B + kRowsPerWg - 1) / kRowsPerWg;
    IQ_LAUNCH(mask_rows_wide_kernel, dim3(grid), dim3(kThreads), 0, iq::as_stream(stream), cloud, region_id, keep, center,
              out, N, R, words_of(R), B, channel_first);
    return IQ_OK;
}

extern "C" int iq_region_assign_wide(const float* cloud, const int32_t* fps_idx, int32_t* region_id, int N, int R,
                                     iq_stream_t stream) {
    IQ_REQUIRE(cloud && fps_idx && region_id, "iq_region_assign_wide: null pointer");
    IQ_REQUIRE(N > 0 && R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_region_assign_wide: N=%d R=%d", N, R);
    IQ_LAUNCH(region_assign_wide_kernel, dim3((N + 255) / 256), dim3(256), 0, iq::as_stream(stream), cloud, fps_idx,
              region_id, N, R);
    return IQ_OK;
}

extern "C" int iq_shapley_accum_wide(const float* v, const int32_t* orders, double* sv_rows, double* phi_sum,
                                     const int32_t* snap_counts, int n_snap, double* snaps, int R, int S, iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS && S >= 0, "iq_shapley_accum_wide: R=%d S=%d", R, S);
    IQ_REQUIRE(phi_sum && sv_rows, "iq_shapley_accum_wide: phi_sum and sv_rows are required");
    IQ_REQUIRE(n_snap == 0 || (snap_counts && snaps), "iq_shapley_accum_wide: snapshots need counts and output");
    IQ_REQUIRE(S == 0 || (v && orders), "iq_shapley_accum_wide: null input");
    hipStream_t st = iq::as_stream(stream);
    if (S > 0) {
        const size_t n = (size_t)S * R;
        IQ_REQUIRE((n + 255) / 256 <= 0x7fffffffu, "iq_shapley_accum_wide: S=%d is too large", S);
        IQ_LAUNCH(shapley_scatter_wide_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, v, orders, sv_rows, R, S);
    }
    IQ_LAUNCH(shapley_sum_wide_kernel, dim3((R + 63) / 64), dim3(iq::kSumThreads), 0, st, sv_rows, phi_sum, snap_counts, n_snap, snaps,
              R, S);
    return IQ_OK;
}
