// The regression (KernelSHAP) estimator of a WIDE region game, 2 <= R <= IQ_MAX_WIDE_REGIONS regions, a row W = ceil(R / 64) words:
// coalition rows from permutations and sizes, the moment b = sum w z (v - v0) of those rows, and phi by the closed form that the
// analytic Gram matrix allows.  include/iq.h has the definitions ("The regression (KernelSHAP) estimator", the wide entry points).
//
// With A = alpha I + c 1 1^T (alpha = 1 / (2 H_{R-1}), c = 1/2 - alpha) the constrained solve collapses to
//     phi_i = 2 H_{R-1} (b_i - mean(b)) + delta / R,
// so there is no matrix, no factorisation and no singular case here; the sampled Gram matrix above 64 regions is not built.
//
// The order of every float64 sum is the narrow estimator's (iq_kshap_order.h, shared with iq_kshap.hip, not copied): rows cut into
// chunks of whole 256-row tiles by chunks_of(M), a workgroup per (chunk, word of the row, game) that sums its chunk's rows for the
// 64 regions of its word, the chunks folded in chunk order by a second kernel.  For R <= 64 that is iq_kshap_accum's b and wsum,
// bit for bit.  No floating-point atomics; a game's sums never meet another game's.
#include "iq_common.h"
#include "iq_kshap_order.h"

// phi is a short chain of individually rounded operations (the header and DESIGN.md 5f name them): no fused multiply-add
#pragma clang fp contract(off)

namespace {

using iq::kshap::Chunks;
using iq::kshap::chunks_of;
using iq::kshap::kThreads;
using iq::kshap::rows_ok;
using iq::kshap::units_of;

constexpr int kMaxW = iq::kMaxKeepWords;
constexpr int kMaxR = IQ_MAX_WIDE_REGIONS;
constexpr int kSamplesPerWg = 4;   // waves of a workgroup, one sample each

// One wave per sample, as context_keep_wide_kernel (iq_wide.hip) has one per context: the lanes stride over the first sizes[m]
// entries of permutation m and OR them into the wave's row in LDS (iq::wave_or_regions), then lanes 0 .. W-1 store the row and,
// paired, lanes W .. 2W-1 its complement within the R bits - one contiguous run of 8 W or 16 W bytes.
// status: 1 = a size outside 1 .. R-1, 2 = an entry outside [0, R); such a row and its complement are written as 0.
__global__ __launch_bounds__(64 * kSamplesPerWg) void kshap_keep_wide_kernel(const int32_t* __restrict__ orders,
                                                                             const int32_t* __restrict__ sizes,
                                                                             unsigned long long* __restrict__ keep, int S, int R, int W,
                                                                             int paired, int32_t* __restrict__ status) {
    __shared__ unsigned long long set_s[kSamplesPerWg][kMaxW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long m = (long long)blockIdx.x * kSamplesPerWg + wave;
    const bool live = m < S;                                    // no early return: every wave reaches both barriers
    if (lane < W) set_s[wave][lane] = 0ull;
    __syncthreads();
    int bad = 0;                                                // the same in every lane of the wave
    if (live) {
        const int s = sizes[m];
        if (s < 1 || s > R - 1) bad = 1;                        // nothing of the permutation is read
        else if (__any(iq::wave_or_regions(orders + (size_t)m * R, s, R, lane, set_s[wave]) ? 1 : 0)) bad = 2;
    }
    __syncthreads();
    if (!live) return;
    if (bad && lane == 0) atomicMax(status, bad);
    const int rows = paired ? 2 : 1;
    if (lane < rows * W) {
        const int q = lane >= W ? 1 : 0, w = lane - q * W;      // row q of the pair, word w of the row
        const unsigned long long set = set_s[wave][w];
        const unsigned long long all = (w == W - 1 && (R & 63)) ? (1ull << (R & 63)) - 1ull : ~0ull;   // bits at or above R stay 0
        keep[(size_t)m * rows * W + lane] = bad ? 0ull : q ? ~set & all : set;
    }
}

// Grid (chunk, word, game).  partB[(g * nchunk + chunk) * R + 64 word + i] = the chunk's sum for region 64 word + i of game g
// (iq::kshap::moment_chunk: the narrow kernel's body on word `word` of the rows); with weights, the workgroups of word 0 and game 0
// also leave partW[chunk], the chunk's sum of weights by the narrow rule.
__global__ __launch_bounds__(kThreads) void kshap_moment_wide_kernel(const unsigned long long* __restrict__ keep, const float* __restrict__ v,
                                                                     const double* __restrict__ v0, const double* __restrict__ weights,
                                                                     long long M, int R, int W, int tiles_per,
                                                                     double* __restrict__ partB, double* __restrict__ partW) {
    const int chunk = blockIdx.x, word = blockIdx.y, g = blockIdx.z;
    iq::kshap::moment_chunk(keep, W, word, v + (size_t)g * M, v0[g], weights, M, tiles_per, chunk,
                            partB + ((size_t)g * gridDim.x + chunk) * R + 64 * word, min(64, R - 64 * word),
                            weights && word == 0 && g == 0 ? partW + chunk : nullptr);
}

// The chunks are folded into b and wsum by iq_kshap_order.h's fold_moments_kernel<false>.

// One workgroup per game.  x_i = b_i / wsum; c = (x_0 + x_1 + ... in index order) / R; y_i = x_i - c; the mean of the centred
// values once more, d = (y_0 + y_1 + ... in index order) / R (zero but for the rounding of c: x is R nearly equal numbers whose
// differences carry phi, and sum(y_i - d) must vanish to the rounding of the small y, not of the large x);
// phi_i = two_h * (y_i - d) + delta / R.  Each operation rounded on its own.
__global__ __launch_bounds__(kThreads) void kshap_phi_analytic_kernel(const double* __restrict__ b, const double* __restrict__ wsum,
                                                                      const double* __restrict__ delta, double* __restrict__ phi, int R,
                                                                      double two_h) {
    __shared__ double y[kMaxR];
    __shared__ double sh_mean;
    const int t = threadIdx.x, g = blockIdx.x;
    const double w = *wsum;
    for (int i = t; i < R; i += kThreads) y[i] = b[(size_t)g * R + i] / w;
    for (int pass = 0; pass < 2; ++pass) {
        __syncthreads();
        if (t == 0) {
            double s = 0.0;
            for (int i = 0; i < R; ++i) s += y[i];
            sh_mean = s / (double)R;
        }
        __syncthreads();
        const double mean = sh_mean;
        if (pass == 0)
            for (int i = t; i < R; i += kThreads) y[i] = y[i] - mean;      // a thread's own entries
        else {
            const double share = delta[g] / (double)R;
            for (int i = t; i < R; i += kThreads) phi[(size_t)g * R + i] = two_h * (y[i] - mean) + share;
        }
    }
}

// ---- iq_kshap_moment_se_wide: the variance of phi under the analytic Gram matrix (include/iq.h, "Standard errors") -----------------
// phi_i = delta / R + (1 / M) sum_u y_ui, y_ui = 2 H D_u (z_ui - s_u / R) over the iid units u (a row, or a row and its complement:
// D_u = d_u or d_2u - d_2u+1; z, s of the unit's first row).  z^2 = z, so sum_u y_ui^2 = 4 H^2 (sum_u e_u z_ui + sum_u f_u) with
// e_u = D_u^2 (1 - 2 s_u / R) and f_u = D_u^2 s_u^2 / R^2: a moment in moment_chunk_of's order with another per-row value, and a scalar.

// One thread per unit: its size once, then e_u and f_u of every game into unit[(2 g + {0, 1}) * U + u].
__global__ __launch_bounds__(kThreads) void kshap_se_unit_wide_kernel(const unsigned long long* __restrict__ keep, const float* __restrict__ v,
                                                                      const double* __restrict__ v0, long long M, long long U, int R, int W,
                                                                      int G, int paired, double* __restrict__ unit) {
    const long long u = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    const long long m = paired ? 2 * u : u;
    const int s = iq::kshap::row_size(keep + (size_t)m * W, W, R);
    const double lin = 1.0 - (double)(2 * s) / (double)R, sq = (double)(s * s) / ((double)R * (double)R);
    for (int g = 0; g < G; ++g) {
        const float* vg = v + (size_t)g * M;
        const double base = v0[g];
        double d = (double)vg[m] - base;
        if (paired) d = d - ((double)vg[m + 1] - base);
        const double d2 = d * d;
        unit[(size_t)(2 * g) * U + u] = d2 * lin;
        unit[(size_t)(2 * g + 1) * U + u] = d2 * sq;
    }
}

// The chunks' sums of e_u z_ui and of f_u over the units are iq_kshap_order.h's unit_moment_kernel<2> and unit_scalar_kernel<2>.

// One workgroup per game.  c = (b_0 + b_1 + ... in index order) / R and F = the chunks' f in chunk order, by thread 0; then per
// region E_i = the chunks' e in chunk order, S1 = two_h (b_i - c), S2 = (two_h two_h) (E_i + F),
// var_i = unit_variance(S1, S2, U, M).  Each operation rounded on its own.
__global__ __launch_bounds__(kThreads) void kshap_moment_var_wide_kernel(const double* __restrict__ b, const double* __restrict__ partE,
                                                                         const double* __restrict__ partF, int nchunk, long long M,
                                                                         long long U, int R, double two_h, double* __restrict__ var) {
    __shared__ double sh_mean, sh_f;
    const int t = threadIdx.x, g = blockIdx.x;
    if (t == 0) {
        double s = 0.0;
        for (int i = 0; i < R; ++i) s += b[(size_t)g * R + i];
        sh_mean = s / (double)R;
        sh_f = iq::kshap::fold_chunks(partF + (size_t)g * nchunk, 1, nchunk);
    }
    __syncthreads();
    const double scale = two_h * two_h;
    for (int i = t; i < R; i += kThreads) {
        const double e = iq::kshap::fold_chunks(partE + (size_t)g * nchunk * R + i, R, nchunk);
        const double s1 = two_h * (b[(size_t)g * R + i] - sh_mean), s2 = scale * (e + sh_f);
        var[(size_t)g * R + i] = iq::kshap::unit_variance(s1, s2, U, M);
    }
}

struct Scratch {
    double *partB, *partW;
    size_t bytes;
};

Scratch carve(void* base, long long M, int R, int G) {
    const Chunks ch = chunks_of(M);
    iq::Carver c(base);
    Scratch s;
    s.partB = c.take<double>((size_t)G * ch.count * R);
    s.partW = c.take<double>((size_t)ch.count);
    s.bytes = c.bytes();
    return s;
}

}  // namespace

extern "C" int iq_kshap_keep_masks_wide(const int32_t* orders, const int32_t* sizes, uint64_t* keep, int S, int R, int paired,
                                        int32_t* status, iq_stream_t stream) {
    IQ_REQUIRE(R >= 2 && R <= kMaxR, "iq_kshap_keep_masks_wide: R=%d is outside 2..%d", R, kMaxR);
    IQ_REQUIRE(S >= 0 && S <= (1 << 29), "iq_kshap_keep_masks_wide: S=%d", S);
    if (S == 0) return IQ_OK;
    IQ_REQUIRE(orders && sizes && keep && status, "iq_kshap_keep_masks_wide: null pointer");
    IQ_LAUNCH(kshap_keep_wide_kernel, dim3((unsigned)((S + kSamplesPerWg - 1) / kSamplesPerWg)), dim3(64 * kSamplesPerWg), 0,
              iq::as_stream(stream), orders, sizes, reinterpret_cast<unsigned long long*>(keep), S, R, iq::keep_words(R),
              paired ? 1 : 0, status);
    return IQ_OK;
}

extern "C" size_t iq_kshap_scratch_bytes_wide(int M, int R, int G) {
    return rows_ok(M, R, G, kMaxR) ? carve(nullptr, M, R, G).bytes : 0;
}

extern "C" int iq_kshap_moment_wide(const uint64_t* keep, const float* v, const double* v0, const double* weights, int M, int R, int G,
                                    double* b, double* wsum, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(rows_ok(M, R, G, kMaxR), "iq_kshap_moment_wide: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G, kMaxR);
    IQ_REQUIRE(keep && v && v0 && b && wsum && scratch, "iq_kshap_moment_wide: null pointer");
    const Scratch s = carve(scratch, M, R, G);
    IQ_TRY(iq::kshap::scratch_ok("iq_kshap_moment_wide", scratch, scratch_bytes, s.bytes));
    const Chunks ch = chunks_of(M);
    const int W = iq::keep_words(R);
    hipStream_t st = iq::as_stream(stream);
    IQ_LAUNCH(kshap_moment_wide_kernel, dim3(ch.count, W, G), dim3(kThreads), 0, st,
              reinterpret_cast<const unsigned long long*>(keep), v, v0, weights, (long long)M, R, W, ch.tiles_per, s.partB, s.partW);
    const long long outputs = (long long)G * R + 1;
    IQ_LAUNCH(iq::kshap::fold_moments_kernel<false>, dim3((unsigned)((outputs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
              (const double*)s.partB, (const double*)nullptr, (const double*)s.partW, weights ? 1 : 0, (long long)M, R, G, ch.count, b,
              (double*)nullptr, wsum);
    return IQ_OK;
}

extern "C" int iq_kshap_phi_analytic(const double* b, const double* wsum, const double* delta, double* phi, int R, int G,
                                     iq_stream_t stream) {
    IQ_REQUIRE(R >= 2 && R <= kMaxR && G >= 1 && G <= 65535, "iq_kshap_phi_analytic: R=%d, G=%d (2 <= R <= %d, 1 <= G <= 65535)", R, G, kMaxR);
    IQ_REQUIRE(b && wsum && delta && phi, "iq_kshap_phi_analytic: null pointer");
    IQ_LAUNCH(kshap_phi_analytic_kernel, dim3(G), dim3(kThreads), 0, iq::as_stream(stream), b, wsum, delta, phi, R,
              iq::kshap::two_harmonic(R));
    return IQ_OK;
}

namespace {

// iq_kshap_moment_se_wide: the scratch of iq_kshap_moment_wide first, then its wsum, the units' (e, f) and their chunks' partials.
struct SeScratch {
    Scratch first;
    double *wsum, *unit, *partE, *partF;
    size_t bytes;
};

SeScratch carve_se(void* base, long long M, int R, int G, long long U) {
    const Chunks ch = chunks_of(U);
    SeScratch s;
    s.first = carve(base, M, R, G);
    iq::Carver c(base);
    c.off = s.first.bytes;
    s.wsum = c.take<double>(1);
    s.unit = c.take<double>((size_t)2 * G * U);
    s.partE = c.take<double>((size_t)G * ch.count * R);
    s.partF = c.take<double>((size_t)G * ch.count);
    s.bytes = c.bytes();
    return s;
}

}  // namespace

extern "C" size_t iq_kshap_moment_se_scratch_bytes_wide(int M, int R, int G, int paired) {
    const long long U = units_of(M, paired);
    return rows_ok(M, R, G, kMaxR) && U ? carve_se(nullptr, M, R, G, U).bytes : 0;
}

extern "C" int iq_kshap_moment_se_wide(const uint64_t* keep, const float* v, const double* v0, int M, int R, int G, int paired, double* b,
                                       double* var, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(rows_ok(M, R, G, kMaxR), "iq_kshap_moment_se_wide: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G,
               kMaxR);
    const long long U = units_of(M, paired);
    IQ_REQUIRE(U, "iq_kshap_moment_se_wide: M=%d %s rows are not two or more whole units", M, paired ? "paired" : "unpaired");
    IQ_REQUIRE(keep && v && v0 && b && var && scratch, "iq_kshap_moment_se_wide: null pointer");
    const SeScratch s = carve_se(scratch, M, R, G, U);
    IQ_TRY(iq::kshap::scratch_ok("iq_kshap_moment_se_wide", scratch, scratch_bytes, s.bytes));
    IQ_TRY(iq_kshap_moment_wide(keep, v, v0, nullptr, M, R, G, b, s.wsum, scratch, s.first.bytes, stream));
    const Chunks ch = chunks_of(U);
    const int W = iq::keep_words(R), stride = paired ? 2 * W : W;
    hipStream_t st = iq::as_stream(stream);
    const unsigned long long* k = reinterpret_cast<const unsigned long long*>(keep);
    IQ_LAUNCH(kshap_se_unit_wide_kernel, dim3((unsigned)((U + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, k, v, v0, (long long)M, U,
              R, W, G, paired ? 1 : 0, s.unit);
    IQ_LAUNCH(iq::kshap::unit_moment_kernel<2>, dim3(ch.count, W, G), dim3(kThreads), 0, st, k, (const double*)s.unit, U, R, stride,
              ch.tiles_per, s.partE);                 // e_u: the first of a game's two arrays
    IQ_LAUNCH(iq::kshap::unit_scalar_kernel<2>, dim3(ch.count, G), dim3(kThreads), 0, st, (const double*)s.unit + U, U, ch.tiles_per,
              s.partF);                               // f_u: the second
    IQ_LAUNCH(kshap_moment_var_wide_kernel, dim3(G), dim3(kThreads), 0, st, (const double*)b, (const double*)s.partE,
              (const double*)s.partF, ch.count, (long long)M, U, R, iq::kshap::two_harmonic(R), var);
    return IQ_OK;
}
