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

// One thread per output: the chunks' partials added in chunk order.  Entries [0, G R): b; the last one wsum.
__global__ __launch_bounds__(kThreads) void kshap_fold_wide_kernel(const double* __restrict__ partB, const double* __restrict__ partW,
                                                                   int weighted, long long M, int R, int G, int nchunk,
                                                                   double* __restrict__ b, double* __restrict__ wsum) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x, nb = (long long)G * R;
    if (e < nb) {
        const long long g = e / R, i = e % R;
        b[e] = iq::kshap::fold_chunks(partB + (size_t)g * nchunk * R + i, R, nchunk);
    } else if (e == nb) {
        *wsum = iq::kshap::fold_wsum(partW, weighted, M, nchunk);
    }
}

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

bool shape_ok(long long M, int R, int G) { return M >= 1 && M <= (1ll << 30) && R >= 2 && R <= kMaxR && G >= 1 && G <= 65535; }

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
    return shape_ok(M, R, G) ? carve(nullptr, M, R, G).bytes : 0;
}

extern "C" int iq_kshap_moment_wide(const uint64_t* keep, const float* v, const double* v0, const double* weights, int M, int R, int G,
                                    double* b, double* wsum, void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(shape_ok(M, R, G), "iq_kshap_moment_wide: M=%d, R=%d, G=%d (1 <= M <= 2^30, 2 <= R <= %d, 1 <= G <= 65535)", M, R, G, kMaxR);
    IQ_REQUIRE(keep && v && v0 && b && wsum && scratch, "iq_kshap_moment_wide: null pointer");
    const Scratch s = carve(scratch, M, R, G);
    if (scratch_bytes < s.bytes || ((uintptr_t)scratch & 7))
        return iq::fail(IQ_EWORKSPACE, "iq_kshap_moment_wide: scratch of %zu bytes (8-byte aligned) needed, got %zu", s.bytes, scratch_bytes);
    const Chunks ch = chunks_of(M);
    const int W = iq::keep_words(R);
    hipStream_t st = iq::as_stream(stream);
    IQ_LAUNCH(kshap_moment_wide_kernel, dim3(ch.count, W, G), dim3(kThreads), 0, st,
              reinterpret_cast<const unsigned long long*>(keep), v, v0, weights, (long long)M, R, W, ch.tiles_per, s.partB, s.partW);
    const long long outputs = (long long)G * R + 1;
    IQ_LAUNCH(kshap_fold_wide_kernel, dim3((unsigned)((outputs + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
              (const double*)s.partB, (const double*)s.partW, weights ? 1 : 0, (long long)M, R, G, ch.count, b, wsum);
    return IQ_OK;
}

extern "C" int iq_kshap_phi_analytic(const double* b, const double* wsum, const double* delta, double* phi, int R, int G,
                                     iq_stream_t stream) {
    IQ_REQUIRE(R >= 2 && R <= kMaxR && G >= 1 && G <= 65535, "iq_kshap_phi_analytic: R=%d, G=%d (2 <= R <= %d, 1 <= G <= 65535)", R, G, kMaxR);
    IQ_REQUIRE(b && wsum && delta && phi, "iq_kshap_phi_analytic: null pointer");
    double h = 0.0;                                   // H_{R-1}, float64, ascending k: summed here on the host, passed by value
    for (int k = 1; k < R; ++k) h += 1.0 / (double)k;
    IQ_LAUNCH(kshap_phi_analytic_kernel, dim3(G), dim3(kThreads), 0, iq::as_stream(stream), b, wsum, delta, phi, R, 2.0 * h);
    return IQ_OK;
}
