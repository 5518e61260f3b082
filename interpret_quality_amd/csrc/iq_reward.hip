// Reward (K3), per-region Shapley accumulation (K4) and interaction reduction (K5); both also for G games on shared rows.
// All tiny next to the forward; written for bit-stability (fixed summation order) first.
#include "iq_common.h"
#include "iq_shapley_sum.h"

namespace {

constexpr int kMaxClasses = 64;

// tools/final_common.py:19-24.  torch.logsumexp(x) = log(sum(exp(x - max))) + max.
__global__ void reward_kernel(const float* __restrict__ logits, int label, int modified,
                              float* __restrict__ v, int B, int C) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float* z = logits + (size_t)b * C;
    float zy = z[label];
    float m = -INFINITY;
    for (int c = 0; c < C; ++c)
        if (!modified || c != label) m = fmaxf(m, z[c]);
    const float ms = (fabsf(m) == INFINITY) ? 0.f : m;
    float s = 0.f;
    for (int c = 0; c < C; ++c)
        if (!modified || c != label) s += expf(z[c] - ms);
    // modified: z_y - logsumexp(others);  normal: log_softmax = (z_y - max) - log(sum)
    v[b] = modified ? zy - (logf(s) + ms) : (zy - ms) - logf(s);
}

// iq_reward for G labels of the same rows.  A workgroup stages kClsRows rows of logits once in LDS (coalesced; the odd row stride
// keeps the lanes on distinct banks), then lane b walks its row for every label in reward_kernel's order, so v[g][b] carries
// reward_kernel's bits for label g.  In normal mode maximum and sum do not depend on the label: once per row.  The labels travel
// by value in the kernel arguments (G <= 64 labels below C <= 64: one byte each).
constexpr int kClsRows = 128;
struct ClassLabels { unsigned char at[kMaxClasses]; };

__global__ __launch_bounds__(kClsRows) void reward_classes_kernel(const float* __restrict__ logits, ClassLabels labels, int G,
                                                                  int modified, float* __restrict__ v, size_t ldv, int B, int C) {
    __shared__ float tile[kClsRows * (kMaxClasses + 1)];
    const long long b0 = (long long)blockIdx.x * kClsRows;
    const int rows = (int)min((long long)kClsRows, B - b0), ld = C | 1;
    const float* src = logits + (size_t)b0 * C;
    for (int i = threadIdx.x; i < rows * C; i += kClsRows) {
        const int row = i / C;
        tile[row * ld + (i - row * C)] = src[i];
    }
    __syncthreads();
    if ((int)threadIdx.x >= rows) return;
    const float* z = tile + threadIdx.x * ld;
    float* out = v + (size_t)b0 + threadIdx.x;
    if (!modified) {
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, z[c]);
        const float ms = (fabsf(m) == INFINITY) ? 0.f : m;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(z[c] - ms);
        const float ls = logf(s);
        for (int g = 0; g < G; ++g) out[(size_t)g * ldv] = (z[labels.at[g]] - ms) - ls;
        return;
    }
    for (int g = 0; g < G; ++g) {
        const int label = labels.at[g];
        const float zy = z[label];
        float m = -INFINITY;
        for (int c = 0; c < C; ++c)
            if (c != label) m = fmaxf(m, z[c]);
        const float ms = (fabsf(m) == INFINITY) ? 0.f : m;
        float s = 0.f;
        for (int c = 0; c < C; ++c)
            if (c != label) s += expf(z[c] - ms);
        out[(size_t)g * ldv] = zy - (logf(s) + ms);
    }
}

// dv = v[i+1] - v[i] in float32, widened to float64 and scattered by the permutation
// (tools/final_common.py:94-96; the float64 target is np.zeros((R,))).
__global__ void shapley_scatter_kernel(const float* __restrict__ v, const int32_t* __restrict__ orders,
                                       double* __restrict__ sv_rows, int R, int S) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S * R) return;
    const int o = t / R, j = t - o * R;
    const float* vo = v + (size_t)o * (R + 1);
    const float dv = vo[j + 1] - vo[j];
    const int r = orders[t];
    if ((unsigned)r < (unsigned)R) sv_rows[(size_t)o * R + r] = (double)dv;  // entries outside [0,R): iq_check_index_range
}

// Sum over permutations in permutation order, one lane per region: the same sequence of float64
// adds the reference's host loop performs, hence bit-identical for identical v (iq_shapley_sum.h).
__global__ __launch_bounds__(iq::kSumThreads) void shapley_sum_kernel(const double* __restrict__ sv_rows, double* __restrict__ phi_sum,
                                                                      const int32_t* __restrict__ snap_counts, int n_snap,
                                                                      double* __restrict__ snaps, int R, int S) {
    iq::shapley_sum_rows(sv_rows, phi_sum, snap_counts, n_snap, snaps, R, S, 0);
}

// ---- iq_shapley_accum_games: G games on the same permutations ---------------------------------------------------------------------
// The scatter of iq_shapley_accum[_wide] writes one (S,R) float64 row table per game.  Where a region stands in a permutation
// does not depend on the game: the permutations are inverted ONCE into 16-bit positions (pos[o][r] = j with orders[o][j] = r),
// and the sum kernel takes game g's difference v[g][o][j + 1] - v[g][o][j] through that table.  A region a row does not name
// keeps kNoPos and contributes 0.0, as the zeroed row table does; an entry outside [0, R) is skipped.  A workgroup inverts as
// many whole permutations as fit kInvEntries entries of LDS, so every store to ``pos`` is coalesced.
constexpr int kInvEntries = IQ_MAX_WIDE_REGIONS, kInvThreads = 256;
constexpr unsigned kNoPos = 0xffffu;

__global__ __launch_bounds__(kInvThreads) void invert_orders_kernel(const int32_t* __restrict__ orders, uint16_t* __restrict__ pos,
                                                                    int R, int S) {
    __shared__ uint16_t tab[kInvEntries];
    const int per = kInvEntries / R;                      // permutations per workgroup
    const int o0 = blockIdx.x * per, n = min(per, S - o0) * R;
    const size_t base = (size_t)o0 * R;
    for (int i = threadIdx.x; i < n; i += kInvThreads) tab[i] = (uint16_t)kNoPos;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kInvThreads) {
        const int o = i / R, j = i - o * R;
        const int r = orders[base + i];
        if ((unsigned)r < (unsigned)R) tab[o * R + r] = (uint16_t)j;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kInvThreads) pos[base + i] = tab[i];
}

// shapley_sum_kernel's body (iq_shapley_sum.h) on a grid of (64 regions, game): the same float64 adds in permutation order.
// kSquare (iq_shapley_sq_accum_games): the widened difference squared - exact in float64 - before it is added.
template <bool kSquare>
__global__ __launch_bounds__(iq::kSumThreads) void shapley_sum_games_kernel(const float* __restrict__ v, size_t ldv,
                                                                            const uint16_t* __restrict__ pos, double* __restrict__ phi_sum,
                                                                            const int32_t* __restrict__ snap_counts, int n_snap,
                                                                            double* __restrict__ snaps, int R, int S) {
    const size_t g = blockIdx.y;
    const float* vg = v + g * ldv;
    iq::shapley_sum_values(
        [&](int o, int r) {
            const unsigned p = pos[(size_t)o * R + r];
            if (p >= (unsigned)R) return 0.0;
            const float* vo = vg + (size_t)o * (R + 1) + p;
            const double d = (double)(vo[1] - vo[0]);
            return kSquare ? __dmul_rn(d, d) : d;
        },
        phi_sum + g * R, snap_counts, n_snap, snaps ? snaps + g * n_snap * R : nullptr, R, S, blockIdx.x * 64);
}

__global__ void interaction_reduce_kernel(const float* __restrict__ v, float* __restrict__ out, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float4 q = reinterpret_cast<const float4*>(v)[k];
    // v[4k] + v[4k+3] - v[4k+1] - v[4k+2], left to right (final_cal_interactions.py:33)
    out[k] = __fsub_rn(__fsub_rn(__fadd_rn(q.x, q.w), q.y), q.z);
}

}  // namespace

extern "C" int iq_reward(const float* logits, int label, int modified, float* v, int B, int C,
                         iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && C >= 2 && C <= kMaxClasses, "iq_reward: B=%d C=%d", B, C);
    IQ_REQUIRE(label >= 0 && label < C, "iq_reward: label %d not in [0,%d)", label, C);
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(logits && v, "iq_reward: null pointer");
    IQ_LAUNCH(reward_kernel, dim3((B + 255) / 256), dim3(256), 0, iq::as_stream(stream), logits, label, modified, v, B, C);
    return IQ_OK;
}

extern "C" int iq_shapley_accum(const float* v, const int32_t* orders, double* sv_rows, double* phi_sum,
                                const int32_t* snap_counts, int n_snap, double* snaps, int R, int S,
                                iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_REGIONS && S >= 0, "iq_shapley_accum: R=%d S=%d", R, S);
    IQ_REQUIRE(phi_sum && sv_rows, "iq_shapley_accum: phi_sum and sv_rows are required");
    IQ_REQUIRE(n_snap == 0 || (snap_counts && snaps), "iq_shapley_accum: snapshots need counts and output");
    IQ_REQUIRE(S == 0 || (v && orders), "iq_shapley_accum: null input");
    hipStream_t st = iq::as_stream(stream);
    if (S > 0) {
        IQ_LAUNCH(shapley_scatter_kernel, dim3((S * R + 255) / 256), dim3(256), 0, st, v, orders, sv_rows, R, S);
    }
    IQ_LAUNCH(shapley_sum_kernel, dim3(1), dim3(iq::kSumThreads), 0, st, sv_rows, phi_sum, snap_counts, n_snap, snaps, R, S);
    return IQ_OK;
}

extern "C" int iq_reward_classes(const float* logits, const int32_t* labels, int G, int modified, float* v, size_t ldv, int B, int C,
                                 iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && C >= 2 && C <= kMaxClasses, "iq_reward_classes: B=%d C=%d", B, C);
    IQ_REQUIRE(G >= 1 && G <= kMaxClasses, "iq_reward_classes: G=%d not in [1,%d]", G, kMaxClasses);
    IQ_REQUIRE(labels || G == C, "iq_reward_classes: labels == NULL means every class, G=%d must be C=%d", G, C);
    IQ_REQUIRE(ldv >= (size_t)B, "iq_reward_classes: ldv=%zu is shorter than B=%d", ldv, B);
    ClassLabels lab = {};
    for (int g = 0; g < G; ++g) {
        const int label = labels ? labels[g] : g;
        IQ_REQUIRE(label >= 0 && label < C, "iq_reward_classes: label %d (position %d) not in [0,%d)", label, g, C);
        lab.at[g] = (unsigned char)label;
    }
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(logits && v, "iq_reward_classes: null pointer");
    IQ_LAUNCH(reward_classes_kernel, dim3((unsigned)(((long long)B + kClsRows - 1) / kClsRows)), dim3(kClsRows), 0,
              iq::as_stream(stream), logits, lab, G, modified, v, ldv, B, C);
    return IQ_OK;
}

extern "C" size_t iq_shapley_games_scratch_bytes(int R, int S, int G) {
    if (R < 1 || R > IQ_MAX_WIDE_REGIONS || S < 0 || G < 1 || G > 65535) return 0;
    return iq::align_up((size_t)S * R * sizeof(uint16_t) + 1, 256);     // the position table; never 0 for accepted arguments
}

// iq_shapley_accum_games and, kSquare, iq_shapley_sq_accum_games: the same checks, position table and grid
template <bool kSquare>
int shapley_accum_games(const char* name, const float* v, size_t ldv, const int32_t* orders, double* phi_sum, const int32_t* snap_counts,
                        int n_snap, double* snaps, int R, int S, int G, void* scratch, size_t scratch_bytes,
                        iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS && S >= 0, "%s: R=%d S=%d", name, R, S);
    IQ_REQUIRE(G >= 1 && G <= 65535, "%s: G=%d not in [1,65535]", name, G);
    IQ_REQUIRE(ldv >= (size_t)S * (R + 1), "%s: ldv=%zu is shorter than S*(R+1)=%zu", name, ldv, (size_t)S * (R + 1));
    IQ_REQUIRE(phi_sum, "%s: phi_sum is required", name);
    IQ_REQUIRE(n_snap >= 0 && (n_snap == 0 || (snap_counts && snaps)), "%s: snapshots need counts and output", name);
    IQ_REQUIRE(S == 0 || (v && orders), "%s: null input", name);
    IQ_REQUIRE(scratch && scratch_bytes >= iq_shapley_games_scratch_bytes(R, S, G),
               "%s: scratch of %zu bytes, iq_shapley_games_scratch_bytes asks for %zu", name, scratch_bytes,
               iq_shapley_games_scratch_bytes(R, S, G));
    hipStream_t st = iq::as_stream(stream);
    uint16_t* pos = static_cast<uint16_t*>(scratch);
    if (S > 0) {
        const int per = kInvEntries / R;
        IQ_LAUNCH(invert_orders_kernel, dim3((S + per - 1) / per), dim3(kInvThreads), 0, st, orders, pos, R, S);
    }
    IQ_LAUNCH(shapley_sum_games_kernel<kSquare>, dim3((R + 63) / 64, G), dim3(iq::kSumThreads), 0, st, v, ldv, pos, phi_sum, snap_counts,
              n_snap, snaps, R, S);
    return IQ_OK;
}

extern "C" int iq_shapley_accum_games(const float* v, size_t ldv, const int32_t* orders, double* phi_sum, const int32_t* snap_counts,
                                      int n_snap, double* snaps, int R, int S, int G, void* scratch, size_t scratch_bytes,
                                      iq_stream_t stream) {
    return shapley_accum_games<false>("iq_shapley_accum_games", v, ldv, orders, phi_sum, snap_counts, n_snap, snaps, R, S, G, scratch,
                                      scratch_bytes, stream);
}

extern "C" int iq_shapley_sq_accum_games(const float* v, size_t ldv, const int32_t* orders, double* sq_sum, const int32_t* snap_counts,
                                         int n_snap, double* sq_snaps, int R, int S, int G, void* scratch, size_t scratch_bytes,
                                         iq_stream_t stream) {
    return shapley_accum_games<true>("iq_shapley_sq_accum_games", v, ldv, orders, sq_sum, snap_counts, n_snap, sq_snaps, R, S, G,
                                     scratch, scratch_bytes, stream);
}

extern "C" int iq_interaction_reduce(const float* v, float* out, int n, iq_stream_t stream) {
    IQ_REQUIRE(n >= 0, "iq_interaction_reduce: n=%d", n);
    if (n == 0) return IQ_OK;
    IQ_REQUIRE(v && out, "iq_interaction_reduce: null pointer");
    IQ_LAUNCH(interaction_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, iq::as_stream(stream), v, out, n);
    return IQ_OK;
}
