// Geometry kernels: nearest-centre region assignment (K6), farthest point sampling (K7) and the standalone
// distance-valued ops of the model files: PointConv's knn_point and compute_density, and the nearest-first ordering
// of a neighbour list.
//
// Both are index-valued, so the floating-point expressions are written with explicitly rounded
// operations (__fmul_rn/__fadd_rn: no FMA contraction) in the order the reference's PyTorch
// expressions evaluate them; ties resolve to the lowest index like the CPU argmin/argmax.
#include "iq_common.h"
#include "iq_mfma.h"
#include "iq_sqdist.h"

// Index-valued results depend on individually rounded operations: forbid the compiler from fusing
// a*b+c into an fma anywhere in this file (explicit fmaf / MFMA calls are unaffected).
#pragma clang fp contract(off)

namespace {

using iq::norm3;      // iq_sqdist.h: the reference's square_distance for one pair, shared with iq_wide.hip
using iq::sqdist3;

// ---- K6: tools/final_util.py:134-147 + final_shapley_value.py:29-31 -------------------------
__global__ __launch_bounds__(256) void region_assign_kernel(const float* __restrict__ cloud,
                                                            const int32_t* __restrict__ fps_idx,
                                                            int32_t* __restrict__ region_id, int N, int R) {
    __shared__ float cs[IQ_MAX_REGIONS * 4];
    if (threadIdx.x < R) {
        const int c = min(max(fps_idx[threadIdx.x], 0), N - 1);  // out-of-range indices: iq_check_index_range
        const float x = cloud[c * 3], y = cloud[c * 3 + 1], z = cloud[c * 3 + 2];
        cs[threadIdx.x * 4 + 0] = x;
        cs[threadIdx.x * 4 + 1] = y;
        cs[threadIdx.x * 4 + 2] = z;
        cs[threadIdx.x * 4 + 3] = norm3(x, y, z);
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

// ---- K7: final_save_fps.py:10-31 --------------------------------------------------------------
// One workgroup per cloud; coordinates and running min-distance live in LDS; per iteration one
// wave-shuffle arg-max + one cross-wave step (2 barriers).
constexpr int kFpsThreads = 256;

__device__ inline void argmax_combine(float& v, int& i, float ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

// n_unique (optional): number of sampled points before the running max distance reaches 0, i.e.
// before every remaining point coincides with an already sampled one; from then on arg-max returns
// index 0 forever (CPU tie rule), so the loop stops and the tail is filled with 0.
__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ xyz,
                                                          int32_t* __restrict__ idx,
                                                          int32_t* __restrict__ n_unique, int N, int S) {
    extern __shared__ float lds[];
    float* px = lds;           // N
    float* py = px + N;        // N
    float* pz = py + N;        // N
    float* mind = pz + N;      // N
    __shared__ float wv[kFpsThreads / 64];
    __shared__ int wi[kFpsThreads / 64];
    __shared__ int far_s;

    const float* src = xyz + (size_t)blockIdx.x * N * 3;
    for (int p = threadIdx.x; p < N; p += kFpsThreads) {
        px[p] = src[p * 3];
        py[p] = src[p * 3 + 1];
        pz[p] = src[p * 3 + 2];
        mind[p] = 1e10f;
    }
    if (threadIdx.x == 0) far_s = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int it = 0; it < S; ++it) {
        const int far = far_s;
        if (threadIdx.x == 0) idx[(size_t)blockIdx.x * S + it] = far;
        const float cx = px[far], cy = py[far], cz = pz[far];
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int p = threadIdx.x; p < N; p += kFpsThreads) {
            const float dx = __fsub_rn(px[p], cx), dy = __fsub_rn(py[p], cy), dz = __fsub_rn(pz[p], cz);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            float m = mind[p];
            if (d < m) { m = d; mind[p] = d; }
            if (m > bv) { bv = m; bi = p; }  // increasing p: strict > keeps the lowest index
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            argmax_combine(bv, bi, ov, oi);
        }
        __syncthreads();  // everyone has read far_s
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float v = wv[0];
            int i = wi[0];
            for (int w = 1; w < kFpsThreads / 64; ++w) argmax_combine(v, i, wv[w], wi[w]);
            far_s = (v == 0.f) ? -1 - it : i;  // negative = exhausted after `it + 1` samples
        }
        __syncthreads();
        if (far_s < 0) {
            const int done = it + 1;
            for (int j = done + threadIdx.x; j < S; j += kFpsThreads) idx[(size_t)blockIdx.x * S + j] = 0;
            if (threadIdx.x == 0 && n_unique) n_unique[blockIdx.x] = done;
            return;
        }
    }
    if (threadIdx.x == 0 && n_unique) n_unique[blockIdx.x] = S;
}

// One WAVE per cloud, the points in registers (lane l owns points l, l + 64, ...): no LDS, no barrier.  FPS is a chain of S
// dependent arg-max rounds, so a launch is latency-bound per cloud and throughput comes from how many clouds are in flight;
// the workgroup form above keeps 2-3 clouds per CU busy with two barriers per round, this one a wave per cloud on every SIMD.
// Same arithmetic per point and the same tie rule (largest distance, then lowest index), so the picks are identical.
// The arg-max runs on a 64-bit key (float bits of the running min-distance, which is >= +0, above the complemented index);
// the winner's coordinates are read from the lane that owns it (its local best IS the winner).
template <int PPL>
__global__ __launch_bounds__(64) void fps_wave_kernel(const float* __restrict__ xyz, int32_t* __restrict__ idx,
                                                      int32_t* __restrict__ n_unique, int N, int S) {
    const int lane = threadIdx.x;
    const float* src = xyz + (size_t)blockIdx.x * N * 3;
    float px[PPL], py[PPL], pz[PPL], md[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int p = lane + 64 * j;
        const bool live = p < N;
        px[j] = live ? src[p * 3] : 0.f;
        py[j] = live ? src[p * 3 + 1] : 0.f;
        pz[j] = live ? src[p * 3 + 2] : 0.f;
        md[j] = live ? 1e10f : -1.f;           // a point that does not exist never wins (keys are built from md >= 0 only)
    }
    int far = 0;
    float cx, cy, cz;
    cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(px[0]), 0));
    cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(py[0]), 0));
    cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pz[0]), 0));
    int32_t* out = idx + (size_t)blockIdx.x * S;
    for (int it = 0; it < S; ++it) {
        if (lane == 0) out[it] = far;
        unsigned long long best = 0ull;         // (float bits of min-distance) << 32 | ~index ; 0 = nothing
        float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const float dx = __fsub_rn(px[j], cx), dy = __fsub_rn(py[j], cy), dz = __fsub_rn(pz[j], cz);
            const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            float m = md[j];
            if (d < m && m >= 0.f) { m = d; md[j] = d; }
            if (m >= 0.f) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(m) << 32) | (unsigned)(~(lane + 64 * j));
                if (key > best) { best = key; bx = px[j]; by = py[j]; bz = pz[j]; }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)(best & 0xffffffffu), off);
            const unsigned hi = __shfl_xor((unsigned)(best >> 32), off);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other > best ? other : best;
        }
        const float v = __uint_as_float((unsigned)(best >> 32));
        const int win = (int)~(unsigned)(best & 0xffffffffu);
        if (v == 0.f) {                         // every remaining point coincides with a sampled one: arg-max returns 0 from now on
            for (int j2 = it + 1 + lane; j2 < S; j2 += 64) out[j2] = 0;
            if (lane == 0 && n_unique) n_unique[blockIdx.x] = it + 1;
            return;
        }
        far = win;
        const int owner = __builtin_amdgcn_readfirstlane(win) & 63;
        cx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bx), owner));
        cy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(by), owner));
        cz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(bz), owner));
    }
    if (lane == 0 && n_unique) n_unique[blockIdx.x] = S;
}

// ---- ordered distance keys -----------------------------------------------------------------------------------------
// A float32 distance as an order-preserving unsigned word (negative values - the expanded form can give slightly negative
// distances - below positive ones) above a 32-bit tie-breaker: comparing keys as integers orders by distance, then tie-breaker.
__device__ __forceinline__ unsigned long long dist_key(float d, unsigned tie) {
    const unsigned u = __float_as_uint(d);
    return ((unsigned long long)(u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u)) << 32) | tie;
}

// ---- models/pointconv.py:103-114 (knn_point), nearest first -------------------------------------------------------
// One wave per query: the keys of all N points (distance, index) go to LDS, padded to a power of two P with keys above every
// real one, and a bitonic sort puts them in ascending order - nearest first, ties to the lower index; the first K are the answer.
__global__ __launch_bounds__(64) void knn_point_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                       int32_t* __restrict__ idx, int N, int S, int K, int P) {
    extern __shared__ unsigned long long keys[];   // P
    const int q = blockIdx.x;                      // b * S + s
    const int b = q / S, lane = threadIdx.x;
    const float qx = new_xyz[(size_t)q * 3], qy = new_xyz[(size_t)q * 3 + 1], qz = new_xyz[(size_t)q * 3 + 2];
    const float qn = norm3(qx, qy, qz);
    const float* kb = xyz + (size_t)b * N * 3;
    for (int j = lane; j < P; j += 64) {
        unsigned long long key = ~0ull;
        if (j < N) {
            const float x = kb[j * 3], y = kb[j * 3 + 1], z = kb[j * 3 + 2];
            key = dist_key(sqdist3(qx, qy, qz, qn, x, y, z, norm3(x, y, z)), (unsigned)j);   // square_distance(new_xyz, xyz)
        }
        keys[j] = key;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < P / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const unsigned long long a = keys[lo], c = keys[hi];
                if ((a > c) == ((lo & size) == 0)) { keys[lo] = c; keys[hi] = a; }
            }
            __syncthreads();
        }
    }
    for (int r = lane; r < K; r += 64) idx[(size_t)q * K + r] = (int32_t)(unsigned)keys[r];
}

// ---- the ordering of models/dgcnn.py:12-18 (topk(sorted=True)) for a given neighbour set ------------------------------------
// One wave per row (4 rows per workgroup).  Every entry's distance to the query in the reference's association: row i of
// -xx - inner - xx^T is -((|x_j|^2 + inner_ij) + |x_i|^2) with inner = -2 x_i.x_j, so the distance is (|k|^2 + (-2 q.k)) + |q|^2
// (dot product as an fma chain, norms as channel-sequential sums of rounded squares).  An entry's rank is the number of entries
// with a smaller (distance, index, position) key.  A row holding an index outside [0, N) is left as it is.
constexpr int kSortMaxK = 128;

__global__ __launch_bounds__(256) void sort_neighbours_kernel(const float* __restrict__ qs, const float* __restrict__ keys,
                                                              int32_t* __restrict__ idx, int rows, int N, int S, int C, int k) {
    __shared__ unsigned long long list[4][kSortMaxK];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;   // b * S + s
    const bool live = row < rows;
    bool bad = false;
    if (live) {
        const int b = row / S;
        const float* qp = qs + (size_t)row * C;
        float qn = __fmul_rn(qp[0], qp[0]);
        for (int c = 1; c < C; ++c) qn = __fadd_rn(qn, __fmul_rn(qp[c], qp[c]));
        for (int e = lane; e < k; e += 64) {
            const int i = idx[(size_t)row * k + e];
            if ((unsigned)i >= (unsigned)N) { bad = true; continue; }
            const float* kp = keys + ((size_t)b * N + i) * C;
            float dot = __fmul_rn(qp[0], kp[0]), kn = __fmul_rn(kp[0], kp[0]);
            for (int c = 1; c < C; ++c) {
                dot = __fmaf_rn(qp[c], kp[c], dot);
                kn = __fadd_rn(kn, __fmul_rn(kp[c], kp[c]));
            }
            const float d = __fadd_rn(__fadd_rn(kn, __fmul_rn(-2.f, dot)), qn);
            list[wave][e] = dist_key(d, ((unsigned)i << 7) | (unsigned)e);
        }
    }
    const bool skip = __any(bad);
    __syncthreads();
    if (!live || skip) return;
    for (int e = lane; e < k; e += 64) {
        const unsigned long long key = list[wave][e];
        int rank = 0;
        for (int f = 0; f < k; ++f) rank += list[wave][f] < key ? 1 : 0;
        idx[(size_t)row * k + rank] = (int32_t)((unsigned)key >> 7);
    }
}

// ---- models/pointconv.py:199-209 (compute_density) -------------------------------------------------------------------------
// density[i] = mean_j exp(-d_ij / c0) / c1 with d = square_distance(xyz, xyz), c0 = 2 h^2 and c1 = 2.5 h rounded to float32 as
// torch rounds the Python scalars; exp and both divisions per pair as in the reference, the mean accumulated in float64.
// One thread per point, the cloud staged through LDS in tiles.
constexpr int kDensityTile = 1024;

__global__ __launch_bounds__(256) void density_kernel(const float* __restrict__ xyz, float c0, float c1, float* __restrict__ out,
                                                      int N) {
    __shared__ float4 pts[kDensityTile];
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float* src = xyz + (size_t)b * N * 3;
    const int iq = min(i, N - 1);
    const float qx = src[iq * 3], qy = src[iq * 3 + 1], qz = src[iq * 3 + 2];
    const float qn = norm3(qx, qy, qz);
    double sum = 0.0;
    for (int j0 = 0; j0 < N; j0 += kDensityTile) {
        const int nt = min(kDensityTile, N - j0);
        __syncthreads();
        for (int p = threadIdx.x; p < nt; p += 256) {
            const float x = src[(j0 + p) * 3], y = src[(j0 + p) * 3 + 1], z = src[(j0 + p) * 3 + 2];
            pts[p] = make_float4(x, y, z, norm3(x, y, z));
        }
        __syncthreads();
        for (int p = 0; p < nt; ++p) {
            const float4 k = pts[p];
            const float d = sqdist3(qx, qy, qz, qn, k.x, k.y, k.z, k.w);
            sum += (double)__fdiv_rn(expf(__fdiv_rn(-d, c0)), c1);
        }
    }
    if (i < N) out[(size_t)b * N + i] = (float)(sum / (double)N);
}

}  // namespace

extern "C" int iq_region_assign(const float* cloud, const int32_t* fps_idx, int32_t* region_id,
                                int N, int R, iq_stream_t stream) {
    IQ_REQUIRE(cloud && fps_idx && region_id, "iq_region_assign: null pointer");
    IQ_REQUIRE(N > 0 && R >= 1 && R <= IQ_MAX_REGIONS, "iq_region_assign: N=%d R=%d", N, R);
    IQ_LAUNCH(region_assign_kernel, dim3((N + 255) / 256), dim3(256), 0, iq::as_stream(stream), cloud, fps_idx, region_id, N, R);
    return IQ_OK;
}

int iq::launch_fps(const float* xyz, int32_t* idx, int32_t* n_unique, int B, int N, int S, hipStream_t st) {
    IQ_REQUIRE(B >= 0 && N > 0 && N <= 8192 && S >= 1, "iq_fps: B=%d N=%d S=%d", B, N, S);
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(xyz && idx, "iq_fps: null pointer");
    // many clouds of at most 1024 points: one wave per cloud (points in registers); few or larger clouds: one workgroup per cloud
    if (B >= 64 && N <= 1024) {
        if (N <= 128) IQ_LAUNCH(fps_wave_kernel<2>, dim3(B), dim3(64), 0, st, xyz, idx, n_unique, N, S);
        else if (N <= 512) IQ_LAUNCH(fps_wave_kernel<8>, dim3(B), dim3(64), 0, st, xyz, idx, n_unique, N, S);
        else IQ_LAUNCH(fps_wave_kernel<16>, dim3(B), dim3(64), 0, st, xyz, idx, n_unique, N, S);
        return IQ_OK;
    }
    const size_t lds = (size_t)N * 4 * sizeof(float);
    if (lds > 48 * 1024) {  // above the default dynamic-LDS limit (N > 3072): opt in, up to 128 KB at N = 8192
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(fps_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
            return iq::fail(IQ_ELAUNCH, "iq_fps: cannot reserve %zu bytes of LDS for N=%d", lds, N);
    }
    IQ_LAUNCH(fps_kernel, dim3(B), dim3(kFpsThreads), lds, st, xyz, idx, n_unique, N, S);
    return IQ_OK;
}

extern "C" int iq_fps(const float* xyz, int32_t* idx, int B, int N, int S, iq_stream_t stream) {
    return iq::launch_fps(xyz, idx, nullptr, B, N, S, iq::as_stream(stream));
}

extern "C" int iq_knn_point(const float* xyz, const float* new_xyz, int K, int32_t* idx, void* tmp, size_t tmp_bytes, int B, int N,
                            int S, iq_stream_t stream) {
    (void)tmp;
    (void)tmp_bytes;
    IQ_REQUIRE(B >= 0 && S >= 0 && N >= 1 && N <= IQ_MAX_POINTS, "iq_knn_point: N=%d outside 1..%d", N, IQ_MAX_POINTS);
    IQ_REQUIRE(K >= 1 && K <= N && K <= 128, "iq_knn_point: K=%d outside 1..min(N=%d, 128)", K, N);
    if ((size_t)B * S == 0) return IQ_OK;
    IQ_REQUIRE(xyz && new_xyz && idx, "iq_knn_point: null pointer");
    IQ_REQUIRE((size_t)B * S <= 0x7fffffffu, "iq_knn_point: B*S=%zu queries", (size_t)B * S);
    int P = 2;
    while (P < N) P <<= 1;
    IQ_LAUNCH(knn_point_kernel, dim3((unsigned)(B * S)), dim3(64), (size_t)P * 8, iq::as_stream(stream), xyz, new_xyz, idx,
              N, S, K, P);
    return IQ_OK;
}

extern "C" int iq_sort_neighbours(const float* q, const float* keys, int32_t* idx, int B, int N, int S, int C, int k,
                                  iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && S >= 0 && N >= 1 && N <= (1 << 24) && C >= 1, "iq_sort_neighbours: B=%d N=%d S=%d C=%d", B, N, S, C);
    IQ_REQUIRE(k >= 1 && k <= kSortMaxK, "iq_sort_neighbours: k=%d outside 1..%d", k, kSortMaxK);
    const size_t rows = (size_t)B * S;
    if (rows == 0) return IQ_OK;
    IQ_REQUIRE(q && keys && idx, "iq_sort_neighbours: null pointer");
    IQ_REQUIRE(rows <= 0x7ffffff0u, "iq_sort_neighbours: B*S=%zu rows", rows);
    IQ_LAUNCH(sort_neighbours_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, iq::as_stream(stream), q, keys, idx,
              (int)rows, N, S, C, k);
    return IQ_OK;
}

extern "C" int iq_density(const float* xyz, double bandwidth, float* out, int B, int N, iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && B <= 65535 && N >= 1, "iq_density: B=%d N=%d", B, N);
    IQ_REQUIRE(bandwidth > 0.0, "iq_density: bandwidth %g must be positive", bandwidth);
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(xyz && out, "iq_density: null pointer");
    const float c0 = (float)(2.0 * bandwidth * bandwidth), c1 = (float)(2.5 * bandwidth);
    IQ_LAUNCH(density_kernel, dim3((N + 255) / 256, B), dim3(256), 0, iq::as_stream(stream), xyz, c0, c1, out, N);
    return IQ_OK;
}
