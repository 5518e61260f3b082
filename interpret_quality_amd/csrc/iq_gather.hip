// Standalone gathers of the four model files: index_points and the grouping of PointNet++ / PointConv
// (models/pointnet2.py:27-43, 93-137, 222-230; models/pointconv.py:35-52, 117-197) and DGCNN's edge features
// (models/dgcnn.py:21-47).  They only copy and subtract (one rounding per element, as the reference's `a - b`), so
// floating-point contraction does not matter here.
//
// Both kernels walk their output flat, four consecutive floats per thread and one 16-byte store, whatever the row length
// (torch.empty allocations are 256-byte aligned; the last partial quad is stored element by element).  A thread decodes its
// first element's coordinates with divisions once and then steps them incrementally, so each row's index is loaded once per
// thread and row.  An index outside [0, N) never addresses memory: every element that depends on it is written as NaN.
#include "iq_common.h"

namespace {

constexpr int kThreads = 256;
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// ---- rows [A, P] or [P, A] ------------------------------------------------------------------------------------------
// Output row r of cloud b (rows m = s*K + k of M = S*K per cloud) is built from source point i = idx[b][m] (idx = null:
// i = m): segment A = a[b][i][0..la) minus the centre c[b][s][0..la) (c = null: nothing subtracted), segment P =
// p[b][i][0..lp).  index_points is la = 0; grouping is la = 3.
struct RowGather {
    const float* a;
    const float* c;
    const float* p;
    const int32_t* idx;
    float* out;
    int la, lp, a_first;
    int N, S, K, B;
};

__device__ __forceinline__ float row_value(const RowGather& g, int b, int s, int i, int col) {
    if ((unsigned)i >= (unsigned)g.N) return __int_as_float(0x7fc00000);
    const int ca = g.a_first ? col : col - g.lp;
    if (ca >= 0 && ca < g.la) {
        const float v = g.a[((size_t)b * g.N + i) * g.la + ca];
        return g.c ? v - g.c[((size_t)b * g.S + s) * g.la + ca] : v;
    }
    const int cp = g.a_first ? col - g.la : col;
    return g.p[((size_t)b * g.N + i) * g.lp + cp];
}

__global__ __launch_bounds__(kThreads) void gather_rows_kernel(RowGather g, unsigned total) {
    const unsigned e0 = (blockIdx.x * kThreads + threadIdx.x) * 4u;
    if (e0 >= total) return;
    const unsigned L = g.la + g.lp, M = (unsigned)g.S * g.K;
    unsigned row = e0 / L;
    int col = (int)(e0 - row * L);
    int b = (int)(row / M);
    int m = (int)(row - (unsigned)b * M);
    int s = m / g.K, k = m - s * g.K;
    int i = g.idx ? g.idx[row] : m;
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        while (col >= (int)L) {   // next row (several when L < 4)
            col -= L;
            ++row;
            ++m;
            if (++k == g.K) { k = 0; ++s; }
            if (m == (int)M) { m = 0; s = 0; ++b; }
            if (e0 + q < total) i = g.idx ? g.idx[row] : m;
        }
        v[q] = e0 + q < total ? row_value(g, b, s, i, col) : 0.f;
        ++col;
    }
    if (e0 + 4 <= total) {
        *reinterpret_cast<f32x4_t*>(g.out + e0) = f32x4_t{v[0], v[1], v[2], v[3]};
    } else {
        for (int q = 0; e0 + q < total; ++q) g.out[e0 + q] = v[q];
    }
}

// index_points with C % 4 == 0: whole 16-byte quads of one source row, loaded as one
__global__ __launch_bounds__(kThreads) void gather_rows4_kernel(const float* __restrict__ p, const int32_t* __restrict__ idx,
                                                                float* __restrict__ out, int N, int M, int C, unsigned total4) {
    const unsigned t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= total4) return;
    const unsigned q4 = (unsigned)C / 4;
    const unsigned row = t / q4, cq = t - row * q4;
    const int b = (int)(row / (unsigned)M);
    const int i = idx[row];
    f32x4_t v;
    if ((unsigned)i < (unsigned)N) {
        v = *reinterpret_cast<const f32x4_t*>(p + ((size_t)b * N + i) * C + cq * 4);
    } else {
        const float nan = __int_as_float(0x7fc00000);
        v = f32x4_t{nan, nan, nan, nan};
    }
    *reinterpret_cast<f32x4_t*>(out + (size_t)t * 4) = v;
}

// ---- EdgeConv features: out (B,2C,N,k), [x_j - x_i ; x_i] ---------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void edgeconv_gather_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                                   float* __restrict__ out, int channel_first, int B, int N,
                                                                   int C, int k, unsigned total) {
    const unsigned e0 = (blockIdx.x * kThreads + threadIdx.x) * 4u;
    if (e0 >= total) return;
    const unsigned plane = (unsigned)N * k;
    const unsigned pl = e0 / plane;
    const unsigned r = e0 - pl * plane;
    int b = (int)(pl / (2u * C)), ch = (int)(pl - (unsigned)b * 2u * C);
    int n = (int)(r / (unsigned)k), j = (int)(r - (unsigned)n * k);
    auto at = [&](int bb, int c, int p) {
        return channel_first ? x[((size_t)bb * C + c) * N + p] : x[((size_t)bb * N + p) * C + c];
    };
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (e0 + q < total) {
            if (ch < C) {
                const int i = idx[((size_t)b * N + n) * k + j];
                v[q] = (unsigned)i < (unsigned)N ? at(b, ch, i) - at(b, ch, n) : __int_as_float(0x7fc00000);
            } else {
                v[q] = at(b, ch - C, n);
            }
        } else {
            v[q] = 0.f;
        }
        if (++j == k) {
            j = 0;
            if (++n == N) {
                n = 0;
                if (++ch == 2 * C) { ch = 0; ++b; }
            }
        }
    }
    if (e0 + 4 <= total) {
        *reinterpret_cast<f32x4_t*>(out + e0) = f32x4_t{v[0], v[1], v[2], v[3]};
    } else {
        for (int q = 0; e0 + q < total; ++q) out[e0 + q] = v[q];
    }
}

// The flat kernels address the output with 32-bit element offsets.
constexpr size_t kMaxElems = 0x7ffffff0u;

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int iq_index_points(const float* points, const int32_t* idx, float* out, int B, int N, int M, int C,
                               iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && N >= 1 && M >= 0 && C >= 1, "iq_index_points: B=%d N=%d M=%d C=%d", B, N, M, C);
    const size_t total = (size_t)B * M * C;
    if (total == 0) return IQ_OK;
    IQ_REQUIRE(points && idx && out, "iq_index_points: null pointer");
    IQ_REQUIRE(aligned16(out), "iq_index_points: out must be 16-byte aligned");
    IQ_REQUIRE(total <= kMaxElems, "iq_index_points: output of %zu floats exceeds 2^31", total);
    hipStream_t st = iq::as_stream(stream);
    if (C % 4 == 0 && aligned16(points)) {
        const unsigned t4 = (unsigned)(total / 4);
        IQ_LAUNCH(gather_rows4_kernel, dim3((t4 + kThreads - 1) / kThreads), dim3(kThreads), 0, st, points, idx, out, N, M, C, t4);
        return IQ_OK;
    }
    const RowGather g{nullptr, nullptr, points, idx, out, 0, C, 0, N, 1, M, B};
    const unsigned quads = (unsigned)((total + 3) / 4);
    IQ_LAUNCH(gather_rows_kernel, dim3((quads + kThreads - 1) / kThreads), dim3(kThreads), 0, st, g, (unsigned)total);
    return IQ_OK;
}

extern "C" int iq_group_points(const float* xyz, const float* points, const float* new_xyz, const int32_t* idx, float* out,
                               int xyz_first, int B, int N, int S, int K, int D, iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && N >= 1 && S >= 0 && K >= 0 && D >= 0, "iq_group_points: B=%d N=%d S=%d K=%d D=%d", B, N, S, K, D);
    IQ_REQUIRE(idx || (S == 1 && K == N), "iq_group_points: idx = NULL groups all N points (S = 1, K = N), got S=%d K=%d", S, K);
    IQ_REQUIRE(points || D == 0, "iq_group_points: points = NULL needs D = 0, got D=%d", D);
    if ((size_t)B * S * K == 0) return IQ_OK;
    IQ_REQUIRE(xyz && out, "iq_group_points: null pointer");
    IQ_REQUIRE(aligned16(out), "iq_group_points: out must be 16-byte aligned");
    RowGather g{xyz, new_xyz, points, idx, out, 3, D, xyz_first ? 1 : 0, N, S, K, B};
    const size_t total = (size_t)B * S * K * (3 + D);
    IQ_REQUIRE(total <= kMaxElems, "iq_group_points: output of %zu floats exceeds 2^31", total);
    const unsigned quads = (unsigned)((total + 3) / 4);
    IQ_LAUNCH(gather_rows_kernel, dim3((quads + kThreads - 1) / kThreads), dim3(kThreads), 0, iq::as_stream(stream), g,
              (unsigned)total);
    return IQ_OK;
}

extern "C" int iq_edgeconv_gather(const float* x, const int32_t* idx, float* out, int channel_first, int B, int N, int C, int k,
                                  iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && N >= 1 && C >= 1 && k >= 1, "iq_edgeconv_gather: B=%d N=%d C=%d k=%d", B, N, C, k);
    const size_t total = (size_t)B * 2 * C * N * k;
    if (total == 0) return IQ_OK;
    IQ_REQUIRE(x && idx && out, "iq_edgeconv_gather: null pointer");
    IQ_REQUIRE(aligned16(out), "iq_edgeconv_gather: out must be 16-byte aligned");
    IQ_REQUIRE(total <= kMaxElems, "iq_edgeconv_gather: output of %zu floats exceeds 2^31", total);
    const unsigned quads = (unsigned)((total + 3) / 4);
    IQ_LAUNCH(edgeconv_gather_kernel, dim3((quads + kThreads - 1) / kThreads), dim3(kThreads), 0, iq::as_stream(stream),
              x, idx, out, channel_first ? 1 : 0, B, N, C, k, (unsigned)total);
    return IQ_OK;
}
