// DGCNN / GCNN forward (models/dgcnn.py:12-194) on materialised (masked) clouds.
//
// EdgeConv restructuring (exact algebra): with W = [W_a | W_b] and BN(eval) y = s.z + t,
//     max_j LeakyReLU(s.(W_a (x_j - x_i) + W_b x_i) + t) = LeakyReLU( max_j P_j + Q_i ),
//     P = (s.W_a) x,  Q = (s.(W_b - W_a)) x + t,
// because the x_i terms are constant over the neighbourhood and LeakyReLU is increasing.  One GEMM
// over the N points per layer (2*Cout outputs) and a gather-max replace the 20x larger edge tensor.
//
// kNN (index-valued): -|x_i|^2 - (-2 x_i.x_j) - |x_j|^2 evaluated in the reference's order, inner
// products on the fp32 MFMA.  Keys run along the accumulator registers and queries along the lanes,
// so every lane keeps the running top-20 of its query in registers; ties between exact duplicates
// (masked points) are harmless because duplicates carry identical features.
//
// Ragged batches.  A masked cloud holds its kept points plus M copies of the centre, and every copy sees the same
// neighbourhoods and produces the same features in every layer.  iq_dgcnn_coalitions therefore never materialises the
// N rows: cloud b becomes D_b = kept + 1 rows - the centre once, carrying the multiplicity min(M, 20) with which it can
// appear in a top-20 (applied when knn_kernel writes the neighbour lists) - padded to a multiple of 32 with dead rows
// whose |x|^2 is +inf so that no query selects them.  Max-pooling and the neighbourhood max are set operations, so they
// are unchanged; the mean pool weights the centre by M.  Exact, and the kNN work drops
// with the square of the kept fraction.  All kernels below run on the ragged layout (row offsets per cloud); the dense
// forward is the special case D_b = N.
//
// Files.  iq_dgcnn_knn.h: the ragged layout (Ragged), the neighbour-list format (nb_encode) and the feature-space graphs
// (rownorm_kernel, knn_kernel, knn_refine_kernel, launch_knn).  iq_edgeconv.h: the EdgeConv layer on its three routes
// (fused_path, launch_edgeconv).  Here: the layout kernels, the layer-1 walk, the pooling's second stage and the host driver.
#include "iq_dgcnn_knn.h"
#include "iq_edgeconv.h"
#include "iq_profile.h"
#include "iq_srclist.h"
#include "iq_twin.h"

namespace {

// ---- pad xyz (B,N,3) -> (B,N,8) -------------------------------------------------------------------
// (B,N,3) -> (B,Np,8), Np = N rounded up to 32; rows N..Np-1 of a cloud are dead (zero; rownorm gives them +inf)
__global__ void pad_xyz_kernel(const float* __restrict__ xyz, float* __restrict__ out, int B, int N, int Np) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * Np) return;
    const int b = t / Np, i = t - b * Np;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 a = z;
    if (i < N) {
        const float* src = xyz + ((size_t)b * N + i) * 3;
        a = (f32x4){src[0], src[1], src[2], 0.f};
    }
    reinterpret_cast<f32x4*>(out)[(size_t)t * 2] = a;
    reinterpret_cast<f32x4*>(out)[(size_t)t * 2 + 1] = z;
}

// dense forward: D_b = N
__global__ void dg_dense_layout_kernel(int32_t* __restrict__ roff, int32_t* __restrict__ nkept, int32_t* __restrict__ ncopy,
                                       int32_t* __restrict__ row_cloud, float* __restrict__ row_w, int B, int N, int Np) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < B * Np) { row_cloud[t] = t / Np; if (row_w) row_w[t] = (t % Np) < N ? 1.f : 0.f; }
    if (t <= B) roff[t] = t * Np;
    if (t < B) { nkept[t] = N; ncopy[t] = 0; }
}

// coalitions: kept points of coalition b = points whose region bit is set in keep[b]
// WIDE (the three kernels that read a mask: count, compact, walk): keep is (B, W) rows of an R-region game, iq::WaveKeep<true>
// (iq_common.h) - a compile-time switch, the narrow instantiations are the kernels as they were; R and W are theirs to ignore.
template <bool WIDE>
__global__ __launch_bounds__(64) void dg_count_kernel(const int32_t* __restrict__ region_id, const uint64_t* __restrict__ keep,
                                                      const int32_t* __restrict__ cloud_of, int32_t* __restrict__ nkept,
                                                      int32_t* __restrict__ ncopy, int32_t* __restrict__ dpad, int N, int nclouds,
                                                      int R, int W) {
    __shared__ uint64_t strip[WIDE ? iq::kMaxKeepWords : 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int c = cloud_of ? cloud_of[b] : (nclouds == 1 ? 0 : b);
    const iq::WaveKeep<WIDE> k(keep, b, R, W, lane, strip);
    const int32_t* rid = region_id + (size_t)c * N;
    int n = 0;
    for (int i = lane; i < N; i += 64) n += (int)k(rid[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) {
        const int copies = min(N - n, kK);        // multiplicity of the centre row in a top-20 (0: nothing masked)
        nkept[b] = n;
        ncopy[b] = copies;
        dpad[b] = (n + (copies > 0 ? 1 : 0) + 31) & ~31;
    }
}

// exclusive scan of dpad -> roff (single workgroup; B is at most a few thousand per call)
__global__ __launch_bounds__(1024) void dg_scan_kernel(const int32_t* __restrict__ dpad, int32_t* __restrict__ roff, int B) {
    __shared__ int32_t part[1024];
    const int t = threadIdx.x;
    const int per = (B + 1023) / 1024;
    const int lo = t * per, hi = min(lo + per, B);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += dpad[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) { roff[i] = run; run += dpad[i]; }
    if (t == 1023) roff[B] = part[1023];
}

// rows of coalition b: kept points in index order, then the centre (once), then dead rows; (.,8) padded xyz
template <bool WIDE>
__global__ __launch_bounds__(64) void dg_compact_kernel(const float* __restrict__ clouds, const float* __restrict__ centers,
                                                        const int32_t* __restrict__ region_id, const uint64_t* __restrict__ keep,
                                                        const int32_t* __restrict__ cloud_of, const int32_t* __restrict__ roff,
                                                        const int32_t* __restrict__ nkept, const int32_t* __restrict__ ncopy,
                                                        float* __restrict__ x0, int32_t* __restrict__ row_cloud,
                                                        float* __restrict__ row_w, int N, int nclouds,
                                                        int16_t* __restrict__ src /*(B,Np) source point of a row, or null*/, int Np,
                                                        int R, int W) {
    __shared__ uint64_t strip[WIDE ? iq::kMaxKeepWords : 1];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int c = cloud_of ? cloud_of[b] : (nclouds == 1 ? 0 : b);
    const iq::WaveKeep<WIDE> k(keep, b, R, W, lane, strip);
    const int32_t* rid = region_id + (size_t)c * N;
    const float* xyz = clouds + (size_t)c * N * 3;
    const int base = roff[b], end = roff[b + 1];
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    int pos = 0;
    for (int i0 = 0; i0 < N; i0 += 64) {
        const int i = i0 + lane;
        const bool kept = i < N && k(rid[i]);
        const unsigned long long m = __ballot(kept);
        if (kept) {
            const int row = base + pos + __popcll(m & ((1ull << lane) - 1ull));
            const f32x4 a = {xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], 0.f};
            reinterpret_cast<f32x4*>(x0)[(size_t)row * 2] = a;
            reinterpret_cast<f32x4*>(x0)[(size_t)row * 2 + 1] = z;
            if (src) src[(size_t)b * Np + (row - base)] = (int16_t)i;
        }
        pos += __popcll(m);
    }
    const int live = nkept[b] + (ncopy[b] > 0 ? 1 : 0);   // ONE centre row; its multiplicity is applied by knn_kernel
    const f32x4 ctr = {centers[c * 3], centers[c * 3 + 1], centers[c * 3 + 2], 0.f};
    for (int row = base + nkept[b] + lane; row < end; row += 64) {
        reinterpret_cast<f32x4*>(x0)[(size_t)row * 2] = (row < base + live) ? ctr : z;
        reinterpret_cast<f32x4*>(x0)[(size_t)row * 2 + 1] = z;
    }
    const int nk = nkept[b];
    if (src && lane == 0 && ncopy[b] > 0) src[(size_t)b * Np + nk] = (int16_t)N;   // the centre row
    for (int row = base + lane; row < end; row += 64) {
        row_cloud[row] = b;
        const int rl = row - base;
        row_w[row] = rl < nk ? 1.f : (rl == nk && ncopy[b] > 0 ? (float)(N - nk) : 0.f);
    }
}

// ---- layer-1 graph of a coalition from the SOURCE cloud's sorted neighbour lists ---------------------------------------
// In xyz space the distance between two kept points does not depend on the coalition, and neither does the centre (the mean
// of the whole cloud): only the SET of candidates does.  So per source cloud (a few per call, against thousands of
// coalitions) every point's complete neighbour list - all other points and the centre, nearest first, by the very
// distances knn_kernel<8> computes - is built once (iq_srclist.h: sl_rows -> sl_dist -> sl_sort), and the 20 nearest of a
// coalition's query are the first entries of its source point's list that the coalition keeps, the centre entry counting
// min(M, 20) times (dg_walk_kernel: a few dozen 2-byte entries per query instead of a D x D distance matrix and a top-k).
// The same neighbours as knn_kernel<8> on the compact rows (same arithmetic for every distance, ties by point index).
// neighbour lists of the rows of coalition b from the sorted lists of its source cloud.  One wave = 64 query rows of one
// coalition.  The wave first builds the coalition's kept-point bitmap (N bits) and the prefix counts of its 32-bit words in
// LDS, so that "is point p kept" and "which compact row is it" (= the number of kept points before p) are two LDS reads
// and a popcount; the only global reads of the walk are the list entries themselves, eight per 16-byte load.
template <bool WIDE>
__global__ __launch_bounds__(64) void dg_walk_kernel(const int16_t* __restrict__ sorted, const int16_t* __restrict__ src,
                                                     const int32_t* __restrict__ region_id, const uint64_t* __restrict__ keep,
                                                     const int32_t* __restrict__ cloud_of, int16_t* __restrict__ idx, Ragged rg,
                                                     int N, int Np, int Nsl, int nclouds, int as_addr, int R, int W) {
    __shared__ uint64_t strip[WIDE ? iq::kMaxKeepWords : 1];
    __shared__ unsigned bits[kWalkMaxN / 32];
    __shared__ int pre[kWalkMaxN / 32];
    const int b = blockIdx.y, lane = threadIdx.x, r = blockIdx.x * 64 + lane;
    const int base = rg.roff[b], D = rg.roff[b + 1] - base;
    if (blockIdx.x * 64 >= D) return;                 // wave-uniform
    const int c = cloud_of ? cloud_of[b] : (nclouds == 1 ? 0 : b);
    const iq::WaveKeep<WIDE> k(keep, b, R, W, lane, strip);
    const int32_t* rid = region_id + (size_t)c * N;
    for (int i0 = 0; i0 < kWalkMaxN; i0 += 64) {      // kept bitmap, 64 points per step
        const int i = i0 + lane;
        const unsigned long long m = __ballot(i < N && k(rid[min(i, N - 1)]));
        if (lane == 0) { bits[i0 >> 5] = (unsigned)m; bits[(i0 >> 5) + 1] = (unsigned)(m >> 32); }
    }
    iq::wave_sync();
    if (lane < kWalkMaxN / 32) {                      // exclusive prefix of the word popcounts (32 words: a wave scan)
        const int cnt = __popc(bits[lane]);
        int run = cnt;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int v = __shfl_up(run, o, 64);
            if (lane >= o) run += v;
        }
        pre[lane] = run - cnt;
    }
    iq::wave_sync();
    if (r >= D) return;
    const int nk = rg.nkept[b], mult = rg.ncopy[b];
    const int live = nk + (mult > 0 ? 1 : 0);
    auto code = [&](int row) { return nb_encode(row, as_addr); };
    int16_t* o = idx + ((size_t)base + r) * kK;
    if (r >= live) {   // dead padding row: never read as a neighbour list that matters; keep it valid
#pragma unroll
        for (int q = 0; q < kK; ++q) o[q] = code(0);
        return;
    }
    const int16_t* list = sorted + ((size_t)c * (N + 1) + src[(size_t)b * Np + r]) * Nsl;
    int weight = 0, n = 0;
    for (int j0 = 0; j0 <= N && weight < kK; j0 += 8) {
        const uint4 chunk = *reinterpret_cast<const uint4*>(list + j0);   // Nsl is a multiple of 8: whole chunks
        const unsigned wds[4] = {chunk.x, chunk.y, chunk.z, chunk.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int p = (int)((wds[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            if (j0 + e > N || weight >= kK) continue;
            if (p == N) {
                if (mult > 0) { o[n++] = code(nk); weight += mult; }     // the centre stands for min(M, 20) identical points
            } else {
                const unsigned wbits = bits[p >> 5];
                if ((wbits >> (p & 31)) & 1u) {
                    o[n++] = code(pre[p >> 5] + __popc(wbits & ((1u << (p & 31)) - 1u)));
                    ++weight;
                }
            }
        }
    }
    const int16_t fill = code(mult > 0 ? nk : r);   // (only a cloud with fewer than 20 distinct rows gets here: it has a centre)
    for (; n < kK; ++n) o[n] = fill;
}

// ---- global max and mean pooling over the N points of each cloud: folded into conv5 (launch_linear_pool) -------------
// Kept rows count once, the centre (all copies identical) counts with its multiplicity M = N - kept (row_w).
// second stage of the pooling after launch_linear_pool: tiles of 32 rows never straddle clouds
__global__ __launch_bounds__(kThreads) void pool_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                               Ragged rg, int N, int C) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= C) return;
    const int t0 = rg.roff[b] >> 5, t1 = rg.roff[b + 1] >> 5;
    float m = -INFINITY, s = 0.f;
    for (int t = t0; t < t1; ++t) {
        const float* p = partial + (size_t)t * 2 * C;
        m = fmaxf(m, p[c]);
        s += p[C + c];
    }
    out[(size_t)b * 2 * C + c] = m;
    out[(size_t)b * 2 * C + C + c] = s / (float)N;
}

struct WsD {
    float* x0;      // (B,N,8)
    float* xc;      // (B,N,512)
    float* pq;      // (B,N,512)
    float* xx;      // (B,N)
    int16_t* idx;   // (B,N,20)
    int32_t* near_tie;  // (B,N) 21st candidate of a query whose neighbourhood boundary the float32 distances cannot decide, else -1
    float* h;       // (B*N/32, 2, 1024) per-tile max / weighted sum of conv5
    float *g, *f1, *f2;
    int32_t *roff, *nkept, *ncopy, *dpad, *row_cloud;  // ragged layout
    float* row_w;
    size_t bytes;
};

WsD carve_d(void* base, int B, int N) {
    WsD s{};
    iq::Carver c(base);
    const size_t r = (size_t)B * ((N + 31) / 32 * 32), b = (size_t)B;
    s.x0 = c.take<float>(r * 8);
    s.xc = c.take<float>(r * 512);
    s.pq = c.take<float>(r * 512);
    s.xx = c.take<float>(r);
    s.idx = c.take<int16_t>(r * kK);
    s.near_tie = c.take<int32_t>(r);
    s.h = c.take<float>(r * 64);  // pooling partials of conv5: (rows/32, 2, 1024)
    s.g = c.take<float>(b * 2048);
    s.f1 = c.take<float>(b * 512);
    s.f2 = c.take<float>(b * 256);
    s.roff = c.take<int32_t>(b + 1);
    s.nkept = c.take<int32_t>(b);
    s.ncopy = c.take<int32_t>(b);
    s.dpad = c.take<int32_t>(b);
    s.row_cloud = c.take<int32_t>(r);
    s.row_w = c.take<float>(r);
    s.bytes = c.bytes();
    return s;
}

__global__ void widen_idx_kernel(const int16_t* __restrict__ in, int32_t* __restrict__ out, size_t n) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = in[t];
}

}  // namespace

extern "C" size_t iq_dgcnn_workspace_bytes(int B, int N) {
    if (B < 0 || N < 0) return 0;
    return carve_d(nullptr, B, N).bytes;
}

// Op-level kNN for tests: x (B,N,C) row-major, C in {3, 64, 128}; idx (B,N,20) int32; tmp >= B*N*84 + 16*B + 8192 bytes
// (+ B*N*C*6 for the bf16x3 operand image of C = 64 / 128: without that room the fp32-MFMA kernels run).
extern "C" int iq_knn(const float* x, int32_t* idx, void* tmp, size_t tmp_bytes, int B, int N, int C, int k,
                      iq_stream_t stream) {
    IQ_REQUIRE(x && idx && tmp, "iq_knn: null pointer");
    IQ_REQUIRE(k == kK, "iq_knn: k=%d (only k=20, tools/final_util.py:19)", k);
    IQ_REQUIRE(B >= 1 && N >= 32 && N % 32 == 0 && N <= 32767, "iq_knn: N=%d must be a multiple of 32", N);
    IQ_REQUIRE(C == 3 || C == 64 || C == 128, "iq_knn: C=%d unsupported", C);
    const size_t r = (size_t)B * N;
    IQ_REQUIRE(tmp_bytes >= r * 84 + (size_t)B * 16 + 8192, "iq_knn: tmp too small");
    hipStream_t st = iq::as_stream(stream);
    iq::Carver c(tmp);
    float* x0 = c.take<float>(r * 8);
    float* xx = c.take<float>(r);
    int16_t* i16 = c.take<int16_t>(r * kK);
    int32_t* near_tie = c.take<int32_t>(r);
    int32_t* row_cloud = c.take<int32_t>(r);
    int32_t* roff = c.take<int32_t>((size_t)B + 1);
    int32_t* nkept = c.take<int32_t>((size_t)B);
    int32_t* ncopy = c.take<int32_t>((size_t)B);
    IQ_LAUNCH(dg_dense_layout_kernel, dim3((r + 256) / 256), dim3(256), 0, st, roff, nkept, ncopy, row_cloud, nullptr, B, N, N);
    const Ragged rg{roff, nkept, ncopy, row_cloud, nullptr};
    const float* src = x;
    int ld = C, cpad = C;
    if (C == 3) {
        IQ_LAUNCH(pad_xyz_kernel, dim3((r + 255) / 256), dim3(256), 0, st, x, x0, B, N, N);
        src = x0; ld = 8; cpad = 8;
    }
    // room for the bf16x3 operand image behind the other scratch: the distances of the feature-space graphs run on the bf16 matrix
    // pipe, as in the model path (twins kTwinKnnFp32Mfma / kTwinKnnFp32Rank: the fp32 MFMA kernels)
    const bool fp32 = iq::twin() == iq::kTwinKnnFp32Mfma || iq::twin() == iq::kTwinKnnFp32Rank;
    unsigned char* planes = nullptr;
    if ((C == 64 || C == 128) && !fp32 && tmp_bytes >= c.bytes() + r * C * 6) planes = c.take<unsigned char>(r * C * 6);
    IQ_LAUNCH(rownorm_kernel, dim3((r + 63) / 64), dim3(kThreads), 0, st, src, ld, C, xx, rg, B, planes, (int)(r / 32));
    IQ_TRY(launch_knn(src, ld, cpad, xx, i16, near_tie, B, N, (int)r, rg, st, false, planes, (int)(r / 32)));
    IQ_LAUNCH(widen_idx_kernel, dim3((r * kK + 255) / 256), dim3(256), 0, st, i16, idx, r * kK);
    return IQ_OK;
}

namespace {

// The network on the ragged rows described by s.roff / s.nkept / s.ncopy / s.row_cloud; s.x0 holds the padded xyz rows.
// `rows` = upper bound of the row count (grid sizes); the live count is roff[B], on the device.
// Layer-1 graph from the source clouds' sorted neighbour lists (dg_walk_kernel) instead of rownorm + knn_kernel<8>
struct WalkCtx {
    const int16_t* sorted;   // (nclouds, N+1, Nsl)
    const int16_t* src;      // (B, Np)
    const int32_t* region_id;
    const uint64_t* keep;
    const int32_t* cloud_of;
    int nclouds, Nsl;
    int R, W;                // wide game: keep is (B, W) rows over R regions; W = 0: uint64 masks
};

int run_network(const iq_dgcnn_weights* w, const WsD& s, float* logits, int B, int N, int rows, int fixed_graph,
                hipStream_t st, const WalkCtx* walk = nullptr) {
    const Ragged rg{s.roff, s.nkept, s.ncopy, s.row_cloud, s.row_w};
    const int32_t* live = s.roff + B;
    const float* src = s.x0;
    int ld = 8, cin = 8, creal = 3, col = 0;
    const int Np = (N + 31) / 32 * 32;
    // edge_fused_kernel for every layer or for none: the kNN kernel writes the neighbour lists in the form the consumer reads
    // (LDS addresses for the fused kernel, row indices otherwise), and GCNN's one list serves all four layers
    const bool fused = fused_path(w, N);
    for (int l = 0; l < 4; ++l) {
        const int co = w->pq[l].cout / 2;
        IQ_REQUIRE(w->pq[l].cin == cin, "iq_dgcnn: layer %d expects %d inputs, got %d", l, cin, w->pq[l].cin);
        if (l == 0 && walk) {
            iq::ProfileSpan span(iq::kSlotPrepool, st);
            IQ_LAUNCH((walk->W ? dg_walk_kernel<true> : dg_walk_kernel<false>), dim3((Np + 63) / 64, B), dim3(64), 0, st,
                      walk->sorted, walk->src, walk->region_id, walk->keep, walk->cloud_of, s.idx, rg, N, Np, walk->Nsl,
                      walk->nclouds, fused ? 1 : 0, walk->R, walk->W);
        } else if (l == 0 || !fixed_graph) {
            iq::ProfileSpan span(iq::kSlotPrepool, st);
            // feature-space graphs of the fused path: distances on the bf16 matrix pipe, the operand image in the upper half of the
            // P/Q buffer (which the fused path leaves alone; the walk tables keep to the lower half).  Twins kTwinKnnFp32Mfma and
            // kTwinKnnFp32Rank: the fp32 MFMA (A/B, tests)
            const bool bf3 = fused && (cin == 64 || cin == 128) && iq::twin() != iq::kTwinKnnFp32Mfma && iq::twin() != iq::kTwinKnnFp32Rank;
            unsigned char* planes = bf3 ? reinterpret_cast<unsigned char*>(s.pq) + (size_t)rows * 1024 : nullptr;
            IQ_LAUNCH(rownorm_kernel, dim3((rows + 63) / 64), dim3(kThreads), 0, st, src, ld, creal, s.xx, rg, B, planes, rows / 32);
            IQ_TRY(launch_knn(src, ld, cin, s.xx, s.idx, s.near_tie, B, N, rows, rg, st, fused, planes, rows / 32));
        }
        {
            iq::ProfileSpan span(iq::kSlotFstn, st);
            IQ_TRY(launch_edgeconv(fused, src, ld, w->pq[l], s.idx, s.pq, s.xc + col, 512, rg, B, Np, rows, live, st));
        }
        src = s.xc + col; ld = 512; cin = co; creal = co; col += co;
    }
    IQ_REQUIRE(col == 512, "iq_dgcnn: concatenated width %d != 512", col);
    {
        iq::ProfileSpan span(iq::kSlotTrunk, st);
        // conv5 + LeakyReLU with the pooling folded into the GEMM epilogue (s.h holds the per-tile partials)
        IQ_REQUIRE(w->conv5.cout == 1024 && w->conv5.cin == 512, "iq_dgcnn: conv5 must be 512 -> 1024");
        double work = 0.0;
        if (iq::profile_enabled()) {  // profiling only: the live row count (one sync); the GEMM issues whole 128-row tiles
            int32_t n = 0;
            if (hipMemcpyAsync(&n, live, sizeof(n), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
                work = 2.0 * 512.0 * 1024.0 * (double)((n + 127) / 128 * 128);
        }
        iq::ProfileSpan dom(iq::kSlotDominant, st, work);
        IQ_TRY(iq::launch_linear_pool(s.xc, 512, w->conv5, s.h, rows, 2, s.row_w, st, live, w->conv5_bf3));
        IQ_LAUNCH(pool_reduce_kernel, dim3(1024 / kThreads, B), dim3(kThreads), 0, st, s.h, s.g, rg, N, 1024);
    }
    IQ_TRY(iq::launch_linear(s.g, 2048, w->fc1, s.f1, 512, B, 2, st));
    IQ_TRY(iq::launch_linear(s.f1, 512, w->fc2, s.f2, 256, B, 2, st));
    IQ_TRY(iq::launch_linear(s.f2, 256, w->fc3, logits, w->fc3.cout, B, 0, st));
    return IQ_OK;
}

}  // namespace

extern "C" int iq_dgcnn_forward(const iq_dgcnn_weights* w, const float* xyz, float* logits, void* workspace,
                                size_t workspace_bytes, int B, int N, int fixed_graph, iq_stream_t stream) {
    IQ_REQUIRE(w && xyz && logits, "iq_dgcnn_forward: null pointer");
    IQ_REQUIRE(B >= 0 && N >= kK && N <= 32767, "iq_dgcnn_forward: N=%d not in [%d, 32767]", N, kK);
    IQ_REQUIRE(w->k == kK, "iq_dgcnn_forward: k=%d (only 20)", w->k);
    if (B == 0) return IQ_OK;
    const size_t need = carve_d(nullptr, B, N).bytes;
    if (!workspace || workspace_bytes < need)
        return iq::fail(IQ_EWORKSPACE, "iq_dgcnn_forward: workspace %zu < %zu bytes", workspace_bytes, need);
    WsD s = carve_d(workspace, B, N);
    hipStream_t st = iq::as_stream(stream);
    const int Np = (N + 31) / 32 * 32;  // rows N..Np-1 of every cloud are dead padding
    const int rows = B * Np;
    iq::ProfileSpan call_span(iq::kSlotCall, st);
    IQ_LAUNCH(dg_dense_layout_kernel, dim3((rows + 256) / 256), dim3(256), 0, st, s.roff, s.nkept, s.ncopy,
              s.row_cloud, s.row_w, B, N, Np);
    IQ_LAUNCH(pad_xyz_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, xyz, s.x0, B, N, Np);
    return run_network(w, s, logits, B, N, rows, fixed_graph, st);
}

namespace {

// iq_dgcnn_coalitions (W = 0: keep holds B uint64 masks) and iq_dgcnn_coalitions_wide (keep holds (B, W) rows of an R-region game):
// the count, the compaction and the walk's bitmap read the coalition, everything after them works on its rows
int dgcnn_coalitions(const char* name, const iq_dgcnn_weights* w, const float* clouds, const float* centers, const int32_t* region_id,
                     const uint64_t* keep, const int32_t* cloud_of, float* logits, void* workspace, size_t workspace_bytes, int B,
                     int nclouds, int N, int fixed_graph, int R, int W, iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && nclouds >= 1, "%s: B=%d nclouds=%d", name, B, nclouds);
    IQ_REQUIRE(w && clouds && centers && region_id && (B == 0 || (keep && logits)), "%s: null pointer", name);
    IQ_REQUIRE(N >= kK && N <= 32767, "%s: N=%d not in [%d, 32767]", name, N, kK);
    IQ_REQUIRE(cloud_of || nclouds == 1 || nclouds == B, "%s: cloud_of required when 1 < nclouds != B", name);
    IQ_REQUIRE(w->k == kK, "%s: k=%d (only 20)", name, w->k);
    if (B == 0) return IQ_OK;
    const size_t need = carve_d(nullptr, B, N).bytes;
    if (!workspace || workspace_bytes < need)
        return iq::fail(IQ_EWORKSPACE, "%s: workspace %zu < %zu bytes", name, workspace_bytes, need);
    WsD s = carve_d(workspace, B, N);
    hipStream_t st = iq::as_stream(stream);
    iq::ProfileSpan call_span(iq::kSlotCall, st);
    // Layer-1 graph from the source clouds' sorted neighbour lists when a few source clouds serve many coalitions.  The
    // tables are carved from the P/Q buffer, which the fused EdgeConv path does not touch (twin kTwinKnnCompact: knn_kernel<8>).
    const int Np = (N + 31) / 32 * 32, Nsp = (N + 1 + 31) / 32 * 32, Nsl = (N + 1 + 7) / 8 * 8;
    WalkCtx walk{};
    bool use_walk = false;
    {
        iq::Carver c(s.pq);
        float* xs = c.take<float>((size_t)nclouds * Nsp * 8);
        float* xxs = c.take<float>((size_t)nclouds * Nsp);
        float* dmat = c.take<float>((size_t)nclouds * Nsp * Nsp);
        int16_t* sorted = c.take<int16_t>((size_t)nclouds * (N + 1) * Nsl);
        int16_t* srcrow = c.take<int16_t>((size_t)B * Np);
        use_walk = N <= kWalkMaxN && (long long)nclouds * 8 <= B && fused_path(w, N) && iq::twin() != iq::kTwinKnnCompact &&
                   c.bytes() <= (size_t)B * Np * 256 * 4;     // the lower half: the upper one holds the kNN operand image (run_network)
        if (use_walk) {
            IQ_LAUNCH(sl_rows_kernel, dim3((Nsp + 255) / 256, nclouds), dim3(256), 0, st, clouds, centers, xs, xxs, N, Nsp);
            IQ_LAUNCH(sl_dist_kernel<0>, dim3(Nsp / 32, nclouds), dim3(64), 0, st, xs, xxs, dmat, Nsp);
            IQ_LAUNCH(sl_sort_kernel, dim3(N + 1, nclouds), dim3(256), 0, st, dmat, sorted, N, Nsp, Nsl);
            walk = WalkCtx{sorted, srcrow, region_id, keep, cloud_of, nclouds, Nsl, R, W};
        }
    }
    IQ_LAUNCH((W ? dg_count_kernel<true> : dg_count_kernel<false>), dim3(B), dim3(64), 0, st, region_id, keep, cloud_of,
              s.nkept, s.ncopy, s.dpad, N, nclouds, R, W);
    IQ_LAUNCH(dg_scan_kernel, dim3(1), dim3(1024), 0, st, s.dpad, s.roff, B);
    IQ_LAUNCH((W ? dg_compact_kernel<true> : dg_compact_kernel<false>), dim3(B), dim3(64), 0, st, clouds, centers, region_id,
              keep, cloud_of, s.roff, s.nkept, s.ncopy, s.x0, s.row_cloud, s.row_w, N, nclouds,
              use_walk ? const_cast<int16_t*>(walk.src) : nullptr, Np, R, W);
    return run_network(w, s, logits, B, N, B * Np, fixed_graph, st, use_walk ? &walk : nullptr);
}

}  // namespace

extern "C" int iq_dgcnn_coalitions(const iq_dgcnn_weights* w, const float* clouds, const float* centers,
                                   const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of, float* logits,
                                   void* workspace, size_t workspace_bytes, int B, int nclouds, int N, int fixed_graph,
                                   iq_stream_t stream) {
    return dgcnn_coalitions("iq_dgcnn_coalitions", w, clouds, centers, region_id, keep, cloud_of, logits, workspace, workspace_bytes, B,
                            nclouds, N, fixed_graph, 64, 0, stream);
}

extern "C" int iq_dgcnn_coalitions_wide(const iq_dgcnn_weights* w, const float* clouds, const float* centers,
                                        const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of, float* logits,
                                        void* workspace, size_t workspace_bytes, int B, int nclouds, int N, int fixed_graph, int R,
                                        iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_dgcnn_coalitions_wide: R=%d not in [1,%d]", R, IQ_MAX_WIDE_REGIONS);
    return dgcnn_coalitions("iq_dgcnn_coalitions_wide", w, clouds, centers, region_id, keep, cloud_of, logits, workspace,
                            workspace_bytes, B, nclouds, N, fixed_graph, R, iq::keep_words(R), stream);
}
