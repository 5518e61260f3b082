// DGCNN's EdgeConv layer, out[i][c] = LeakyReLU(max_j P[idx[i][j]][c] + Q[i][c]) (iq_dgcnn.hip's file comment), on three routes:
// edge_fused_kernel (GEMM and neighbourhood max in one kernel), or the GEMM of iq_linear.hip followed by gather_lds_kernel
// or gather_max_kernel.  fused_path decides per forward, launch_edgeconv per layer.  Included by iq_dgcnn.hip alone.
#pragma once
#include "iq_dgcnn_knn.h"
#include "iq_twin.h"

namespace {

// the kK neighbours of a query from the five 8-byte words of its list (iq_dgcnn_knn.h, "neighbour lists")
template <class T>
__device__ __forceinline__ void nb_unpack(const uint2 (&w)[kK / 4], T (&nb)[kK]) {
#pragma unroll
    for (int i = 0; i < kK / 4; ++i) {
        nb[4 * i] = (T)(w[i].x & 0xffffu); nb[4 * i + 1] = (T)(w[i].x >> 16);
        nb[4 * i + 2] = (T)(w[i].y & 0xffffu); nb[4 * i + 3] = (T)(w[i].y >> 16);
    }
}

// LeakyReLU(0.2) of the neighbourhood maximum plus the query's own term
__device__ __forceinline__ f32x4 leaky_sum(f32x4 m, f32x4 q) {
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float y = m[e] + q[e];
        o[e] = y > 0.f ? y : 0.2f * y;
    }
    return o;
}

// ---- the gather straight from L2 ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gather_max_kernel(const float* __restrict__ pq, int Co,
                                                              const int16_t* __restrict__ idx, float* __restrict__ out,
                                                              int ldo, Ragged rg, int B, int wgs_per_cloud) {
    const int per = Co / 4;                               // float4 lanes per point
    // Workgroups go round-robin over the 8 XCDs: give each XCD whole clouds (cloud b -> XCD b % 8, its workgroups
    // consecutive there), so that the ~20 reads of every P row of a cloud hit ONE L2.  In plain block order the rows of a
    // cloud were pulled into all eight L2s: FETCH_SIZE showed 4-9x the bytes of the PQ matrix per launch at 57 % L2 hit
    // rate and the kernel ran at the fabric's 6.4 TB/s (profiles/r02_stream_kernels.csv).  Adjacent clouds run on
    // adjacent XCDs at the same time, so the eight row streams stay close together in memory.
    const int slot = blockIdx.x >> 3;
    const int b = iq::xcd_cloud(blockIdx.x, wgs_per_cloud, B);
    if (b >= B) return;
    const int base = rg.roff[b];
    const int pt = base + (slot % wgs_per_cloud) * (kThreads / per) + threadIdx.x / per;
    const int c4 = threadIdx.x % per;
    if (pt >= rg.roff[b + 1]) return;
    // the 20 neighbour indices of the point: 40 contiguous bytes, read as five 8-byte words
    const uint2* nbw = reinterpret_cast<const uint2*>(idx + (size_t)pt * kK);
    const uint2 words[kK / 4] = {nbw[0], nbw[1], nbw[2], nbw[3], nbw[4]};
    int nb[kK];
    nb_unpack(words, nb);
    // All 20 row loads of a thread are in flight together, as raw buffer loads with 32-bit offsets on a resource based at
    // this cloud's first row (one multiply-add of address arithmetic per load instead of a 64-bit chain).
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pq) + (size_t)base * (2 * Co), 0, 0x7fffffff, 0x00020000);
    const int row_bytes = 2 * Co * 4;
    f32x4 v[kK];
#pragma unroll
    for (int j = 0; j < kK; ++j)
        v[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, nb[j] * row_bytes + c4 * 16, 0, 0));
    const f32x4 q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, (pt - base) * row_bytes + (per + c4) * 16, 0, 0));
    f32x4 m = v[0];
#pragma unroll
    for (int j = 1; j < kK; ++j) {
        m[0] = fmaxf(m[0], v[j][0]); m[1] = fmaxf(m[1], v[j][1]); m[2] = fmaxf(m[2], v[j][2]); m[3] = fmaxf(m[3], v[j][3]);
    }
    *reinterpret_cast<f32x4*>(out + (size_t)pt * ldo + c4 * 4) = leaky_sum(m, q);
}

// ---- the same with the P rows of a cloud staged in LDS -----------------------------------------------------------------
// Every P row of a cloud is read ~20 times (once per query that has it among its neighbours), in no order the caches can
// use: gather_max_kernel moves 20 x the P matrix through the texture-address path and L2 (7 TB/s measured, the fabric's
// limit).  Here a workgroup owns (cloud, channel chunk): it streams its D x cw slice of P into LDS once (coalesced, every
// byte of P leaves L2 once), and the 20 reads per output come from LDS.  cw is chosen per cloud so that the slice fills the
// 64 KB budget (D <= 256: 64 channels, <= 512: 32, <= 1024: 16); the grid holds Co / 16 workgroups per cloud and the
// surplus ones of small clouds exit at once.  Two workgroups per CU: one streams while the other gathers.
// max() is order-independent on the finite values here, so the result is bit-identical to gather_max_kernel.
constexpr int kGlThreads = 512;
constexpr int kGlFloats = 16384;   // 64 KB of P slice per workgroup
constexpr int kGlMaxRows = 1024;   // D * 16 channels must fit

__global__ __launch_bounds__(kGlThreads, 4) void gather_lds_kernel(const float* __restrict__ pq, int Co,
                                                                const int16_t* __restrict__ idx, float* __restrict__ out,
                                                                int ldo, Ragged rg, int B, int wgs_per_cloud) {
    __shared__ f32x4 slice[kGlFloats / 4];
    const int slot = blockIdx.x >> 3;   // whole clouds per XCD, as in gather_max_kernel
    const int b = iq::xcd_cloud(blockIdx.x, wgs_per_cloud, B);
    if (b >= B) return;
    const int base = rg.roff[b];
    const int D = rg.roff[b + 1] - base;
    int shift = 2;                                            // log2(float4 lanes per row of the slice)
    if (D * 32 <= kGlFloats && Co >= 32) shift = 3;
    if (D * 64 <= kGlFloats && Co >= 64) shift = 4;
    const int per = 1 << shift, cw = 4 * per;
    const int chunk = slot % wgs_per_cloud;
    if (chunk * cw >= Co || D == 0) return;
    const int c0 = chunk * cw;                                // first channel of this workgroup
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(pq) + (size_t)base * (2 * Co), 0, 0x7fffffff, 0x00020000);
    const int row_bytes = 2 * Co * 4;
    const int items = D << shift;                             // (row, float4 lane) pairs, <= 4096; D % 32 == 0
    const int tid = threadIdx.x;
    // the neighbour lists (40 bytes per row, five 8-byte words) and the Q values of an item; the first item's are
    // requested before the slice, every later item's one item ahead
    const __amdgpu_buffer_rsrc_t irsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<int16_t*>(idx) + (size_t)base * kK, 0, 0x7fffffff, 0x00020000);
    struct Item { uint2 w[kK / 4]; f32x4 q; };
    auto fetch = [&](int t) {
        Item it;
        const int r = min(t, items - 1) >> shift, c4 = t & (per - 1);
#pragma unroll
        for (int w = 0; w < kK / 4; ++w) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(irsrc, r * (kK * 2) + 8 * w, 0, 0);
            it.w[w] = __builtin_bit_cast(uint2, v);
        }
        it.q = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, r * row_bytes + (Co + c0 + 4 * c4) * 4, 0, 0));
        return it;
    };
    Item cur = fetch(tid);
    // phase 1: the slice, all (up to eight) loads of a thread in flight (items is a multiple of 128, at most 4096)
    {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int t = tid + u * kGlThreads;
            const int off = (t >> shift) * row_bytes + (c0 + 4 * (t & (per - 1))) * 4;
            if (t < items) v[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 0));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int t = tid + u * kGlThreads;
            if (t < items) slice[t] = v[u];
        }
    }
    __syncthreads();
    // phase 2
    const unsigned last = (unsigned)D - 1u;
    for (int t = tid; t < items; t += kGlThreads) {
        const int r = t >> shift, c4 = t & (per - 1);
        const Item it = cur;
        if (t + kGlThreads < items) cur = fetch(t + kGlThreads);
        const f32x4 q = it.q;
        unsigned nb[kK];
        nb_unpack(it.w, nb);
        f32x4 m = slice[(min(nb[0], last) << shift) + c4];
#pragma unroll
        for (int j = 1; j < kK; ++j) {
            const f32x4 v = slice[(min(nb[j], last) << shift) + c4];   // min: rows outside the slice are never addressed
            m[0] = fmaxf(m[0], v[0]); m[1] = fmaxf(m[1], v[1]); m[2] = fmaxf(m[2], v[2]); m[3] = fmaxf(m[3], v[3]);
        }
        *reinterpret_cast<f32x4*>(out + (size_t)(base + r) * ldo + c0 + 4 * c4) = leaky_sum(m, q);
    }
}

// ---- EdgeConv layer in one kernel: P/Q GEMM + neighbourhood max --------------------------------------------------------
// out[i][c] = LeakyReLU(max_j P[idx[i][j]][c] + Q[i][c]) with [P | Q] = x W^T + bias computed HERE: the (rows, 2 Co) matrix
// never goes to HBM (the separate GEMM wrote it and the gather read it back: 2 x 8 KB per row over the four layers, and
// both ran at 2-3 TB/s).  A workgroup owns (cloud, 16 output channels).  The MFMA runs TRANSPOSED: its 32 "rows" are 32
// columns of the layer - 16 of P and the 16 of Q for the same channels - and its 32 "columns" are 32 points, so one
// 32x32 tile gives a lane (point = lane & 31, half h) P and Q of 8 channels of its point:
//     accumulator i:  0-3  P[4h + i]    4-7  P[8 + 4h + (i-4)]    8-11  Q[4h + (i-8)]    12-15  Q[8 + 4h + (i-12)]
// (weights are the A operand: lane m = lane & 31 holds column m < 16 ? c0 + m : Co + c0 + m - 16 of the packed image;
// products and the order over k are those of the plain GEMM, so the results are bit-identical to launch_linear +
// gather_max_kernel).  P goes to LDS (D x 16 floats <= 64 KB), Q stays in the accumulators; after the barrier every lane
// takes the maxima of its point's 20 neighbours from LDS (two 16-byte reads per neighbour) and writes 2 x 16 bytes.
// Two workgroups per CU: the MFMA phase of one runs under the LDS phase of the other.
//
// Operands.  The 32 x Cin weight slice of the workgroup (<= 16 KB) is staged in LDS once and read from there as
// fragments.  A wave works through its point tiles one after the other, a stage = the four k-blocks of a 128-byte line
// of x; the x fragments (global) and weight fragments (LDS) of stage q + 1 are requested before the MFMAs of stage q.
// (Measured and of no effect: perfectly coalesced fake x addresses, x groups 2-4 stages ahead.)
template <int KB>   // Cin / 8
__global__ __launch_bounds__(kGlThreads, 4) void edge_fused_kernel(const float* __restrict__ x, int ldx,
                                                                   const float* __restrict__ wp, const float* __restrict__ bias,
                                                                   int Co, const int16_t* __restrict__ idx,
                                                                   float* __restrict__ out, int ldo, Ragged rg, int B,
                                                                   int wgs_per_cloud) {
    constexpr int G = KB >= 4 ? 4 : KB;                       // k-blocks per group (one 128-byte line of x when KB >= 4)
    constexpr int NG = KB / G;
    __shared__ f32x4 slice[kGlFloats / 4];                    // [row][4 float4]
    __shared__ f32x4 wl[KB * 64];                             // weight fragments [kb][lane]
    const int slot = blockIdx.x >> 3;   // whole clouds per XCD, as in gather_max_kernel
    const int b = iq::xcd_cloud(blockIdx.x, wgs_per_cloud, B);
    if (b >= B) return;
    const int base = rg.roff[b];
    const int D = rg.roff[b + 1] - base;                      // multiple of 32, <= kGlMaxRows (host)
    if (D == 0) return;
    const int c0 = (slot % wgs_per_cloud) * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int p = lane & 31, h = lane >> 5;
    const int ntiles = D >> 5;
    const int nv = min(4, max(0, (ntiles - wave + 7) >> 3));  // this wave's point tiles: wave, wave + 8, ... (wave-uniform)

    // weight slice -> LDS: entry e = (kb, lane l) is the fragment element of MFMA row m = l & 31, half l >> 5
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wp), 0, 0x7fffffff, 0x00020000);
    for (int e = tid; e < KB * 64; e += kGlThreads) {
        const int kb = e >> 6, l = e & 63, m = l & 31;
        const int n = m < 16 ? c0 + m : Co + c0 + m - 16;     // layer column in MFMA row m
        wl[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, ((((n >> 5) * KB + kb) * 64) + (n & 31) + (l & 32)) * 16, 0, 0));
    }
    const __amdgpu_buffer_rsrc_t xrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x) + (size_t)base * ldx, 0, 0x7fffffff, 0x00020000);
    auto xvoff = [&](int u) { return ((min(wave + 8 * u, ntiles - 1) * 32 + p) * ldx + 4 * h) * 4; };
    struct XG { f32x4 f[G]; };
    auto xgroup = [&](int voff, int g) {
        XG r;
#pragma unroll
        for (int j = 0; j < G; ++j) r.f[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xrs, voff, (g * G + j) * 32, 0));
        return r;
    };
    // Operand pipeline: the x group (global) and the weight group (LDS) of stage q + 1 are requested before the MFMAs of
    // stage q (a stage = G k-blocks of one tile = 4 G MFMAs); sched_group_barrier pins that order - left alone the
    // scheduler read two weight fragments, waited for them, issued 8 MFMAs, read the next two ... and the wave stood
    // still for an LDS round trip (behind the other workgroup's gather traffic) every 8 MFMAs: 50 % MFMA-busy.
    constexpr int TOTAL = 4 * NG;
    struct WGp { f32x4 f[G]; };
    auto wgroup = [&](int g) {
        WGp r;
#pragma unroll
        for (int j = 0; j < G; ++j) r.f[j] = wl[(g * G + j) * 64 + lane];
        return r;
    };
    XG xr[2];
    WGp wr[2];
    xr[0] = xgroup(xvoff(0), 0);
    const __amdgpu_buffer_rsrc_t irs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<int16_t*>(idx) + (size_t)base * kK, 0, 0x7fffffff, 0x00020000);
    struct Nb { uint2 w[kK / 4]; };
    auto fetch_nb = [&](int u) {
        Nb v;
        const int r = min(wave + 8 * u, ntiles - 1) * 32 + p;
#pragma unroll
        for (int w = 0; w < kK / 4; ++w) v.w[w] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(irs, r * (kK * 2) + 8 * w, 0, 0));
        return v;
    };
    // bias of the 16 channels (P) and of their Q columns: wave-uniform, in SGPRs; a lane picks its 8 by h
    float bps[16], bqs[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        bps[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bias[c0 + e])));
        bqs[e] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bias[Co + c0 + e])));
    }
    __syncthreads();                                          // wl complete
    wr[0] = wgroup(0);

    // The slice is XOR-swizzled (iq_dgcnn_knn.h, "neighbour lists").  Unswizzled, the 16 lanes of a ds_read_b128 lane group (same h,
    // random rows) all read column h: 16 of the 64 banks; swizzled, one of 16 slots (measured: 7 conflict cycles per LDS instruction).
    f32x4 q0[4], q1[4];                                       // Q of this lane's channels, per tile
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < nv) {
            f32x16 acc = {0};
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int q = u * NG + g;
                const XG xf = xr[q & 1];
                const WGp wf = wr[q & 1];
                if (q + 1 < TOTAL) {
                    const int un = (q + 1) / NG;              // compile-time after unrolling
                    xr[(q + 1) & 1] = xgroup(xvoff(min(un, nv - 1)), (q + 1) % NG);
                    wr[(q + 1) & 1] = wgroup((q + 1) % NG);
                }
#pragma unroll
                for (int j = 0; j < G; ++j) acc = mfma4(wf.f[j], xf.f[j], acc);
                if (q + 1 < TOTAL) {
                    __builtin_amdgcn_sched_group_barrier(0x020, G, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, G, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 4 * G, 0);
            }
            const int r = (wave + 8 * u) * 32 + p;
            f32x4 p0, p1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                p0[e] = acc[e] + (h ? bps[4 + e] : bps[e]); p1[e] = acc[4 + e] + (h ? bps[12 + e] : bps[8 + e]);
                q0[u][e] = acc[8 + e] + (h ? bqs[4 + e] : bqs[e]); q1[u][e] = acc[12 + e] + (h ? bqs[12 + e] : bqs[8 + e]);
            }
            const int a = r * 4 + (h ^ ((r >> 2) & 3));
            slice[a] = p0;
            slice[a ^ 2] = p1;
        }
    }
    Nb cur = fetch_nb(0);                                     // neighbour lists of the first tile (in flight across the barrier)
    __syncthreads();                                          // slice complete
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < nv) {
            const Nb it = cur;
            if (u + 1 < nv) cur = fetch_nb(u + 1);
            const int r = (wave + 8 * u) * 32 + p;
            // the lists hold LDS byte addresses (nb_encode, as_addr): this lane's two float4 are at (address ^ 16 h) and that ^ 32
            unsigned nb[kK];
            nb_unpack(it.w, nb);
            const char* sb = reinterpret_cast<const char*>(slice);
            const unsigned hx = (unsigned)h << 4;
            auto rd = [&](unsigned a) { return *reinterpret_cast<const f32x4*>(sb + a); };
            f32x4 m0 = rd(nb[0] ^ hx), m1 = rd(nb[0] ^ hx ^ 32u);
#pragma unroll
            for (int j = 1; j < kK; ++j) {
                const unsigned a = nb[j] ^ hx;
                const f32x4 v0 = rd(a), v1 = rd(a ^ 32u);
#pragma unroll
                for (int e = 0; e < 4; ++e) { m0[e] = fmaxf(m0[e], v0[e]); m1[e] = fmaxf(m1[e], v1[e]); }
            }
            float* o = out + (size_t)(base + r) * ldo + c0 + 4 * h;
            *reinterpret_cast<f32x4*>(o) = leaky_sum(m0, q0[u]);
            *reinterpret_cast<f32x4*>(o + 8) = leaky_sum(m1, q1[u]);
        }
    }
}

// does run_network take the fused EdgeConv path?  (the walk tables live in the P/Q buffer that only the other path uses)
bool fused_path(const iq_dgcnn_weights* w, int N) {
    // twins kTwinEdgeGemmL2 / kTwinEdgeGemmLds: GEMM + L2 gather / GEMM + LDS gather (A/B and tests)
    bool fused = (N + 31) / 32 * 32 <= kGlMaxRows && iq::twin() != iq::kTwinEdgeGemmL2 && iq::twin() != iq::kTwinEdgeGemmLds;
    int ci = 8;
    for (int l = 0; l < 4; ++l) {
        const int co = w->pq[l].cout / 2;
        fused = fused && co % 16 == 0 && (ci == 8 || ci == 64 || ci == 128) && w->pq[l].cin == ci;
        ci = co;
    }
    return fused;
}

// One EdgeConv layer on the route the forward takes: x (rows, ldx) with L.cin inputs -> out (rows, ldo), L.cout / 2 channels.
// `fused` = fused_path() of this forward (idx then holds LDS addresses); pq (rows, L.cout) is scratch of the two GEMM routes only.
// Np = rows of the largest cloud; rows / live = upper bound / device count of all rows.
int launch_edgeconv(bool fused, const float* x, int ldx, const iq_dense_layer& L, const int16_t* idx, float* pq, float* out, int ldo,
                    const Ragged& rg, int B, int Np, int rows, const int32_t* live, hipStream_t st) {
    const int co = L.cout / 2;
    // whole clouds per XCD (iq::xcd_cloud): the grid covers a multiple of eight clouds
    auto grid = [&](int wgs_per_cloud) { return dim3((unsigned)((B + 7) / 8 * 8 * wgs_per_cloud)); };
    if (fused) {
        // the whole layer in one kernel: co / 16 workgroups per cloud
        const auto kernel = L.cin == 8 ? edge_fused_kernel<1> : L.cin == 64 ? edge_fused_kernel<8> : edge_fused_kernel<16>;
        IQ_TRY(iq::launch("edge_fused_kernel", kernel, grid(co / 16), dim3(kGlThreads), 0, st, x, ldx, L.w, L.b, co, idx, out, ldo, rg, B, co / 16));
        return IQ_OK;
    }
    IQ_TRY(iq::launch_linear(x, ldx, L, pq, 2 * co, rows, 0, st, live));
    if (Np <= kGlMaxRows && co % 16 == 0 && iq::twin() != iq::kTwinEdgeGemmL2) {
        // P slices through LDS: co / 16 workgroups per cloud (the surplus ones of small clouds exit at once)
        IQ_LAUNCH(gather_lds_kernel, grid(co / 16), dim3(kGlThreads), 0, st, pq, co, idx, out, ldo, rg, B, co / 16);
    } else {
        // clouds of more than 1024 rows (or twin kTwinEdgeGemmL2): straight from L2.  Grid sized for the largest cloud (Np rows);
        // workgroups past a cloud's live row count exit at once
        const int pts_per_wg = kThreads / (co / 4);
        const int wgs_per_cloud = (Np + pts_per_wg - 1) / pts_per_wg;
        IQ_LAUNCH(gather_max_kernel, grid(wgs_per_cloud), dim3(kThreads), 0, st, pq, co, idx, out, ldo, rg, B, wgs_per_cloud);
    }
    return IQ_OK;
}

}  // namespace
