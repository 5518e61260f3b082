// What the grouped-MLP kernels of PointNet++ (pn2_group_kernel, pn2_group_bf3_kernel, iq_pointnet2.hip) and PointConv
// (pc_group_kernel, pc_group_bf3_kernel, iq_pointconv.hip) share: stage 0b (layer 1 on the VALU, with the gather of the per-point
// rows U[p]), the float32 layer 2, and the bf16x3 layers with their weight rings and the layer-2 epilogue.  Only those two files
// include this header: both are compiled with -ffp-contract=off, without -fno-honor-nans and with packed fp32 off (build.py), the
// flags under which these kernels were tuned.
#pragma once
#include "iq_bf3.h"
#include "iq_mfma.h"

constexpr int kGroupThreads = 256;   // workgroup of the four kernels

// ---- stage 0b: layer 1 of a chunk's rows, 3 relative coordinates -> C1 channels, on the VALU ---------------------------------
// A thread owns 4 consecutive channels (c4) of NR rows; the per-point layer-1 rows U[p] arrive as 16-byte raw buffer loads
// (resource on this cloud's U rows, 32-bit per-lane offsets): 4x fewer vector-memory instructions and no 64-bit address
// arithmetic next to the MFMAs.  `rel` rows are (dx, dy, dz, member index as bits).
// add_u: whether row() adds the gathered row.  PointNet++ always does (zeros without U), PointConv only when U is given - the two
// differ on -0.0f, and each family keeps its rule.
template <int C1, int MC>
struct Stage0b {
    static constexpr int Q1 = C1 / 4;                     // channel quads per row
    static constexpr int NR = MC * Q1 / kGroupThreads;    // rows per thread
    f32x4 w1[4];                                          // [channel of the quad] = (wx0, wx1, wx2, bias)
    __amdgpu_buffer_rsrc_t ursrc;
    f32x4 ureg[NR];
    int c4, rsub, ldu;
    bool has_u, add_u;

    __device__ __forceinline__ Stage0b(const float* w1x, const float* U, int ldu_, int cloud, int N, int tid, bool add_u_)
        : ursrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(U ? U + (size_t)cloud * N * ldu_ : w1x), 0, 0x7fffffff, 0x00020000)),
          c4(tid % Q1), rsub(tid / Q1), ldu(ldu_), has_u(U != nullptr), add_u(add_u_) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w1[e] = *reinterpret_cast<const f32x4*>(w1x + (c4 * 4 + e) * 4);
    }
    __device__ __forceinline__ int r(int i) const { return rsub + i * (kGroupThreads / Q1); }   // chunk row of the i-th row
    // request U[p] of this thread's rows; relbuf = the MC rel rows of one buffer
    __device__ __forceinline__ void gather(const float* relbuf) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int p = __float_as_int(relbuf[r(i) * 4 + 3]);
            if (has_u) ureg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ursrc, (p * ldu + c4 * 4) * 4, 0, 0));
            else ureg[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    }
    // layer-1 output of the i-th row (channels 4 c4 .. 4 c4 + 3), v = its rel row
    __device__ __forceinline__ f32x4 row(int i, f32x4 v) const {
        f32x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float t = fmaf(w1[e][2], v[2], fmaf(w1[e][1], v[1], w1[e][0] * v[0])) + w1[e][3];
            if (add_u) t += ureg[i][e];
            h[e] = fmaxf(t, 0.f);
        }
        return h;
    }
};

// ---- float32 layer 2: act1 (MC x C1) -> bias + ReLU -> act2, the n-tiles dealt over the four waves ---------------------------
// Four or more n-tiles: one per wave and pass through the weight ring (primed by the caller before stage 0b), both m-tiles of a
// 64-row chunk on one fragment; fewer: (m-tile, n-tile) pairs round-robin.  mts = m-tiles that hold live rows.
template <int C1, int C2, int MC>
__device__ __forceinline__ void group_layer2_f32(const float* a1base, float* c2base, const WBuf& w2b, WRing& ring2, const float* b2,
                                                 int wave, int wave_s, int fl, int mts) {
    constexpr int LD1 = C1 + 4, LD2 = C2 + 4, KB1 = C1 / 8, NT2 = C2 / 32;
    if (NT2 >= 4) {
#pragma unroll
        for (int q = 0; q < NT2 / 4; ++q) {
            const int nt = q * 4 + wave, nts = q * 4 + wave_s;
            f32x16 acc0 = {0}, acc1 = {0};
            const int wq = nts * KB1 * kFragBytes;
            const int wn = (q + 1 < NT2 / 4 ? nts + 4 : nts) * KB1 * kFragBytes;
            if (MC == 64 && mts == 2) mfma_ntile<LD1, KB1, 2>(a1base, w2b, wq, wn, ring2, acc0, acc1);
            else                      mfma_ntile<LD1, KB1, 1>(a1base, w2b, wq, wn, ring2, acc0, acc1);
            const float bias = b2[nt * 32 + fl];
            float* dst = c2base + nt * 32;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                dst[c_row_i(i) * LD2] = fmaxf(acc0[i] + bias, 0.f);
                if (MC == 64) dst[(32 + c_row_i(i)) * LD2] = fmaxf(acc1[i] + bias, 0.f);
            }
        }
    } else {
        for (int t = wave; t < mts * NT2; t += 4) {
            const int mt = t / NT2, nt = t - mt * NT2;
            f32x16 acc = {0};
            const int wq = uniform(nt) * KB1 * kFragBytes;
#pragma unroll 4
            for (int kb = 0; kb < KB1; ++kb)
                acc = mfma4(lds_frag<LD1>(a1base + mt * 32 * LD1, 0, kb), wbuf_load(w2b, wq + kb * kFragBytes), acc);
            const float bias = b2[nt * 32 + fl];
            float* dst = c2base + mt * 32 * LD2 + nt * 32;
#pragma unroll
            for (int i = 0; i < 16; ++i) dst[c_row_i(i) * LD2] = fmaxf(acc[i] + bias, 0.f);
        }
    }
}

// ---- the 128-128-256 stage on the bf16 matrix pipe: bf16x3, float32-exact (iq_bf3.h) -------------------------
// Layers 2 and 3 as six bf16 products per float32 product.  The bf16 pipe is 2.67x faster per float32 MAC, so operand delivery
// decides the shape: 64-row chunks (a weight fragment - three 1 KiB terms from L2 - feeds two m-tiles; with 32-row chunks the four
// waves would ask the L1 path for 64 B / clk, all it has), layer 3 as 2 x 2 tiles per wave (the A terms of a k-step are read from
// LDS once for both n-tiles).  Activations live in LDS as three bf16 planes of 272-byte rows (conflict-free ds_read_b128), split
// where they are produced; act1 and act2 SHARE one 52 KB image - layer 2 keeps its two tiles in registers until every wave has
// read act1 - so that two workgroups fit a CU and fill each other's barriers and stage-0 phases (four barriers per chunk instead
// of two).  Weights come through small register rings.
// Round 5, three closed experiments on the 0.55 MFMA-busy of these kernels (profiles/r05_grouped_schedule.txt; patches under
// tools/experiments/): (1) s_setprio 1 inside the MFMA loops, or inside the VALU phases: no change (81.3-82.1 k coalitions/s
// either way); (2) "ping-pong": one 512-thread workgroup running two block ranges, the second half one phase behind, every barrier
// shared, so that each SIMD always pairs a VALU phase of one wave with an MFMA loop of the other: bit-identical, 9 % SLOWER
// (80.3 -> 73.3 k; PointConv 84.5 -> 82.3 k), and still 8 % slower with the A terms of the MFMA loops prefetched one k-step ahead
// (83.2 -> 76.6 k) - one wave alone does not keep the matrix pipe fed, the two workgroups' waves overlapping in their MFMA loops
// is what saturates it; (3) the VALU phases (layer 1, the three-term splits) written stage by stage over eight independent values
// instead of value by value (the compiler's schedule is one dependent chain after the other on two or three temporaries):
// bit-identical, no change (81.5 / 81.9 k; PointConv 85.0 / 84.9 k; chain kernel 781.2 / 781.7 k).

// layer 2's weights (n-tile nt = the wave), requested before stage 0b
__device__ __forceinline__ void gb_ring2_prime(B3 (&ring)[4], const __amdgpu_buffer_rsrc_t& rs, int voff, int nt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) ring[i] = b3_load_at(rs, voff, (nt * 8 + i) * 1024, 4 * 8 * 1024);
}
// Layer 2 on TRANSPOSED tiles (weights as the A operand, iq_bf3.h ct_tile_to_planes), so that act2 is stored with whole 8-byte
// stores and without the two-lane DPP trade
template <int MTS>
__device__ __forceinline__ void gb_layer2(const unsigned char* abase, const __amdgpu_buffer_rsrc_t& rs, int voff, int nt,
                                          B3 (&ring)[4], f32x16 (&acc)[MTS][1]) {
    constexpr int ROWB = 272, PLANEB = 64 * ROWB, TS = 4 * 8 * 1024;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        bf16x8 af[MTS][3];
#pragma unroll
        for (int i = 0; i < MTS; ++i) a3_load<PLANEB>(af[i], abase + i * 32 * ROWB, ks);
        const B3 b = ring[ks & 3];
        if (ks + 4 < 8) ring[ks & 3] = b3_load_at(rs, voff, (nt * 8 + ks + 4) * 1024, TS);
        mfma_bf3_block_tr<MTS>(af, b, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// Layer 2's epilogue: bias + ReLU of the wave's MTS tiles (n-tile = wave) into the planes of act2.  Register r = channel
// c_row_i(r) + 4 fh of the n-tile: bq holds the biases of the lane's 16 channels.
template <int MTS>
__device__ __forceinline__ void gb_act2_store(unsigned char* planes, const float* b2, int wave, int lane, const f32x16 (&acc)[2][1]) {
    constexpr int ROWB = 272, PLANEB = 64 * ROWB;
    f32x4 bq[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const f32x4*>(b2 + wave * 32 + 8 * g + 4 * (lane >> 5));
#pragma unroll
    for (int i = 0; i < MTS; ++i)
        ct_tile_to_planes<ROWB, PLANEB>(planes + i * 32 * ROWB + wave * 64, lane,
                                        [&](int r) { return fmaxf(acc[i][0][r] + bq[r >> 2][r & 3], 0.f); });
}
struct B3x2 { B3 b[2]; };
// layer 3's weights (n-tiles nt0 = the wave and nt0 + 4), requested before layer 2's epilogue
__device__ __forceinline__ void gb_ring3_prime(B3x2 (&ring)[2], const __amdgpu_buffer_rsrc_t& rs, int voff, int nt0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        ring[i].b[0] = b3_load_at(rs, voff, (nt0 * 8 + i) * 1024, 8 * 8 * 1024);
        ring[i].b[1] = b3_load_at(rs, voff, ((nt0 + 4) * 8 + i) * 1024, 8 * 8 * 1024);
    }
}
template <int MTS>
__device__ __forceinline__ void gb_layer3(const unsigned char* abase, const __amdgpu_buffer_rsrc_t& rs, int voff, int nt0,
                                          B3x2 (&ring)[2], f32x16 (&acc)[MTS][2]) {
    constexpr int ROWB = 272, PLANEB = 64 * ROWB, TS = 8 * 8 * 1024;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        bf16x8 af[MTS][3];
#pragma unroll
        for (int i = 0; i < MTS; ++i) a3_load<PLANEB>(af[i], abase + i * 32 * ROWB, ks);
        const B3 b[2] = {ring[ks & 1].b[0], ring[ks & 1].b[1]};
        if (ks + 2 < 8) {
            ring[ks & 1].b[0] = b3_load_at(rs, voff, (nt0 * 8 + ks + 2) * 1024, TS);
            ring[ks & 1].b[1] = b3_load_at(rs, voff, ((nt0 + 4) * 8 + ks + 2) * 1024, TS);
        }
        mfma_bf3_block<MTS, 2>(af, b, acc);
        __builtin_amdgcn_sched_barrier(0);
    }
}
