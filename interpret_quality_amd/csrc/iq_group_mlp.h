// The bf16x3 layers of the grouped MLP that PointNet++ sa2 (pn2_group_bf3_kernel, iq_pointnet2.hip) and PointConv sa2
// (pc_group_bf3_kernel, iq_pointconv.hip) share.  Only those two files include this header: both are compiled with
// -ffp-contract=off, without -fno-honor-nans and with packed fp32 off (build.py), the flags under which these kernels were tuned.
#pragma once
#include "iq_bf3.h"
#include "iq_mfma.h"

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
struct B3x2 { B3 b[2]; };
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
