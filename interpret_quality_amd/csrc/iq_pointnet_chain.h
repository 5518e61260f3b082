// The PointNet chain kernel (included by iq_pointnet.hip, which keeps the region tables, row lists, launch order and entry points).
//
// One workgroup (4 waves) per coalition, 64-row chunks (96 in the product instantiations, below):
//   stage0 (VALU)  x -> x.trans -> conv1(3->64)+bn+relu                      -> LDS act0
//   L1  (MFMA)     64->64   (fstn.conv1 | per-coalition trans_feat product)  -> LDS act1
//   L2  (MFMA)     64->128  conv2+bn+relu                                    -> LDS act2
//   L3  (MFMA)     128->1024 conv3+bn(+relu), column max over rows           -> registers
// pn_chain_kernel<mode, L3V, ARGMAX> is a common prologue and ONE of three bodies; the point fetcher (stage 0a), layer 2's bf16x3
// store and the two epilogues are written once and shared:
//   chain_fp32 (L3V = 2: pre-pool, fp32 twins, fp32 arg-max): v_mfma_f32_32x32x2_f32 throughout (exact fp32 fma chains).  A operands
//     come from LDS (row stride padded by 4 floats: conflict-free ds_read_b128), B operands (weights) stream from L2 in a pre-packed
//     fragment order (1 KiB contiguous per wave-load).  LDS = 51 KB (act0/act2 33 KB, act1 17 KB, xs 1 KB) -> 3 workgroups/CU.
//   chain_bf3_64 (L3V = 3: the arg-max trunk, the twins kFstn64 / kTrunk64 of kTwinChainL3Single): layers 1-3 as six exact bf16
//     products per float32 product on v_mfma_f32_16x16x32_bf16 (iq_bf3.h; DESIGN.md 5a: the kernel is power-bound and this shape
//     holds a 10 % higher clock than 32x32x16), activations - act0 included, split by stage 0b - as three swizzled bf16 planes in
//     LDS.  Layer 1 reads its weights out of the SAME fp32 images as the fp32 body (the packed fstn.conv1, the per-coalition
//     transform) and splits them into bf16 terms in registers, four b128 loads per wave and chunk (l1_raw_load, l1_bf3): wave w =
//     the 16 channels of n-tile w for every 16-row m-tile.  No v_mfma_f32_32x32x2_f32 is left (tests/test_isa_chain_l1_cpu.py).
//     LDS = 73 KB (act0/act2 48 KB, act1 24 KB, xs 1 KB), <= 256 VGPRs -> 2 workgroups/CU.
//   chain_bf3_96 (the two product instantiations <kFstn | kTrunk, 3, false>): 96-ROW chunks: a layer-3 weight fragment then feeds
//     six 16-row m-tiles instead of four, a third less weight streaming out of L2 per row.  Two workgroups still fit a CU because
//     act0, act1 and act2 share ONE 72 KB image (act0 bytes 0 - 36 K, act1 36 - 72 K, act2 all of it: layer 2 keeps its 96 x 32
//     outputs per wave in registers until every wave has read act1, one more barrier per chunk): LDS = 73.5 KB (image 72 KB, xs
//     1.5 KB), 252 VGPRs, no scratch.  Every row's arithmetic is chain_bf3_64's, which is this body's bitwise reference.
// Row lists are padded for both chunk sizes (iq_pointnet.hip, padded_rows).
#pragma once
#include <type_traits>

#include "iq_common.h"
#include "iq_twin.h"

#include "iq_bf3.h"
#include "iq_mfma.h"

namespace {

constexpr int kFeat = IQ_NUM_FEAT;
constexpr int kMC = 64;        // rows per chunk (the product instantiations of the chain kernel: kMC96)
constexpr int kMC96 = 96;
constexpr int kMaxN = 4096;    // points per cloud supported by the chain kernel (= IQ_MAX_POINTS; row lists are uint16)
constexpr int kThreads = 256;
constexpr int kRowCap = kMaxN + kMC;  // row-list stride per item (uint16)

// kFstn64 / kTrunk64: the same two bf16x3 chains in 64-row chunks, one n-tile per pass (twin kTwinChainL3Single, the bitwise reference
// of the product instantiations <kFstn | kTrunk, 3, false>, which keep their names and work on 96-row chunks).  The chunk size rides
// in the mode because the kernel keeps its three template arguments <mode, L3V, ARGMAX> (tests/test_isa_cpu.py pins them).
enum ChainMode { kPrepool = 0, kFstn = 1, kTrunk = 2, kFstn64 = 3, kTrunk64 = 4 };

// LDS activation images are row-major [row][k] with the row stride padded by 4 floats (68 / 132):
// a 16-lane ds_read_b128 group reads 16 different rows at one k, i.e. bank offsets 4*row mod 64 ->
// conflict-free, and every address in the MFMA loops is ONE per-lane base plus an immediate.
constexpr int kLd1 = 64 + 4;    // act0 / act1 (64 channels)
constexpr int kLd2 = 128 + 4;   // act2 (128 channels)

struct ChainArgs {
    const float* clouds;       // strides below, in floats
    int ps, cs, cl;            // point, channel, cloud stride
    const float* centers;      // (nclouds,3)
    const uint16_t* rows;        // (items,kRowCap) compacted point list of every item (pn_rows_kernel)
    const int32_t* nrows;        // (items) row count | centre flag << 16
    const int32_t* item_order;   // (items) launch order (largest coalitions first) or null
    const int32_t* cloud_of;   // (items) or null                          [kFstn/kTrunk]
    const float* trans;        // (items,9) input transform                [kFstn/kTrunk]
    const float* w_in;         // [64][4] folded 3->64 layer
    const float* w1;           // kFstn: packed 64x64; kTrunk: per item packed image (items,4096)
    const float* b1;
    const float* w2;
    const float* b2;
    const float* w3;
    const float* b3;
    const unsigned short* w3_bf3;   // layer 3's weights as three bf16 terms (iq_pack_weight_bf3) or null: L3 on the bf16 matrix pipe (L3V = 3)
    const unsigned short* w2_bf3;   // layer 2's, likewise (L3V = 3 needs both)
    float* out;                // (items,1024)
    int32_t* argrow;           // (items,1024) point index of the row that attains each column maximum, or null [ARGMAX trunk only]
    const int32_t* arg_row;    // (items) the row of argrow that an item writes, or null: its own                [ARGMAX trunk only]
    const int32_t* n_dev;      // the live item count where only the device knows it (the distinct coalitions of a batch,
                               // pn_compact kernels), or null: `items`.  A workgroup past it leaves at once       [kFstn/kTrunk]
    int N, R, items, nclouds, with_centre;
    int tail16;                  // last m-tile of an item on 16x16x4 MFMAs when it holds at most 16 rows (l3_tail16)
    int l3_single;               // twin kTwinChainL3Single: the 64-row bf16x3 kernel, one n-tile per pass (launch_chain; the 96-row kernel's reference)
};

// ---- L3: 128 -> 1024 for one 64-row chunk; wave `wave` owns the n-tiles q*4 + wave ------------
// Variant 2: an 8-deep register ring of B fragments (32 VGPRs) that runs 8 K-blocks (4 096 MFMA
// cycles) ahead and never drains: it rolls over n-tile boundaries and, through `ring`, over chunk
// boundaries (the last n-tile of a chunk prefetches the first K-blocks of n-tile 0).  A fragments are
// double-buffered one K-block ahead.  sched_group_barrier pins the issue order inside each K-block:
// LDS reads of the next block, the MFMAs of this one, one ring refill.
struct BRing {
    f32x4 r[8];
};

__device__ __forceinline__ void bring_init(BRing& ring, const WBuf& w3, int wave_s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ring.r[i] = wbuf_load(w3, (wave_s * 16 + i) * kFragBytes);
}

// wave_s: the wave index as a scalar; the fragment offsets are then scalar too (iq_mfma.h: WBuf)
// ARGMAX (dense forward with crt_points only): besides the column maximum, the position in the item's row list of the row
// that attains it (largest value, then lowest row).  `rowbase` = first row of this chunk, fh = lane >> 5.
template <int MTS, bool ARGMAX = false>
__device__ __forceinline__ void l3_pass_v2(const WBuf& w3, const float* abase, int wave_s, float (&runmax)[8], BRing& ring,
                                           int (&runarg)[8], int rowbase = 0, int fh = 0) {
    const int w0 = wave_s * 16 * kFragBytes;
    int wq = w0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const int wn = (q < 7) ? wq + 4 * 16 * kFragBytes : w0;
        f32x16 acc0 = {0}, acc1 = {0};
        f32x4 a0n = lds_frag<kLd2>(abase, 0, 0), a1n = a0n;
        if (MTS == 2) a1n = lds_frag<kLd2>(abase, 1, 0);
#pragma unroll
        for (int kb = 0; kb < 16; ++kb) {
            const f32x4 a0 = a0n, a1 = a1n;
            if (kb + 1 < 16) {
                a0n = lds_frag<kLd2>(abase, 0, kb + 1);
                if (MTS == 2) a1n = lds_frag<kLd2>(abase, 1, kb + 1);
            }
            const f32x4 bk = ring.r[kb & 7];
            acc0 = mfma4(a0, bk, acc0);
            if (MTS == 2) acc1 = mfma4(a1, bk, acc1);
            ring.r[kb & 7] = wbuf_load(w3, kb < 8 ? wq + (kb + 8) * kFragBytes : wn + (kb - 8) * kFragBytes);
            if (kb + 1 < 16) __builtin_amdgcn_sched_group_barrier(0x100, MTS, 0);  // DS reads of K-block kb+1
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * MTS, 0);               // MFMAs of K-block kb
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                     // ring refill
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ARGMAX) {
            float m = -INFINITY;
            int r = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {          // rows ascend with i inside a tile: strict > keeps the lowest row
                if (acc0[i] > m) { m = acc0[i]; r = rowbase + c_row_i(i) + 4 * fh; }
            }
            if (MTS == 2) {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (acc1[i] > m) { m = acc1[i]; r = rowbase + 32 + c_row_i(i) + 4 * fh; }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {           // chunks come in row order: strict > again
                const bool better = (i == q) && m > runmax[i];
                runarg[i] = better ? r : runarg[i];
                runmax[i] = better ? m : runmax[i];
            }
        } else {
            float m = max16(acc0);
            if (MTS == 2) m = fmaxf(m, max16(acc1));
#pragma unroll
            for (int i = 0; i < 8; ++i) runmax[i] = (i == q) ? fmaxf(runmax[i], m) : runmax[i];
        }
        wq = wn;
    }
}

// ---- Variant 3: L3 on the bf16 matrix pipe, float32-exact -----------------------------------------------------------------------
// (csrc/iq_linear.hip, pn_gemm_bf3_kernel<pool>, has the arithmetic: a float32 is three bf16 terms, a product the six largest of the
// nine term products, each exact, accumulated in float32; 32 k cost 6 x 16 matrix cycles per 16 x 16 tile.)  The instruction is
// v_mfma_f32_16x16x32_bf16 (iq_bf3.h, 16x16x32 forms; DESIGN.md 5a: the kernel is power-bound and this shape draws less power per
// FLOP than 32x32x16, so the board holds a higher clock).  act2 lives in LDS as three bf16 planes [64][128] of unpadded, XOR-swizzled
// 256-byte rows (conflict-free ds_read_b128 for this shape), written split by layer 2's epilogue; the weights come split and packed
// from the host (iq_pack_weight_bf3: fragment (term, n-tile, k-step of 16) at ((term 32 + n-tile) 8 + k-step) KB - the 16x16x32
// fragments are read out of the same image), through a register ring that rolls over pass and chunk boundaries like BRing.  A row's
// result does not depend on the tile, lane group or chunk it sits in, so the pooled maxima are those of the same rows in any
// arrangement (fused = materialised, bitwise, as before).  16-row tail tiles are not used here (m-tiles go in pairs of 16 rows).
constexpr int kLdB = 256;                 // bytes per act2 row of one bf16 plane (128 k, unpadded, swizzled)
constexpr int kPlaneB = kMC * kLdB;       // bytes per plane
struct B3Ring { B3 r[4]; };
constexpr int kLd1B = 128;                // bytes per act1 row of one bf16 plane (64 k, unpadded, swizzled)
constexpr int kPlane1B = kMC * kLd1B;

// layer 2's 16x16x32 weight fragment (the A operand of the transposed tile): 32-channel n-tile nt of 4, its half hf, k-step t of 2
// (32 input channels), out of iq_pack_weight_bf3 of a (128,64) matrix; voff = b16_lane_off(lane)
__device__ __forceinline__ B3 b3_load16_l2(const __amdgpu_buffer_rsrc_t& rs, int voff, int nt, int t, int hf) {
    return b3_load_at(rs, voff, (nt * 4 + 2 * t) * 1024 + 256 * hf, 16 * 1024);
}

// layer 3's 16x16x32 weight fragment: 32-column n-tile (q mod 8) 4 + wave, its column half hf, k-step t of 4 (32 channels);
// voff = b16_lane_off(lane)
__device__ __forceinline__ B3 b3_load16(const __amdgpu_buffer_rsrc_t& rs, int voff, int q, int t, int hf, int wave_s) {
    return b3_load_at(rs, voff, (((q & 7) * 4 + wave_s) * 8 + 2 * t) * 1024 + 256 * hf, 32 * 8 * 1024);
}

// running column maxima of a lane: runmax[2 q + hf] = column ((q 4 + wave) 32 + 16 hf + (lane & 15)) over the rows 4 kq + i of every
// 16-row m-tile seen so far; the four kq lanes of a column meet in the kernel's epilogue.  ARGMAX: with the position in the item's
// row list of the row that attains it (largest value, then lowest row: rows ascend with i, m-tile and chunk, so strict > everywhere).
template <int MT, bool ARGMAX>
__device__ __forceinline__ void l3_pool16(const f32x4 (&acc)[MT], bool take, float& runmax, int& runarg, int row0) {
    if (ARGMAX) {
        float m = -INFINITY;
        int r = 0;
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (acc[mi][i] > m) { m = acc[mi][i]; r = row0 + 16 * mi + i; }
        const bool better = take && m > runmax;
        runarg = better ? r : runarg;
        runmax = better ? m : runmax;
    } else {
        float m = fmaxf(fmaxf(acc[0][0], acc[0][1]), acc[0][2]);
        m = fmaxf(fmaxf(m, acc[0][3]), acc[1][0]);
        m = fmaxf(fmaxf(m, acc[1][1]), acc[1][2]);
        m = fmaxf(m, acc[1][3]);
#pragma unroll
        for (int p = 2; p < MT; p += 2) {      // a further pair of m-tiles
            float n = fmaxf(fmaxf(acc[p][0], acc[p][1]), acc[p][2]);
            n = fmaxf(fmaxf(n, acc[p][3]), acc[p + 1][0]);
            n = fmaxf(fmaxf(n, acc[p + 1][1]), acc[p + 1][2]);
            m = fmaxf(fmaxf(m, n), acc[p + 1][3]);
        }
        runmax = take ? fmaxf(runmax, m) : runmax;
    }
}

// One n-tile of 32 columns (two 16-column halves) per pass: the ARGMAX instantiation and twin kTwinChainL3Single.
// ring.r[2 (t & 1) + hf] = fragment (k-step parity, half), two k-steps ahead, rolling over n-tile and chunk boundaries.
// abase: plane 0 of act2; aoff = a16_lane_off(lane); row0 = first row of this chunk + 4 kq.
template <int MTS, bool ARGMAX = false>
__device__ __forceinline__ void l3_pass_bf3(const __amdgpu_buffer_rsrc_t& rs, int voff, const unsigned char* abase, int aoff, int wave_s,
                                            float (&runmax)[16], B3Ring& ring, int (&runarg)[16], int row0 = 0) {
    constexpr int MT = 2 * MTS;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        f32x4 acc[2][MT];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            bf16x8 af[MT][3];
#pragma unroll
            for (int i = 0; i < MT; ++i) a16_load<kLdB, kPlaneB>(af[i], abase, aoff, i, t);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const B3 b = ring.r[2 * (t & 1) + j];
                mfma16_bf3_col<MT>(af, b, acc[j]);
                // k-step t + 2 of this n-tile, or k-step t - 2 of the next one (b3_load16 takes the n-tile index mod 8)
                ring.r[2 * (t & 1) + j] = b3_load16(rs, voff, t + 2 < 4 ? q : q + 1, (t + 2) & 3, j, wave_s);
            }
            // issue order inside a k-step: the A reads, then per column tile its MFMAs and its ring refill (left alone the
            // scheduler sinks every refill to the end of the k-step); one k-step at a time (it otherwise hoists every step's
            // operand reads to the top of the n-tile)
            __builtin_amdgcn_sched_group_barrier(0x100, 3 * MT, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                __builtin_amdgcn_sched_group_barrier(0x008, 6 * MT, 0);
                __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) l3_pool16<MT, ARGMAX>(acc[j], i == q, runmax[2 * i + j], runarg[2 * i + j], row0);
    }
}

// The same layer with TWO n-tiles per pass (n-tiles (2 qp) 4 + wave and (2 qp + 1) 4 + wave: 4 column tiles of 16) over the 96-row
// chunks of the product instantiations: MT = 2, 4 or 6 m-tiles of 16 rows, a 96 x 64 wave tile, 96 accumulator registers.  Every
// tile sees the same products in the same order, so the maxima are bit-identical to l3_pass_bf3's.  A weight fragment feeds up to
// six m-tiles (a third less weight streaming per row than with 64-row chunks).  Six m-tiles go as two halves of three, one after
// the other: the A terms of a half (36 registers; all six would be 72 and do not fit beside 96 + 48) are read from LDS once for
// all four column tiles, then the half's 72 MFMAs go column-tile-major.  ring.r[jj] = fragment of column tile jj (n-tile jj >> 1,
// half jj & 1) of the CURRENT k-step, refilled with the next k-step's as soon as the LAST half's MFMAs of that column tile are
// issued: a refilled slot is next read 3 x 6 x (MT / NH) MFMAs later (the other three column tiles, one half each; 54 MFMAs = 864 matrix
// cycles at MT = 6, 1 152 at MT = 4 as with 64-row chunks, 576 at MT = 2) and the ring rolls over pass and chunk boundaries.
template <int MTS, int PLANEB>
__device__ __forceinline__ void l3_pass_bf3_2x2(const __amdgpu_buffer_rsrc_t& rs, int voff, const unsigned char* abase, int aoff,
                                                int wave_s, float (&runmax)[16], B3Ring& ring) {
    constexpr int MT = 2 * MTS, NH = MTS == 3 ? 2 : 1, HT = MT / NH;
    int noarg = 0;
#pragma unroll 1
    for (int qp = 0; qp < 4; ++qp) {
        f32x4 acc[4][MT];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                bf16x8 af[HT][3];
#pragma unroll
                for (int i = 0; i < HT; ++i) a16_load<kLdB, PLANEB>(af[i], abase, aoff, h * HT + i, t);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const B3 b = ring.r[j];
                    mfma16_bf3_col<HT>(af, b, reinterpret_cast<f32x4(&)[HT]>(acc[j][h * HT]));
                    // k-step t + 1 of this pair of n-tiles, or k-step 0 of the next pair
                    if (h == NH - 1)
                        ring.r[j] = b3_load16(rs, voff, (t + 1 < 4 ? 2 * qp : 2 * qp + 2) + (j >> 1), (t + 1) & 3, j & 1, wave_s);
                }
                // issue order (as l3_pass_bf3): the half's A reads, then per column tile its MFMAs and - last half - its refill
                __builtin_amdgcn_sched_group_barrier(0x100, 3 * HT, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 6 * HT, 0);
                    if (h == NH - 1) __builtin_amdgcn_sched_group_barrier(0x020, 3, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) l3_pool16<MT, false>(acc[j], i == qp, runmax[4 * i + j], noarg, 0);
    }
}

// L3 for a LAST m-tile of at most 16 rows (rows row0 .. row0 + 15 of act2): v_mfma_f32_16x16x4_f32 instead of a 32-row tile
// of which half would be padding (a coalition's row count is uniform mod 32, so this saves a quarter tile per coalition and
// chain on average: 1.5 % of the kernel).  BIT-IDENTICAL to the 32x32x2 path: that instruction accumulates its two k values
// (8 kb + j for half h = 0, 8 kb + 4 + j for h = 1) and the 16x16x4 instruction its four as ONE sequential fma chain in operand
// order, so feeding the four lane groups kq = 0..3 with k = (j, 4 + j, j + 1, 5 + j), j = 0 then 2, repeats the chain of the
// steps (j, j + 1) of a k-block exactly (tools/micro/mfma_tail.hip: 0 of 102 400 outputs differ; the plain k order differs in
// 77 %).  Both operands come out of the SAME images: lane (r16 = lane & 15, kq) reads the float4 of act2 row row0 + r16 at
// k = 8 kb + 4 (kq & 1) and the float4 of weight-fragment lane (16 half + r16) + 32 (kq & 1), and takes elements (kq >> 1) and
// (kq >> 1) + 2.  C layout of 16x16x4: element i of lane l = row 4 (l >> 4) + i, column l & 15.
__device__ __forceinline__ void l3_tail16(const WBuf& w3, const float* act2, int row0, int wave_s, int lane, float (&runmax)[8],
                                          BRing& ring) {
    const int r16 = lane & 15, kq = lane >> 4, hsel = kq & 1;
    const bool odd = (kq >> 1) != 0;
    float a0[16], a1[16];
    const float* arow = act2 + (row0 + r16) * kLd2 + 4 * hsel;
#pragma unroll
    for (int kb = 0; kb < 16; ++kb) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(arow + 8 * kb);
        a0[kb] = odd ? v[1] : v[0];
        a1[kb] = odd ? v[3] : v[2];
    }
    const int voff0 = (r16 + 32 * hsel) * 16, voff1 = (16 + r16 + 32 * hsel) * 16;   // bytes inside a fragment, column halves 0 / 1
    // the B ring of the 32-row passes (dead by now: this is the item's last tile) holds the weight float4s of 4 k-blocks x 2
    // column halves, 4 k-blocks (16 MFMAs = 512 cycles) ahead, rolling over the n-tile boundaries
    const int w0 = wave_s * 16 * kFragBytes;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        ring.r[2 * d] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w3.rsrc, voff0, w0 + d * kFragBytes, 0));
        ring.r[2 * d + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w3.rsrc, voff1, w0 + d * kFragBytes, 0));
    }
    int wq = w0;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        const int wn = (q < 7) ? wq + 4 * 16 * kFragBytes : w0;
        f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
        for (int kb = 0; kb < 16; ++kb) {
            const f32x4 b0 = ring.r[2 * (kb & 3)], b1 = ring.r[2 * (kb & 3) + 1];
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[kb], odd ? b0[1] : b0[0], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[kb], odd ? b1[1] : b1[0], c1, 0, 0, 0);
            c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[kb], odd ? b0[3] : b0[2], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[kb], odd ? b1[3] : b1[2], c1, 0, 0, 0);
            const int soff = kb < 12 ? wq + (kb + 4) * kFragBytes : wn + (kb - 12) * kFragBytes;
            ring.r[2 * (kb & 3)] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w3.rsrc, voff0, soff, 0));
            ring.r[2 * (kb & 3) + 1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w3.rsrc, voff1, soff, 0));
        }
        float m0 = fmaxf(fmaxf(c0[0], c0[1]), fmaxf(c0[2], c0[3])), m1 = fmaxf(fmaxf(c1[0], c1[1]), fmaxf(c1[2], c1[3]));
        m0 = fmaxf(m0, __shfl_xor(m0, 16)); m1 = fmaxf(m1, __shfl_xor(m1, 16));
        m0 = fmaxf(m0, __shfl_xor(m0, 32)); m1 = fmaxf(m1, __shfl_xor(m1, 32));
        const float m = (lane & 16) ? m1 : m0;            // lane l keeps column l & 31 of the n-tile, as the 32x32 path does
#pragma unroll
        for (int i = 0; i < 8; ++i) runmax[i] = (i == q) ? fmaxf(runmax[i], m) : runmax[i];
        wq = wn;
    }
}

// relu(v + b) of a lane's four channels: layer 1 of the feature STN and layer 2 of the bf16x3 bodies
__device__ __forceinline__ f32x4 bias_relu4(f32x4 v, f32x4 b) {
    return (f32x4){fmaxf(v[0] + b[0], 0.f), fmaxf(v[1] + b[1], 0.f), fmaxf(v[2] + b[2], 0.f), fmaxf(v[3] + b[3], 0.f)};
}

// ---- stage 0b and layer 1 of the bf16x3 kernels (L3V = 3): act0 as three bf16 planes, layer 1 on v_mfma_f32_16x16x32_bf16 --------
// act0 has act1's format: three planes of unpadded, XOR-swizzled 128-byte rows (iq_bf3.h), read with a16_load<kLd1B, ...>.
// stage 0b, 3 -> 64 (+bn, relu): thread t = (channel quad t & 15, rows (t >> 4) + 16 i), so a lane splits four consecutive channels
// of a row into one 8-byte store per plane and a wave's store covers four whole rows (512 contiguous bytes: conflict-free).
// wi[j] = the folded 3 -> 64 layer's row of channel 4 (t & 15) + j.
template <int ROWS, int PLANEB>
__device__ __forceinline__ void stage0b_planes(unsigned char* act0, const float* xs, const f32x4 (&wi)[4], int t) {
    const int cq = t & 15;
#pragma unroll
    for (int i = 0; i < ROWS / 16; ++i) {
        const int row = (t >> 4) + 16 * i;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + row * 4);
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(wi[j][2], xv[2], fmaf(wi[j][1], xv[1], wi[j][0] * xv[0])) + wi[j][3], 0.f);
        row4_to_planes<PLANEB>(act0 + row * kLd1B + 16 * ((cq >> 1) ^ swz_of_row<kLd1B>(row)) + 8 * (cq & 1), v);
    }
}

// Layer 1's weights come out of the fp32 image that the fp32 kernels read (32x32x2 fragment order, iq_mfma.h: fragment (n-tile,
// k-block kb of 8) = 1 KiB, lane (n & 31) + 32 h holds k = 8 kb + 4 h + 0..3 of column n).  Wave w owns the 16 output channels
// n = 16 w + c; the 16x16x32 operand of lane (c, kq) at k-step t is k = 32 t + 8 kq + 0..7 = the two float4s of lanes (n & 31) and
// 32 + (n & 31) of fragment (w >> 1, 4 t + kq): four b128 loads per chunk, split into bf16 terms in registers after the barrier.
struct L1Raw { f32x4 r[2][2]; };   // [k-step][half of the eight k values]
__device__ __forceinline__ L1Raw l1_raw_load(const __amdgpu_buffer_rsrc_t& rs, int ln, int wave_s) {
    const int voff = ((ln >> 4) * 64 + 16 * (wave_s & 1) + (ln & 15)) * 16;
    L1Raw w;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h)
            w.r[t][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 512 * h, ((wave_s >> 1) * 8 + 4 * t) * kFragBytes, 0));
    return w;
}
// 64 -> 64 over MT 16-row m-tiles, transposed tiles as layer 2 has them (the weight fragment is the A operand: lane (row l & 15 of
// the m-tile, kq) holds channels 16 w + 4 kq + 0..3), two k-steps of 32 channels, the six products of mfma16_bf3_col_tr per k-step.
// The m-tiles go G at a time; a tile's accumulation chain is the same whatever G, m-tile or chunk, so a row's result does not depend
// on where it sits.  bq: b1 of the lane's four channels (RELU: the feature STN; the trunk's product has neither bias nor relu).
template <int MT, int PLANEB, bool RELU>
__device__ __forceinline__ void l1_bf3(const unsigned char* act0, unsigned char* act1, const L1Raw& raw, f32x4 bq, int ln, int wave_s) {
    constexpr int G = MT % 3 == 0 ? 3 : 2;
    static_assert(MT % G == 0, "m-tiles go G at a time");
    const int a0off = a16_lane_off<kLd1B>(ln), l15 = ln & 15;
    const B3 w[2] = {b3_split8(raw.r[0][0], raw.r[0][1]), b3_split8(raw.r[1][0], raw.r[1][1])};
#pragma unroll
    for (int p = 0; p < MT; p += G) {
        f32x4 acc[G];
#pragma unroll
        for (int i = 0; i < G; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            bf16x8 af[G][3];
#pragma unroll
            for (int i = 0; i < G; ++i) a16_load<kLd1B, PLANEB>(af[i], act0, a0off, p + i, t);
            mfma16_bf3_col_tr<G>(w[t], af, acc);
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
            f32x4 v = acc[i];
            if (RELU) v = bias_relu4(v, bq);
            c16_tile_to_planes_swz<kLd1B, PLANEB>(act1, 16 * (p + i) + l15, 2 * wave_s, ln, v);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- what the three bodies share: buffer resources, the point fetcher (stage 0a), layer 2's store, the two epilogues ---------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t chain_rsrc(const void* base) {   // raw buffer over a wave-uniform base (iq_mfma.h: wbuf_make)
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

// Input points travel ahead in registers: lanes 0..15 (23) of each wave own 16 (24) rows of a chunk of MC.  The
// row index of chunk c+2 and the coordinates of chunk c+1 are requested while chunk c computes, so
// neither of the two dependent global loads is ever waited for.
template <int MODE, int MC>
struct PointFetcher {
    const ChainArgs& a;
    const int item, cloud, nchunks, frow;
    const bool fetcher;
    const uint16_t* rowp;
    float px = 0.f, py = 0.f, pz = 0.f;
    int pnext = 0;

    __device__ __forceinline__ PointFetcher(const ChainArgs& a_, int item_, int cloud_, int nchunks_, int lane, int wave)
        : a(a_), item(item_), cloud(cloud_), nchunks(nchunks_), frow(wave * (MC / 4) + lane), fetcher(lane < MC / 4),
          rowp(a_.rows + (size_t)item_ * kRowCap + frow) {
        if (fetcher) {
            load_point(rowp[0]);
            if (nchunks > 1) pnext = rowp[MC];
        }
    }
    __device__ __forceinline__ void load_point(int p) {
        if (p == a.N) {
            px = a.centers[cloud * 3]; py = a.centers[cloud * 3 + 1]; pz = a.centers[cloud * 3 + 2];
        } else {
            const float* src = a.clouds + (size_t)cloud * a.cl + (size_t)p * a.ps;
            px = src[0]; py = src[a.cs]; pz = src[2 * a.cs];
        }
    }
    // stage 0a: input transform (models/pointnet.py:67-69) of the chunk's rows -> xs (x,y,z,-); a barrier follows
    __device__ __forceinline__ void stage0a(float* xs) const {
        if (fetcher) {
            float x = px, y = py, z = pz;
            if (MODE != kPrepool) {
                const float* t9 = a.trans + (size_t)item * 9;  // uniform -> scalar loads
                const float x2 = fmaf(z, t9[6], fmaf(y, t9[3], x * t9[0]));
                const float y2 = fmaf(z, t9[7], fmaf(y, t9[4], x * t9[1]));
                const float z2 = fmaf(z, t9[8], fmaf(y, t9[5], x * t9[2]));
                x = x2; y = y2; z = z2;
            }
            *reinterpret_cast<f32x4*>(xs + frow * 4) = (f32x4){x, y, z, 0.f};
        }
    }
    // after that barrier: chunk ch's point is consumed, request the next one and the row index after it
    __device__ __forceinline__ void advance(int ch) {
        if (fetcher && ch + 1 < nchunks) {
            load_point(pnext);
            if (ch + 2 < nchunks) pnext = rowp[(ch + 2) * MC];
        }
    }
};

// layer 2's epilogue of the bf16x3 bodies for the two 16-row tiles of a 32-row m-tile: bias (bq: b2 of the lane's four channels,
// 16-channel tile starting at channel c), relu, split into act2's three planes.  row: the lane's row in the first tile.
template <int PLANEB>
__device__ __forceinline__ void l2_store_bf3(unsigned char* act2, const f32x4 (&acc)[2], f32x4 bq, int row, int c, int ln) {
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) c16_tile_to_planes_swz<kLdB, PLANEB>(act2, row + 16 * pi, c / 8, ln, bias_relu4(acc[pi], bq));
}

// The epilogues: max commutes with the (monotone) per-column bias add and relu.  runarg: read with ARGMAX only.
// fp32 layer 3: runmax[q] = n-tile q * 4 + wave, column lane & 31; the two half-waves of a column meet here.
template <int MODE, bool ARGMAX>
__device__ __forceinline__ void chain_epilogue_fp32(const ChainArgs& a, int item, int wave, int lane, const float (&runmax)[8],
                                                    const int (&runarg)[8]) {
    float* outp = a.out + (size_t)item * kFeat;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        float v = runmax[q];
        const int n = (q * 4 + wave) * 32 + (lane & 31);
        if constexpr (ARGMAX) {   // the other half-wave saw rows 4..7 (+8 k) of every tile: larger value wins, then the lower row
            const float v2 = __shfl_xor(v, 32);
            const int r2 = __shfl_xor(runarg[q], 32);
            const int r = (v2 > v || (v2 == v && r2 < runarg[q])) ? r2 : runarg[q];
            if (lane < 32 && a.argrow) a.argrow[(size_t)(a.arg_row ? a.arg_row[item] : item) * kFeat + n] = (int)a.rows[(size_t)item * kRowCap + r];   // row -> point
        }
        v = fmaxf(v, __shfl_xor(v, 32));
        v += a.b3[n];
        if (MODE != kTrunk) v = fmaxf(v, 0.f);
        if (lane < 32) outp[n] = v;
    }
}

// bf16x3 layer 3: runmax[2 q + half] (l3_pool16); the four kq lanes of a column hold rows 4 kq + i of every m-tile: larger value
// wins, then the lower row
template <int MODE, bool ARGMAX>
__device__ __forceinline__ void chain_epilogue_bf3(const ChainArgs& a, int item, int wave, int lane, const float (&runmax)[16],
                                                   const int* runarg) {
    float* outp = a.out + (size_t)item * kFeat;
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        float v = runmax[x];
        const int n = ((x >> 1) * 4 + wave) * 32 + 16 * (x & 1) + (lane & 15);
        if constexpr (ARGMAX) {
            int r = runarg[x];
#pragma unroll
            for (int d = 16; d <= 32; d *= 2) {
                const float v2 = __shfl_xor(v, d);
                const int r2 = __shfl_xor(r, d);
                const bool other = v2 > v || (v2 == v && r2 < r);
                r = other ? r2 : r;
                v = other ? v2 : v;
            }
            if (lane < 16 && a.argrow) a.argrow[(size_t)(a.arg_row ? a.arg_row[item] : item) * kFeat + n] = (int)a.rows[(size_t)item * kRowCap + r];   // row -> point
        } else {
            v = fmaxf(v, __shfl_xor(v, 16));
            v = fmaxf(v, __shfl_xor(v, 32));
        }
        v += a.b3[n];
        if (MODE != kTrunk) v = fmaxf(v, 0.f);
        if (lane < 16) outp[n] = v;
    }
}

// ---- body 1 of 3: fp32 (L3V = 2: pre-pool, the fp32 twins, fp32 arg-max), 64-row chunks, v_mfma_f32_32x32x2_f32 throughout --------
template <int MODE, bool ARGMAX>
__device__ __forceinline__ void chain_fp32(const ChainArgs& a, int item, int cloud, int nrows) {
    __shared__ __attribute__((aligned(16))) float bufA[kMC * kLd2];   // act0 (ld 68), then act2 (ld 132)
    __shared__ __attribute__((aligned(16))) float bufB[kMC * kLd1];   // act1
    __shared__ __attribute__((aligned(16))) float xs[kMC * 4];        // transformed inputs of the chunk (x,y,z,-)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunks = (nrows + kMC - 1) / kMC;

    // stage 0b's channel and row group
    const int c0 = tid & 63, rg = tid >> 6;
    const f32x4 win = *reinterpret_cast<const f32x4*>(a.w_in + c0 * 4);
    const int wave_s = uniform(wave);
    // weight images as buffer resources (kTrunk: layer 1 is this item's packed 64x64 transform)
    const WBuf w1b = wbuf_make((MODE == kTrunk) ? a.w1 + (size_t)item * 4096 : a.w1, lane);
    const WBuf w2b = wbuf_make(a.w2, lane), w3b = wbuf_make(a.w3, lane);
    // per-lane bases: A-fragment reads and C-tile writes are base + immediate everywhere below
    const int frag_lane = (lane & 31), frag_h = lane >> 5;
    const float* a1base_A = bufA + frag_lane * kLd1 + 4 * frag_h;   // act0 in bufA
    const float* a1base_B = bufB + frag_lane * kLd1 + 4 * frag_h;   // act1 in bufB
    const float* a2base = bufA + frag_lane * kLd2 + 4 * frag_h;     // act2 in bufA
    float* c1base = bufB + (4 * frag_h) * kLd1 + frag_lane;         // C tiles of L1 -> act1
    float* c2base = bufA + (4 * frag_h) * kLd2 + frag_lane;         // C tiles of L2 -> act2

    float runmax[8];   // running column maxima: [q] = n-tile q * 4 + wave, column lane & 31
    int runarg[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { runmax[q] = -INFINITY; runarg[q] = 0; }
    PointFetcher<MODE, kMC> pf(a, item, cloud, nchunks, lane, wave);
    BRing ring;
    bring_init(ring, w3b, wave_s);

    for (int ch = 0; ch < nchunks; ++ch) {
        const int rows_here = min(kMC, nrows - ch * kMC);
        const int mts = rows_here > 32 ? 2 : 1;
        pf.stage0a(xs);
        __syncthreads();  // also orders the previous chunk's L3 reads of bufA before stage 0b rewrites it
        pf.advance(ch);
        // ---- stage 0b: 3 -> 64 (+bn, relu), thread = (channel c0, 16 rows) ------------------
        {
            float* dst = ((MODE == kPrepool) ? bufB : bufA) + rg * 16 * kLd1 + c0;
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + (rg * 16 + i) * 4);
                const float f = fmaf(win[2], xv[2], fmaf(win[1], xv[1], win[0] * xv[0])) + win[3];
                dst[i * kLd1] = fmaxf(f, 0.f);
            }
        }
        // ---- L1: 64 -> 64 (the pre-pool has none) -------------------------------------------
        if (MODE != kPrepool) {
            const int mt = wave & 1, nt = wave >> 1;
            const int wq = (wave_s >> 1) * 8 * kFragBytes;
            f32x4 bw[8];  // weight fragments are requested before the barrier, consumed after it
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) bw[kb] = wbuf_load(w1b, wq + kb * kFragBytes);
            __syncthreads();
            if (mt < mts) {
                f32x16 acc = {0};
#pragma unroll
                for (int kb = 0; kb < 8; ++kb) {
                    acc = mfma4(lds_frag<kLd1>(a1base_A + mt * 32 * kLd1, 0, kb), bw[kb], acc);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const float bias = (MODE == kFstn) ? a.b1[nt * 32 + frag_lane] : 0.f;
                float* dst = c1base + mt * 32 * kLd1 + nt * 32;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float v = acc[i] + bias;
                    if (MODE == kFstn) v = fmaxf(v, 0.f);
                    dst[c_row_i(i) * kLd1] = v;
                }
            }
        }
        // ---- L2: 64 -> 128 (+bn, relu): two passes (n-tiles nt0, nt0+2); the second pass's weights
        //      are requested while the first pass computes ------------------------------------
        {
            const int mt = wave & 1, nt0 = wave >> 1;
            const int wq0 = (wave_s >> 1) * 8 * kFragBytes;
            f32x4 bw[8];
#pragma unroll
            for (int kb = 0; kb < 8; ++kb) bw[kb] = wbuf_load(w2b, wq0 + kb * kFragBytes);
            __syncthreads();
            if (mt < mts) {
                const float* arow = a1base_B + mt * 32 * kLd1;
                float* dst = c2base + mt * 32 * kLd2 + nt0 * 32;
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    f32x16 acc = {0};
#pragma unroll
                    for (int kb = 0; kb < 8; ++kb) {
                        acc = mfma4(lds_frag<kLd1>(arow, 0, kb), bw[kb], acc);
                        if (pass == 0) bw[kb] = wbuf_load(w2b, wq0 + (2 * 8 + kb) * kFragBytes);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    const float bias = a.b2[nt0 * 32 + pass * 64 + frag_lane];
#pragma unroll
                    for (int i = 0; i < 16; ++i) dst[c_row_i(i) * kLd2 + pass * 64] = fmaxf(acc[i] + bias, 0.f);
                }
            }
        }
        __syncthreads();
        // ---- L3: 128 -> 1024, running column max -------------------------------------------
        const bool tail = !ARGMAX && a.tail16 && rows_here - 32 * (mts - 1) <= 16;   // (uniform) the last m-tile holds <= 16 rows
        if (mts == 2 && !tail) l3_pass_v2<2, ARGMAX>(w3b, a2base, wave_s, runmax, ring, runarg, ch * kMC, frag_h);
        else if (mts == 2 || !tail) l3_pass_v2<1, ARGMAX>(w3b, a2base, wave_s, runmax, ring, runarg, ch * kMC, frag_h);
        if (tail) l3_tail16(w3b, bufA, 32 * (mts - 1), wave_s, lane, runmax, ring);
    }
    chain_epilogue_fp32<MODE, ARGMAX>(a, item, wave, lane, runmax, runarg);
}

// ---- body 2 of 3: bf16x3 (L3V = 3), 64-row chunks: the arg-max trunk and the twins kFstn64 / kTrunk64, one n-tile per layer-3 pass --
template <int MODE, bool ARGMAX>
__device__ __forceinline__ void chain_bf3_64(const ChainArgs& a, int item, int cloud, int nrows) {
    // act0 as three bf16 planes of 128-byte rows (24 KB), then act2 as three bf16 planes of 256-byte rows; act1 as act0
    __shared__ __attribute__((aligned(16))) unsigned char img[3 * kPlaneB];
    __shared__ __attribute__((aligned(16))) unsigned char act1[3 * kPlane1B];
    __shared__ __attribute__((aligned(16))) float xs[kMC * 4];        // transformed inputs of the chunk (x,y,z,-)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunks = (nrows + kMC - 1) / kMC;
    const int wave_s = uniform(wave);
    // weight images as buffer resources (kTrunk: layer 1 is this item's packed 64x64 transform, the fp32 kernels' image)
    const __amdgpu_buffer_rsrc_t w1rs = chain_rsrc((MODE == kTrunk) ? a.w1 + (size_t)item * 4096 : a.w1);
    const __amdgpu_buffer_rsrc_t w2rs = chain_rsrc(a.w2_bf3), w3rs = chain_rsrc(a.w3_bf3);

    float runmax[16];   // running column maxima: [2 q + half], l3_pool16
    int runarg[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) { runmax[q] = -INFINITY; runarg[q] = 0; }
    PointFetcher<MODE, kMC> pf(a, item, cloud, nchunks, lane, wave);
    B3Ring ring3;
#pragma unroll
    for (int i = 0; i < 4; ++i) ring3.r[i] = b3_load16(w3rs, b16_lane_off(lane), 0, i >> 1, i & 1, wave_s);   // l3_pass_bf3: k-steps 0..1 of n-tile 0, both halves

    for (int ch = 0; ch < nchunks; ++ch) {
        const int rows_here = min(kMC, nrows - ch * kMC);
        const int mts = rows_here > 32 ? 2 : 1;
        // the per-lane addresses of stage 0b and layer 1 derive from `tq`, a copy of the thread index the compiler cannot see
        // through, and the folded 3 -> 64 rows of the lane's four channels are loaded per chunk, ahead of the barrier: loop-invariant,
        // they would otherwise sit in registers across layer 3, which has none to spare
        int tq = tid;
        asm volatile("" : "+v"(tq));
        f32x4 wi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wi[j] = *reinterpret_cast<const f32x4*>(a.w_in + ((tq & 15) * 4 + j) * 4);
        pf.stage0a(xs);
        __syncthreads();  // also orders the previous chunk's L3 reads of img before stage 0b rewrites it
        pf.advance(ch);
        // ---- stage 0b: 3 -> 64 (+bn, relu) -> act0 as three bf16 planes in img ---------------
        stage0b_planes<kMC, kPlane1B>(img, xs, wi, tq);
        // ---- L1: 64 -> 64 on v_mfma_f32_16x16x32_bf16 (l1_bf3): wave w = the 16 channels of n-tile w for every m-tile ----
        {
            const int ln = tq & 63;
            const L1Raw raw = l1_raw_load(w1rs, ln, wave_s);   // requested before the barrier, split and consumed after it
            f32x4 bq = {0.f, 0.f, 0.f, 0.f};
            if (MODE == kFstn) bq = *reinterpret_cast<const f32x4*>(a.b1 + 16 * wave_s + 4 * (ln >> 4));
            __syncthreads();
            if (mts == 2) l1_bf3<4, kPlane1B, MODE == kFstn>(img, act1, raw, bq, ln, wave_s);
            else          l1_bf3<2, kPlane1B, MODE == kFstn>(img, act1, raw, bq, ln, wave_s);
        }
        // ---- L2: 64 -> 128 (+bn, relu) on the bf16 matrix pipe: act1 and the weights as three bf16 terms, six products each
        //      (float32-exact).  v_mfma_f32_16x16x32_bf16, transposed tiles (the weight fragment as the A operand): the lane holds
        //      four consecutive channels of its row.  Per wave 32 rows x 64 channels = two passes (n-tiles nt0, nt0+2) of 2 point
        //      tiles x 2 channel tiles, 2 k-steps of 32; the second pass's weights are requested while the first computes ----
        {
            const int mt = wave & 1, nt0 = wave >> 1, nts = wave_s >> 1;
            constexpr int PF = ARGMAX ? 2 : 4;   // weight fragments in flight (the arg-max variant has no registers to spare)
            const int boff = b16_lane_off(lane);
            B3 bw[PF];
#pragma unroll
            for (int f = 0; f < PF; ++f) bw[f] = b3_load16_l2(w2rs, boff, nts, f >> 1, f & 1);   // fragment f of 8 = (pass, k-step, half)
            __syncthreads();
            if (mt < mts) {
                const unsigned char* a1p = act1 + mt * 32 * kLd1B;
                const int a1off = a16_lane_off<kLd1B>(lane), row = mt * 32 + (lane & 15), kq = lane >> 4;
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    f32x4 acc[2][2];
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) { acc[hf][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[hf][1] = acc[hf][0]; }
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        bf16x8 af[2][3];
#pragma unroll
                        for (int pi = 0; pi < 2; ++pi) a16_load<kLd1B, kPlane1B>(af[pi], a1p, a1off, pi, t);
#pragma unroll
                        for (int hf = 0; hf < 2; ++hf) {
                            const int f = pass * 4 + t * 2 + hf, nx = f + PF;
                            const B3 b = bw[f % PF];
                            if (nx < 8) bw[f % PF] = b3_load16_l2(w2rs, boff, nts + 2 * (nx >> 2), (nx >> 1) & 1, nx & 1);
                            mfma16_bf3_col_tr<2>(b, af, acc[hf]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const int c = (nt0 + 2 * pass) * 32 + 16 * hf;
                        l2_store_bf3<kPlaneB>(img, acc[hf], *reinterpret_cast<const f32x4*>(a.b2 + c + 4 * kq), row, c, lane);
                    }
                }
            }
        }
        __syncthreads();
        // ---- L3: 128 -> 1024, running column max: one n-tile per pass (the bitwise reference of the 96-row body) ----
        const int aoff = a16_lane_off<kLdB>(lane), boff = b16_lane_off(lane), row0 = ch * kMC + 4 * (lane >> 4);   // row0: ARGMAX only
        if (mts == 2) l3_pass_bf3<2, ARGMAX>(w3rs, boff, img, aoff, wave_s, runmax, ring3, runarg, row0);
        else          l3_pass_bf3<1, ARGMAX>(w3rs, boff, img, aoff, wave_s, runmax, ring3, runarg, row0);
    }
    chain_epilogue_bf3<MODE, ARGMAX>(a, item, wave, lane, runmax, runarg);
}

// ---- body 3 of 3: bf16x3 (L3V = 3), 96-row chunks: the two product instantiations <kFstn | kTrunk, 3, false> ----------------------
// act0 (bf16 planes, bytes 0 - 36 K), act1 (bf16 planes, bytes 36 K - 72 K) and act2 (bf16 planes, all 72 K) in ONE image, five
// barriers per chunk.  Every row's arithmetic is the 64-row body's.
template <int MODE>
__device__ __forceinline__ void chain_bf3_96(const ChainArgs& a, int item, int cloud, int nrows) {
    constexpr int kPlane96 = kMC96 * kLdB, kPlane96_1 = kMC96 * kLd1B, kAct1Off = 3 * kPlane96 - 3 * kPlane96_1;
    static_assert(3 * kPlane96_1 <= kAct1Off, "act0 and act1 are disjoint");
    __shared__ __attribute__((aligned(16))) unsigned char img[3 * kPlane96];
    __shared__ __attribute__((aligned(16))) float xs[kMC96 * 4];      // transformed inputs of the chunk (x,y,z,-)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nchunks = (nrows + kMC96 - 1) / kMC96;
    const int wave_s = uniform(wave);
    // weight images as buffer resources (kTrunk: layer 1 is this item's packed 64x64 transform, the fp32 kernels' image)
    const __amdgpu_buffer_rsrc_t w1rs = chain_rsrc((MODE == kTrunk) ? a.w1 + (size_t)item * 4096 : a.w1);
    const __amdgpu_buffer_rsrc_t w2rs = chain_rsrc(a.w2_bf3), w3rs = chain_rsrc(a.w3_bf3);

    float runmax[16];   // running column maxima: [2 q + half] as in the 64-row body, l3_pool16
#pragma unroll
    for (int q = 0; q < 16; ++q) runmax[q] = -INFINITY;
    PointFetcher<MODE, kMC96> pf(a, item, cloud, nchunks, lane, wave);
    B3Ring ring3;
#pragma unroll
    for (int i = 0; i < 4; ++i) ring3.r[i] = b3_load16(w3rs, b16_lane_off(lane), i >> 1, 0, i & 1, wave_s);   // l3_pass_bf3_2x2: k-step 0 of n-tiles 0 and 1

    // One 96-row chunk of MTS 32-row m-tiles.  Every chunk but an item's last is full, so the chunk loop holds the MTS = 3 body
    // alone and the last chunk picks its own: with the three layer-3 loops inside one chunk loop the compiler keeps the weight
    // ring and the running maxima in registers twice (before and inside each loop) and spills.
    auto chunk = [&](auto mtc, const int ch) {
        constexpr int mts = decltype(mtc)::value;
        unsigned char* const act1 = img + kAct1Off;
        // Every per-lane address below derives from `ln`, a copy of the lane index the compiler cannot see through: it otherwise
        // hoists some eighty loop-invariant addresses out of the chunk loop and keeps them in registers across layer 3, whose
        // 96 + 48 + 36 registers leave no room for them (they cost a few VALU instructions per chunk instead).
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int l15 = ln & 15, kq = ln >> 4;
        f32x4 wi[4];   // per chunk, ahead of the barrier: no registers for them across layer 3
#pragma unroll
        for (int j = 0; j < 4; ++j) wi[j] = *reinterpret_cast<const f32x4*>(a.w_in + ((ln & 15) * 4 + j) * 4);
        pf.stage0a(xs);
        __syncthreads();  // also orders the previous chunk's L3 reads of the image before stage 0b and layer 1 rewrite it
        pf.advance(ch);
        // stage 0b: 3 -> 64 (+bn, relu) -> act0 as three bf16 planes
        stage0b_planes<kMC96, kPlane96_1>(img, xs, wi, wave_s * 64 + ln);
        // L1: 64 -> 64 on v_mfma_f32_16x16x32_bf16, transposed tiles: wave w = the 16 channels of n-tile w for every m-tile
        {
            const L1Raw raw = l1_raw_load(w1rs, ln, wave_s);   // requested before the barrier, split and consumed after it
            f32x4 bq = {0.f, 0.f, 0.f, 0.f};
            if (MODE == kFstn) bq = *reinterpret_cast<const f32x4*>(a.b1 + 16 * wave_s + 4 * kq);
            __syncthreads();
            l1_bf3<2 * mts, kPlane96_1, MODE == kFstn>(img, act1, raw, bq, ln, wave_s);
        }
        // L2: 64 -> 128 (+bn, relu) on v_mfma_f32_16x16x32_bf16, transposed tiles: wave w = the 32 channels of n-tile w for every
        // m-tile, so its four weight fragments (2 k-steps x 2 halves, requested before the barrier) are loaded once per chunk.  The
        // 96 x 32 outputs stay in registers until every wave has read act1, which act2 overwrites.
        {
            const int boff = b16_lane_off(ln), a1off = a16_lane_off<kLd1B>(ln);
            B3 bw[4];
#pragma unroll
            for (int f = 0; f < 4; ++f) bw[f] = b3_load16_l2(w2rs, boff, wave_s, f >> 1, f & 1);   // fragment f = (k-step, half)
            f32x4 acc[2][3][2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) { acc[hf][mt][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[hf][mt][1] = acc[hf][mt][0]; }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int mt = 0; mt < 3; ++mt) {
                    if (mt < mts) {
                        bf16x8 af[2][3];
#pragma unroll
                        for (int pi = 0; pi < 2; ++pi) a16_load<kLd1B, kPlane96_1>(af[pi], act1, a1off, 2 * mt + pi, t);
#pragma unroll
                        for (int hf = 0; hf < 2; ++hf) mfma16_bf3_col_tr<2>(bw[2 * t + hf], af, acc[hf][mt]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            __syncthreads();   // act1 is read: act2 may take its place
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                const int c = wave_s * 32 + 16 * hf;
                const f32x4 bq = *reinterpret_cast<const f32x4*>(a.b2 + c + 4 * kq);
#pragma unroll
                for (int mt = 0; mt < 3; ++mt)
                    if (mt < mts) l2_store_bf3<kPlane96>(img, acc[hf][mt], bq, mt * 32 + l15, c, ln);
            }
        }
        __syncthreads();
        // L3: 128 -> 1024, running column max
        l3_pass_bf3_2x2<mts, kPlane96>(w3rs, b16_lane_off(ln), img, a16_lane_off<kLdB>(ln), wave_s, runmax, ring3);
    };
    for (int ch = 0; ch + 1 < nchunks; ++ch) chunk(std::integral_constant<int, 3>{}, ch);
    const int rows_last = nrows - (nchunks - 1) * kMC96;
    if (rows_last > 64)      chunk(std::integral_constant<int, 3>{}, nchunks - 1);
    else if (rows_last > 32) chunk(std::integral_constant<int, 2>{}, nchunks - 1);
    else                     chunk(std::integral_constant<int, 1>{}, nchunks - 1);
    chain_epilogue_bf3<MODE, false>(a, item, wave, lane, runmax, nullptr);
}

// CM = ChainMode; MODE = the chain it names.  The common prologue, then ONE choice of body: fp32 (L3V = 2), or - L3V = 3 - 96-row
// chunks in the two product instantiations <kFstn | kTrunk, 3, false> and 64-row chunks in the others.
template <int CM, int L3V, bool ARGMAX = false>
__global__ __launch_bounds__(kThreads, L3V == 3 ? 2 : 3) void pn_chain_kernel(ChainArgs a) {
    constexpr int MODE = CM >= kFstn64 ? CM - kFstn64 + kFstn : CM;
    static_assert(CM < kFstn64 || (L3V == 3 && !ARGMAX), "kFstn64 / kTrunk64: the 64-row twins of the product instantiations only");
    if (MODE != kPrepool && a.n_dev && (int)blockIdx.x >= *a.n_dev) return;   // past the distinct coalitions: no entry in item_order
    const int item = a.item_order ? a.item_order[blockIdx.x] : blockIdx.x;
    int cloud;
    if (MODE == kPrepool) cloud = item / (a.R + a.with_centre);
    else cloud = a.cloud_of ? a.cloud_of[item] : (a.nclouds == 1 ? 0 : item);

    const int nrows = a.nrows[item] & 0xffff;
    if (nrows == 0) {  // empty region in the pre-pool: identity of max
        float* outp = a.out + (size_t)item * kFeat;
        for (int c = threadIdx.x; c < kFeat; c += kThreads) outp[c] = -INFINITY;
        return;
    }
    if constexpr (L3V == 2) chain_fp32<MODE, ARGMAX>(a, item, cloud, nrows);
    else if constexpr ((CM == kFstn || CM == kTrunk) && !ARGMAX) chain_bf3_96<MODE>(a, item, cloud, nrows);
    else chain_bf3_64<MODE, ARGMAX>(a, item, cloud, nrows);
}

template <int MODE>
int launch_chain(const ChainArgs& a, hipStream_t st) {
    // twins kTwinChainL3Fp32 / kTwinChainL3Fp32NoTail16: layer 3 on the fp32 MFMA (round 3's kernel; A/B and tests)
    const bool bf3 = a.w3_bf3 && a.w2_bf3 && iq::twin() != iq::kTwinChainL3Fp32 && iq::twin() != iq::kTwinChainL3Fp32NoTail16;
    if constexpr (MODE == kTrunk) {
        if (a.argrow) {
            if (bf3) IQ_LAUNCH((pn_chain_kernel<kTrunk, 3, true>), dim3(a.items), dim3(kThreads), 0, st, a);
            else     IQ_LAUNCH((pn_chain_kernel<kTrunk, 2, true>), dim3(a.items), dim3(kThreads), 0, st, a);
            return IQ_OK;
        }
    }
    if constexpr (MODE != kPrepool) {
        if (bf3) {   // the product path: 96-row chunks; twin kTwinChainL3Single: 64-row chunks, one n-tile per pass (its bitwise reference)
            if (a.l3_single) IQ_LAUNCH((pn_chain_kernel<MODE - kFstn + kFstn64, 3>), dim3(a.items), dim3(kThreads), 0, st, a);
            else             IQ_LAUNCH((pn_chain_kernel<MODE, 3>), dim3(a.items), dim3(kThreads), 0, st, a);
            return IQ_OK;
        }
    }
    IQ_LAUNCH((pn_chain_kernel<MODE, 2>), dim3(a.items), dim3(kThreads), 0, st, a);
    return IQ_OK;
}

}  // namespace
