// Fused fp32-MFMA PointNet forward over coalitions (models/pointnet.py:11-115).
//
// A masked cloud is {kept points} + {the centre, if anything was masked}.  Every per-point layer
// is a pointwise function and every pooling is a max, so
//   * the input-STN's 3->64->128->1024 chain is evaluated ONCE per cloud and pre-pooled per region
//     (chain<kPrepool>); a coalition's pooled feature is a max over its kept regions (+ centre);
//   * the feature-STN and trunk chains run only over a coalition's DISTINCT points.
// Both are exact with respect to evaluating the same kernels on the materialised cloud.
//
// chain kernel: one workgroup (4 waves) per coalition, 64-row chunks (96 in the product instantiations, below):
//   stage0 (VALU)  x -> x.trans -> conv1(3->64)+bn+relu                      -> LDS act0
//   L1  (MFMA)     64->64   (fstn.conv1 | per-coalition trans_feat product)  -> LDS act1
//   L2  (MFMA)     64->128  conv2+bn+relu                                    -> LDS act2
//   L3  (MFMA)     128->1024 conv3+bn(+relu), column max over rows           -> registers
// L3V = 2: v_mfma_f32_32x32x2_f32 throughout (exact fp32 fma chains).  A operands come from LDS (row stride padded by 4 floats:
// conflict-free ds_read_b128), B operands (weights) stream from L2 in a pre-packed fragment order (1 KiB contiguous per wave-load).
// LDS = 52 KB -> 3 workgroups/CU.
// L3V = 3 (the product path of the feature-STN and trunk chains): layers 1-3 as six exact bf16 products per float32 product on
// v_mfma_f32_16x16x32_bf16 (iq_bf3.h; DESIGN.md 5a: the kernel is power-bound and this shape holds a 10 % higher clock than
// 32x32x16), activations - act0 included, split by stage 0b - as three swizzled bf16 planes in LDS.  Layer 1 reads its weights out
// of the SAME fp32 images as the fp32 kernels (the packed fstn.conv1, the per-coalition transform) and splits them into bf16 terms
// in registers, four b128 loads per wave and chunk (l1_raw_load, l1_bf3): wave w = the 16 channels of n-tile w for every 16-row
// m-tile.  No v_mfma_f32_32x32x2_f32 is left in these kernels (tests/test_isa_chain_l1_cpu.py).  LDS = 74.8 KB, <= 256 VGPRs ->
// 2 workgroups/CU.
// The two product instantiations (<kFstn | kTrunk, 3, false>) work on 96-ROW chunks: a layer-3 weight fragment then feeds six
// 16-row m-tiles instead of four, a third less weight streaming out of L2 per row.  Two workgroups still fit a CU because act0,
// act1 and act2 share ONE 72 KB image (act0 bytes 0 - 36 K, act1 36 - 72 K, act2 all of it: layer 2 keeps its 96 x 32 outputs per
// wave in registers until every wave has read act1, one more barrier per chunk): LDS = 73.5 KB, 252 VGPRs, no scratch.  Every
// row's arithmetic is the 64-row kernels', which stay as they are from layer 2 on (pre-pool, fp32 twins, arg-max, twin
// kTwinChainL3Single) and are the 96-row kernel's bitwise reference.  Row lists are padded for both chunk sizes (padded_rows).
#include <algorithm>
#include <type_traits>

#include "iq_common.h"
#include "iq_profile.h"

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
    const int32_t* dup_rep;    // [2] first full-set / first empty-set item of the batch, or null: the other such items are copies of
                               // it and leave at once (pn_dup_rep_kernel, pn_dup_copy_kernel)              [kFstn/kTrunk]
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
            if (RELU) v = (f32x4){fmaxf(v[0] + bq[0], 0.f), fmaxf(v[1] + bq[1], 0.f), fmaxf(v[2] + bq[2], 0.f), fmaxf(v[3] + bq[3], 0.f)};
            c16_tile_to_planes_swz<kLd1B, PLANEB>(act1, 16 * (p + i) + l15, 2 * wave_s, ln, v);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Coalitions that recur in a batch: every permutation of a Shapley sample contributes the full set (prefix R) and the empty set
// (prefix 0), 2 of its R + 1 coalitions, and all full sets of a cloud are the same rows under the same transforms.  nrows tells
// both: all N points and no centre row (nothing masked) -> 0, the centre row alone -> 1, anything else -> -1.
__device__ __forceinline__ int dup_kind(int nrows_word, int N) { return nrows_word == N ? 0 : nrows_word == ((1 << 16) | 1) ? 1 : -1; }

// CM = ChainMode; MODE = the chain it names, MC = rows per chunk: 96 in the two product instantiations <kFstn | kTrunk, 3, false>, else 64
template <int CM, int L3V, bool ARGMAX = false>
__global__ __launch_bounds__(kThreads, L3V == 3 ? 2 : 3) void pn_chain_kernel(ChainArgs a) {
    constexpr int MODE = CM >= kFstn64 ? CM - kFstn64 + kFstn : CM;
    constexpr int MC = (CM == kFstn || CM == kTrunk) && L3V == 3 && !ARGMAX ? kMC96 : kMC;
    static_assert(CM < kFstn64 || (L3V == 3 && !ARGMAX), "kFstn64 / kTrunk64: the 64-row twins of the product instantiations only");
    // act0 (ld 68) then act2: float image (ld 132), or - L3V = 3 - act0 as three bf16 planes of 128-byte rows (24 KB), then act2
    // as three bf16 planes of 256-byte rows.  MC = 96: the ONE image
    // that act0, act1 and act2 share (kAct1Off); bufB is then a placeholder for the 64-row bases below and takes no LDS
    __shared__ __attribute__((aligned(16))) float bufA[L3V == 3 ? 3 * MC * kLdB / 4 : kMC * kLd2];
    __shared__ __attribute__((aligned(16))) float bufB[MC == kMC96 ? 4 : (L3V == 3 ? 3 * kPlane1B / 4 : kMC * kLd1)];  // act1 (L3V = 3: three bf16 planes)
    __shared__ __attribute__((aligned(16))) float xs[MC * 4];        // transformed inputs of the chunk (x,y,z,-)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int item = a.item_order ? a.item_order[blockIdx.x] : blockIdx.x;
    const int N = a.N;
    int cloud;
    if (MODE == kPrepool) cloud = item / (a.R + a.with_centre);
    else cloud = a.cloud_of ? a.cloud_of[item] : (a.nclouds == 1 ? 0 : item);

    const int nrows = a.nrows[item] & 0xffff;
    if (MODE != kPrepool && a.dup_rep) {   // a repeated full or empty set: pn_dup_copy_kernel fills its row from the first one's
        const int kind = dup_kind(a.nrows[item], N);
        if (kind >= 0 && a.dup_rep[kind] != item) return;
    }
    float* outp = a.out + (size_t)item * kFeat;
    if (nrows == 0) {  // empty region in the pre-pool: identity of max
        for (int c = tid; c < kFeat; c += kThreads) outp[c] = -INFINITY;
        return;
    }
    const int nchunks = (nrows + MC - 1) / MC;

    // (64-row chunks: stage 0b's channel and row group, the fp32 weight images and the per-lane bases; the 96-row body derives its own)
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

    // running column maxima: fp32 layer 3 - [q] = n-tile q * 4 + wave, column lane & 31; bf16x3 layer 3 - [2 q + half], l3_pool16
    constexpr int NRUN = L3V == 3 ? 16 : 8;
    float runmax[NRUN];
    int runarg[NRUN];
#pragma unroll
    for (int q = 0; q < NRUN; ++q) { runmax[q] = -INFINITY; runarg[q] = 0; }

    // Input points travel ahead in registers: lanes 0..15 (23) of each wave own 16 (24) rows of a chunk.  The
    // row index of chunk c+2 and the coordinates of chunk c+1 are requested while chunk c computes, so
    // neither of the two dependent global loads is ever waited for.
    const bool fetcher = lane < MC / 4;
    const int frow = wave * (MC / 4) + lane;
    const uint16_t* rowp = a.rows + (size_t)item * kRowCap + frow;
    float px = 0.f, py = 0.f, pz = 0.f;
    auto load_point = [&](int p) {
        if (p == N) {
            px = a.centers[cloud * 3]; py = a.centers[cloud * 3 + 1]; pz = a.centers[cloud * 3 + 2];
        } else {
            const float* src = a.clouds + (size_t)cloud * a.cl + (size_t)p * a.ps;
            px = src[0]; py = src[a.cs]; pz = src[2 * a.cs];
        }
    };
    int pnext = 0;
    if (fetcher) {
        load_point(rowp[0]);
        if (nchunks > 1) pnext = rowp[MC];
    }

    BRing ring;
    if (L3V == 2) bring_init(ring, w3b, wave_s);
    [[maybe_unused]] B3Ring ring3;
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t w3rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(L3V == 3 ? a.w3_bf3 : nullptr), 0, 0x7fffffff, 0x00020000);
    [[maybe_unused]] const __amdgpu_buffer_rsrc_t w2rs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short*>(L3V == 3 ? a.w2_bf3 : nullptr), 0, 0x7fffffff, 0x00020000);
    if (L3V == 3) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // l3_pass_bf3: k-steps 0..1 of n-tile 0, both halves; l3_pass_bf3_2x2: k-step 0 of n-tiles 0 and 1
            const bool single = MC == kMC;   // 64-row chunks: the arg-max instantiation and twin kTwinChainL3Single
            ring3.r[i] = b3_load16(w3rs, b16_lane_off(lane), single ? 0 : i >> 1, single ? i >> 1 : 0, i & 1, wave_s);
        }
    }
    if constexpr (MC == kMC96) {
        // One 96-row chunk of MTS 32-row m-tiles.  Every chunk but an item's last is full, so the chunk loop holds the MTS = 3 body
        // alone and the last chunk picks its own: with the three layer-3 loops inside one chunk loop the compiler keeps the weight
        // ring and the running maxima in registers twice (before and inside each loop) and spills.
        auto chunk = [&](auto mtc, const int ch) {
            constexpr int mts = decltype(mtc)::value;
            // ---- 96-row chunk: act0 (bf16 planes, bytes 0 - 36 K), act1 (bf16 planes, bytes 36 K - 72 K) and act2 (bf16 planes, all 72 K)
            //      in ONE image, five barriers.  Every row's arithmetic is the 64-row body's. ---------------------------------------
            constexpr int kPlane96 = kMC96 * kLdB, kPlane96_1 = kMC96 * kLd1B, kAct1Off = 3 * kPlane96 - 3 * kPlane96_1;
            static_assert(3 * kPlane96_1 <= kAct1Off, "act0 and act1 are disjoint");
            unsigned char* const img = reinterpret_cast<unsigned char*>(bufA);
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
            // stage 0a: input transform
            if (fetcher) {
                float x = px, y = py, z = pz;
                const float* t9 = a.trans + (size_t)item * 9;  // uniform -> scalar loads
                const float x2 = fmaf(z, t9[6], fmaf(y, t9[3], x * t9[0]));
                const float y2 = fmaf(z, t9[7], fmaf(y, t9[4], x * t9[1]));
                const float z2 = fmaf(z, t9[8], fmaf(y, t9[5], x * t9[2]));
                *reinterpret_cast<f32x4*>(xs + frow * 4) = (f32x4){x2, y2, z2, 0.f};
            }
            __syncthreads();  // also orders the previous chunk's L3 reads of the image before stage 0b and layer 1 rewrite it
            if (fetcher && ch + 1 < nchunks) {
                load_point(pnext);
                if (ch + 2 < nchunks) pnext = rowp[(ch + 2) * MC];
            }
            // stage 0b: 3 -> 64 (+bn, relu) -> act0 as three bf16 planes
            stage0b_planes<kMC96, kPlane96_1>(img, xs, wi, wave_s * 64 + ln);
            // L1: 64 -> 64 on v_mfma_f32_16x16x32_bf16, transposed tiles: wave w = the 16 channels of n-tile w for every m-tile
            {
                const L1Raw raw = l1_raw_load(w1b.rsrc, ln, wave_s);   // requested before the barrier, split and consumed after it
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
                    for (int mt = 0; mt < 3; ++mt) {
                        if (mt < mts) {
#pragma unroll
                            for (int pi = 0; pi < 2; ++pi) {
                                const f32x4 v = {fmaxf(acc[hf][mt][pi][0] + bq[0], 0.f), fmaxf(acc[hf][mt][pi][1] + bq[1], 0.f),
                                                 fmaxf(acc[hf][mt][pi][2] + bq[2], 0.f), fmaxf(acc[hf][mt][pi][3] + bq[3], 0.f)};
                                c16_tile_to_planes_swz<kLdB, kPlane96>(img, mt * 32 + 16 * pi + l15, c / 8, ln, v);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            // L3: 128 -> 1024, running column max
            {
                const int aoff = a16_lane_off<kLdB>(ln), boff = b16_lane_off(ln);
                l3_pass_bf3_2x2<mts, kPlane96>(w3rs, boff, img, aoff, wave_s, runmax, ring3);
            }
        };
        for (int ch = 0; ch + 1 < nchunks; ++ch) chunk(std::integral_constant<int, 3>{}, ch);
        const int rows_last = nrows - (nchunks - 1) * MC;
        if (rows_last > 64)      chunk(std::integral_constant<int, 3>{}, nchunks - 1);
        else if (rows_last > 32) chunk(std::integral_constant<int, 2>{}, nchunks - 1);
        else                     chunk(std::integral_constant<int, 1>{}, nchunks - 1);
    } else   // 64-row chunks: the loop below
    for (int ch = 0; ch < nchunks; ++ch) {
        const int rows_here = min(kMC, nrows - ch * kMC);
        const int mts = rows_here > 32 ? 2 : 1;
        // (L3V = 3) the per-lane addresses of stage 0b and layer 1 derive from `tq`, a copy of the thread index the compiler cannot see
        // through, and the folded 3 -> 64 rows of the lane's four channels are loaded per chunk, ahead of the barrier: loop-invariant,
        // they would otherwise sit in registers across layer 3, which has none to spare
        [[maybe_unused]] int tq = tid;
        [[maybe_unused]] f32x4 wi[4];
        if constexpr (L3V == 3) {
            asm volatile("" : "+v"(tq));
#pragma unroll
            for (int j = 0; j < 4; ++j) wi[j] = *reinterpret_cast<const f32x4*>(a.w_in + ((tq & 15) * 4 + j) * 4);
        }
        // ---- stage 0a: input transform (models/pointnet.py:67-69) --------------------------
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
        __syncthreads();  // also orders the previous chunk's L3 reads of bufA before stage 0b rewrites it
        if (fetcher && ch + 1 < nchunks) {
            load_point(pnext);
            if (ch + 2 < nchunks) pnext = rowp[(ch + 2) * MC];
        }
        // ---- stage 0b: 3 -> 64 (+bn, relu), thread = (channel c0, 16 rows); L3V = 3: act0 as three bf16 planes in bufA ----
        if constexpr (L3V == 3) {
            stage0b_planes<kMC, kPlane1B>(reinterpret_cast<unsigned char*>(bufA), xs, wi, tq);
        } else {
            float* dst = ((MODE == kPrepool) ? bufB : bufA) + rg * 16 * kLd1 + c0;
#pragma unroll 4
            for (int i = 0; i < 16; ++i) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + (rg * 16 + i) * 4);
                const float f = fmaf(win[2], xv[2], fmaf(win[1], xv[1], win[0] * xv[0])) + win[3];
                dst[i * kLd1] = fmaxf(f, 0.f);
            }
        }
        // ---- L1: 64 -> 64 ------------------------------------------------------------------
        if constexpr (L3V == 3) {   // on v_mfma_f32_16x16x32_bf16 (l1_bf3): wave w = the 16 channels of n-tile w for every m-tile
            const int ln = tq & 63;
            const L1Raw raw = l1_raw_load(w1b.rsrc, ln, wave_s);   // requested before the barrier, split and consumed after it
            f32x4 bq = {0.f, 0.f, 0.f, 0.f};
            if (MODE == kFstn) bq = *reinterpret_cast<const f32x4*>(a.b1 + 16 * wave_s + 4 * (ln >> 4));
            __syncthreads();
            unsigned char* const act0 = reinterpret_cast<unsigned char*>(bufA);
            unsigned char* const act1 = reinterpret_cast<unsigned char*>(bufB);
            if (mts == 2) l1_bf3<4, kPlane1B, MODE == kFstn>(act0, act1, raw, bq, ln, wave_s);
            else          l1_bf3<2, kPlane1B, MODE == kFstn>(act0, act1, raw, bq, ln, wave_s);
        } else if (MODE != kPrepool) {
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
        if constexpr (L3V == 3) {   // on the bf16 matrix pipe: act1 and the weights as three bf16 terms, six products each (float32-exact)
            // v_mfma_f32_16x16x32_bf16, transposed tiles (the weight fragment as the A operand): the lane holds four consecutive
            // channels of its row.  Per wave 32 rows x 64 channels = two passes of 2 point tiles x 2 channel tiles, 2 k-steps of 32.
            const int mt = wave & 1, nt0 = wave >> 1, nts = wave_s >> 1;
            constexpr int PF = ARGMAX ? 2 : 4;   // weight fragments in flight (the arg-max variant has no registers to spare)
            const int boff = b16_lane_off(lane);
            B3 bw[PF];
#pragma unroll
            for (int f = 0; f < PF; ++f) bw[f] = b3_load16_l2(w2rs, boff, nts, f >> 1, f & 1);   // fragment f of 8 = (pass, k-step, half)
            __syncthreads();
            if (mt < mts) {
                const unsigned char* a1p = reinterpret_cast<const unsigned char*>(bufB) + mt * 32 * kLd1B;
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
                        const int ch = (nt0 + 2 * pass) * 32 + 16 * hf;
                        const f32x4 bq = *reinterpret_cast<const f32x4*>(a.b2 + ch + 4 * kq);
#pragma unroll
                        for (int pi = 0; pi < 2; ++pi) {
                            const f32x4 v = {fmaxf(acc[hf][pi][0] + bq[0], 0.f), fmaxf(acc[hf][pi][1] + bq[1], 0.f),
                                             fmaxf(acc[hf][pi][2] + bq[2], 0.f), fmaxf(acc[hf][pi][3] + bq[3], 0.f)};
                            c16_tile_to_planes_swz<kLdB, kPlaneB>(reinterpret_cast<unsigned char*>(bufA), row + 16 * pi, ch / 8, lane, v);
                        }
                    }
                }
            }
        } else {
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
        if constexpr (L3V == 3) {
            const unsigned char* ab3 = reinterpret_cast<const unsigned char*>(bufA);
            const int aoff = a16_lane_off<kLdB>(lane), boff = b16_lane_off(lane);
            if constexpr (ARGMAX) {
                const int row0 = ch * kMC + 4 * (lane >> 4);
                if (mts == 2) l3_pass_bf3<2, true>(w3rs, boff, ab3, aoff, wave_s, runmax, ring3, runarg, row0);
                else          l3_pass_bf3<1, true>(w3rs, boff, ab3, aoff, wave_s, runmax, ring3, runarg, row0);
            } else {   // twin kTwinChainL3Single (launch_chain): one n-tile per pass, the bitwise reference of the 96-row kernel
                if (mts == 2) l3_pass_bf3<2>(w3rs, boff, ab3, aoff, wave_s, runmax, ring3, runarg);
                else          l3_pass_bf3<1>(w3rs, boff, ab3, aoff, wave_s, runmax, ring3, runarg);
            }
        } else {
            const bool tail = !ARGMAX && a.tail16 && rows_here - 32 * (mts - 1) <= 16;   // (uniform) the last m-tile holds <= 16 rows
            if (mts == 2 && !tail) l3_pass_v2<2, ARGMAX>(w3b, a2base, wave_s, runmax, ring, runarg, ch * kMC, frag_h);
            else if (mts == 2 || !tail) l3_pass_v2<1, ARGMAX>(w3b, a2base, wave_s, runmax, ring, runarg, ch * kMC, frag_h);
            if (tail) l3_tail16(w3b, bufA, 32 * (mts - 1), wave_s, lane, runmax, ring);
        }
    }

    // max commutes with the (monotone) per-column bias add and relu
    if constexpr (L3V == 3) {   // the four kq lanes of a column hold rows 4 kq + i of every m-tile: larger value wins, then the lower row
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
                if (lane < 16 && a.argrow) a.argrow[(size_t)item * kFeat + n] = (int)a.rows[(size_t)item * kRowCap + r];   // row -> point
            } else {
                v = fmaxf(v, __shfl_xor(v, 16));
                v = fmaxf(v, __shfl_xor(v, 32));
            }
            v += a.b3[n];
            if (MODE != kTrunk) v = fmaxf(v, 0.f);
            if (lane < 16) outp[n] = v;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float v = runmax[q];
            const int n = (q * 4 + wave) * 32 + (lane & 31);
            if constexpr (ARGMAX) {   // the other half-wave saw rows 4..7 (+8 k) of every tile: larger value wins, then the lower row
                const float v2 = __shfl_xor(v, 32);
                const int r2 = __shfl_xor(runarg[q], 32);
                const int r = (v2 > v || (v2 == v && r2 < runarg[q])) ? r2 : runarg[q];
                if (lane < 32 && a.argrow) a.argrow[(size_t)item * kFeat + n] = (int)a.rows[(size_t)item * kRowCap + r];   // row -> point
            }
            v = fmaxf(v, __shfl_xor(v, 32));
            v += a.b3[n];
            if (MODE != kTrunk) v = fmaxf(v, 0.f);
            if (lane < 32) outp[n] = v;
        }
    }
}

// ---- per-cloud region tables: points grouped by region (counting sort) ------------------------
// sorted_pts: the points of region 0, 1, .. R-1 in ascending point order; roff[r]: where region r starts (roff[R]: the end).
// A stable counting sort on kThreads / 64 waves: wave w owns the w-th quarter of the points.  Counts per (wave, region), one
// scan over the regions that turns them into the first slot of each wave in each region, then every wave walks its points 64
// at a time: the lanes of one region find each other by ballot, a lane's rank among them is a population count, and the slot
// table is read and moved once per 64 points.  (The rank used to be a loop over all earlier points, per point.)  MAXR: IQ_MAX_REGIONS or IQ_MAX_WIDE_REGIONS, the size of the tables.
template <int MAXR>
__device__ __forceinline__ void pn_prepare_body(const int32_t* __restrict__ region_id, uint16_t* __restrict__ sorted_pts,
                                                int32_t* __restrict__ roff, int N, int R) {
    constexpr int kWaves = kThreads / 64;
    __shared__ int16_t rid[kMaxN];
    __shared__ int cnt[kWaves][MAXR + 1];          // points of (wave, region); after the scan: the next free slot of that wave there
    const int cloud = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int r = tid; r <= R; r += kThreads)
        for (int w = 0; w < kWaves; ++w) cnt[w][r] = 0;
    for (int p = tid; p < N; p += kThreads) {
        // an id outside [0,R) (rejected by iq_check_index_range; never produced by iq_region_assign) goes to bucket R,
        // which no coalition keeps: the point counts as masked instead of indexing LDS / the workspace out of bounds
        const int r = region_id[(size_t)cloud * N + p];
        rid[p] = (int16_t)((unsigned)r < (unsigned)R ? r : R);
    }
    __syncthreads();
    const int per = (N + kThreads - 1) / kThreads * 64;          // points per wave, whole steps of 64
    const int begin = min(wave * per, N), end = min(begin + per, N);
    for (int p = begin + lane; p < end; p += 64) atomicAdd(&cnt[wave][rid[p]], 1);
    __syncthreads();
    if (wave == 0) {                               // exclusive scan over (region, wave), 64 regions at a time; bucket R holds nothing
        int carry = 0;
        for (int r0 = 0; r0 <= R; r0 += 64) {
            const int r = r0 + lane;
            int c[kWaves], tot = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) { c[w] = r < R ? cnt[w][r] : 0; tot += c[w]; }
            int inc = tot;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(inc, off);
                if (lane >= off) inc += t;
            }
            int slot = carry + inc - tot;
            if (r <= R) {
                roff[(size_t)cloud * (R + 1) + r] = slot;
#pragma unroll
                for (int w = 0; w < kWaves; ++w) { cnt[w][r] = slot; slot += c[w]; }
            }
            carry += __shfl(inc, 63);
        }
    }
    __syncthreads();
    for (int p0 = begin; p0 < end; p0 += 64) {
        const int p = p0 + lane;
        const int r = p < end ? rid[p] : R;
        const bool placed = r < R;
        int rank = 0, total = 0;                   // this lane among the lanes of its region, and how many they are
        unsigned long long pending = __ballot(placed);
        while (pending) {                          // one trip per region present among the 64 points, registers only
            const int rl = __builtin_amdgcn_readlane(r, __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1));
            const unsigned long long same = __ballot(placed && r == rl);
            if (placed && r == rl) {
                rank = __popcll(same & ((1ull << lane) - 1));
                total = __popcll(same);
            }
            pending &= ~same;
        }
        const int slot = cnt[wave][r];             // (bucket R: read, never used)
        if (placed) sorted_pts[(size_t)cloud * N + slot + rank] = (uint16_t)p;
        __builtin_amdgcn_wave_barrier();           // every lane has read its slot before the first of a region moves it
        if (placed && rank == 0) cnt[wave][r] = slot + total;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

__global__ __launch_bounds__(kThreads) void pn_prepare_kernel(const int32_t* __restrict__ region_id,
                                                              uint16_t* __restrict__ sorted_pts,
                                                              int32_t* __restrict__ roff, int N, int R) {
    pn_prepare_body<IQ_MAX_REGIONS>(region_id, sorted_pts, roff, N, R);
}

// ---- compacted row list of every work item (one wave per item) --------------------------------
// Coalition items: keep[item] (null = everything), centre appended iff a point is masked.
// Pre-pool items (prepool != 0): item = cloud*(R+with_centre) + r; r < R keeps region r only (no
// centre), r == R is the centre alone.  The list is padded with replicas of a valid row (duplicates
// never change a max) to a multiple of the chunk size of either chain kernel, whichever ends later:
// the 96-row kernel's fetch lanes read whole chunks (at most 43 x 96 = 4128 <= kRowCap entries).
__device__ __forceinline__ int padded_rows(int nrows) {
    static_assert((kMaxN + kMC96 - 1) / kMC96 * kMC96 <= kRowCap, "a padded row list fits its stride");
    return max((nrows + kMC - 1) / kMC * kMC, (nrows + kMC96 - 1) / kMC96 * kMC96);
}
__global__ __launch_bounds__(64) void pn_rows_kernel(const uint16_t* __restrict__ sorted_all,
                                                     const int32_t* __restrict__ roff_all,
                                                     const uint64_t* __restrict__ keep_all,
                                                     const int32_t* __restrict__ cloud_of, uint16_t* __restrict__ rows_all,
                                                     int32_t* __restrict__ nrows_all, int N, int R, int nclouds,
                                                     int with_centre, int prepool) {
    const int item = blockIdx.x, lane = threadIdx.x;
    int cloud;
    uint64_t keep;
    bool add_centre;
    if (prepool) {
        const int per = R + with_centre;
        cloud = item / per;
        const int r = item - cloud * per;
        keep = r < R ? (1ull << r) : 0ull;
        add_centre = (r == R);
    } else {
        cloud = cloud_of ? cloud_of[item] : (nclouds == 1 ? 0 : item);
        const uint64_t full = R >= 64 ? ~0ull : ((1ull << R) - 1);
        keep = (keep_all ? keep_all[item] : ~0ull) & full;
        add_centre = false;
    }
    const int32_t* roff = roff_all + (size_t)cloud * (R + 1);
    const uint16_t* sorted_pts = sorted_all + (size_t)cloud * N;
    uint16_t* rows = rows_all + (size_t)item * kRowCap;

    const int sz = (lane < R && ((keep >> lane) & 1)) ? roff[lane + 1] - roff[lane] : 0;
    int inc = sz;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    const int kst = inc - sz;
    const int nkept = __shfl(inc, 63);
    if (!prepool) add_centre = with_centre && nkept < N;
    const int nrows = nkept + (add_centre ? 1 : 0);
    for (int r = 0; r < R; ++r) {
        if (!((keep >> r) & 1)) continue;
        const int ks = __shfl(kst, r), off = roff[r], n = roff[r + 1] - off;
        for (int j = lane; j < n; j += 64) rows[ks + j] = sorted_pts[off + j];
    }
    // padding value: the centre if present, else the last kept point
    int padval = N;
    if (!add_centre && nkept > 0) {
        const unsigned long long last = __ballot(sz > 0 && kst + sz == nkept);
        const int rl = __ffsll((long long)last) - 1;
        padval = sorted_pts[roff[rl + 1] - 1];
    }
    const int npad = padded_rows(nrows);
    for (int i = nkept + lane; i < npad; i += 64) rows[i] = (uint16_t)padval;
    if (lane == 0) nrows_all[item] = nrows | (add_centre ? (1 << 16) : 0);
}

// ---- the same two kernels for wide coalitions (R up to IQ_MAX_WIDE_REGIONS, keep rows of W = ceil(R / 64) words) --------------
// They write what their narrow twins write - points grouped by region in ascending point order; row lists of the kept regions in
// ascending region order, the centre and the padding by the same rules - so the chain kernel sees the same lists for R <= 64.
constexpr int kMaxW = IQ_MAX_WIDE_REGIONS / 64;

__global__ __launch_bounds__(kThreads) void pn_prepare_wide_kernel(const int32_t* __restrict__ region_id,
                                                                   uint16_t* __restrict__ sorted_pts,
                                                                   int32_t* __restrict__ roff, int N, int R) {
    pn_prepare_body<IQ_MAX_WIDE_REGIONS>(region_id, sorted_pts, roff, N, R);
}

// One wave per item.  The start of every kept region in the row list comes from a scan over the regions, 64 at a time.  A region of
// a wide game holds few points (N / R: one at R = N), so above 64 regions a lane copies whole regions instead of the wave one.
__global__ __launch_bounds__(64) void pn_rows_wide_kernel(const uint16_t* __restrict__ sorted_all,
                                                          const int32_t* __restrict__ roff_all,
                                                          const uint64_t* __restrict__ keep_all,
                                                          const int32_t* __restrict__ cloud_of, uint16_t* __restrict__ rows_all,
                                                          int32_t* __restrict__ nrows_all, int N, int R, int W, int nclouds,
                                                          int with_centre, int prepool) {
    __shared__ int kst_s[IQ_MAX_WIDE_REGIONS];   // first row of a kept region, -1 = not kept
    const int item = blockIdx.x, lane = threadIdx.x;
    uint16_t* rows = rows_all + (size_t)item * kRowCap;
    int nkept = 0, padval = N;
    bool add_centre;
    if (prepool) {   // item = cloud * (R + with_centre) + r: region r alone (no centre), r == R the centre alone
        const int per = R + with_centre, cloud = item / per, r = item - cloud * per;
        const int32_t* roff = roff_all + (size_t)cloud * (R + 1);
        const uint16_t* sorted_pts = sorted_all + (size_t)cloud * N;
        add_centre = (r == R);
        if (r < R) {
            const int off = roff[r];
            nkept = roff[r + 1] - off;
            for (int j = lane; j < nkept; j += 64) rows[j] = sorted_pts[off + j];
            if (nkept > 0) padval = sorted_pts[off + nkept - 1];
        }
    } else {
        const int cloud = cloud_of ? cloud_of[item] : (nclouds == 1 ? 0 : item);
        const int32_t* roff = roff_all + (size_t)cloud * (R + 1);
        const uint16_t* sorted_pts = sorted_all + (size_t)cloud * N;
        const uint64_t* keep = keep_all ? keep_all + (size_t)item * W : nullptr;   // null = everything
        int last_r = -1;   // the last kept region that holds a point
        for (int r0 = 0; r0 < R; r0 += 64) {
            const int r = r0 + lane;
            const bool kept = r < R && (!keep || ((keep[r0 >> 6] >> lane) & 1));
            const int sz = kept ? roff[r + 1] - roff[r] : 0;
            int inc = sz;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(inc, off);
                if (lane >= off) inc += t;
            }
            if (r < R) kst_s[r] = kept ? nkept + inc - sz : -1;
            const unsigned long long ne = __ballot(sz > 0);
            if (ne) last_r = r0 + 63 - __clzll((long long)ne);
            nkept += __shfl(inc, 63);
        }
        __syncthreads();
        add_centre = with_centre && nkept < N;
        if (R <= 64) {
            for (int r = 0; r < R; ++r) {
                const int ks = kst_s[r];
                if (ks < 0) continue;
                const int off = roff[r], n = roff[r + 1] - off;
                for (int j = lane; j < n; j += 64) rows[ks + j] = sorted_pts[off + j];
            }
        } else {
            for (int r = lane; r < R; r += 64) {
                const int ks = kst_s[r];
                if (ks < 0) continue;
                const int off = roff[r], n = roff[r + 1] - off;
                for (int j = 0; j < n; ++j) rows[ks + j] = sorted_pts[off + j];
            }
        }
        if (!add_centre && nkept > 0) padval = sorted_pts[roff[last_r + 1] - 1];   // padding: the centre if present, else the last kept point
    }
    const int nrows = nkept + (add_centre ? 1 : 0);
    const int npad = padded_rows(nrows);
    for (int i = nkept + lane; i < npad; i += 64) rows[i] = (uint16_t)padval;
    if (lane == 0) nrows_all[item] = nrows | (add_centre ? (1 << 16) : 0);
}

// ---- prefix coalitions straight from permutations (iq_pointnet_prefix_coalitions_wide): no keep rows ---------------------------
// Item o * (R + 1) + i keeps orders[o][0 .. i-1] with the set semantics of iq_prefix_keep_masks_wide: an entry outside [0, R) adds
// nothing, and neither does a region that an earlier entry of the same permutation named.  The "seen" set is kept as the position
// of every region's FIRST occurrence (atomicMin over the entries: the same table whatever the schedule), so all entries are
// classified at once: entry i counts iff first_s[ord[i]] == i.  A region therefore counts once and a row list never exceeds N.
static_assert(IQ_MAX_WIDE_REGIONS <= 4 * kThreads, "pn_rows_prefix_kernel: a thread scans four entries of a permutation");

__device__ __forceinline__ void prefix_first_seen(const int32_t* __restrict__ ord, int R, int* first_s) {
    for (int r = threadIdx.x; r < R; r += blockDim.x) first_s[r] = R;
    __syncthreads();
    for (int i = threadIdx.x; i < R; i += blockDim.x) {
        const int r = ord[i];
        if ((unsigned)r < (unsigned)R) atomicMin(&first_s[r], i);
    }
    __syncthreads();
}
__device__ __forceinline__ int prefix_entry_region(const int32_t* __restrict__ ord, int R, const int* first_s, int i) {
    const int r = ord[i];
    return ((unsigned)r < (unsigned)R && first_s[r] == i) ? r : -1;   // -1: the entry adds nothing
}

// One workgroup per permutation.  P = the points of the counting entries in permutation order (LDS), pos[i] = points after i
// entries (a scan over the R entry sizes); the row list of item i is P[0 : pos[i]], then the centre and the padding by the rules of
// pn_rows_wide_kernel.  A wave writes an item, eight entries (16 bytes) per lane: kRowCap and every padded length are multiples of 8.
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
static_assert(kRowCap % 8 == 0 && kMC % 8 == 0 && kMC96 % 8 == 0, "row lists are written 8 entries at a time");

__global__ __launch_bounds__(kThreads) void pn_rows_prefix_kernel(const uint16_t* __restrict__ sorted_all,
                                                                  const int32_t* __restrict__ roff_all,
                                                                  const int32_t* __restrict__ orders,
                                                                  const int32_t* __restrict__ cloud_of, uint16_t* __restrict__ rows_all,
                                                                  int32_t* __restrict__ nrows_all, int N, int R, int nclouds,
                                                                  int with_centre) {
    __shared__ __attribute__((aligned(16))) uint16_t P[kMaxN + 8];
    __shared__ int first_s[IQ_MAX_WIDE_REGIONS];
    __shared__ int src_s[IQ_MAX_WIDE_REGIONS];       // region of entry i, -1 = adds nothing
    __shared__ int pos_s[IQ_MAX_WIDE_REGIONS + 1];
    __shared__ int wsum_s[kThreads / 64];
    const int o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cloud = cloud_of ? cloud_of[o] : (nclouds == 1 ? 0 : o);
    const int32_t* ord = orders + (size_t)o * R;
    const int32_t* roff = roff_all + (size_t)cloud * (R + 1);
    const uint16_t* sorted_pts = sorted_all + (size_t)cloud * N;
    prefix_first_seen(ord, R, first_s);

    // exclusive scan of the entry sizes: four consecutive entries per thread, the wave, then the four waves
    int sz[4], tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = 4 * tid + k;
        int r = -1;
        if (i < R) src_s[i] = r = prefix_entry_region(ord, R, first_s, i);
        sz[k] = r >= 0 ? roff[r + 1] - roff[r] : 0;
        tot += sz[k];
    }
    int inc = tot;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) wsum_s[wave] = inc;
    __syncthreads();
    int run = inc - tot;
    for (int w = 0; w < wave; ++w) run += wsum_s[w];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = 4 * tid + k;
        if (i < R) {
            pos_s[i] = run;
            run += sz[k];
            if (i == R - 1) pos_s[R] = run;
        }
    }
    __syncthreads();

    // P: slot p belongs to the entry i with pos[i] <= p < pos[i+1] (binary search; entries that add nothing have pos[i] == pos[i+1])
    const int total = pos_s[R];   // <= N: every region counts once
    for (int p = tid; p < total; p += kThreads) {
        int lo = 0, hi = R - 1;   // the first entry whose end pos[i+1] exceeds p; pos[R] = total > p
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pos_s[mid + 1] > p) hi = mid; else lo = mid + 1;
        }
        P[p] = sorted_pts[roff[src_s[lo]] + p - pos_s[lo]];
    }
    __syncthreads();

    for (int i = wave; i <= R; i += kThreads / 64) {
        const int nkept = pos_s[i];
        const bool add_centre = with_centre && nkept < N;
        const int nrows = nkept + (add_centre ? 1 : 0);
        const unsigned short padval = (unsigned short)((add_centre || nkept == 0) ? N : P[nkept - 1]);   // the centre, else the last kept point
        const size_t item = (size_t)o * (R + 1) + i;
        uint16_t* rows = rows_all + item * kRowCap;
        const int npad = padded_rows(nrows);
        for (int j = lane * 8; j < npad; j += 64 * 8) {
            u16x8 v = {padval, padval, padval, padval, padval, padval, padval, padval};
            if (j < nkept) {      // j + 7 <= nkept + 6 < kMaxN + 8
                const u16x8 p8 = *reinterpret_cast<const u16x8*>(&P[j]);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = j + k < nkept ? p8[k] : padval;
            }
            *reinterpret_cast<u16x8*>(&rows[j]) = v;
        }
        if (lane == 0) nrows_all[item] = nrows | (add_centre ? (1 << 16) : 0);
    }
}

// ---- launch order: largest coalitions first (LPT), a counting sort on the chunk count ---------
constexpr int kBins = kMaxN / kMC + 2;

__global__ __launch_bounds__(kThreads) void pn_order_count_kernel(const int32_t* __restrict__ nrows_all,
                                                                  int32_t* __restrict__ bin_of, int32_t* __restrict__ hist,
                                                                  int B) {
    __shared__ int lh[kBins];   // per-workgroup histogram: one global atomic per bin and workgroup instead of one per item
    if (threadIdx.x < kBins) lh[threadIdx.x] = 0;
    __syncthreads();
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item < B) {
        const int rows = nrows_all[item] & 0xffff;
        const int bin = kBins - 1 - min(kBins - 1, (rows + kMC - 1) / kMC);  // bin 0 = most chunks
        bin_of[item] = bin;
        atomicAdd(&lh[bin], 1);
    }
    __syncthreads();
    if (threadIdx.x < kBins && lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

__global__ void pn_order_scan_kernel(int32_t* __restrict__ hist) {
    if (threadIdx.x == 0) {
        int run = 0;
        for (int b = 0; b < kBins; ++b) { const int c = hist[b]; hist[b] = run; run += c; }
    }
}

// position inside a bin: the workgroup reserves a range per bin with one global atomic, its items take consecutive slots
// (the order inside a bin is irrelevant: equal chunk counts)
__global__ __launch_bounds__(kThreads) void pn_order_scatter_kernel(const int32_t* __restrict__ bin_of,
                                                                    int32_t* __restrict__ cursor,
                                                                    int32_t* __restrict__ order, int B) {
    __shared__ int lh[kBins], base[kBins];
    if (threadIdx.x < kBins) lh[threadIdx.x] = 0;
    __syncthreads();
    const int item = blockIdx.x * blockDim.x + threadIdx.x;
    int bin = 0, pos = 0;
    if (item < B) {
        bin = bin_of[item];
        pos = atomicAdd(&lh[bin], 1);
    }
    __syncthreads();
    if (threadIdx.x < kBins && lh[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], lh[threadIdx.x]);
    __syncthreads();
    if (item < B) order[base[bin] + pos] = item;
}

// The four steps above in one launch for a batch that one workgroup covers (a pose of a sweep: 3 300 coalitions): the clear, the
// histogram and the scan stay in LDS, and an item keeps its position inside its bin in a register.  Above kOrderFusedMax items a
// single workgroup would take longer than the four launches' grids, so those stay.  pointnet.ORDER_FUSED_MAX (Python) repeats
// kOrderFusedMax for the tests that probe both sides of the bound: the two move together.
constexpr int kOrderThreads = 1024, kOrderPer = 4, kOrderFusedMax = kOrderThreads * kOrderPer;

__global__ __launch_bounds__(kOrderThreads) void pn_order_fused_kernel(const int32_t* __restrict__ nrows_all,
                                                                       int32_t* __restrict__ order, int B) {
    __shared__ int lh[kBins];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < kBins) lh[tid] = 0;
    __syncthreads();
    int bin[kOrderPer], pos[kOrderPer];
#pragma unroll
    for (int j = 0; j < kOrderPer; ++j) {
        const int item = tid + j * kOrderThreads;
        if (item < B) {
            const int rows = nrows_all[item] & 0xffff;
            bin[j] = kBins - 1 - min(kBins - 1, (rows + kMC - 1) / kMC);  // bin 0 = most chunks
            pos[j] = atomicAdd(&lh[bin[j]], 1);
        }
    }
    __syncthreads();
    if (tid < 64) {                                // exclusive scan, 64 bins at a time
        int carry = 0;
        for (int b0 = 0; b0 < kBins; b0 += 64) {
            const int b = b0 + lane, c = b < kBins ? lh[b] : 0;
            int inc = c;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int t = __shfl_up(inc, off);
                if (lane >= off) inc += t;
            }
            if (b < kBins) lh[b] = carry + inc - c;
            carry += __shfl(inc, 63);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kOrderPer; ++j) {
        const int item = tid + j * kOrderThreads;
        if (item < B) order[lh[bin[j]] + pos[j]] = item;
    }
}

// ---- repeated full and empty sets (one cloud per call): the first of each kind is computed, the others copy its chain output ----
constexpr int kDupRepOff = kBins;   // rep[2] lives in the padding behind the launch-order histogram: workspace sizes stay what they were
static_assert(iq::align_up((kBins + 2) * sizeof(int32_t), 256) == iq::align_up(kBins * sizeof(int32_t), 256), "room behind hist");

__global__ __launch_bounds__(kOrderThreads) void pn_dup_rep_kernel(const int32_t* __restrict__ nrows_all, int32_t* __restrict__ rep,
                                                                   int B, int N) {
    __shared__ int first[2];
    if (threadIdx.x < 2) first[threadIdx.x] = B;
    __syncthreads();
    for (int item = threadIdx.x; item < B; item += kOrderThreads) {
        const int kind = dup_kind(nrows_all[item], N);
        if (kind >= 0) atomicMin(&first[kind], item);
    }
    __syncthreads();
    if (threadIdx.x < 2) rep[threadIdx.x] = first[threadIdx.x];
}

// after a chain launch: row `item` of out (and of argrow, if any) = the row of the first item of its kind
__global__ __launch_bounds__(kThreads) void pn_dup_copy_kernel(const int32_t* __restrict__ nrows_all, const int32_t* __restrict__ rep,
                                                               float* __restrict__ out, int32_t* __restrict__ argrow, int N) {
    const int item = blockIdx.x;
    const int kind = dup_kind(nrows_all[item], N);
    if (kind < 0) return;
    const int src = rep[kind];
    if (src == item) return;
    static_assert(kFeat == 4 * kThreads, "one float4 per thread");
    reinterpret_cast<f32x4*>(out + (size_t)item * kFeat)[threadIdx.x] = reinterpret_cast<const f32x4*>(out + (size_t)src * kFeat)[threadIdx.x];
    if (argrow) {
        const int4 v = reinterpret_cast<const int4*>(argrow + (size_t)src * kFeat)[threadIdx.x];
        reinterpret_cast<int4*>(argrow + (size_t)item * kFeat)[threadIdx.x] = v;
    }
}

// ---- pooled input-STN feature of a coalition: max over kept regions (+ centre) -------------
__global__ __launch_bounds__(kThreads) void pn_stn_gather_kernel(const float* __restrict__ G,
                                                                 const int32_t* __restrict__ nrows_all,
                                                                 const uint64_t* __restrict__ keep,
                                                                 const int32_t* __restrict__ cloud_of,
                                                                 float* __restrict__ out, int R, int nclouds,
                                                                 int with_centre) {
    const int item = blockIdx.x;
    const int cloud = cloud_of ? cloud_of[item] : (nclouds == 1 ? 0 : item);
    const uint64_t full = R >= 64 ? ~0ull : ((1ull << R) - 1);
    const uint64_t k = (keep ? keep[item] : ~0ull) & full;
    const int per = R + with_centre;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(G) + (size_t)cloud * per * (kFeat / 4) + threadIdx.x;
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int r = 0; r < R; ++r) {
        if ((k >> r) & 1) {
            const f32x4 v = g4[(size_t)r * (kFeat / 4)];
            m[0] = fmaxf(m[0], v[0]); m[1] = fmaxf(m[1], v[1]); m[2] = fmaxf(m[2], v[2]); m[3] = fmaxf(m[3], v[3]);
        }
    }
    if (nrows_all[item] >> 16) {  // a centre row exists (something was masked)
        const f32x4 v = g4[(size_t)R * (kFeat / 4)];
        m[0] = fmaxf(m[0], v[0]); m[1] = fmaxf(m[1], v[1]); m[2] = fmaxf(m[2], v[2]); m[3] = fmaxf(m[3], v[3]);
    }
    reinterpret_cast<f32x4*>(out)[(size_t)item * (kFeat / 4) + threadIdx.x] = m;
}

// The same for a wide keep row (W words, in LDS once): the set bits in ascending order, four rows of G in flight per thread (a
// row read twice to fill a group of four never changes a max).  A coalition reads 4 KB per kept region: 4 MB at most at R = 1024,
// 2 MB on average over the prefix coalitions of a permutation.
__global__ __launch_bounds__(kThreads) void pn_stn_gather_wide_kernel(const float* __restrict__ G,
                                                                      const int32_t* __restrict__ nrows_all,
                                                                      const uint64_t* __restrict__ keep,
                                                                      const int32_t* __restrict__ cloud_of,
                                                                      float* __restrict__ out, int R, int W, int nclouds,
                                                                      int with_centre) {
    __shared__ uint64_t ks[kMaxW];
    const int item = blockIdx.x;
    const int cloud = cloud_of ? cloud_of[item] : (nclouds == 1 ? 0 : item);
    if ((int)threadIdx.x < W) {
        uint64_t k = keep ? keep[(size_t)item * W + threadIdx.x] : ~0ull;
        if ((int)threadIdx.x == W - 1 && (R & 63)) k &= (1ull << (R & 63)) - 1;   // bits at or above R are ignored
        ks[threadIdx.x] = k;
    }
    __syncthreads();
    const int per = R + with_centre;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(G) + (size_t)cloud * per * (kFeat / 4) + threadIdx.x;
    f32x4 m = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int w = 0; w < W; ++w) {
        const uint64_t kw = ks[w];
        uint64_t k = ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(kw >> 32)) << 32) |
                     (unsigned)__builtin_amdgcn_readfirstlane((int)kw);                      // the same for every lane
        while (k) {
            int r[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                r[q] = k ? w * 64 + __ffsll((long long)k) - 1 : r[0];
                k &= k - 1;
            }
            f32x4 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = g4[(size_t)r[q] * (kFeat / 4)];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                m[0] = fmaxf(m[0], v[q][0]); m[1] = fmaxf(m[1], v[q][1]); m[2] = fmaxf(m[2], v[q][2]); m[3] = fmaxf(m[3], v[q][3]);
            }
        }
    }
    if (nrows_all[item] >> 16) {  // a centre row exists (something was masked)
        const f32x4 v = g4[(size_t)R * (kFeat / 4)];
        m[0] = fmaxf(m[0], v[0]); m[1] = fmaxf(m[1], v[1]); m[2] = fmaxf(m[2], v[2]); m[3] = fmaxf(m[3], v[3]);
    }
    reinterpret_cast<f32x4*>(out)[(size_t)item * (kFeat / 4) + threadIdx.x] = m;
}

// The same for the prefix coalitions of a permutation: the pooled feature of item i is the running maximum of the rows of G along
// the permutation, R rows per permutation instead of R^2 / 2.  kFeat / 256 workgroups of one wave per permutation (a float4 of
// channels per lane), kPrefixRows rows of G in flight.  max is exact and order-independent, so the bits are the gather's.  The wave
// that owns channels 0 .. 255 also writes every item's cloud for the chain kernels (item_cloud, null for one cloud: they take a
// cloud per ITEM, this entry a cloud per permutation).
constexpr int kPrefixRows = 8;

__global__ __launch_bounds__(64) void pn_stn_prefix_kernel(const float* __restrict__ G, const int32_t* __restrict__ nrows_all,
                                                           const int32_t* __restrict__ orders,
                                                           const int32_t* __restrict__ cloud_of, float* __restrict__ out,
                                                           int32_t* __restrict__ item_cloud, int R, int nclouds, int with_centre) {
    __shared__ int first_s[IQ_MAX_WIDE_REGIONS];
    __shared__ int src_s[IQ_MAX_WIDE_REGIONS];
    __shared__ unsigned char flag_s[IQ_MAX_WIDE_REGIONS + 1];
    const int o = blockIdx.x, part = blockIdx.y, lane = threadIdx.x;
    const int cloud = cloud_of ? cloud_of[o] : (nclouds == 1 ? 0 : o);
    const int32_t* ord = orders + (size_t)o * R;
    const size_t item0 = (size_t)o * (R + 1);
    prefix_first_seen(ord, R, first_s);
    for (int i = lane; i < R; i += 64) src_s[i] = prefix_entry_region(ord, R, first_s, i);
    for (int i = lane; i <= R; i += 64) {
        flag_s[i] = (unsigned char)(nrows_all[item0 + i] >> 16);   // a centre row exists (something was masked)
        if (item_cloud && part == 0) item_cloud[item0 + i] = cloud;
    }
    __syncthreads();
    const int per = R + with_centre;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(G) + (size_t)cloud * per * (kFeat / 4) + part * 64 + lane;
    f32x4* o4 = reinterpret_cast<f32x4*>(out) + item0 * (kFeat / 4) + part * 64 + lane;
    const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const f32x4 c = with_centre ? g4[(size_t)R * (kFeat / 4)] : ninf;
    f32x4 m = ninf;
    for (int i0 = 0; i0 <= R; i0 += kPrefixRows) {
        f32x4 v[kPrefixRows];
#pragma unroll
        for (int q = 0; q < kPrefixRows; ++q) {
            const int i = i0 + q;
            const int r = __builtin_amdgcn_readfirstlane(i < R ? src_s[i] : -1);   // the same for every lane
            v[q] = r >= 0 ? g4[(size_t)r * (kFeat / 4)] : ninf;
        }
#pragma unroll
        for (int q = 0; q < kPrefixRows; ++q) {
            const int i = i0 + q;
            if (i > R) break;
            f32x4 w = m;
            if (flag_s[i]) { w[0] = fmaxf(w[0], c[0]); w[1] = fmaxf(w[1], c[1]); w[2] = fmaxf(w[2], c[2]); w[3] = fmaxf(w[3], c[3]); }
            o4[(size_t)i * (kFeat / 4)] = w;
            m[0] = fmaxf(m[0], v[q][0]); m[1] = fmaxf(m[1], v[q][1]); m[2] = fmaxf(m[2], v[q][2]); m[3] = fmaxf(m[3], v[q][3]);
        }
    }
}

// every item's 64 x 64 transform := one packed image (4096 floats), float4 per thread
__global__ __launch_bounds__(kThreads) void pn_fill_rows_kernel(float* __restrict__ out, const float* __restrict__ image, int B) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (size_t)B * 1024) return;
    reinterpret_cast<f32x4*>(out)[t] = reinterpret_cast<const f32x4*>(image)[t & 1023];
}

template <int MODE>
void launch_chain(const ChainArgs& a, hipStream_t st) {
    // twins kTwinChainL3Fp32 / kTwinChainL3Fp32NoTail16: layer 3 on the fp32 MFMA (round 3's kernel; A/B and tests)
    const bool fp32_l3 = iq::twin() == iq::kTwinChainL3Fp32 || iq::twin() == iq::kTwinChainL3Fp32NoTail16;
    const bool bf3 = a.w3_bf3 && a.w2_bf3 && !fp32_l3;
    if constexpr (MODE == kTrunk) {
        if (a.argrow) {
            if (bf3) hipLaunchKernelGGL((pn_chain_kernel<kTrunk, 3, true>), dim3(a.items), dim3(kThreads), 0, st, a);
            else     hipLaunchKernelGGL((pn_chain_kernel<kTrunk, 2, true>), dim3(a.items), dim3(kThreads), 0, st, a);
            return;
        }
    }
    if constexpr (MODE != kPrepool) {
        if (bf3) {   // the product path: 96-row chunks; twin kTwinChainL3Single: 64-row chunks, one n-tile per pass (its bitwise reference)
            if (a.l3_single) hipLaunchKernelGGL((pn_chain_kernel<MODE - kFstn + kFstn64, 3>), dim3(a.items), dim3(kThreads), 0, st, a);
            else             hipLaunchKernelGGL((pn_chain_kernel<MODE, 3>), dim3(a.items), dim3(kThreads), 0, st, a);
            return;
        }
    }
    hipLaunchKernelGGL((pn_chain_kernel<MODE, 2>), dim3(a.items), dim3(kThreads), 0, st, a);
}

}  // namespace

namespace {
using iq::launch_linear;   // (the heads pass fit_tiles = true: tile heights that fill the chip, iq_mfma.h)

struct Workspace {
    uint16_t* sorted_pts;
    int32_t* roff;
    uint16_t* rows_pre;  // (nclouds*(R+1), kRowCap)
    int32_t* nrows_pre;
    uint16_t* rows;      // (B, kRowCap)
    int32_t* nrows;      // (B)
    int32_t* order;    // (B) launch order
    int32_t* bin_of;   // (B)
    int32_t* hist;     // (kBins)
    float* G;
    float* gbuf;
    float* h1;
    float* h2;
    float* trans;
    float* tfp;
    uint16_t* fc3_bf3;   // fstn.fc3's weights as three bf16 terms, derived per call from the float32 image (pointnet_coalitions)
    size_t bytes;
};

// roff_entries: offsets per cloud - IQ_MAX_REGIONS + 1 for the narrow entry points (their layout since ABI 100), R + 1 for the wide one
Workspace carve(void* base, int B, int nclouds, int N, int R, int roff_entries = IQ_MAX_REGIONS + 1) {
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off = iq::align_up(off + bytes, 256);
        return reinterpret_cast<char*>(base) + o;
    };
    w.sorted_pts = reinterpret_cast<uint16_t*>(take((size_t)nclouds * N * sizeof(uint16_t)));
    w.roff = reinterpret_cast<int32_t*>(take((size_t)nclouds * roff_entries * sizeof(int32_t)));
    w.rows_pre = reinterpret_cast<uint16_t*>(take((size_t)nclouds * (R + 1) * kRowCap * sizeof(uint16_t)));
    w.nrows_pre = reinterpret_cast<int32_t*>(take((size_t)nclouds * (R + 1) * sizeof(int32_t)));
    w.rows = reinterpret_cast<uint16_t*>(take((size_t)B * kRowCap * sizeof(uint16_t)));
    w.nrows = reinterpret_cast<int32_t*>(take((size_t)B * sizeof(int32_t)));
    w.order = reinterpret_cast<int32_t*>(take((size_t)B * sizeof(int32_t)));
    w.bin_of = reinterpret_cast<int32_t*>(take((size_t)B * sizeof(int32_t)));
    w.hist = reinterpret_cast<int32_t*>(take((size_t)(kBins + 2) * sizeof(int32_t)));   // + pn_dup_rep_kernel's two
    w.G = reinterpret_cast<float*>(take((size_t)nclouds * (R + 1) * kFeat * sizeof(float)));
    w.gbuf = reinterpret_cast<float*>(take((size_t)B * kFeat * sizeof(float)));
    w.h1 = reinterpret_cast<float*>(take((size_t)B * 512 * sizeof(float)));
    w.h2 = reinterpret_cast<float*>(take((size_t)B * 256 * sizeof(float)));
    w.trans = reinterpret_cast<float*>(take((size_t)B * 9 * sizeof(float)));
    w.tfp = reinterpret_cast<float*>(take((size_t)B * 4096 * sizeof(float)));
    w.fc3_bf3 = reinterpret_cast<uint16_t*>(take(iq_packed_bf3_elems(4096, 256) * sizeof(uint16_t)));
    w.bytes = off;
    return w;
}

}  // namespace

extern "C" size_t iq_pointnet_workspace_bytes(int B, int nclouds, int N, int R) {
    if (B < 0 || nclouds < 0 || N < 0 || R < 0) return 0;
    return carve(nullptr, B, nclouds, N, R).bytes;
}

extern "C" double iq_pointnet_flops_per_coalition(int N) {
    // MACs per point: stn 3*64+64*128+128*1024, bmm 9, conv1 192, fstn 64*64+64*128+128*1024,
    // bmm 4096, conv2 8192, conv3 131072 = 426377; FC heads: stn 1024*512+512*256+256*9,
    // fstn ...+256*4096, cls ...+256*10
    const double per_point = 426377.0;
    const double fc = 3.0 * (1024.0 * 512 + 512.0 * 256) + 256.0 * (9 + 4096 + 10);
    return 2.0 * (per_point * N + fc);
}

extern "C" int iq_pointnet_coalitions(const iq_pointnet_weights* w, const float* clouds, const float* centers,
                                      const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of,
                                      float* logits, float* trans_feat_packed, void* workspace,
                                      size_t workspace_bytes, int B, int nclouds, int N, int R,
                                      int channel_first, iq_stream_t stream) {
    return iq_pointnet_coalitions_crt(w, clouds, centers, region_id, keep, cloud_of, logits, trans_feat_packed, nullptr, workspace,
                                      workspace_bytes, B, nclouds, N, R, channel_first, stream);
}

namespace {

// The forward behind iq_pointnet_coalitions[_crt] (wide_words = 0: keep (B) masks, R <= IQ_MAX_REGIONS), behind
// iq_pointnet_coalitions_wide (wide_words = W: keep (B,W) rows) and behind iq_pointnet_prefix_coalitions_wide (wide_words = W and
// orders (B / (R+1), R): item o*(R+1)+i keeps orders[o][:i], no keep rows; cloud_of then names a cloud per PERMUTATION).  Only the
// kernels that fill rows, nrows and gbuf differ; the chains, the launch order and the heads are the same launches.
int pointnet_coalitions(const iq_pointnet_weights* w, const float* clouds, const float* centers, const int32_t* region_id,
                        const uint64_t* keep, int wide_words, const int32_t* orders, const int32_t* cloud_of, float* logits,
                        float* trans_feat_packed, int32_t* crt_points, void* workspace, size_t workspace_bytes, int B, int nclouds,
                        int N, int R, int channel_first, iq_stream_t stream) {
    const char* who = orders ? "iq_pointnet_prefix_coalitions_wide"                           // the entry point a message names
                             : wide_words ? "iq_pointnet_coalitions_wide" : "iq_pointnet_coalitions";
    IQ_REQUIRE(B >= 0 && nclouds >= 1, "%s: B=%d nclouds=%d", who, B, nclouds);
    IQ_REQUIRE(w && clouds && region_id && (logits || B == 0), "%s: null pointer", who);
    IQ_REQUIRE(N >= 1 && N <= kMaxN, "%s: N=%d not in [1,%d]", who, N, kMaxN);
    const int max_regions = wide_words ? IQ_MAX_WIDE_REGIONS : IQ_MAX_REGIONS;
    IQ_REQUIRE(R >= 1 && R <= max_regions, "%s: R=%d not in [1,%d]", who, R, max_regions);
    const int groups = orders ? B / (R + 1) : B;   // what cloud_of names a cloud for: a permutation, else a coalition
    IQ_REQUIRE(cloud_of || nclouds == 1 || nclouds == groups, "%s: cloud_of required when 1 < nclouds != %s", who, orders ? "S" : "B");
    const int with_centre = centers ? 1 : 0;  // no centre = dense mode (nothing is ever masked)
    IQ_REQUIRE(centers || !(keep || orders), "%s: %s need centers", who, orders ? "prefix coalitions" : "keep masks");
    if (B == 0) return IQ_OK;
    const size_t need = wide_words ? iq_pointnet_wide_workspace_bytes(B, nclouds, N, R) : iq_pointnet_workspace_bytes(B, nclouds, N, R);
    if (!workspace || workspace_bytes < need)
        return iq::fail(IQ_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    Workspace ws = wide_words ? carve(workspace, B, nclouds, N, R, R + 1) : carve(workspace, B, nclouds, N, R);
    hipStream_t st = iq::as_stream(stream);
    int rc;
    iq::ProfileSpan call_span(iq::kSlotCall, st);

    const int pre_items = nclouds * (R + with_centre);
    // the chain kernels take a cloud per item: the prefix route writes one (pn_stn_prefix_kernel) where the launch order kept its
    // bins, which nothing reads once the order is scattered
    const int32_t* item_cloud = orders ? (nclouds > 1 ? ws.bin_of : nullptr) : cloud_of;
    if (wide_words) {
        hipLaunchKernelGGL(pn_prepare_wide_kernel, dim3(nclouds), dim3(kThreads), 0, st, region_id, ws.sorted_pts, ws.roff, N, R);
        if ((rc = iq::check_launch("pn_prepare_wide_kernel"))) return rc;
        hipLaunchKernelGGL(pn_rows_wide_kernel, dim3(pre_items), dim3(64), 0, st, ws.sorted_pts, ws.roff, nullptr, nullptr,
                           ws.rows_pre, ws.nrows_pre, N, R, wide_words, nclouds, with_centre, 1);
        if ((rc = iq::check_launch("pn_rows_wide_kernel"))) return rc;
        if (orders) {
            hipLaunchKernelGGL(pn_rows_prefix_kernel, dim3(groups), dim3(kThreads), 0, st, ws.sorted_pts, ws.roff, orders, cloud_of,
                               ws.rows, ws.nrows, N, R, nclouds, with_centre);
            if ((rc = iq::check_launch("pn_rows_prefix_kernel"))) return rc;
        } else {
            hipLaunchKernelGGL(pn_rows_wide_kernel, dim3(B), dim3(64), 0, st, ws.sorted_pts, ws.roff, keep, cloud_of, ws.rows,
                               ws.nrows, N, R, wide_words, nclouds, with_centre, 0);
            if ((rc = iq::check_launch("pn_rows_wide_kernel"))) return rc;
        }
    } else {
        hipLaunchKernelGGL(pn_prepare_kernel, dim3(nclouds), dim3(kThreads), 0, st, region_id, ws.sorted_pts, ws.roff, N, R);
        if ((rc = iq::check_launch("pn_prepare_kernel"))) return rc;
        hipLaunchKernelGGL(pn_rows_kernel, dim3(pre_items), dim3(64), 0, st, ws.sorted_pts, ws.roff, nullptr, nullptr,
                           ws.rows_pre, ws.nrows_pre, N, R, nclouds, with_centre, 1);
        hipLaunchKernelGGL(pn_rows_kernel, dim3(B), dim3(64), 0, st, ws.sorted_pts, ws.roff, keep, cloud_of, ws.rows,
                           ws.nrows, N, R, nclouds, with_centre, 0);
        if ((rc = iq::check_launch("pn_rows_kernel"))) return rc;
    }
    // launch order of the coalition chains: most rows first, so the grid drains evenly
    if (B <= kOrderFusedMax) {
        hipLaunchKernelGGL(pn_order_fused_kernel, dim3(1), dim3(kOrderThreads), 0, st, ws.nrows, ws.order, B);
    } else {
        if (hipMemsetAsync(ws.hist, 0, kBins * sizeof(int32_t), st) != hipSuccess)
            return iq::fail(IQ_ELAUNCH, "%s: memset failed", who);
        hipLaunchKernelGGL(pn_order_count_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ws.nrows,
                           ws.bin_of, ws.hist, B);
        hipLaunchKernelGGL(pn_order_scan_kernel, dim3(1), dim3(64), 0, st, ws.hist);
        hipLaunchKernelGGL(pn_order_scatter_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                           ws.bin_of, ws.hist, ws.order, B);
    }
    if ((rc = iq::check_launch("pn_order kernels"))) return rc;
    // repeated full / empty sets: one cloud and keep masks in table order only (a prefix route's row lists follow its permutations)
    const int32_t* dup_rep = nullptr;
    if (nclouds == 1 && !wide_words && B > 1 && iq::twin() != iq::kTwinChainNoDedup) {
        hipLaunchKernelGGL(pn_dup_rep_kernel, dim3(1), dim3(kOrderThreads), 0, st, ws.nrows, ws.hist + kDupRepOff, B, N);
        if ((rc = iq::check_launch("pn_dup_rep_kernel"))) return rc;
        dup_rep = ws.hist + kDupRepOff;
    }

    ChainArgs a{};
    a.clouds = clouds;
    if (channel_first) { a.ps = 1; a.cs = N; } else { a.ps = 3; a.cs = 1; }
    a.cl = 3 * N;
    a.centers = centers;
    a.rows = ws.rows_pre;
    a.nrows = ws.nrows_pre;
    a.item_order = nullptr;
    a.N = N; a.R = R; a.nclouds = nclouds; a.with_centre = with_centre;
    a.tail16 = iq::twin() != iq::kTwinChainL3Fp32NoTail16;
    a.l3_single = iq::twin() == iq::kTwinChainL3Single;


    // 1. input-STN chain, pre-pooled per (cloud, region) [+ centre]
    a.cloud_of = nullptr; a.trans = nullptr;
    a.w_in = w->stn_in;
    a.w1 = nullptr; a.b1 = nullptr;
    a.w2 = w->stn_c2.w; a.b2 = w->stn_c2.b;
    a.w3 = w->stn_c3.w; a.b3 = w->stn_c3.b;
    a.out = ws.G;
    a.items = pre_items;
    {
        iq::ProfileSpan span(iq::kSlotPrepool, st);
        launch_chain<kPrepool>(a, st);
    }
    if ((rc = iq::check_launch("pn_chain_kernel<prepool>"))) return rc;

    if (orders)
        hipLaunchKernelGGL(pn_stn_prefix_kernel, dim3(groups, kFeat / 256), dim3(64), 0, st, ws.G, ws.nrows, orders, cloud_of, ws.gbuf,
                           item_cloud ? ws.bin_of : nullptr, R, nclouds, with_centre);
    else if (wide_words)
        hipLaunchKernelGGL(pn_stn_gather_wide_kernel, dim3(B), dim3(kThreads), 0, st, ws.G, ws.nrows, keep, cloud_of, ws.gbuf,
                           R, wide_words, nclouds, with_centre);
    else
        hipLaunchKernelGGL(pn_stn_gather_kernel, dim3(B), dim3(kThreads), 0, st, ws.G, ws.nrows, keep, cloud_of, ws.gbuf,
                           R, nclouds, with_centre);
    if ((rc = iq::check_launch(orders ? "pn_stn_prefix_kernel" : wide_words ? "pn_stn_gather_wide_kernel" : "pn_stn_gather_kernel")))
        return rc;
    if ((rc = launch_linear(ws.gbuf, kFeat, w->stn_fc1, ws.h1, 512, B, 1, st, nullptr, nullptr, 0, true))) return rc;
    if ((rc = launch_linear(ws.h1, 512, w->stn_fc2, ws.h2, 256, B, 1, st, nullptr, nullptr, 0, true))) return rc;
    if ((rc = launch_linear(ws.h2, 256, w->stn_fc3, ws.trans, 9, B, 0, st, nullptr, nullptr, 0, true))) return rc;

    // 2. feature-STN chain over each coalition's distinct points
    a.cloud_of = item_cloud; a.trans = ws.trans;
    a.rows = ws.rows; a.nrows = ws.nrows;
    a.item_order = ws.order;
    a.dup_rep = dup_rep;
    a.w_in = w->feat_in;
    a.items = B;
    a.out = ws.gbuf;
    float* tfp = trans_feat_packed ? trans_feat_packed : ws.tfp;
    if (w->fstn_c1.w) {
        a.w1 = w->fstn_c1.w; a.b1 = w->fstn_c1.b;
        a.w2 = w->fstn_c2.w; a.b2 = w->fstn_c2.b;
        a.w3 = w->fstn_c3.w; a.b3 = w->fstn_c3.b; a.w3_bf3 = reinterpret_cast<const unsigned short*>(w->fstn_c3_bf3);
        a.w2_bf3 = reinterpret_cast<const unsigned short*>(w->fstn_c2_bf3);
        {
            iq::ProfileSpan span(iq::kSlotFstn, st);
            launch_chain<kFstn>(a, st);
        }
        if (dup_rep) hipLaunchKernelGGL(pn_dup_copy_kernel, dim3(B), dim3(kThreads), 0, st, ws.nrows, dup_rep, ws.gbuf, nullptr, N);
        if ((rc = iq::check_launch("pn_chain_kernel<fstn>"))) return rc;
        if ((rc = launch_linear(ws.gbuf, kFeat, w->fstn_fc1, ws.h1, 512, B, 1, st, nullptr, nullptr, 0, true))) return rc;
        if ((rc = launch_linear(ws.h1, 512, w->fstn_fc2, ws.h2, 256, B, 1, st, nullptr, nullptr, 0, true))) return rc;
        // fstn.fc3 (256 -> 4096, 70 % of the heads' FLOP) on the bf16 matrix pipe like the other wide layers.  The descriptor brings
        // no bf16x3 image of it (its rows are permuted by iq_pack_fstn_fc3; the packed weight set is what it has always been), so the
        // image is split off the float32 one here, per call: 1 M weights, a few microseconds, and nothing to go stale when a
        // caller reuses a pointer for other weights.  Twin kTwinDenseFp32: no split, the fp32-MFMA kernel.
        iq_dense_layer fc3 = w->fstn_fc3;
        IQ_REQUIRE(fc3.cin == 256 && fc3.cout == 4096, "%s: fstn_fc3 is %d -> %d, not 256 -> 4096", who, fc3.cin, fc3.cout);
        if (!fc3.w_bf3 && iq::twin() != iq::kTwinDenseFp32) {
            if ((rc = iq::launch_split_bf3(fc3.w, ws.fc3_bf3, 4096, 256, st))) return rc;
            fc3.w_bf3 = ws.fc3_bf3;
        }
        if ((rc = launch_linear(ws.h2, 256, fc3, tfp, 4096, B, 0, st, nullptr, nullptr, 0, true))) return rc;
    } else {
        // feature_transform = False (models/pointnet.py:62-63,72-78): no feature STN.  The trunk multiplies by the packed
        // IDENTITY instead (fstn_fc3.b = iq_pack_fstn_fc3 of a zero layer): sum_k f[k] I[k][n] = f[n] + zeros, exact.
        IQ_REQUIRE(w->fstn_fc3.b, "%s: without a feature STN, fstn_fc3.b must hold the packed identity", who);
        hipLaunchKernelGGL(pn_fill_rows_kernel, dim3((unsigned)(((size_t)B * 1024 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           tfp, w->fstn_fc3.b, B);
        if ((rc = iq::check_launch("pn_fill_rows_kernel"))) return rc;
    }

    // 3. trunk chain
    a.argrow = crt_points;
    a.w1 = tfp; a.b1 = nullptr;
    a.w2 = w->feat_c2.w; a.b2 = w->feat_c2.b;
    a.w3 = w->feat_c3.w; a.b3 = w->feat_c3.b; a.w3_bf3 = reinterpret_cast<const unsigned short*>(w->feat_c3_bf3);
    a.w2_bf3 = reinterpret_cast<const unsigned short*>(w->feat_c2_bf3);
    {
        iq::ProfileSpan span(iq::kSlotTrunk, st);
        launch_chain<kTrunk>(a, st);
    }
    if (dup_rep) hipLaunchKernelGGL(pn_dup_copy_kernel, dim3(B), dim3(kThreads), 0, st, ws.nrows, dup_rep, ws.gbuf, crt_points, N);
    if ((rc = iq::check_launch("pn_chain_kernel<trunk>"))) return rc;
    if ((rc = launch_linear(ws.gbuf, kFeat, w->cls_fc1, ws.h1, 512, B, 1, st, nullptr, nullptr, 0, true))) return rc;
    if ((rc = launch_linear(ws.h1, 512, w->cls_fc2, ws.h2, 256, B, 1, st, nullptr, nullptr, 0, true))) return rc;
    if ((rc = launch_linear(ws.h2, 256, w->cls_fc3, logits, w->cls_fc3.cout, B, 0, st, nullptr, nullptr, 0, true))) return rc;
    return IQ_OK;
}

}  // namespace

extern "C" int iq_pointnet_coalitions_crt(const iq_pointnet_weights* w, const float* clouds, const float* centers,
                                          const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of,
                                          float* logits, float* trans_feat_packed, int32_t* crt_points, void* workspace,
                                          size_t workspace_bytes, int B, int nclouds, int N, int R,
                                          int channel_first, iq_stream_t stream) {
    return pointnet_coalitions(w, clouds, centers, region_id, keep, 0, nullptr, cloud_of, logits, trans_feat_packed, crt_points, workspace,
                               workspace_bytes, B, nclouds, N, R, channel_first, stream);
}

extern "C" size_t iq_pointnet_wide_workspace_bytes(int B, int nclouds, int N, int R) {
    if (B < 0 || nclouds < 0 || N < 0 || R < 0) return 0;
    return carve(nullptr, B, nclouds, N, R, R + 1).bytes;
}

extern "C" int iq_pointnet_coalitions_wide(const iq_pointnet_weights* w, const float* clouds, const float* centers,
                                           const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of,
                                           float* logits, float* trans_feat_packed, void* workspace, size_t workspace_bytes,
                                           int B, int nclouds, int N, int R, int channel_first, iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_pointnet_coalitions_wide: R=%d not in [1,%d]", R, IQ_MAX_WIDE_REGIONS);
    return pointnet_coalitions(w, clouds, centers, region_id, keep, (R + 63) / 64, nullptr, cloud_of, logits, trans_feat_packed,
                               nullptr, workspace, workspace_bytes, B, nclouds, N, R, channel_first, stream);
}

extern "C" int iq_pointnet_prefix_coalitions_wide(const iq_pointnet_weights* w, const float* clouds, const float* centers,
                                                  const int32_t* region_id, const int32_t* orders, const int32_t* cloud_of,
                                                  float* logits, float* trans_feat_packed, void* workspace, size_t workspace_bytes,
                                                  int S, int nclouds, int N, int R, iq_stream_t stream) {
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_WIDE_REGIONS, "iq_pointnet_prefix_coalitions_wide: R=%d not in [1,%d]", R, IQ_MAX_WIDE_REGIONS);
    IQ_REQUIRE(S >= 0 && S <= 0x7fffffff / (R + 1), "iq_pointnet_prefix_coalitions_wide: S=%d (R=%d)", S, R);
    IQ_REQUIRE(centers && (orders || S == 0), "iq_pointnet_prefix_coalitions_wide: null pointer");
    return pointnet_coalitions(w, clouds, centers, region_id, nullptr, (R + 63) / 64, orders, cloud_of, logits, trans_feat_packed,
                               nullptr, workspace, workspace_bytes, S * (R + 1), nclouds, N, R, 0, stream);
}

// ---- host-side packing of the feature-STN output layer (generic packing: iq_linear.hip) ------------
extern "C" int iq_pack_fstn_fc3(const float* w, const float* b, float* out_w, float* out_b, int32_t* perm) {
    IQ_REQUIRE(w && b && out_w && out_b, "iq_pack_fstn_fc3: null pointer");
    // Output element e of the layer must be element e of the packed B image of trans_feat for the
    // product f1 @ trans_feat (models/pointnet.py:74-76): B[k][n] = trans_feat[k][n], i.e. source
    // row k*64 + n of fc3, at e = ((nt*8 + kb)*64 + lane)*4 + j.
    float* tmp = new float[4096 * 256];
    for (int nt = 0; nt < 2; ++nt)
        for (int kb = 0; kb < 8; ++kb)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 4; ++j) {
                    const int n = nt * 32 + (lane & 31), k = 8 * kb + 4 * (lane >> 5) + j;
                    const int e = ((nt * 8 + kb) * 64 + lane) * 4 + j;
                    const int src = k * 64 + n;
                    for (int c = 0; c < 256; ++c) tmp[(size_t)e * 256 + c] = w[(size_t)src * 256 + c];
                    out_b[e] = b[src] + (k == n ? 1.f : 0.f);
                    if (perm) perm[e] = src;
                }
    const int rc = iq_pack_weight(tmp, out_w, 4096, 256);
    delete[] tmp;
    return rc;
}
