// bf16x3 building blocks (gfx950, v_mfma_f32_32x32x16_bf16; the 16x16x32 forms at the end are the PointNet chain kernel's layers 1-3):
// float32 GEMMs on the bf16 matrix pipe, float32-exact.
// A float32 is three bf16 terms, x = h + m + l (round to nearest, residuals exact); a product is the six largest of the nine
// term products, each exact, accumulated in float32 (small terms first).  See DESIGN.md 5a and iq_pack_weight_bf3 (iq_linear.hip)
// for the weight image: fragment (term, n-tile, k-step of 16) = 1 KiB at ((term * NT + n-tile) * KS + k-step) KiB, lane l at l * 16.
#pragma once
#include "iq_mfma.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

struct B3 { bf16x8 h, m, l; };

// Two float32 -> two bf16 (round to nearest even) in one dword, and back.
__device__ __forceinline__ unsigned bf16_pair(float lo, float hi) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
__device__ __forceinline__ float bf16_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
__device__ __forceinline__ float bf16_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xffff0000u); }

// fragment at byte offset `off` of the image's first term; the other two terms lie term_stride bytes apart
__device__ __forceinline__ B3 b3_load_at(const __amdgpu_buffer_rsrc_t& rs, int voff, int off, int term_stride) {
    return B3{__builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, off, 0)),
              __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, off + term_stride, 0)),
              __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, off + 2 * term_stride, 0))};
}

// A fragment of k-step ks from three bf16 planes in LDS: abase = plane 0 + (first row of the m-tile + (lane & 31)) * ROWB +
// 16 * (lane >> 5); rows of ROWB bytes, ROWB / 4 = 4 (mod 8) dwords for conflict-free ds_read_b128
template <int PLANEB>
__device__ __forceinline__ void a3_load(bf16x8 (&a)[3], const unsigned char* abase, int ks) {
#pragma unroll
    for (int e = 0; e < 3; ++e) a[e] = *reinterpret_cast<const bf16x8*>(abase + e * PLANEB + ks * 32);
}

__device__ __forceinline__ f32x16 mfma_bf3(const bf16x8 (&a)[3], const B3& b, f32x16 acc) {   // six products, small terms first
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b.l, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b.h, acc, 0, 0, 0);
    return acc;
}

// four consecutive channels of one row -> the three planes (8 bytes each); dst = plane 0 + row * ROWB + channel * 2
template <int PLANEB>
__device__ __forceinline__ void row4_to_planes(unsigned char* dst, f32x4 v) {
    const unsigned h0 = bf16_pair(v[0], v[1]), h1 = bf16_pair(v[2], v[3]);
    const float r0 = v[0] - bf16_lo(h0), r1 = v[1] - bf16_hi(h0), r2 = v[2] - bf16_lo(h1), r3 = v[3] - bf16_hi(h1);
    const unsigned m0 = bf16_pair(r0, r1), m1 = bf16_pair(r2, r3);
    *reinterpret_cast<u32x2*>(dst) = u32x2{h0, h1};
    *reinterpret_cast<u32x2*>(dst + PLANEB) = u32x2{m0, m1};
    *reinterpret_cast<u32x2*>(dst + 2 * PLANEB) =
        u32x2{bf16_pair(r0 - bf16_lo(m0), r1 - bf16_hi(m0)), bf16_pair(r2 - bf16_lo(m1), r3 - bf16_hi(m1))};
}

// four float32 values -> their three bf16 terms, packed two per dword (element 2 p in the low half)
__device__ __forceinline__ void split4(f32x4 v, u32x2& h, u32x2& m, u32x2& l) {
    const unsigned h0 = bf16_pair(v[0], v[1]), h1 = bf16_pair(v[2], v[3]);
    const float r0 = v[0] - bf16_lo(h0), r1 = v[1] - bf16_hi(h0), r2 = v[2] - bf16_lo(h1), r3 = v[3] - bf16_hi(h1);
    const unsigned m0 = bf16_pair(r0, r1), m1 = bf16_pair(r2, r3);
    h = u32x2{h0, h1};
    m = u32x2{m0, m1};
    l = u32x2{bf16_pair(r0 - bf16_lo(m0), r1 - bf16_hi(m0)), bf16_pair(r2 - bf16_lo(m1), r3 - bf16_hi(m1))};
}

// The TRANSPOSED C tile of a layer whose output goes back to LDS as an activation image (round 5): with the weight fragment as the
// A operand and the activation fragment as B - the same two fragments, swapped - lane (row = lane & 31 of the m-tile, half) holds its
// row's channels 8 g + 4 half + 0..3 in registers 4 g .. 4 g + 3: four consecutive channels per register quad, so the three bf16
// planes take whole 8-byte stores and the two-lane DPP trade of the untransposed tile (4 VALU per value pair) is not needed.
// `tile`: plane 0, first row of the m-tile, first channel of the n-tile; value(r): register r after bias / activation, where
// register r is channel c_row_i(r) + 4 * (lane >> 5) of the n-tile.
template <int ROWB, int PLANEB, typename F>
__device__ __forceinline__ void ct_tile_to_planes(unsigned char* tile, int lane, F value) {
    unsigned char* d = tile + (lane & 31) * ROWB + 8 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        u32x2 h, m, l;
        split4(f32x4{value(4 * g), value(4 * g + 1), value(4 * g + 2), value(4 * g + 3)}, h, m, l);
        unsigned char* o = d + g * 16;
        *reinterpret_cast<u32x2*>(o) = h;
        *reinterpret_cast<u32x2*>(o + PLANEB) = m;
        *reinterpret_cast<u32x2*>(o + 2 * PLANEB) = l;
    }
}

// one tile, transposed: the six products of mfma_bf3 with the operands swapped (weights = A operand)
__device__ __forceinline__ f32x16 mfma_bf3_tr(const B3& w, const bf16x8 (&x)[3], f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.h, x[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.l, x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.m, x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.h, x[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.m, x[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.h, x[0], acc, 0, 0, 0);
    return acc;
}

// transposed six-product k-step over MT m-tiles and ONE n-tile: the weight fragment as the A operand, the activation terms as B;
// term-major over the tiles (a dependent MFMA is MT instructions away), small terms first, the same products in the same order
// as mfma_bf3_block<MT, 1>
template <int TW, int TX, int MT>
__device__ __forceinline__ void mfma_term_block_tr(const B3& w, const bf16x8 (&x)[MT][3], f32x16 (&acc)[MT][1]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
        acc[i][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(TW == 0 ? w.h : (TW == 1 ? w.m : w.l), x[i][TX], acc[i][0], 0, 0, 0);
}
template <int MT>
__device__ __forceinline__ void mfma_bf3_block_tr(const bf16x8 (&x)[MT][3], const B3& w, f32x16 (&acc)[MT][1]) {
    mfma_term_block_tr<0, 2, MT>(w, x, acc);   // (activation l) x (weight h)
    mfma_term_block_tr<2, 0, MT>(w, x, acc);   // (activation h) x (weight l)
    mfma_term_block_tr<1, 1, MT>(w, x, acc);
    mfma_term_block_tr<0, 1, MT>(w, x, acc);   // (activation m) x (weight h)
    mfma_term_block_tr<1, 0, MT>(w, x, acc);   // (activation h) x (weight m)
    mfma_term_block_tr<0, 0, MT>(w, x, acc);
}

// MT x NT tiles of one k-step: six products per tile, the tiles' accumulation chains interleaved (a dependent MFMA is MT * NT
// instructions away), small terms first
template <int TA, int TB>
__device__ __forceinline__ f32x16 mfma_term(const bf16x8 (&a)[3], const B3& b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[TA], TB == 0 ? b.h : (TB == 1 ? b.m : b.l), c, 0, 0, 0);
}
template <int TA, int TB, int MT, int NT>
__device__ __forceinline__ void mfma_term_block(const bf16x8 (&a)[MT][3], const B3 (&b)[NT], f32x16 (&acc)[MT][NT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = mfma_term<TA, TB>(a[i], b[j], acc[i][j]);
}
template <int MT, int NT>
__device__ __forceinline__ void mfma_bf3_block(const bf16x8 (&a)[MT][3], const B3 (&b)[NT], f32x16 (&acc)[MT][NT]) {
    mfma_term_block<2, 0, MT, NT>(a, b, acc);
    mfma_term_block<0, 2, MT, NT>(a, b, acc);
    mfma_term_block<1, 1, MT, NT>(a, b, acc);
    mfma_term_block<1, 0, MT, NT>(a, b, acc);
    mfma_term_block<0, 1, MT, NT>(a, b, acc);
    mfma_term_block<0, 0, MT, NT>(a, b, acc);
}

// ---- v_mfma_f32_16x16x32_bf16 forms (PointNet chain kernel, layers 1-3) ---------------------------------------------------
// Operands (lane l: c = l & 15, kq = l >> 4): A = row c, channels 8 kq .. 8 kq + 7 of the 32-channel k-step; B = column c, the same
// channels; C = rows 4 kq + i (register i < 4) of column c.
//
// B comes out of the SAME iq_pack_weight_bf3 image as the 32x32x16 fragments: the 16 columns 16 hf .. 16 hf + 15 (hf = 0, 1) of a 32-column
// n-tile and the 32 channels of k-step t are, inside the adjacent 1 KiB blocks of the 16-channel k-steps 2 t and 2 t + 1, the bytes
// 1024 (kq >> 1) + 512 (kq & 1) + 256 hf + 16 c (four whole 256-byte runs per wave load).  b16_lane_off is the per-lane part.
__device__ __forceinline__ int b16_lane_off(int lane) {
    const int c = lane & 15, kq = lane >> 4;
    return 1024 * (kq >> 1) + 512 * (kq & 1) + 16 * c;
}

// The activation operand comes from three bf16 planes in LDS with UNPADDED rows (ROWB = 256 bytes: 128 channels, 128: 64 channels)
// whose 16-byte pieces are stored XOR-swizzled by the row: piece p of row r lies at ROWB r + 16 (p ^ swz(r)), swz(r) = r & 15
// (256-byte rows) or (r >> 1) & 7 (128-byte rows: two rows share a 256-byte bank line).  The 16x16x32 read (row c, piece 4 t + kq)
// is then conflict-free: a ds_read_b128 lane group holds rows {0-3, 12-15} of one kq and rows {4-11} of the next, the XOR maps both
// sets onto disjoint sixteen-byte bank groups (with padded rows that pattern is 2-way conflicted).  The planes' only writers are
// stage 0b (act0: stage0b_planes, iq_pointnet_chain.h) and the epilogues of layers 1 and 2 (c16_tile_to_planes_swz).  a16_lane_off: the per-lane byte offset of k-step
// 0; k-step t is that offset ^ (64 t).
template <int ROWB>
__device__ __forceinline__ int swz_of_row(int row) {
    static_assert(ROWB == 256 || ROWB == 128, "swizzled planes have 256- or 128-byte rows");
    return ROWB == 256 ? (row & 15) : ((row >> 1) & 7);
}
template <int ROWB>
__device__ __forceinline__ int a16_lane_off(int lane) {
    const int r = lane & 15, kq = lane >> 4;
    return r * ROWB + 16 * (kq ^ swz_of_row<ROWB>(r));
}
// fragment of m-tile mi (16 rows) and k-step t (32 channels); plane0 = row 0 of the tile range (a multiple of 16 rows)
template <int ROWB, int PLANEB>
__device__ __forceinline__ void a16_load(bf16x8 (&a)[3], const unsigned char* plane0, int lane_off, int mi, int t) {
#pragma unroll
    for (int e = 0; e < 3; ++e)
        a[e] = *reinterpret_cast<const bf16x8*>(plane0 + (lane_off ^ (64 * t)) + e * PLANEB + mi * 16 * ROWB);
}

// ct_tile_to_planes into a swizzled image: `row` = the lane's row of the chunk (first row of the m-tile + (lane & 31)), piece0 =
// first channel of the n-tile / 8; the lane's register quad g holds channels 8 g + 4 (lane >> 5) + 0..3 = one half of piece piece0 + g
template <int ROWB, int PLANEB, typename F>
__device__ __forceinline__ void ct_tile_to_planes_swz(unsigned char* plane0, int row, int piece0, int lane, F value) {
    unsigned char* d = plane0 + row * ROWB + 8 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        u32x2 h, m, l;
        split4(f32x4{value(4 * g), value(4 * g + 1), value(4 * g + 2), value(4 * g + 3)}, h, m, l);
        unsigned char* o = d + 16 * ((piece0 + g) ^ swz_of_row<ROWB>(row));
        *reinterpret_cast<u32x2*>(o) = h;
        *reinterpret_cast<u32x2*>(o + PLANEB) = m;
        *reinterpret_cast<u32x2*>(o + 2 * PLANEB) = l;
    }
}
// the TRANSPOSED 16x16x32 C tile (weights as the A operand): lane (point c = lane & 15, kq) holds channels 4 kq + 0..3 of the
// 16-channel tile = one half of piece piece0 + (kq >> 1); `row` = the lane's row of the chunk, v = the four values after bias / activation
template <int ROWB, int PLANEB>
__device__ __forceinline__ void c16_tile_to_planes_swz(unsigned char* plane0, int row, int piece0, int lane, f32x4 v) {
    const int kq = lane >> 4;
    unsigned char* o = plane0 + row * ROWB + 16 * ((piece0 + (kq >> 1)) ^ swz_of_row<ROWB>(row)) + 8 * (kq & 1);
    u32x2 h, m, l;
    split4(v, h, m, l);
    *reinterpret_cast<u32x2*>(o) = h;
    *reinterpret_cast<u32x2*>(o + PLANEB) = m;
    *reinterpret_cast<u32x2*>(o + 2 * PLANEB) = l;
}

// A 16x16x32 weight fragment split in registers (PointNet chain kernel, layer 1): the lane's eight consecutive float32 k values
// (two float4s of a 32x32x2 fragment image, iq_mfma.h) -> their three bf16 terms
__device__ __forceinline__ B3 b3_split8(f32x4 lo, f32x4 hi) {
    u32x2 h0, m0, l0, h1, m1, l1;
    split4(lo, h0, m0, l0);
    split4(hi, h1, m1, l1);
    return B3{__builtin_bit_cast(bf16x8, u32x4{h0[0], h0[1], h1[0], h1[1]}), __builtin_bit_cast(bf16x8, u32x4{m0[0], m0[1], m1[0], m1[1]}),
              __builtin_bit_cast(bf16x8, u32x4{l0[0], l0[1], l1[0], l1[1]})};
}

// MT m-tiles x ONE 16-column n-tile of one 32-channel k-step: the six products of mfma_bf3 in the same order (small terms first),
// term-major over the m-tiles (a dependent MFMA is MT instructions away)
template <int TA, int TB, int MT>
__device__ __forceinline__ void mfma16_term_col(const bf16x8 (&a)[MT][3], const B3& b, f32x4 (&acc)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i][TA], TB == 0 ? b.h : (TB == 1 ? b.m : b.l), acc[i], 0, 0, 0);
}
template <int MT>
__device__ __forceinline__ void mfma16_bf3_col(const bf16x8 (&a)[MT][3], const B3& b, f32x4 (&acc)[MT]) {
    mfma16_term_col<2, 0, MT>(a, b, acc);
    mfma16_term_col<0, 2, MT>(a, b, acc);
    mfma16_term_col<1, 1, MT>(a, b, acc);
    mfma16_term_col<1, 0, MT>(a, b, acc);
    mfma16_term_col<0, 1, MT>(a, b, acc);
    mfma16_term_col<0, 0, MT>(a, b, acc);
}
// the same with the operands swapped (weights = A operand, transposed C tile: layer 2): MT point tiles x ONE 16-channel tile
template <int TW, int TX, int MT>
__device__ __forceinline__ void mfma16_term_col_tr(const B3& w, const bf16x8 (&x)[MT][3], f32x4 (&acc)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(TW == 0 ? w.h : (TW == 1 ? w.m : w.l), x[i][TX], acc[i], 0, 0, 0);
}
template <int MT>
__device__ __forceinline__ void mfma16_bf3_col_tr(const B3& w, const bf16x8 (&x)[MT][3], f32x4 (&acc)[MT]) {
    mfma16_term_col_tr<0, 2, MT>(w, x, acc);   // (activation l) x (weight h)
    mfma16_term_col_tr<2, 0, MT>(w, x, acc);   // (activation h) x (weight l)
    mfma16_term_col_tr<1, 1, MT>(w, x, acc);
    mfma16_term_col_tr<0, 1, MT>(w, x, acc);   // (activation m) x (weight h)
    mfma16_term_col_tr<1, 0, MT>(w, x, acc);   // (activation h) x (weight m)
    mfma16_term_col_tr<0, 0, MT>(w, x, acc);
}
