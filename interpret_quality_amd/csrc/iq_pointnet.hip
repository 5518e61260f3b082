// Fused fp32-MFMA PointNet forward over coalitions (models/pointnet.py:11-115).
//
// A masked cloud is {kept points} + {the centre, if anything was masked}.  Every per-point layer
// is a pointwise function and every pooling is a max, so
//   * the input-STN's 3->64->128->1024 chain is evaluated ONCE per cloud and pre-pooled per region
//     (chain<kPrepool>); a coalition's pooled feature is a max over its kept regions (+ centre);
//   * the feature-STN and trunk chains run only over a coalition's DISTINCT points.
// Both are exact with respect to evaluating the same kernels on the materialised cloud.
//
// The chain kernel itself (pn_chain_kernel, its three bodies, launch_chain) lives in iq_pointnet_chain.h.
#include <algorithm>

#include "iq_pointnet_chain.h"
#include "iq_profile.h"
#include "iq_twin.h"

namespace {

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
// Distinct coalitions only (pn_compact kernels): item = a slot, cloud_of = a cloud per slot, src = the batch item whose mask the slot
// takes, n_dev = the slots in use; a workgroup past them leaves.
__device__ __forceinline__ int padded_rows(int nrows) {
    static_assert((kMaxN + kMC96 - 1) / kMC96 * kMC96 <= kRowCap, "a padded row list fits its stride");
    return max((nrows + kMC - 1) / kMC * kMC, (nrows + kMC96 - 1) / kMC96 * kMC96);
}
__global__ __launch_bounds__(64) void pn_rows_kernel(const uint16_t* __restrict__ sorted_all,
                                                     const int32_t* __restrict__ roff_all,
                                                     const uint64_t* __restrict__ keep_all,
                                                     const int32_t* __restrict__ cloud_of, uint16_t* __restrict__ rows_all,
                                                     int32_t* __restrict__ nrows_all, int N, int R, int nclouds,
                                                     int with_centre, int prepool, const int32_t* __restrict__ src,
                                                     const int32_t* __restrict__ n_dev) {
    const int item = blockIdx.x, lane = threadIdx.x;
    if (n_dev && item >= *n_dev) return;
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
        keep = (keep_all ? keep_all[src ? src[item] : item] : ~0ull) & full;
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
                                                                  int B, const int32_t* __restrict__ n_dev) {
    __shared__ int lh[kBins];   // per-workgroup histogram: one global atomic per bin and workgroup instead of one per item
    if (n_dev) B = min(B, *n_dev);   // the live items where only the device knows them: the others do not enter the order
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
                                                                    int32_t* __restrict__ order, int B,
                                                                    const int32_t* __restrict__ n_dev) {
    __shared__ int lh[kBins], base[kBins];
    if (n_dev) B = min(B, *n_dev);
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
                                                                       int32_t* __restrict__ order, int B,
                                                                       const int32_t* __restrict__ n_dev) {
    __shared__ int lh[kBins];
    const int tid = threadIdx.x, lane = tid & 63;
    if (n_dev) B = min(B, *n_dev);
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

// ---- repeated coalitions of a batch: only the first item of every (cloud, keep mask) is evaluated, the others take its results ----
// rep[i] = the lowest item j <= i on i's cloud with the same kept regions (the mask's low R bits, as pn_stn_gather_kernel forms them):
// the same row list in table order under the same transforms, so whichever member computes, the row is the same; the lowest makes rep
// independent of timing and rep[rep[i]] == rep[i].  An open-addressing table of item indices, cleared to -1, at most half full:
// pn_rep_insert_kernel claims a slot per distinct key (atomicCAS; a slot always holds SOME member of its group, so a later item
// compares keys through it and probes on if they differ) and keeps the group's lowest index there (atomicMin); it leaves each
// item's slot in rep, and pn_rep_write_kernel replaces the slot by what it holds.  The launch boundary orders the two phases.
__host__ __device__ inline size_t rep_slots(int B) {   // a power of two >= 2 B
    size_t s = 4;
    while (s < 2 * (size_t)B) s <<= 1;
    return s;
}

__device__ __forceinline__ uint32_t rep_hash(uint64_t k, int cloud) {
    uint64_t x = k * 0x9E3779B97F4A7C15ull + (uint64_t)(uint32_t)cloud * 0xC2B2AE3D27D4EB4Full;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return (uint32_t)(x >> 32);
}

__global__ __launch_bounds__(kThreads) void pn_rep_insert_kernel(const uint64_t* __restrict__ keep, const int32_t* __restrict__ cloud_of,
                                                                 int32_t* table, int32_t* __restrict__ rep, int B, int R,
                                                                 uint32_t slot_mask) {
    const int item = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = item < B;
    const uint64_t full = R >= 64 ? ~0ull : ((1ull << R) - 1);
    const uint64_t k = live ? keep[item] & full : 0;
    const int cloud = live && cloud_of ? cloud_of[item] : 0;
    // equal keys inside a wave go through their lowest lane (= lowest item): a batch of B copies of one mask then costs B / 64
    // atomics on its slot instead of B.  A Shapley batch has close to 64 keys per wave, hence 64 rounds: l is wave-uniform, so
    // the leader's key comes by v_readlane, not through the LDS crossbar of __shfl
    const int k_lo = (int)(uint32_t)k, k_hi = (int)(uint32_t)(k >> 32);
    int leader = lane;
    for (uint64_t todo = __ballot(live); todo;) {
        const int l = __ffsll((unsigned long long)todo) - 1;
        const bool same = live && k_lo == __builtin_amdgcn_readlane(k_lo, l) && k_hi == __builtin_amdgcn_readlane(k_hi, l) &&
                          cloud == __builtin_amdgcn_readlane(cloud, l);
        if (same) leader = l;
        todo &= ~__ballot(same);
    }
    int slot = 0;
    if (live && leader == lane) {
        uint32_t h = rep_hash(k, cloud) & slot_mask;
        for (;;) {   // at most B of >= 2 B slots are ever claimed: an empty one is always ahead
            // a plain look first: a slot only ever goes from -1 to a member of one group and then down inside it, so whatever
            // the load returns, however old, is still a valid witness - and a lower member there needs no atomic at all (the
            // full and the empty set of a Shapley sample would otherwise queue two atomics per wave on two addresses)
            int old = __atomic_load_n(&table[h], __ATOMIC_RELAXED);
            if (old == -1) old = atomicCAS(&table[h], -1, item);
            if (old == -1) break;
            if ((keep[old] & full) == k && (cloud_of ? cloud_of[old] : 0) == cloud) {
                if (item < old) atomicMin(&table[h], item);
                break;
            }
            h = (h + 1) & slot_mask;
        }
        slot = (int)h;
    }
    slot = __shfl(slot, leader);
    if (live) rep[item] = slot;
}

// block_cnt (optional): the representatives among this workgroup's kThreads items, for pn_compact_scan_kernel
__global__ __launch_bounds__(kThreads) void pn_rep_write_kernel(const int32_t* __restrict__ table, int32_t* __restrict__ rep, int B,
                                                                int32_t* __restrict__ block_cnt) {
    const int item = blockIdx.x * kThreads + threadIdx.x;
    int r = -1;
    if (item < B) rep[item] = r = table[rep[item]];
    if (block_cnt) {
        const int n = __syncthreads_count(r == item);
        if (threadIdx.x == 0) block_cnt[blockIdx.x] = n;
    }
}

// rep (B) from keep (B) and cloud_of (B, or null: one cloud); table: rep_slots(B) int32 of scratch.  The same three launches for
// every B: one workgroup with the table in LDS took 40 us on a pose-sized batch against 26 us for these (profiles/chain_repeats_ab.txt)
int launch_reps(const uint64_t* keep, const int32_t* cloud_of, int B, int R, int32_t* rep, int32_t* table, hipStream_t st,
                int32_t* block_cnt = nullptr) {
    const size_t slots = rep_slots(B);
    IQ_TRY(iq::hip_ok(hipMemsetAsync(table, 0xff, slots * sizeof(int32_t), st), "pn_rep table memset"));
    const dim3 grid((B + kThreads - 1) / kThreads);
    IQ_LAUNCH(pn_rep_insert_kernel, grid, dim3(kThreads), 0, st, keep, cloud_of, table, rep, B, R, (uint32_t)(slots - 1));
    IQ_LAUNCH(pn_rep_write_kernel, grid, dim3(kThreads), 0, st, table, rep, B, block_cnt);
    return IQ_OK;
}

// The distinct coalitions of a batch in slots 0 .. U-1, in the order of their first items: slot_of[i] = the number of representatives
// below rep[i] (a rank, so the map does not depend on timing), item_u[s] = the representative in slot s, cloud_u[s] = its cloud (only
// with cloud_of), *n_distinct = U.  Everything after this runs on U slots, a count that stays on the device; pn_expand kernels give
// every item its slot's results at the end.  Up to kOrderFusedMax items one workgroup does it, a thread kOrderPer CONSECUTIVE
// items; above, the count (pn_rep_write_kernel) / scan / scatter / fill launches below, as the launch order does.
__device__ __forceinline__ int block_exclusive_scan(int v, int* wsum, int& total) {   // blockDim.x / 64 <= 16 waves; wsum: one int each
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    __syncthreads();   // wsum may still be read from an earlier call
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int run = inc - v;
    total = 0;
    for (int w = 0; w < nw; ++w) {
        const int c = wsum[w];
        if (w < wave) run += c;
        total += c;
    }
    return run;
}

__global__ __launch_bounds__(kOrderThreads) void pn_compact_fused_kernel(const int32_t* __restrict__ rep, const int32_t* __restrict__ cloud_of,
                                                                         int32_t* __restrict__ slot_of, int32_t* __restrict__ item_u,
                                                                         int32_t* __restrict__ cloud_u, int32_t* __restrict__ n_distinct,
                                                                         int B) {
    __shared__ int slot_s[kOrderFusedMax];   // a representative's slot
    __shared__ int wsum[kOrderThreads / 64];
    const int tid = threadIdx.x;
    int r[kOrderPer], cnt = 0;
#pragma unroll
    for (int j = 0; j < kOrderPer; ++j) {
        const int item = tid * kOrderPer + j;
        r[j] = item < B ? rep[item] : -1;
        cnt += r[j] == item;
    }
    int total;
    int slot = block_exclusive_scan(cnt, wsum, total);
#pragma unroll
    for (int j = 0; j < kOrderPer; ++j) {
        const int item = tid * kOrderPer + j;
        if (r[j] == item) {
            slot_s[item] = slot;
            item_u[slot] = item;
            if (cloud_of) cloud_u[slot] = cloud_of[item];
            ++slot;
        }
    }
    if (tid == 0) *n_distinct = total;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kOrderPer; ++j) {
        const int item = tid * kOrderPer + j;
        if (item < B) slot_of[item] = slot_s[r[j]];
    }
}

// block_cnt (nb counts of representatives, pn_rep_write_kernel) -> the first slot of every workgroup, in place; *n_distinct
__global__ __launch_bounds__(kThreads) void pn_compact_scan_kernel(int32_t* __restrict__ block_cnt, int32_t* __restrict__ n_distinct, int nb) {
    __shared__ int wsum[kThreads / 64];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += kThreads) {
        const int b = b0 + threadIdx.x, c = b < nb ? block_cnt[b] : 0;
        int total;
        const int ex = block_exclusive_scan(c, wsum, total);
        if (b < nb) block_cnt[b] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *n_distinct = carry;
}

// the representatives: their slot (slot_of), and the slot's item and cloud
__global__ __launch_bounds__(kThreads) void pn_compact_scatter_kernel(const int32_t* __restrict__ rep, const int32_t* __restrict__ cloud_of,
                                                                      const int32_t* __restrict__ block_first,
                                                                      int32_t* __restrict__ slot_of, int32_t* __restrict__ item_u,
                                                                      int32_t* __restrict__ cloud_u, int B) {
    __shared__ int wsum[kThreads / 64];
    const int item = blockIdx.x * kThreads + threadIdx.x;
    const bool is_rep = item < B && rep[item] == item;
    int total;
    const int slot = block_first[blockIdx.x] + block_exclusive_scan(is_rep ? 1 : 0, wsum, total);
    if (is_rep) {
        slot_of[item] = slot;
        item_u[slot] = item;
        if (cloud_of) cloud_u[slot] = cloud_of[item];
    }
}

// the other items: their representative's slot (written by the launch before)
__global__ __launch_bounds__(kThreads) void pn_compact_fill_kernel(const int32_t* __restrict__ rep, int32_t* slot_of, int B) {
    const int item = blockIdx.x * kThreads + threadIdx.x;
    if (item >= B) return;
    const int r = rep[item];
    if (r != item) slot_of[item] = slot_of[r];
}

// rep (B; launch_reps with block_cnt above kOrderFusedMax items) -> slot_of (B), item_u, cloud_u (null without cloud_of), n_distinct
int launch_compact(const int32_t* rep, const int32_t* cloud_of, int B, int32_t* block_cnt, int32_t* slot_of, int32_t* item_u,
                   int32_t* cloud_u, int32_t* n_distinct, hipStream_t st) {
    if (B <= kOrderFusedMax) {
        IQ_LAUNCH(pn_compact_fused_kernel, dim3(1), dim3(kOrderThreads), 0, st, rep, cloud_of, slot_of, item_u, cloud_u,
                  n_distinct, B);
    } else {
        const int nb = (B + kThreads - 1) / kThreads;
        IQ_LAUNCH(pn_compact_scan_kernel, dim3(1), dim3(kThreads), 0, st, block_cnt, n_distinct, nb);
        IQ_LAUNCH(pn_compact_scatter_kernel, dim3(nb), dim3(kThreads), 0, st, rep, cloud_of, block_cnt, slot_of, item_u,
                  cloud_u, B);
        IQ_LAUNCH(pn_compact_fill_kernel, dim3(nb), dim3(kThreads), 0, st, rep, slot_of, B);
    }
    return IQ_OK;
}

// at the end: every item takes its slot's logits ...
__global__ __launch_bounds__(kThreads) void pn_expand_logits_kernel(const float* __restrict__ logits_u, const int32_t* __restrict__ slot_of,
                                                                    float* __restrict__ logits, int B, int ncls) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (size_t)B * ncls) return;
    const int item = (int)(t / ncls), c = (int)(t - (size_t)item * ncls);
    logits[t] = logits_u[(size_t)slot_of[item] * ncls + c];
}

// ... and, where the caller asked for them, its slot's packed feature transform (tfp_u, by slot, -> tfp, by item) and its
// representative's row of crt_points, which the trunk chain wrote in place (ChainArgs::arg_row): representatives' rows are only read
__global__ __launch_bounds__(kThreads) void pn_expand_rows_kernel(const int32_t* __restrict__ slot_of, const int32_t* __restrict__ item_u,
                                                                  const float* __restrict__ tfp_u, float* __restrict__ tfp,
                                                                  int32_t* crt_points) {
    const int item = blockIdx.x, slot = slot_of[item];
    static_assert(kFeat == 4 * kThreads, "one int4 per thread");
    if (tfp) {
        const f32x4* s4 = reinterpret_cast<const f32x4*>(tfp_u + (size_t)slot * 4096);
        f32x4* d4 = reinterpret_cast<f32x4*>(tfp + (size_t)item * 4096);
#pragma unroll
        for (int q = 0; q < 4096 / 4 / kThreads; ++q) d4[threadIdx.x + q * kThreads] = s4[threadIdx.x + q * kThreads];
    }
    if (crt_points) {
        const int src = item_u[slot];
        if (src != item) {
            const int4 v = reinterpret_cast<const int4*>(crt_points + (size_t)src * kFeat)[threadIdx.x];
            reinterpret_cast<int4*>(crt_points + (size_t)item * kFeat)[threadIdx.x] = v;
        }
    }
}

// ---- pooled input-STN feature of a coalition: max over kept regions (+ centre) -------------
__global__ __launch_bounds__(kThreads) void pn_stn_gather_kernel(const float* __restrict__ G,
                                                                 const int32_t* __restrict__ nrows_all,
                                                                 const uint64_t* __restrict__ keep,
                                                                 const int32_t* __restrict__ cloud_of,
                                                                 float* __restrict__ out, int R, int nclouds,
                                                                 int with_centre, const int32_t* __restrict__ src,
                                                                 const int32_t* __restrict__ n_dev) {
    const int item = blockIdx.x;   // src, n_dev: as in pn_rows_kernel
    if (n_dev && item >= *n_dev) return;
    const int cloud = cloud_of ? cloud_of[item] : (nclouds == 1 ? 0 : item);
    const uint64_t full = R >= 64 ? ~0ull : ((1ull << R) - 1);
    const uint64_t k = (keep ? keep[src ? src[item] : item] : ~0ull) & full;
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

using iq::launch_linear;   // (the heads pass fit_tiles = true: tile heights that fill the chip, iq_mfma.h)

struct Workspace {
    uint16_t* sorted_pts;
    int32_t* roff;
    uint16_t* rows_pre;  // (nclouds*(R+1), kRowCap)
    int32_t* nrows_pre;
    uint16_t* rows;      // (B, kRowCap)
    int32_t* nrows;      // (B)
    int32_t* order;    // (B) launch order
    int32_t* bin_of;   // (B) on the narrow keep-mask route every item's representative (launch_reps) until the slots are assigned; then
                       // launch-order bins until the order is scattered (above kOrderFusedMax items only); afterwards, on the prefix
                       // route, a cloud per item
    int32_t* hist;     // (kBins)
    int32_t* slot_of;  // (B) the slot of every item, (B) the item and (B) the cloud of every slot, and the number of slots in use
    int32_t* item_u;   // (pn_compact kernels): one block of 3 B + 1 int32
    int32_t* cloud_u;
    int32_t* n_distinct;
    float* G;
    float* gbuf;
    float* h1;         // (B,512) the heads' first hidden layer, and at the end the logits by slot; before the input-STN head writes
                       // it, the table of launch_reps (rep_slots(B) int32 < 4 B of them) and behind it the compaction's counts
    float* h2;
    float* trans;
    float* tfp;
    uint16_t* fc3_bf3;   // fstn.fc3's weights as three bf16 terms, derived per call from the float32 image (pointnet_coalitions)
    size_t bytes;
};

// roff_entries: offsets per cloud - IQ_MAX_REGIONS + 1 for the narrow entry points (their layout since ABI 100), R + 1 for the wide one
Workspace carve(void* base, int B, int nclouds, int N, int R, int roff_entries = IQ_MAX_REGIONS + 1) {
    Workspace w;
    iq::Carver c(base);
    const size_t b = (size_t)B, nc = (size_t)nclouds;
    w.sorted_pts = c.take<uint16_t>(nc * N);
    w.roff = c.take<int32_t>(nc * roff_entries);
    w.rows_pre = c.take<uint16_t>(nc * (R + 1) * kRowCap);
    w.nrows_pre = c.take<int32_t>(nc * (R + 1));
    w.rows = c.take<uint16_t>(b * kRowCap);
    w.nrows = c.take<int32_t>(b);
    w.order = c.take<int32_t>(b);
    w.bin_of = c.take<int32_t>(b);
    w.hist = c.take<int32_t>((size_t)kBins);
    w.slot_of = c.take<int32_t>(3 * b + 1);
    w.item_u = w.slot_of + b;
    w.cloud_u = w.item_u + b;
    w.n_distinct = w.cloud_u + b;
    w.G = c.take<float>(nc * (R + 1) * kFeat);
    w.gbuf = c.take<float>(b * kFeat);
    w.h1 = c.take<float>(b * 512);
    w.h2 = c.take<float>(b * 256);
    w.trans = c.take<float>(b * 9);
    w.tfp = c.take<float>(b * 4096);
    w.fc3_bf3 = c.take<uint16_t>(iq_packed_bf3_elems(4096, 256));
    w.bytes = c.bytes();
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
    iq::ProfileSpan call_span(iq::kSlotCall, st);

    // Repeated coalitions: narrow keep masks in table order only (a prefix route's row lists follow its permutations), and a cloud
    // per item that is known - without cloud_of and with several clouds every item has its own.  The distinct ones move to slots
    // 0 .. U-1 (pn_compact kernels) and every launch below works on slots: grids for B, the bound the host knows, and n_dev = U on
    // the device for the workgroups past it to leave.  rows, nrows, gbuf, trans, tfp, h1 and h2 are then indexed by slot.  Every
    // other call is the same launches with the identity map: n_dev null, an item its own slot.  rep borrows the launch order's
    // bins, the table and the counts h1: both idle up to here (Workspace).
    const int32_t *n_dev = nullptr, *slot_item = nullptr, *slot_cloud = cloud_of;
    if (!wide_words && !orders && keep && B > 1 && (cloud_of || nclouds == 1) && iq::twin() != iq::kTwinChainNoDedup) {
        static_assert(sizeof(int32_t) * 5 <= sizeof(float) * 512, "rep_slots(B) < 4 B int32 and B / kThreads + 1 counts inside h1's (B,512) floats");
        int32_t* table = reinterpret_cast<int32_t*>(ws.h1);
        int32_t* block_cnt = B > kOrderFusedMax ? table + rep_slots(B) : nullptr;
        IQ_TRY(launch_reps(keep, cloud_of, B, R, ws.bin_of, table, st, block_cnt));
        IQ_TRY(launch_compact(ws.bin_of, cloud_of, B, block_cnt, ws.slot_of, ws.item_u, ws.cloud_u, ws.n_distinct, st));
        n_dev = ws.n_distinct;
        slot_item = ws.item_u;
        if (cloud_of) slot_cloud = ws.cloud_u;
    }

    const int pre_items = nclouds * (R + with_centre);
    // the chain kernels take a cloud per item: the prefix route writes one (pn_stn_prefix_kernel) where the launch order kept its
    // bins, which nothing reads once the order is scattered
    const int32_t* item_cloud = orders ? (nclouds > 1 ? ws.bin_of : nullptr) : slot_cloud;
    if (wide_words) {
        IQ_LAUNCH(pn_prepare_wide_kernel, dim3(nclouds), dim3(kThreads), 0, st, region_id, ws.sorted_pts, ws.roff, N, R);
        IQ_LAUNCH(pn_rows_wide_kernel, dim3(pre_items), dim3(64), 0, st, ws.sorted_pts, ws.roff, nullptr, nullptr,
                  ws.rows_pre, ws.nrows_pre, N, R, wide_words, nclouds, with_centre, 1);
        if (orders) {
            IQ_LAUNCH(pn_rows_prefix_kernel, dim3(groups), dim3(kThreads), 0, st, ws.sorted_pts, ws.roff, orders, cloud_of,
                      ws.rows, ws.nrows, N, R, nclouds, with_centre);
        } else {
            IQ_LAUNCH(pn_rows_wide_kernel, dim3(B), dim3(64), 0, st, ws.sorted_pts, ws.roff, keep, cloud_of, ws.rows,
                      ws.nrows, N, R, wide_words, nclouds, with_centre, 0);
        }
    } else {
        IQ_LAUNCH(pn_prepare_kernel, dim3(nclouds), dim3(kThreads), 0, st, region_id, ws.sorted_pts, ws.roff, N, R);
        IQ_LAUNCH(pn_rows_kernel, dim3(pre_items), dim3(64), 0, st, ws.sorted_pts, ws.roff, nullptr, nullptr,
                  ws.rows_pre, ws.nrows_pre, N, R, nclouds, with_centre, 1, nullptr, nullptr);
        IQ_LAUNCH(pn_rows_kernel, dim3(B), dim3(64), 0, st, ws.sorted_pts, ws.roff, keep, slot_cloud, ws.rows,
                  ws.nrows, N, R, nclouds, with_centre, 0, slot_item, n_dev);
    }
    // launch order of the coalition chains: most rows first, so the grid drains evenly
    if (B <= kOrderFusedMax) {
        IQ_LAUNCH(pn_order_fused_kernel, dim3(1), dim3(kOrderThreads), 0, st, ws.nrows, ws.order, B, n_dev);
    } else {
        IQ_TRY(iq::hip_ok(hipMemsetAsync(ws.hist, 0, kBins * sizeof(int32_t), st), "pn_order histogram memset"));
        IQ_LAUNCH(pn_order_count_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ws.nrows,
                  ws.bin_of, ws.hist, B, n_dev);
        IQ_LAUNCH(pn_order_scan_kernel, dim3(1), dim3(64), 0, st, ws.hist);
        IQ_LAUNCH(pn_order_scatter_kernel, dim3((B + kThreads - 1) / kThreads), dim3(kThreads), 0, st,
                  ws.bin_of, ws.hist, ws.order, B, n_dev);
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
        IQ_TRY(launch_chain<kPrepool>(a, st));
    }

    if (orders)
        IQ_LAUNCH(pn_stn_prefix_kernel, dim3(groups, kFeat / 256), dim3(64), 0, st, ws.G, ws.nrows, orders, cloud_of, ws.gbuf,
                  item_cloud ? ws.bin_of : nullptr, R, nclouds, with_centre);
    else if (wide_words)
        IQ_LAUNCH(pn_stn_gather_wide_kernel, dim3(B), dim3(kThreads), 0, st, ws.G, ws.nrows, keep, cloud_of, ws.gbuf,
                  R, wide_words, nclouds, with_centre);
    else
        IQ_LAUNCH(pn_stn_gather_kernel, dim3(B), dim3(kThreads), 0, st, ws.G, ws.nrows, keep, slot_cloud, ws.gbuf,
                  R, nclouds, with_centre, slot_item, n_dev);
    IQ_TRY(launch_linear(ws.gbuf, kFeat, w->stn_fc1, ws.h1, 512, B, 1, st, n_dev, nullptr, 0, true));
    IQ_TRY(launch_linear(ws.h1, 512, w->stn_fc2, ws.h2, 256, B, 1, st, n_dev, nullptr, 0, true));
    IQ_TRY(launch_linear(ws.h2, 256, w->stn_fc3, ws.trans, 9, B, 0, st, n_dev, nullptr, 0, true));

    // 2. feature-STN chain over each coalition's distinct points
    a.cloud_of = item_cloud; a.trans = ws.trans;
    a.rows = ws.rows; a.nrows = ws.nrows;
    a.item_order = ws.order;
    a.n_dev = n_dev;
    a.w_in = w->feat_in;
    a.items = B;
    a.out = ws.gbuf;
    // by slot: the workspace's image; the caller's, if any, is expanded from it at the end
    float* tfp = trans_feat_packed && !n_dev ? trans_feat_packed : ws.tfp;
    if (w->fstn_c1.w) {
        a.w1 = w->fstn_c1.w; a.b1 = w->fstn_c1.b;
        a.w2 = w->fstn_c2.w; a.b2 = w->fstn_c2.b;
        a.w3 = w->fstn_c3.w; a.b3 = w->fstn_c3.b; a.w3_bf3 = reinterpret_cast<const unsigned short*>(w->fstn_c3_bf3);
        a.w2_bf3 = reinterpret_cast<const unsigned short*>(w->fstn_c2_bf3);
        {
            iq::ProfileSpan span(iq::kSlotFstn, st);
            IQ_TRY(launch_chain<kFstn>(a, st));
        }
        IQ_TRY(launch_linear(ws.gbuf, kFeat, w->fstn_fc1, ws.h1, 512, B, 1, st, n_dev, nullptr, 0, true));
        IQ_TRY(launch_linear(ws.h1, 512, w->fstn_fc2, ws.h2, 256, B, 1, st, n_dev, nullptr, 0, true));
        // fstn.fc3 (256 -> 4096, 70 % of the heads' FLOP) on the bf16 matrix pipe like the other wide layers.  The descriptor brings
        // no bf16x3 image of it (its rows are permuted by iq_pack_fstn_fc3; the packed weight set is what it has always been), so the
        // image is split off the float32 one here, per call: 1 M weights, a few microseconds, and nothing to go stale when a
        // caller reuses a pointer for other weights.  Twin kTwinDenseFp32: no split, the fp32-MFMA kernel.
        iq_dense_layer fc3 = w->fstn_fc3;
        IQ_REQUIRE(fc3.cin == 256 && fc3.cout == 4096, "%s: fstn_fc3 is %d -> %d, not 256 -> 4096", who, fc3.cin, fc3.cout);
        if (!fc3.w_bf3 && iq::twin() != iq::kTwinDenseFp32) {
            IQ_TRY(iq::launch_split_bf3(fc3.w, ws.fc3_bf3, 4096, 256, st));
            fc3.w_bf3 = ws.fc3_bf3;
        }
        IQ_TRY(launch_linear(ws.h2, 256, fc3, tfp, 4096, B, 0, st, n_dev, nullptr, 0, true));
    } else {
        // feature_transform = False (models/pointnet.py:62-63,72-78): no feature STN.  The trunk multiplies by the packed
        // IDENTITY instead (fstn_fc3.b = iq_pack_fstn_fc3 of a zero layer): sum_k f[k] I[k][n] = f[n] + zeros, exact.
        IQ_REQUIRE(w->fstn_fc3.b, "%s: without a feature STN, fstn_fc3.b must hold the packed identity", who);
        IQ_LAUNCH(pn_fill_rows_kernel, dim3((unsigned)(((size_t)B * 1024 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                  tfp, w->fstn_fc3.b, B);
    }

    // 3. trunk chain
    a.argrow = crt_points;
    a.arg_row = slot_item;   // a representative writes its own row of crt_points: the others copy it (pn_expand_rows_kernel)
    a.w1 = tfp; a.b1 = nullptr;
    a.w2 = w->feat_c2.w; a.b2 = w->feat_c2.b;
    a.w3 = w->feat_c3.w; a.b3 = w->feat_c3.b; a.w3_bf3 = reinterpret_cast<const unsigned short*>(w->feat_c3_bf3);
    a.w2_bf3 = reinterpret_cast<const unsigned short*>(w->feat_c2_bf3);
    {
        iq::ProfileSpan span(iq::kSlotTrunk, st);
        IQ_TRY(launch_chain<kTrunk>(a, st));
    }
    IQ_TRY(launch_linear(ws.gbuf, kFeat, w->cls_fc1, ws.h1, 512, B, 1, st, n_dev, nullptr, 0, true));
    IQ_TRY(launch_linear(ws.h1, 512, w->cls_fc2, ws.h2, 256, B, 1, st, n_dev, nullptr, 0, true));
    if (!n_dev) return launch_linear(ws.h2, 256, w->cls_fc3, logits, w->cls_fc3.cout, B, 0, st, nullptr, nullptr, 0, true);
    // the logits by slot where h1 was (cls_fc2 has read it), then every item its slot's results
    const int ncls = w->cls_fc3.cout;
    IQ_REQUIRE(ncls <= 512, "%s: %d classes", who, ncls);
    IQ_TRY(launch_linear(ws.h2, 256, w->cls_fc3, ws.h1, ncls, B, 0, st, n_dev, nullptr, 0, true));
    IQ_LAUNCH(pn_expand_logits_kernel, dim3((unsigned)(((size_t)B * ncls + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
              ws.h1, ws.slot_of, logits, B, ncls);
    if (trans_feat_packed || crt_points)
        IQ_LAUNCH(pn_expand_rows_kernel, dim3(B), dim3(kThreads), 0, st, ws.slot_of, ws.item_u, ws.tfp, trans_feat_packed,
                  crt_points);
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

// include/iq_debug.h: the representatives alone, from the launcher the forward uses, with the caller's scratch for the table
extern "C" int iq_debug_pointnet_reps(const uint64_t* keep, const int32_t* cloud_of, int B, int nclouds, int R, int32_t* rep_out,
                                      void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && nclouds >= 1, "iq_debug_pointnet_reps: B=%d nclouds=%d", B, nclouds);
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_REGIONS, "iq_debug_pointnet_reps: R=%d not in [1,%d]", R, IQ_MAX_REGIONS);
    IQ_REQUIRE(cloud_of || nclouds == 1, "iq_debug_pointnet_reps: cloud_of required when nclouds > 1");
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(keep && rep_out, "iq_debug_pointnet_reps: null pointer");
    const size_t need = rep_slots(B) * sizeof(int32_t);
    if (!scratch || scratch_bytes < need)
        return iq::fail(IQ_EWORKSPACE, "iq_debug_pointnet_reps: scratch %zu < %zu bytes", scratch_bytes, need);
    return launch_reps(keep, cloud_of, B, R, rep_out, reinterpret_cast<int32_t*>(scratch), iq::as_stream(stream));
}

// include/iq_debug.h: the slot map alone, from the two launchers the forward uses, with the caller's scratch for rep, table and counts
extern "C" int iq_debug_pointnet_slots(const uint64_t* keep, const int32_t* cloud_of, int B, int nclouds, int R, int32_t* slots_out,
                                       void* scratch, size_t scratch_bytes, iq_stream_t stream) {
    IQ_REQUIRE(B >= 0 && nclouds >= 1, "iq_debug_pointnet_slots: B=%d nclouds=%d", B, nclouds);
    IQ_REQUIRE(R >= 1 && R <= IQ_MAX_REGIONS, "iq_debug_pointnet_slots: R=%d not in [1,%d]", R, IQ_MAX_REGIONS);
    IQ_REQUIRE(cloud_of || nclouds == 1, "iq_debug_pointnet_slots: cloud_of required when nclouds > 1");
    if (B == 0) return IQ_OK;
    IQ_REQUIRE(keep && slots_out, "iq_debug_pointnet_slots: null pointer");
    const size_t b = (size_t)B, nb = (b + kThreads - 1) / kThreads, need = (b + rep_slots(B) + nb) * sizeof(int32_t);
    if (!scratch || scratch_bytes < need)
        return iq::fail(IQ_EWORKSPACE, "iq_debug_pointnet_slots: scratch %zu < %zu bytes", scratch_bytes, need);
    hipStream_t st = iq::as_stream(stream);
    int32_t *rep = reinterpret_cast<int32_t*>(scratch), *table = rep + b;
    int32_t* block_cnt = B > kOrderFusedMax ? table + rep_slots(B) : nullptr;
    IQ_TRY(launch_reps(keep, cloud_of, B, R, rep, table, st, block_cnt));
    return launch_compact(rep, cloud_of, B, block_cnt, slots_out, slots_out + b, slots_out + 2 * b, slots_out + 3 * b, st);
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
