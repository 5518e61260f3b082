// Shared host-side helpers for libiq_hip.so (gfx950 only).
//
// Launch convention: every kernel goes out through iq::launch, which checks it under the kernel's own name, so after a launch
// that failed nothing more is started.  Host code writes IQ_LAUNCH(kernel, grid, block, lds, stream, args...) - an instantiation
// with a comma in parentheses, (k<1, 2>) - and IQ_TRY(f(...)) for any call that returns a status; both return the status from
// the enclosing function, as IQ_REQUIRE does.  Where no early return is possible (a generic lambda, a loop that must finish
// its bookkeeping) iq::launch("name", ...) is called directly and its status passed on.  The arguments are converted to the
// kernel's parameter types, so a bare nullptr or 0 is fine.  HIP runtime calls (memset, copy, synchronise) go through
// IQ_TRY(iq::hip_ok(call, "what")).  tests/test_cabi_cpu.py keeps the spelling from eroding.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/iq.h"

namespace iq {

inline char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(IQ_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return IQ_OK;
}

// One kernel launch and its check: a launch error comes back under the kernel's own name, and nothing is launched after it.
template <class... P, class... A>
inline int launch(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, static_cast<P>(args)...);
    return check_launch(name);
}

// A HIP runtime call (memset, copy, synchronise) and its check, with HIP's own error string.
inline int hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) return fail(IQ_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return IQ_OK;
}

inline hipStream_t as_stream(iq_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

constexpr size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Arrays carved one after the other out of a workspace, each starting on a 256-byte boundary.  A null base only measures.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base(reinterpret_cast<char*>(b)) {}
    template <class T> T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + off);
        off = align_up(off + count * sizeof(T), 256);
        return p;
    }
    size_t bytes() const { return off; }
};

// The lanes of ONE wave exchange data through LDS: what every lane wrote before is visible to every lane after (LDS is coherent
// within a workgroup; the fences keep the compiler from moving reads above the writes, the barrier keeps the lanes together).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Bit `rid` of a coalition's keep mask; a region id outside [0, 64) (which iq_check_index_range rejects) is never kept,
// so an unvalidated id gives a defined result instead of an undefined shift.
__host__ __device__ inline bool keep_bit(unsigned long long keep, int rid) {
    return (unsigned)rid < 64u && ((keep >> rid) & 1ull);
}

// ---- wide coalitions (include/iq.h, "Wide coalitions"): a row of W = ceil(R / 64) words ------------------------------------------
constexpr int kMaxKeepWords = IQ_MAX_WIDE_REGIONS / 64;

__host__ __device__ inline int keep_words(int R) { return (R + 63) >> 6; }

// bit `rid` of a wide keep row; a region id outside [0, R) is never kept (keep_bit's rule)
__device__ __forceinline__ bool keep_bit_wide(const uint64_t* keep, int rid, int R) {
    return (unsigned)rid < (unsigned)R && ((keep[rid >> 6] >> (rid & 63)) & 1ull);
}

// The 64 lanes of ONE WAVE stride over `count` region ids (row-contiguous: coalesced) and OR their bits into the wave's own row
// `set` of LDS words (zeroed before, and read only after a barrier).  OR is order-independent: the words do not depend on the
// schedule.  An id outside [0, R) sets nothing; the return value says whether this lane met one.
__device__ __forceinline__ bool wave_or_regions(const int32_t* __restrict__ ids, int count, int R, int lane, unsigned long long* set) {
    bool outside = false;
    for (int j = lane; j < count; j += 64) {
        const int r = ids[j];
        if ((unsigned)r < (unsigned)R) atomicOr(&set[r >> 6], 1ull << (r & 63));
        else outside = true;
    }
    return outside;
}

// The coalition of ONE WAVE, for the small kernels of the compact coalition paths that turn a coalition's mask into its kept
// points (a wave per coalition).  The switch between the two kinds of game is this template argument, so a narrow kernel holds
// no trace of the wide form:
//   WIDE = false: keep[b] is the uint64 mask, held in a register and tested with keep_bit - R, W and `strip` are not looked at;
//   WIDE = true:  keep is (B, W); lane l < W loads word l of row b into `strip` (the wave's own kMaxKeepWords words of LDS), once,
//                 and every test afterwards is an LDS read - no global read per point.  The fences and the wave barrier make the
//                 W lanes' words visible to all 64 (LDS is coherent within a workgroup; they keep the compiler from moving the
//                 reads above the writes).  Every lane of the wave must construct it (no divergent return before).
template <bool WIDE>
struct WaveKeep {
    unsigned long long k = 0;
    const uint64_t* row = nullptr;
    int R = 64;
    __device__ __forceinline__ WaveKeep(const uint64_t* keep, int b, int R_, int W, int lane, uint64_t* strip) {
        if constexpr (WIDE) {
            if (lane < W) strip[lane] = keep[(size_t)b * W + lane];
            wave_sync();
            row = strip;
            R = R_;
        } else {
            k = keep[b];
        }
    }
    __device__ __forceinline__ bool operator()(int rid) const {
        if constexpr (WIDE) return keep_bit_wide(row, rid, R);
        else return keep_bit(k, rid);
    }
};

// The cloud a workgroup of an XCD-aware grid works on.  Workgroups go round-robin over the 8 XCDs (blockIdx & 7); all
// workgroups of a cloud sit on one XCD (they share its rows through one L2), clouds c = 8 k + xcd.  A batch whose work has
// period 4 in the cloud index - the four masked clouds S+{i,j}, S+{i}, S+{j}, S of every interaction context, largest first
// (final_point_binary_interaction_logits.py:48-52) - would put every largest cloud on XCDs 0 and 4 and every smallest on 3 and
// 7 (kNN work ~ rows^2: 9.6 % above the mean over the 13 ratios, 2x for the low orders): the low two bits of the cloud index
// are rotated by the group-of-eight number, so each XCD sees all four kinds equally often.  A bijection on every full group of 4.
__device__ inline int xcd_cloud(int block, int wgs_per_cloud, int B) {
    const int c = ((block >> 3) / wgs_per_cloud) * 8 + (block & 7);
    return (c | 3) < B ? (c & ~3) | ((c + (c >> 3)) & 3) : c;
}

}  // namespace iq

#define IQ_REQUIRE(cond, ...) \
    do {                      \
        if (!(cond)) return iq::fail(IQ_EINVAL, __VA_ARGS__); \
    } while (0)
#define IQ_TRY(expr)  do { if (int rc_ = (expr)) return rc_; } while (0)
#define IQ_LAUNCH(kernel, ...) IQ_TRY(iq::launch(#kernel, kernel, __VA_ARGS__))
