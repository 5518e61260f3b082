// RAII HIP-event bracket around a kernel launch, recorded on the launch stream (bench.py's
// roofline leg reads the totals through iq_profile_read).  Costs nothing when disabled.
#pragma once
#include <hip/hip_runtime.h>

namespace iq {

// kSlotDominant: the ONE kernel that dominates a model's step (bench.py's per-model roofline), with the FLOP its MFMA tiles
// execute attached as `work`
enum ProfileSlot { kSlotPrepool = 0, kSlotFstn = 1, kSlotTrunk = 2, kSlotCall = 3, kSlotMask = 4, kSlotDominant = 5 };

bool profile_enabled();

// Experiment knobs (iq_set_tuning): the twins of product kernels that a test or bench.py selects as a reference, inside one
// process (guide rule 24).  These are the only (key, value) pairs iq_set_tuning accepts; value 0 on either key = the product paths.
enum TuneKey { kTuneNoLdsGemm = 3, kTuneTwin = 5 };   // key 3 = 1: dense layers without the LDS-staged GEMM
enum Twin {                                           // key 5
    kTwinEdgeGemmL2 = 7,             // DGCNN EdgeConv as GEMM + L2 gather
    kTwinEdgeGemmLds = 8,            // DGCNN EdgeConv as GEMM + LDS gather
    kTwinKnnCompact = 12,            // DGCNN compact-row knn_kernel<8> instead of the region walk
    kTwinPcKnn = 14,                 // PointConv kNN path instead of the walk
    kTwinPcGroupedMlp = 15,          // PointConv grouped MLP
    kTwinKnnFp32Rank = 20,           // DGCNN kNN ranking in float32 only
    kTwinPn2MemberWalk = 21,         // PointNet++ member walk
    kTwinKnnFp32Mfma = 22,           // DGCNN feature-space kNN distances on the fp32 MFMA
    kTwinPcTwoKernel = 31,           // PointConv sa1 contraction and 2048 -> 128 layer as two kernels
    kTwinChainL3Fp32 = 54,           // PointNet chain layer 3 on the fp32 MFMA
    kTwinChainL3Fp32NoTail16 = 55,   // the same, 32-row tiles only
    kTwinGroupFp32 = 56,             // fp32-MFMA grouped kernels (PointNet++ 32-row chunks, PointConv)
    kTwinDenseFp32 = 57,             // dense layers on the fp32 MFMA
    kTwinChainL3Single = 58,         // bf16x3 chain layer 3 with one n-tile per pass
    kTwinDenseTile128 = 59,          // bf16x3 dense layers with 128-row tiles only, the former launch
    kTwinChainNoDedup = 60,          // PointNet coalition chains compute every repeated coalition of a batch
    kTwinGroupFp32Chunk64 = 64,      // PointNet++ fp32-MFMA grouped kernel with 64-row chunks
};
bool no_lds_gemm();   // the calling thread's key 3
int twin();           // the calling thread's key 5 (a Twin, or 0)

class ProfileSpan {
  public:
    ProfileSpan(int which, hipStream_t st, double work = 0.0);
    ~ProfileSpan();
    ProfileSpan(const ProfileSpan&) = delete;
    ProfileSpan& operator=(const ProfileSpan&) = delete;

  private:
    int which_;
    hipStream_t st_;
    bool on_;
    double work_;
    hipEvent_t start_{}, stop_{};
};

}  // namespace iq
