// Experiment knobs (iq_set_tuning): the twins of product kernels that a test or bench.py selects as a reference, inside one
// process (guide rule 24).  These are the only (key, value) pairs iq_set_tuning accepts; value 0 on either key = the product paths.
// IQ_TWINS is THE list: the enum, is_twin, interpret_quality_amd/tuning.py's names and include/iq_debug.h's table follow it
// (tests/test_cabi_cpu.py holds them to it).
#pragma once

// (enumerator suffix, key-5 value, what it selects)
#define IQ_TWINS(X)                                                                                             \
    X(EdgeGemmL2, 7, "DGCNN EdgeConv as GEMM + L2 gather")                                                      \
    X(EdgeGemmLds, 8, "DGCNN EdgeConv as GEMM + LDS gather")                                                    \
    X(KnnCompact, 12, "DGCNN compact-row knn_kernel<8> instead of the region walk")                             \
    X(PcKnn, 14, "PointConv kNN path instead of the walk")                                                      \
    X(PcGroupedMlp, 15, "PointConv grouped MLP")                                                                \
    X(KnnFp32Rank, 20, "DGCNN kNN ranking in float32 only")                                                     \
    X(Pn2MemberWalk, 21, "PointNet++ member walk")                                                              \
    X(KnnFp32Mfma, 22, "DGCNN feature-space kNN distances on the fp32 MFMA")                                    \
    X(PcTwoKernel, 31, "PointConv sa1 contraction and 2048 -> 128 layer as two kernels")                        \
    X(ChainL3Fp32, 54, "PointNet chain layer 3 on the fp32 MFMA")                                               \
    X(ChainL3Fp32NoTail16, 55, "the same, 32-row tiles only")                                                   \
    X(GroupFp32, 56, "fp32-MFMA grouped kernels (PointNet++ 32-row chunks, PointConv)")                         \
    X(DenseFp32, 57, "dense layers on the fp32 MFMA")                                                           \
    X(ChainL3Single, 58, "bf16x3 chain layer 3 with one n-tile per pass")                                       \
    X(DenseTile128, 59, "bf16x3 dense layers with 128-row tiles only, the former launch")                       \
    X(ChainNoDedup, 60, "PointNet coalition chains compute every repeated coalition of a batch")                \
    X(GroupFp32Chunk64, 64, "PointNet++ fp32-MFMA grouped kernel with 64-row chunks")

namespace iq {

enum TuneKey { kTuneNoLdsGemm = 3, kTuneTwin = 5 };   // key 3 = 1: dense layers without the LDS-staged GEMM
enum Twin {                                           // key 5
#define IQ_TWIN_ENUMERATOR(name, value, what) kTwin##name = value,
    IQ_TWINS(IQ_TWIN_ENUMERATOR)
#undef IQ_TWIN_ENUMERATOR
};
inline bool is_twin(int value) {
#define IQ_TWIN_MATCH(name, value_, what) if (value == value_) return true;
    IQ_TWINS(IQ_TWIN_MATCH)
#undef IQ_TWIN_MATCH
    return false;
}
bool no_lds_gemm();   // the calling thread's key 3
int twin();           // the calling thread's key 5 (a Twin, or 0)

}  // namespace iq
