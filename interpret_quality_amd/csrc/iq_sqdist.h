// The reference's square_distance for one pair of 3-D points, shared by every index-valued kernel that ranks by it
// (iq_geom.hip: region assignment, knn_point, neighbour ordering; iq_wide.hip: the wide region assignment).  Explicitly rounded
// operations in the order the reference's PyTorch expressions evaluate them; the including file is compiled without contraction
// (build.py NO_CONTRACT); the pragma below holds for the rest of the translation unit, which every includer wants anyway.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace iq {

// |p|^2 as torch.sum(p ** 2, -1) evaluates it for three coordinates
__device__ __forceinline__ float norm3(float x, float y, float z) {
    return __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
}

// square_distance(src, dst) (tools/final_util.py:134-147, models/pointnet2.py:12-25, models/pointconv.py:13-32) for one pair:
// the matmul row (K = 3) as an fma chain, then * -2, + |src|^2, + |dst|^2
__device__ __forceinline__ float sqdist3(float sx, float sy, float sz, float sn, float dx, float dy, float dz, float dn) {
    float dot = __fmul_rn(sx, dx);
    dot = __fmaf_rn(sy, dy, dot);
    dot = __fmaf_rn(sz, dz, dot);
    float d = __fmul_rn(-2.f, dot);
    d = __fadd_rn(d, sn);
    return __fadd_rn(d, dn);
}

}  // namespace iq
