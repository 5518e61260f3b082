/*
 * iq_debug.h - diagnostic entry points of libiq_hip.so: the HIP-event profiler bench.py's roofline leg reads, the experiment
 * knobs that tests, bench.py and the A/B tools under tools/ flip, and a matrix-pipe diagnostic.  They are exported by the same library but are NOT part of the
 * drop-in surface (include/iq.h): nothing in the reference's interface corresponds to them and no product path calls them.
 *
 * State: everything here is state of the CALLING THREAD (thread_local in iq_api.hip, like iq_last_error): a thread that enables
 * the profiler or flips a knob affects only the launches it issues itself; other threads and other processes are untouched.
 * WITHIN that thread a knob applies to every engine: iq_set_tuning(5, v) in particular switches the arithmetic path (bf16x3 <->
 * float32 MFMA twins, fused <-> two-kernel forms) of all later launches of the thread until it is set back - tests and tools
 * select a knob through the context managers of interpret_quality_amd/tuning.py, which check both calls and restore it.
 */
#ifndef IQ_DEBUG_H_
#define IQ_DEBUG_H_

#include "iq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Optional HIP-event profiler (bench.py's roofline leg).  While enabled, iq_pointnet_coalitions
 * brackets its chain-kernel launches with hipEvents recorded on the launch stream.
 * iq_profile_read(slot) synchronises on the recorded events of that slot, returns their summed
 * duration and count, and forgets them.  Slots: 0 = input-STN pre-pool chain, 1 = feature-STN
 * chain, 2 = trunk chain, 3 = whole iq_pointnet_coalitions call. */
int iq_profile_enable(int on);
/* As iq_profile_read, plus the summed `work` (executed FLOP of the MFMA tiles issued) the library attached to the spans
 * of that slot.  Slot 5 = the dominant kernel of a model's step: PointNet++ pn2_group_kernel<128,128,256> (sa2, third
 * scale), DGCNN / GCNN conv5 + pooling GEMM, PointConv pc_group_kernel<128,128,256> (sa2).  Profiler state and the
 * iq_set_tuning knobs belong to the calling thread (like iq_last_error). */
int iq_profile_read_work(int slot, double* total_ms, int* launches, double* total_work);
/* Experiment knob: selects the twin of a product kernel that a test or bench.py uses as a reference, so that the two can be
 * compared or timed interleaved in ONE process.  Value 0 on either key restores the product paths.  Any other (key, value)
 * returns IQ_EINVAL and iq_last_error names it.
 *
 * The key-5 values are the twins listed once in interpret_quality_amd/csrc/iq_twin.h (IQ_TWINS); the names below are the ones
 * interpret_quality_amd/tuning.py selects them by (the enumerator kTwin<Name> in snake case).
 *
 *   key  value  name                     selects
 *   3    1                               dense layers without the LDS-staged GEMM (pn_gemm_lds_kernel)
 *   5    7      edge_gemm_l2             DGCNN EdgeConv as GEMM + L2 gather
 *   5    8      edge_gemm_lds            DGCNN EdgeConv as GEMM + LDS gather
 *   5    12     knn_compact              DGCNN compact-row knn_kernel<8> instead of the region walk
 *   5    14     pc_knn                   PointConv kNN path instead of the walk
 *   5    15     pc_grouped_mlp           PointConv grouped MLP
 *   5    20     knn_fp32_rank            DGCNN kNN ranking in float32 only
 *   5    21     pn2_member_walk          PointNet++ member walk
 *   5    22     knn_fp32_mfma            DGCNN feature-space kNN distances on the fp32 MFMA
 *   5    31     pc_two_kernel            PointConv sa1 contraction and 2048 -> 128 layer as two kernels
 *   5    54     chain_l3_fp32            PointNet chain layer 3 on the fp32 MFMA
 *   5    55     chain_l3_fp32_no_tail16  the same without the 16-row tail tiles
 *   5    56     group_fp32               fp32-MFMA grouped kernels (PointNet++ 32-row chunks, PointConv)
 *   5    57     dense_fp32               dense layers on the fp32 MFMA
 *   5    58     chain_l3_single          bf16x3 chain layer 3 with one n-tile per pass
 *   5    59     dense_tile128            bf16x3 dense layers with 128-row tiles only (the launch before the short tiles;
 *                                        bit-identical results)
 *   5    60     chain_no_dedup           PointNet coalition chains run every repeated coalition of a batch instead of copying the
 *                                        first one's rows (no representatives are sought, every item is its own slot and nothing
 *                                        is expanded; bit-identical results)
 *   5    64     group_fp32_chunk64       PointNet++ fp32-MFMA grouped kernel with 64-row chunks */
int iq_set_tuning(int key, int value);
int iq_profile_read(int slot, double* total_ms, int* launches);

/* Diagnostic: the rate the bf16 matrix pipe SUSTAINS on this board now - a register-only loop of v_mfma_f32_32x32x16_bf16 on
 * random operands, one wave per SIMD on every CU, for about `seconds` (two launches: a calibration, then the measurement; both
 * synchronise the stream).  tflops: dense bf16 TFLOP/s of the measured launch; clock_ghz (optional): shader clock held by its first
 * wave (s_memtime ticks / wall time of the launch).  scratch: device buffer of at least 256 * compute-unit-count floats.  MFMA-dense kernels
 * on MI355X are power-bound: bench.py divides by THIS figure for `frac_of_sustained_bf16_ceiling` instead of a constant. */
int iq_debug_mfma_sustained(double seconds, float* scratch /*device*/, size_t scratch_floats, double* tflops /*host*/,
                            double* clock_ghz /*host or NULL*/, iq_stream_t stream);
/* The same diagnostic per instruction shape: shape = 32 is the loop above (v_mfma_f32_32x32x16_bf16, four accumulator tiles of 16
 * registers per wave), shape = 16 the same loop on v_mfma_f32_16x16x32_bf16 (sixteen tiles of 4 registers: the same 64 accumulator
 * VGPRs, the same operands, the same FLOP per iteration and the same FLOP accounting).  The kernel is power-bound and the two shapes
 * draw different power per FLOP: tools/chain_shape_probe.py alternates them.  Any other shape: IQ_EINVAL. */
int iq_debug_mfma_sustained_shape(int shape, double seconds, float* scratch /*device*/, size_t scratch_floats, double* tflops /*host*/,
                                  double* clock_ghz /*host or NULL*/, iq_stream_t stream);

/* Diagnostic: the representatives iq_pointnet_coalitions finds in a batch of keep masks before its chains run - the same launches
 * from the same launcher, with the caller's scratch in place of the workspace.  rep_out[i] = the lowest j <= i with
 * cloud_of[j] == cloud_of[i] (NULL: one cloud, nclouds must be 1) and (keep[j] ^ keep[i]) clear in its low R bits; items with
 * rep_out[i] != i are the ones the forward does not evaluate: they take the results of item rep_out[i].  keep (B) uint64, cloud_of (B) int32 or
 * NULL, rep_out (B) int32: device.  scratch: device, 4 bytes times the smallest power of two >= max(4, 2 B) - 16 * max(B, 1) bytes
 * always suffice; less is IQ_EWORKSPACE.  No synchronisation. */
int iq_debug_pointnet_reps(const uint64_t* keep /*device*/, const int32_t* cloud_of /*device or NULL*/, int B, int nclouds, int R,
                           int32_t* rep_out /*device*/, void* scratch /*device*/, size_t scratch_bytes, iq_stream_t stream);

/* Diagnostic: the slots iq_pointnet_coalitions then gives the distinct coalitions - the forward's launches again, the caller's scratch
 * in place of the workspace.  slots_out (3 B + 1) int32, device: slot_of[B], slot_of[i] = the number of representatives j == rep[j]
 * below rep[i]; item_u[B], its first U entries the representatives in ascending order; cloud_u[B], its first U entries their clouds
 * (not written when cloud_of is NULL); n_distinct = U.  Entries at U and beyond are not written.  scratch: device,
 * 24 * max(B, 1) + 8 bytes always suffice; less than needed is IQ_EWORKSPACE.  No synchronisation. */
int iq_debug_pointnet_slots(const uint64_t* keep /*device*/, const int32_t* cloud_of /*device or NULL*/, int B, int nclouds, int R,
                            int32_t* slots_out /*device*/, void* scratch /*device*/, size_t scratch_bytes, iq_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* IQ_DEBUG_H_ */
