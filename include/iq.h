/*
 * iq.h - C ABI of libiq_hip.so, the MI355X (gfx950) implementation of the Shapley-value /
 * multi-order-interaction hot path of ada-shen/Interpret_quality.
 *
 * The reference has no FFI of its own: the path sits behind Python functions.
 * Each entry point below therefore names the reference function (file:line, relative to the
 * reference root) whose device work it replaces; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (e.g. torch.Tensor.data_ptr()),
 *    row-major contiguous, unless the parameter is documented as "host";
 *  - no allocation inside the library: scratch memory is a caller-provided workspace.  Every `workspace` / `scratch` / `tmp`
 *    argument may hold anything on entry, and no call writes outside [ptr, ptr + bytes) of the size its *_bytes function
 *    returns; only iq_pointconv_coalitions_cached gives meaning to earlier contents, and only to the first
 *    iq_pointconv_tables_bytes bytes (tests/test_workspace_contents_gpu.py);
 *  - every launch function takes a hipStream_t (passed as void*; NULL = default stream) and is
 *    asynchronous with respect to the host;
 *  - return value: IQ_OK (0) or a negative IQ_E* code; a message for the calling thread's last
 *    error is available from iq_last_error();
 *  - indices are int32 at the ABI (the Python wrappers convert from int64), coalitions are
 *    uint64 bit masks over regions (bit r set = region r kept), so num_regions <= 64 - except at the
 *    iq_*_wide entry points ("Wide coalitions" below), which take rows of ceil(num_regions / 64) words
 *    for up to IQ_MAX_WIDE_REGIONS regions.
 */
#ifndef IQ_H_
#define IQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* iq_stream_t; /* hipStream_t */

enum {
    IQ_OK = 0,
    IQ_EINVAL = -1,      /* bad argument (shape, null pointer, unsupported size) */
    IQ_ELAUNCH = -2,     /* HIP launch or runtime error */
    IQ_EWORKSPACE = -3,  /* workspace too small */
    IQ_EUNSUPPORTED = -4
};

#define IQ_MAX_REGIONS 64
#define IQ_MAX_POINTS 4096
#define IQ_NUM_FEAT 1024
#define IQ_MAX_EXACT_PLAYERS 24
#define IQ_MAX_WIDE_REGIONS 1024   /* iq_*_wide: a coalition is a row of at most 16 words */
#define IQ_KSHAP_SPARSE_MAX_FEATURES 2080   /* iq_kshap_feat_*: the unknowns of a fitted surrogate, 64 + 64 63 / 2 */

/* ABI version: 100 * major + minor.  101 (round 4): every weight descriptor (iq_dense_layer, iq_pointnet_weights, ...) gained
 * optional `*_bf3` fields (weights split into three bf16 terms, iq_pack_weight_bf3).  Descriptors MUST be zero-initialised before
 * they are filled (`iq_dense_layer l = {0};` / memset): a NULL *_bf3 pointer selects the float32-MFMA kernels, a non-NULL one is
 * dereferenced on the device.  A client built against an older header must be rebuilt (the structs grew).
 * 102 (round 5): no layout change; a bf16x3 weight image (iq_pack_weight_bf3) now has its k range padded to a multiple of 32 (only images of layers with cin % 32 == 16 differ, and no kernel consumed those before), dense
 * layers take the image for any cin >= 32 and cout = 256 n or 256 n + 64, iq_knn uses a larger tmp when it is given one, PointNet
 * takes clouds of up to IQ_MAX_POINTS points and PointConv of 64 and more.
 * 103: new entry points, no layout change (the standalone geometric ops: iq_index_points .. iq_density).
 * 104: new entry points, no layout change (exact games by full enumeration: iq_enum_keep_masks .. iq_exact_scratch_bytes).
 * 105: new entry points, no layout change (wide coalitions: iq_prefix_keep_masks_wide .. iq_pointnet_coalitions_wide).
 * 106: new entry point, no layout change (iq_context_keep_masks_wide: the interaction stage of wide games).
 * 107: new entry point, no layout change (iq_pointnet_prefix_coalitions_wide: prefix coalitions straight from permutations).
 * 108: new entry points, no layout change (the other families' compact coalition paths for wide keep rows:
 * iq_dgcnn_coalitions_wide, iq_pointnet2_coalitions_wide, iq_pointconv_coalitions_wide, iq_pointconv_coalitions_cached_wide).
 * 109: new entry points, no layout change (iq_split_packed_weight_bf3, iq_split_packed_weight_bf3_host); the PointNet workspaces
 * grew by the bf16x3 image of fstn.fc3 (iq_pointnet_workspace_bytes, iq_pointnet_wide_workspace_bytes).
 * 110: one new entry point, no layout change (iq_smoothness_enum_wide: the smoothness enumeration of a wide game).
 * 112: one new diagnostic entry point, no layout change and no workspace size changed (iq_debug.h: iq_debug_pointnet_reps).
 * 113: new entry points, no layout change (the device sampler for wide games: iq_sample_wide_workspace_bytes,
 * iq_sample_permutations_wide, iq_context_regions_wide).
 * 114: new entry points, no layout change (the regression estimator of Shapley values: iq_kshap_keep_masks .. iq_kshap_solve).
 * 115: new entry points, no layout change (the regression estimator of wide games: iq_kshap_keep_masks_wide,
 * iq_kshap_scratch_bytes_wide, iq_kshap_moment_wide, iq_kshap_phi_analytic).
 * 116: new entry point, no layout change (the counter-based draw of a wide game's rows: iq_kshap_draw_counter).
 * 117: new entry point, no layout change (the fused PointConv path's inverse density on its own: iq_pointconv_inverse_density).
 * 118: new entry points, no layout change (all-class games on shared coalitions: iq_reward_classes, iq_shapley_games_scratch_bytes,
 * iq_shapley_accum_games).
 * 119: one new diagnostic entry point, no layout change (iq_debug.h: iq_debug_pointnet_slots); the narrow PointNet workspace grew by
 * 12 bytes per coalition (iq_pointnet_workspace_bytes, iq_pointnet_wide_workspace_bytes: the slots of the distinct coalitions).
 * 120: new entry points, no layout change (all-pairs interactions from the regression rows: iq_kshap_pairs_scratch_bytes,
 * iq_kshap_pairs).
 * 121: new entry points, no layout change (standard errors of the sampled estimates: iq_shapley_sq_accum_games,
 * iq_kshap_pairs_se_scratch_bytes, iq_kshap_pairs_se, iq_kshap_moment_se_scratch_bytes_wide, iq_kshap_moment_se_wide).
 * 122: new entry points, no layout change (control variates for the all-pairs map: iq_kshap_pairs_terms, iq_kshap_pairs_terms_se,
 * iq_kshap_pair_features, iq_kshap_pair_gram, iq_kshap_pair_fit_scratch_bytes, iq_kshap_pair_fit, iq_kshap_pair_surrogate,
 * iq_kshap_pair_shift_terms).
 * 123: new entry points, no layout change (sparse regression control variate: iq_kshap_sparse_expand, iq_kshap_feat_gram,
 * iq_kshap_feat_fit_scratch_bytes, iq_kshap_feat_fit, iq_kshap_feat_surrogate). */
#define IQ_ABI_VERSION 123
int iq_version(void);
const char* iq_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Coalition masking
 * ------------------------------------------------------------------------------------------- */

/* Shapley prefix masking: replaces tools/final_common.py:46-61 (mask_data_batch) together with
 * the expand().clone() at :88, and final_shapley_value.py:74-88 (mask_data) for bs = 1.
 * Row o*(R+1)+i of `out` keeps the regions orders[o][0..i-1]; every other point := center.
 * out is (bs*(R+1), N, 3) if channel_first == 0, else (bs*(R+1), 3, N)
 * (the layout after the permute().contiguous() of tools/final_common.py:35). */
int iq_mask_shapley(const float* cloud /*N,3*/, const int32_t* region_id /*N*/,
                    const int32_t* orders /*bs,R*/, const float* center /*3*/, float* out,
                    int N, int R, int bs, int channel_first, iq_stream_t stream);

/* Interaction masking: replaces final_point_binary_interaction_logits.py:45-56.
 * For context k: rows 4k..4k+3 of out (4*nb, 3, N) keep S+{i,j}, S+{i}, S+{j}, S where
 * S = ctx_mask[k] (bit mask over regions) and (i, j) = pairs[k]; masked entries := center. */
int iq_mask_interaction(const float* cloud /*N,3*/, const int32_t* region_id /*N*/,
                        const int32_t* pairs /*nb,2*/, const uint64_t* ctx_mask /*nb*/,
                        const float* center /*3*/, float* out /*4nb,3,N*/,
                        int N, int R, int nb, iq_stream_t stream);

/* Generic coalition masking from explicit keep masks: out row b keeps the regions in keep[b].
 * (Used by the models that consume materialised clouds; PointNet never materialises them.) */
int iq_mask_coalitions(const float* cloud /*N,3*/, const int32_t* region_id /*N*/,
                       const uint64_t* keep /*B*/, const float* center /*3*/, float* out,
                       int N, int B, int channel_first, iq_stream_t stream);

/* Validation of index inputs (region ids in [0,R), permutation / pair entries in [0,R), FPS indices in [0,N)):
 * returns IQ_EINVAL and names the first offending position if any idx[i] lies outside [lo, hi).  The ONE entry point
 * that synchronises `stream` (it reads a 4-byte verdict back); `scratch` = 4 bytes of device memory.  The launch
 * functions themselves never fault on an out-of-range id - such a point is treated as belonging to no region (always
 * masked), an out-of-range order entry is ignored - but their results are then meaningless; callers that take ids from
 * files (region_id.npy, all_orders.npy: tools/final_common.py:120-121) validate once per cloud with this call. */
int iq_check_index_range(const int32_t* idx, size_t count, int lo, int hi, uint32_t* scratch /*4 B, device*/,
                         iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Coalition sampling (on the device)
 * ------------------------------------------------------------------------------------------- */

/* final_shapley_value.py:59-72 (generate_all_orders): S permutations of 0..R-1 drawn from NumPy's legacy global
 * generator, i.e. MT19937 + RandomState.shuffle's back-to-front Fisher-Yates with masked rejection sampling, CONTINUED
 * ON THE DEVICE: mt_state is the generator's state as np.random.get_state() returns it - 624 key words followed by the
 * position (625 uint32, device memory) - and is advanced in place, so permutations and every later host draw (after
 * np.random.set_state with the returned words) are bit-identical to the reference's stream for the same seed.
 * One workgroup (the stream is sequential); 0.40 ms for 1000 permutations of 32 regions. */
int iq_sample_permutations(uint32_t* mt_state /*625*/, int32_t* orders /*S,R*/, int S, int R, iq_stream_t stream);

/* The same draw, same bits in orders and mt_state, spread over many workgroups: only the twist of the generator is sequential.
 * The library allocates nothing, so the caller lends a workspace (device memory, 8-byte aligned, contents irrelevant before and
 * after); iq_sample_workspace_bytes(S, R) is the size at which the wide kernels expect to draw everything.  The number of words
 * a draw consumes is random, the size an estimate: with a smaller workspace (any size, none included) or an unlucky draw the
 * one-workgroup kernel of iq_sample_permutations, which always runs last, draws the rest.  No host synchronisation;
 * 0.075 ms for 1000 permutations of 32 regions (five launches; a call that fits one batch of the one-workgroup kernel, about
 * 100 permutations of 32 regions, stays on it, and iq_sample_workspace_bytes answers 0 for it). */
size_t iq_sample_workspace_bytes(int S, int R);
int iq_sample_permutations_ws(uint32_t* mt_state /*625*/, int32_t* orders /*S,R*/, int S, int R, void* workspace,
                              size_t workspace_bytes, iq_stream_t stream);

/* tools/final_common.py:56-60 as bit masks: keep[s*(R+1) + i] = the regions orders[s][0..i-1]
 * (row 0 = nothing kept = all-centre cloud, row R = the unmodified cloud). */
int iq_prefix_keep_masks(const int32_t* orders /*S,R*/, uint64_t* keep /*S*(R+1)*/, int S, int R, iq_stream_t stream);

/* final_point_binary_interaction_logits.py:45-52 as bit masks: for pair p = (i, j) and its context c = contexts[p][c][0..m-1]
 * (np.in1d(region_id, context)): keep[4(pC + c) + 0..3] = S+{i,j}, S+{i}, S+{j}, S.  m = 0: the empty context. */
int iq_context_keep_masks(const int32_t* pairs /*P,2*/, const int32_t* contexts /*P,C,m*/, uint64_t* keep /*4PC*/,
                          int P, int C, int m, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Reward and reductions
 * ------------------------------------------------------------------------------------------- */

/* tools/final_common.py:11-24 (get_reward).  modified != 0: v = z_y - logsumexp(z_{!=y});
 * modified == 0 ("normal"): v = log_softmax(z)[y]. */
int iq_reward(const float* logits /*B,C*/, int label, int modified, float* v /*B*/,
              int B, int C, iq_stream_t stream);

/* tools/final_common.py:92-96 and final_shapley_value.py:145-150: dv = v[1:] - v[:-1] per
 * permutation (float32), scattered by the permutation into float64 rows and summed over the
 * permutations IN ORDER (bit-stable, matches the host loop of the reference).
 *   sv_rows  (S,R) float64  = the rows of region_sv_all.npy        (may be NULL)
 *   phi_sum  (R,)  float64  = sum over the S permutations (not divided)
 *   snaps    (n_snap,R) float64 = running sums after snap_counts[k] permutations (may be NULL),
 *            i.e. what save_shapley (final_shapley_value.py:91-106) divides by count. */
int iq_shapley_accum(const float* v /*S*(R+1)*/, const int32_t* orders /*S,R*/,
                     double* sv_rows, double* phi_sum, const int32_t* snap_counts, int n_snap,
                     double* snaps, int R, int S, iq_stream_t stream);

/* iq_reward for G labels of the same logits - the G games a forward has already paid for: v[g*ldv + b] is what
 * iq_reward(logits, labels[g], modified, ...) writes to v[b], bit for bit (the same maximum and sum over c ascending with the
 * label skipped when modified, the same |m| == inf rule and final association; in normal mode maximum and sum do not depend
 * on the label and are taken once per row).  labels: HOST pointer to G labels in [0, C), in any order, repeats allowed; they
 * travel by value in the kernel arguments.  NULL = the labels 0 .. C-1, and G must equal C.  v: G rows of ldv >= B floats; the
 * floats b >= B of a row are not touched, so a (G, M) table is filled one chunk of coalitions at a time (v + first, ldv = M).
 * A row of logits is staged once in LDS for its G labels; stores are coalesced along b.
 * Checks (IQ_EINVAL, nothing launched): 2 <= C <= 64, 1 <= G <= 64, every label in [0, C), ldv >= B.  B == 0 is IQ_OK. */
int iq_reward_classes(const float* logits /*B,C*/, const int32_t* labels /*HOST: G, or NULL*/, int G, int modified,
                      float* v /*G rows of ldv*/, size_t ldv, int B, int C, iq_stream_t stream);

/* iq_shapley_accum / iq_shapley_accum_wide for G games on the same permutations: game g's rewards are v + g*ldv
 * (ldv >= S*(R+1): the (G, M) table iq_reward_classes fills), its outputs phi_sum + g*R and snaps + g*n_snap*R, and they carry
 * the bits iq_shapley_accum_wide gives for v + g*ldv alone - for R <= 64 also iq_shapley_accum's: float32 differences, widened
 * to float64, added per region strictly in permutation order.  1 <= R <= IQ_MAX_WIDE_REGIONS (one entry for narrow and wide
 * games), S >= 0, 1 <= G <= 65535; snap_counts ascending.  There is no sv_rows output: no (S,R) float64 row table exists, for
 * any game.  One kernel inverts the permutations once for all games into a 16-bit (S,R) position table - that is the whole
 * scratch, iq_shapley_games_scratch_bytes(R, S, G) (0 for refused arguments), which therefore does not grow with G - and a grid
 * of (ceil(R/64), G) workgroups runs the staged sum of iq_shapley_accum, reading v[g][o*(R+1)+p+1] - v[g][o*(R+1)+p] through
 * the table.  A region that a row does not name contributes 0.0; an order entry outside [0, R) is skipped and nothing is read
 * out of bounds.  No atomics, nothing allocated, no host synchronisation. */
size_t iq_shapley_games_scratch_bytes(int R, int S, int G);
int iq_shapley_accum_games(const float* v /*G rows of ldv*/, size_t ldv, const int32_t* orders /*S,R*/, double* phi_sum /*G,R*/,
                           const int32_t* snap_counts, int n_snap, double* snaps /*G,n_snap,R*/, int R, int S, int G,
                           void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* The second moment beside iq_shapley_accum_games, for the standard error of the permutation estimator: the same arguments,
 * position table, scratch size and skip rules, with sq_sum[g][r] = sum over the permutations p, strictly in permutation order, of
 * ((double)dv)^2, dv the float32 difference iq_shapley_accum_games adds for (g, p, r) - the square of a widened float32 is exact
 * in float64 - and sq_snaps the running sums at snap_counts.  At a count n >= 2 the host forms
 * se_r = sqrt(max(sq - sum^2 / n, 0) / (n (n - 1))) from the two sums. */
int iq_shapley_sq_accum_games(const float* v /*G rows of ldv*/, size_t ldv, const int32_t* orders /*S,R*/, double* sq_sum /*G,R*/,
                              const int32_t* snap_counts, int n_snap, double* sq_snaps /*G,n_snap,R*/, int R, int S, int G,
                              void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* final_cal_interactions.py:28-36: I[k] = ((v[4k] + v[4k+3]) - v[4k+1]) - v[4k+2] in float32. */
int iq_interaction_reduce(const float* v /*4n*/, float* out /*n*/, int n, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Geometry
 * ------------------------------------------------------------------------------------------- */

/* final_shapley_value.py:20-35 (cal_region_id) with tools/final_util.py:134-147: nearest FPS
 * centre per point by the expanded-form squared distance, first index on ties. */
int iq_region_assign(const float* cloud /*N,3*/, const int32_t* fps_idx /*R*/,
                     int32_t* region_id /*N*/, int N, int R, iq_stream_t stream);

/* final_save_fps.py:10-31 (= models/pointnet2.py:45-68): farthest point sampling, start index 0,
 * ties -> lowest index.  xyz (B,N,3) -> idx (B,S). */
int iq_fps(const float* xyz, int32_t* idx, int B, int N, int S, iq_stream_t stream);

/* final_smoothness_center_enum_all.py:183-242 (update_region) for every region and every epoch of
 * test_all_region's loop (:303-335) in one launch: gradient ascent (objective +1) / descent (-1) on the
 * linearity (mode 0) / planarity (1) / scattering (2) of each region's points, under the reference's
 * variance bounds (:66-82), distance bound (:102-118) and stop conditions (:163-180).  The constants are
 * the reference's module-level STEP .. MAX_ITERATION (:13-19).  Regions only move their own points, so
 * epoch e of region r does not depend on other regions.  Outputs:
 *   data_out   (epochs,N,3)  the cloud after epoch e (data_list, :326)
 *   smooth_out (epochs,R)    smoothness of region r recorded in epoch e (smoothness_list, :325)
 *   var_out    (epochs,R,3)  last variances on o1,o2,o3 (the "var1: .." log line, :239)
 *   orig_out   (R,4)         original variances on o1,o2,o3 and original smoothness (:256-261)
 *   stop_epoch (R)           epoch in which the region stopped updating (indicator False), `epochs` if it
 *                            never did, -1 for a region of fewer than two points (left untouched;
 *                            the reference cannot process such a region)
 * The caller evaluates epochs 0 .. min(epochs, max_r stop_epoch + 1) - 1, as the break at :333-334 does.
 * `origin` (optional) restarts the enumeration from an already deformed `cloud`: orientations, variance
 * bounds, the distance bound and the first target are taken from `origin` (NULL: from `cloud`).
 * Every region_id[i] must lie in [0, R); neither entry point checks it (iq_check_index_range does, and hip_ops.smoothness_enum
 * calls it before the launch).  A point with an id outside [0, R) belongs to no region: it takes no part in any region's
 * covariance or step, the launch copies its row of `cloud` into every epoch of data_out, and rc is still 0. */
typedef struct iq_smoothness_params {
    double step;           /* STEP = 1e-3 */
    double enum_step;      /* ENUM_STEP = 0.05 */
    double var_threshold;  /* VAR_THRESHOLD = 0.003 */
    double dist_threshold; /* DIST_THRESHOLD = 0.03 */
    double stop_ratio;     /* STOP_RATIO = 0.5 */
    int32_t epochs;        /* EPOCH = 50 */
    int32_t max_iteration; /* MAX_ITERATION = 100 */
    int32_t project_to_bound; /* 0 = as the reference behaves: points beyond dist_threshold are counted (stop
                                 condition) but stay where they are, because its write-back at :117 assigns to a
                                 temporary view; 1 = project them back onto the sphere as :110-117 intends */
    int32_t reserved;
} iq_smoothness_params;
int iq_smoothness_enum(const float* cloud /*N,3*/, const float* origin /*N,3 or NULL*/, const int32_t* region_id /*N*/, int N, int R, int mode,
                       int objective, const iq_smoothness_params* prm, float* data_out, float* smooth_out,
                       float* var_out, float* orig_out, int32_t* stop_epoch, iq_stream_t stream);
/* The same enumeration for a wide game ("Wide coalitions" below): the same arguments and outputs, 1 <= R <= IQ_MAX_WIDE_REGIONS.
 * Both entry points take 1 <= N <= 1024 - a region's points live in the kernel's LDS arrays - and launch the same kernel, one
 * wave per region; a region's trajectory reads only that region's points, so for R <= 64 the five outputs are
 * iq_smoothness_enum's bit for bit.  Above a few hundred regions many regions hold fewer than two points: stop_epoch -1, NaN. */
int iq_smoothness_enum_wide(const float* cloud /*N,3*/, const float* origin /*N,3 or NULL*/, const int32_t* region_id /*N*/, int N, int R,
                            int mode, int objective, const iq_smoothness_params* prm, float* data_out, float* smooth_out,
                            float* var_out, float* orig_out, int32_t* stop_epoch, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PointNet (models/pointnet.py:11-115) - fused fp32-MFMA forward over coalitions
 * ------------------------------------------------------------------------------------------- */

/* One dense layer y = act(W x + b), BatchNorm(eval) already folded in.  `w` is in the library's
 * MFMA B-fragment order (iq_pack_weight), `b` has cout_padded entries. */
typedef struct iq_dense_layer {
    const float* w;
    const float* b;
    int32_t cin;
    int32_t cout;
    const void* w_bf3;   /* optional (NULL: fp32 MFMA): the same weights as three bf16 terms (iq_pack_weight_bf3); wide layers
                          * (cout a multiple of 256, cin >= 32) then take their products on the bf16 matrix pipe,
                          * float32-exact; cout = 256 n + 64: the first 256 n columns do, the last 64 stay on the fp32 MFMA */
} iq_dense_layer;

typedef struct iq_pointnet_weights {
    const float* stn_in;  /* [64][4] = (w0,w1,w2,bias) of feat.stn.conv1+bn1 */
    iq_dense_layer stn_c2, stn_c3, stn_fc1, stn_fc2, stn_fc3;       /* fc3 bias includes +I */
    const float* feat_in; /* [64][4] of feat.conv1+bn1 */
    iq_dense_layer fstn_c1, fstn_c2, fstn_c3, fstn_fc1, fstn_fc2, fstn_fc3; /* fc3: iq_pack_fstn_fc3.  feature_transform = False
        (models/pointnet.py:62-63): fstn_c1.w = NULL and fstn_fc3.b = the packed identity (iq_pack_fstn_fc3 of a zero layer) */
    iq_dense_layer feat_c2, feat_c3, cls_fc1, cls_fc2, cls_fc3;
    /* optional (NULL: fp32 MFMA): the folded 128 -> 1024 layers of the feature STN and of the trunk as three bf16 terms
     * (iq_pack_weight_bf3): layer 3 of the coalition chains - 91 % of their work - then runs on the bf16 matrix pipe, float32-exact */
    const void* fstn_c3_bf3;
    const void* feat_c3_bf3;
    /* optional, used together with the two above: the 64 -> 128 layers before them, likewise */
    const void* fstn_c2_bf3;
    const void* feat_c2_bf3;
} iq_pointnet_weights;

/* out (M,ldo) = act(A (M,lda) . W^T + b): the dense layer every model kernel shares (1x1 convolutions and
 * fully connected layers with BatchNorm folded: models/pointnet.py:24-29, models/dgcnn.py:66-80,
 * models/pointnet2.py:163-170 ...), exposed for tests and callers that fold their own layers.
 * act: 0 none, 1 ReLU, 2 LeakyReLU(0.2).  Device pointers; L->cin % 8 == 0. */
int iq_linear(const float* A, int lda, const iq_dense_layer* L, float* out, int ldo, int M, int act,
              iq_stream_t stream);

/* Host-side packing helpers (host pointers).  iq_packed_floats = number of floats of the packed
 * image of a (cout, cin) weight; cin must be a multiple of 8. */
size_t iq_packed_floats(int cout, int cin);
int iq_padded_cout(int cout);
int iq_pack_weight(const float* w_host /*cout,cin*/, float* out_host, int cout, int cin);
/* The same weight as THREE bf16 terms (h = bf16(w), m = bf16(w - h), l = bf16(w - h - m), round to nearest even: 24 mantissa bits)
 * in the fragment order of v_mfma_f32_32x32x16_bf16: [term][n-tile][k-step of 16][lane][8], iq_packed_bf3_elems 16-bit elements.
 * A layer that is given it (iq_dgcnn_weights.conv5_bf3) takes its products on the bf16 matrix pipe - six exact bf16 products
 * per float32 product, float32 accumulation: float32 accuracy at 3/8 of the matrix cycles of the fp32 MFMA.  cin % 8 == 0; the image's
 * k range is cin rounded up to a multiple of 32, zero beyond cin (the dense layer never reads A's columns there). */
size_t iq_packed_bf3_elems(int cout, int cin);
int iq_pack_weight_bf3(const float* w_host /*cout,cin*/, unsigned short* out_host, int cout, int cin);
/* The same image derived from the layer's float32 image (iq_pack_weight order) ON THE DEVICE: packed_w and out_bf3 are device
 * pointers (iq_packed_floats and iq_packed_bf3_elems elements), byte for byte what iq_pack_weight_bf3 gives for the weight that
 * packed_w was packed from.  iq_pointnet_coalitions derives fstn.fc3's bf16x3 image this way, once per call, into its workspace.
 * _host: the same maps and split in a host loop over host pointers (for checks without a device). */
int iq_split_packed_weight_bf3(const float* packed_w, unsigned short* out_bf3, int cout, int cin, iq_stream_t stream);
int iq_split_packed_weight_bf3_host(const float* packed_w_host, unsigned short* out_host, int cout, int cin);
/* feat.fstn.fc3 (4096 x 256): permutes the output rows so that the layer's output vector IS the
 * packed B-fragment image of trans_feat for the trunk's per-coalition 64x64 product, and adds the
 * identity (models/pointnet.py:42-45) into the bias.  out_w has iq_packed_floats(4096,256)
 * floats, out_b 4096.  perm_host[r] (4096 int32, may be NULL) receives the source row of output
 * row r, so a caller can undo the permutation. */
int iq_pack_fstn_fc3(const float* w_host, const float* b_host, float* out_w, float* out_b,
                     int32_t* perm_host);

/* Workspace (bytes) needed by iq_pointnet_coalitions for B coalitions over nclouds clouds. */
size_t iq_pointnet_workspace_bytes(int B, int nclouds, int N, int R);

/* Logits of B coalitions without materialising the masked clouds.  Replaces, for PointNet, the
 * chain mask_data_batch -> cal_reward -> model(...) of tools/final_common.py:88-91 and
 * final_point_binary_interaction_logits.py:45-60.
 *   clouds    (nclouds, N, 3) if channel_first == 0, else (nclouds, 3, N)
 *   centers   (nclouds, 3)   the point every masked point collapses onto
 *   region_id (nclouds, N)   int32 in [0, R)
 *   keep      (B,) uint64    bit r set = region r keeps its points
 *   cloud_of  (B,) int32     cloud index of each coalition (NULL = all 0)
 *   logits    (B, 10)
 *   trans_feat_packed (B, 4096) optional output (NULL to skip): packed image of trans_feat
 * Exact with respect to the dense evaluation of the same kernels: identical points produce
 * identical features and max-pooling ignores duplicates. */
int iq_pointnet_coalitions(const iq_pointnet_weights* w /*host struct of device pointers*/,
                           const float* clouds, const float* centers, const int32_t* region_id,
                           const uint64_t* keep, const int32_t* cloud_of, float* logits,
                           float* trans_feat_packed, void* workspace, size_t workspace_bytes,
                           int B, int nclouds, int N, int R, int channel_first,
                           iq_stream_t stream);

/* The same with PointNetfeat's `crt_points` (models/pointnet.py:83: the arg-max of the trunk's max-pool, third element of
 * PointNetCls's output tuple): crt_points (B, 1024) int32 receives, per coalition and channel, the index of the point that
 * attains the maximum (largest value, then the first in region-sorted row order = lowest point index for the dense
 * forward, where all points share one region); index N stands for the centre that masked points collapse to.  NULL = the
 * entry point above.  The hot-path callers discard crt_points (tools/final_common.py:36-37); the arg-max variant of the
 * trunk kernel costs a few percent and is only instantiated for this entry point. */
int iq_pointnet_coalitions_crt(const iq_pointnet_weights* w, const float* clouds, const float* centers,
                               const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of, float* logits,
                               float* trans_feat_packed, int32_t* crt_points, void* workspace, size_t workspace_bytes,
                               int B, int nclouds, int N, int R, int channel_first, iq_stream_t stream);

/* Algorithmic FLOP of the dense reference network per coalition (0.879 GFLOP at
 * N = 1024), the basis of bench.py's roofline figures. */
double iq_pointnet_flops_per_coalition(int N);

/* ---------------------------------------------------------------------------------------------
 * PointNet++ MSG (models/pointnet2.py:12-276)
 * ------------------------------------------------------------------------------------------- */

/* models/pointnet2.py:70-91 (query_ball_point): for every centroid the K LOWEST-INDEX points with
 * squared distance <= radius^2 (expanded form -2 c.p + |c|^2 + |p|^2), padded with the first hit.
 * xyz (B,N,3), new_xyz (B,S,3) -> idx (B,S,K) int32. */
int iq_ball_query(const float* xyz, const float* new_xyz, float radius, int K, int32_t* idx,
                  int B, int N, int S, iq_stream_t stream);

/* One scale of a multi-scale set abstraction: layer 1 = relu(w1x . (x_p - c) [+ U_p]), then the
 * dense layers l2, l3 (BN folded, packed), max over the `nsample` members. */
typedef struct iq_pn2_scale {
    const float* w1x;      /* [C1][4] = (wx0, wx1, wx2, bias); bias = 0 when the per-point part U carries it */
    iq_dense_layer l2, l3;
    float radius;
    int32_t nsample;
} iq_pn2_scale;

typedef struct iq_pointnet2_weights {
    iq_pn2_scale sa1[3];
    iq_dense_layer sa2_u;  /* 320 -> 64+128+128: feature part of layer 1 of the three sa2 scales (+bias) */
    iq_pn2_scale sa2[3];
    iq_dense_layer sa3_l1, sa3_l2, sa3_l3;  /* 643 (zero-padded to 648: [xyz, features]) -> 256 -> 512 -> 1024 */
    iq_dense_layer fc1, fc2, fc3;
    /* optional (NULL: fp32 MFMA): layers 2 and 3 of an sa2 scale as three bf16 terms (iq_pack_weight_bf3); a 128-128-256 scale
     * that has both runs its grouped MLP on the bf16 matrix pipe, float32-exact (pn2_group_bf3_kernel) */
    const void* sa2_l2_bf3[3];
    const void* sa2_l3_bf3[3];
} iq_pointnet2_weights;

size_t iq_pointnet2_workspace_bytes(int B);

/* Eval-mode PointNet2ClsMsg.forward (models/pointnet2.py:264-276) on B materialised clouds.
 * xyz (B,N,3) channel-LAST (what iq_mask_* writes with channel_first = 0) -> logits (B,10). */
int iq_pointnet2_forward(const iq_pointnet2_weights* w /*host struct of device pointers*/, const float* xyz,
                         float* logits, void* workspace, size_t workspace_bytes, int B, int N,
                         iq_stream_t stream);

/* The same network on B coalitions given as region bit masks (argument convention of iq_pointnet_coalitions):
 * replaces the masking + forward of tools/final_common.py:88-91 and
 * final_point_binary_interaction_logits.py:45-60 for PointNet++.  The masked clouds are written internally
 * (FPS, ball query and sa2 / sa3 run on them as in iq_pointnet2_forward), but sa1 - which has no input
 * features, so a member row is a function of the point pair only - is a gather-max over per-source-cloud tables
 * MLP_s(P[q] - P[p]) of all pairs inside each radius (P = the cloud's points plus the centre masked points
 * collapse to), built once per call with the ball query's own distance expression and the grouped kernel's layer
 * arithmetic: bit-identical features.  A scale whose pair count exceeds the table capacity (192 pairs per point
 * on average) falls back to the grouped MLP.  Reads the pair counts back once per call (the only host round
 * trip); otherwise asynchronous on `stream`. */
size_t iq_pointnet2_coalitions_workspace_bytes(int B, int nclouds, int N);
int iq_pointnet2_coalitions(const iq_pointnet2_weights* w, const float* clouds, const float* centers,
                            const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of,
                            float* logits, void* workspace, size_t workspace_bytes, int B, int nclouds, int N,
                            iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DGCNN / GCNN (models/dgcnn.py:12-194)
 * ------------------------------------------------------------------------------------------- */

/* models/dgcnn.py:12-18 (knn): the k = 20 largest of -|x_i|^2 - (-2 x_i.x_j) - |x_j|^2 per row, self
 * included, as an (unordered) index set.  x (B,N,C) row-major with C in {3, 64, 128}; idx (B,N,20)
 * int32; tmp = scratch of at least B*N*84 + 16*B + 8192 bytes; with B*N*C*6 bytes more (C = 64, 128) the inner products run on
 * the bf16 matrix pipe as three-term bf16 products, float32-accurate, as they do inside iq_dgcnn_* (csrc/iq_dgcnn_knn.h: knn_kernel
 * <.., BF3>; iq_set_tuning(5, 22): the fp32 MFMA kernels).  Both arithmetics stand in front of the same exact re-ranking:
 * Feature-space graphs (C = 64, 128): where the float32 expanded form cannot separate the 20th from the 21st nearest
 * (gap below 1e-5 of the magnitude of the summed terms: rounding noise decides for the reference's float32 path too), the
 * query's 21 best candidates are re-ranked by -sum (x_i - x_j)^2 accumulated in float64, i.e. the order the reference
 * finds in float64 (csrc/iq_dgcnn_knn.h: knn_refine_kernel, 0.7 % of the queries; iq_set_tuning(5, 20) keeps the float32
 * ranking, for A/B runs).  Standing in front of that re-ranking, the float32 selection of these two cases compares distances in
 * buckets of 32 ulps (3.8e-6 relative; csrc/iq_topk.h: TaggedTopK) - a fifth of the narrowest re-ranked band; C = 3 is exact. */
int iq_knn(const float* x, int32_t* idx, void* tmp, size_t tmp_bytes, int B, int N, int C, int k,
           iq_stream_t stream);

/* pq[l]: layer l's EdgeConv as ONE dense layer over the points with 2*Cout outputs
 * [P = (s.W_a) x ; Q = (s.(W_b - W_a)) x + t] (BN folded; see csrc/iq_dgcnn.hip, csrc/iq_edgeconv.h); conv5/fc1/fc2 are
 * followed by LeakyReLU(0.2). */
typedef struct iq_dgcnn_weights {
    iq_dense_layer pq[4];
    iq_dense_layer conv5, fc1, fc2, fc3;
    int32_t k;
    int32_t reserved;
    const void* conv5_bf3;    /* optional (NULL: fp32 MFMA): conv5's folded weights as three bf16 terms, iq_pack_weight_bf3 */
} iq_dgcnn_weights;

size_t iq_dgcnn_workspace_bytes(int B, int N);

/* Eval-mode DGCNN_cls.forward (models/dgcnn.py:83-120; fixed_graph = 0) or GCNN_cls.forward
 * (:156-194; fixed_graph = 1: one xyz graph for all four EdgeConv layers) on B materialised clouds.
 * xyz (B,N,3) channel-last -> logits (B,10).  Any 20 <= N <= 32767 (clouds are padded to a multiple of 32 rows
 * internally with rows no query can select). */
int iq_dgcnn_forward(const iq_dgcnn_weights* w /*host struct of device pointers*/, const float* xyz,
                     float* logits, void* workspace, size_t workspace_bytes, int B, int N,
                     int fixed_graph, iq_stream_t stream);

/* The same network on B coalitions WITHOUT materialising the masked clouds (the argument convention of
 * iq_pointnet_coalitions: clouds (nclouds,N,3), centers (nclouds,3), region_id (nclouds,N), keep (B) region
 * bit masks, cloud_of (B) or NULL when nclouds is 1 or B).  Replaces the masking + forward of
 * tools/final_common.py:88-91 and final_point_binary_interaction_logits.py:45-60 for DGCNN / GCNN.  A masked
 * cloud is its kept points plus M copies of the centre that behave identically in every layer, so each
 * coalition runs on kept + min(M,20) rows (exact: neighbourhood max and max-pool are set operations, the
 * mean pool weights the centre by M).  Same workspace as iq_dgcnn_forward(B, N). */
int iq_dgcnn_coalitions(const iq_dgcnn_weights* w, const float* clouds, const float* centers,
                        const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of, float* logits,
                        void* workspace, size_t workspace_bytes, int B, int nclouds, int N, int fixed_graph,
                        iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * PointConv with density (models/pointconv.py:103-424)
 * ------------------------------------------------------------------------------------------- */

/* One PointConvDensitySetAbstraction (BN folded).  Layer 1 of the shared MLP is split:
 * relu(w1x . (x_p - c) + U_p) with U = u(features) (bias inside; sa1 has no features: bias in w1x[3]).
 * densitynet: rows [w | b] of 1->16->8->1 (32 + 136 + 9 floats); weightnet: 3->8->8->16 (32 + 72 + 144). */
typedef struct iq_pointconv_sa {
    const float* w1x;         /* [C1][4] = (wx0, wx1, wx2, bias) */
    iq_dense_layer u;         /* features -> C1 (unused for sa1) */
    iq_dense_layer l2, l3;
    const float* densitynet;
    const float* weightnet;
    iq_dense_layer linear;    /* 16*C3 -> C3, + bn_linear, ReLU */
    float bandwidth;
    int32_t nsample;          /* 32, 64, 0 = group all */
} iq_pointconv_sa;

typedef struct iq_pointconv_weights {
    iq_pointconv_sa sa[3];
    iq_dense_layer fc1, fc2, fc3;
    /* optional (NULL: fp32 MFMA): layers 2 and 3 of sa[1] (128 -> 128 -> 256) as three bf16 terms (iq_pack_weight_bf3): its
     * grouped MLP then runs on the bf16 matrix pipe, float32-exact (pc_group_bf3_kernel) */
    const void* sa2_l2_bf3;
    const void* sa2_l3_bf3;
} iq_pointconv_weights;

size_t iq_pointconv_workspace_bytes(int B, int N);

/* Eval-mode PointConvDensityClsSsg.forward (models/pointconv.py:414-424) on B materialised clouds.
 * xyz (B,N,3) channel-last -> logits (B,10). */
int iq_pointconv_forward(const iq_pointconv_weights* w /*host struct of device pointers*/, const float* xyz,
                         float* logits, void* workspace, size_t workspace_bytes, int B, int N,
                         iq_stream_t stream);

/* Logits of B coalitions given as region bit masks over nclouds source clouds - the same call as
 * iq_pointnet2_coalitions / iq_dgcnn_coalitions; replaces mask_data_batch + model(...) of tools/final_common.py:46-61,
 * 26-43 and final_point_binary_interaction_logits.py:45-60 for PointConv.  The masked clouds are written into the
 * workspace and run through the forward of iq_pointconv_forward.  When a few source clouds serve many coalitions
 * (nclouds <= 8, or nclouds * 8 <= B) the K-nearest groups of sa1 and sa2 (models/pointconv.py:103-114) are read off per-source-cloud
 * sorted neighbour lists, built once per call with the kNN kernel's own distance expression: in xyz space neither the
 * distance between two points nor the centre depends on the coalition, only the candidate set does (the same point
 * sets as the kNN kernel up to ties; masked points are interchangeable).  With at most eight source clouds sa1's MLP rows
 * - functions of (member point, centroid point) only, sa1 having no input features - come from a table of all (N+1)^2
 * pairs (0.54 GB of workspace per source cloud) and a group is 32 table rows contracted with the members' density x
 * WeightNet weights, in one kernel with the 2048 -> 128 layer behind it.  64 <= N <= 1024 (fewer than 512 points: sa1's
 * farthest point sampling returns index 0 once the points are used up, models/pointconv.py:54-77, and so does this).  Asynchronous on `stream`. */
size_t iq_pointconv_coalitions_workspace_bytes(int B, int nclouds, int N);
int iq_pointconv_coalitions(const iq_pointconv_weights* w, const float* clouds, const float* centers,
                            const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of, float* logits,
                            void* workspace, size_t workspace_bytes, int B, int nclouds, int N, iq_stream_t stream);
/* The same call for several launches on the SAME source clouds (the chunks of one interaction setting,
 * final_point_binary_interaction_logits.py:37-66; the batches of one pose, tools/final_common.py:78-96).  The per-cloud
 * structures (padded rows, sorted neighbour lists, pair tables) occupy the first iq_pointconv_tables_bytes(nclouds, N) bytes of
 * `workspace`, whatever B is.  `tables_state` (HOST int, in / out; NULL = build everything, keep nothing): bit 0 = the lists,
 * bit 1 = the pair tables are already there for exactly these clouds, centers, nclouds and N - the caller's promise (same
 * workspace base, bytes untouched since the call that set the bit).  Missing parts are built and their bits set.
 * Bits 2-3 (in, returned unchanged) name how the K-nearest groups are formed: 0 = decided from THIS launch (the sorted-list walk
 * when nclouds <= 8 or nclouds * 8 <= B, else a per-coalition kNN), 1 = always the walk, 2 = never.  The two sum a group's members
 * in a different order (results equal to rounding, not bitwise): a caller that splits ONE batch over several launches and wants
 * launch-size-independent bits passes 1 or 2 on every launch (interpret_quality_amd/pointconv.py decides from the whole batch). */
size_t iq_pointconv_tables_bytes(int nclouds, int N);
int iq_pointconv_coalitions_cached(const iq_pointconv_weights* w, const float* clouds, const float* centers,
                                   const int32_t* region_id, const uint64_t* keep, const int32_t* cloud_of, float* logits,
                                   void* workspace, size_t workspace_bytes, int B, int nclouds, int N, int* tables_state,
                                   iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Standalone geometric ops of the model files (the building blocks the fused model kernels use
 * internally, for callers that keep their own PyTorch modules)
 *
 * Every index read is guarded: an index outside [0, N) never addresses memory, and every output
 * element that depends on one is written as NaN (iq_sort_neighbours: the row is left as it is).
 * The Python front end validates caller indices with iq_check_index_range before it launches.
 * Float outputs must be 16-byte aligned (every torch allocation is).
 * ------------------------------------------------------------------------------------------- */

/* models/pointnet2.py:27-43 and models/pointconv.py:35-52 (index_points):
 * out[b,m,:] = points[b, idx[b,m], :].  points (B,N,C), any C >= 1; idx (B,M) int32 where M is the
 * product of the reference's trailing index dims; out (B,M,C).  B*M*C < 2^31. */
int iq_index_points(const float* points, const int32_t* idx, float* out, int B, int N, int M, int C,
                    iq_stream_t stream);

/* Grouping: models/pointnet2.py:93-137 (sample_and_group / _all), models/pointconv.py:117-197
 * (sample_and_group / _all / group) with xyz_first = 1, and PointNetSetAbstractionMsg.forward
 * (models/pointnet2.py:222-230) with xyz_first = 0.  Row (b,s,k) of out (B,S,K,3+D) is
 * [xyz[b,i] - c, points[b,i]] (xyz_first) or [points[b,i], xyz[b,i] - c] with i = idx[b,s,k] and
 * c = new_xyz[b,s]: one float32 subtraction per coordinate, as the reference's.  new_xyz = NULL:
 * nothing subtracted; idx = NULL: all N points in order (S = 1, K = N); points = NULL: D = 0.
 * B*S*K*(3+D) < 2^31. */
int iq_group_points(const float* xyz /*B,N,3*/, const float* points /*B,N,D*/, const float* new_xyz /*B,S,3*/,
                    const int32_t* idx /*B,S,K*/, float* out, int xyz_first, int B, int N, int S, int K, int D,
                    iq_stream_t stream);

/* models/dgcnn.py:21-47 (get_graph_feature) for a given idx:
 * out[b,c,n,j] = x[b,c,idx[b,n,j]] - x[b,c,n] and out[b,C+c,n,j] = x[b,c,n] (c < C).
 * x is (B,C,N) if channel_first, else (B,N,C); idx (B,N,k) int32; out (B,2C,N,k).  B*2C*N*k < 2^31. */
int iq_edgeconv_gather(const float* x, const int32_t* idx, float* out, int channel_first, int B, int N, int C,
                       int k, iq_stream_t stream);

/* models/pointconv.py:103-114 (knn_point): per query the K nearest keys by square_distance(new_xyz, xyz)
 * in the reference's op order (the region assignment's expression), SORTED nearest first, ties to the
 * lower index (the reference returns the same set unsorted).  xyz (B,N,3), new_xyz (B,S,3) -> idx
 * (B,S,K) int32.  1 <= N <= IQ_MAX_POINTS, 1 <= K <= min(N, 128).  tmp / tmp_bytes: reserved, the
 * kernel needs no scratch (NULL, 0). */
int iq_knn_point(const float* xyz, const float* new_xyz, int K, int32_t* idx, void* tmp, size_t tmp_bytes,
                 int B, int N, int S, iq_stream_t stream);

/* The order of models/dgcnn.py:12-18 (knn: topk(sorted=True)) for an index set that iq_knn returns
 * unordered: each row of idx (B,S,k) int32 is reordered in place nearest first by the float32
 * distance in the association of -xx - inner - xx^T: (|x|^2 + (-2 q.x)) + |q|^2 (channel-sequential
 * sums, the dot product as an fma chain), ties to the lower index.  q (B,S,C), keys (B,N,C); for knn(x) both are x as (B,N,C).
 * 1 <= k <= 128, N <= 2^24. */
int iq_sort_neighbours(const float* q, const float* keys, int32_t* idx, int B, int N, int S, int C, int k,
                       iq_stream_t stream);

/* models/pointconv.py:199-209 (compute_density): out[b,i] = mean_j exp(-d_ij / (2h^2)) / (2.5h) with
 * d = square_distance(xyz, xyz) - the density itself (the fused PointConv path keeps its inverse).
 * Within 2e-6 relative of the reference.  xyz (B,N,3) -> out (B,N); B <= 65535. */
int iq_density(const float* xyz, double bandwidth, float* out, int B, int N, iq_stream_t stream);

/* The kernel the fused PointConv path (iq_pointconv_forward, iq_pointconv_coalitions) runs in front of each DensityNet, on its own:
 * out[b,i] = 1 / iq_density's value, the sum taken as exp2(d * k) on the hardware exponential with one division at the end.  The
 * bandwidth is rounded to float32, as the weights hold it.  xyz (B,N,3) -> out (B,N); B <= 65535, N <= 3072. */
int iq_pointconv_inverse_density(const float* xyz, double bandwidth, float* out, int B, int N, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Exact games by full enumeration (csrc/iq_lattice.hip)
 *
 * The reference only ever SAMPLES its game: 1000 permutations per cloud (final_shapley_value.py:59-72, 138-156), at most
 * 100 contexts per pair and order (final_gen_pair.py:25-41).  With n <= IQ_MAX_EXACT_PLAYERS players the game can be
 * enumerated instead.  Coalition index c in [0, 2^n) has bit k set when player k is present; v[c] is the float32 reward
 * (iq_reward) of coalition c.  The three reductions accumulate in float64 in an order that depends on (n, P) only - no
 * floating-point atomics - so two calls give the same bits, however the table was produced.  n = 1 and n = 2 work.
 * v must be 8-byte aligned (every torch allocation is).
 * ------------------------------------------------------------------------------------------- */

/* keep[b] = base | (the regions players[k] of every set bit k < n of first + b), b < count <= 2^30: the keep masks every
 * iq_*_coalitions entry point takes, for a slice of the 2^n coalitions (a table is produced in chunks).  Bits n and above of
 * first + b are ignored.  players: HOST pointer to n region ids in [0, IQ_MAX_REGIONS), NULL = player k is region k.  base: regions
 * kept in EVERY coalition; a region in neither is always masked - an exact game among some of the regions.  IQ_EINVAL: a
 * region named by two players, or by a player and base. */
int iq_enum_keep_masks(uint64_t* keep /*count*/, uint64_t first, size_t count, const int32_t* players /*host, n*/, int n,
                       uint64_t base, iq_stream_t stream);

/* Scratch (bytes) that serves iq_exact_shapley(n) and iq_exact_interactions(n, P); 0 for arguments out of range
 * (n outside 1 .. IQ_MAX_EXACT_PLAYERS, P outside 0 .. 65535). */
size_t iq_exact_scratch_bytes(int n, int P);

/* The Shapley value itself, where tools/final_common.py:92-97 and final_shapley_value.py:145-150 average marginal
 * contributions over sampled permutations: phi[k] = sum over s of w(s) * sum over {c without bit k, popcount(c) = s} of
 * (double)(v[c | 1<<k] - v[c]), w(s) = 1 / (n * C(n-1, s)), the difference taken in float32 as tools/final_common.py:93
 * takes it.  Each stratum's sum is divided by the integer 1 / w(s).  v (2^n) float32, phi (n) float64. */
int iq_exact_shapley(const float* v, int n, double* phi, void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* The reference's I_ij^(m) (final_cal_interactions.py:28-36 over the contexts of final_gen_pair.py:25-41, m = int((R-2) * ratio))
 * with the expectation taken over ALL contexts: for pair p = (i, j) = pairs[p] (player positions) and every order
 * m = 0 .. n-2, out[p][m] = the mean over the C(n-2, m) contexts c without bits i, j and popcount(c) = m of
 * ((v[c|i|j] + v[c]) - v[c|i]) - v[c|j], in the float32 association of iq_interaction_reduce.  pairs (P,2) int32 on the
 * device, out (P, n-1) float64; P <= 65535 pairs per call (IQ_EINVAL beyond).  A pair with an entry outside [0, n) or with i = j reads nothing and gives NaN. */
int iq_exact_interactions(const float* v, int n, const int32_t* pairs /*P,2*/, int P, double* out /*P,n-1*/, void* scratch,
                          size_t scratch_bytes, iq_stream_t stream);

/* Harsanyi dividends (Moebius transform): a[c] = sum over subsets t of c of (-1)^(|c|-|t|) v[t], as n butterfly passes
 * a[c] -= a[c without bit b] over a float64 copy of v, bit 0 first.  v (2^n) float32, a (2^n) float64; needs no scratch.
 * Ties the two reductions above down: phi_k = sum over {c with bit k} of a[c] / |c|, and the interaction term of context S is
 * the sum of a[T + {i,j}] over the subsets T of S. */
int iq_moebius(const float* v, int n, double* a, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The regression (KernelSHAP) estimator of Shapley values (csrc/iq_kshap.hip)
 *
 * The reference estimates Shapley values from sampled permutations only (final_shapley_value.py:138-156).  The weighted
 * least-squares estimator takes M coalition rows z_m in {0,1}^n of a game of 2 <= n <= IQ_MAX_REGIONS regions, weights w_m (all 1
 * when the rows are sampled from the Shapley kernel), rewards v(z_m), v0 = v(empty) and delta = v(all) - v(empty):
 *     A = (1/W) sum w_m z_m z_m^T,   b = (1/W) sum w_m z_m ((double)v(z_m) - v0),   W = sum w_m,
 *     x = A^-1 b,  y = A^-1 1,  phi = x - y (1^T x - delta) / (1^T y)          (so sum(phi) = delta by construction).
 * With all 2^n - 2 proper coalitions and w(S) = (n-1) / (C(n,|S|) |S| (n-|S|)) phi is the exact Shapley vector.  The three entry
 * points below build the rows, reduce them to the RAW sums (the caller divides by W) and solve.  All float64 sums are taken in an
 * order that depends on (M, n, G) only - no floating-point atomics - so two calls give the same bits; G games that share the
 * rows (the poses of a sweep) give per game the bits of a call with G = 1.
 *
 * Wide games (65 .. IQ_MAX_WIDE_REGIONS regions, rows in the format of "Wide coalitions" below; csrc/iq_kshap_wide.hip) have the
 * estimator with the ANALYTIC A only: A = E[z z^T] under the size law p(s) ~ 1 / (s (R - s)) is alpha I + c 1 1^T with
 * alpha = 1 / (2 H_{R-1}), c = 1/2 - alpha, H_{R-1} = sum_{k<R} 1/k, so y = A^-1 1 is a multiple of 1 and the formula above becomes
 *     phi_i = 2 H_{R-1} (b_i - mean(b)) + delta / R:
 * no matrix, no factorisation, no singular case, sum(phi) = delta by construction, and with the enumerated rows and weights still
 * the exact Shapley vector.  The three wide entry points after iq_kshap_solve build the rows, reduce them to the raw b and W, and
 * evaluate that formula.  The A of sampled rows above 64 regions is not built.
 * ------------------------------------------------------------------------------------------- */

/* Row m of a sampled game: the regions orders[m][0 .. sizes[m]-1] of permutation m (iq_sample_permutations) as a keep mask.
 * paired != 0: keep[2m] = that set, keep[2m+1] = its complement within the n bits (keep holds 2S masks); else keep[m] (S masks).
 * status (1 int32, device, zeroed by the caller) becomes 1 if a size lies outside 1 .. n-1 and 2 if an order entry lies outside
 * [0, n); such a row is written as 0, nothing is read out of bounds, and the caller reads status when it needs the verdict. */
int iq_kshap_keep_masks(const int32_t* orders /*S,n*/, const int32_t* sizes /*S*/, uint64_t* keep /*M*/, int S, int n, int paired,
                        int32_t* status /*1, device*/, iq_stream_t stream);

/* Scratch (bytes) of iq_kshap_accum; 0 for arguments out of range (M outside 1 .. 2^30, n outside 2 .. 64, G outside 1 .. 65535). */
size_t iq_kshap_scratch_bytes(int M, int n, int G);

/* The raw moments of M rows shared by G games: A[i][j] = sum w_m z_mi z_mj (n,n), b[g][i] = sum w_m z_mi ((double)v[g][m] - v0[g])
 * (G,n), wsum = sum w_m; bit i of keep[m] is z_mi (every bit 0 .. 63 alike).  weights == NULL: w_m = 1, A holds co-occurrence
 * counts accumulated in integers (exact, order-free) and wsum = M.  Rows are summed in row order within a chunk of rows and the
 * chunks in chunk order by a second kernel; the chunking is a function of M alone. */
int iq_kshap_accum(const uint64_t* keep /*M*/, const float* v /*G,M*/, const double* v0 /*G*/, const double* weights /*M or NULL*/,
                   int M, int n, int G, double* A /*n,n*/, double* b /*G,n*/, double* wsum /*1*/, void* scratch, size_t scratch_bytes,
                   iq_stream_t stream);

/* phi[g] = x - y (1^T x - delta[g]) / (1^T y) with x = A^-1 b[g], y = A^-1 1: one workgroup, float64 Cholesky of A in LDS and two
 * triangular solves per right-hand side.  A (n,n) symmetric (the lower triangle is read), any positive scale common to A and b
 * aside.  status (1 int32, device) becomes 0, or 1 when a pivot is <= n 2^-52 max_i A_ii (or NaN): the rows do not determine
 * the regression, phi is left unwritten. */
int iq_kshap_solve(const double* A /*n,n*/, const double* b /*G,n*/, const double* delta /*G*/, double* phi /*G,n*/,
                   int32_t* status /*1, device*/, int n, int G, iq_stream_t stream);

/* iq_kshap_keep_masks for wide rows, 2 <= R <= IQ_MAX_WIDE_REGIONS, W = ceil(R / 64): row m (paired: row 2m) holds the first
 * sizes[m] entries of permutation m, bit (r & 63) of word (r >> 6); paired: row 2m+1 is its complement within the R bits, the bits
 * at or above R of the last word 0 in both.  status as in the narrow entry (1 = a size outside 1 .. R-1, 2 = an entry outside
 * [0, R)): the row and its complement are written as 0, nothing is read out of bounds.  One wave per sample.  For R <= 64 the
 * words are iq_kshap_keep_masks's. */
int iq_kshap_keep_masks_wide(const int32_t* orders /*S,R*/, const int32_t* sizes /*S*/, uint64_t* keep /*M,W*/, int S, int R, int paired,
                             int32_t* status /*1, device*/, iq_stream_t stream);

/* Scratch (bytes) of iq_kshap_moment_wide; 0 for arguments out of range (M outside 1 .. 2^30, R outside 2 .. IQ_MAX_WIDE_REGIONS,
 * G outside 1 .. 65535). */
size_t iq_kshap_scratch_bytes_wide(int M, int R, int G);

/* The raw moment of M wide rows shared by G games: b[g][i] = sum w_m z_mi ((double)v[g][m] - v0[g]) (G,R) and wsum = sum w_m (M
 * when weights == NULL).  The summation order per region is iq_kshap_accum's - rows cut into chunks of whole 256-row tiles by the
 * same function of M, within a chunk wave q of four adds rows 64 q .. 64 q + 63 of every tile in row order, the waves added as
 * ((0 + 1) + 2) + 3, the chunks in chunk order by a second kernel; wsum by the narrow rule - so for R <= 64 b and wsum are that
 * entry's bits, two calls give the same bits, and G games give per game the bits of a call with G = 1. */
int iq_kshap_moment_wide(const uint64_t* keep /*M,W*/, const float* v /*G,M*/, const double* v0 /*G*/,
                         const double* weights /*M or NULL*/, int M, int R, int G, double* b /*G,R*/, double* wsum /*1*/,
                         void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* phi[g][i] = 2 H_{R-1} (x_i - mean(x)) + delta[g] / R with x = b[g] / wsum (b and wsum RAW, as iq_kshap_moment_wide leaves them on
 * the device: no host round trip), 2 <= R <= IQ_MAX_WIDE_REGIONS.  H_{R-1} is summed in float64 in ascending k on the host, inside this
 * call, and passed to the kernel by value.  Per game, in this order, every operation rounded on its own: x_i = b_i / wsum;
 * c = (x_0 + x_1 + ...) / R in index order; y_i = x_i - c; d = (y_0 + y_1 + ...) / R in index order (the mean of the centred
 * values: 0 but for the rounding of c); phi_i = (2 H) (y_i - d) + delta / R.  No status word: there is no singular case. */
int iq_kshap_phi_analytic(const double* b /*G,R raw*/, const double* wsum /*1, device*/, const double* delta /*G*/,
                          double* phi /*G,R*/, int R, int G, iq_stream_t stream);

/* The COUNTER-BASED draw of a wide game's rows (csrc/iq_kshap_draw.hip): sizes and members of samples first .. first + S - 1 of one
 * cloud in one launch, each a pure function of (seed, stream, m, R) - no generator state, no sequential part, any range of rows
 * drawn alone, the chunking without influence.  Another contract than the MT19937 stream of iq_kshap_keep_masks_wide's callers,
 * which stays the default; the estimator needs a size under p(s) ~ 1 / (s (R - s)), a uniform s-subset and repeatability only.
 *
 * Generator: Philox4x32-10.  Multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85 after every round
 * but the last; ten rounds of (c0,c1,c2,c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)).
 * Known answers: counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ffffffff -> 408f276d 41c83b0e a20bc7c6 6d5451fd;
 * counter 243f6a88 85a308d3 13198a2e 03707344, key a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1.
 * Key: (seed & 0xffffffff, stream & 0xffffffff); the drivers pass --seed and the cloud's index.  m: the 64-bit sample index
 * within the cloud, from 0, as (m_lo, m_hi).
 *
 * Size of sample m: words w0 .. w3 of the block with counter (m_lo, m_hi, 0, 1); u = ((w0 >> 5) 2^26 + (w1 >> 6)) / 2^53 (NumPy's
 * random_sample construction); s = min(R - 1, 1 + #{k : cdf[k] <= u}) (searchsorted, side = "right").  cdf: R - 1 float64 on the
 * device, the host's table of P(size <= k + 1); the device divides nothing, so host and device agree bit for bit.
 * Members of sample m: region i has the 32-bit key u_i = word (i & 3) of the block with counter (m_lo, m_hi, i >> 2, 0) and the
 * composite key (u_i << 10) | i - 42 bits, no two regions share one; S_m = the s regions of the smallest composite keys.  That is
 * the random-keys construction of a uniform s-subset, exact except where the s-th and (s+1)-th 32-bit keys are equal: there the
 * lower index wins.  A row holds two equal 32-bit keys AT ALL with probability below R^2 / 2^33, and they must also be the s-th and
 * (s+1)-th: at most a fraction R / 2^32 of the rows (2.4e-7 at R = 1024) can be affected.
 * Rows: unpaired, row j of keep is S_{first + j}; paired, row 2j is S_{first + j} and row 2j + 1 its complement within the R bits;
 * bits at or above R are 0; keep is (rows, W), W = ceil(R / 64), in the format of "Wide coalitions" below.  sizes[j] = s of sample
 * first + j (NULL: not written).
 * Checks: 2 <= R <= IQ_MAX_WIDE_REGIONS; 0 <= S <= 2^29; first >= 0 and first + S <= 2^62; S == 0 is IQ_OK and nothing is read;
 * otherwise cdf and keep must not be NULL.  One wave per sample, no atomics, nothing read back. */
int iq_kshap_draw_counter(uint64_t seed, uint64_t stream, int64_t first, int S, int R, const double* cdf /*R-1, device*/, int paired,
                          uint64_t* keep /*rows,W*/, int32_t* sizes /*S or NULL*/, iq_stream_t queue);

/* ---------------------------------------------------------------------------------------------
 * All-pairs interactions from the regression rows (SHAP-IQ; csrc/iq_kshap_pairs.hip)
 *
 * The rows of the regression estimator are drawn from the Shapley kernel with known probabilities: P(S) = p(s) / C(R,s),
 * p(s) = 1 / (s (R - s) Z), Z = 2 H / R, H = H_{R-1} = sum_{k<R} 1/k (float64, ascending k, on the host).  The pairwise Shapley
 * interaction index SII_ij = sum_S v(S) gamma(|S|, |S & {i,j}|), gamma(s,k) = (-1)^k (s-k)! (R-s-2+k)! / (R-1)!, is therefore
 * estimated without bias, for all R (R-1) / 2 pairs at once and with no further model evaluation, by (Fumagalli et al., 2023)
 *     I_ij = delta / (R - 1) + (1 / W_sum) sum_m d_m mu(s_m, z_mi + z_mj),      i != j,
 *     mu(s,2) = 2 H (R - s) / (s - 1)  (s >= 2),   mu(s,1) = -2 H,   mu(s,0) = 2 H s / (R - s - 1)  (s <= R - 2),
 * with mu = gamma C(R,s) / p(s), s_m = popcount(z_m), d_m = w_m ((double)v_m - v0) as the moment b forms it, W_sum = sum w_m,
 * v0 = v(empty), delta = v(all) - v(empty).  Subtracting v0 is free (a constant game has no interaction) and leaves
 * delta / (R - 1) from the full coalition.  A row with s = 0 (a row the keep kernels wrote as 0 after a refusal) or s = R
 * contributes 0 whatever its reward, but counts in W_sum, as in iq_kshap_accum.  With all 2^R - 2 proper coalitions and the
 * weights w(S) = (R-1) / (C(R,s) s (R-s)) the sum is the exact SII: the mean over the orders m = 0 .. R-2 of the
 * context-averaged I_ij^(m) of iq_exact_interactions.
 *
 * Computed in the form of one product, mu(s,k) = alpha_s + beta_s k + gamma_s [k = 2] with alpha_s = mu(s,0) (0 at s = R-1),
 * beta_s = -2H - alpha_s, gamma_s = mu(s,2) + 4H + alpha_s (0 at s = 1), rows 0 and R zero - the (R+1, 3) float64 table `coef`
 * the host builds (kernelshap.pair_coefficients):
 *     I_ij = delta / (R-1) + (((A + L_i) + L_j) + Q_ij) / W_sum,
 *     A = sum d_m alpha_s,   L_i = sum (d_m beta_s) z_mi,   Q_ij = sum (d_m gamma_s) z_mi z_mj.
 * The terms cancel near s = R-2 (alpha and gamma of size 2 H R, mu(s,2) small): in float64 the error stays within
 * (M + 16) 2^-53 sum_m |d_m| (|alpha_s| + 2 |beta_s| + |gamma_s|) / W_sum for any summation order.
 *
 * Order.  Q on v_mfma_f64_16x16x4_f64: rows cut into chunks of whole 256-row tiles, chunks_of(M) with the count capped so that
 * count * R * R * 8 bytes stay within 64 MB (8 chunks at R = 1024) - a function of (M, R) alone; within a chunk wave q of four
 * adds rows 64 q .. 64 q + 63 of every tile, four rows per instruction in row order, the waves added as ((0 + 1) + 2) + 3, the
 * chunks in chunk order.  L, A and W_sum: the order of iq_kshap_moment_wide on chunks_of(M) (A: a chunk's sum as its sum of
 * weights is taken).  No floating-point atomics, no grid chosen at run time: two calls give the same bits, a game's bits do not
 * depend on G or on its place among the games, and a game never meets another game's rewards.
 * ------------------------------------------------------------------------------------------- */

/* Scratch (bytes) of iq_kshap_pairs; 0 for arguments out of range (M outside 1 .. 2^30, R outside 2 .. IQ_MAX_WIDE_REGIONS,
 * G outside 1 .. 65535). */
size_t iq_kshap_pairs_scratch_bytes(int M, int R, int G);

/* out[g][i][j] = I_ij of game g from M rows of W = ceil(R / 64) words (W = 1: the narrow format; bits at or above R are ignored)
 * shared by G games; out[g][i][i] = 0, and out[g][i][j] and out[g][j][i] are the same bits (the upper triangle is built and
 * mirrored).  coef: the (R+1, 3) table above, on the device.  weights == NULL: w_m = 1 and W_sum = M. */
int iq_kshap_pairs(const uint64_t* keep /*M,W*/, const float* v /*G,M*/, const double* v0 /*G*/, const double* delta /*G*/,
                   const double* weights /*M or NULL*/, const double* coef /*R+1,3 device*/, int M, int R, int G,
                   double* out /*G,R,R*/, void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Standard errors of the sampled estimates (csrc/iq_kshap_pairs.hip, csrc/iq_kshap_wide.hip)
 *
 * For SAMPLED rows only (weights == NULL): enumerated or weighted rows have no sampling error.  A UNIT u is the iid draw:
 * unpaired, row u (c = 1 row per unit); paired, rows 2u and 2u + 1, a set and its complement (c = 2, M even).  U units, M = c U
 * rows, U >= 2.  For an estimate est = const + (1/M) sum_u y_u, with S1 = sum y_u and S2 = sum y_u^2,
 *     var = (U / (U - 1)) (S2 - S1^2 / U) / M^2,      se = sqrt(max(var, 0)),
 * is unbiased for the variance of est (the two rows of a paired unit are NOT independent: the unit, not the row, is squared).
 * No further model evaluation: second moments of the same rows and rewards.
 *
 * Pairs.  mu as above, 0 where a case cannot occur (mu(s,0) at s = R-1, mu(s,2) at s = 1), evaluated in closed form from 2 H (two
 * roundings an entry, not from the differences of `coef`).  For the pair {i,j}, k = the number of its members in the unit's first
 * row, of size s: unpaired x_u(k) = d_u mu(s,k); paired x_u(k) = d_2u mu(s,k) + d_2u+1 mu(R-s, 2-k); d_m = (double)v_m - v0; a unit
 * whose first row has size 0 or R has x = 0 and counts in U.  Any function of k in {0,1,2} is P + B k + G [k = 2]:
 *     P_u = x_u(0)^2,   B_u = x_u(1)^2 - x_u(0)^2,   G_u = (x_u(2)^2 - 2 x_u(1)^2) + x_u(0)^2,
 *     S2_ij = ((sum P + sum B z_i) + sum B z_j) + sum G z_i z_j          (z = the unit's first row),
 * one scalar, one moment and one R x R x U product: the shape and the order of A, L and Q above on the units' first rows -
 * pair_chunks_of(U, R) for the product on v_mfma_f64_16x16x4_f64, chunks_of(U) for the moment and the scalar.
 * S1_ij = ((A + L_i) + L_j) + Q_ij of the estimate itself (= M (I_ij - delta / (R-1))).  Then, each operation rounded on its own,
 * var = ((U / (U-1)) (S2 - S1 S1 / U)) / (M M) and se = sqrt(var), 0 where var < 0.  In float64 S2 stays within
 * (U + 16) 2^-53 sum_u (|P_u| + 2 |B_u| + |G_u|) of its value for any summation order.
 *
 * phi under the analytic Gram matrix.  phi_i = delta / R + (1/M) sum_u y_ui, y_ui = 2 H D_u (z_ui - s_u / R), D_u = d_u
 * (unpaired) or d_2u - d_2u+1 (paired), z and s of the unit's first row.  z^2 = z, so
 *     S2_i = (2H 2H) (sum_u e_u z_ui + sum_u f_u),   e_u = D_u^2 (1 - 2 s_u / R),   f_u = D_u^2 (s_u^2 / R^2),
 * a moment in iq_kshap_moment_wide's order on chunks_of(U) and a scalar (a chunk's sum as its sum of weights is taken), and
 * S1_i = 2H (b_i - (b_0 + b_1 + ... in index order) / R) from the raw float64 b, not from phi's rounded bits.
 * The sampled-Gram solve (iq_kshap_solve) has no standard error here.
 *
 * As above: no floating-point atomics, no grid chosen at run time, two calls give the same bits, a game's bits depend neither on G
 * nor on a neighbouring game's rewards.
 * ------------------------------------------------------------------------------------------- */

/* Scratch (bytes) of iq_kshap_pairs_se; 0 for arguments iq_kshap_pairs_scratch_bytes refuses, for fewer than 2 units and for
 * paired != 0 with odd M. */
size_t iq_kshap_pairs_se_scratch_bytes(int M, int R, int G, int paired);

/* out: the bits of iq_kshap_pairs on the same arguments with weights == NULL (its kernels, unchanged).  se[g][i][j] = the standard
 * error of out[g][i][j] as defined above, symmetric bit for bit, se[g][i][i] = 0.  IQ_EINVAL for fewer than 2 units, and for
 * paired != 0 with odd M. */
int iq_kshap_pairs_se(const uint64_t* keep /*M,W*/, const float* v /*G,M*/, const double* v0 /*G*/, const double* delta /*G*/,
                      const double* coef /*R+1,3 device*/, int M, int R, int G, int paired, double* out /*G,R,R*/,
                      double* se /*G,R,R*/, void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* Scratch (bytes) of iq_kshap_moment_se_wide; 0 for arguments iq_kshap_scratch_bytes_wide refuses, for fewer than 2 units and for
 * paired != 0 with odd M. */
size_t iq_kshap_moment_se_scratch_bytes_wide(int M, int R, int G, int paired);

/* b: the raw moment, the bits of iq_kshap_moment_wide with weights == NULL (wsum = M).  var[g][i] = the variance of phi_i of game g
 * as defined above (it may be a rounding below 0; the caller takes sqrt(max(var, 0))).  Narrow rows are rows of W = 1 word.
 * IQ_EINVAL for fewer than 2 units, and for paired != 0 with odd M. */
int iq_kshap_moment_se_wide(const uint64_t* keep /*M,W*/, const float* v /*G,M*/, const double* v0 /*G*/, int M, int R, int G,
                            int paired, double* b /*G,R*/, double* var /*G,R*/, void* scratch, size_t scratch_bytes,
                            iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Control variates for the all-pairs map (csrc/iq_kshap_paircv.hip, csrc/iq_kshap_pairs.hip)
 *
 * The SHAP-IQ estimate above is unbiased and, at the budget of the Shapley stage, mostly noise.  Both estimators here run on the
 * SAME sampled rows (weights == NULL) and rewards, with no further model evaluation, and subtract from every row a game whose
 * pair interactions are known.  SHAPIQ(t) below is the estimator above on float64 per-row terms t_m in place of d_m and without
 * its delta / (R-1) term: (((A + L_i) + L_j) + Q_ij) / W_sum (iq_kshap_pairs_terms), its standard error the formulas of "Standard
 * errors" on t (iq_kshap_pairs_terms_se).  The delta term is the share of the full set, which no row holds: a subtracted game
 * that is EFFICIENT, g(N) = delta, g(empty) = 0, leaves a residual game whose full and empty set are worth 0.
 *
 * shift, 2 <= R <= IQ_MAX_WIDE_REGIONS, narrow and wide rows, paired or not.  The additive game delta s / R has no pair
 * interaction:
 *     t_m = ((double)v_m - v0) - (delta (double)s_m) / (double)R       (iq_kshap_pair_shift_terms),      I = SHAPIQ(t).
 * On paired rows mu(s,k) = mu(R-s, 2-k) makes a row and its complement enter as mu (d(S) + d(S^c)), to which an additive part of
 * the game contributes only its total: the shift removes it.
 *
 * regression, 2 <= R <= IQ_MAX_REGIONS, narrow rows.  Features a = 0 .. d-1, d = R + R (R-1) / 2: the singles first, then the
 * pairs (i < j) in row-major order; fm_a the 64-bit mask of the feature's regions, f_a(S) = [fm_a subset of S].  The U units of
 * the rows (a row, or paired a row and its complement) are cut into two contiguous folds, units [0, U/2) and [U/2, U), each of at
 * least 2 units.  Per fold f (M_f rows) and game:
 *     Gram_f[a][b] = #{m in f : fm_a | fm_b subset of S_m}                      (iq_kshap_pair_gram: exact counts),
 *     c_f[a] = sum_{m in f} f_a(S_m) ((double)v_m - v0)                         (float64, the moments' order on chunks_of(M_f)),
 *     A = Gram_f + ridge I = L L^T,  beta_u = A^-1 c_f,  w = A^-1 1,            (ridge >= 0; the caller's default is M_f / 64)
 *     beta = beta_u - w ((1 beta_u - delta) / (1 w))                            (iq_kshap_pair_fit: sum(beta) = delta),
 * a pivot not above d 2^-52 max_i A_ii sets the status word (iq_kshap_solve's rule) and the betas are then meaningless.  The
 * surrogate g_beta(S) = sum_a f_a(S) beta_a is 2-additive: its pair interaction C_ij(beta) is the coefficient of the pair.  Then
 *     t_m = ((double)v_m - v0) - g_{beta of the OTHER fold}(S_m),   m in f      (iq_kshap_pair_surrogate),
 *     I_f = C(beta_other) + (delta - 1 beta_other) / (R-1) + SHAPIQ_f(t),       se_f as in "Standard errors" on t over f's units,
 *     I = (M_0 I_0 + M_1 I_1) / M,       se = sqrt(M_0^2 se_0^2 + M_1^2 se_1^2) / M          (host, float64).
 * Each I_f is unbiased whatever the fit is, because beta_other does not depend on the rows of f; the fit decides the variance
 * only.  (delta - 1 beta) is the rounding of the efficiency constraint, kept so that the identity is exact for any beta.  The two
 * I_f are not independent (each fold's rows fit the other's surrogate); se NEGLECTS that cross-fold covariance.
 *
 * Order: the Gram matrix is sums of ones on v_mfma_f64_16x16x4_f64, exact in any order.  The Cholesky factor is blocked (panels of
 * 32 columns: diagonal block in one workgroup's LDS, panel below it a row per thread, trailing update a thread per entry, the
 * panel's columns subtracted in order), the triangular solves one workgroup per right-hand side, the surrogate one thread per
 * row with the features added in index order in one chain.  One stream, no floating-point atomics, no grid chosen at run time:
 * two calls give the same bits, a game's bits depend neither on G nor on a neighbouring game's rewards.
 * ------------------------------------------------------------------------------------------- */

/* iq_kshap_pairs on float64 terms t (G,M) in place of (v, v0, delta): out = SHAPIQ(t) as defined above.  weights as there (the
 * enumerated rows with their weights give the exact index of a game whose full and empty set are worth 0).  Scratch:
 * iq_kshap_pairs_scratch_bytes. */
int iq_kshap_pairs_terms(const uint64_t* keep /*M,W*/, const double* t /*G,M*/, const double* weights /*M or NULL*/,
                         const double* coef /*R+1,3 device*/, int M, int R, int G, double* out /*G,R,R*/, void* scratch,
                         size_t scratch_bytes, iq_stream_t stream);

/* iq_kshap_pairs_se on float64 terms t (G,M): out the bits of iq_kshap_pairs_terms with weights == NULL, se its standard error.
 * Scratch: iq_kshap_pairs_se_scratch_bytes. */
int iq_kshap_pairs_terms_se(const uint64_t* keep /*M,W*/, const double* t /*G,M*/, const double* coef /*R+1,3 device*/, int M, int R,
                            int G, int paired, double* out /*G,R,R*/, double* se /*G,R,R*/, void* scratch, size_t scratch_bytes,
                            iq_stream_t stream);

/* d = R + R (R-1) / 2, the features of the surrogate; 0 outside 2 <= R <= IQ_MAX_REGIONS. */
int iq_kshap_pair_features(int R);

/* gram (d,d) float64, symmetric: the exact counts Gram[a][b] of the narrow rows keep (M); bits at or above R are ignored. */
int iq_kshap_pair_gram(const uint64_t* keep /*M*/, int M, int R, double* gram /*d,d*/, iq_stream_t stream);

/* Scratch (bytes) of iq_kshap_pair_fit: A (d,d), the right-hand sides' partials (G, chunks_of(M), d), the right-hand sides
 * (G+1, d) and one float64, each rounded up to 256 bytes; 0 outside 1 <= M <= 2^30, 2 <= R <= IQ_MAX_REGIONS, 1 <= G <= 65535. */
size_t iq_kshap_pair_fit_scratch_bytes(int M, int R, int G);

/* beta (G,d) of the rows keep (M) with rewards v (G,M), from gram = iq_kshap_pair_gram of the same rows (unchanged).  solves
 * (G+1,d) or NULL: rows 0 .. G-1 the unconstrained beta_u, row G w = A^-1 1, as the constraint read them.  *status (device): 0,
 * or 1 where a pivot failed.  IQ_EINVAL for ridge < 0 or NaN. */
int iq_kshap_pair_fit(const double* gram /*d,d*/, const uint64_t* keep /*M*/, const float* v /*G,M*/, const double* v0 /*G*/,
                      const double* delta /*G*/, double ridge, int M, int R, int G, double* beta /*G,d*/,
                      double* solves /*G+1,d or NULL*/, int32_t* status, void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* out_g[g][m] = g_{beta[g]}(S_m); out_t[g][m] = ((double)v[g][m] - v0[g]) - out_g[g][m].  Either output may be NULL (not both);
 * v and v0 are read for out_t only. */
int iq_kshap_pair_surrogate(const uint64_t* keep /*M*/, const double* beta /*G,d*/, const float* v /*G,M or NULL*/,
                            const double* v0 /*G or NULL*/, int M, int R, int G, double* out_g /*G,M or NULL*/,
                            double* out_t /*G,M or NULL*/, iq_stream_t stream);

/* The terms of the shift, t[g][m] as defined above, for rows of W words, 2 <= R <= IQ_MAX_WIDE_REGIONS. */
int iq_kshap_pair_shift_terms(const uint64_t* keep /*M,W*/, const float* v /*G,M*/, const double* v0 /*G*/, const double* delta /*G*/,
                              int M, int R, int G, double* t /*G,M*/, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse regression control variate (csrc/iq_kshap_sparsecv.hip, csrc/iq_kshap_fit.h)
 *
 * The regression control above with a surrogate of all R singles and a caller-chosen list of K pairs, for narrow and wide rows of
 * 2 <= R <= IQ_MAX_WIDE_REGIONS regions.  A pair list is pairs (K,2) int32 with 0 <= i < j < R, strictly increasing in row-major
 * order (so without duplicates), K >= 0.  Features a = 0 .. d-1, d = R + K <= IQ_KSHAP_SPARSE_MAX_FEATURES: the singles first, then
 * the listed pairs in list order; f_a(S) = 1 when the feature's one or two regions are all in S.  K = 0 is a fitted additive
 * control; the complete row-major list at R <= IQ_MAX_REGIONS is the regression control above, bit for bit.
 *
 * Everything else is the regression control's contract with this d and these features: the two contiguous folds of units; per
 * fold Gram = exact counts, c, A = Gram + ridge I, beta under sum(beta) = delta; the OTHER fold's beta gives
 * t_m = ((double)v_m - v0) - g_beta(S_m); I_f = C(beta) + (delta - 1 beta) / (R-1) + SHAPIQ_f(t) (iq_kshap_pairs_terms_se on the
 * original rows, narrow or wide); the row-weighted average; the se that neglects the cross-fold covariance.  C(beta) holds
 * beta_{R+k} at (i_k, j_k) and (j_k, i_k) and 0 elsewhere.
 *
 * Unbiased whatever the list and the fit are, PROVIDED THE LIST DOES NOT DEPEND ON THE REWARDS OF THE ROWS IT IS APPLIED TO: a
 * list from the geometry of the regions (the neighbours of the caller's default) or from other rows satisfies it, a list screened
 * on the same rows' rewards does not.
 *
 * The entries work on FEATURE ROWS: feat (M, Wd) uint64, Wd = ceil(d / 64), bit (a & 63) of word (a >> 6) of row m = f_a(S_m).
 * Gram, right-hand sides and surrogate are then the kernels of the regression control on rows of Wd words; ridge, factor, solves
 * and constraint are the very kernels of iq_kshap_pair_fit.  The Gram matrix is one workgroup per 64 x 64 block on or above the
 * diagonal walking every row (561 workgroups at d = 2080), not cut into chunks: the counts are exact in any order.  The same
 * guarantees: one stream, no floating-point atomics, no grid chosen at run time, two calls give the same bits, a game's bits
 * depend neither on G nor on a neighbouring game's rewards.
 * ------------------------------------------------------------------------------------------- */

/* feat (M, ceil((R + K) / 64)) of the rows keep (M, W = ceil(R / 64)): bits of keep at or above R are ignored, bits of feat at or
 * above d = R + K are written 0.  A list entry outside 0 <= i < j < R is never used as an index: it yields a feature that no row
 * holds (the order of the list is not checked here: the entry cannot see the list without a synchronisation; callers check it).
 * pairs may be NULL when K == 0. */
int iq_kshap_sparse_expand(const uint64_t* keep /*M,W*/, const int32_t* pairs /*K,2*/, int M, int R, int K, uint64_t* feat /*M,Wd*/,
                           iq_stream_t stream);

/* gram (d,d) float64, symmetric: Gram[a][b] = the number of feature rows that hold bits a and b, exact counts; bits at or above
 * d are ignored.  1 <= M <= 2^30, 2 <= d <= IQ_KSHAP_SPARSE_MAX_FEATURES. */
int iq_kshap_feat_gram(const uint64_t* feat /*M,Wd*/, int M, int d, double* gram /*d,d*/, iq_stream_t stream);

/* Scratch (bytes) of iq_kshap_feat_fit: that of iq_kshap_pair_fit with this d; 0 outside 1 <= M <= 2^30,
 * 2 <= d <= IQ_KSHAP_SPARSE_MAX_FEATURES, 1 <= G <= 65535. */
size_t iq_kshap_feat_fit_scratch_bytes(int M, int d, int G);

/* iq_kshap_pair_fit on feature rows: beta (G,d) from gram = iq_kshap_feat_gram of the same rows; solves, *status, ridge as there. */
int iq_kshap_feat_fit(const double* gram /*d,d*/, const uint64_t* feat /*M,Wd*/, const float* v /*G,M*/, const double* v0 /*G*/,
                      const double* delta /*G*/, double ridge, int M, int d, int G, double* beta /*G,d*/,
                      double* solves /*G+1,d or NULL*/, int32_t* status, void* scratch, size_t scratch_bytes, iq_stream_t stream);

/* iq_kshap_pair_surrogate on feature rows: out_g[g][m] = the beta[g] of the set bits of row m below d, added in index order in
 * one chain; out_t[g][m] = ((double)v[g][m] - v0[g]) - out_g[g][m].  Either output may be NULL (not both). */
int iq_kshap_feat_surrogate(const uint64_t* feat /*M,Wd*/, const double* beta /*G,d*/, const float* v /*G,M or NULL*/,
                            const double* v0 /*G or NULL*/, int M, int d, int G, double* out_g /*G,M or NULL*/,
                            double* out_t /*G,M or NULL*/, iq_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Wide coalitions: region games of more than 64 regions, up to one region per point (csrc/iq_wide.hip, csrc/iq_pointnet.hip)
 *
 * In the reference NUM_REGIONS is a constant (tools/final_util.py:20-22) and mask_data_batch (tools/final_common.py:46-61),
 * cal_region_id (final_shapley_value.py:20-35) and the sampling loop (:138-156) work for any region count up to the number of
 * points.  A WIDE coalition is a row of W = ceil(R / 64) uint64 words: bit (r & 63) of word (r >> 6) set = region r kept; bits
 * at or above R are ignored.  1 <= R <= IQ_MAX_WIDE_REGIONS.  Every entry point above keeps its R <= 64 check and its code;
 * for R <= 64 (W = 1) the entry points below give the same bits as their narrow twins.  The permutations of a wide game and
 * the contexts of its interaction stage (final_shapley_value.py:59-72, final_gen_pair.py:18-43: NumPy's global generator) are
 * drawn on the host or, the same bits, on the device: iq_sample_permutations_wide is iq_sample_permutations_ws's kernels with
 * 16-bit rows and longer windows, and iq_context_regions_wide turns the head of a permutation into a context.  The multi-order
 * interactions of a wide game need one more wide entry point only, iq_context_keep_masks_wide: iq_reward and
 * iq_interaction_reduce never see a mask.
 * Every family's coalition entry has a wide form (the compact paths of PointNet++ / DGCNN / GCNN / PointConv: the few small kernels
 * that turn a mask into a coalition's kept points, csrc/iq_common.h WaveKeep; everything behind them works on points); those
 * families can also evaluate wide coalitions with iq_mask_coalitions_wide + their iq_*_forward.  The pose sweeps of a wide
 * game need no entry point of their own - every pose of a cloud goes through the coalition entries below - and its smoothness
 * stage needs one, iq_smoothness_enum_wide (declared beside iq_smoothness_enum above: the same kernel, N <= 1024).
 * ------------------------------------------------------------------------------------------- */

/* iq_sample_permutations_ws for 1 <= R <= IQ_MAX_WIDE_REGIONS: the same draw as NumPy's legacy RandomState.permutation(R), S
 * times, and the same state handed back; for R <= 64 the rows are iq_sample_permutations's.  Of every permutation the first
 * `head` entries are written (0 <= head <= R), rows of `head`: a sampled context is the head of a permutation
 * (final_gen_pair.py:29: np.random.choice(rest, m, replace=False)), and at R = 1024 the full rows of one ratio of the interaction
 * stage would be 123 MB.  head = 0 or orders = NULL: the draw advances the state and writes nothing (the contexts of a cloud that
 * is not selected).  The conventions of iq_sample_permutations_ws hold: nothing is allocated and the host is never synchronised;
 * iq_sample_wide_workspace_bytes(S, R) - 16 bytes per estimated word, 0 for a refused argument or a draw that one batch of the
 * one-workgroup kernel covers, never smaller for a larger S - is the size at which the spread kernels expect to draw everything,
 * and with any smaller workspace, none included, or an unlucky draw the one-workgroup kernel, which runs last, draws the rest:
 * rows and state never depend on the workspace or on how a draw is cut into calls.  A malformed or poisoned state gives rows
 * of -1 and stays poisoned. */
size_t iq_sample_wide_workspace_bytes(int S, int R);
int iq_sample_permutations_wide(uint32_t* mt_state /*625*/, int32_t* orders /*S,head or NULL*/, int S, int R, int head,
                                void* workspace, size_t workspace_bytes, iq_stream_t stream);

/* final_gen_pair.py:25-29: heads of permutations of R - 2 -> context regions, in place.  Entry k becomes rest[k] for the ascending
 * list `rest` of the regions outside pair p = (i, j): k + (k >= lo) + (k + 1 >= hi) with lo < hi the pair.  One coalesced pass;
 * 0 <= m <= R - 2.  The pair is not checked here (i == j or an entry outside [0, R): the caller refuses it). */
int iq_context_regions_wide(const int32_t* pairs /*P,2*/, int32_t* heads /*P,C,m: in place -> contexts*/, int P, int C, int m, int R,
                            iq_stream_t stream);

/* tools/final_common.py:56-60 as wide masks: row s*(R+1) + i of keep keeps orders[s][0..i-1]; an entry outside [0, R) is ignored. */
int iq_prefix_keep_masks_wide(const int32_t* orders /*S,R*/, uint64_t* keep /*S*(R+1),W*/, int S, int R, iq_stream_t stream);

/* final_point_binary_interaction_logits.py:45-52 as wide masks (iq_context_keep_masks's rows): for pair p = (i, j) and its
 * context c = contexts[p][c][0..m-1], rows 4(pC + c) + 0..3 of keep = S+{i,j}, S+{i}, S+{j}, S.  0 <= m <= R; contexts may be
 * NULL when m = 0 (the empty context).  A pair or context entry outside [0, R) is ignored: no bit at or above R is ever set.
 * For R <= 64 the words are iq_context_keep_masks's.  One wave per context: coalesced loads, one contiguous 32 W-byte store. */
int iq_context_keep_masks_wide(const int32_t* pairs /*P,2*/, const int32_t* contexts /*P,C,m*/, uint64_t* keep /*4PC,W*/,
                               int P, int C, int m, int R, iq_stream_t stream);

/* iq_mask_coalitions for wide keep rows (tools/final_common.py:46-61 for arbitrary coalitions): out row b keeps the regions of
 * keep[b]; a point whose region id lies outside [0, R) is masked.  out (B,N,3) or (B,3,N); any 1 <= N <= IQ_MAX_POINTS. */
int iq_mask_coalitions_wide(const float* cloud /*N,3*/, const int32_t* region_id /*N*/, const uint64_t* keep /*B,W*/,
                            const float* center /*3*/, float* out, int N, int R, int B, int channel_first, iq_stream_t stream);

/* iq_region_assign (final_shapley_value.py:20-35 with tools/final_util.py:134-147) for up to IQ_MAX_WIDE_REGIONS centres: the
 * same expanded-form distance in the same operation order, first index on ties.  With R = N (one region per point; FPS repeats
 * index 0 once the distinct locations are used up) duplicate points leave empty regions. */
int iq_region_assign_wide(const float* cloud /*N,3*/, const int32_t* fps_idx /*R*/, int32_t* region_id /*N*/, int N, int R,
                          iq_stream_t stream);

/* iq_shapley_accum (tools/final_common.py:92-96, final_shapley_value.py:145-150) for R <= IQ_MAX_WIDE_REGIONS: the same
 * arguments, the same float32 differences, the same float64 adds in permutation order per region. */
int iq_shapley_accum_wide(const float* v /*S*(R+1)*/, const int32_t* orders /*S,R*/, double* sv_rows, double* phi_sum,
                          const int32_t* snap_counts, int n_snap, double* snaps, int R, int S, iq_stream_t stream);

/* iq_pointnet_coalitions for wide keep rows (B,W): the per-cloud counting sort, the row-list builder and the pooled input-STN
 * gather in their wide form, then the same chain kernels and heads on the resulting lists - for R <= 64 the lists, hence the
 * logits, are iq_pointnet_coalitions's bit for bit.  A region may be empty (its player's marginal contribution is 0).  The
 * workspace holds nclouds*(R+1) pre-pooled feature rows of 4 KB and as many row lists. */
size_t iq_pointnet_wide_workspace_bytes(int B, int nclouds, int N, int R);
int iq_pointnet_coalitions_wide(const iq_pointnet_weights* w, const float* clouds, const float* centers,
                                const int32_t* region_id, const uint64_t* keep /*B,W*/, const int32_t* cloud_of, float* logits,
                                float* trans_feat_packed, void* workspace, size_t workspace_bytes, int B, int nclouds, int N,
                                int R, int channel_first, iq_stream_t stream);

/* The prefix coalitions of S permutations without keep rows: item o*(R+1) + i keeps orders[o][0..i-1], with the set semantics
 * of iq_prefix_keep_masks_wide (an entry outside [0, R) is ignored, a region named twice counts once).  The row list of an item
 * is a prefix of the permutation-ordered point list and its pooled input-STN feature the running maximum along the permutation
 * (R rows of the pre-pool per permutation, not R^2 / 2); a row list holds the points of iq_pointnet_coalitions_wide's in another
 * order and every pooling is an exact maximum, so logits and trans_feat_packed are that entry's on
 * iq_prefix_keep_masks_wide(orders), bit for bit.  cloud_of[o] is the cloud of PERMUTATION o (required when 1 < nclouds != S);
 * centers is required; clouds are channel-last.  1 <= R <= IQ_MAX_WIDE_REGIONS (for R <= 64 the bits are the narrow entry's).
 * Workspace: iq_pointnet_wide_workspace_bytes(S*(R+1), nclouds, N, R). */
int iq_pointnet_prefix_coalitions_wide(const iq_pointnet_weights* w, const float* clouds /*nclouds,N,3*/,
                                       const float* centers /*nclouds,3*/, const int32_t* region_id /*nclouds,N*/,
                                       const int32_t* orders /*S,R*/, const int32_t* cloud_of /*S or NULL*/,
                                       float* logits /*S*(R+1),C*/, float* trans_feat_packed /*S*(R+1),4096 or NULL*/,
                                       void* workspace, size_t workspace_bytes, int S, int nclouds, int N, int R,
                                       iq_stream_t stream);

/* iq_dgcnn_coalitions, iq_pointnet2_coalitions, iq_pointconv_coalitions and iq_pointconv_coalitions_cached for wide keep rows
 * (B,W): the arguments of the narrow twin plus R, 1 <= R <= IQ_MAX_WIDE_REGIONS; a point whose region id lies outside [0, R) is
 * masked, bits at or above R change nothing.  The same workspace functions as the twins (iq_dgcnn_workspace_bytes,
 * iq_pointnet2_coalitions_workspace_bytes, iq_pointconv_coalitions_workspace_bytes / iq_pointconv_tables_bytes) and the same
 * limits on N, except PointNet++: N <= 1024 (its wide form takes "kept" from the coalition's 1024-point bitmap).  Only the
 * kernels that read a mask differ, so a coalition's logits are the narrow entry's on the same kept points, bit for bit - for
 * R <= 64 on the same mask.  PointNet++ runs sa1 without the region-reduced tables (they hold 64 regions): the member walk,
 * the same bits.  PointConv's per-cloud tables do not depend on the mask: `tables_state` and the tables at the head of the
 * workspace are shared with the narrow entry. */
int iq_dgcnn_coalitions_wide(const iq_dgcnn_weights* w, const float* clouds, const float* centers, const int32_t* region_id,
                             const uint64_t* keep /*B,W*/, const int32_t* cloud_of, float* logits, void* workspace,
                             size_t workspace_bytes, int B, int nclouds, int N, int fixed_graph, int R, iq_stream_t stream);
int iq_pointnet2_coalitions_wide(const iq_pointnet2_weights* w, const float* clouds, const float* centers,
                                 const int32_t* region_id, const uint64_t* keep /*B,W*/, const int32_t* cloud_of, float* logits,
                                 void* workspace, size_t workspace_bytes, int B, int nclouds, int N, int R, iq_stream_t stream);
int iq_pointconv_coalitions_wide(const iq_pointconv_weights* w, const float* clouds, const float* centers,
                                 const int32_t* region_id, const uint64_t* keep /*B,W*/, const int32_t* cloud_of, float* logits,
                                 void* workspace, size_t workspace_bytes, int B, int nclouds, int N, int R, iq_stream_t stream);
int iq_pointconv_coalitions_cached_wide(const iq_pointconv_weights* w, const float* clouds, const float* centers,
                                        const int32_t* region_id, const uint64_t* keep /*B,W*/, const int32_t* cloud_of,
                                        float* logits, void* workspace, size_t workspace_bytes, int B, int nclouds, int N,
                                        int* tables_state, int R, iq_stream_t stream);

/* The diagnostic entry points (HIP-event profiler, experiment knobs, debug counters) are NOT part of the drop-in surface:
 * they are declared in iq_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* IQ_H_ */
