/*
 * mvp_hip.h -- C ABI of libmvp_hip.so: the MI355X (gfx950) replacement for the six
 * CUDA extensions of maxjaritz/mvpnet plus the 2D->3D lifting that the reference runs
 * on the CPU inside its dataloader.
 *
 * This is the drop-in boundary.  The reference binds each op as a
 * pybind11 module taking at::Tensor; here every entry point takes plain DEVICE pointers
 * and sizes, an explicit HIP stream, and returns an int:
 *     0            success (kernel(s) enqueued on `stream`; nothing is synchronised)
 *     < 0          MVP_E* argument error, nothing was launched
 *     > 0          hipError_t reported by the launch
 * No entry point synchronises.  None allocates or keeps state either, with these exceptions: mvp_fps_* for float32 clouds of 8193..65536
 * points (a few KB per cloud: the exchange buffer of the workgroups that share a cloud) and for clouds beyond that (the running distances)
 * takes and returns a stream-ordered scratch (hipMallocAsync / hipFreeAsync on `stream`); the mvp_set_* switches are
 * process-wide DEFAULTS.  The kernels that let their last workgroup finalize keep their completion counter in caller memory (one extra
 * element behind `stat` / `acc`, zero on entry), so there is no device-side state shared between launches, streams, threads or graphs.
 * All tensors are dense row-major ("contiguous") in the stated shape.
 * Index tensors are int64 as in the reference (all reference index outputs are int64).
 *
 * Arithmetic contract: squared distances are
 * (dx*dx + dy*dy) + dz*dz with every operation individually rounded in T (no FMA
 * contraction); every tie is won by the lowest index.
 *
 * Reference interface each declaration replaces is cited as file:line relative to the
 * reference checkout.
 */
#ifndef MVP_HIP_H_
#define MVP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mvp_stream_t; /* hipStream_t; NULL = the null stream */

#define MVP_OK 0
#define MVP_EINVAL (-1)       /* shape / size precondition violated (reference: CHECK_* -> RuntimeError) */
#define MVP_EUNSUPPORTED (-2) /* valid request this build does not cover (e.g. k != 3 for knn_distance) */
#define MVP_ENULL (-3)        /* required pointer is NULL */

/* library version / build info; never fails */
const char* mvp_version(void);
/* human readable text for a return code of this library (static storage) */
const char* mvp_strerror(int code);

/* Launch shape of the sampling kernels for 4096 < N <= 8192 points: 0 (default) = the shortest dependency chain (16 waves per cloud),
 * 1 = half the waves (15 % longer chain, half the issue slots) for batches of >= 8 clouds whose chain runs hidden beside other kernels --
 * the prefetched geometry of a training step.  Same results either way (bit-exact goldens).  mvp_fps_shape_* take the shape PER CALL;
 * mvp_set_fps_mode only sets the process default that the reference-signature entry points mvp_fps_f32 / _f64 use (returns the old one). */
int mvp_set_fps_mode(int mode);

/* ---- farthest point sampling -------------------------------------------------------
 * replaces fps_cuda.farthest_point_sample  (mvpnet/ops/cuda/fps.cpp:7-13,
 * mvpnet/ops/cuda/fps_kernel.cu:144-180).  points (B,N,D) D in {2,3}; index (B,M).
 * index[b,0] = 0; index[b,i] = first argmax_j min_{l<i} d2(p_j, p_index[b,l]).
 * Preconditions (fps_kernel.cu:154-156): M > 0, N >= M. */
int mvp_fps_f32(const float* points, int64_t B, int64_t N, int64_t D, int64_t M, int64_t* index, mvp_stream_t stream);
int mvp_fps_f64(const double* points, int64_t B, int64_t N, int64_t D, int64_t M, int64_t* index, mvp_stream_t stream);
/* the same with the launch shape (0 / 1, see mvp_set_fps_mode) as an argument: nothing process-wide is read */
int mvp_fps_shape_f32(const float* points, int64_t B, int64_t N, int64_t D, int64_t M, int64_t* index, int shape, mvp_stream_t stream);
int mvp_fps_shape_f64(const double* points, int64_t B, int64_t N, int64_t D, int64_t M, int64_t* index, int shape, mvp_stream_t stream);
/* the same with a caller-provided DEVICE status word (may be NULL).  float32 clouds of 8193..65536 points are sampled by four workgroups
 * per cloud that wait for each other's row results; a workgroup that polls 2^22 times without seeing its partners (they were not resident
 * together: other streams held the CUs) gives up, leaves -1 in its rows and sets *status = 1 (sticky: the library never clears it).  The
 * one-workgroup kernel is queued right behind with the flag as its guard and re-samples the call's clouds when -- and only when -- the flag
 * is set, so `index` holds the exact chain in either case (reference contract: a failed launch is an error, never wrong indices --
 * fps_kernel.cu:177 THCudaCheck).  mvp_fps_debug_spin_limit(polls) sets the poll bound (<= 0: the default 2^22) and returns the old one:
 * a test hook that forces the time-out path. */
int mvp_fps_checked_f32(const float* points, int64_t B, int64_t N, int64_t D, int64_t M, int64_t* index, int shape, int* status,
                        mvp_stream_t stream);
int mvp_fps_debug_spin_limit(int polls);
/* Which kernel family the LAST mvp_fps_* call of the calling thread launched -- the choice is made inside the library from the cloud's shape
 * (and the MVP_FPS_ROUNDS=0 baseline switch), so tests assert it next to the oracle comparison: 0 none yet, 1 one sample per barrier
 * (fps_kernel / fps_fast_kernel), 2 fps_rounds_kernel, 3 fps_stream_kernel (4097..8192 float32 points: the training step's sampler),
 * 4 fps_rounds_multi_kernel (several workgroups per cloud), 5 fps_global_kernel.  A test aid: thread-local, no device work. */
int mvp_fps_last_kernel(void);
/* Centroids of a CHAIN of sampling levels from the first level's indices (mvpnet/models/pn2/modules.py:74-87 applied level after level,
 * pn2ssg.py:92-99): outs[l][b, m, :] = points[b, index[b, m], :] for m < counts[l], counts[0] = M >= counts[1] >= ... (host arrays of
 * `levels` <= 8 entries; outs[l] = device pointer to (B, counts[l], D)).  Farthest point sampling of a cloud that is itself the output of
 * a sampling run, in sampling order, returns 0, 1, 2, ...: the running distances of the second chain are the first chain's, its maxima are
 * attained by the same points, and every tie is won by the lowest index; when all remaining distances are 0 both chains return point 0,
 * whose coordinates the prefix holds as well -- so the deeper levels' centroid coordinates are the PREFIXES of the first level's. */
int mvp_fps_centroid_levels_f32(const float* points, const int64_t* index, int64_t B, int64_t N, int64_t D, int64_t M, int64_t levels,
                                const int64_t* counts, float* const* outs, mvp_stream_t stream);

/* ---- ball query ---------------------------------------------------------------------
 * replaces ball_query_cuda.ball_query (mvpnet/ops/cuda/ball_query.cpp:7-15,
 * ball_query_kernel.cu:147-187) and ball_query_distance_cuda.ball_query_distance
 * (ball_query_distance.cpp:7-15, ball_query_distance_kernel.cu:150-195).
 * query (B,N1,3), key (B,N2,3) -> index (B,N1,K) [, distance (B,N1,K)].
 * radius is a C float at the boundary and is squared in T (ball_query_kernel.cu:45,73).
 * First K keys in index order with d2 < r2 (strict); fewer than K hits: remaining index
 * slots repeat the first hit, remaining distance slots are -1; no hit: whole row -1. */
int mvp_ball_query_f32(const float* query, const float* key, int64_t B, int64_t N1, int64_t N2, float radius,
                       int64_t K, int64_t* index, mvp_stream_t stream);
int mvp_ball_query_f64(const double* query, const double* key, int64_t B, int64_t N1, int64_t N2, float radius,
                       int64_t K, int64_t* index, mvp_stream_t stream);
int mvp_ball_query_distance_f32(const float* query, const float* key, int64_t B, int64_t N1, int64_t N2, float radius,
                                int64_t K, int64_t* index, float* distance, mvp_stream_t stream);
int mvp_ball_query_distance_f64(const double* query, const double* key, int64_t B, int64_t N1, int64_t N2,
                                float radius, int64_t K, int64_t* index, double* distance, mvp_stream_t stream);
/* The same two operations for LARGE float32 clouds through a cell grid (csrc/ball_grid.hip): one build launch (bounding box, <= 16^3 cells
 * of edge >= 1.001 radius, counting sort) + one query launch that tests only the keys of the 27 cells around each query with the identical
 * float expression and reads the row off a per-query bitmap in key order -- bit-identical index / distance rows for every input (no cap on
 * the hits, non-finite coordinates included), ~20x fewer pair tests at the reference network's level 1 (8192 keys, radius 0.1).
 * mvp_ball_query_grid_workspace: bytes of device scratch the call needs, 0 = shape not taken (N2 < 2048, N2 > 32768 or fewer than 2^24 (query, key) pairs: use mvp_ball_query_f32).
 * The call itself takes any N2 <= 32768 with B * (16 N2 + 16512) bytes of scratch (the same figure).
 * distance == NULL: ball_query_cuda.ball_query; else ball_query_distance_cuda.ball_query_distance.  workspace: 16-byte aligned, reusable
 * once the launches have run (stream order). */
int64_t mvp_ball_query_grid_workspace(int64_t B, int64_t N1, int64_t N2);
int mvp_ball_query_grid_f32(const float* query, const float* key, int64_t B, int64_t N1, int64_t N2, float radius, int64_t K,
                            int64_t* index, float* distance, void* workspace, int64_t workspace_bytes, mvp_stream_t stream);
/* 3-NN through the same grid (replaces knn_distance_cuda.knn_distance, knn_distance_kernel.cu:35-124,150-190, + the weights of
 * FeatureInterpolator.forward, modules.py:135-140, as mvp_knn3_weights_f32 does): cells of extent / g per axis, g ~ cbrt(N2) / 1.3; 16 lanes
 * per query keep the three smallest (distance, key index) pairs of the 27 cells around the query -- strict < on the distance, the lower
 * index among equals, as the sweep -- and the triple stands when its third distance is below 0.999 x the distance to the nearest face
 * of the 27-cell block with keys beyond it; otherwise the lanes sweep all keys for that query.  Identical index / distance / weight on
 * every input.  weight and / or distance may be NULL.  mvp_knn3_grid_workspace: scratch bytes, 0 = stay with the sweep (fewer than 2^24
 * pairs, N2 < 256 or N2 > 65536); the call takes any 3 <= N2 <= 65536 with B * (16 N2 + 16512) bytes. */
int64_t mvp_knn3_grid_workspace(int64_t B, int64_t N1, int64_t N2);
int mvp_knn3_grid_f32(const float* query, const float* key, int64_t B, int64_t N1, int64_t N2, float eps, int64_t* index, float* weight,
                      float* distance, void* workspace, int64_t workspace_bytes, mvp_stream_t stream);

/* ---- group_points -------------------------------------------------------------------
 * replaces group_points_cuda.group_points_forward / _backward
 * (mvpnet/ops/cuda/group_points.cpp:7-19, group_points_kernel.cu:25-47, 99-145).
 * forward : input (B,C,N1), index (B,N2,K) -> out (B,C,N2,K), out[b,c,m,k] = input[b,c,index[b,m,k]]
 * backward: grad_out (B,C,N2,K), index -> grad_in (B,C,N1) (zero-filled here, then scatter-added).
 * Index values must lie in [0,N1); out-of-range values are skipped (forward writes 0). */
int mvp_group_points_forward_f32(const float* input, const int64_t* index, int64_t B, int64_t C, int64_t N1,
                                 int64_t N2, int64_t K, float* out, mvp_stream_t stream);
int mvp_group_points_forward_f64(const double* input, const int64_t* index, int64_t B, int64_t C, int64_t N1,
                                 int64_t N2, int64_t K, double* out, mvp_stream_t stream);
int mvp_group_points_backward_f32(const float* grad_out, const int64_t* index, int64_t B, int64_t C, int64_t N1,
                                  int64_t N2, int64_t K, float* grad_in, mvp_stream_t stream);
int mvp_group_points_backward_f64(const double* grad_out, const int64_t* index, int64_t B, int64_t C, int64_t N1,
                                  int64_t N2, int64_t K, double* grad_in, mvp_stream_t stream);
/* The same with a STRIDED feature operand, walked in place as the reference's TensorInfo path does (group_points_kernel.cu:131-133)
 * instead of being copied: sb, sc, sn = element strides of input (B,C,N1); sb, sc, sm, sk = element strides of grad_out (B,C,N2,K).
 * Any layout (a transposed channels-last view, a slice of a wider tensor); index and outputs stay contiguous. */
int mvp_group_points_forward_strided_f32(const float* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, int64_t B,
                                         int64_t C, int64_t N1, int64_t N2, int64_t K, float* out, mvp_stream_t stream);
int mvp_group_points_forward_strided_f64(const double* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, int64_t B,
                                         int64_t C, int64_t N1, int64_t N2, int64_t K, double* out, mvp_stream_t stream);
int mvp_group_points_backward_strided_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t sm, int64_t sk, const int64_t* index,
                                          int64_t B, int64_t C, int64_t N1, int64_t N2, int64_t K, float* grad_in, mvp_stream_t stream);
int mvp_group_points_backward_strided_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sm, int64_t sk, const int64_t* index,
                                          int64_t B, int64_t C, int64_t N1, int64_t N2, int64_t K, double* grad_in, mvp_stream_t stream);
/* bfloat16 VALUES (uint16_t = the bf16 bit pattern; SURVEY 8b: "+bf16 for gather/interp/MLP values"): the gather is a copy (bit-exact);
 * the backward accumulates in fp32 and rounds ONCE to bf16 when the sums are written (clouds whose fp32 sums do not fit the LDS of a
 * workgroup, N1 > 30720, go through stream-ordered fp32 scratch). */
int mvp_group_points_forward_bf16(const uint16_t* input, const int64_t* index, int64_t B, int64_t C, int64_t N1, int64_t N2, int64_t K,
                                  uint16_t* out, mvp_stream_t stream);
int mvp_group_points_backward_bf16(const uint16_t* grad_out, const int64_t* index, int64_t B, int64_t C, int64_t N1, int64_t N2, int64_t K,
                                   uint16_t* grad_in, mvp_stream_t stream);
int mvp_group_points_forward_strided_bf16(const uint16_t* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, int64_t B,
                                          int64_t C, int64_t N1, int64_t N2, int64_t K, uint16_t* out, mvp_stream_t stream);
int mvp_group_points_backward_strided_bf16(const uint16_t* grad_out, int64_t sb, int64_t sc, int64_t sm, int64_t sk, const int64_t* index,
                                           int64_t B, int64_t C, int64_t N1, int64_t N2, int64_t K, uint16_t* grad_in, mvp_stream_t stream);

/* ---- 3-NN with squared distances ------------------------------------------------------
 * replaces knn_distance_cuda.knn_distance (mvpnet/ops/cuda/knn_distance.cpp:8-15,
 * knn_distance_kernel.cu:154-196).  query (B,N1,3), key (B,N2,3) -> index (B,N1,3),
 * distance (B,N1,3) ascending, SQUARED; k must be 3 (knn_distance_kernel.cu:171) and
 * N2 >= k (:167-170). */
int mvp_knn_distance_f32(const float* query, const float* key, int64_t B, int64_t N1, int64_t N2, int64_t k,
                         int64_t* index, float* distance, mvp_stream_t stream);
int mvp_knn_distance_f64(const double* query, const double* key, int64_t B, int64_t N1, int64_t N2, int64_t k,
                         int64_t* index, double* distance, mvp_stream_t stream);
/* 3-NN + FeatureInterpolator's weights (mvpnet/models/pn2/modules.py:135-140) in one launch:
 *   weight[b,n,k] = (1 / max(d2_k, eps)) / sum_j (1 / max(d2_j, eps)), every operation rounded once (float32);
 *   distance may be NULL.  N2 >= 3. */
int mvp_knn3_weights_f32(const float* query, const float* key, int64_t B, int64_t N1, int64_t N2, float eps, int64_t* index,
                         float* weight, float* distance, mvp_stream_t stream);

/* ---- feature interpolation (K = 3) ----------------------------------------------------
 * replaces interpolate_cuda.interpolate_forward / _backward
 * (mvpnet/ops/cuda/interpolate.cpp:8-22, interpolate_kernel.cu:78-124, 184-230).
 * forward : input (B,C,N1), index (B,N2,3), weight (B,N2,3) -> out (B,C,N2)
 * backward: grad_out (B,C,N2) -> grad_in (B,C,N1) (zero-filled here; gradient to input only). */
int mvp_interpolate_forward_f32(const float* input, const int64_t* index, const float* weight, int64_t B, int64_t C,
                                int64_t N1, int64_t N2, float* out, mvp_stream_t stream);
int mvp_interpolate_forward_f64(const double* input, const int64_t* index, const double* weight, int64_t B,
                                int64_t C, int64_t N1, int64_t N2, double* out, mvp_stream_t stream);
int mvp_interpolate_backward_f32(const float* grad_out, const int64_t* index, const float* weight, int64_t B,
                                 int64_t C, int64_t N1, int64_t N2, float* grad_in, mvp_stream_t stream);
int mvp_interpolate_backward_f64(const double* grad_out, const int64_t* index, const double* weight, int64_t B,
                                 int64_t C, int64_t N1, int64_t N2, double* grad_in, mvp_stream_t stream);
/* Strided feature operand (interpolate_kernel.cu:108-111 walks TensorInfo): sb, sc, sn = element strides of input (B,C,N1) /
 * grad_out (B,C,N2).  index, weight and the outputs stay contiguous. */
int mvp_interpolate_forward_strided_f32(const float* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, const float* weight,
                                        int64_t B, int64_t C, int64_t N1, int64_t N2, float* out, mvp_stream_t stream);
int mvp_interpolate_forward_strided_f64(const double* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index, const double* weight,
                                        int64_t B, int64_t C, int64_t N1, int64_t N2, double* out, mvp_stream_t stream);
int mvp_interpolate_backward_strided_f32(const float* grad_out, int64_t sb, int64_t sc, int64_t sn, const int64_t* index,
                                         const float* weight, int64_t B, int64_t C, int64_t N1, int64_t N2, float* grad_in,
                                         mvp_stream_t stream);
int mvp_interpolate_backward_strided_f64(const double* grad_out, int64_t sb, int64_t sc, int64_t sn, const int64_t* index,
                                         const double* weight, int64_t B, int64_t C, int64_t N1, int64_t N2, double* grad_in,
                                         mvp_stream_t stream);
/* bfloat16 VALUES (uint16_t = the bf16 bit pattern), fp32 weights: the fp32 kernel's arithmetic on the widened values,
 * out = bf16_rn((f0 w0 + f1 w1) + f2 w2); the backward adds g w_k in fp32 and rounds ONCE to bf16 when the sums are written. */
int mvp_interpolate_forward_bf16(const uint16_t* input, const int64_t* index, const float* weight, int64_t B, int64_t C, int64_t N1,
                                 int64_t N2, uint16_t* out, mvp_stream_t stream);
int mvp_interpolate_backward_bf16(const uint16_t* grad_out, const int64_t* index, const float* weight, int64_t B, int64_t C, int64_t N1,
                                  int64_t N2, uint16_t* grad_in, mvp_stream_t stream);
int mvp_interpolate_forward_strided_bf16(const uint16_t* input, int64_t sb, int64_t sc, int64_t sn, const int64_t* index,
                                         const float* weight, int64_t B, int64_t C, int64_t N1, int64_t N2, uint16_t* out,
                                         mvp_stream_t stream);
int mvp_interpolate_backward_strided_bf16(const uint16_t* grad_out, int64_t sb, int64_t sc, int64_t sn, const int64_t* index,
                                          const float* weight, int64_t B, int64_t C, int64_t N1, int64_t N2, uint16_t* grad_in,
                                          mvp_stream_t stream);

/* ---- 2D -> 3D lifting (NEW on the device; the reference does this in dataloader workers) ----
 * un-projection: replaces depth2xyz + pose + masks of ScanNet2D3DChunks.get_rgbd_data
 * (mvpnet/data/scannet_2d3d.py:33-39, 255-281).
 *   depth   (B,nv,h,w)  metres float32, or millimetres uint16 (= PNG/1000, :255)
 *   kinv    (B,nv,3,3)  float32 inverse intrinsics (np.linalg.inv(cam_matrix[:3,:3]), :38)
 *   pose    (B,nv,4,4)  float32 camera-to-world
 *   box     (B,4)       float32 (x_min,y_min,x_max,y_max) ALREADY expanded by the 0.1 m margin, or NULL
 *   -> image_xyz (B,nv,h,w,3) float32 (float64 math rounded once, like :317), mask (B,nv,h,w) uint8
 *   pixel (row v, col u): X_w = R.(Kinv.[u,v,1]^T * depth) + t;  mask = z_cam > 0 && inside box (x,y). */
int mvp_unproject_f32(const float* depth_m, const float* kinv, const float* pose, const float* box, int64_t B,
                      int64_t nv, int64_t h, int64_t w, float* image_xyz, uint8_t* mask, mvp_stream_t stream);
int mvp_unproject_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, const float* box, int64_t B,
                      int64_t nv, int64_t h, int64_t w, float* image_xyz, uint8_t* mask, mvp_stream_t stream);

/* pixel k-NN: replaces NearestNeighbors(k,'ball_tree').fit(valid).kneighbors(points) + remap
 * (mvpnet/data/scannet_2d3d.py:297-313).  Exact k nearest VALID pixels per chunk point,
 * ascending, ties -> lowest flat pixel id  view*h*w + row*w + col.
 *   image_xyz (B,P,3) float32, mask (B,P) uint8, points (B,N,3) float32, 1 <= k <= 8
 *   -> index (B,N,k) int64 [, distance (B,N,k) float32 squared, may be NULL]; missing -> -1.
 * _bruteforce: O(N*P) scan, needs no camera model.
 * _projective: same result; uses the pin-hole structure (cam (B,nv,3,3) forward intrinsics,
 *   pose (B,nv,4,4)) to search an image window around each point's projection and widens it
 *   until a conservative bound proves exactness; P = nv*h*w. */
int mvp_pixel_knn_bruteforce_f32(const float* image_xyz, const uint8_t* mask, const float* points, int64_t B,
                                 int64_t P, int64_t N, int64_t k, int64_t* index, float* distance,
                                 mvp_stream_t stream);
int mvp_pixel_knn_projective_f32(const float* image_xyz, const uint8_t* mask, const float* points, const float* cam,
                                 const float* pose, int64_t B, int64_t nv, int64_t h, int64_t w, int64_t N,
                                 int64_t k, int64_t* index, float* distance, mvp_stream_t stream);

/* lifting gather, channels-last: replaces the two group_points calls of MVPNet3D.forward
 * (mvpnet/models/mvpnet_3d.py:99-109) without the transpose().contiguous() copy of :101.
 *   feature (B,P,C) float32 (= (B,nv,h,w,C)), image_xyz (B,P,3), index (B,N,k) int64
 *   -> gfeature (B,N,k,C), gxyz (B,N,k,3) (either output may be NULL).
 * backward (only needed when the 2D network is trained): grad_gfeature (B,N,k,C) -> grad_feature (B,P,C),
 * zero-filled here. */
int mvp_lift_gather_f32(const float* feature, const float* image_xyz, const int64_t* index, int64_t B, int64_t P,
                        int64_t C, int64_t N, int64_t k, float* gfeature, float* gxyz, mvp_stream_t stream);
int mvp_lift_gather_backward_f32(const float* grad_gfeature, const int64_t* index, int64_t B, int64_t P, int64_t C,
                                 int64_t N, int64_t k, float* grad_feature, mvp_stream_t stream);
/* The same gradient as a GATHER: reproducible, no zero fill, no float atomics (csrc/lift_bwd.hip).  With E = N*k and e = n*k + slot:
 *   grad_feature[b,j,:] is an accumulator that starts at +0.0f and adds grad_gfeature[b,e,:] for every e with index[b,e] == j, in
 *   ASCENDING e, by plain float32 additions (one rounding each) -- the sequential loop over the chunk's edges.  The result is a function
 *   of the inputs alone; mvp_lift_gather_backward_f32 adds the same terms in the order its atomics arrive.
 *   grad_gfeature (B,N,k,C), index (B,N,k) int64 as the mvp_lift_* entries write it (flat pixel ids, mirrored ids for flipped views, -1
 *   for a missing neighbour): an index outside [0,P) is ignored, never an address.
 *   -> grad_feature (B,P,C): EVERY element is written (the caller does not pre-fill; a pixel nobody names gets +0.0f).
 *   workspace: caller-owned device scratch of mvp_lift_backward_workspace_bytes(B,P,N,k) bytes, 16-byte aligned (else MVP_EINVAL),
 *   reusable once the launches have run (stream order): the transposed index, offsets (B,P+1) and slots (B,E) int32, built by the first
 *   launch with integer LDS atomics on counters only (every list is then sorted); the second launch walks the lists and stores the rows.
 *   C % 4 == 0 with 16-byte aligned grad_gfeature / grad_feature: 16 bytes per lane (C = 20, MVPNet2D's logits, included); any other C:
 *   one element per lane.  E == 0 still writes the zero map; C == 0 or B == 0 does nothing.
 *   Positions and pixels are 32-bit inside: E >= 2^31, P >= 2^31 or B >= 65536 is MVP_EUNSUPPORTED (the workspace size is then 0, as
 *   for a negative argument).  All checks come before the first launch. */
int64_t mvp_lift_backward_workspace_bytes(int64_t B, int64_t P, int64_t N, int64_t k);
int mvp_lift_backward_f32(const float* grad_gfeature, const int64_t* index, int64_t B, int64_t P, int64_t C,
                          int64_t N, int64_t k, void* workspace, float* grad_feature, mvp_stream_t stream);

/* fused lifting: un-projection + exact pixel k-NN + channels-last gather in two launches
 * (replaces scannet_2d3d.py:254-313 + mvpnet_3d.py:99-109 end to end).
 *   depth (B,nv,h,w) float32 metres (depth_is_u16 = 0) or uint16 millimetres (= 1); kinv, cam (B,nv,3,3);
 *   pose (B,nv,4,4); box (B,4) or NULL; points (B,N,3); feature (B,nv,h,w,C) channels-last, C % 4 == 0
 *   workspace: caller-owned device scratch of mvp_lift_workspace_bytes(B,nv,h,w,N) bytes, 16-byte aligned
 *   -> knn_index (B,N,k) int64, gfeature (B,N,k,C) or NULL, gxyz (B,N,k,3) or NULL,
 *      image_xyz (B,nv,h,w,3) or NULL, mask (B,nv,h,w) or NULL   (same values as the separate entry points). */
int64_t mvp_lift_workspace_bytes(int64_t B, int64_t nv, int64_t h, int64_t w, int64_t N);
int mvp_lift_f32(const void* depth, int depth_is_u16, const float* kinv, const float* cam, const float* pose,
                 const float* box, const float* points, const float* feature, int64_t B, int64_t nv, int64_t h,
                 int64_t w, int64_t N, int64_t C, int64_t k, void* workspace, int64_t* knn_index, float* gfeature,
                 float* gxyz, float* image_xyz, uint8_t* mask, mvp_stream_t stream);
/* mvp_lift_f32 + the loader's augmentation applied where the reference applies it (mvpnet/data/scannet_2d3d.py):
 *   flip (B,nv) uint8 or NULL: views mirrored horizontally AFTER the un-projection (:293-296: image, image_xyz, image_mask are
 *        `np.fliplr`ed) -> knn_index holds the mirrored flat ids `view*h*w + row*w + (w-1-col)`, `feature` is indexed in mirrored
 *        order (the 2D network saw the mirrored image), image_xyz / mask are written mirrored; equal distances are ordered by
 *        the sensor-order id (the ball tree's tie order is unspecified upstream);
 *   rot (B,3,3) float64 row-major or NULL: rotation applied AFTER the k-NN search (:400-409, `Rotation.apply` = float64 product,
 *        one rounding to float32) to the gathered xyz and to the points -> points_out (B,N,3) or NULL.  The public image_xyz
 *        tensor is not rotated by this call (the model never reads it; mvp_rotate_rows_f32 does it on request). */
int mvp_lift_aug_f32(const void* depth, int depth_is_u16, const float* kinv, const float* cam, const float* pose,
                     const float* box, const float* points, const float* feature, int64_t B, int64_t nv, int64_t h,
                     int64_t w, int64_t N, int64_t C, int64_t k, void* workspace, int64_t* knn_index, float* gfeature,
                     float* gxyz, float* image_xyz, uint8_t* mask, const uint8_t* flip, const double* rot, float* points_out,
                     mvp_stream_t stream);
/* mvp_lift_f32 with the feature rows read from a store shared by all chunks (whole-scene test: every distinct frame goes through the
 * 2D network once, scene.infer_scene_shared) instead of a per-batch (B,nv,h,w,C) tensor.  Forward only; no flip, no rotation.
 *   store (U,h,w,C) float32 channels-last, 16-byte aligned: one feature map per distinct frame, U * h * w < 2^31 (else
 *        MVP_EUNSUPPORTED); view_slot (B,nv) int32: the store slot of view v of chunk b;
 *   depth, kinv, cam, pose, box, points, workspace (mvp_lift_workspace_bytes), the shape limits: as mvp_lift_f32
 *   -> knn_index (B,N,k) int64: the chunk-local flat ids view*h*w + pixel, what mvp_lift_f32 writes; gfeature (B,N,k,C) (required):
 *      neighbour id = v*h*w + p of chunk b is row view_slot[b,v]*h*w + p of the store -- a slot outside [0,U) counts as a missing
 *      neighbour: a zero row, never an address (the convention of mvp_lift_vote_f32) --; gxyz (B,N,k,3) or NULL.
 *   Bit-equal to mvp_lift_f32 on the materialised copy store[view_slot]. */
int mvp_lift_store_f32(const void* depth, int depth_is_u16, const float* kinv, const float* cam, const float* pose,
                       const float* box, const float* points, const float* store, const int32_t* view_slot, int64_t U,
                       int64_t B, int64_t nv, int64_t h, int64_t w, int64_t N, int64_t C, int64_t k, void* workspace,
                       int64_t* knn_index, float* gfeature, float* gxyz, mvp_stream_t stream);
/* ---- lifting from 16-bit feature maps and stores: the rows are widened in the gather, no float32 copy is made ----
 * The four entries below are their `_f32` siblings with the feature map / store as `const void*` followed by `int feature_type`
 * (the `depth, depth_is_u16` convention): bfloat16 or float16 elements, 16-byte aligned (else MVP_EINVAL); any other feature_type is
 * MVP_EINVAL.  Everything else -- the other inputs, the shape limits, the checks, the outputs, `float* gfeature` included -- is the
 * sibling's.  Widening bfloat16 / float16 to float32 is exact (subnormals, infinities and signed zeros included), so the results do not
 * depend on where it happens.  Forward only: there is no backward entry for a 16-bit map. */
#define MVP_FEATURE_BF16 1
#define MVP_FEATURE_F16 2
/* mvp_lift_gather_f32 on a 16-bit feature (B,P,C): bit-equal to the `_f32` entry on the exactly widened copy.  C % 4 != 0 is served
 * (one element per lane), as there. */
int mvp_lift_gather_h16(const void* feature, int feature_type, const float* image_xyz, const int64_t* index, int64_t B, int64_t P,
                        int64_t C, int64_t N, int64_t k, float* gfeature, float* gxyz, mvp_stream_t stream);
/* mvp_lift_f32 on a 16-bit feature (B,nv,h,w,C), C % 4 == 0: bit-equal to the `_f32` entry on the exactly widened copy. */
int mvp_lift_h16(const void* depth, int depth_is_u16, const float* kinv, const float* cam, const float* pose,
                 const float* box, const float* points, const void* feature, int feature_type, int64_t B, int64_t nv, int64_t h,
                 int64_t w, int64_t N, int64_t C, int64_t k, void* workspace, int64_t* knn_index, float* gfeature,
                 float* gxyz, float* image_xyz, uint8_t* mask, mvp_stream_t stream);
/* mvp_lift_aug_f32 on a 16-bit feature (B,nv,h,w,C), C % 4 == 0: bit-equal to the `_f32` entry on the exactly widened copy. */
int mvp_lift_aug_h16(const void* depth, int depth_is_u16, const float* kinv, const float* cam, const float* pose,
                     const float* box, const float* points, const void* feature, int feature_type, int64_t B, int64_t nv, int64_t h,
                     int64_t w, int64_t N, int64_t C, int64_t k, void* workspace, int64_t* knn_index, float* gfeature,
                     float* gxyz, float* image_xyz, uint8_t* mask, const uint8_t* flip, const double* rot, float* points_out,
                     mvp_stream_t stream);
/* mvp_lift_store_f32 on a 16-bit store (U,h,w,C), C % 4 == 0: bit-equal to the `_f32` entry on the exactly widened copy.  A given
 * number of bytes holds twice the frames. */
int mvp_lift_store_h16(const void* depth, int depth_is_u16, const float* kinv, const float* cam, const float* pose,
                       const float* box, const float* points, const void* store, int feature_type, const int32_t* view_slot,
                       int64_t U, int64_t B, int64_t nv, int64_t h, int64_t w, int64_t N, int64_t C, int64_t k, void* workspace,
                       int64_t* knn_index, float* gfeature, float* gxyz, mvp_stream_t stream);
/* out[b,r,:] = float32( rot[b] (float64 3x3) . xyz[b,r,:] ), rows R per batch element: the z-rotation augmentation of `points`
 * / `image_xyz` (scannet_2d3d.py:400-409) for tensors that did not go through mvp_lift_aug_f32.  In place allowed. */
int mvp_rotate_rows_f32(const float* xyz, const double* rot, int64_t B, int64_t R, float* out, mvp_stream_t stream);

/* ---- frame selection inputs (NEW on the device; the reference computes the overlap offline) ----
 * RGB-D overlap: replaces compute_rgbd_knn (mvpnet/data/preprocess/preprocess.py:99-170: un-project every frame, look up each
 * pixel's nearest base point in an open3d KD-tree, max_nn = 1, mark it when closer than 0.1 m).
 *   depth (F,h,w) metres float32 or millimetres uint16; kinv (F,3,3), pose (F,4,4) float32; base_points (nb,3) float32
 *   -> overlap_bits (F,W) uint32, W = ceil(nb / 32), zero-filled here: bit j % 32 of word j / 32 of row f = frame f sees base point j.
 * Pinned definition:
 *   - a pixel's world point is what mvp_unproject_* writes for it with box = NULL, and it takes part when that mask is set (z_cam > 0);
 *   - a frame with a non-finite entry in its 4x4 pose is skipped, its row stays zero (preprocess.py:137-139);
 *   - j* = argmin_j d2, d2 = (dx*dx + dy*dy) + dz*dz in float32 without contraction (the arithmetic of the ball query), lowest j on ties;
 *   - bit (f, j*) is set iff d2 < fl32(fl32(radius) * fl32(radius)); only the nearest point is marked (preprocess.py:156).
 * The base points are held in LDS: nb <= MVP_OVERLAP_MAX_BASE, MVP_EUNSUPPORTED beyond.  F * h * w < 2^31, radius >= 0. */
#define MVP_OVERLAP_MAX_BASE 4096
int mvp_frame_overlap_f32(const float* depth_m, const float* kinv, const float* pose, const float* base_points, int64_t F, int64_t h,
                          int64_t w, int64_t nb, float radius, uint32_t* overlap_bits, mvp_stream_t stream);
int mvp_frame_overlap_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, const float* base_points, int64_t F, int64_t h,
                          int64_t w, int64_t nb, float radius, uint32_t* overlap_bits, mvp_stream_t stream);

/* greedy frame selection for all chunks of a scene in one launch: per chunk c the result of
 * select_frames(pointwise_rgbd_overlap[base points of the chunk], n_pick) (mvpnet/data/scannet_2d3d.py:20-30, called from :204-220).
 *   overlap_bits (F,W) as above; chunk_bits (C,W): bit j of row c = base point j lies in chunk c
 *   -> picked (C,n_pick) int64 frame indices; gain (C,n_pick) int32 or NULL: base points of the chunk newly covered by each pick.
 * Each pick takes the frame covering most still-uncovered base points of the chunk, the LOWEST frame index on ties (numpy.argmax) --
 * frame 0 again and again once nothing is left to cover.  F >= 1; W <= 1024 (32768 base points), MVP_EUNSUPPORTED beyond. */
int mvp_select_frames_u32(const uint32_t* overlap_bits, const uint32_t* chunk_bits, int64_t F, int64_t C, int64_t W, int64_t n_pick,
                          int64_t* picked, int32_t* gain, mvp_stream_t stream);

/* the same greedy selection for chunks of DIFFERENT scenes (a training batch): overlap_bits (Ftot,W) holds all scenes' frame rows
 * one scene after the other; chunk c chooses among rows [frame_begin[c], frame_begin[c] + frame_count[c]) only (both (C,) int64 ON THE
 * DEVICE), by the rule above with the lowest row on ties, and gets GLOBAL row indices in picked (C,n_pick); gain as above.
 * frame_count[c] >= 1 and the range inside [0, Ftot) are the caller's, like any index array's contents (the entry cannot read the
 * device arrays without a synchronisation): a range is cut to [0, Ftot) and a chunk left with no frame gets picked = -1, gain = 0 --
 * no row outside the matrix is read.  Ftot >= 1 (MVP_EINVAL: no chunk could have a frame); W <= 1024, MVP_EUNSUPPORTED beyond. */
int mvp_select_frames_ranges_u32(const uint32_t* overlap_bits, const uint32_t* chunk_bits, const int64_t* frame_begin,
                                 const int64_t* frame_count, int64_t Ftot, int64_t C, int64_t W, int64_t n_pick, int64_t* picked,
                                 int32_t* gain, mvp_stream_t stream);

/* ---- scene cloud from RGB-D frames (NEW on the device; csrc/fuse_cloud.hip) ----
 * Replaces the one input the whole-scene calls could not make: the reference reads `points` from the vertices of ScanNet's offline mesh
 * reconstruction (mvpnet/data/preprocess/preprocess.py:204, the PLY of the scan).  Here the cloud is a voxel-grid fusion of the
 * un-projected depth pixels, in integers, so the result does not depend on the order in which frames or pixels arrive.
 *   depth (F,h,w) metres float32 or millimetres uint16; kinv (F,3,3), pose (F,4,4) float32; images (F,h,w,3) uint8 or NULL
 * Pinned definition, per pixel (f, v, u):
 *   - X = the float32 world point mvp_unproject_* writes for it with box = NULL (float64 math, rounded once);
 *   - valid iff z_cam > 0 (that mask), the three coordinates are finite with |coordinate| < 32768, depth_min <= d <= depth_max on the
 *     float32 depth in metres (pass -INFINITY / INFINITY for no bound; a NaN depth is never valid), and every voxel index
 *     i_a = floor((double)X_a / voxel) -- a float64 DIVISION -- lies in [-2^20, 2^20).  Invalid pixels are ignored;
 *   - key = ((i_z + 2^20) << 42) | ((i_y + 2^20) << 21) | (i_x + 2^20), unsigned 64-bit; all ones = the empty mark (no valid key);
 *   - the voxel's count += 1, sum_a += llrint((double)X_a * 65536) (int64, nearest even), and with images csum_c += channel (uint64).
 * The table is caller memory of mvp_fuse_cloud_table_bytes(capacity, colors) bytes, 8-byte aligned, `capacity` a power of two:
 *     uint64 key[capacity] | int64 sum[capacity][3] | uint64 csum[capacity][3] (only with colors != 0) | uint32 count[capacity] |
 *     uint32 overflow[2]                                                      (the size rounded up to a multiple of 8)
 * The caller fills key[] with all ones and everything behind it with zero before the first insert; any number of inserts may follow.
 * Open addressing, linear probing from a mix of the key: a 64-bit compare-and-swap claims or finds the slot (old == empty or old == key:
 * this slot; otherwise the next one), then integer atomic adds.  The probe loop is bounded by `capacity` steps and never waits for
 * another lane.  A pixel that finds neither its key nor an empty slot sets overflow[0] = 1 and is dropped: nothing outside the table is
 * written.  No allocation, no synchronisation.
 *
 * mvp_fuse_cloud_table_bytes: the table's size; 0 unless capacity is a power of two in [1, 2^31).
 * mvp_fuse_cloud_insert_*: MVP_ENULL (depth, kinv, pose, table); MVP_EINVAL for F < 0, h or w < 1, voxel not finite or <= 0, a NaN
 *   bound, capacity < 1 or not a power of two, images given with colors == 0; MVP_EUNSUPPORTED for F*h*w >= 2^31 or capacity >= 2^31.
 *   F == 0: nothing is launched.
 * mvp_fuse_cloud_finish: slots (n,) int64 = the table slots that survive, in ascending key order (the caller's compaction and sort;
 *   a slot outside [0, capacity) is skipped); one lane per output row r:
 *     points[r,a] = (float)((double)sum_a / (double)count * 2^-16);  colors[r,c] = (2 * csum_c + count) / (2 * count) as uint8
 *     counts[r] = count as int32;  rank_of_slot[slots[r]] = r   (rank_of_slot (capacity,) int32, filled with -1 by the caller)
 *   MVP_ENULL (table, slots, points, counts, rank_of_slot); MVP_EINVAL for n < 0, n > capacity, a bad capacity, colors_out given with
 *   colors == 0; MVP_EUNSUPPORTED for capacity >= 2^31.  n == 0: nothing is launched.
 * mvp_fuse_cloud_lookup_*: pixel_point (F,h,w) int32 = rank_of_slot[slot of the pixel's key], -1 for an invalid pixel (same rule, same
 *   bounds) and for a key the table does not hold; the probe only reads.  Any frames, fused ones or others.  Errors as for insert, and
 *   MVP_ENULL for rank_of_slot or pixel_point. */
size_t mvp_fuse_cloud_table_bytes(int64_t capacity, int colors);
int mvp_fuse_cloud_insert_f32(const float* depth_m, const float* kinv, const float* pose, const uint8_t* images, int64_t F, int64_t h,
                              int64_t w, double voxel, float depth_min, float depth_max, void* table, int64_t capacity, int colors,
                              mvp_stream_t stream);
int mvp_fuse_cloud_insert_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, const uint8_t* images, int64_t F, int64_t h,
                              int64_t w, double voxel, float depth_min, float depth_max, void* table, int64_t capacity, int colors,
                              mvp_stream_t stream);
int mvp_fuse_cloud_finish(const void* table, int64_t capacity, int colors, const int64_t* slots, int64_t n, float* points,
                          uint8_t* colors_out, int32_t* counts, int32_t* rank_of_slot, mvp_stream_t stream);
int mvp_fuse_cloud_lookup_f32(const float* depth_m, const float* kinv, const float* pose, int64_t F, int64_t h, int64_t w, double voxel,
                              float depth_min, float depth_max, const void* table, int64_t capacity, const int32_t* rank_of_slot,
                              int32_t* pixel_point, mvp_stream_t stream);
int mvp_fuse_cloud_lookup_u16(const uint16_t* depth_mm, const float* kinv, const float* pose, int64_t F, int64_t h, int64_t w,
                              double voxel, float depth_min, float depth_max, const void* table, int64_t capacity,
                              const int32_t* rank_of_slot, int32_t* pixel_point, mvp_stream_t stream);

/* ---- training chunks (NEW on the device; the reference draws them in a data-loader worker) ----
 * One call draws B training chunks from resident scenes: ScanNet2D3DChunks.__getitem__ (mvpnet/data/scannet_2d3d.py:341-381) and the
 * base-point mask of get_rgbd_data (:199-204), without a host synchronisation and without an allocation (graph-capturable).
 *   points (Ntot,3) float32, seg_label (Ntot,) int64: S scenes one after the other, labels already mapped (negative = unlabelled);
 *   scene_offsets (S+1,) int64; scene_of_chunk (B,) int64 (a scene may occur more than once); center_ind (B,T) int64: the centres to
 *   try, point indices inside the chunk's scene (the reference tries T = 10); base_point_ind (S,nbp) int64 indices inside each scene, or
 *   NULL with nbp = 0.  All on the device.  Index arrays' contents are the caller's: out-of-range values are clamped into the arrays
 *   (a wrong result, never a stray access).
 * The try rule, in float32, each operation rounded once, never contracted (float32 chunk_size / chunk_margin as in :134-136):
 *   c = xy[center_ind[b,t]];  lo = (c - 0.5f*size) - margin;  hi = (c + 0.5f*size) + margin   (size, margin rounded to float32 first)
 *   point j is a member iff x >= lo.x && x <= hi.x && y >= lo.y && y <= hi.y (inclusive; a NaN coordinate is never a member);
 *   m = members, l = members with label >= 0; try t passes iff m > 0 && (double)l / (double)m >= chunk_thresh (numpy.mean of a bool
 *   array against the Python float, :358-362).  The first passing t wins: try_index[b] = t, chunk_box[b] = (lo.x, lo.y, hi.x, hi.y).
 * Fallback (:364-369), no try passes: try_index = -1, EVERY point of the scene is a member, chunk_box = (min_xy - margin, max_xy + margin)
 *   in float32 (numpy.min / max: a NaN coordinate makes that bound NaN).
 * bounds_f64 != 0: lo, hi in float64 from the float32 centre and the float64 size / margin, float32 coordinates compared as doubles --
 *   ScanNet3DChunks (mvpnet/data/scannet_3d.py:128-162); chunk_box holds the bounds rounded to float32.
 * Resampling to nb_pts (:374-381; the reference's law, the draws are a counter hash as for the dropout mask): h = lowbias32
 *   (csrc/dropout.h), seed32 = low ^ high word of the seed (*seed_device when that pointer is not NULL: one int64 ON THE DEVICE, so a
 *   replayed graph can draw afresh; else `seed`), s_b = h(seed32 + 0x9E3779B9 * (b+1)), members = the member indices, ascending.
 *   pad (m < nb_pts):  choice[b,s] = members[s] for s < m, members[((uint64)h(s ^ s_b ^ 0x85EBCA6B) * m) >> 32] for s >= m;
 *   crop (m >= nb_pts): the member with point index j has key h(j ^ s_b) -- h is a bijection, the keys of a chunk are distinct --,
 *     choice[b,s] = the member with the s-th smallest key: a random subset in random ORDER (not in mesh-vertex order, which would bias
 *     ball query's first-32 rule and FPS's start at slot 0).
 * Outputs: choice (B,nb_pts) int64 indices inside the scene; out_points (B,3,nb_pts) float32; out_label (B,nb_pts) int64; chunk_box
 *   (B,4) float32; try_index (B,), num_members (B,) int32; base_bits (B,ceil(nbp/32)) uint32 when nbp > 0: bit j % 32 of word j / 32 =
 *   base point j of the chunk's scene is a member (the rows mvp_select_frames_ranges_u32 reads; padding bits zero).
 * Every result is a function of the arguments alone (integer counts, distinct keys): bit-reproducible.
 * Limits: nb_pts <= MVP_SAMPLE_MAX_PTS (the crop sorts its (key, index) pairs in 64 KiB of LDS), T <= MVP_SAMPLE_MAX_TRIES,
 *   Ntot < 2^31 (so every scene's n < 2^31), B <= MVP_SAMPLE_MAX_CHUNKS: MVP_EUNSUPPORTED beyond, nothing is launched.  MVP_EINVAL
 *   unless Ntot, S, T, nb_pts >= 1, B, nbp >= 0, no NaN among size / margin / chunk_thresh, workspace 16-byte aligned with
 *   workspace_bytes >= mvp_sample_chunks_workspace(Ntot, B, T, nb_pts) (0 for shapes the call refuses).  The scratch is reusable once
 *   the launches have run (stream order). */
#define MVP_SAMPLE_MAX_PTS 8192
#define MVP_SAMPLE_MAX_TRIES 32
#define MVP_SAMPLE_MAX_CHUNKS 65535
int64_t mvp_sample_chunks_workspace(int64_t Ntot, int64_t B, int64_t T, int64_t nb_pts);
int mvp_sample_chunks_f32(const float* points, const int64_t* seg_label, const int64_t* scene_offsets, const int64_t* scene_of_chunk,
                          const int64_t* center_ind, const int64_t* base_point_ind, int64_t Ntot, int64_t S, int64_t B, int64_t T,
                          int64_t nbp, int64_t nb_pts, double size_x, double size_y, double margin_x, double margin_y,
                          double chunk_thresh, int bounds_f64, uint64_t seed, const int64_t* seed_device, int64_t* choice,
                          float* out_points, int64_t* out_label, float* chunk_box, int32_t* try_index, int32_t* num_members,
                          uint32_t* base_bits, void* workspace, int64_t workspace_bytes, mvp_stream_t stream);

/* ---- 3D-baseline batches (NEW on the device; the reference crops, pads and rotates in a data-loader worker) ----
 * mvp_sample_scenes_f32: `CropPad(nb_pts)` (mvpnet/data/transforms.py:112-133) of B whole resident scenes, what ScanNet3DScene feeds
 * (mvpnet/data/scannet_3d.py:206-221; configs/scannet/3d_baselines/pn2ssg_scene.yaml crops to 32768), without a host synchronisation
 * and without an allocation (graph-capturable on one stream).
 *   scene_offsets (S+1,) int64; scene_of_row (B,) int64 (a scene may occur more than once); seed / seed_device exactly as in
 *   mvp_sample_chunks_f32.  All on the device; out-of-range scene numbers and offsets are clamped into the arrays (a wrong result,
 *   never a stray access).
 * The draw is mvp_sample_chunks_f32's resampling rule with EVERY point of the scene a member: h = lowbias32, seed32 = low ^ high word of
 * the seed, s_b = h(seed32 + 0x9E3779B9 * (b+1)), n = the scene's point count;
 *   pad (n < nb_pts):   choice[b,s] = s for s < n, ((uint64)h(s ^ s_b ^ 0x85EBCA6B) * n) >> 32 for s >= n;
 *   crop (n >= nb_pts): point j has key h(j ^ s_b) (distinct keys), choice[b,s] = the point with the s-th smallest key.
 *   At nb_pts <= MVP_SAMPLE_MAX_PTS this is, bit for bit, the choice of mvp_sample_chunks_f32's whole-scene fallback for the same seed.
 * Outputs: choice (B,nb_pts) int64 indices inside the scene; num_points (B,) int32 = n.  A scene without points: choice = 0, n = 0.
 * Every result is a function of the arguments alone (integer counts, distinct keys): bit-reproducible.
 * Limits: nb_pts <= MVP_SAMPLE_SCENE_MAX_PTS (what the sampler's multi-workgroup FPS serves), Ntot < 2^31, B <= MVP_SAMPLE_MAX_CHUNKS:
 *   MVP_EUNSUPPORTED beyond, nothing is launched.  MVP_EINVAL unless Ntot, S, nb_pts >= 1, B >= 0, workspace 16-byte aligned with
 *   workspace_bytes >= mvp_sample_scenes_workspace(Ntot, B, nb_pts) (0 for shapes the call refuses).  The scratch is reusable once the
 *   launches have run (stream order). */
#define MVP_SAMPLE_SCENE_MAX_PTS 65536
int64_t mvp_sample_scenes_workspace(int64_t Ntot, int64_t B, int64_t nb_pts);
int mvp_sample_scenes_f32(const int64_t* scene_offsets, const int64_t* scene_of_row, int64_t Ntot, int64_t S, int64_t B, int64_t nb_pts,
                          uint64_t seed, const int64_t* seed_device, int64_t* choice, int32_t* num_points, void* workspace,
                          int64_t workspace_bytes, mvp_stream_t stream);

/* mvp_gather_cloud_f32: a `choice` of either sampler as the 3D baselines' network inputs, one launch.
 *   points (Ntot,3) float32; seg_label (Ntot,) int64 or NULL; colors (Ntot,3) uint8 or NULL; scene_offsets (S+1,), scene_of_row (B,),
 *   choice (B,nb_pts) int64; rot (B,3,3) float32 or NULL.  Slot s of row b reads store row j = scene_offsets[scene] + choice[b,s], the
 *   scene's slice cut to [0, Ntot] and choice clamped into the scene (64-bit addressing: 3 * Ntot may exceed 2^31).
 *   out_points[b,a,s]  = (R[a,0]*x + R[a,1]*y) + R[a,2]*z in float32, each operation rounded once, never contracted -- `points @ R.T` of
 *                        transforms.py:78-85 with R = rot[b]; rot NULL: an exact copy of the bits (-0.0, NaN);
 *   out_label[b,s]     = seg_label[j];
 *   out_feature[b,c,s] = (float)colors[j,c] / 255.0f, an IEEE division: `colors.astype(np.float32) / 255.` (scannet_3d.py:82, :185).
 *   (B,3,nb_pts), (B,nb_pts), (B,3,nb_pts), channel-major as PN2SSG reads them; an absent input's output is not written (may be NULL).
 *   A row whose scene has no points: zeros, label -100.
 * MVP_EINVAL unless Ntot, S, nb_pts >= 1, B >= 0; MVP_EUNSUPPORTED for nb_pts >= 2^31 or B > MVP_SAMPLE_MAX_CHUNKS. */
int mvp_gather_cloud_f32(const float* points, const int64_t* seg_label, const uint8_t* colors, const int64_t* scene_offsets,
                         const int64_t* scene_of_row, const int64_t* choice, const float* rot, int64_t Ntot, int64_t S, int64_t B,
                         int64_t nb_pts, float* out_points, int64_t* out_label, float* out_feature, mvp_stream_t stream);

/* ---- ragged scenes: the whole-scene chunker and the packing of its chunks (NEW on the device) ----
 * scene2chunks_legacy (mvpnet/utils/chunk_util.py:4-53) for all sliding windows of a scene, as index lists in CSR form instead of
 * (windows x points) membership matrices.  points (n,3) float32; corners (nc,2) float32: the windows' lower xy corners, computed by the
 * caller from the scene's extent (float32: `coord_min + float32(i * stride)`); size, margin: the Python floats, as doubles.
 * The rule, pinned (the arithmetic of the reference under NumPy 2: float32 + Python float stays float32, corner + ndarray(float64) is
 * float64), per axis a in {x, y}, nothing contracted:
 *   inner: p.a >= lo.a in float32  &&  (double)p.a <= (double)lo.a + size.a
 *   outer: (double)p.a >= (double)lo.a - margin.a  &&  (double)p.a <= ((double)lo.a + size.a) + margin.a
 *   a NaN coordinate is never a member (every comparison is false); z takes no part.
 * mvp_scene_chunks_count_f32: inner_count[w], outer_count[w] (nc,) int32 for every window, one pass.  The caller reads them back --
 *   batch shapes are host values --, keeps the windows with inner_count >= thresh (chunk_util.py:33-36) and forms
 *   kept (C,) int32 window ids, ascending, and offsets (C+1,) int64, the exclusive sums of their outer counts, both on the device.
 * mvp_scene_chunks_fill_f32: for kept window c
 *   index[offsets[c] .. offsets[c+1]) = its members by the outer test, in ASCENDING point index (int64; `total` = elements of index);
 *   zbox[c] = (min z, max z) over them, float32, NaN-propagating like torch.amin / amax; (+inf, -inf) for an empty list;
 *   base_bits (C,ceil(nb/32)) uint32 when nb > 0: bit j % 32 of word j / 32 = base point base_point_ind[j] ((nb,) int64) is a member
 *   (the rows mvp_select_frames_u32 reads; padding bits zero).  base_point_ind NULL with nb = 0.
 * Index arrays' contents are the caller's: kept and base_point_ind values are clamped into their ranges, a slice of offsets is cut to
 * [0, total] and a list longer than its slice loses its tail (a wrong result, never a stray access).
 * Limits: n < 2^31, nc and C <= MVP_CHUNKER_MAX_WINDOWS, nb <= MVP_OVERLAP_MAX_BASE: MVP_EUNSUPPORTED beyond, nothing is launched.
 * MVP_EINVAL unless n, nc >= 1, C, nb, total >= 0 and no NaN among size / margin.  Integer counts and ordered lists: bit-reproducible. */
#define MVP_CHUNKER_MAX_WINDOWS 65535
int mvp_scene_chunks_count_f32(const float* points, int64_t n, const float* corners, int64_t nc, double size_x, double size_y,
                               double margin_x, double margin_y, int32_t* inner_count, int32_t* outer_count, mvp_stream_t stream);
int mvp_scene_chunks_fill_f32(const float* points, int64_t n, const float* corners, int64_t nc, double size_x, double size_y,
                              double margin_x, double margin_y, const int32_t* kept, const int64_t* offsets, int64_t C,
                              const int64_t* base_point_ind, int64_t nb, int64_t* index, int64_t total, float* zbox, uint32_t* base_bits,
                              mvp_stream_t stream);

/* All chunks of a scene written as padded coordinate rows in one launch: chunk c, with n_c = offsets[c+1] - offsets[c] members
 * index[offsets[c] ..), becomes the (3, N_c) float32 matrix at out + out_base[c], N_c = out_len[c] (offsets (C+1,), out_base, out_len
 * (C,) int64 on the device; out_base in floats) -- chunks of one N_c laid one after the other are a (B,3,N_c) batch.
 *   slot s < n_c  takes points[index[offsets[c] + s]];
 *   slot s >= n_c takes member ((uint64)h(s ^ s_c ^ 0x85EBCA6B) * n_c) >> 32, s_c = h(seed32 + 0x9E3779B9 * (c+1)), h = lowbias32 and
 *   seed32 = low ^ high word of the seed: the pad rule of mvp_sample_chunks_f32 -- uniform duplicates of the chunk's own points BEHIND the
 *   originals, the law of mvpnet/test_mvpnet_3d.py:146-154, not its draws.
 * host_lengths, host_out_len (C,) int64 ON THE HOST: n_c and N_c once more (the launch shape needs the widest chunk; the caller holds
 * both): MVP_EINVAL unless N_c >= n_c >= 1 for every chunk.  The device arrays' contents are the caller's: point indices are clamped
 * into [0, n), a chunk whose rows would leave [out, out + out_floats) or whose slice of index is empty is not written at all.
 * n < 2^31, C <= MVP_CHUNKER_MAX_WINDOWS, N_c < 2^31: MVP_EUNSUPPORTED beyond. */
int mvp_pack_chunks_f32(const float* points, int64_t n, const int64_t* index, int64_t total, const int64_t* offsets, int64_t C,
                        const int64_t* out_base, const int64_t* out_len, const int64_t* host_lengths, const int64_t* host_out_len,
                        uint64_t seed, float* out, int64_t out_floats, mvp_stream_t stream);

/* mvp_pack_chunks_f32 with a per-point feature beside the coordinates and the chunks placed in SLOTS: the batches of the 3D baselines'
 * sliding-window test (mvpnet/test_3d_chunks.py:106-167), one launch for a whole scene.  Chunk c's N_c = out_len[c] slots start at slot
 * slot_base[c] ((C,) int64 on the device): its points are the (3,N_c) matrix at out_points + 3*slot_base[c], its features the (Cf,N_c)
 * matrix at out_feature + Cf*slot_base[c] -- chunks of one N_c in consecutive slots are a (B,3,N_c) and a (B,Cf,N_c) batch, as PN2SSG
 * reads them.  The member of a slot is mvp_pack_chunks_f32's, computed ONCE per slot: a duplicate carries its source point's feature,
 * and out_points is bit-identical to what mvp_pack_chunks_f32 writes with out_base = 3*slot_base.  The feature source is one of
 *   colors (n,3) uint8: out = (float)c / 255.0f, an IEEE division (mvp_gather_cloud_f32's expression, scannet_3d.py:82), Cf must be 3;
 *   feature (n,Cf) float32, 1 <= Cf <= MVP_PACK_CLOUD_MAX_CHANNELS: copied bit for bit;
 *   neither (both NULL): only the points are written, Cf is not looked at and out_feature may be NULL.
 * out_slots: the slots the buffers hold (3*out_slots and Cf*out_slots floats); a chunk whose slots would leave them, or whose slice of
 * index is empty, is not written at all; point indices are clamped into [0, n).  host_lengths, host_out_len, seed: as
 * mvp_pack_chunks_f32.  MVP_EINVAL unless n, total >= 1, C, out_slots >= 0, N_c >= n_c >= 1, at most one feature source and a Cf that
 * fits it; MVP_EUNSUPPORTED for n >= 2^31, C > MVP_CHUNKER_MAX_WINDOWS, N_c >= 2^31 or Cf > MVP_PACK_CLOUD_MAX_CHANNELS. */
#define MVP_PACK_CLOUD_MAX_CHANNELS 8
int mvp_pack_cloud_f32(const float* points, const uint8_t* colors, const float* feature, int64_t Cf, int64_t n, const int64_t* index,
                       int64_t total, const int64_t* offsets, int64_t C, const int64_t* slot_base, const int64_t* out_len,
                       const int64_t* host_lengths, const int64_t* host_out_len, uint64_t seed, float* out_points, float* out_feature,
                       int64_t out_slots, mvp_stream_t stream);

/* ---- frames (NEW on the device; the reference prepares every frame in a data-loader worker) ----
 * The picked frames of a raw uint8 store as the 2D network reads them: T.ColorJitter(brightness, contrast, saturation) on the PIL
 * image, `/ 255.`, `(image - mean) / std`, np.fliplr (mvpnet/data/scannet_2d3d.py:241-252, :293-296; mvpnet/data/scannet_2d.py:158-171).
 *   frames (Ftot,H,W,3) uint8 RGB as a PNG decodes; picked (Nf,) int64 global rows, clamped to [0, Ftot) (the contents of an index
 *   array are the caller's: a wrong frame, never a stray read); factor (Nf,3) float32 = (brightness, contrast, saturation) and order
 *   (Nf,3) uint8, both or neither (NULL: no jitter); flip (Nf,) uint8 or NULL; mean_std: 6 float32 ON THE DEVICE (mean rgb, std rgb)
 *   or NULL; -> out (Nf,3,H,W) float32, or (Nf,H,W,3) when channels_last != 0.
 * Pinned definition -- for given factors and order bit-identical to PIL's ImageEnhance.{Brightness,Contrast,Color}(img).enhance(f)
 * chain (what torchvision's PIL path calls); every step maps uint8 RGB to uint8 RGB:
 *   gray(r,g,b) = (r*19595 + g*38470 + b*7471 + 0x8000) >> 16                                  (PIL's convert('L'))
 *   blend(d,p,f): t = fl32(fl32(d) + fl32(f * fl32(p - d))), p - d the integer difference, nothing contracted;
 *                 0 if t <= 0, 255 if t >= 255, else (uint8)(int)t  (for 0 <= f <= 1, where PIL does not clip, t lies in [0, 255])
 *   brightness: channel = blend(0, channel, f);  saturation: blend(gray(pixel), channel, f);  contrast: blend(m, channel, f) with
 *   m = (2*S + n) / (2*n) in integers, S = the sum of gray over the n = H*W pixels of the image AS IT ENTERS this step
 *   (PIL: int(S / n + 0.5) in double -- the same number for every size this entry takes).
 *   order[i] = the op applied i-th: 0 brightness, 1 contrast, 2 saturation, any other value = no step; a second contrast code is
 *   skipped too (one mean per frame).  A factor of exactly 1 leaves the image unchanged (t = p).
 *   value: v = fl32(fl32(u) / 255.f); with mean_std fl32(fl32(v - mean[c]) / std[c]) -- IEEE float32 divisions, NumPy's arithmetic.
 *   flip[i] != 0: output column x holds input column W-1-x, after everything else (the contrast mean does not depend on it).
 * Any alignment is accepted: with W % 4 == 0, frames 4-byte and out 16-byte aligned a lane handles four pixels with wide loads and
 * stores, otherwise one pixel; the results are the same.
 * Two launches behind one hipMemsetAsync of the workspace (the frames' grey sums, integer atomics: bit-reproducible), one launch without
 * a jitter; no allocation, no synchronisation (graph-capturable).  workspace: mvp_prepare_frames_workspace(Nf) bytes, 8-byte aligned;
 * needed with a jitter only.  Frame bases are 64-bit (a store may exceed 4 GiB), offsets inside a frame 32-bit.
 * MVP_EINVAL for Ftot, H, W or Nf < 1 or exactly one of factor / order NULL; MVP_EUNSUPPORTED for H*W*3 >= 2^31. */
size_t mvp_prepare_frames_workspace(int64_t Nf);
int mvp_prepare_frames_u8(const uint8_t* frames, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, const float* factor,
                          const uint8_t* order, const uint8_t* flip, const float* mean_std, int channels_last, float* out, void* workspace,
                          mvp_stream_t stream);

/* ---- resize and label maps (NEW on the device; the reference calls Pillow per frame in a data-loader worker) ----
 * `image.resize(size, Image.BILINEAR)` on uint8 RGB and `label.resize(size, Image.NEAREST)` on a 16-bit label image
 * (mvpnet/data/scannet_2d.py:153-156, mvpnet/data/scannet_2d3d.py:234-239), bit-identical to Pillow.
 *
 * Host tables, in double, no GPU (Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter), one axis inS -> outS:
 *   scale = inS / outS, fs = max(scale, 1), support = fs, ksize = ceil(support) * 2 + 1; per output xx: center = (xx + 0.5) * scale,
 *   xmin = max((int)(center - support + 0.5), 0), count = min((int)(center + support + 0.5), inS) - xmin; weights
 *   max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|) for x < count, summed in index order and divided by the sum; integer weights
 *   (int)(w * 2^22 + 0.5) for w >= 0, (int)(w * 2^22 - 0.5) below; entries behind count are 0.
 * mvp_resize_bilinear_table writes xmin (outS), count (outS), coef (outS * ksize) and *ksize; with the three arrays NULL only *ksize.
 * mvp_resize_nearest_table writes index[x] = min((int)(scale * (x + 0.5)), inS - 1): the rule Pillow applies to 16-bit ("I;16")
 * images, which is what ScanNet's label PNGs are (its 8-bit and float modes accumulate the coordinate instead; not reproduced: the
 * reference never resizes such an image with NEAREST).  MVP_EINVAL unless inS, outS >= 1; MVP_EUNSUPPORTED for sizes of 2^31 and more. */
int mvp_resize_bilinear_table(int64_t inS, int64_t outS, int32_t* xmin, int32_t* count, int32_t* coef, int32_t* ksize);
int mvp_resize_nearest_table(int64_t inS, int64_t outS, int32_t* index);

/* frames (Ftot,H,W,3) uint8; picked (Nf,) int64 global rows, clamped to [0, Ftot) -> out (Nf,h,w,3) uint8: the picked frames resized.
 * xtab / ytab ON THE DEVICE: an axis' table as int32 [xmin (outS) | count (outS) | coef (outS * ksize)], W -> w and H -> h; NULL exactly
 * when that axis keeps its size.  Pillow's two passes in Pillow's order, each clip8((2^21 + sum pixel * coef) >> 22) in 32-bit integers
 * (255 * 2^22 < 2^31), no floating point: horizontal first, ITS RESULT ROUNDED TO uint8, then vertical.  One launch (per 65535 frames):
 * a workgroup owns a tile of 8 x 32 output pixels and keeps the intermediate rows its tile draws on in LDS (18 KiB); with one table
 * NULL only the other pass runs, with both NULL the frames are copied.  A table's contents are the caller's: windows are clamped into
 * the image, a wrong table gives wrong pixels and no stray read.
 * Accepted sizes: at most 64 taps per changed axis (inS / outS <= 31) and, when both axes change, a tile's
 * ceil(7 * H/h + 2 * max(H/h, 1)) + 2 input rows <= 192 (H / h up to ~21): 1296x968 -> 160x120 (ksize 19 on both axes, 75 rows), 640x480 ->
 * 160x120 (ksize 9, 38 rows) and every enlargement fit.  MVP_EUNSUPPORTED beyond, and for an image of 2^31 bytes or more; MVP_EINVAL for a
 * size < 1, Nf < 1 or a table that is NULL for a changed axis / given for an unchanged one.  Nothing is launched on an error. */
int mvp_resize_frames_u8(const uint8_t* frames, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, int64_t h, int64_t w,
                         const int32_t* xtab, const int32_t* ytab, uint8_t* out, mvp_stream_t stream);

/* labels (Ftot,H,W) uint16 raw ids as a label PNG decodes; picked (Nf,) as above -> out (Nf,h,w) int64, one launch:
 *   raw = labels[picked[f], yi[y], xi[flip[f] ? w - 1 - x : x]];  out = mapping ? (raw < T ? mapping[raw] : ignore_value) : raw
 * (`label.resize(size, Image.NEAREST)`, F.hflip, `label_mapping[label]`: scannet_2d.py:156, :163, :167-168; a raw id beyond the table
 * raises there, here it is ignored).  yi (h) / xi (w) int32 ON THE DEVICE (mvp_resize_nearest_table), clamped into the image; NULL =
 * identity, for h == H / w == W only.  flip (Nf,) uint8 or NULL; mapping (T,) int64 on the device or NULL.
 * MVP_EINVAL for a size < 1, Nf < 1, a NULL table for a changed axis or T < 0; MVP_EUNSUPPORTED for H*W or h*w >= 2^31. */
int mvp_prepare_labels_u16(const uint16_t* labels, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, int64_t h, int64_t w,
                           const int32_t* yi, const int32_t* xi, const uint8_t* flip, const int64_t* mapping, int64_t T, int64_t ignore_value,
                           int64_t* out, mvp_stream_t stream);

/* Column slices of several row-major float matrices in one launch (host-side helper of the shared-MLP path: the reference slices
 * nothing -- it concatenates the inputs instead, modules.py:32-35,178-186 -- the linear-first factorisation of those layers needs
 * each column group of the weight as its own aligned operand).  table: n x 6 int64 ON THE DEVICE, per entry
 * {src pointer, dst pointer, src row stride, dst row stride, rows, cols} in floats; dst[r*ldd + c] = src[r*lds + c], c < cols. */
int mvp_copy_slices_f32(const int64_t* table, int64_t n, mvp_stream_t stream);

/* ---- channels-last ("rows") PointNet++ kernels ---------------------------------------------
 * Same mathematics as the channel-major ops above with a point's C features stored as one
 * contiguous row; these are what the model pipeline runs (mvpnet_amd/pn2.py).  All C, ld % 4 == 0.
 * group_rows: replaces QueryGrouper.forward's two group_points + centre subtraction + cat
 *   (mvpnet/models/pn2/modules.py:20-37): feature (B,N,C) [C may be 0], xyz (B,N,3) and center (B,M,3)
 *   or both NULL, index (B,M,K) -> out (B,M,K,ld) = [feature row | xyz - center | zero pad].
 * group_rows_backward: grad_out (B,M,K,ld) -> grad_feature (B,N,C) (zero-filled here; first C columns).
 * interp_rows(_backward): feature_interpolate (mvpnet/ops/interpolate.py:5-34) on rows;
 *   feature (B,N1,C), index/weight (B,N2,3) -> out (B,N2,ld) columns [0,C). */
int mvp_group_rows_f32(const float* feature, const float* xyz, const float* center, const int64_t* index, int64_t B,
                       int64_t N, int64_t C, int64_t M, int64_t K, int64_t ld, float* out, mvp_stream_t stream);
int mvp_group_rows_backward_f32(const float* grad_out, const int64_t* index, int64_t B, int64_t N, int64_t C, int64_t M,
                                int64_t K, int64_t ld, float* grad_feature, mvp_stream_t stream);
/* FeatureAggregation input (mvpnet/models/mvpnet_3d.py:55-56: cat[feature, src - tgt, |src - tgt|^2]) on rows:
 * feature (R*K, C) gathered rows, src_xyz (R*K, 3), tgt_xyz (R, 3) -> out (R*K, C+4), C % 4 == 0, in one pass. */
int mvp_relation_rows_f32(const float* feature, const float* src_xyz, const float* tgt_xyz, int64_t R, int64_t K, int64_t C,
                          float* out, mvp_stream_t stream);
/* Set-abstraction grouping AFTER the feature part of the (linear) first shared-MLP layer (modules.py:20-37,107):
 *   out (B,M,K,C) = zf (B,N,C)[index] + wxyz (C,3) . (xyz (B,N,3)[index] - centre (B,M,3))
 * with zf = W1[:, :C_in] . feature evaluated once per point (8x fewer conv rows than grouping first) and the coordinate
 * columns evaluated on the difference, as the reference does.  zf may be NULL (no input feature).  diff, if not NULL,
 * receives the (B,M,K,4) rows [dx,dy,dz,0] (operand of the W1_xyz weight gradient).  stat, if not NULL (2*C float64,
 * accumulated into): column sums of out and out^2 -- the layer's batch statistics without another pass; it needs the
 * scratch `partial` of mvp_group_lin_partial_count(B,C,M,K) float64. */
int64_t mvp_group_lin_partial_count(int64_t B, int64_t C, int64_t M, int64_t K);
int mvp_group_lin_rows_f32(const float* zf, const float* xyz, const float* centre, const float* wxyz, const int64_t* index,
                           int64_t B, int64_t N, int64_t C, int64_t M, int64_t K, float* out, float* diff, double* stat,
                           double* partial, mvp_stream_t stream);
/* The same with the BatchNorm finalize of the layer (batch statistics over the B*M*K rows: mean, invstd (C floats out), running
 * statistics and num_batches_tracked updated when not NULL -- the arithmetic of mvp_bn_finalize_f32) carried by the last workgroup
 * of the statistics reduction: no finalize launch behind it.  stat: 2*C + 1 float64, ZERO on entry (sums + completion counter). */
int mvp_group_lin_rows_bn_f32(const float* zf, const float* xyz, const float* centre, const float* wxyz, const int64_t* index, int64_t B,
                              int64_t N, int64_t C, int64_t M, int64_t K, float* out, float* diff, double* stat, double* partial, float eps,
                              float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                              int64_t* num_batches_tracked, mvp_stream_t stream);
/* stat (2*C float64) += column sums of y and y^2 over the R rows of y (R,C); accumulated: the caller provides zeros */
int mvp_colstats_f32(const float* y, int64_t R, int64_t C, double* stat, double* partial, mvp_stream_t stream);
/* `partial` of mvp_colstats_f32 / mvp_bn_rows_forward_f32 / mvp_bn_rows_backward_f32: optional scratch of
 * mvp_colstats_partial_count(G*K rows, C) float64.  With it the column sums are reduced through per-workgroup slots by up to 1024
 * workgroups; without it (NULL) by at most 256 workgroups with fp64 atomics, which queue per result address. */
int64_t mvp_colstats_partial_count(int64_t R, int64_t C);
int mvp_interp_rows_f32(const float* feature, const int64_t* index, const float* weight, int64_t B, int64_t N1, int64_t C,
                        int64_t N2, int64_t ld, float* out, mvp_stream_t stream);
/* Transposed index of a gather out[b,e] = f[b, index[b,e]] (index (B,E) int64, values outside [0,N) are ignored):
 *   offsets (B,N+1) int32, slots (B,E) int32: the positions e that read point j are slots[b][offsets[b][j] .. offsets[b][j+1]).
 * cursor: (B,N) int32 scratch.  With it the scatter-add backward of group_points / feature_interpolate
 * (group_points_kernel.cu:50-89, interpolate_kernel.cu:131-174: one atomicAdd per element) is a gather:
 *   grad_feature (B,N,C) = sum over the slots p of point j of weight[b,p] * grad_out[b, slot / S, :]
 * (weight NULL = 1; S = slots per grad_out row: 1 for the grouping with E = M*K rows, 3 for the 3-NN interpolation with E = 3*N2).
 * No atomics on the data, no zero fill.  While a chunk's N counters fit in LDS (N <= ~37 000) the build is one launch, one workgroup per
 * chunk; beyond that (whole-scene vote plans) three launches with global atomics.  The entries of a list are in arrival order (differs
 * from run to run).  mvp_csr_build_sorted_i64: on the one-launch path every list of up to 1024 slots is also sorted ascending, so the
 * gather backward adds in the same order in every run -- the reproducible training mode's build (the sort is 40-55 % of the kernel). */
int mvp_csr_build_i64(const int64_t* index, int64_t B, int64_t E, int64_t N, int32_t* offsets, int32_t* slots, int32_t* cursor,
                      mvp_stream_t stream);
int mvp_csr_build_sorted_i64(const int64_t* index, int64_t B, int64_t E, int64_t N, int32_t* offsets, int32_t* slots, int32_t* cursor,
                             mvp_stream_t stream);
int mvp_gather_rows_backward_csr_f32(const float* grad_out, const int32_t* offsets, const int32_t* slots, const float* weight,
                                     int64_t B, int64_t N, int64_t C, int64_t E, int64_t S, int64_t ld, float* grad_feature,
                                     mvp_stream_t stream);
/* The same gather with the BatchNorm-backward finish of the gathered tensor's layer applied on load (round 5): dz / y (B * E / S, ld), stat (2 C)
 * = column sums of dz and dz * xhat over all rows; gathered rows = gamma*invstd * (dz - stat[c]/R - xhat * stat[C+c]/R).  Replaces
 * mvp_bn_rows_backward_finish_f32 + mvp_gather_rows_backward_csr_f32 where the finished gradient has no other consumer (FeaturePropagation
 * without a skip feature, mvpnet/models/pn2/modules.py:178-186, pn2ssg.py:101-112: the last propagation level). */
int mvp_gather_rows_backward_csr_finish_f32(const float* dz, const float* y, const float* mean, const float* invstd, const float* gamma,
                                            const double* stat, int training, const int32_t* offsets, const int32_t* slots, const float* weight,
                                            int64_t B, int64_t N, int64_t C, int64_t E, int64_t S, int64_t ld, float* grad_feature,
                                            mvp_stream_t stream);
/* out (B,N2,C) = 3-point interpolation of feature (B,N1,C) (+ add (B,N2,C) if not NULL): feature propagation with the (linear)
 * first shared-MLP layer applied before the interpolation (pn2/modules.py:135-145,178-186):
 *   W.[interp(f_sparse) | skip] = interp(Wa.f_sparse) + Wb.skip.
 * stat (2*C float64, accumulated into) / partial (mvp_group_lin_partial_count(B,C,N2,1) float64) as in mvp_group_lin_rows_f32. */
int mvp_interp_add_rows_f32(const float* feature, const int64_t* index, const float* weight, const float* add, int64_t B, int64_t N1,
                            int64_t C, int64_t N2, float* out, double* stat, double* partial, mvp_stream_t stream);
/* ... with the BatchNorm finalize over the B*N2 rows carried by the reduction, as mvp_group_lin_rows_bn_f32 (stat: 2*C + 1, zero). */
int mvp_interp_add_rows_bn_f32(const float* feature, const int64_t* index, const float* weight, const float* add, int64_t B, int64_t N1,
                               int64_t C, int64_t N2, float* out, double* stat, double* partial, float eps, float momentum, float* mean,
                               float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, mvp_stream_t stream);
int mvp_interp_rows_backward_f32(const float* grad_out, const int64_t* index, const float* weight, int64_t B, int64_t N1,
                                 int64_t C, int64_t N2, int64_t ld, float* grad_feature, mvp_stream_t stream);
/* BatchNorm (+ReLU) (+max over K consecutive rows) on a row matrix y (G*K, C): replaces the BN / ReLU /
 * torch.max(dim=3) modules after each 1x1 conv (common/nn/modules/conv.py:41-51, pn2/modules.py:107-108).
 * forward : training != 0: batch statistics (float64 accumulation) -> mean, invstd (outputs), running_* updated
 *           (momentum, unbiased variance; may be NULL); training == 0: mean / invstd are INPUTS.
 *           out (G,C) = max_k act(((y-mean)*invstd)*gamma+beta), arg (G,C) uint8 = first arg-max (K > 1 only);
 *           K > 1 with arg == NULL: out = SUM over k instead (FeatureAggregation reduction='sum', mvpnet_3d.py:40-41,59),
 *           backward likewise (out is then unused).
 *           stat: 2*C float64 scratch.
 * backward: dsrc = d out (G,C) [K > 1] or d act (G*K,C) [K == 1] -> dy (G*K,C); on return
 *           stat[0:C] = d beta, stat[C:2C] = d gamma (float64), also written as float32 to dgamma / dbeta when those
 *           are not NULL.  training == 0: statistics were constants (eval mode), the batch terms are dropped. */
int mvp_bn_rows_forward_f32(const float* y, const float* gamma, const float* beta, int64_t G, int64_t K, int64_t C,
                            int training, float eps, float momentum, int relu, float* running_mean, float* running_var,
                            double* stat, float* mean, float* invstd, float* out, uint8_t* arg, double* partial,
                            mvp_stream_t stream);
int mvp_bn_rows_backward_f32(const float* dsrc, const float* out, const uint8_t* arg, const float* y, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, int64_t G, int64_t K, int64_t C,
                             int relu, int training, double* stat, float* dy, float* dgamma, float* dbeta, double* partial,
                             mvp_stream_t stream);
/* The K = 1 forms with DROPOUT behind the activation (SharedMLPDO: Conv + BN + ReLU + Dropout, common/nn/modules/mlp.py:86-92; the
 * reference runs nn.Dropout as its own pass and keeps the mask): out = act(bn(y)) * keep / (1 - drop_p) with keep a counter-based hash of
 * (seed, row * C + column) that forward and backward regenerate -- no mask tensor.  0 <= drop_p < 1, R * C < 2^32.  Independent
 * Bernoulli(1 - drop_p) per element like torch's, not the same random stream.
 * mvp_bn_rows_backward[_dropout]_f32 with dy == NULL (K = 1, or K > 1 with arg == NULL: the backward of the SUM over K): only `stat` (the two
 * BatchNorm-backward column sums) is produced -- the caller forms dy itself (mvp_mlp_layer_backward_wide[_pooled]_p_f32, mode 2). */
int mvp_bn_rows_forward_dropout_f32(const float* y, const float* gamma, const float* beta, int64_t R, int64_t C, int training, float eps,
                                    float momentum, int relu, float* running_mean, float* running_var, double* stat, float* mean,
                                    float* invstd, float* out, double* partial, float drop_p, uint64_t seed, mvp_stream_t stream);
int mvp_bn_rows_backward_dropout_f32(const float* dsrc, const float* y, const float* mean, const float* invstd, const float* gamma,
                                     const float* beta, int64_t R, int64_t C, int relu, int training, double* stat, float* dy,
                                     float* dgamma, float* dbeta, double* partial, float drop_p, uint64_t seed, mvp_stream_t stream);
/* second half of the BatchNorm backward with known column sums stat = [sum dz | sum dz*xhat] (from mvp_mlp_input_grad_f32) */
int mvp_bn_rows_backward_finish_f32(const float* dz, const float* y, const float* mean, const float* invstd,
                                    const float* gamma, const float* beta, int64_t R, int64_t C, int training,
                                    const double* stat, float* dy, float* dgamma, float* dbeta, mvp_stream_t stream);
/* mean / invstd (+ running statistics update and num_batches_tracked += 1, each may be NULL) from column sums
 * stat = [sum y | sum y^2] over R rows */
int mvp_bn_finalize_f32(const double* stat, int64_t R, int64_t C, float eps, float momentum, float* mean, float* invstd,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, mvp_stream_t stream);
/* ---- fused set-abstraction level, inference (csrc/sa_fused.hip) --------------------------------------------------------------
 * gather of the ball's K = 32 neighbours -> first layer (zf = its feature columns applied per point, + coordinate columns on the
 * centred xyz) -> BN + ReLU -> layer 2 -> BN + ReLU -> layer 3 -> BN + ReLU -> max over the neighbours, in ONE kernel: nothing between
 * the gathered rows and the (B,M,C3) output touches HBM (reference: QueryGrouper + SharedMLP(ndim=2) + torch.max,
 * mvpnet/models/pn2/modules.py:20-37,100-108).  One wave per ball, activations between layers staged through a wave-private LDS tile,
 * both weight matrices resident in LDS, split-bf16 MFMA.
 *   zf (B,N,C1) or NULL, xyz (B,N,3), centre (B,M,3), index (B,M,32) int64 (-1 = empty slot), wxyz (C1,3);
 *   bnL_* = mean, invstd (= 1/sqrt(running_var + eps)), gamma, beta of layer L; W2 (C2,C1), W3 (C3,C2) row-major;
 *   out (B,M,C3), arg (B,M,C3) uint8 or NULL (first neighbour attaining the maximum).
 * MVP_EUNSUPPORTED unless K == 32, C1, C2 <= 64, C3 <= 128, all % 4 == 0 and a split-bf16 precision is set, and beyond the limits of the
 * kernel's 32-bit ball and row-offset arithmetic: N, M <= INT_MAX, B * M <= 2^31 - 16, N * max(C1, 3) < 2^32. */
int mvp_sa_fused_forward_f32(const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz, int64_t B,
                             int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd,
                             const float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean,
                             const float* bn2_invstd, const float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3,
                             const float* bn3_mean, const float* bn3_invstd, const float* bn3_gamma, const float* bn3_beta, float* out,
                             uint8_t* arg, mvp_stream_t stream);

/* Contraction precision of the three shared-MLP entry points below (process-wide):
 *   terms = 0  fp32 MFMA (v_mfma_f32_32x32x2_f32: an exact fp32 FMA chain);
 *   terms = 6  (the default) split-bf16: every fp32 operand as 3 bf16 pieces, the 6 products of order <= 2 on v_mfma_f32_32x32x16_bf16 with fp32
 *              accumulation -- fp32-level accuracy at 2.67x the fp32-MFMA rate;
 *   terms = 3  2 pieces, 3 products: ~2^-17 relative error per product, 5.3x the rate;
 *   terms = 1  plain bf16 operands (each fp32 operand rounded to bf16 ONCE, one product, fp32 accumulation, fp32 storage): ~2^-9 per
 *              product -- the accuracy of a bf16 autocast of the convolution; opt-in, OUTSIDE the fp32 parity bar (BASELINE.json's
 *              configs[2] names bf16; the default stays the fp32-equivalent split).
 * Layers with max(Cin, Cout) < min_width keep the fp32 MFMA.  Returns MVP_EINVAL for other values. */
int mvp_set_mlp_precision(int terms, int min_width);
int mvp_get_mlp_precision(void);
/* min_width of the last mvp_set_mlp_precision (0 until then): what a host that routes layers between entry points has to agree with */
int mvp_get_mlp_min_width(void);
/* Split of the gradient contractions (dW, input gradient, mvp_mlp_layer_backward_f32) while the forward precision is a split one:
 * terms = 3 (default), 6 or 1. */
int mvp_set_mlp_precision_backward(int terms);
int mvp_get_mlp_precision_backward(void);
/* The two settings above are process-wide DEFAULTS.  mvp_mlp_precision_scope overrides them for the calls the CALLING host thread makes
 * (thread-local; terms / terms_backward = -1 keeps the default): nothing global is written, so several models or threads in one process
 * never see each other's choice.  Returns the previous override packed as (terms + 1) * 16 + (terms_backward + 1), MVP_EINVAL for other
 * values.  The getters return what the calling thread's launches use. */
int mvp_mlp_precision_scope(int terms, int terms_backward);
/* One Adam step of n float32 tensors in one launch (adam.hip; replaces, on the GPU, torch.optim.Adam.step of the reference's training loop:
 * common/solver/build.py:7-22, train_mvpnet_3d.py:176).  params / grads / exp_avg / exp_avg_sq: HOST arrays of n device pointers, numel
 * their element counts (< 2^31 each); torch.optim.Adam semantics (L2 weight decay added to the gradient, no amsgrad, minimising):
 *   g' = g + weight_decay p;  m += (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;  p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * step >= 1 is the number of THIS update; fp32 arithmetic, the bias corrections in double on the host.  96 tensors per launch. */
int mvp_adam_step_f32(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel,
                      int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay, double step, mvp_stream_t stream);
/* The same step with its step number and learning rate ON THE DEVICE (adam.hip), so that a captured graph which holds these launches
 * takes update t + 1 at the current learning rate on every replay.  None of the three synchronises or allocates; every check below
 * happens before any launch.
 *   mvp_adam_advance_f32: one small launch.  step_counts: n_counts float32 values on the device, the `step` of every parameter of a
 *       group, all equal (the caller's rule); lr: one double on the device; hyper: MVP_SOLVER_HYPER_F32 floats on the device.  Adds 1.0f
 *       to every count, takes t = (int64)step_counts[0] after the add (a float32 count is exact below 2^24 updates) and writes, all in
 *       double, every operation rounded once, nothing contracted, no pow():
 *           pow_int(b, t):  r = 1; x = b; while (t) { if (t & 1) r = r * x; x = x * x; t >>= 1; }
 *           bc1 = 1 - pow_int(beta1, t);  bc2 = 1 - pow_int(beta2, t)
 *           hyper[0] = (float)(lr / bc1);  hyper[1] = (float)sqrt(bc2) (a correctly rounded double sqrt);  hyper[2] = (float)lr;  hyper[3] = 0
 *       -- a function of the count alone, the same bits wherever it is restated (host and device pow() may differ in the last place, so
 *       mvp_adam_step_f32's corrections may differ from these by one place of the two float32 factors).
 *       MVP_ENULL (step_counts, lr, hyper); MVP_EINVAL unless n_counts >= 1 and both betas in [0, 1).
 *   mvp_adam_step_dev_f32: mvp_adam_step_f32's update and launches (96 tensors each, same vector / tail / unaligned paths) with
 *       step_size = hyper[0] and bc2_sqrt = hyper[1] read on the device; 1 - beta in double on the host as there.  grad_scale: NULL or a
 *       DEVICE pointer to one float: g' = g * grad_scale, one rounded product as the gradient is read, before the weight decay -- the
 *       arithmetic of mvp_sgd_step_f32's grad_scale and of mvp_grad_clip_finish_f32's in-place scale; the gradients are not written.
 *       mvp_adam_step_f32's argument checks (no step); hyper NULL with n > 0: MVP_ENULL.
 *   mvp_lr_multistep_f64: torch's MultiStepLR in its chainable form (group['lr'] * gamma ** milestones[last_epoch]) in the same doubles,
 *       one small launch:  e = *epoch + 1;  for i < n_milestones: if (milestones[i] == e) for g < n_groups: lr[g] = lr[g] * factors[i];
 *       *epoch = e.  epoch: one int64 and lr: n_groups doubles on the device; milestones (distinct, strictly ascending) and factors
 *       (gamma ** multiplicity, evaluated by the caller) are HOST arrays that travel by value in the argument block.
 *       MVP_ENULL (epoch, lr; milestones, factors when n_milestones > 0); MVP_EINVAL unless n_groups >= 1, n_milestones >= 0, the
 *       milestones strictly ascending and no factor NaN; MVP_EUNSUPPORTED for n_milestones > MVP_SOLVER_MILESTONE_SLOTS. */
#define MVP_SOLVER_MILESTONE_SLOTS 16
#define MVP_SOLVER_HYPER_F32 4      /* step_size, bc2_sqrt, (float)lr, reserved */
int mvp_adam_advance_f32(float* step_counts, int64_t n_counts, const double* lr, double beta1, double beta2, float* hyper, mvp_stream_t stream);
int mvp_adam_step_dev_f32(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel,
                          int64_t n, const float* hyper, const float* grad_scale, double beta1, double beta2, double eps, double weight_decay,
                          mvp_stream_t stream);
int mvp_lr_multistep_f64(int64_t* epoch, double* lr, int64_t n_groups, const int64_t* milestones, const double* factors, int64_t n_milestones,
                         mvp_stream_t stream);
/* One SGD step of n float32 tensors (solver.hip; replaces, on the GPU, torch.optim.SGD.step of the reference's 2D stage:
 * common/solver/build.py:7-22 with configs/scannet/unet_resnet34.yaml).  params / grads / momentum_buf: HOST arrays of n device pointers,
 * numel their element counts (< 2^31 each), first: a HOST array of n bytes, grad_scale: NULL or a DEVICE pointer to one float (a clip
 * coefficient that never left the device).  torch.optim.SGD semantics per element in fp32:
 *   g' = g * grad_scale (when given: one rounded product);  g' += weight_decay p (when weight_decay != 0);
 *   momentum != 0:  buf = g' where first[i] != 0 (torch's first step: a copy, no dampening; the buffer is not read),
 *                   else buf = (momentum buf) + (1 - dampening) g';   g' = nesterov ? g' + momentum buf : buf;
 *   p = p - lr g'
 * every `x + alpha y` above is one fused multiply-add (4 roundings per element and step, not 6), momentum buf a rounded product.
 * momentum == 0 touches no buffer (momentum_buf and first may be NULL).  Tensors on their first and on later steps share a launch (the
 * bytes of `first` travel as a bit mask); 124 tensors per launch.  MVP_EINVAL, before any launch, for n < 0, momentum < 0, lr < 0 and
 * for nesterov with momentum <= 0 or dampening != 0. */
int mvp_sgd_step_f32(void* const* params, const void* const* grads, void* const* momentum_buf, const int64_t* numel, const uint8_t* first,
                     int64_t n, double lr, double momentum, double dampening, double weight_decay, int nesterov, const float* grad_scale,
                     mvp_stream_t stream);
/* Global 2-norm of n float32 gradient tensors and the clip by it (solver.hip; replaces nn.utils.clip_grad_norm_ of the reference's train
 * loops, train_2d.py:181-185), without atomics and without a host synchronisation; bit-reproducible.
 *   mvp_grad_clip_partials_count: the number of partial sums for these element counts (one per 8192 elements of each tensor, rounded up):
 *       sizes `partials` on the host; negative MVP_E* on bad arguments.
 *   mvp_grad_sqnorm_partials_f32: grads is a HOST array of n device pointers; every workgroup writes the fp32 sum of the squares of its
 *       8192 elements to its own slot of `partials` (device); n_partials_out (host, may be NULL) receives the count.
 *   mvp_grad_clip_finish_f32: EVERY workgroup adds the n_partials partials in the same fixed order (strided over its lanes, then the
 *       workgroup tree: all hold the same bits), then
 *           total = sqrt(sum);  c = max_norm / (total + 1e-6);  coef = c < 1 ? c : (c is NaN ? c : 1)     (torch.clamp(c, max=1))
 *       and multiplies its 8192 elements of grads by coef -- always, as torch does; workgroup 0 writes total and coef to the two device
 *       floats.  grads == NULL: a one-workgroup launch that writes only the scalars (the coefficient is then applied by
 *       mvp_sgd_step_f32's grad_scale).  max_norm < 0: no clipping, coef = 1.  With grads, n_partials must be the count of (numel, n). */
int64_t mvp_grad_clip_partials_count(const int64_t* numel, int64_t n);
int mvp_grad_sqnorm_partials_f32(const void* const* grads, const int64_t* numel, int64_t n, float* partials, int64_t* n_partials_out,
                                 mvp_stream_t stream);
int mvp_grad_clip_finish_f32(void* const* grads, const int64_t* numel, int64_t n, const float* partials, int64_t n_partials, double max_norm,
                             float* total_norm_out, float* coef_out, mvp_stream_t stream);

/* Shared-MLP layer on bfloat16 VALUES (mlp_bf16.hip; SURVEY 8b "+bf16 for gather/interp/MLP values"; uint16_t = bf16 bit patterns):
 *   Y (R, ldy)[:, :Cout] = act((X (R, ldx)[:, :Cin] . bf16_rn(W (Cout, ldw)[:, :Cin])^T + bias) * scale + shift)
 * -- the reference's conv -> BatchNorm -> ReLU layer (common/nn/modules/conv.py:41-51) in inference with the running-statistics
 * BatchNorm folded into scale / shift by the caller; bias, scale, shift (Cout floats) may be NULL, relu != 0 clamps at zero.  Native
 * v_mfma_f32_32x32x16_bf16, fp32 accumulation, every fp32 step rounded once (no fused multiply-add), one rounding to bf16 on the way
 * out.  Not part of the fp32 parity path.  MVP_EUNSUPPORTED unless Cin % 16 == 0, Cout % 8 == 0, ldx % 8 == 0, ldy % 8 == 0 and X, Y
 * are 16-byte aligned. */
int mvp_mlp_forward_bf16(const uint16_t* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
                         const float* bias, const float* scale, const float* shift, int relu, uint16_t* Y, int64_t ldy,
                         mvp_stream_t stream);

/* Switch (returns the previous value): 1 (default since round 3: 12-23 % faster alone at the step's shapes, 0.8 % on the step -- in round 2,
 * beside the atomics-bound side-stream kernels of that time, it measured 1.2 % slower) = long narrow forward layers (>= 32768 rows, C_in,
 * C_out <= 128) run on the persistent streaming kernel with the weight matrix resident in LDS; 0 = the per-tile kernel. */
int mvp_set_mlp_stream(int on);

/* Shared-MLP layer on rows with fp32 MFMA (mlp.hip): Y (R,Cout) = act(X (R,ldx)[:, :Cin]) . W (Cout,ldw)[:, :Cin]^T (+ bias).
 * act = identity when act_mean == NULL, else relu(((x-mean)*invstd)*gamma+beta) per input column: the previous
 * layer's BatchNorm + ReLU fused into the load (common/nn/modules/conv.py:41-51), so that activation is never stored.
 * stat != NULL: 2*Cout float64, the column sums of y and y^2 (this layer's batch statistics) are ADDED to it -- in all
 * three entry points `stat` and `dW` are accumulated into, so the caller provides zeros (one zeroed arena for a whole
 * layer chain instead of a memset per call) or a running sum (gradient accumulation). */
int mvp_mlp_forward_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
                        const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta,
                        const float* bias, float* Y, double* stat, double* partial, mvp_stream_t stream);
/* mvp_mlp_forward_f32 (no bias) + the layer's training-mode BatchNorm finalize (what mvp_bn_finalize_f32 computes from `stat`: mean,
 * invstd with the biased variance; running_mean / running_var with momentum and the unbiased variance, may be NULL;
 * num_batches_tracked += 1, may be NULL) carried by the last workgroup of the statistics reduction: one launch fewer per layer.
 * stat: 2*Cout + 1 float64, ALL zero on entry: [column sums of y | of y^2 | completion counter of this launch (zero again on exit)]. */
int mvp_mlp_forward_bn_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
                           const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, float* Y,
                           double* stat, double* partial, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                           float* running_var, int64_t* num_batches_tracked, mvp_stream_t stream);
/* A layer whose input is [X | rel] WITHOUT the concatenated tensor: Y = X (R,ldx)[:, :Cin] . W (Cout,ldw)[:, :Cin]^T + rel (R,4) . wrel (Cout,4)^T.
 * Replaces the cat + first conv of FeatureAggregation (mvpnet/models/mvpnet_3d.py:55-58): X = the gathered feature rows, rel = the relation
 * columns [src - tgt | squared length] (mvp_relation4_rows_f32), W = the conv weight with its own row stride (ldw = Cin + 4), wrel = its last
 * four columns as a contiguous (Cout,4) matrix.  The relation part is evaluated in fp32 in the epilogue.  16-byte aligned operands,
 * Cin, Cout, ldx, ldw multiples of 4.  stat (2*Cout + 1 float64, zero on entry), mean, invstd, running_*: as mvp_mlp_forward_bn_f32, or all
 * NULL (no statistics: inference). */
int mvp_mlp_forward_rel_bn_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout, const float* rel,
                               const float* wrel, float* Y, double* stat, double* partial, float eps, float momentum, float* mean,
                               float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, mvp_stream_t stream);
/* out (R*K,4) = [src (R,K,3) - tgt (R,3) | squared length], the relation columns alone (pinned (dx*dx + dy*dy) + dz*dz) */
int mvp_relation4_rows_f32(const float* src_xyz, const float* tgt_xyz, int64_t R, int64_t K, float* out, mvp_stream_t stream);
/* Last layer of a set-abstraction shared MLP, training mode, WITHOUT materialising its (R,Cout) output (reference shape being replaced:
 * the (B,C,M,32) tensor of mvpnet/models/pn2/modules.py:100-108 + torch.max over dim 3).  Rows are groups of K = 32 consecutive
 * neighbours (R = 32 G).  Leaves per group and column the largest / smallest PRE-BatchNorm value (ymax, ymin (G,Cout) float32) and the
 * first row attaining each (amax, amin (G,Cout) uint8), the layer's batch statistics (stat, 2*Cout + 1 float64 zero on entry; partial = scratch of
 * ceil(R/128)*2*Cout doubles) and its BatchNorm finalize as mvp_mlp_forward_bn_f32.  mvp_pool_finalize_f32 then gives
 * out = max_k relu(bn(y_k)) (exact: bn o relu is monotone in y), arg, and ysel (the pre-BN value behind out: the backward's xhat).
 * MVP_EUNSUPPORTED unless split-bf16 precision, Cin, Cout <= 128, Cin % 4 == 0, Cout % 4 == 0, R % 32 == 0, R >= 32768. */
int mvp_mlp_forward_pool_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
                             const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, float* ymax,
                             float* ymin, uint8_t* amax, uint8_t* amin, double* stat, double* partial, float eps, float momentum,
                             float* mean, float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                             mvp_stream_t stream);
int mvp_pool_finalize_f32(const float* ymax, const float* ymin, const uint8_t* amax, const uint8_t* amin, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, int64_t G, int64_t C, int relu, float* out,
                          uint8_t* arg, float* ysel, mvp_stream_t stream);
/* BatchNorm-backward column sums of such a layer from the (G,C) tensors: stat[0:C] = sum dz, stat[C:2C] = sum dz * xhat, dz = dout where
 * out > 0 (relu), xhat = (ysel - mean) * invstd; stat is (re)initialised; partial = mvp_colstats_partial_count(G, C) doubles. */
int mvp_pool_backward_stats_f32(const float* dout, const float* out, const float* ysel, const float* mean, const float* invstd,
                                int64_t G, int64_t C, int relu, double* stat, double* partial, mvp_stream_t stream);
/* `partial` (both entry points below and above): optional scratch of ceil(R/128) * 2 * (output columns) float64; when
 * given, the statistics are reduced without atomics (recommended for R >~ 1e5), otherwise with fp64 atomics. */
/* d(input) with the previous layer's ReLU mask and BatchNorm-backward column sums fused into the epilogue:
 * dZ (R,Cin) = (dY (R,Cout) . W) * [bn(y_prev) > 0], W (Cout,Cin) as the forward uses it; stat (2*Cin float64) = [sum dZ | sum dZ*xhat].
 * y_prev == NULL: plain dX = dY . W. */
int mvp_mlp_input_grad_f32(const float* dY, int64_t R, int64_t Cout, const float* W, int64_t Cin, const float* y_prev,
                           const float* mean, const float* invstd, const float* gamma, const float* beta, float* dZ,
                           double* stat, double* partial, mvp_stream_t stream);
/* The same with the DROPOUT that sits behind the previous layer's activation (round 6; common/nn/modules/mlp.py:86-92: the segmentation head in front
 * of the logit layer, mvpnet/models/pn2/pn2ssg.py:111-118): dZ = (dY . W) * keep * 1/(1-p) * [bn(y_prev) > 0] with the keep mask regenerated from
 * (drop_p, drop_seed, element index) exactly as mvp_bn_rows_forward_dropout_f32 made it.  dZ and stat are then what the head's backward starts
 * from: its own pass over (gradient, y) for the two column sums (123 us + a reduction per step) is not run.  y_prev required; R * Cin < 2^32. */
int mvp_mlp_input_grad_dropout_f32(const float* dY, int64_t R, int64_t Cout, const float* W, int64_t Cin, const float* y_prev,
                                   const float* mean, const float* invstd, const float* gamma, const float* beta, float drop_p,
                                   uint64_t drop_seed, float* dZ, double* stat, double* partial, mvp_stream_t stream);

/* The WHOLE backward of shared-MLP layer i in one kernel (csrc/mlp_bwd.hip): BatchNorm-backward "finish" + weight gradient + input
 * gradient with the previous layer's ReLU mask and BatchNorm-backward column sums, from ONE read of dz_i, y_i and y_{i-1}
 * (2 C + 2 Cp floats of HBM traffic per row instead of the 5 C + 3 Cp of the three entry points above; no dy_i tensor).
 *   G (R,C): dz_i when Yi != NULL -- then dy_i = gamma_i*invstd_i * (dz_i - stat_i[c]/R - xhat_i * stat_i[C+c]/R), xhat_i from Yi,
 *            (training = 0 drops the two batch terms) and dgamma_i / dbeta_i (C, may be NULL) receive stat_i[C+c] / stat_i[c] --
 *            or dy_i itself when Yi == NULL;
 *   X (R,ldx): the layer's input; act_* != NULL: X is y_{i-1} and the input is relu(bn_{i-1}(y_{i-1})), re-created on the fly;
 *   dW (C,lddw) += dy_i^T . input;  dZ (R,Cp) or NULL = (dy_i . W) [* relu'(bn_{i-1}(y_{i-1}))];
 *   stat_prev (2 Cp, accumulated into): column sums of dZ and dZ * xhat_{i-1} (needs act_* and dZ; partial = float64 scratch of
 *   mvp_mlp_layer_backward_partial_count(R, Cp) values).
 * Contraction: split-bf16 only (mvp_set_mlp_precision 3 or 6); C <= 128, Cp <= 128, Cp % 4 == 0 -- otherwise MVP_EUNSUPPORTED.
 * Layers wider than 64 input channels are cut into c_in slices (one workgroup row each) that re-read dy_i.
 *   pool_dout / pool_out (R/32, C) float32, pool_arg (R/32, C) uint8, all NULL or all set: layer i is the last layer of a
 *            set-abstraction MLP that ran through mvp_mlp_forward_pool_f32 (its (R,C) output was never stored; rows = groups of 32
 *            neighbours).  G and Yi are then ignored (pass NULL): y_i is re-computed from X, dz_i = pool_dout at the arg-max row where
 *            pool_out > 0, stat_i from mvp_pool_backward_stats_f32.  Needs C, Cp <= 64, R % 32 == 0, act_* set. */
int64_t mvp_mlp_layer_backward_partial_count(int64_t R, int64_t Cp);
int mvp_mlp_layer_backward_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float* gamma_i,
                               const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* X, int64_t ldx,
                               const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta,
                               const float* W, int64_t ldw, int64_t R, int64_t C, int64_t Cp, float* dW, int64_t lddw, float* dZ,
                               double* stat_prev, double* partial, const float* pool_dout, const float* pool_out,
                               const uint8_t* pool_arg, mvp_stream_t stream);
/* The same with the weight gradient through a workspace + ordered reduction instead of fp32 atomics (see mvp_mlp_weight_grad_ws_f32;
 * mvp_mlp_weight_grad_workspace_floats() floats are enough, a smaller / NULL workspace takes the atomics). */
int mvp_mlp_layer_backward_ws_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float* gamma_i,
                               const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* X, int64_t ldx,
                               const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta,
                               const float* W, int64_t ldw, int64_t R, int64_t C, int64_t Cp, float* dW, int64_t lddw, float* dZ,
                               double* stat_prev, double* partial, const float* pool_dout, const float* pool_out,
                               const uint8_t* pool_arg, float* workspace, int64_t workspace_floats, mvp_stream_t stream);
/* One-pass backward of a shared-MLP layer with up to 128 channels on either side (csrc/mlp_bwd_wide.hip, round 5): what
 * mvp_mlp_layer_backward_f32 computes -- BatchNorm-backward finish of layer i, dW_i, dz_{i-1} with the ReLU mask and the two
 * BatchNorm-backward column sums of layer i-1 -- with the row tile staged in LDS (64 rows per persistent workgroup, transpose reads feed
 * the dW contraction): 2 C + 2 Cp floats of HBM traffic per row at 128 channels, where the register-resident kernel has to slice c_in.
 * Replaces autograd through common/nn/modules/conv.py:41-51 for the 128-wide layers of mvpnet/models/pn2/pn2ssg.py:69-82,101-118.
 *   mode 0: G (R,C) is dy_i itself (Yi, mean_i .. stat_i unused);
 *   mode 1: G is dz_i = the gradient w.r.t. layer i's activation, ReLU mask applied: dy_i = gamma_i*invstd_i * (dz_i - stat_i[c]/R -
 *           xhat_i * stat_i[C+c]/R), xhat_i from Yi (training = 0 drops the batch terms);
 *   mode 2: G is da_i = the gradient w.r.t. the layer's OUTPUT -- after its ReLU and, with drop_p > 0, after the dropout of
 *           mvp_bn_rows_forward_dropout_f32(drop_p, drop_seed) -- dz_i is formed while the rows are loaded (keep mask regenerated, ReLU mask
 *           from Yi, beta_i needed), then as mode 1; stat_i = the sums mvp_bn_rows_backward[_dropout]_f32 leaves with dy == NULL.
 *   dgamma_i / dbeta_i (C, may be NULL; modes 1, 2) <- stat_i[C + c] / stat_i[c].
 *   X (R,ldx) = y_{i-1} with act_* (all four) = BatchNorm + ReLU of layer i-1, or the plain layer input with act_* NULL;
 *   dW (C,lddw) += dy_i^T . input;  dZ (R,Cp) = (dy_i . W) [* relu'(bn_{i-1}(y_{i-1}))];  stat_prev (2 Cp, with act_*) += the column
 *   sums of dZ and dZ * xhat_{i-1} (fp64 atomics, one per column and workgroup: no reduction launch).
 *   ticket: one zeroed int32 of caller memory, or NULL.  With it the workgroups take their tiles in ticket order, so a CU that another
 *           stream keeps busy costs its share of the tiles instead of a second round; NULL = static round-robin.
 *   workspace / workspace_floats: as mvp_mlp_layer_backward_ws_f32 (reproducible weight gradient: ordered reduction, static tile order);
 *           NULL / 0 = fp32 atomics.
 *   precision / precision_backward: as every `_p_f32` entry point (-1 = the process defaults).  Needs a 1- or 2-piece backward split
 *   (bf16 / bf16x3), C, Cp <= 128, C % 4 == Cp % 4 == ldx % 4 == 0, 16-byte aligned G / Yi / X / dZ: MVP_EUNSUPPORTED otherwise (callers
 *   then take mvp_mlp_layer_backward_f32 or the three separate entry points). */
int mvp_mlp_layer_backward_wide_p_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float* gamma_i,
                                      const float* beta_i, const double* stat_i, float* dgamma_i, float* dbeta_i, int training, int mode,
                                      float drop_p, uint64_t drop_seed, const float* X, int64_t ldx, const float* act_mean,
                                      const float* act_invstd, const float* act_gamma, const float* act_beta, const float* W, int64_t ldw,
                                      int64_t R, int64_t C, int64_t Cp, float* dW, int64_t lddw, float* dZ, double* stat_prev, int* ticket,
                                      float* workspace, int64_t workspace_floats, int precision, int precision_backward, mvp_stream_t stream);
/* The same with a SUM over pool_k consecutive rows behind the layer (FeatureAggregation's last layer: mvpnet/models/mvpnet_3d.py:40-41,59 sums the
 * k neighbours): mode 2, G (R / pool_k, C) = the gradient w.r.t. the POOLED output, row r of the layer takes row r / pool_k of it while the rows
 * are loaded -- no (R, C) gradient tensor and no pass that writes one.  stat_i = the sums mvp_bn_rows_backward_f32(K = pool_k, arg = NULL,
 * dy = NULL) leaves.  pool_k == 1: exactly mvp_mlp_layer_backward_wide_p_f32 (any mode); pool_k > 1 needs mode 2, drop_p == 0, R % pool_k == 0. */
int mvp_mlp_layer_backward_wide_pooled_p_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float* gamma_i,
                                             const float* beta_i, const double* stat_i, float* dgamma_i, float* dbeta_i, int training, int mode,
                                             int64_t pool_k, float drop_p, uint64_t drop_seed, const float* X, int64_t ldx, const float* act_mean,
                                             const float* act_invstd, const float* act_gamma, const float* act_beta, const float* W, int64_t ldw,
                                             int64_t R, int64_t C, int64_t Cp, float* dW, int64_t lddw, float* dZ, double* stat_prev, int* ticket,
                                             float* workspace, int64_t workspace_floats, int precision, int precision_backward, mvp_stream_t stream);
/* dW (Cout,Cin) += dy^T . X with the BatchNorm-backward FINISH of the dY operand applied while it is loaded (round 5): dZ (R,Cout) = the gradient
 * w.r.t. the layer's activation with its ReLU mask applied, Y (R,Cout) its pre-BN output, stat (2 Cout) = [sum dZ | sum dZ * xhat]:
 * dy = gamma * invstd * ((dZ - stat[c] / R) - xhat * stat[Cout + c] / R) (training = 0: no batch terms), formed in registers with the operations
 * of mvp_bn_rows_backward_finish_f32 -- the result of that pass followed by mvp_mlp_weight_grad[_ws]_f32 without the pass and without the (R,Cout)
 * tensor it writes.  For a first layer whose input needs no gradient (FeatureAggregation on a frozen 2D branch, mvpnet/models/mvpnet_3d.py:37-61)
 * nothing else needs dy.  X (R,ldx) plain (no activation prologue).  workspace / workspace_floats as mvp_mlp_weight_grad_ws_f32 (NULL / 0: fp32
 * atomics); precision arguments as every `_p_f32` entry point.  Supported: Cout % 4 == 0, 33 <= Cout, 16-byte aligned dZ / Y, and either Cin >= 33
 * on the split-bf16 kernel (1 or 2 backward pieces) or Cin <= 32 with 16-byte aligned rows on the fp32 kernel -- the kernel of the fp32 precision
 * and, under a split precision, of Cin < 8 only (8 <= Cin <= 32 under a split precision is refused); MVP_EUNSUPPORTED otherwise (the caller
 * then runs the finish pass). */
int mvp_mlp_weight_grad_finish_p_f32(const float* dZ, const float* Y, const float* mean, const float* invstd, const float* gamma, const double* stat,
                                     int training, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx, float* dW, int64_t lddw,
                                     float* workspace, int64_t workspace_floats, int precision, int precision_backward, mvp_stream_t stream);
/* The same for a FIRST layer over [X (R,Cin) | REL (R,4)] in ONE launch (round 6): dW (Cout,lddw)[:, :Cin] += dy^T . X and dWrel (Cout,lddw)[:, :4] += dy^T . REL
 * -- FeatureAggregation's first conv over cat[feature, src - tgt, |src - tgt|^2] (mvpnet/models/mvpnet_3d.py:55-58), whose weight gradient was two
 * launches that each streamed dZ and Y (the last, exposed kernels of the backward pass).  33 <= Cin <= 64, 33 <= Cout, one- or two-piece backward
 * split, fp32 atomics only (the reproducible mode keeps the two launches); MVP_EUNSUPPORTED otherwise. */
int mvp_mlp_weight_grad_finish_rel_p_f32(const float* dZ, const float* Y, const float* mean, const float* invstd, const float* gamma, const double* stat,
                                         int training, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx, const float* REL, float* dW,
                                         float* dWrel, int64_t lddw, int precision, int precision_backward, mvp_stream_t stream);
/* The same with X = the previous layer's PRE-BN output and its BatchNorm + ReLU applied while it is loaded (act_*: as mvp_mlp_weight_grad_f32, all
 * NULL = X plain): the weight gradient of an INNER layer whose finish pass is skipped (round 6: the 256- / 512-wide layers, whose input gradient
 * forms dy on load as well -- mvp_mlp_input_grad_wide_p_f32).  Same support matrix as above; an activation needs the split-bf16 kernel (Cin >= 33). */
int mvp_mlp_weight_grad_finish_act_p_f32(const float* dZ, const float* Y, const float* mean, const float* invstd, const float* gamma, const double* stat,
                                         int training, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx, const float* act_mean,
                                         const float* act_invstd, const float* act_gamma, const float* act_beta, float* dW, int64_t lddw,
                                         float* workspace, int64_t workspace_floats, int precision, int precision_backward, mvp_stream_t stream);
/* Input gradient of a WIDE shared-MLP layer i (C = 64 .. 512 output channels in multiples of 64, Cp input channels in multiples of 128) in one
 * pass (round 6, csrc/mlp_dx_wide.hip; replaces, for the 256- / 512-wide layers of mvpnet/models/pn2/pn2ssg.py:26,30,69-82, the BatchNorm-backward
 * finish pass + mvp_mlp_input_grad_f32 + its reduction launch; autograd through common/nn/modules/conv.py:41-51):
 *   dZ (R,Cp) = (dy_i . W) * [ bn(y_{i-1}) > 0 ],  stat_prev (2 Cp, accumulated into) += [sum dZ | sum dZ * xhat_{i-1}],
 * with dy_i = G (Yi == NULL) or formed from dz_i = G while it is loaded (Yi, mean_i, invstd_i, gamma_i, stat_i, training: as
 * mvp_mlp_weight_grad_finish_p_f32; dgamma_i / dbeta_i (may be NULL) <- the two halves of stat_i).  X (R,ldx) = y_{i-1} with the BatchNorm of
 * layer i-1 in act_* (required).  W (C,ldw) is read through a pre-split bf16 image that the call writes into `workspace` first
 * (mvp_mlp_input_grad_wide_workspace_bytes(C, Cp) bytes, 16-byte aligned, contents irrelevant, not kept).  One- or two-piece backward split,
 * 16-byte aligned G / Yi / X / dZ, ldx % 4 == 0; MVP_EUNSUPPORTED otherwise (the caller keeps the per-layer kernels).  No dW: the weight
 * gradient of such a layer is its own launch (mvp_mlp_weight_grad_f32 / mvp_mlp_weight_grad_finish_act_p_f32). */
int64_t mvp_mlp_input_grad_wide_workspace_bytes(int64_t C, int64_t Cp);
int mvp_mlp_input_grad_wide_p_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float* gamma_i,
                                  const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* X, int64_t ldx,
                                  const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, const float* W,
                                  int64_t ldw, int64_t R, int64_t C, int64_t Cp, float* dZ, double* stat_prev, void* workspace,
                                  int64_t workspace_bytes, int precision, int precision_backward, mvp_stream_t stream);
/* dW (Cout,Cin) += dY (R,Cout)^T . act(X (R,ldx)[:, :Cin]) with the same act() prologue.  lddw >= Cin = row stride of dW:
 * Cin for a dense gradient, the full weight's column count when dW points at a column slice of it. */
int mvp_mlp_weight_grad_f32(const float* dY, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx,
                            const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta,
                            float* dW, int64_t lddw, mvp_stream_t stream);
/* The same through a caller-provided workspace (contents irrelevant, not kept): the workgroups of the split-bf16 kernel leave their
 * partial tiles there and a second launch adds them to dW in row-split order: no fp32 atomics (the flush of ~1000 workgroups queues up
 * to 512 of them on every dW element) and the same dW bit for bit in every run.  mvp_mlp_weight_grad_workspace_floats() floats are
 * always enough; a smaller or NULL workspace takes the atomics path above.  One workspace per stream. */
int64_t mvp_mlp_weight_grad_workspace_floats(void);
int mvp_mlp_weight_grad_ws_f32(const float* dY, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx,
                               const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta,
                               float* dW, int64_t lddw, float* workspace, int64_t workspace_floats, mvp_stream_t stream);

/* ---- a set-abstraction level in TRAINING mode without its (B*M*32, C) tensors (csrc/sa_train.hip) ---------------------------------------
 * replaces, forward and backward, QueryGrouper + SharedMLP(ndim=2, bn=True) + torch.max of mvpnet/models/pn2/modules.py:20-37,100-108
 * (common/nn/modules/conv.py:41-51 with BATCH statistics).  Batch statistics force one pass over the level per layer; each pass
 * RE-CREATES the ball's rows from the per-point tensor zf (B,N,C1) = first-layer feature columns applied per point, the coordinates and
 * the ball index instead of loading stored activations:
 *   plan      mvp_sa_geom_sums_f32: per point the sum of the centred coordinates of the rows that gathered it and their count (dsum (B,N,4)),
 *             and the batch-wide first and second moments of the centred coordinates (gsum: 16 float64, zero on entry) -- coordinates only
 *   forward   pass 1: mvp_sa_train_stats1_f32: statistics of y_1 + BatchNorm-1 finalize from per-POINT sums (y_1 is affine in per-point data),
 *                     + zsum (C1,3) for the backward  (or mvp_group_lin_rows_bn_f32 with out == NULL: the same statistics row by row)
 *             pass 2: mvp_sa_train_forward_f32(stage 2): statistics of y_2 + BatchNorm-2 finalize (mean, invstd, running statistics)
 *             pass 3: mvp_sa_train_forward_f32(stage 3): statistics of y_3 + finalize, and per ball and column the largest / smallest pre-BN
 *                     y_3 with the first row attaining each (ymax, ymin, amax, amin: (B*M, C3)) -> mvp_pool_finalize_f32 pools exactly
 *   backward  mvp_pool_backward_stats_f32, then
 *             mvp_sa_train_backward_f32(layer 3): dW3 +=, dz_2 (B*M*32, C2) stored, its two column sums += stat_prev, dgamma3 / dbeta3
 *             mvp_sa_train_backward_f32(layer 2): dz_2 read, dW2 +=, dz_1 (B*M*32, C1) stored, column sums, dgamma2 / dbeta2
 *             mvp_sa_train_backward1_f32: per POINT: a plain gather of dz_1 through the transposed ball index (mvp_csr_build_i64) + the
 *                     closed-form BatchNorm-backward terms -> gradient of zf; gradient of the first layer's coordinate columns from tsum
 *                     (accumulated by the layer-2 pass), zsum, gsum; dgamma1 / dbeta1
 * Only dz_2 and dz_1 ever have the shape (B*M*32, C) in memory -- and y_2, where the caller chooses the _y2 forms below.  stat: 2*C + 1 float64, ALL zero on entry (sums of y, of y^2, completion
 * counter: zero again on exit); stat_prev: 2*Cp float64 accumulated into.  training = 0 drops the batch terms of the BatchNorm backward.
 * Needs K == 32, C1, C2 <= 64, C3 <= 64 (C3 <= 128 when C1, C2 > 32: level 2 of the reference network), multiples of 4, zf 16-byte aligned, a
 * split-bf16 precision: MVP_EUNSUPPORTED otherwise (callers then take the per-layer entry points).  mvp_sa_train_forward_f32 and
 * mvp_sa_train_backward_f32 also return MVP_EUNSUPPORTED beyond the limits of their 32-bit ball and row-offset arithmetic: N, M <= INT_MAX,
 * B * M <= 2^31 - 16, N * max(C1, 3) < 2^32. */
int mvp_sa_train_forward_f32(int stage, const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz,
                             int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd,
                             const float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean,
                             const float* bn2_invstd, const float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3,
                             double* stat, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                             float* running_var, int64_t* num_batches_tracked, float* ymax, float* ymin, uint8_t* amax, uint8_t* amin,
                             mvp_stream_t stream);
int mvp_sa_train_backward_f32(int layer, const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz,
                              int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd,
                              const float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean,
                              const float* bn2_invstd, const float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3,
                              const float* mean_i, const float* invstd_i, const float* gamma_i, const double* stat_i, float* dgamma_i,
                              float* dbeta_i, int training, const float* G, const float* pool_dout, const float* pool_out,
                              const uint8_t* pool_arg, float* dW, int64_t lddw, float* dZ, double* stat_prev, float* tsum, mvp_stream_t stream);
/* The same two with y_2 STORED once instead of re-created by every pass that needs it: one more parameter in front of the stream,
 * Y2 (B*M*32, C2) float32, 16-byte aligned.  forward(stage 2) also writes y_2 there; forward(stage 3), backward(layer 3) and backward(layer 2)
 * read it and skip the chain that re-creates it (the level's rows -> BatchNorm 1 + ReLU -> the contraction with W2).  Every pass may be
 * given Y2 or not independently of the others (the values are the same bit for bit: stage 3 repeats stage 2's code and the backward
 * re-computes with the forward's split), as long as the stage-2 call that precedes a reader was given it.  Y2 == NULL: exactly
 * mvp_sa_train_forward_f32 / mvp_sa_train_backward_f32.  MVP_EUNSUPPORTED for a Y2 that is not 16-byte aligned. */
int mvp_sa_train_forward_y2_f32(int stage, const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz,
                                int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd,
                                const float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean,
                                const float* bn2_invstd, const float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3,
                                double* stat, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                                float* running_var, int64_t* num_batches_tracked, float* ymax, float* ymin, uint8_t* amax, uint8_t* amin,
                                float* Y2, mvp_stream_t stream);
int mvp_sa_train_backward_y2_f32(int layer, const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz,
                                 int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd,
                                 const float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean,
                                 const float* bn2_invstd, const float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3,
                                 const float* mean_i, const float* invstd_i, const float* gamma_i, const double* stat_i, float* dgamma_i,
                                 float* dbeta_i, int training, const float* G, const float* pool_dout, const float* pool_out,
                                 const uint8_t* pool_arg, float* dW, int64_t lddw, float* dZ, double* stat_prev, float* tsum, const float* Y2,
                                 mvp_stream_t stream);
int mvp_sa_train_backward1_f32(const float* dz1, const int32_t* offsets, const int32_t* slots, const float* zf, const float* dsum,
                               const float* wxyz, const float* tsum, const double* zsum, const double* gsum, int64_t B, int64_t N, int64_t M,
                               int64_t K, int64_t C1, const float* mean, const float* invstd, const float* gamma, const double* stat,
                               int training, float* dgamma, float* dbeta, float* gz, float* dWxyz, int64_t lddw, mvp_stream_t stream);
int mvp_sa_geom_sums_f32(const int32_t* offsets, const int32_t* slots, const float* xyz, const float* centre, int64_t B, int64_t N, int64_t M,
                         int64_t K, float* dsum, double* gsum, mvp_stream_t stream);
int mvp_sa_train_stats1_f32(const float* zf, const float* dsum, const float* wxyz, const double* gsum, int64_t B, int64_t N, int64_t M, int64_t K,
                            int64_t C1, double* stat, double* zsum, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, mvp_stream_t stream);
/* The same with a scratch of `scratch_doubles` float64, ZERO on entry: up to 16 replicas of the 5 C1 sums that the workgroups add into (an fp64
 * atomic on one address costs ~0.16 us and every workgroup ends with one per address: 58 -> ~25 us at 262 144 points); the last workgroup adds the
 * replicas up into stat / zsum.  scratch == NULL or fewer than 10 C1 doubles: exactly mvp_sa_train_stats1_f32. */
int mvp_sa_train_stats1_ws_f32(const float* zf, const float* dsum, const float* wxyz, const double* gsum, int64_t B, int64_t N, int64_t M, int64_t K,
                               int64_t C1, double* stat, double* zsum, float eps, float momentum, float* mean, float* invstd, float* running_mean,
                               float* running_var, int64_t* num_batches_tracked, double* scratch, int64_t scratch_doubles, mvp_stream_t stream);

/* ---- the shared-MLP entry points with the contraction precision as ARGUMENTS (csrc/mlp_prec.hip) -----------------------------------
 * mvp_<name>_p_f32 = mvp_<name>_f32 with two more parameters in front of the stream:
 *     precision           contraction of this call: 0 = fp32 MFMA, 1 = bf16, 3 = bf16x3, 6 = bf16x6, -1 = the default
 *     precision_backward  split of a gradient contraction made by this call: 1, 3, 6, -1 = the default
 * With both >= 0 nothing process-wide is read: mvp_set_mlp_precision[_backward] only provide the defaults that -1 selects (SURVEY 8b:
 * stateless, re-entrant -- the reference's ops take everything they depend on as arguments: the pybind signatures under mvpnet/ops/cuda).  The host code hands
 * the precision a forward ran with to the node's backward calls, which autograd issues from another thread.  MVP_EINVAL for other values. */
int mvp_mlp_forward_p_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout, const
    float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, const float* bias, float* Y,
    double* stat, double* partial, int precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_forward_bn_p_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
    const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, float* Y, double* stat,
    double* partial, float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var, int64_t*
    num_batches_tracked, int precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_forward_rel_bn_p_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
    const float* rel, const float* wrel, float* Y, double* stat, double* partial, float eps, float momentum, float* mean, float*
    invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, int precision, int precision_backward,
    mvp_stream_t stream);
int mvp_mlp_forward_pool_p_f32(const float* X, int64_t R, int64_t Cin, int64_t ldx, const float* W, int64_t ldw, int64_t Cout,
    const float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, float* ymax, float* ymin,
    uint8_t* amax, uint8_t* amin, double* stat, double* partial, float eps, float momentum, float* mean, float* invstd, float*
    running_mean, float* running_var, int64_t* num_batches_tracked, int precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_input_grad_p_f32(const float* dY, int64_t R, int64_t Cout, const float* W, int64_t Cin, const float* y_prev, const
    float* mean, const float* invstd, const float* gamma, const float* beta, float* dZ, double* stat, double* partial, int
    precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_input_grad_dropout_p_f32(const float* dY, int64_t R, int64_t Cout, const float* W, int64_t Cin, const float* y_prev, const
    float* mean, const float* invstd, const float* gamma, const float* beta, float drop_p, uint64_t drop_seed, float* dZ, double* stat,
    double* partial, int precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_weight_grad_p_f32(const float* dY, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx, const float*
    act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, float* dW, int64_t lddw, int precision,
    int precision_backward, mvp_stream_t stream);
int mvp_mlp_weight_grad_ws_p_f32(const float* dY, const float* X, int64_t R, int64_t Cout, int64_t Cin, int64_t ldx, const
    float* act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, float* dW, int64_t lddw, float*
    workspace, int64_t workspace_floats, int precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_layer_backward_p_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float*
    gamma_i, const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* X, int64_t ldx, const float*
    act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, const float* W, int64_t ldw, int64_t R,
    int64_t C, int64_t Cp, float* dW, int64_t lddw, float* dZ, double* stat_prev, double* partial, const float* pool_dout, const
    float* pool_out, const uint8_t* pool_arg, int precision, int precision_backward, mvp_stream_t stream);
int mvp_mlp_layer_backward_ws_p_f32(const float* G, const float* Yi, const float* mean_i, const float* invstd_i, const float*
    gamma_i, const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* X, int64_t ldx, const float*
    act_mean, const float* act_invstd, const float* act_gamma, const float* act_beta, const float* W, int64_t ldw, int64_t R,
    int64_t C, int64_t Cp, float* dW, int64_t lddw, float* dZ, double* stat_prev, double* partial, const float* pool_dout, const
    float* pool_out, const uint8_t* pool_arg, float* workspace, int64_t workspace_floats, int precision, int precision_backward,
    mvp_stream_t stream);
int mvp_sa_fused_forward_p_f32(const float* zf, const float* xyz, const float* centre, const int64_t* index, const float* wxyz,
    int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd, const float*
    bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean, const float* bn2_invstd, const float*
    bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3, const float* bn3_mean, const float* bn3_invstd, const float*
    bn3_gamma, const float* bn3_beta, float* out, uint8_t* arg, int precision, int precision_backward, mvp_stream_t stream);

int mvp_sa_train_forward_p_f32(int stage, const float* zf, const float* xyz, const float* centre, const int64_t* index, const
    float* wxyz, int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd, const
    float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean, const float* bn2_invstd, const
    float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3, double* stat, float eps, float momentum, float* mean,
    float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* ymax, float* ymin, uint8_t*
    amax, uint8_t* amin, int precision, int precision_backward, mvp_stream_t stream);
int mvp_sa_train_backward_p_f32(int layer, const float* zf, const float* xyz, const float* centre, const int64_t* index, const
    float* wxyz, int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd, const
    float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean, const float* bn2_invstd, const
    float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3, const float* mean_i, const float* invstd_i, const
    float* gamma_i, const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* G, const float* pool_dout,
    const float* pool_out, const uint8_t* pool_arg, float* dW, int64_t lddw, float* dZ, double* stat_prev, float* tsum, int precision, int
    precision_backward, mvp_stream_t stream);
int mvp_sa_train_forward_y2_p_f32(int stage, const float* zf, const float* xyz, const float* centre, const int64_t* index, const
    float* wxyz, int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd, const
    float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean, const float* bn2_invstd, const
    float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3, double* stat, float eps, float momentum, float* mean,
    float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked, float* ymax, float* ymin, uint8_t*
    amax, uint8_t* amin, float* Y2, int precision, int precision_backward, mvp_stream_t stream);
int mvp_sa_train_backward_y2_p_f32(int layer, const float* zf, const float* xyz, const float* centre, const int64_t* index, const
    float* wxyz, int64_t B, int64_t N, int64_t M, int64_t K, int64_t C1, const float* bn1_mean, const float* bn1_invstd, const
    float* bn1_gamma, const float* bn1_beta, const float* W2, int64_t C2, const float* bn2_mean, const float* bn2_invstd, const
    float* bn2_gamma, const float* bn2_beta, const float* W3, int64_t C3, const float* mean_i, const float* invstd_i, const
    float* gamma_i, const double* stat_i, float* dgamma_i, float* dbeta_i, int training, const float* G, const float* pool_dout,
    const float* pool_out, const uint8_t* pool_arg, float* dW, int64_t lddw, float* dZ, double* stat_prev, float* tsum, const float* Y2,
    int precision, int precision_backward, mvp_stream_t stream);

/* ---- the coordinate-only work of a PointNet++ (SSG) network in ONE call (csrc/plan.hip) -----------------------------------------------
 * replaces the geometry half of SetAbstraction / FeatureInterpolator called level after level from Python (mvpnet/models/pn2/modules.py:
 * 74-87,122-140, pn2ssg.py:92-115): one sampling launch + the centroid prefixes of all levels (mvp_fps_centroid_levels_f32), a ball query per
 * level, 3-NN + interpolation weights per propagation level, optionally (flags bit 0) the transposed index of every ball / 3-NN index
 * (bit 2: the sorted build) and (bit 1) mvp_sa_geom_sums_f32 for the levels with geom[l] != 0; bit 3: the table ends with one more entry,
 * scratch of max_l of mvp_ball_query_grid_workspace(B, M_l, N_l) and mvp_knn3_grid_workspace(B, N_l, M_l) bytes, and the levels those functions accept use mvp_ball_query_grid_f32 / mvp_knn3_grid_f32 -- the same launches in the same order on
 * `stream`, from one table of caller-allocated buffers instead of ~25 calls (0.65 ms of host time per plan from Python).
 * xyz (B,N,3); centroids / radius / neighbours: host arrays of `levels` <= 8 entries, centroids non-increasing and <= N.
 * buffers (host array of n_buffers device pointers, all non-NULL, in this order; N_l = N for l = 0, else centroids[l-1]):
 *   fps_index (B,centroids[0]) i64;
 *   per level l = 0 ..: new_xyz (B,M_l,3) f32, ball (B,M_l,K_l) i64 [, offsets (B,N_l+1) i32, slots (B,M_l*K_l) i32, cursor (B,N_l) i32
 *                       [, dsum (B,N_l,4) f32, gsum (16) f64 zeroed by the caller]];
 *   per propagation level l = levels-1 .. 0: index (B,N_l,3) i64, weight (B,N_l,3) f32 [, offsets (B,M_l+1) i32, slots (B,3*N_l) i32, cursor (B,M_l) i32].
 * events: NULL or `levels` hipEvent_t handles, events[l] recorded once level l's centroids + ball index (+ transposed index, sums) are queued.
 * fps_status: see mvp_fps_checked_f32 (may be NULL).  MVP_EINVAL when n_buffers does not match the flags. */
int mvp_pn2_plan_f32(const float* xyz, int64_t B, int64_t N, int64_t levels, const int64_t* centroids, const float* radius,
                     const int64_t* neighbours, const int32_t* geom, int fps_shape, int flags, float knn_eps, void* const* buffers,
                     int64_t n_buffers, void* const* events, int* fps_status, mvp_stream_t stream);

/* ---- chunk -> scene vote ----------------------------------------------------------------
 * replaces the NumPy accumulation of mvpnet/test_mvpnet_3d.py:137-138,160-174.
 * accumulate: logit (n,C) rows of one chunk (row stride ld, so a (C,n) tensor can be passed
 *   transposed: element (r,c) at logit[r*ld_r + c*ld_c]); sum (n_pts,C) += , count (n_pts) int32 += 1.
 * finish    : mean = sum / max(count,1); label = argmax (first max), count == 0 -> C. */
int mvp_vote_accumulate_f32(const float* logit, int64_t ld_r, int64_t ld_c, const int64_t* chunk_ind, int64_t n,
                            int64_t C, float* sum, int32_t* count, mvp_stream_t stream);
/* all chunks of a scene in ONE launch (the reference loop: mvpnet/test_mvpnet_3d.py:142-174), atomics-free and in the reference's order of
 * additions: chunk i's logits at logit + i*ld_chunk, element (r,c) of it at r*ld_r + c*ld_c; chunk_offsets (num_chunks + 1 int64): where each
 * chunk's index list starts in the concatenation of all lists; point_offsets (n_pts + 1) / point_slots: the transposed index of that
 * concatenation (mvp_csr_build_i64 with B = 1: for every scene point the flat positions that name it).  sum (n_pts,C) and count (n_pts)
 * are WRITTEN (not accumulated): sum[p] = the logits of p's positions added in ascending position = chunk order, bit-identical to
 * num_chunks calls of mvp_vote_accumulate_f32 in chunk order. */
int mvp_vote_gather_f32(const float* logit, int64_t ld_chunk, int64_t ld_r, int64_t ld_c, const int64_t* chunk_offsets, int64_t num_chunks,
                        const int32_t* point_offsets, const int32_t* point_slots, int64_t n_pts, int64_t C, float* sum, int32_t* count,
                        mvp_stream_t stream);
int mvp_vote_finish_f32(const float* sum, const int32_t* count, int64_t n_pts, int64_t C, float* mean, int64_t* label,
                        mvp_stream_t stream);
/* the whole-scene test of the 2D baseline behind the 2D network (mvpnet/test_2d_chunks.py:119-157 with mvpnet/models/mvpnet_2d.py:22-34:
 * per chunk, class logits gathered through the pixel k-NN, averaged over k, `+=` into the scene) in ONE launch, atomics-free, from a
 * store that holds the logits of every DISTINCT picked frame once.
 *   logit: element (store frame u, pixel q, class c) at logit[u*ld_f + q*ld_p + c*ld_c], U frames of hw = h*w pixels and C classes: the
 *     network's output where it lies, NCHW (ld_c = hw, ld_p = 1) or channels-last (ld_p = C, ld_c = 1).  A channels-last store with
 *     C % 4 == 0, ld_p % 4 == 0, ld_f % 4 == 0 and 16-byte aligned logit / sum is read with 16-byte loads; anything else one dword per class.
 *   view_frame (num_chunks,nv) int32: the store frame of each chunk's view; a frame outside [0,U) counts as missing.
 *   knn: int64 rows of k chunk-local flat pixel ids view*hw + q, as mvp_lift_f32 / mvp_pixel_knn_projective_f32 write them; an id < 0
 *     (or >= nv*hw) is missing.  knn_base (num_chunks) int64: the row in knn of each chunk's first point (chunks are searched in padded
 *     batches, so their rows are not back to back).  Rows beyond a chunk's valid length are never read.
 *   chunk_offsets (num_chunks + 1), point_offsets (n_pts + 1), point_slots: exactly as mvp_vote_gather_f32 takes them.
 *   sum (n_pts,C), count (n_pts): WRITTEN, not accumulated.
 * Definition (pinned).  For position e of the concatenated chunk lists, in chunk i at row r = e - chunk_offsets[i], with l_j[c] the
 * logit of neighbour j = knn[(knn_base[i] + r)*k + j] -- +0 for a missing one --:
 *     m_e[c] = (((l_0[c] + l_1[c]) + ...) + l_{k-1}[c]) / k     in float32, every addition and the division rounded once (__fdiv_rn,
 *                                                               no reciprocal), never contracted;
 *     sum[p][c] = ((0 + m_e1[c]) + m_e2[c]) + ...               over p's positions in ASCENDING position = chunk order, the reference's
 *                                                               `+=` order; count[p] = the number of positions.
 * The same bits every run.  Mean and labels: mvp_vote_finish_f32.
 * Before any launch: MVP_EINVAL unless 1 <= k <= 8, 1 <= C <= 64, nv, U, hw, num_chunks >= 1, n_pts >= 0 and ld_f, ld_p, ld_c >= 0;
 * MVP_EUNSUPPORTED unless nv*hw < 2^31, U < 2^31, num_chunks < 2^30, num_chunks*nv < 2^31 and n_pts < 2^31 (what the kernel holds in 32
 * bits; offsets into logit, knn and sum are formed in 64).  n_pts == 0: nothing is launched. */
int mvp_lift_vote_f32(const float* logit, int64_t ld_f, int64_t ld_p, int64_t ld_c, int64_t U, int64_t hw, int64_t C,
                      const int32_t* view_frame, int64_t nv, const int64_t* knn, int64_t k, const int64_t* knn_base,
                      const int64_t* chunk_offsets, int64_t num_chunks, const int32_t* point_offsets, const int32_t* point_slots,
                      int64_t n_pts, float* sum, int32_t* count, mvp_stream_t stream);
/* whole-scene voting (mvpnet/test_3d_scene.py:152-164: per vote a scikit-learn ball tree over the vote's sampled points on the host,
 * `pred_logit_whole_scene += seg_logit_per_vote[nn_indices[:, 0]]`): all votes in ONE query launch behind one grid-build launch.
 * points (n,3): the scene's points, shared by all votes.  key (V,nb,3): the sampled points of each vote.  logit: element (v,j,c) at
 * logit[v*ld_vote + j*ld_r + c*ld_c], so the network's (V,C,nb) output goes in with its own strides, row-major storage included.
 *   nearest key: nn_v(p) = the key j of vote v with the smallest float32 (dx*dx + dy*dy) + dz*dz to p (each operation rounded once,
 *     never contracted: the expression of every index kernel here); among equal distances the LOWEST key index wins.
 *   sum (n,C), WRITTEN: sum[p,c] = (...(logit[0,nn_0(p),c] + logit[1,nn_1(p),c]) + ...) in vote order in float32, without atomics:
 *     bit-reproducible, and the reference's `+=` on a zeroed array.  Division by the number of votes and the argmax (first maximum) are
 *     mvp_vote_finish_f32 with a count of V for every point.
 *   nn_index (V,n) int64 or NULL: nn_v(p).
 *   swept: NULL, or one int32 counter ZEROED by the caller: += 1 for every (point, vote) whose search swept all nb keys because the
 *     27 cells around the point did not certify their minimum (and for every one when nb < 256, where there is no grid).
 *   non-finite coordinates: no fault, no hang; a point or key with a NaN / inf coordinate is never a nearest pair (such distances do
 *     not compare), a row without any comparable key gets index 0; rows whose point is finite are exact over the finite keys, and
 *     every index lies in [0, nb).
 * EINVAL before any launch unless 0 <= n < 2^31, 1 <= nb <= 65536, 1 <= V < 65536, 1 <= C <= 64, and -- when
 * mvp_vote_nearest_workspace(V, nb) > 0 -- workspace_bytes >= that figure and workspace 16-byte aligned.
 * mvp_vote_nearest_workspace: V * (16 nb + 16512) bytes of device scratch, reusable once the launches have run (stream order);
 * 0 for nb < 256 (the keys are swept, workspace may be NULL) and for shapes the call refuses. */
int64_t mvp_vote_nearest_workspace(int64_t V, int64_t nb);
int mvp_vote_nearest_f32(const float* points, int64_t n, const float* key, int64_t V, int64_t nb, const float* logit, int64_t ld_vote,
                         int64_t ld_r, int64_t ld_c, int64_t C, float* sum, int64_t* nn_index, int32_t* swept, void* workspace,
                         int64_t workspace_bytes, mvp_stream_t stream);

/* ---- segmentation loss and confusion matrix (the step after the path) -------------
 * Logits are addressed as element (b,c,n) at logit[b*ld_b + c*ld_c + n*ld_n]: the reference's (B,C,N) tensor
 * (ld_b = C*N, ld_c = N, ld_n = 1) or channels-last rows (B = 1, N = rows, ld_n = C, ld_c = 1).  label (B*N) int64;
 * points whose label is ignore_index (or outside [0,C)) are skipped.
 * mvp_seg_loss_f32: replaces F.cross_entropy(logit, label, weight, ignore_index) of mvpnet/models/loss.py:5-21 (mean
 *   reduction: sum w[y]*nll / sum w[y]).  acc: 3 float64, ZEROED by the caller ([sum w*nll, sum w, ticket]); loss: 1 float,
 *   written by the last workgroup (nan when no point is valid, as torch).  weight may be NULL.
 * mvp_seg_loss_backward_f32: grad_logit (own strides gld_*) = *grad_out * w[y]/acc[1] * (softmax - onehot), 0 for skipped
 *   points; acc as left by the forward, grad_out = 1 float on the device.
 * mvp_seg_confusion_f32: mat (C,C) int64 += 1 at [label][argmax_c logit] (first maximum), i.e. the argmax + mask +
 *   bincount of mvpnet/models/metric.py:13-24,38-53 in one pass; accumulated into (the caller zeroes / keeps a running matrix). */
int mvp_seg_loss_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                     const int64_t* label, const float* weight, int64_t ignore_index, double* acc, float* loss, mvp_stream_t stream);
int mvp_seg_loss_backward_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                              const int64_t* label, const float* weight, int64_t ignore_index, const double* acc,
                              const float* grad_out, float* grad_logit, int64_t gld_b, int64_t gld_c, int64_t gld_n,
                              mvp_stream_t stream);
int mvp_seg_confusion_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                          const int64_t* label, int64_t ignore_index, int64_t* mat, mvp_stream_t stream);
/* mvp_seg_loss_meter_f32: mvp_seg_loss_f32 and the meters of a training iteration (mvpnet/train_mvpnet_3d.py:170-173: SegAccuracy,
 *   SegIoU, the loss meter) in ONE launch, with the meter state resident on the device.  logit .. loss: as mvp_seg_loss_f32 -- the same
 *   row arithmetic and workgroup partition, acc[0..2] and *loss are what that entry point leaves (mvp_seg_loss_backward_f32 takes the acc);
 *   acc == NULL && loss == NULL is the meters-only form (no loss is formed; the loss slots below get a NaN); exactly one of the two NULL:
 *   MVP_ENULL.  The state is owned by the caller and ZEROED once (construction / reset), never per call; W = window, 1 <= W <= 64:
 *     meter_i64, MVP_SEG_METER_I64(C, W) int64: [0] u, the number of updates; [1] correct, [2] valid: cumulative counts of the valid points
 *       (argmax == label / all); [3] the launch's ticket, back at 0 when the launch ends; [4 + 2 s], [5 + 2 s], s = 0 .. W: a ring of the
 *       (correct, valid) pairs as they stood after update s (mod W + 1) -- slot 0 is the zero state before the first update --, so the
 *       counts of the last k = min(u, W) updates are cumulative - ring[(u - k) % (W + 1)], in exact integers; then the running (C,C)
 *       matrix mat[label][argmax] (first maximum, as mvp_seg_confusion_f32).
 *     meter_f64, MVP_SEG_METER_F64(W) float64: [0] the sum of the per-update losses (added in update order); [1 + j % W]: the float32 loss
 *       of update j, the last W of them.
 *   The LAST workgroup of the launch takes the cumulative pair, increments u and writes the two ring slots: the cursor lives on the
 *   device, so every launch has the same arguments and may sit in a captured graph.  Launches that share a state must be ordered (one
 *   stream).  Errors: a NULL pointer (weight excepted) is MVP_ENULL ahead of any other error; window or sizes out of range MVP_EINVAL. */
#define MVP_SEG_METER_MAX_WINDOW 64
#define MVP_SEG_METER_I64(C, W) (4 + 2 * ((W) + 1) + (C) * (C))
#define MVP_SEG_METER_F64(W) (1 + (W))
int mvp_seg_loss_meter_f32(const float* logit, int64_t B, int64_t C, int64_t N, int64_t ld_b, int64_t ld_c, int64_t ld_n,
                           const int64_t* label, const float* weight, int64_t ignore_index, double* acc, float* loss,
                           int64_t* meter_i64, double* meter_f64, int64_t window, mvp_stream_t stream);

/* ---- scene results: the model ensemble and the evaluator's confusion matrix (NEW on the device) ----
 * mvp_ensemble_softmax_f32: mvpnet/ensemble.py:45-49 -- `sum_m scipy.special.softmax(logit_m, axis=1)`, then argmax -- in ONE launch.
 *   logits: a HOST array of M device pointers, 1 <= M <= MVP_ENSEMBLE_MAX_MODELS (handed to the kernel by value: no pointer table on the
 *   device, no stacked copy); model m's element (r,c) is at logits[m][r*ld_r + c*ld_c], the strides common to all models: (n,C) rows,
 *   the transposed view of a (C,n) network output and rows with a padded stride go in as they lie.  1 <= C <= 64, n < 2^31.
 *   prob (n,C) float32, contiguous, or NULL; label (n,) int64.
 * Definition (pinned).  All arithmetic in float32, every operation rounded once, never contracted; per row:
 *     per model m:   mx = max_c x_c                         (NaN-propagating, as numpy.max)
 *                    e_c = expf(x_c - mx)                   (the accurate library expf, no fast intrinsic)
 *                    s = ((e_0 + e_1) + ...) + e_{C-1}      in class order
 *                    p_c = e_c / s                          an IEEE division
 *     over models:   P_c = ((p0_c + p1_c) + ...)            in model order;   prob[r,c] = P_c
 *     label[r] = the first maximum of P: by strict `>` from P_0.
 *   A NaN anywhere in a model's row makes mx, hence every e_c, s and p_c of that model NaN: the whole P row is NaN and the label is 0
 *   (numpy.argmax's answer for an all-NaN row).  An infinite logit gives what the expression gives (+inf: inf - inf = NaN, the row as
 *   above; a row of -inf likewise).  No fault and no hang for any input; no atomics, the same bits every run.
 *   Rows are read with 16-byte loads when ld_c == 1, C % 4 == 0, ld_r % 4 == 0 and every pointer (prob included) is 16-byte aligned,
 *   one dword per element otherwise.
 * Before any launch: MVP_ENULL (logits, one of its first M entries, label), MVP_EINVAL unless M, C >= 1 and n, ld_r, ld_c >= 0,
 * MVP_EUNSUPPORTED for M > MVP_ENSEMBLE_MAX_MODELS, C > 64 or n >= 2^31.  n == 0: nothing is launched.
 *
 * mvp_label_confusion_i64: evaluate_3d.py:25-40 -- sklearn's confusion_matrix(gt, pred, labels=...) added to a running matrix.
 *   pred, gt (n,) int64; pred_lut (Lp,), gt_lut (Lg,) int32 or NULL (with L = 0): value -> position among the evaluator's labels.
 *     position of v: with a table, lut[v] for 0 <= v < L, else -1 (a table entry outside [0,C) is -1 as well);
 *                    without one, v for 0 <= v < C, else -1.
 *   mat (C,C) int64 += 1 at [position(gt)][position(pred)] where both are >= 0: ignored ground truth (-100), raw ids that are no
 *   evaluation class and the "no prediction" label drop out.  Integer sums (a per-workgroup histogram for C <= 64, global atomics
 *   beyond): the same bits every run.
 * Before any launch: MVP_ENULL (pred, gt, mat), MVP_EINVAL unless n >= 0, C >= 1 and each table comes with its length (NULL <=> 0),
 * MVP_EUNSUPPORTED for C > MVP_CONFUSION_MAX_CLASSES.  n == 0: nothing is launched. */
#define MVP_ENSEMBLE_MAX_MODELS 8
#define MVP_CONFUSION_MAX_CLASSES 32768
int mvp_ensemble_softmax_f32(const float* const* logits, int64_t M, int64_t n, int64_t C, int64_t ld_r, int64_t ld_c, float* prob,
                             int64_t* label, mvp_stream_t stream);
int mvp_label_confusion_i64(const int64_t* pred, const int64_t* gt, int64_t n, int64_t C, const int32_t* pred_lut, int64_t Lp,
                            const int32_t* gt_lut, int64_t Lg, int64_t* mat, mvp_stream_t stream);

/* ---- stage one: test, validation and class weights from the frame store (NEW on the device) ----
 * mvpnet/test_2d.py:103-118 and the validation pass of mvpnet/train_2d.py:240-312 (argmax of the 2D network's logits against the label
 * frames), mvpnet/data/preprocess/compute_label_weights.py (np.bincount of the labels): raw 16-bit label frames through Pillow's
 * NEAREST indices and the label mapping into integer counts, without the (Nf,h,w) int64 label tensor of mvp_prepare_labels_u16.
 *
 * The label arguments mean what they mean for mvp_prepare_labels_u16 (no flip): labels (Ftot,H,W) uint16; picked (Nf,) int64 global rows,
 * clamped into [0, Ftot); yi (h) / xi (w) int32 ON THE DEVICE (mvp_resize_nearest_table), clamped into the image, NULL exactly when that
 * axis keeps its size; mapping (T,) int64 on the device or NULL:
 *     raw = labels[picked[f], yi[y], xi[x]];   label = mapping ? (raw < T ? mapping[raw] : ignore_value) : raw
 *
 * mvp_frame_confusion_f32: logit covers (Nf,C,h,w) float32, element (f,c,y,x) at logit[f*ld_f + c*ld_c + y*ld_y + x*ld_x] -- contiguous
 *   NCHW, channels-last memory and a view with a padded ld_f go in as they lie.
 *     am = the first maximum of the pixel's C logits: by strict `>` from class 0, as mvp_seg_confusion_f32 and torch.argmax.  NaN logits
 *          are outside the contract (a NaN never wins a `>`: no fault, but not torch's answer).
 *     mat (C,C) int64 += 1 at [label][am] for every pixel whose label lies in [0,C);
 *     pred (Nf,h,w) int64 or NULL: am of EVERY pixel, ignored ones included.
 *   labels and mat may both be NULL (an unlabelled split): then pred is required and only it is written; the label arguments are still
 *   checked (pass H = h, W = w, Ftot = 1 and no tables), picked is not read.
 *   One launch (per 65535 frames), one lane per output pixel, a 64-bit frame base and 32-bit offsets inside a frame; a pixel's logits
 *   are read whether its label counts or not.  With ld_x == 1 the per-channel loads of a wave are contiguous; with ld_c == 1, C % 4 == 0, C <= 32 and 16-byte
 *   aligned rows a lane reads its row in 16-byte loads.  A workgroup-private LDS histogram for C * C <= 4096 flushed with 64-bit integer atomics,
 *   global integer atomics beyond: integer sums only, the same bits every run.  No allocation, no synchronisation (graph-capturable).
 *   Before any launch: MVP_ENULL (logit; picked when labels and mat are given; pred when they are not); MVP_EINVAL for a size < 1 (Ftot, H,
 *   W, h, w, C), Nf < 1, T < 0, a NULL table for a changed axis or a table for an unchanged one, labels without mat or mat without labels;
 *   MVP_EUNSUPPORTED for C >= 2^16, H*W or h*w >= 2^31, or a logit frame whose extent (C-1)*ld_c + (h-1)*ld_y + (w-1)*ld_x reaches 2^30
 *   elements (offsets inside a frame are 32-bit byte offsets); MVP_EINVAL for a negative stride.
 *
 * mvp_label_histogram_u16: hist (nbins,) int64 += 1 per pixel of the picked, resized frames whose label -- the mapped value, or the raw id
 *   without a mapping; a raw id >= T counts nowhere -- lies in [0,nbins).  One launch (per 65535 frames), no label tensor.  An LDS histogram for
 *   nbins <= 4096 (the 20 and 41 bins of the class weights), global integer atomics up to nbins = MVP_HISTOGRAM_MAX_BINS = 65536 (every raw
 *   id).  MVP_ENULL (labels, picked, hist); MVP_EINVAL as above and for nbins < 1; MVP_EUNSUPPORTED for nbins > MVP_HISTOGRAM_MAX_BINS,
 *   H*W or h*w >= 2^31.
 * mvp_label_histogram_i64: label (n,) int64; hist (nbins,) int64 += 1 per value in [0,nbins): np.bincount(label, minlength) accumulated
 *   (compute_3d_weights), negative and too large values dropped.  MVP_ENULL (label, hist); MVP_EINVAL unless n >= 0 and nbins >= 1;
 *   MVP_EUNSUPPORTED for nbins > MVP_HISTOGRAM_MAX_BINS or n >= 2^40.  n == 0: nothing is launched. */
#define MVP_HISTOGRAM_MAX_BINS 65536
int mvp_frame_confusion_f32(const float* logit, int64_t Nf, int64_t C, int64_t h, int64_t w, int64_t ld_f, int64_t ld_c, int64_t ld_y,
                            int64_t ld_x, const uint16_t* labels, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, const int32_t* yi,
                            const int32_t* xi, const int64_t* mapping, int64_t T, int64_t ignore_value, int64_t* mat, int64_t* pred,
                            mvp_stream_t stream);
int mvp_label_histogram_u16(const uint16_t* labels, int64_t Ftot, int64_t H, int64_t W, const int64_t* picked, int64_t Nf, int64_t h,
                            int64_t w, const int32_t* yi, const int32_t* xi, const int64_t* mapping, int64_t T, int64_t nbins, int64_t* hist,
                            mvp_stream_t stream);
int mvp_label_histogram_i64(const int64_t* label, int64_t n, int64_t nbins, int64_t* hist, mvp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVP_HIP_H_ */
