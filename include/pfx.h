/* =====================================================================================
 * pfx.h -- C-ABI of the MI355X-native (gfx950) feature-extraction path.
 *
 * This is the drop-in boundary that replaces the PCL 1.7 calls srv/pcl_feature_extraction
 * makes on its hot path.  Plain pointers and sizes, no torch or PCL
 * types.  Every entry point returns 0 on success; on failure a nonzero pfx_status and the
 * message is available from pfx_last_error(ctx).  PCL's own error behaviour (initCompute
 * failure -> PCL_ERROR + empty output; per-point failure -> NaN fill) is mapped by the C++
 * facade (include/pfx_pcl.hpp) onto these codes.
 *
 * Two families:
 *   pfx_*      host pointers in / host pointers out (synchronous, H2D/D2H inside)
 *   pfx_*_dev  device pointers in / device pointers out, stream-ordered on the ctx stream
 * Arrays are structure-of-arrays float32 (x, y, z / nx, ny, nz), indexed by the caller's
 * point index, exactly the order of PointCloud<T>::points.
 *
 * Replaced reference interfaces (file:line in /root/reference):
 *   pfx_normals*        <- Tools::estimateNormals -> NormalEstimationOMP<PointXYZRGB,Normal>
 *                          ::compute  (include/pcl_feature_extraction/tools.h:22-32)
 *   pfx_fpfh*           <- FPFHEstimation<PointXYZRGB,Normal,FPFHSignature33>::compute via
 *                          Features<T>::compute (features.h:175-196, evaluation.cpp:593-612)
 *   pfx_shot*           <- SHOTEstimationOMP<PointXYZRGB,Normal,SHOT352>::compute
 *                          (features.h:175-196, evaluation.cpp:766-785)
 *   pfx_shot_color*     <- SHOTColorEstimationOMP<PointXYZRGB,Normal,SHOT1344>::compute
 *                          (features.h:175-196, evaluation.cpp:786-805)
 *   pfx_pfh*            <- PFHEstimation<PointXYZRGB,Normal,PFHSignature125>::compute
 *                          (features.h:175-196, evaluation.cpp:676-695)
 *   pfx_spin_image*     <- SpinImageEstimation<PointXYZRGB,Normal,Histogram<153>>::compute
 *                          (evaluation.cpp:514-553)
 *   pfx_intensity_gradient* <- IntensityGradientEstimation<PointXYZI,Normal,IntensityGradient,
 *                          IntensityFieldAccessor<PointXYZI>>::compute (evaluation.cpp:416-465;
 *                          Tools::computeGradient, tools.h:40-54)
 *   pfx_rift*           <- RIFTEstimation<PointXYZI,IntensityGradient,Histogram<32>>::compute
 *                          (evaluation.cpp:716-765)
 *   pfx_intensity_spin* <- IntensitySpinEstimation<PointXYZI,Histogram<20>>::compute
 *                          (evaluation.cpp:466-514)
 *   pfx_shape_context*  <- ShapeContext3DEstimation<PointXYZRGB,Normal,ShapeContext1980>::compute
 *                          (features.h:175-196, evaluation.cpp:319-345)
 *   pfx_usc*            <- UniqueShapeContext<PointXYZRGB,ShapeContext1980>::compute
 *                          (evaluation.cpp:346-371); pfx_shot_lrf* its frames
 *   pfx_moment_invariants* <- MomentInvariantsEstimation<PointXYZRGB,MomentInvariants>::compute
 *                          (features.h:175-196, evaluation.cpp:554-572)
 *   pfx_principal_curvatures* <- PrincipalCurvaturesEstimation<PointXYZRGB,Normal,
 *                          PrincipalCurvatures>::compute (features.h:175-196, evaluation.cpp:696-715)
 *   pfx_board_lrf*      <- BOARDLocalReferenceFrameEstimation<PointXYZRGB,Normal,ReferenceFrame>
 *                          ::compute (features.h:175-196, evaluation.cpp:372-393)
 *   pfx_boundary*       <- BoundaryEstimation<PointXYZRGB,Normal,Boundary>::compute
 *                          (features.h:175-196, evaluation.cpp:394-415)
 *   pfx_cvfh*           <- CVFHEstimation<PointXYZRGB,Normal,VFHSignature308>::compute through the
 *                          Feature base pointer (features.h:175-196, evaluation.cpp:649-675)
 *   pfx_smooth_clusters* <- extractEuclideanClustersSmooth, CVFH's clustering stage
 *   pfx_range_image_planar* <- RangeImagePlanar::createFromPointCloudWithFixedSize
 *                          (keypoints.h:212-216, tools.h:61-77)
 *   pfx_narf_keypoints* <- RangeImageBorderExtractor + NarfKeypoint::compute
 *                          (keypoints.h:219-224)
 *   pfx_narf_descriptors* <- NarfDescriptor::compute (evaluation.cpp:613-648)
 *   pfx_point_indices*  <- Tools::getIndices (tools.h:91-102)
 *   pfx_radius_search*  <- search::KdTree<PointXYZRGB>::radiusSearch (features.h:192,
 *                          tools.h:29; FLANN order: (d^2, index) ascending, strict d^2 < r^2)
 *   pfx_knn_search*     <- KdTreeFLANN<PointXYZRGB>::nearestKSearch (FLANN's KNNSimpleResultSet: the
 *                          k smallest (d^2, index), self included; exact d^2 ties by index)
 *   pfx_normals_knn*    <- NormalEstimationOMP<PointXYZRGB,Normal>::compute with setKSearch(k)
 *   pfx_nearest_descriptors_dev <- Features<T>::getCorrespondences (features.h:255-273):
 *                          KdTreeFLANN<FeatureT>::nearestKSearch(k = 1) per descriptor
 *   pfx_correspondences* <- Features<T>::findCorrespondences (features.h:224-253)
 *   pfx_pcd_*           <- pcl::io::loadPCDFile<PointXYZRGB> (evaluation.cpp:226-235)
 *   pfx_cloud_resolution* <- Keypoints::computeCloudResolution (keypoints.h:401-428)
 *   pfx_iss_keypoints*  <- ISSKeypoint3D<PointXYZRGB,PointXYZRGB>::compute as configured by
 *                          Keypoints::compute's ISS branch (keypoints.h:177-189)
 *   pfx_uniform_sampling* <- UniformSampling<PointXYZRGB>::compute as Keypoints::compute's
 *                          UNIFORM_SAMPLING branch configures it (keypoints.h:274-290)
 *   pfx_harris3d_keypoints* <- HarrisKeypoint3D<PointXYZRGB,PointXYZI>::compute + getKeypointsCloud
 *   pfx_harris6d_keypoints* <- HarrisKeypoint6D<PointXYZRGB,PointXYZI>::compute + getKeypointsCloud
 *                          (Keypoints::compute's HARRIS_3D branch, keypoints.h:150-162, 365-395)
 *   pfx_ransac_rejector <- registration::CorrespondenceRejectorSampleConsensus<PointXYZRGB> in
 *                          Features<T>::filterCorrespondences (features.h:282-297)
 *   pfx_icp*            <- IterativeClosestPoint<PointXYZRGB,PointXYZRGB>::align in icpAlign
 *                          (evaluation.cpp:863-885)
 * ===================================================================================== */
#ifndef PFX_H_
#define PFX_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pfx_ctx pfx_ctx;
typedef int32_t pfx_status;

enum {
  PFX_OK = 0,
  PFX_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, radius <= 0, ...) */
  PFX_ERR_DEVICE = 2,      /* HIP runtime error (message from hipGetErrorString)            */
  PFX_ERR_CAPACITY = 3,    /* caller buffer too small (required size in the out count)      */
  PFX_ERR_UNSUPPORTED = 4  /* parameter combination the path does not implement             */
};

/* NarfKeypoint::Parameters + RangeImageBorderExtractor::Parameters (PCL 1.7 defaults; the
 * reference sets only support_size = 0.2f, keypoints.h:223). */
typedef struct pfx_narf_params {
  float support_size;                            /* -1 (must be set > 0)   */
  int32_t max_no_of_interest_points;             /* -1 = unlimited          */
  float min_distance_between_interest_points;    /* 0.25 (x support_size)   */
  float optimal_distance_to_high_surface_change; /* 0.25                    */
  float min_interest_value;                      /* 0.45                    */
  float min_surface_change_score;                /* 0.2                     */
  /* 1.  The greedy selection then orders the survivors with std::sort on strength, as PCL does:
   * the order of EQUAL strengths is the sort implementation's (the libstdc++ this library is
   * built with; PCL's was an Indigo-era GCC).  It decides the keypoints only when two tied
   * survivors lie closer than min_distance_between_interest_points * support_size:
   * scripts/narf_tie_report.py finds none on the reference's four clouds (their keypoints are
   * independent of the toolchain: tests/test_oracle_narf_ties.py) and 6-11 such pairs on each
   * configs[2] synthetic room, where 4-7 of ~85 keypoints move between the two extreme tie
   * orders (profiles/r05_narf_tie_report.jsonl).  The GPU path and the oracle share this
   * build's order. */
  int32_t do_non_maximum_suppression;
  /* 1 (PCL's default).  Either value computes NarfKeypoint's COMPLETE interest formula
   * (calculateCompleteInterestImage); 1 only skips pixels that provably cannot reach
   * min_interest_value, so 0 and 1 give the same keypoints.  PCL 1.7's own sparse heuristics
   * (calculateSparseInterestImage, source absent here) are NOT reproduced: parity with that
   * mode is unpinned, with a measured sensitivity of 1-2 keypoints per reference cloud
   * (DESIGN.md section 5).  pfx_ctx_last_stats(ctx, "narf_interest_formula") = 0 after every
   * NARF call (0 = complete formula). */
  int32_t calculate_sparse_interest_image;
  int32_t no_of_polynomial_approximations_per_point; /* 0 (only 0 supported) */
  int32_t add_points_on_straight_edges;          /* 0 (only 0 supported)    */
  /* RangeImageBorderExtractor::Parameters.  Bounds (PFX_ERR_INVALID beyond them, before anything
   * is launched): pixel_radius_plane_extraction in [0, 4] (at most 4 x 4 neighbours per pixel in the
   * kernel's 25 sorted slots); the other three radii in [0, 1024].  Those three size no array, tile
   * or mask in any kernel -- they are loop bounds, linear (borders, principal curvature) or
   * quadratic (border direction) in run time per pixel -- and 1024 is the widest image accepted.
   * support_size has no fixed upper bound: region-grow windows that outgrow the 128 x 128 masks or
   * the 65,536-pixel bitmap move to the next tier, the last of which holds the whole image.  The
   * two queue-based tiers keep at most 2048 pending pixels, which is one breadth-first level of the
   * region plus the 64-pixel batch in flight.  A level of a filled region is a square ring clipped
   * to the image: at most 8 d pixels at ring radius d and fewer than 4 min(width, height), so
   * 1912 at 640 x 480 and 4 x 119 at 161 x 119 (tests run support 0.1 .. 1.0 there).  A region
   * whose level outgrows the queue -- a whole-image region of a near-square image beyond ~500 px a
   * side, or a contrived many-armed one -- ends the call with PFX_ERR_CAPACITY ("interest
   * region-grow queue overflow"): a checked condition, never a wrong image. */
  int32_t pixel_radius_borders;                  /* 3   */
  int32_t pixel_radius_plane_extraction;         /* 2   */
  int32_t pixel_radius_border_direction;         /* 2   */
  float minimum_border_probability;              /* 0.8 */
  int32_t pixel_radius_principal_curvature;      /* 2   */
} pfx_narf_params;

/* RangeImagePlanar::createFromPointCloudWithFixedSize arguments.  pfx_narf_keypoints* accepts
 * width <= 1024 and width*height <= 307,200 (PFX_ERR_INVALID beyond); noise_level != 0 is
 * PFX_ERR_UNSUPPORTED. */
typedef struct pfx_camera {
  int32_t width, height;          /* 640, 480 (keypoints.h:204)     */
  float center_x, center_y;       /* 320, 240 (keypoints.h:205)     */
  float focal_length_x, focal_length_y; /* 525, 525 (keypoints.h:206, both fx) */
  float sensor_pose[16];          /* row-major 4x4 Affine3f (sensor_origin_ * orientation_) */
  int32_t coordinate_frame;       /* 0 = CAMERA_FRAME, 1 = LASER_FRAME */
  float noise_level;              /* 0 */
  float min_range;                /* 0 */
} pfx_camera;

void pfx_narf_params_default(pfx_narf_params* p);
/* The reference's NARF setup (keypoints.h:203-223) with an identity pose */
void pfx_camera_default(pfx_camera* c);

/* ---- context ---------------------------------------------------------------------- */
pfx_status pfx_ctx_create(int device, pfx_ctx** out);
void pfx_ctx_destroy(pfx_ctx* ctx);
const char* pfx_last_error(const pfx_ctx* ctx);
/* Use an external hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL is HIP's
 * null stream (torch's default stream).  A new ctx runs on its own non-blocking stream, created
 * by the first call that runs on it (a ctx set to an external stream first never creates one). */
pfx_status pfx_ctx_set_stream(pfx_ctx* ctx, void* hip_stream);
/* Back to the ctx-owned non-blocking stream. */
pfx_status pfx_ctx_use_own_stream(pfx_ctx* ctx);
void* pfx_ctx_get_stream(pfx_ctx* ctx);
/* Frees every device scratch buffer of ctx (grids, neighbour lists, the rarely used overflow
 * scratch of the list builder, the FPFH weighting and PFH, NARF images) after synchronising its
 * stream; the next call reallocates what it needs.  Held state (lists kept for
 * pfx_normals_chains_dev / pfx_fpfh_after_normals_dev, prepared FPFH grids) is dropped. */
pfx_status pfx_ctx_trim(pfx_ctx* ctx);
pfx_status pfx_ctx_synchronize(pfx_ctx* ctx);
/* Launch-shape hint, no effect on results: another stream of this process runs latency-critical
 * work on the device at the same time (the overlapped NARF + normal estimation step).
 * NARF's flood fill then runs on 4 instead of 20 waves per CU, so the concurrent grid build
 * and list set-up find free wave slots (1M-pt room: 161.4 -> 162.6 Mpoints/s; alone the
 * interest stage takes 0.63 instead of 0.47 ms, hence off by default). */
pfx_status pfx_ctx_set_shared(pfx_ctx* ctx, int shared);
/* HIP-event timing on the ctx stream (for bench.py's live roofline): enable = 1 times every kernel
 * group, 2 only the stage scopes (one event pair per stage call: "normals", "normals_fast", "iss",
 * "harris3d", ...; the per-kernel pairs cost ~2 % of the headline step in host launch time), 0 off. */
pfx_status pfx_ctx_set_timing(pfx_ctx* ctx, int enable);
pfx_status pfx_ctx_reset_timing(pfx_ctx* ctx);
/* Accumulated device time and launch count of the kernel `name`; syncs the stream. */
pfx_status pfx_ctx_kernel_time(pfx_ctx* ctx, const char* name, double* total_ms,
                               int64_t* launches);
/* Statistics of the last calls on ctx, by name: e.g. "normals_neighbors" (sum over queries of
 * |N_r(q)| of the last normals call -- the per-launch unit count for the neighbour-gather
 * roofline), "narf_keypoints", "narf_interest_formula" (0 = NarfKeypoint's complete formula, the
 * only one implemented; see pfx_narf_params.calculate_sparse_interest_image). */
pfx_status pfx_ctx_last_stats(pfx_ctx* ctx, const char* what, int64_t* value);

/* ---- radius search (FLANN semantics) ---------------------------------------------- */
/* counts[nq] = |{p : d2(q,p) < (float)(r*r)}|; if idx != NULL also the first `cap`
 * neighbours of each query in (d2, index) order, row-major with row stride `cap`. */
pfx_status pfx_radius_search(pfx_ctx* ctx, const float* x, const float* y, const float* z,
                             int64_t n, const float* qx, const float* qy, const float* qz,
                             int64_t nq, double radius, int64_t* counts, int32_t* idx,
                             float* d2, int64_t cap);

/* ---- k-nearest-neighbour search (FLANN semantics; DESIGN.md "k-NN: the contract") ---- */
/* The largest k of pfx_knn_search* and pfx_normals_knn* (a wave keeps a row and one batch of 64
 * candidates in its 4 KB of LDS). */
#define PFX_KNN_MAX_K 256
/* The surface is the finite points of (x, y, z), m of them; a non-finite point is never a
 * neighbour (PCL's kd-tree drops them).  A finite query receives the min(k, m) surface points of
 * smallest key (d2, index) in ascending key order, d2 = ((0 + dx*dx) + dy*dy) + dz*dz in float32,
 * dx = q - p, no FMA (the radius search's d2): counts[q] = min(k, m), idx / d2 rows of stride k, the
 * rest of a row idx = -1 and d2 = NaN.  A query that is a surface point finds itself first (d2 = 0),
 * its duplicates after it in index order.  A non-finite query: counts = 0, the whole row -1 / NaN.
 * Exact float-d2 ties are broken by index, inside a row and for the k-th place; FLANN breaks them by
 * the order its kd-tree visits the leaves (the one departure from PCL; DESIGN.md gives its measured
 * frequency).  The result does not depend on density, extent or launch order.
 *   PFX_ERR_INVALID   k < 1, a negative count, a null pointer where its side has rows;
 *   PFX_ERR_CAPACITY  k > PFX_KNN_MAX_K; 2^28 points or queries and more (the neighbour lists'
 *                     limit).  The outputs are untouched in both cases.
 * n = 0 (every count 0) and nq = 0 succeed.  Host waits: the bounds, then one per grid searched
 * (at most 6).  Statistics: "knn_queries" (nq), "knn_rounds" (grids built), and one per path a query
 * takes: "knn_first" (certified on the first grid), "knn_requeued" (on a later grid of doubled
 * cell), "knn_exhaustive" (by the scan of every point), "knn_skipped" (non-finite); they sum to nq
 * when the surface has a finite point. */
pfx_status pfx_knn_search(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                          const float* qx, const float* qy, const float* qz, int64_t nq, int32_t k,
                          int64_t* counts, int32_t* idx, float* d2);
pfx_status pfx_knn_search_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                              const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq, int32_t k,
                              int64_t* d_counts, int32_t* d_idx, float* d_d2);

/* ---- normals: NormalEstimationOMP (input == surface) ------------------------------- */
pfx_status pfx_normals(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                       double radius, const float viewpoint[3], float* nx, float* ny, float* nz,
                       float* curvature);
pfx_status pfx_normals_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                           int64_t n, double radius, const float viewpoint[3], float* d_nx,
                           float* d_ny, float* d_nz, float* d_curvature);
/* NormalEstimationOMP with setKSearch(k), input == surface: point i takes query i's row of
 * pfx_knn_search (surface = queries = the cloud), and from it the single-pass float covariance in
 * row order, pcl::eigen33, the curvature and the flip towards the viewpoint (NULL: the origin) --
 * pfx_normals' arithmetic.  Fewer than 3 neighbours (so k = 1, k = 2, or a cloud of fewer than 3
 * finite points) and non-finite points give four NaNs, as PCL.  k, its errors and the statistics are
 * pfx_knn_search's. */
pfx_status pfx_normals_knn(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, int32_t k,
                           const float viewpoint[3], float* nx, float* ny, float* nz, float* curvature);
pfx_status pfx_normals_knn_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                               int32_t k, const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                               float* d_curvature);
/* The same computation in two phases, so that a caller can order the points it needs first
 * (results identical to pfx_normals_dev):
 *   lists  -- radius-neighbour lists of every finite point, kept in ctx; outputs NaN-filled;
 *   chains -- the normals of the points with (d_mask[i] != 0) == want (all when d_mask is
 *             null), on ctx's stream, from the lists held by `lists_ctx` (ctx itself or another
 *             context on the same device whose lists phase is ordered before this call).  Two
 *             chains calls with complementary masks may run concurrently on two contexts.
 *             want = 3 / 2: workgroup partition -- every point of a block of 256 consecutive
 *             (cell-ordered) queries that holds any masked point / holds none, so the two passes
 *             stage each block's candidates once between them (the masked points are a subset
 *             of pass 3's). */
pfx_status pfx_normals_lists_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                 int64_t n, double radius, float* d_nx, float* d_ny, float* d_nz,
                                 float* d_curvature);
pfx_status pfx_normals_chains_dev(pfx_ctx* ctx, pfx_ctx* lists_ctx, const uint8_t* d_mask, int32_t want,
                                  const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                                  float* d_curvature);

/* pfx_normals_dev split at its one host round trip, so a consumer (FPFH) can be queued on another
 * stream right behind the estimation: _launch queues grid, lists and chains with no host wait
 * (the chains compute nothing unless the lists turn out whole); _finish validates them (host
 * wait on ctx's stream) and, rarely -- a scan outside the previous scan's widened bounds, a list
 * buffer to grow, the first very long lists -- reruns the exact path, stream-ordered on ctx's
 * stream, and sets *rerun = 1: whatever read the outputs in between must then run again.
 * Results after _finish are pfx_normals_dev's, bit for bit. */
pfx_status pfx_normals_launch_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                  int64_t n, double radius, const float viewpoint[3], float* d_nx,
                                  float* d_ny, float* d_nz, float* d_curvature);
pfx_status pfx_normals_finish_dev(pfx_ctx* ctx, int32_t* rerun);

/* Scheduling hint (no reference counterpart): the next pfx_normals_launch_dev / pfx_normals_dev on
 * ctx makes its stream wait for hip_event (a hipEvent_t already recorded by the caller) after its
 * grid build and list set-up and before its neighbour-list kernels, once.  The list kernels are
 * persistent and fill the device; a short stage on another stream that must not queue behind
 * them (FPFH's surface grid, which NARF's chain then follows) is kept ahead this way.  NULL
 * clears it. */
pfx_status pfx_normals_gate_dev(pfx_ctx* ctx, void* hip_event);
/* Scheduling aid: queue the (speculative) grid of the next pfx_normals_launch_dev /
 * pfx_normals_dev on the same d_x, d_y, d_z, n and radius now, so the caller can issue it before another
 * stream's work (and that work's gate, pfx_normals_gate_dev) and the estimation's lists after.
 * Results are unchanged; any other call in between on ctx discards it. */
pfx_status pfx_normals_grid_launch_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                       int64_t n, double radius);

/* NormalEstimationOMP (tools.h:22-32) over a subset of the cloud: the points with
 * (d_mask[i] != 0) == want get PCL's normal and curvature bit for bit (their neighbours are
 * searched in the whole cloud); every other output entry is left untouched.  Two calls, want = 1
 * then 0, give pfx_normals_dev's result.  Use: FPFH's support (pfx_fpfh_support_ball_dev) first,
 * so FPFHEstimation starts on another stream while the rest is estimated -- the normals are
 * Features::compute's intermediate (features.h:185-187), FPFH reads only the support's.
 * pfx_normals_prepare_dev builds the cloud's grid ahead (coordinates only), e.g. while the mask
 * is still being computed; pfx_normals_subset_dev builds it itself otherwise. */
pfx_status pfx_normals_prepare_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                   int64_t n, double radius);
pfx_status pfx_normals_subset_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                  int64_t n, double radius, const uint8_t* d_mask, int32_t want,
                                  const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                                  float* d_curvature);

/* Opt-in fast mode, NOT parity-exact (BASELINE north_star "MFMA for the 3x3
 * covariance accumulation"): the same neighbour set (FLANN's d2 < (float)(r*r)), but the
 * covariance sums are one MFMA contraction per 16 points -- hit mask x candidate features,
 * centred on the group's first point -- instead of PCL's sequential float chains in FLANN order,
 * so no neighbour list is sorted or stored.  Results differ from pfx_normals by rounding (the
 * sums carry less rounding than PCL's raw-coordinate ones); bench.py --workload fastnormals
 * reports the deviation.  Same NaN rules (< 3 neighbours, non-finite points). */
pfx_status pfx_normals_fast(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                            double radius, const float viewpoint[3], float* nx, float* ny, float* nz,
                            float* curvature);
pfx_status pfx_normals_fast_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                int64_t n, double radius, const float viewpoint[3], float* d_nx,
                                float* d_ny, float* d_nz, float* d_curvature);

/* ---- FPFH-33: FPFHEstimation (surface + normals, queries = input cloud) ------------- */
/* same_as_surface != 0 selects PCL's "input_ == surface_ && indices == all" branch (queries
 * must then be the surface itself).  out: nq x 33 row-major (FPFHSignature33::histogram).
 * A null surface or normal array with n_surface > 0, or a null query array with nq > 0 and
 * same_as_surface == 0, is PFX_ERR_INVALID ("fpfh: invalid arguments") before any copy. */
pfx_status pfx_fpfh(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                    const float* snx, const float* sny, const float* snz, int64_t n_surface,
                    const float* qx, const float* qy, const float* qz, int64_t nq,
                    int same_as_surface, double radius, float* out);
/* _dev: stream-ordered, no host synchronisation; its statistics (pfx_ctx_last_stats) and a
 * neighbourhood beyond the 2^22 capacity (PFX_ERR_CAPACITY) are reported by the next
 * pfx_ctx_synchronize / pfx_ctx_last_stats on this ctx.
 * pfx_fpfh_dev never reuses state of an earlier normal estimation: it builds its own lists. */
pfx_status pfx_fpfh_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                        const float* d_snx, const float* d_sny, const float* d_snz,
                        int64_t n_surface, const float* d_qx, const float* d_qy,
                        const float* d_qz, int64_t nq, int same_as_surface, double radius,
                        float* d_out);
/* Features::compute's sequence (features.h:187-195): pfx_fpfh_dev right after a
 * pfx_normals_dev / pfx_normals_lists_dev on this ctx over the same device cloud.  The caller
 * vouches that (d_sx, d_sy, d_sz) still hold the cloud that normal estimation ran on; with
 * same_as_surface, equal pointers, n_surface and radius, its FLANN-ordered neighbour lists are
 * then reused for the weighting (else they are built as in pfx_fpfh_dev).  Either way the
 * held lists are released, so a second call cannot reuse them. */
pfx_status pfx_fpfh_after_normals_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                      const float* d_snx, const float* d_sny, const float* d_snz,
                                      int64_t n_surface, const float* d_qx, const float* d_qy,
                                      const float* d_qz, int64_t nq, int same_as_surface, double radius,
                                      float* d_out);

/* Builds the search-surface index of the next pfx_fpfh_dev call on this ctx ahead of time (the
 * surface grid needs only the coordinates, so it can overlap normal estimation -- PCL builds the
 * same tree inside FPFHEstimation::compute, features.h:192-195).  The next pfx_fpfh_dev with the
 * same (d_sx, n_surface, radius) consumes it; the surface must not change in between. */
pfx_status pfx_fpfh_prepare_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                int64_t n_surface, double radius);
/* Also marks the SPFH point set S of the next pfx_fpfh_dev (input != surface) for these queries
 * (d_qx must be the same pointer, nq the same count): S needs only the coordinates, so it can be
 * found while the normals are still being computed.  Builds the surface grid first if needed.
 * For up to 512 queries it also gathers and sorts every query's neighbours (the keypoint
 * weighting's keys, 64 KiB of scratch per query), which that pfx_fpfh_dev then takes as they are;
 * the query coordinates must not change in between. */
pfx_status pfx_fpfh_prepare_queries_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                        int64_t n_surface, const float* d_qx, const float* d_qy,
                                        const float* d_qz, int64_t nq, double radius);
/* d_mask[i] = 1 for every surface point whose normal FPFHEstimation reads for these queries
 * (the r-neighbours of the SPFH set S = the r-neighbourhoods of the queries, fpfh.hpp), else 0.
 * n_surface bytes.  The next pfx_fpfh_dev on ctx reads only these normals, so the others may
 * still be computed concurrently (pfx_normals_chains_dev with want = 0 on another stream). */
pfx_status pfx_fpfh_support_mask_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                     int64_t n_surface, const float* d_qx, const float* d_qy,
                                     const float* d_qz, int64_t nq, double radius, uint8_t* d_mask);

/* Conservative form of pfx_fpfh_support_mask_dev: d_mask[i] = 1 for every surface point within
 * 2 * radius of a query (a superset of the normals FPFHEstimation reads, marked in one pass over
 * the queries' 5x5x5 cell blocks instead of one per SPFH point).  Same contract for the next
 * pfx_fpfh_dev on ctx. */
pfx_status pfx_fpfh_support_ball_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                     int64_t n_surface, const float* d_qx, const float* d_qy,
                                     const float* d_qz, int64_t nq, double radius, uint8_t* d_mask);

/* ---- SHOT-352: SHOTEstimationOMP + SHOTLocalReferenceFrameEstimation ---------------- */
/* desc: nq x 352, rf: nq x 9 (x_axis, y_axis, z_axis) -- SHOT352::{descriptor, rf}.
 * A null surface or normal array with n_surface > 0, or a null query array with nq > 0, is
 * PFX_ERR_INVALID ("shot: invalid arguments") before any copy or launch, in both forms.
 * Statistics of the last call: "shot_neighbors" (sum of the neighbourhood sizes), "shot_queued"
 * (queries with more than 2048 neighbours, which the split kernels pass on to the one-workgroup
 * kernel). */
pfx_status pfx_shot(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                    const float* snx, const float* sny, const float* snz, int64_t n_surface,
                    const float* qx, const float* qy, const float* qz, int64_t nq,
                    double radius, float* desc, float* rf);
pfx_status pfx_shot_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                        const float* d_snx, const float* d_sny, const float* d_snz,
                        int64_t n_surface, const float* d_qx, const float* d_qy,
                        const float* d_qz, int64_t nq, double radius, float* d_desc,
                        float* d_rf);

/* ---- SHOT-1344: SHOTColorEstimationOMP (evaluation.cpp:786-805) ----------------------- */
/* The shape and colour descriptor (describe_shape and describe_color both on, PCL's defaults).
 * srgb / qrgb: one packed 0x00RRGGBB word per surface point / per query (PointXYZRGB::rgba; only
 * the low 24 bits are read).  The reference colour of a query is qrgb's, as PCL takes it from the
 * input cloud, not from the surface.  desc: nq x 1344 -- desc[v * 11 + s] is shape volume v
 * (0..31), slot s (0..10); desc[352 + v * 31 + s] is colour slot s (0..30) of volume v.  rf:
 * nq x 9, equal to pfx_shot's bit for bit; neighbours, frame and NaN rows follow pfx_shot's rules,
 * and so does the capacity (more than 16384 neighbours: PFX_ERR_CAPACITY).  radius <= 0 or a null
 * pointer: PFX_ERR_INVALID.  RGB2CIELAB reads its sXYZ table one past the end for pure white in
 * PCL; here that index is clamped to the last entry.  Statistics of the last call:
 * "shot_color_neighbors" (sum of the neighbourhood sizes), "shot_color_lut_clamped" (surface
 * points plus queries whose table index was clamped); "shot_color_cap_small" (the longest list of
 * the split kernels; longer ones take the one-workgroup path) can be read from a new ctx. */
pfx_status pfx_shot_color(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                          const float* snx, const float* sny, const float* snz, const uint32_t* srgb,
                          int64_t n_surface, const float* qx, const float* qy, const float* qz,
                          const uint32_t* qrgb, int64_t nq, double radius, float* desc, float* rf);
/* Device pointers, stream-ordered on the ctx stream like pfx_shot_dev (one host wait at the end,
 * for the capacity check and the statistics). */
pfx_status pfx_shot_color_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                              const float* d_snx, const float* d_sny, const float* d_snz,
                              const uint32_t* d_srgb, int64_t n_surface, const float* d_qx,
                              const float* d_qy, const float* d_qz, const uint32_t* d_qrgb, int64_t nq,
                              double radius, float* d_desc, float* d_rf);

/* ---- PFH-125: PFHEstimation (surface + normals, queries = input cloud) ---------------- */
/* out: nq x 125 row-major (PFHSignature125::histogram): every pair of a query's radius
 * neighbourhood binned 5 x 5 x 5, each hit adding 100 / (k (k - 1) / 2); a non-finite query or
 * an empty neighbourhood gives a NaN row.  PFH has no input == surface branch, so there is no
 * same_as_surface flag; the feature cache (use_cache_) and k-NN search are not supported. */
pfx_status pfx_pfh(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                   const float* snx, const float* sny, const float* snz, int64_t n_surface,
                   const float* qx, const float* qy, const float* qz, int64_t nq,
                   double radius, float* out);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation.  A query with more
 * than 65535 neighbours (its pair count no longer fits 32 bits) gets a NaN row and
 * PFX_ERR_CAPACITY from the next pfx_ctx_synchronize / pfx_ctx_last_stats on ctx.  Statistics of
 * the last call: "pfh_pairs" (sum over the queries of k (k - 1) / 2), "pfh_kmax", "pfh_global"
 * (queries whose neighbourhood exceeded "pfh_cap_lds", the LDS staging capacity, and took the
 * global-scratch pass; "pfh_cap_lds" itself can be read from a new ctx). */
pfx_status pfx_pfh_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                       const float* d_snx, const float* d_sny, const float* d_snz,
                       int64_t n_surface, const float* d_qx, const float* d_qy,
                       const float* d_qz, int64_t nq, double radius, float* d_out);

/* ---- spin images: SpinImageEstimation (evaluation.cpp:514-553) ------------------------ */
/* image_width W in [1, 16] (PCL's default 8: Histogram<153> = (W + 1)(2W + 1));
 * support_angle_cos in [0, 1]; min_pts_neighb >= 0; radial / angular: only 0 is supported
 * (anything else: PFX_ERR_UNSUPPORTED).  pfx_spin_params_default fills 8, 0.0, 0, 0, 0. */
typedef struct pfx_spin_params {
  int32_t image_width;
  double support_angle_cos;
  int32_t min_pts_neighb;
  int32_t radial, angular;
} pfx_spin_params;
void pfx_spin_params_default(pfx_spin_params* p);
/* out: nq x S floats, S = (W + 1)(2W + 1); out[alpha_bin (2W + 1) + beta_bin], alpha_bin in [0, W]
 * the distance from the axis, beta_bin in [0, 2W] the signed height along it, both in bins of
 * radius / W / sqrt(2).  The rotation axis of query i is (qnx, qny, qnz)[i]: the normal of the
 * *input* cloud at that point, as PCL takes it, not the surface's.  Every radius neighbour, in
 * FLANN order, adds four bilinear weights to a double matrix; with more than one neighbour the
 * matrix is scaled by 1 / its sum (Eigen 3.2's summation order), then cast to float.  A NaN axis
 * makes every cosine exactly 1.0, as libstdc++'s min / max do in PCL's clamp: such a row is finite
 * and has mass in alpha_bin 0 only.  k <= 1 (a non-finite query has k = 0): a zero row; k > 1 with
 * nothing contributing: a NaN row (0 x inf).  snx / sny / snz (the surface normals) are read only
 * when support_angle_cos > 0 and may be null otherwise: a neighbour whose |cos| between the axis
 * and its normal is below support_angle_cos is skipped; counter-directed normals are kept.
 * Null pointers other than the optional ones, radius <= 0, W outside [1, 16], support_angle_cos
 * outside [0, 1] or NaN, or support_angle_cos > 0 without surface normals: PFX_ERR_INVALID before
 * any launch.  Where PCL throws -- fewer than min_pts_neighb neighbours, or a cosine beyond
 * 1 + 10 FLT_EPSILON in magnitude (an axis or normal not of unit length) -- the call returns
 * PFX_ERR_INVALID after the kernel, pfx_last_error names the first offending query row and the
 * rule, the outputs are unspecified and the next call is unaffected.  More than 16384 neighbours:
 * PFX_ERR_CAPACITY.  raw (nullable): nq x S doubles, the matrix before normalisation, in out's
 * index order; sums (nullable): nq doubles, the matrix sum as formed (0 where k <= 1 and no sum
 * is taken).  Statistics of the last call: "spin_neighbors" (sum of k), "spin_kmax",
 * "spin_too_few" / "spin_bad_cos" (rows that broke either rule), "spin_queued" (rows with more
 * than "spin_cap_small" neighbours, which take the second pass); "spin_cap_small" and
 * "spin_chunk" (neighbours per accumulation chunk) can be read from a new ctx. */
pfx_status pfx_spin_image(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                          const float* snx, const float* sny, const float* snz, int64_t n_surface,
                          const float* qx, const float* qy, const float* qz, const float* qnx,
                          const float* qny, const float* qnz, int64_t nq, double radius,
                          const pfx_spin_params* params, float* out, double* raw, double* sums);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation: the errors above that
 * follow the kernel, and the statistics, are reported by the next pfx_ctx_synchronize /
 * pfx_ctx_last_stats on ctx. */
pfx_status pfx_spin_image_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                              const float* d_snx, const float* d_sny, const float* d_snz,
                              int64_t n_surface, const float* d_qx, const float* d_qy,
                              const float* d_qz, const float* d_qnx, const float* d_qny,
                              const float* d_qnz, int64_t nq, double radius,
                              const pfx_spin_params* params, float* d_out, double* d_raw,
                              double* d_sums);

/* ---- intensity gradients: IntensityGradientEstimation<PointXYZI, Normal, IntensityGradient,
 *      IntensityFieldAccessor<PointXYZI>> (evaluation.cpp:416-465, tools.h:40-54) ------------- */
/* out: nq x 3 floats.  si: the surface's intensities (pfx has no PointXYZI: PointXYZRGBtoXYZI's
 * I = (0.299f r + 0.587f g) + 0.114f b is the caller's, Python's rgb_to_intensity).  Over the
 * radius neighbours of query i in the surface, in FLANN order, all in float32: the centroid
 * (sequential sums, times 1 / float(k)) and the mean intensity (sequential sum / float(k)); then,
 * skipping a neighbour whose intensity is not finite, the six upper sums of A += p p^T and the
 * three of b += p (I - mean) with p the neighbour minus the centroid; x = Eigen 3.2's
 * A.colPivHouseholderQr().solve(b); the row is (Identity - n n^T) x with n = (qnx, qny, qnz)[i],
 * the caller's, as for the spin-image axis.  No normalisation.  k < 3 (a non-finite query has
 * k = 0): a NaN row.  A NaN normal, or a NaN intensity among the neighbours, gives a NaN row by
 * that arithmetic.  Every NaN is written as 0x7fc00000.
 * same_as_surface != 0: the queries are the surface itself (nq == n_surface; in the _dev form
 * qx == sx, qy == sy, qz == sz), the case of Tools::computeGradient.  That call builds the normal
 * estimation's neighbour lists and runs lane per list: its capacity is pfx_normals' and, like
 * pfx_normals_dev, its _dev form reads the list sizes back inside the call.  Otherwise one
 * workgroup serves a query, with at most 16384 neighbours (PFX_ERR_CAPACITY beyond, reported as
 * the spin image's late errors are).  Both paths give the same bits for the same query.
 * Null pointers, negative sizes, radius <= 0 or a same_as_surface call whose queries are not
 * the surface: PFX_ERR_INVALID before any launch.  Statistics: "igrad_neighbors" (sum of k),
 * "igrad_kmax". */
pfx_status pfx_intensity_gradient(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                                  const float* si, int64_t n_surface, const float* qx, const float* qy,
                                  const float* qz, const float* qnx, const float* qny, const float* qnz,
                                  int64_t nq, int32_t same_as_surface, double radius, float* out);
/* Device pointers, stream-ordered on the ctx stream; late errors and statistics as pfx_spin_image_dev. */
pfx_status pfx_intensity_gradient_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                      const float* d_si, int64_t n_surface, const float* d_qx,
                                      const float* d_qy, const float* d_qz, const float* d_qnx,
                                      const float* d_qny, const float* d_qnz, int64_t nq,
                                      int32_t same_as_surface, double radius, float* d_out);

/* ---- RIFT: RIFTEstimation<PointXYZI, IntensityGradient, Histogram<32>> (evaluation.cpp:716-765) */
/* out: nq x D G floats, D = nr_distance_bins and G = nr_gradient_bins, each in [1, 16];
 * out[gradient_bin D + distance_bin], PCL's histogram order.  (cx, cy, cz)[i] is the centre of
 * row i; (sgx, sgy, sgz) are the surface's intensity gradients.  Every radius neighbour, in FLANN
 * order, spreads its gradient magnitude bilinearly over its distance bins and (cyclically) its
 * angle bins; the matrix is then scaled by 1 / sqrt(sum of squares), in Eigen 3.2's float
 * summation order.  DESIGN.md "RIFT: the contract" states every operation; the CPU restatement
 * of that text is the truth the kernel is tested against (parity with PCL itself is unpinned).
 * The centre itself, when it is a neighbour, has no direction: angle 0.  A row whose gradients
 * are all zero is NaN (0 x inf), as is a row with a NaN gradient in its ball.  No neighbour at
 * all (a non-finite centre included): a NaN row, where PCL would leave the previous row's values.
 * Every NaN is written as 0x7fc00000.  Null pointers, negative sizes, radius <= 0, D or G outside
 * [1, 16]: PFX_ERR_INVALID before any launch.  More than 16384 neighbours: PFX_ERR_CAPACITY.
 * Statistics: "rift_neighbors" (sum of k), "rift_kmax", "rift_queued" (rows with more than
 * "rift_cap_small" neighbours, which take the second pass); "rift_cap_small" can be read from a
 * new ctx. */
pfx_status pfx_rift(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* sgx,
                    const float* sgy, const float* sgz, int64_t n_surface, const float* cx, const float* cy,
                    const float* cz, int64_t nq, double radius, int32_t nr_distance_bins,
                    int32_t nr_gradient_bins, float* out);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation; late errors and
 * statistics as pfx_spin_image_dev. */
pfx_status pfx_rift_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                        const float* d_sgx, const float* d_sgy, const float* d_sgz, int64_t n_surface,
                        const float* d_cx, const float* d_cy, const float* d_cz, int64_t nq, double radius,
                        int32_t nr_distance_bins, int32_t nr_gradient_bins, float* d_out);

/* ---- intensity spin images: IntensitySpinEstimation<PointXYZI, Histogram<20>>
 *      (evaluation.cpp:466-514) ---------------------------------------------------------------- */
/* out: nq x D I floats, D = nr_distance_bins and I = nr_intensity_bins, each in [1, 16];
 * out[distance_bin I + intensity_bin], PCL's copy order.  (cx, cy, cz)[i] is the centre of row i; si
 * are the surface's intensities (as for pfx_intensity_gradient).  No normals are read.  Over the
 * radius neighbours of a centre in FLANN order, all in float32 without FMA: the neighbourhood's
 * intensity range [min, max] (NaN intensities ignored); per neighbour d = D sqrt(d^2) / (radius +
 * FLT_EPSILON) and i = I (I_n - min) / ((max - min) + FLT_EPSILON); with sigma > 0 every bin
 * (dj, ii) of the window floor(d - 3 sigma) .. ceil(d + 3 sigma), floor(i - 3 sigma) .. ceil(i +
 * 3 sigma), clamped to the image, receives pfx_expf(-(d - dj)^2 c - (i - ii)^2 c), c = 1 / (2 sigma
 * sigma), a float addition per bin in neighbour order.  pfx_expf (csrc/pfx_expf.h) is the contract's
 * exponential, the same bits on host and device, faithfully rounded; it is not the C library's.
 * DESIGN.md "Intensity spin: the contract" states every operation; the CPU restatement of that text
 * is the truth the kernel is tested against (parity with PCL itself is unpinned).  No normalisation
 * (PCL has none).  A neighbour whose i is not finite (a NaN intensity; a range that overflows)
 * contributes nothing, so a ball whose intensities are all NaN gives a row of zeros.
 * Deliberate deviation, sigma == 0: the neighbour adds 1 to the bin ((int)d, (int)i); PCL writes out
 * of bounds when (int)i == I (the brightest neighbour of almost every ball) or (int)d == D; here
 * such a neighbour, and one whose i is not finite, is dropped.
 * No neighbour at all (a non-finite centre included): a NaN row, as PCL.  Every NaN is written as
 * 0x7fc00000.  Null pointers, negative sizes, radius <= 0 or NaN, D or I outside [1, 16], sigma
 * negative, NaN or above 2^20: PFX_ERR_INVALID before any launch.  More than 16384 neighbours:
 * PFX_ERR_CAPACITY.  Statistics: "ispin_neighbors" (sum of k), "ispin_kmax", "ispin_queued" (rows
 * with more than "ispin_cap_small" neighbours, which take the second pass); "ispin_cap_small",
 * "ispin_tile_words" and "ispin_tile" (the neighbours whose weights are formed at once: min(256,
 * ispin_tile_words / (D I | 1)), given for D I = 20) can be read from a new ctx. */
pfx_status pfx_intensity_spin(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* si,
                              int64_t n_surface, const float* cx, const float* cy, const float* cz, int64_t nq,
                              double radius, int32_t nr_distance_bins, int32_t nr_intensity_bins, float sigma,
                              float* out);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation; late errors and
 * statistics as pfx_spin_image_dev. */
pfx_status pfx_intensity_spin_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                  const float* d_si, int64_t n_surface, const float* d_cx, const float* d_cy,
                                  const float* d_cz, int64_t nq, double radius, int32_t nr_distance_bins,
                                  int32_t nr_intensity_bins, float sigma, float* d_out);

/* ---- 3D shape contexts: ShapeContext3DEstimation<PointXYZRGB, Normal, ShapeContext1980>
 * (evaluation.cpp:319-345) and UniqueShapeContext<PointXYZRGB, ShapeContext1980> (:346-371) ---- */
/* desc: nq x 1980 floats, bin = azimuth * 165 + elevation * 15 + radial (12 x 11 x 15, PCL 1.7's
 * fixed bins); rf: nq x 9 floats (x, y, z axis).  Every radius neighbour of a query (FLANN order,
 * strict d^2 < (float)(radius^2)) that is not within the close-point skip (|d^2| < FLT_EPSILON)
 * adds (1 / density) * lut[bin] to its bin, a float addition in neighbour order; density is the
 * number of surface points with d^2 < (float)(point_density_radius^2) around that neighbour,
 * itself included.  DESIGN.md "Shape contexts: the contract" states every operation; the CPU
 * restatement of that text is the truth the kernels are tested against (parity with PCL itself is
 * unpinned).
 * pfx_shape_context: the z axis of a row is the surface normal of its nearest neighbour; its x axis
 * is made from three floats of a random stream, orthogonalised against the normal.  rnd == NULL:
 * the stream of boost::mt19937 seeded 12345 through uniform_01<float>, from its start; else rnd
 * holds 3 nq floats and the t-th drawing row takes rnd[3t .. 3t + 2].  A row draws when its query
 * is finite and has a neighbour; a row that does not is NaN with a zero rf.  A NaN normal gives
 * NaN x and y axes and a finite row.
 * pfx_usc: the frame of row i is frames[9 i ..] (x, y, z axis; pfx_shot_lrf's layout): x its x
 * axis, the normal its z axis, rf a copy.  A non-finite query, or a frame whose x, y or z axis has
 * a non-finite first component: a NaN row with a zero rf.  No neighbour: a zero row.
 * Every NaN is written as 0x7fc00000.  Null pointers (rnd excepted), negative sizes, any radius
 * <= 0 or radius < min_radius: PFX_ERR_INVALID before any launch.  More than 16384 neighbours:
 * PFX_ERR_CAPACITY.  Statistics: "sc_neighbors" (sum of k), "sc_kmax", "sc_draws" (drawing rows),
 * "sc_skipped_close", "sc_support" (surface points whose density was counted: those in the ball of
 * a finite query), "sc_queued" (rows with more than "sc_cap_small" neighbours, which take the
 * second pass); "sc_cap_small" can be read from a new ctx. */
pfx_status pfx_shape_context(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                             const float* sny, const float* snz, int64_t n_surface, const float* qx,
                             const float* qy, const float* qz, int64_t nq, double radius, double min_radius,
                             double point_density_radius, const float* rnd, float* desc, float* rf);
pfx_status pfx_usc(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                   const float* qx, const float* qy, const float* qz, const float* frames, int64_t nq,
                   double radius, double min_radius, double point_density_radius, float* desc, float* rf);
/* SHOTLocalReferenceFrameEstimation alone: rf (nq x 9) equals pfx_shot's rf at the same radius bit
 * for bit, NaN rows (a non-finite query, fewer than five valid neighbours) and capacity (16384
 * neighbours, PFX_ERR_CAPACITY beyond) included. */
pfx_status pfx_shot_lrf(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                        const float* qx, const float* qy, const float* qz, int64_t nq, double radius, float* rf);
/* Device pointers, stream-ordered on the ctx stream (the surface grid's bounds are read back when
 * it was not prepared ahead, as for pfx_spin_image_dev; the first pfx_shape_context_dev call
 * without rnd uploads the default stream); late errors and statistics as pfx_spin_image_dev. */
pfx_status pfx_shape_context_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                 const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                                 const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq,
                                 double radius, double min_radius, double point_density_radius,
                                 const float* d_rnd, float* d_desc, float* d_rf);
pfx_status pfx_usc_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, int64_t n_surface,
                       const float* d_qx, const float* d_qy, const float* d_qz, const float* d_frames, int64_t nq,
                       double radius, double min_radius, double point_density_radius, float* d_desc,
                       float* d_rf);
pfx_status pfx_shot_lrf_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                            int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq,
                            double radius, float* d_rf);
/* Host only: n floats of the stream of boost::mt19937 seeded `seed` (init_genrand) read through
 * uniform_01<float> (v = (float)u32 / 2^32, drawn again unless v < 1), after skipping `skip`
 * floats. */
pfx_status pfx_rng_uniform01(uint32_t seed, int64_t skip, int64_t n, float* out);

/* ---- moment invariants: MomentInvariantsEstimation<PointXYZRGB, MomentInvariants>
 *      (evaluation.cpp:554-572) and principal curvatures: PrincipalCurvaturesEstimation<PointXYZRGB,
 *      Normal, PrincipalCurvatures> (evaluation.cpp:696-715) --------------------------------- */
/* Both read the radius neighbours of query i in the surface, in FLANN order, all in float32 with
 * no FMA contraction.  DESIGN.md "Moments and curvatures: the contract" states every operation;
 * the CPU restatement of that text is the truth the kernels are tested against (parity with PCL
 * itself is unpinned).
 * pfx_moment_invariants: out is nq x 3 floats, j1 j2 j3.  The centroid (three sequential sums,
 * each times 1 / float(k)); with t the neighbour minus the centroid, the six sequential sums mu200
 * mu020 mu002 mu110 mu101 mu011 of t0 t0, t1 t1, t2 t2, t0 t1, t0 t2, t1 t2; then
 *   j1 = mu200 + mu020 + mu002
 *   j2 = mu200 mu020 + mu200 mu002 + mu020 mu002 - mu110^2 - mu101^2 - mu011^2
 *   j3 = mu200 mu020 mu002 + 2 mu110 mu101 mu011 - mu002 mu110^2 - mu020 mu101^2 - mu200 mu011^2
 * left to right.  k = 1 gives 0 0 0.
 * pfx_principal_curvatures: out is nq x 5 floats, the principal direction x y z, then pc1 and pc2.
 * (snx, sny, snz) are the surface normals and n = (qnx, qny, qnz)[i] the caller's query normal, as
 * for the spin-image axis.  Every neighbour normal is projected by M = Identity - n n^T; the
 * centroid of the projections (sequential sums, times 1 / float(k)) and the six upper sums of
 * their covariance follow; pcl::eigen33 gives its eigenvalues (ascending),
 * pcl::computeCorrespondingEigenVector the direction of the largest; pc1 and pc2 are the largest
 * and the middle eigenvalue times 1 / float(k).  Equal normals in the ball (k = 1 included) give
 * pc1 = pc2 = 0 and a NaN direction (0 / 0), PCL's result.  A NaN query normal or a NaN normal
 * among the neighbours gives whatever that arithmetic gives.
 * Both: k = 0 (a non-finite query included) is a NaN row; every NaN is written as 0x7fc00000.
 * Null pointers, negative sizes or radius <= 0: PFX_ERR_INVALID before any launch; nq == 0
 * succeeds without a launch.  One workgroup serves a query, with at most 16384 neighbours
 * (PFX_ERR_CAPACITY beyond, reported as the spin image's late errors are).  Statistics:
 * "moments_neighbors" / "pcurv_neighbors" (sum of k), "moments_kmax" / "pcurv_kmax",
 * "moments_queued" / "pcurv_queued" (rows with more than "moments_cap_small" neighbours, which take
 * the second pass); "moments_cap_small" can be read from a new ctx. */
pfx_status pfx_moment_invariants(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                                 int64_t n_surface, const float* qx, const float* qy, const float* qz,
                                 int64_t nq, double radius, float* out);
pfx_status pfx_principal_curvatures(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                                    const float* snx, const float* sny, const float* snz, int64_t n_surface,
                                    const float* qx, const float* qy, const float* qz, const float* qnx,
                                    const float* qny, const float* qnz, int64_t nq, double radius, float* out);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation; late errors and
 * statistics as pfx_spin_image_dev. */
pfx_status pfx_moment_invariants_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                     int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz,
                                     int64_t nq, double radius, float* d_out);
pfx_status pfx_principal_curvatures_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                        const float* d_snx, const float* d_sny, const float* d_snz,
                                        int64_t n_surface, const float* d_qx, const float* d_qy,
                                        const float* d_qz, const float* d_qnx, const float* d_qny,
                                        const float* d_qnz, int64_t nq, double radius, float* d_out);

/* ---- BOARD local reference frames: BOARDLocalReferenceFrameEstimation<PointXYZRGB, Normal,
 *      ReferenceFrame> (evaluation.cpp:372-393) ---------------------------------------------- */
/* PCL's setters.  tangent_radius (0: unset, PCL's default and the reference's) and margin_thresh
 * (0.85) must be finite and >= 0.  find_holes: only 0 is supported (PFX_ERR_UNSUPPORTED otherwise:
 * PCL then seeds its angular bins from rand(), whose sequence runs on from one keypoint to the
 * next).  check_margin_array_size (24), hole_size_prob_thresh (0.2) and steep_thresh (0.1) matter
 * only with find_holes and are carried unused.  pfx_board_params_default fills 0, 0.85, 0, 24,
 * 0.2, 0.1. */
typedef struct pfx_board_params {
  float tangent_radius;
  float margin_thresh;
  int32_t find_holes;
  int32_t check_margin_array_size;
  float hole_size_prob_thresh;
  float steep_thresh;
} pfx_board_params;
void pfx_board_params_default(pfx_board_params* p);
/* rf: nq x 9 floats, the x, y and z axis of every row (pfx_shot_lrf's layout).  DESIGN.md "BOARD:
 * the contract" states every operation; the CPU restatement of that text is the truth the kernel
 * is tested against (parity with PCL itself is unpinned, and the z axis is this project's
 * definition: PCL's float SVD cannot be restated bit for bit).  All in float32 left to right
 * without FMA contraction unless said otherwise; neighbours in FLANN order, strict
 * d^2 < (float)(radius^2).
 *   support    the radius neighbours of query i; fewer than 6: a NaN row.
 *   z          centroid = the sequential sums of the neighbours' xyz, each / float(k); the six
 *              sums of (s - c)(s - c)^T in double, in neighbour order; z = the eigenvector of the
 *              smallest eigenvalue (Eigen 3.2's SelfAdjointEigenSolver<Matrix3d>, as for SHOT's
 *              frames), cast to float; negated when its dot product with the normalised sum of
 *              the neighbours' normals is < 0 (a NaN sum never flips).
 *   tangent    with tangent_radius != 0 and != radius, the neighbours at tangent_radius replace
 *              the support from here on.  margin2 = (margin_thresh margin_thresh) (tangent_radius
 *              tangent_radius): 0 with the tangent radius unset, so that every neighbour with
 *              d^2 > 0 is "on the margin" (PCL 1.7's behaviour, kept).
 *   x          the neighbour with d^2 > margin2 whose normal has the smallest z . n, the first
 *              strict minimum in neighbour order (a NaN never wins); when no neighbour has
 *              d^2 > margin2, the same over all of them; nothing chosen: a NaN row.  With b that
 *              neighbour and p the query: x = (b - (z . (b - p)) z) - p, divided by its norm;
 *              y = z cross x.  b on the line through p along z: x and y NaN, z finite.
 * Every NaN is written as 0x7fc00000.  A null required pointer (params included), a negative
 * size, radius <= 0, a negative or non-finite tangent_radius or margin_thresh: PFX_ERR_INVALID
 * before anything is copied or launched.  nq == 0 is a no-op; n_surface == 0 fills rf with NaN.
 * The keys of a query are gathered once at max(radius, tangent_radius): more than 16384 of them
 * is PFX_ERR_CAPACITY.  Statistics: "board_neighbors" (sum of the gathered k), "board_kmax",
 * "board_queued" (rows with more than "board_cap_small" keys, which take the second pass);
 * "board_cap_small" can be read from a new ctx. */
pfx_status pfx_board_lrf(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                         const float* sny, const float* snz, int64_t n_surface, const float* qx, const float* qy,
                         const float* qz, int64_t nq, double radius, const pfx_board_params* params, float* rf);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation (the surface grid's
 * bounds are read back when it was not prepared ahead); late errors and statistics as
 * pfx_spin_image_dev. */
pfx_status pfx_board_lrf_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                             const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                             const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq, double radius,
                             const pfx_board_params* params, float* d_rf);

/* ---- boundary points: BoundaryEstimation<PointXYZRGB, Normal, Boundary>
 *      (evaluation.cpp:394-415) ------------------------------------------------------------ */
/* out: nq bytes, 1 for a query on a boundary of the surface (a scan edge, a hole's rim), 0 for one
 * that is not, PFX_BOUNDARY_NO_NEIGHBORS for one without a neighbour.  (qnx, qny, qnz) are the
 * normals of the QUERIES, one per query; no surface normal is read.  DESIGN.md "Boundary: the
 * contract" states every operation; the CPU restatement of that text is the truth the kernel is
 * tested against (parity with PCL itself is unpinned).  All in float32 left to right without FMA
 * contraction; the neighbours are the set with d^2 < (float)(radius^2), k of them, in any order.
 *   k == 0     PFX_BOUNDARY_NO_NEIGHBORS; k < 3: 0.
 *   axes       v = Eigen's unitOrthogonal of (n, 0), u = n cross v (PCL's
 *              getCoordinateSystemOnPlane); a non-finite component of either (a NaN, an infinite or
 *              a zero normal): 0.
 *   angles     atan2f(v . d, u . d) for every neighbour with d = p - q != 0 (glibc's routine);
 *              none: 0.  A NaN angle (dot products that overflow): 0.
 *   gap test   1 when two angles adjacent in ascending order differ by more than angle_threshold,
 *              or (2 pi - the largest) + the smallest does; else 0.
 * angle_threshold (PCL's default: pi / 2) below (float)(pi / 64) is PFX_ERR_UNSUPPORTED: the kernel
 * does not sort; it compares the angles across 256 bins and never within one, which is exact only
 * for a threshold of at least two bin widths.  A NaN angle_threshold, a null required pointer, a
 * negative size, radius <= 0: PFX_ERR_INVALID before anything is copied or launched.  nq == 0 is a
 * no-op; n_surface == 0 fills out with PFX_BOUNDARY_NO_NEIGHBORS.  There is no capacity: a query
 * may have any number of neighbours.  Statistics: "boundary_neighbors" (sum of k),
 * "boundary_kmax", "boundary_flagged" (the number of 1s). */
#define PFX_BOUNDARY_NO_NEIGHBORS 255
pfx_status pfx_boundary(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                        const float* qx, const float* qy, const float* qz, const float* qnx, const float* qny,
                        const float* qnz, int64_t nq, double radius, float angle_threshold, uint8_t* out);
/* Device pointers, stream-ordered on the ctx stream, no host synchronisation (the surface grid's
 * bounds are read back when it was not prepared ahead); nothing is reported late but the
 * statistics, which the next synchronisation of the ctx brings. */
pfx_status pfx_boundary_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                            int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz,
                            const float* d_qnx, const float* d_qny, const float* d_qnz, int64_t nq,
                            double radius, float angle_threshold, uint8_t* d_out);

/* ---- smooth clusters and CVFH: CVFHEstimation<PointXYZRGB, Normal, VFHSignature308>
 *      (evaluation.cpp:649-675) -------------------------------------------------------------- */
/* pfx_smooth_clusters is pcl::extractEuclideanClustersSmooth: the connected components of the graph
 * whose edges i - j (i != j) are the pairs with
 *   d^2 < (float)(t t), t = (double)tolerance, d^2 = ((0 + dx^2) + dy^2) + dz^2, and
 *   acos((double)dot) < eps_angle, dot the float ((n_i.x n_j.x + n_i.y n_j.y) + n_i.z n_j.z);
 * a NaN anywhere, or dot > 1 (acos is NaN), gives no edge.  A component of at least min_points points
 * is a cluster; the clusters are numbered by their lowest index.  labels: n int32, the point's
 * cluster or -1; *n_clusters: their number.  DESIGN.md "CVFH: the contract" states every operation;
 * the CPU restatement of that text is the truth the kernels are tested against (parity with PCL
 * itself is unpinned).  Nothing is kept per point but a parent word: there is no capacity.
 * A null required pointer, a negative size, a NaN or non-positive tolerance, a NaN eps_angle,
 * min_points < 1 or n >= 2^31: PFX_ERR_INVALID before anything is copied or launched.  n == 0 gives
 * no cluster.  Statistics: "cvfh_edges" (the edges, each once), "cvfh_cc_rounds" (hooking rounds,
 * the last one, which changes nothing, included), "cvfh_clusters". */
pfx_status pfx_smooth_clusters(pfx_ctx* ctx, const float* x, const float* y, const float* z, const float* nx,
                               const float* ny, const float* nz, int64_t n, float tolerance, double eps_angle,
                               int32_t min_points, int32_t* labels, int64_t* n_clusters);
/* Device pointers (d_n_clusters too), on the ctx stream.  The call waits on the host once, for the
 * flag that says the components are complete (and again for every 8 hooking rounds beyond the
 * first 8); the statistics are set when it returns. */
pfx_status pfx_smooth_clusters_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                   const float* d_nx, const float* d_ny, const float* d_nz, int64_t n,
                                   float tolerance, double eps_angle, int32_t min_points, int32_t* d_labels,
                                   int64_t* d_n_clusters);

/* PCL 1.7's defaults (pfx_cvfh_params_default): viewpoint (0, 0, 0), radius_normals and
 * cluster_tolerance 3 * 0.005f (leaf_size_ * 3), eps_angle_threshold 0.125f, curvature_threshold
 * 0.03f, min_points 50, normalize_bins 0. */
typedef struct pfx_cvfh_params {
  float viewpoint[3];
  float radius_normals;
  float cluster_tolerance;
  float eps_angle_threshold;
  float curvature_threshold;
  int32_t min_points;
  int32_t normalize_bins;
} pfx_cvfh_params;
void pfx_cvfh_params_default(pfx_cvfh_params* p);

#define PFX_CVFH_DIM 308
/* CVFH over the n_indices points indices[0..) of the surface (indices == NULL: all n_surface points,
 * and n_indices must equal n_surface): the points whose curvature is not above the threshold are
 * given new normals (pfx_normals at radius_normals, viewpoint (0, 0, 0)) and clustered
 * (pfx_smooth_clusters); every cluster gives one row, a VFH signature of ALL indexed points about
 * the cluster's mean point and normalised mean normal: 45 bins each of f1, f2, f3 and f4, then 128 of
 * the viewpoint component.  Without a cluster there is one row, about the centroid of the whole
 * surface and the mean of the indexed normals.  Every bin is the float sum of a count of equal
 * increments, so a row is a function of integer counts; nothing depends on the order of execution.
 *   out               cap x 308 floats; *n_rows the number of rows
 *   centroids         (nullable) cap x 3, dominant_normals (nullable) cap x 3: what each row is about
 *   labels            (nullable) n_indices int32: the indexed point's cluster, or -1
 * More rows than cap: PFX_ERR_CAPACITY with the required number in *n_rows and nothing written.
 * n_indices > 2^24 (a float stops counting exactly): PFX_ERR_CAPACITY.  n_indices == 0: no row.
 * An index outside [0, n_surface), a null required pointer, a negative size, a NaN or non-positive
 * radius_normals or cluster_tolerance, a NaN eps_angle_threshold, min_points < 1: PFX_ERR_INVALID.
 * Statistics: "cvfh_filtered" (the points that pass the curvature filter), "cvfh_clusters",
 * "cvfh_edges", "cvfh_cc_rounds", "cvfh_rows". */
pfx_status pfx_cvfh(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                    const float* sny, const float* snz, const float* scurvature, int64_t n_surface,
                    const int32_t* indices, int64_t n_indices, const pfx_cvfh_params* params, float* out, int64_t cap,
                    int64_t* n_rows, float* centroids, float* dominant_normals, int32_t* labels);
/* Device pointers (d_n_rows too), on the ctx stream.  The call waits on the host as pfx_normals_dev
 * does for its lists and then once for the cluster count (and as pfx_smooth_clusters_dev says beyond
 * 8 rounds); the capacity and index errors are returned by the call itself and the statistics are
 * set when it returns.  The rows are complete in stream order. */
pfx_status pfx_cvfh_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, const float* d_snx,
                        const float* d_sny, const float* d_snz, const float* d_scurvature, int64_t n_surface,
                        const int32_t* d_indices, int64_t n_indices, const pfx_cvfh_params* params, float* d_out,
                        int64_t cap, int64_t* d_n_rows, float* d_centroids, float* d_dominant_normals,
                        int32_t* d_labels);

/* ---- range image + NARF keypoints ---------------------------------------------------- */
/* out_points: width*height x 4 floats {x, y, z, range} (PointWithRange); unobserved pixels
 * are {NaN, NaN, NaN, -inf}. */
pfx_status pfx_range_image_planar(pfx_ctx* ctx, const float* x, const float* y, const float* z,
                                  int64_t n, const pfx_camera* cam, float* out_points);
/* Keypoint pixel indices (y*width + x), ascending, as NarfKeypoint::compute returns them in
 * PointCloud<int>.  *n_out = number of keypoints; PFX_ERR_CAPACITY if it exceeds cap. */
pfx_status pfx_narf_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z,
                              int64_t n, const pfx_camera* cam, const pfx_narf_params* params,
                              int32_t* out, int64_t cap, int64_t* n_out);
pfx_status pfx_narf_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y,
                                  const float* d_z, int64_t n, const pfx_camera* cam,
                                  const pfx_narf_params* params, int32_t* out, int64_t cap,
                                  int64_t* n_out);
/* Debug/parity access to the NARF intermediates of the last pfx_narf_keypoints* call
 * (host buffers of width*height elements):  "interest" (float), "surface_change" (float),
 * "border_traits" (uint32 bitset, PCL BorderTrait order), "range" (float).  count must be exactly
 * width*height of that call's camera: any other count is PFX_ERR_CAPACITY and nothing is written.
 * A NARF call that fails leaves no images behind (PFX_ERR_INVALID until the next one succeeds). */
pfx_status pfx_narf_debug_image(pfx_ctx* ctx, const char* which, void* out, int64_t count);

/* ---- NARF descriptors: NarfDescriptor (evaluation.cpp:613-648) ---------------------------- */
/* The 36-float NARF descriptor (PCL's defaults: descriptor length 36, a 10 x 10 patch; nothing
 * else is offered) of the entries of pixel_idx (y * width + x) on the planar range image of the
 * cloud and camera, which the call builds itself.  DESIGN.md "NARF descriptors: the contract"
 * states every operation; the CPU restatement of that text is the truth the kernel is tested
 * against bit for bit (parity with PCL itself is unpinned).  All in float32 left to right without
 * FMA contraction.  For every entry, in order:
 *   validity   a negative index, one beyond the image, or a pixel without a finite range: no row
 *              ("narf_desc_invalid_pixels").
 *   pose       getNormalBasedUprightTransformation (point, support_size / 2): the weighted
 *              VectorAverage3f of the ring pixels within support_size / 2, its smallest
 *              eigenvector the normal; with 10 samples or fewer getNormalForClosestNeighbors
 *              ("narf_desc_fallback_normals"); no normal, or a frame that is not finite (a normal
 *              along (0, 1, 0)): no row ("narf_desc_pose_failed").
 *   patch      getInterpolatedSurfaceProjection (pose, 10, support_size), unseen cells in front of
 *              something further than support_size / 2 behind set to +inf
 *              ("narf_desc_background_cells"), blurred by getBlurredSurfacePatch (20, 1).
 *   rows       rotation_invariant == 0: one row, extractDescriptor (36) at rotation 0 with the pose
 *              above.  Otherwise one row for each of getRotations' 0 to 5 rotations rho, in the
 *              order they are chosen: the descriptor at rho and Rz (-rho) * pose.  A perfectly
 *              flat patch has no rotation and so no row.
 * desc: cap x 36; pose: cap x 12, the row-major 3 x 4 [R | t] that takes world to patch
 * coordinates; row_key: cap, the entry of pixel_idx a row came from.  Rows come in entry order; cap
 * = 5 nk never overflows.  *n_out = the number of rows; more than cap: PFX_ERR_CAPACITY, nothing
 * written but *n_out, the size needed.  A null required pointer, a negative size, support_size <= 0
 * or NaN, nk above 2^28: PFX_ERR_INVALID before anything is copied or launched; so is a camera beyond
 * pfx_narf_keypoints' bounds, and noise_level != 0 is PFX_ERR_UNSUPPORTED.  nk == 0 gives no row; n
 * == 0 an empty image, every entry invalid.  Statistics: "narf_desc_rows" and the four above,
 * "narf_desc_ring_max" (the largest ring radius walked by the pose and the patch). */
typedef struct pfx_narf_desc_params {
  float support_size;         /* -1: must be set > 0 (the reference passes its support_size) */
  int32_t rotation_invariant; /* 1 */
} pfx_narf_desc_params;
void pfx_narf_desc_params_default(pfx_narf_desc_params* p);
pfx_status pfx_narf_descriptors(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                const pfx_camera* cam, const int32_t* pixel_idx, int64_t nk,
                                const pfx_narf_desc_params* params, float* desc, float* pose, int32_t* row_key,
                                int64_t cap, int64_t* n_out);
/* Device pointers (pixel_idx, the outputs and the count d_n_out included), stream-ordered on the ctx
 * stream, no host synchronisation.  With more rows than cap the first cap rows are written and
 * *d_n_out is the full count; the statistics come with the next synchronisation of the ctx. */
pfx_status pfx_narf_descriptors_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                    const pfx_camera* cam, const int32_t* d_pixel_idx, int64_t nk,
                                    const pfx_narf_desc_params* params, float* d_desc, float* d_pose,
                                    int32_t* d_row_key, int64_t cap, int64_t* d_n_out);

/* ---- Tools::getIndices (tools.h:91-102) --------------------------------------------------- */
/* For each keypoint i in order, every cloud index j ascending with |kx[i] - x[j]| < tol and the
 * same in y and z (Tools::areEqual; the reference's tol is 1e-4f).  A NaN matches nothing; a
 * keypoint may give none or several indices.  *n_out = their number; more than cap:
 * PFX_ERR_CAPACITY, nothing written but *n_out.  A null required pointer, a negative size, tol NaN
 * or n >= 2^31: PFX_ERR_INVALID before anything is copied or launched. */
pfx_status pfx_point_indices(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                             const float* kx, const float* ky, const float* kz, int64_t nk, float tol, int32_t* out,
                             int64_t cap, int64_t* n_out);
/* Device pointers, stream-ordered, no host synchronisation: the first cap indices and, in
 * *d_n_out (device), the full count. */
pfx_status pfx_point_indices_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                 const float* d_kx, const float* d_ky, const float* d_kz, int64_t nk, float tol,
                                 int32_t* d_out, int64_t cap, int64_t* d_n_out);

/* Test hook of the uniform grid (host buffers): builds the normal-radius grid of a cloud and
 * copies it out.
 *   mode 0:  exact build (bounds pass, radix sort); leaves the bounds hint of this grid
 *   mode 1:  speculative build on that hint (counting sort where eligible), then what a caller
 *            does: the validation word is read back and, when non-zero, the grid is rebuilt
 *            exactly; the arrays are those of the grid the caller ends up with
 *   mode -1: no build, the arrays of the grid the last call left (n must be its point count)
 * Outputs, each nullable: perm[n], skeys[n], sp[4 n] (x, y, z, 0 per sorted position),
 * cell_start[ncells + 2] (cell_start_cap: elements the buffer holds; too few ->
 * PFX_ERR_CAPACITY), params[4] = the exact cell mapping (origin x, y, z, 1 / cell),
 * info[8] = nx, ny, nz, ncells, the raw validation word of the (first) build, its builder
 * (0 radix sort, 1 counting sort), 1 if it was rebuilt exactly, the counting builder's cell cap. */
pfx_status pfx_grid_debug(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                          double radius, int32_t mode, int32_t* perm, uint32_t* skeys, float* sp,
                          int32_t* cell_start, int64_t cell_start_cap, double* params, int64_t* info);

/* ---- the reference's keypoint -> cloud mapping (keypoints.h:227-229) ----------------- */
/* k_xyz[i] = cloud[idx[i]] for 0 <= idx[i] < n (the reference indexes the cloud with pixel
 * indices; out-of-range indices are an out-of-bounds read there and are skipped here).
 * d_kx/d_ky/d_kz hold `cap` floats each; more in-range indices than `cap` -> PFX_ERR_CAPACITY
 * (nothing written).  Returns the number of points written in *n_out. */
pfx_status pfx_gather_points_dev(pfx_ctx* ctx, const float* d_x, const float* d_y,
                                 const float* d_z, int64_t n, const int32_t* idx, int64_t k,
                                 float* d_kx, float* d_ky, float* d_kz, int64_t cap, int64_t* n_out);

/* Descriptor matching.  Rows are `dim` floats, `*_stride` floats apart
 * (FPFHSignature33: dim 33, stride 33; PointCloud<SHOT352> read in place: dim 352, stride 361;
 * PointCloud<SHOT1344>: dim 1344, stride 1353).
 * Distance = FLANN L2_Simple<float> (sequential float sum of squared differences), exact 1-NN;
 * equal distances -> the lowest row (FLANN: first visited, unpinned); a source row with a
 * non-finite value, or no finite target row -> -1 and NaN distance.  Every finite row is
 * matched, whatever its magnitude: subnormal distances keep their bits, and a row whose squared
 * differences overflow gets the nearest row by float order (all distances +inf -> the lowest
 * finite row, distance +inf).
 * Both directions in one pass: d_s2t[i] = nearest target row of source row i (+ its squared
 * distance), d_t2s[j] = nearest source row of target row j.  Distance and t2s outputs are
 * nullable.  Stream-ordered except for one host read of the candidate count. */
pfx_status pfx_nearest_descriptors_dev(pfx_ctx* ctx, const float* d_src, int64_t n_src, int64_t src_stride,
                                       const float* d_tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                                       int32_t* d_s2t, float* d_s2t_dist, int32_t* d_t2s, float* d_t2s_dist);
/* Host-pointer form of one direction (the facade's KdTreeFLANN<FeatureT>::nearestKSearch). */
pfx_status pfx_nearest_descriptors(pfx_ctx* ctx, const float* src, int64_t n_src, int64_t src_stride,
                                   const float* tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                                   int32_t* s2t, float* s2t_dist);
/* Mutual nearest neighbours (index_query, index_match) in source order.  *n_out = the number
 * of correspondences (host); PFX_ERR_CAPACITY (nothing written) when it exceeds cap. */
pfx_status pfx_correspondences_dev(pfx_ctx* ctx, const float* d_src, int64_t n_src, int64_t src_stride,
                                   const float* d_tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                                   int32_t* d_query, int32_t* d_match, int64_t cap, int64_t* n_out);
pfx_status pfx_correspondences(pfx_ctx* ctx, const float* src, int64_t n_src, int64_t src_stride,
                               const float* tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                               int32_t* query, int32_t* match, int64_t cap, int64_t* n_out);

/* ---- PCD v0.7 input ------------------------------------------------- */
typedef struct pfx_pcd_header {
  int64_t points;          /* POINTS (default WIDTH * HEIGHT)                                  */
  int32_t width, height;
  int32_t data;            /* 0 ascii, 1 binary, 2 binary_compressed                            */
  int32_t point_size;      /* binary: bytes per point; ascii: columns per point                 */
  int32_t x_offset, y_offset, z_offset; /* binary: byte offsets; ascii: column indices          */
  int32_t nfields;
  float viewpoint[7];      /* VIEWPOINT tx ty tz qw qx qy qz (sensor_origin_, sensor_orientation_) */
  int64_t data_offset;     /* byte offset of the data block                                     */
} pfx_pcd_header;
/* Header only (host, no device, no context).  x, y, z must be single float32 fields. */
pfx_status pfx_pcd_read_header(const char* path, pfx_pcd_header* out);
/* loadPCDFile: x, y, z of every point into device SoA arrays (caller order = file order, NaN
 * points kept as in PCL's non-dense clouds).  *n_out = POINTS; PFX_ERR_CAPACITY (nothing
 * written) when it exceeds cap.  hdr (nullable) receives the header (viewpoint = the cloud's
 * sensor pose, which NARF's range image uses: keypoints.h:207-210). */
pfx_status pfx_pcd_load_xyz_dev(pfx_ctx* ctx, const char* path, float* d_x, float* d_y, float* d_z,
                                int64_t cap, int64_t* n_out, pfx_pcd_header* hdr);

/* ---- active-list keypoints ------------------------------------------ */
/* Keypoints::computeCloudResolution: mean distance of every finite point to its nearest other
 * point (FLANN kNN k = 2, the first hit being the point itself), 0 without such points. */
pfx_status pfx_cloud_resolution_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                    double* resolution);
pfx_status pfx_cloud_resolution(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                double* resolution);
/* ISSKeypoint3D::compute (PCL 1.7 iss_3d.hpp): setSalientRadius, setNonMaxRadius,
 * setMinNeighbors, setThreshold21, setThreshold32 (keypoints.h:182-187; no border radius).
 * Keypoint cloud indices in ascending order into idx[0..cap); *n_out = their number
 * (PFX_ERR_CAPACITY, nothing written, when it exceeds cap).  third (nullable, n doubles): the
 * per-point third eigenvalue map (0 where the point is not a candidate).  A parameter that
 * PCL's initCompute rejects (radius, threshold or min neighbours <= 0) -> PFX_ERR_INVALID. */
pfx_status pfx_iss_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                 double salient_radius, double non_max_radius, int32_t min_neighbors,
                                 double threshold21, double threshold32, int32_t* d_idx, int64_t cap,
                                 int64_t* n_out, double* d_third);
pfx_status pfx_iss_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                             double salient_radius, double non_max_radius, int32_t min_neighbors,
                             double threshold21, double threshold32, int32_t* idx, int64_t cap, int64_t* n_out,
                             double* third);

/* UniformSampling::compute (PCL 1.7 keypoints/impl/uniform_sampling.hpp) with setRadiusSearch(radius):
 * one keypoint per occupied voxel of edge leaf = (float)radius, by DESIGN.md "Uniform sampling: the
 * contract".  A point with a non-finite coordinate takes no part.  The cell of a point is
 * (int)floorf(coordinate * inv), inv = 1.0f / leaf; its winner is the point with the smallest
 * (diff, index), diff = (dx*dx + dz*dz) + (dy*dy + 1.0f) in float32 with dx = x - (float)i, ...:
 * PCL subtracts the integer cell coordinates, not the cell's centre.  idx[0..cap) receives the
 * winners' cloud indices in ascending leaf index (PCL: the iteration order of a
 * boost::unordered_map, the same set), leaf (nullable, cap) each keypoint's leaf index
 * (i - min_i) + (j - min_j) div_x + (k - min_k) div_x div_y, *n_out the number of occupied cells;
 * 0 for n == 0 or a cloud without a finite point.
 *   PFX_ERR_INVALID   unless leaf is finite and > 0 and inv is finite (radius 0, negative, NaN, 1e-46);
 *   PFX_ERR_CAPACITY  nothing written: *n_out exceeds cap (*n_out = the required count); or a product
 *                     coordinate * inv lies outside [-2^31, 2^31), or the bounding box holds more than
 *                     2^31 - 1 cells (*n_out = 0; PCL's int leaf index overflows silently there).
 * There is no other limit on the extent: memory grows with n, never with the number of cells.  Two
 * host waits (the bounds, the count).  Statistics: "uniform_points" (the points that took part),
 * "uniform_leaves" (*n_out), "uniform_cells" (div_x div_y div_z). */
pfx_status pfx_uniform_sampling_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                    double radius, int32_t* d_idx, int64_t cap, int64_t* n_out, int32_t* d_leaf);
pfx_status pfx_uniform_sampling(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                double radius, int32_t* idx, int64_t cap, int64_t* n_out, int32_t* leaf);

/* HarrisKeypoint3D (method HARRIS) + Keypoints::getKeypointsCloud: response over the normals of
 * the radius ball (NormalEstimation at the same radius, viewpoint 0), non-maximum suppression
 * above `threshold`, corner refinement (refine != 0, PCL's default), then every corner snapped
 * to its nearest cloud point when d2 < 0.0001.  idx[0..cap): those cloud indices in corner
 * (= index) order, *n_out their number (PFX_ERR_CAPACITY when it or the corner count exceeds
 * cap).  response (nullable, n floats): per-point intensity; corners (nullable, 3 * cap floats)
 * and n_corners (nullable): the refined corners; corner_idx (nullable, cap int32): the cloud index
 * of each corner's own point (PCL's output intensity = response[corner_idx]).  non_max == 0 ->
 * PFX_ERR_UNSUPPORTED (not used by the reference: keypoints.h:155). */
pfx_status pfx_harris3d_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                      double radius, float threshold, int32_t non_max, int32_t refine,
                                      int32_t* d_idx, int64_t cap, int64_t* n_out, float* d_response,
                                      float* d_corners, int64_t* n_corners, int32_t* d_corner_idx);
pfx_status pfx_harris3d_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                  double radius, float threshold, int32_t non_max, int32_t refine, int32_t* idx,
                                  int64_t cap, int64_t* n_out, float* response, float* corners, int64_t* n_corners,
                                  int32_t* corner_idx);

/* HarrisKeypoint6D (keypoints.h:164-176) + Keypoints::getKeypointsCloud: normals at the radius
 * (viewpoint 0), IntensityGradientEstimation at the radius over the colour intensity
 * float(299 r + 587 g + 114 b) * 0.001f (IntensityFieldAccessor<PointXYZRGB>), gradients of
 * squared length > 200 scaled to unit length and every other gradient (NaN ones included) set
 * to 0 (harris_6d.hpp's else branch), the 6x6 covariance of (normal, gradient) over the
 * radius ball and its fourth eigenvalue as the response (responseTomasi), non-maximum
 * suppression above `threshold`, corner refinement, snap -- outputs as the Harris3D entry.
 * rgb: one packed 0x00RRGGBB word per point (the bits of PointXYZRGB::rgb).  grad (nullable,
 * 3 n floats): the normalised gradient of every point (0 where PCL's normalisation zeroes it). */
pfx_status pfx_harris6d_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                      const uint32_t* d_rgb, int64_t n, double radius, float threshold,
                                      int32_t non_max, int32_t refine, int32_t* d_idx, int64_t cap, int64_t* n_out,
                                      float* d_response, float* d_corners, int64_t* n_corners, float* d_grad,
                                      int32_t* d_corner_idx);
pfx_status pfx_harris6d_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z, const uint32_t* rgb,
                                  int64_t n, double radius, float threshold, int32_t non_max, int32_t refine,
                                  int32_t* idx, int64_t cap, int64_t* n_out, float* response, float* corners,
                                  int64_t* n_corners, float* grad, int32_t* corner_idx);

/* ---- RANSAC correspondence rejection --------------------------------- */
/* CorrespondenceRejectorSampleConsensus::getCorrespondences + getBestTransformation (host
 * arrays: the two keypoint clouds and the n correspondences index_query -> index_match):
 * setInlierThreshold(threshold), setMaximumIterations(max_iterations).  keep[0..*n_keep) =
 * positions of the remaining correspondences in input order (all of them when RANSAC finds no
 * model or fewer than 3 inliers, as PCL), transformation = the best model, row-major 4x4
 * (identity in those cases). */
pfx_status pfx_ransac_rejector(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns,
                               const float* tx, const float* ty, const float* tz, int64_t nt, const int32_t* query,
                               const int32_t* match, int64_t n, double threshold, int32_t max_iterations,
                               int32_t* keep, int64_t* n_keep, float* transformation);

/* ---- ICP alignment (evaluation.cpp:863-885, icpAlign) --------------------------------- */
/* pcl::IterativeClosestPoint<PointXYZRGB,PointXYZRGB>::align as PCL 1.7.2 runs it with its
 * defaults (correspondence estimation without reciprocity, no rejectors, Umeyama's fit in float,
 * DefaultConvergenceCriteria), restated in DESIGN.md "ICP: the contract"; results equal the CPU
 * restatement tests/cpp/icp_ref.cpp bit for bit, parity with real PCL is unpinned.
 * pfx_icp_params_default fills PCL's defaults: sqrt(DBL_MAX), 10, 0, -DBL_MAX (the reference sets
 * 0.07, 100, 1e-6, 1e-4).  Sigma is accumulated over depth blocks of PFX_ICP_GEMM_DEPTH
 * correspondences (Eigen 3.2's GEMM panel for a 32 KiB L1). */
#define PFX_ICP_GEMM_DEPTH 1024
typedef struct pfx_icp_params {
  double max_correspondence_distance; /* setMaxCorrespondenceDistance, > 0                     */
  int32_t max_iterations;             /* setMaximumIterations, >= 0 (0 still runs one)         */
  double transformation_epsilon;      /* setTransformationEpsilon                              */
  double euclidean_fitness_epsilon;   /* setEuclideanFitnessEpsilon                            */
} pfx_icp_params;
void pfx_icp_params_default(pfx_icp_params* p);
/* DefaultConvergenceCriteria's state after align; PFX_ICP_NO_CORRESPONDENCES: fewer than 3 pairs */
enum {
  PFX_ICP_NOT_CONVERGED = 0,
  PFX_ICP_ITERATIONS = 1,
  PFX_ICP_TRANSFORM = 2,
  PFX_ICP_ABS_MSE = 3,
  PFX_ICP_REL_MSE = 4,
  PFX_ICP_NO_CORRESPONDENCES = 5
};
/* Source and target clouds as SoA floats (non-finite points are skipped); guess: row-major 4x4 or
 * NULL for the identity.  Outputs (host, in both entry points): transformation[16] row-major
 * (getFinalTransformation), *fitness (getFitnessScore(): mean squared distance of every finite
 * transformed source point to its nearest target point, DBL_MAX without any), *converged
 * (hasConverged), *iterations, *state.  ax/ay/az (nullable, ns floats each; device memory for
 * pfx_icp_dev): the aligned source cloud, i.e. the cloud align() hands back.  Both calls return
 * after the last iteration (one host synchronisation per iteration, two where the mean squared
 * error cannot be summed exactly in parallel and one lane runs PCL's loop).  A null pointer, a negative
 * count, max_correspondence_distance <= 0, max_iterations < 0 or a NaN parameter:
 * PFX_ERR_INVALID.  Statistics: "icp_iterations", "icp_state", "icp_correspondences" (last
 * iteration), "icp_nn_rounds" (most grid rounds one search needed), "icp_brute" (queries that fell
 * to the exhaustive scan, whole call), "icp_exact_sum" (1: every double sum took the exact
 * integer route). */
pfx_status pfx_icp(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, const float* tx,
                   const float* ty, const float* tz, int64_t nt, const pfx_icp_params* params, const float* guess,
                   float* transformation, double* fitness, int32_t* converged, int32_t* iterations, int32_t* state,
                   float* ax, float* ay, float* az);
pfx_status pfx_icp_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, int64_t ns,
                       const float* d_tx, const float* d_ty, const float* d_tz, int64_t nt,
                       const pfx_icp_params* params, const float* guess, float* transformation, double* fitness,
                       int32_t* converged, int32_t* iterations, int32_t* state, float* d_ax, float* d_ay,
                       float* d_az);

/* ---- multi-GPU scan batch (SURVEY 8(e), configs[4]) ------------------------------------- */
/* Replaces the reference's per-scan loop for the (Narf, FPFH) pair (evaluation.cpp:272-852 over
 * Keypoints::compute, keypoints.h:199-231, and Features<FPFHSignature33>::compute,
 * features.h:175-196) for a C++ host with several GPUs in one process.  pfx_batch_create: the
 * devices (ordinals), two contexts and two streams per device, and an RCCL communicator over them
 * (ncclCommInitAll). */
typedef struct pfx_batch pfx_batch;
pfx_status pfx_batch_create(const int* devices, int n_devices, pfx_batch** out);
void pfx_batch_destroy(pfx_batch* batch);
const char* pfx_batch_last_error(const pfx_batch* batch);
/* n_scans host clouds (x[s], y[s], z[s], n[s] points; SoA float); scan s runs on device
 * s % n_devices: NARF keypoints (cam, params as pfx_narf_keypoints), the in-range pixel indices
 * mapped to cloud points (keypoints.h:229), normals of the whole cloud at normal_radius, FPFH at the
 * keypoints at feature_radius -- each device pipelines its scans over two streams.  The K_s x 33
 * descriptors and K_s cloud indices of every scan are gathered on the first device over RCCL and
 * copied out in scan order: rows[s] = K_s, scan s's rows start at sum_{t<s} K_t of desc
 * (cap_rows x 33) and idx (cap_rows).  Results equal the per-scan entry points bit for bit.
 * PFX_ERR_CAPACITY (rows filled in) when sum K_s > cap_rows. */
/* The batch's host-side plan (no device work; pfx_batch_narf_fpfh follows it): scan s runs on
 * device device_of_scan[s] = s % n_devices as that device's slot slot_of_scan[s] = s / n_devices
 * (its scans pipelined in slot order), and given each scan's descriptor rows K_s, its rows land at
 * row_offset[s] = sum_{t<s} K_t of the gathered output (row_offset has n_scans + 1 entries: the last
 * is the total).  Any output pointer may be NULL.  PFX_ERR_INVALID for n_scans < 0,
 * n_devices <= 0 or a negative K_s. */
pfx_status pfx_batch_plan(int n_scans, int n_devices, const int64_t* rows_per_scan, int32_t* device_of_scan,
                          int32_t* slot_of_scan, int64_t* row_offset);
pfx_status pfx_batch_narf_fpfh(pfx_batch* batch, int n_scans, const float* const* x, const float* const* y,
                               const float* const* z, const int64_t* n, const pfx_camera* cam,
                               const pfx_narf_params* params, double normal_radius, double feature_radius,
                               float* desc, int32_t* idx, int64_t cap_rows, int64_t* rows);

#ifdef __cplusplus
} /* extern "C" */
#endif
#endif /* PFX_H_ */
