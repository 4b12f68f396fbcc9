// pfx_api.hip -- the extern "C" boundary (include/pfx.h).  Host-pointer entry points stage
// through ctx-owned device buffers and call the stream-ordered *_dev implementations.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pfx_internal.h"

using pfx::Error;

#define PFX_API_BEGIN try {
#define PFX_API_END(ctx)                                            \
  }                                                                 \
  catch (const pfx::Error& e) {                                     \
    if (ctx) (ctx)->last_error = e.what();                          \
    return e.code;                                                  \
  }                                                                 \
  catch (const std::exception& e) {                                 \
    if (ctx) (ctx)->last_error = e.what();                          \
    return PFX_ERR_DEVICE;                                          \
  }                                                                 \
  return PFX_OK;

namespace {

void harvest_timing(pfx_ctx* ctx) {
  if (ctx->timer.pending.empty()) return;
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  for (auto& p : ctx->timer.pending) {
    float ms = 0.f;
    PFX_HIP(hipEventElapsedTime(&ms, p.a, p.b));
    auto& acc = ctx->timer.acc[p.name];
    acc.first += ms;
    acc.second += 1;
    ctx->timer.pool.push_back(p.a);
    ctx->timer.pool.push_back(p.b);
  }
  ctx->timer.pending.clear();
}

float* stage_in(pfx_ctx* ctx, const std::string& name, const float* host, int64_t count) {
  float* d = ctx->bufs[name].as<float>(count > 0 ? count : 1);
  if (count > 0) PFX_HIP(hipMemcpyAsync(d, host, sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
  return d;
}

// A coordinate triple staged under a name stem: "in_" -> in_x in_y in_z (the surface), "in_n" ->
// in_nx .. (its normals, or RIFT's gradients), "in_q" -> in_qx .. (the queries), "in_qn" -> in_qnx ..
// (their normals or axes).
struct Dev3 {
  float *x, *y, *z;
};
Dev3 stage3(pfx_ctx* ctx, const std::string& stem, const float* x, const float* y, const float* z, int64_t count) {
  return Dev3{stage_in(ctx, stem + "x", x, count), stage_in(ctx, stem + "y", y, count),
              stage_in(ctx, stem + "z", z, count)};
}

// nq rows of `width` elements back to the host, in stream order (host nullable: not wanted)
template <class T>
void rows_out(pfx_ctx* ctx, T* host, const T* dev, int64_t nq, int64_t width) {
  if (nq && host) PFX_HIP(hipMemcpyAsync(host, dev, sizeof(T) * nq * width, hipMemcpyDeviceToHost, ctx->stream));
}

void check_ctx(pfx_ctx* ctx) {
  if (!ctx) throw Error(PFX_ERR_INVALID, "null pfx_ctx");
  PFX_HIP(hipSetDevice(ctx->device));
  // the ctx-owned stream exists only once a call runs on it: a ctx re-pointed at the caller's
  // stream right after creation (the torch pipeline, the batch driver) never holds one, so it
  // takes no hardware queue (GPU_MAX_HW_QUEUES = 4 per process)
  if (ctx->on_own_stream && !ctx->own_stream) {
    PFX_HIP(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
  }
}

// ---- what the descriptor entry points are written from ----------------------------------------
// An argument rule (one *_rule per family, for its host and its device form alike) is written from
// all_set over the triples and pointers a side needs, and args_rule for what every family asks:
// counts >= 0, a side's pointers set where the side has rows, and `scalars_ok`, the radius test
// where the family has one.  A family's own rules follow it in the *_rule, with their own texts.
struct In3 {  // a caller's coordinate triple, host or device
  const float *x, *y, *z;
};
bool is_set(const void* p) { return p != nullptr; }
bool is_set(const In3& t) { return t.x && t.y && t.z; }
template <class... A>
bool all_set(const A&... a) {
  return (... && is_set(a));
}
void args_rule(const char* name, int64_t n_surface, bool surface_set, int64_t nq, bool queries_set,
               bool scalars_ok = true) {
  if (n_surface < 0 || nq < 0 || !scalars_ok || (n_surface && !surface_set) || (nq && !queries_set))
    throw Error(PFX_ERR_INVALID, std::string(name) + ": invalid arguments");
}

// The end of a host form: every output's nq rows back from its ctx-owned buffer in stream order,
// the stream drained, and the family's deferred reports resolved where it posts any (the host API
// reports at once)
struct Rows {
  template <class T>
  Rows(T* host, const T* dev, int64_t width) : host(host), dev(dev), row_bytes(sizeof(T) * width) {}
  void* host;  // nullable: not wanted
  const void* dev;
  size_t row_bytes;
};
constexpr pfx::ReportSlot kNoReports = pfx::kReportSlots;
void finish_host(pfx_ctx* ctx, int64_t nq, std::initializer_list<Rows> outs, pfx::ReportSlot first = kNoReports,
                 pfx::ReportSlot last = kNoReports) {
  for (const Rows& o : outs) rows_out(ctx, (char*)o.host, (const char*)o.dev, nq, (int64_t)o.row_bytes);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  if (first != kNoReports) pfx::reports_resolve(ctx, first, last);
}

// the host form of pfx_normals and pfx_normals_fast: stage, run `impl`, copy the four columns back
using NormalsImpl = void (*)(pfx_ctx*, const float*, const float*, const float*, int64_t, double, const float*, float*,
                             float*, float*, float*);
void normals_host(pfx_ctx* ctx, NormalsImpl impl, const char* what, const float* x, const float* y, const float* z,
                  int64_t n, double radius, const float viewpoint[3], float* nx, float* ny, float* nz,
                  float* curvature) {
  check_ctx(ctx);
  if (n < 0 || (n && (!x || !y || !z || !nx || !ny || !nz || !curvature)))
    throw Error(PFX_ERR_INVALID, std::string(what) + ": invalid arguments");
  const Dev3 d = stage3(ctx, "in_", x, y, z, n);
  float* o = ctx->buf("out_normals").as<float>(4 * n + 4);
  const float vp0[3] = {0.f, 0.f, 0.f};
  impl(ctx, d.x, d.y, d.z, n, radius, viewpoint ? viewpoint : vp0, o, o + n, o + 2 * n, o + 3 * n);
  rows_out(ctx, nx, o, n, 1);
  rows_out(ctx, ny, o + n, n, 1);
  rows_out(ctx, nz, o + 2 * n, n, 1);
  rows_out(ctx, curvature, o + 3 * n, n, 1);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
}

}  // namespace

extern "C" {

void pfx_narf_params_default(pfx_narf_params* p) {
  if (!p) return;
  p->support_size = -1.0f;
  p->max_no_of_interest_points = -1;
  p->min_distance_between_interest_points = 0.25f;
  p->optimal_distance_to_high_surface_change = 0.25f;
  p->min_interest_value = 0.45f;
  p->min_surface_change_score = 0.2f;
  p->do_non_maximum_suppression = 1;
  p->calculate_sparse_interest_image = 1;
  p->no_of_polynomial_approximations_per_point = 0;
  p->add_points_on_straight_edges = 0;
  p->pixel_radius_borders = 3;
  p->pixel_radius_plane_extraction = 2;
  p->pixel_radius_border_direction = 2;
  p->minimum_border_probability = 0.8f;
  p->pixel_radius_principal_curvature = 2;
}

void pfx_narf_desc_params_default(pfx_narf_desc_params* p) {
  if (!p) return;
  p->support_size = -1.0f;
  p->rotation_invariant = 1;
}

void pfx_camera_default(pfx_camera* c) {
  if (!c) return;
  c->width = 640;
  c->height = 480;
  c->center_x = 640.0f / 2.0f;
  c->center_y = 480.0f / 2.0f;
  c->focal_length_x = 525.0f;
  c->focal_length_y = 525.0f;
  for (int i = 0; i < 16; ++i) c->sensor_pose[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  c->coordinate_frame = 0;
  c->noise_level = 0.0f;
  c->min_range = 0.0f;
}

pfx_status pfx_ctx_create(int device, pfx_ctx** out) {
  if (!out) return PFX_ERR_INVALID;
  *out = nullptr;
  pfx_ctx* ctx = nullptr;
  try {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
      throw Error(PFX_ERR_DEVICE, std::string("no HIP device available: ") + hipGetErrorString(e));
    if (device < 0 || device >= count) throw Error(PFX_ERR_INVALID, "device ordinal out of range");
    ctx = new pfx_ctx();
    ctx->device = device;
    PFX_HIP(hipSetDevice(device));
    ctx->on_own_stream = true;  // created on first use (check_ctx)
    ctx->stats["pfh_cap_lds"] = pfx::pfh_cap_lds();
    ctx->stats["shot_color_cap_small"] = pfx::shot_color_cap_small();
    ctx->stats["spin_cap_small"] = pfx::spin_cap_small();
    ctx->stats["spin_chunk"] = pfx::spin_chunk();
    ctx->stats["rift_cap_small"] = pfx::rift_cap_small();
    ctx->stats["ispin_cap_small"] = pfx::ispin_cap_small();
    ctx->stats["ispin_tile_words"] = pfx::ispin_tile_words();
    ctx->stats["ispin_tile"] = pfx::ispin_tile(20);  // of the default 4 x 5 image
    ctx->stats["sc_cap_small"] = pfx::sc_cap_small();
    ctx->stats["moments_cap_small"] = pfx::moments_cap_small();
    ctx->stats["board_cap_small"] = pfx::board_cap_small();
    // grid builds by builder (pfx_grid.hip), and speculative counting builds that met a fat cell
    for (const char* s : {"grid_count_builds", "grid_sort_builds", "grid_hinted_sort_builds", "grid_fat_fallbacks"})
      ctx->stats[s] = 0;
    *out = ctx;
    return PFX_OK;
  } catch (const Error& e) {
    delete ctx;
    return e.code;
  }
}

void pfx_ctx_destroy(pfx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  pfx::narf_release(ctx);
  pfx::normals_release(ctx);
  pfx::keypoints_release(ctx);
  pfx::icp_release(ctx);
  ctx->grid_a.release();
  ctx->grid_b.release();
  for (auto& kv : ctx->bufs) kv.second.release();
  for (auto& p : ctx->timer.pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto e : ctx->timer.pool) (void)hipEventDestroy(e);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  if (ctx->side) (void)hipStreamDestroy(ctx->side);
  for (auto& e : ctx->fork_ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->spin_ev) (void)hipEventDestroy(ctx->spin_ev);
  if (ctx->host_rb) (void)hipHostFree(ctx->host_rb);
  if (ctx->host_scratch) (void)hipHostFree(ctx->host_scratch);
  if (ctx->reports.host) (void)hipHostFree(ctx->reports.host);
  delete ctx;
}

const char* pfx_last_error(const pfx_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null pfx_ctx"; }

pfx_status pfx_ctx_set_stream(pfx_ctx* ctx, void* hip_stream) {
  PFX_API_BEGIN
  check_ctx(ctx);
  harvest_timing(ctx);
  ctx->on_own_stream = false;
  ctx->stream = static_cast<hipStream_t>(hip_stream);  // NULL = HIP's null (legacy default) stream
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_use_own_stream(pfx_ctx* ctx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  harvest_timing(ctx);
  ctx->on_own_stream = true;
  check_ctx(ctx);
  ctx->stream = ctx->own_stream;
  PFX_API_END(ctx)
}

void* pfx_ctx_get_stream(pfx_ctx* ctx) {
  if (!ctx) return nullptr;
  try {
    check_ctx(ctx);
  } catch (const pfx::Error& e) {
    ctx->last_error = e.what();
    return nullptr;
  }
  return (void*)ctx->stream;
}

pfx_status pfx_ctx_trim(pfx_ctx* ctx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  // a split estimation still owes its lists check (normals_launch_dev): conclude it first, so
  // the outputs it launched are validated (and rerun if needed) before its state goes
  pfx::normals_finish_dev(ctx);
  ctx->lists_gate = nullptr;  // a borrowed event the next call must not wait on
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  pfx::reports_resolve(ctx);
  pfx::narf_release(ctx);
  pfx::normals_release(ctx);
  pfx::keypoints_release(ctx);
  pfx::icp_release(ctx);
  ctx->grid_a.release();
  ctx->grid_b.release();
  for (auto& kv : ctx->bufs) kv.second.release();
  ctx->prep_x = nullptr;
  ctx->prep_n = -1;
  ctx->prep_qx = nullptr;
  ctx->prep_nq = -1;
  ctx->fpfh_support = nullptr;
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_synchronize(pfx_ctx* ctx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  pfx::reports_resolve(ctx);  // deferred statistics / capacity errors of the stream-ordered calls
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_set_timing(pfx_ctx* ctx, int enable) {
  PFX_API_BEGIN
  check_ctx(ctx);
  harvest_timing(ctx);
  ctx->timer.enabled = enable != 0;
  ctx->timer.stages_only = enable == 2;
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_set_shared(pfx_ctx* ctx, int shared) {
  PFX_API_BEGIN
  check_ctx(ctx);
  ctx->shared_device = shared != 0;
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_reset_timing(pfx_ctx* ctx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  harvest_timing(ctx);
  ctx->timer.acc.clear();
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_kernel_time(pfx_ctx* ctx, const char* name, double* total_ms, int64_t* launches) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!name || !total_ms || !launches) throw Error(PFX_ERR_INVALID, "null argument");
  harvest_timing(ctx);
  auto it = ctx->timer.acc.find(name);
  *total_ms = it == ctx->timer.acc.end() ? 0.0 : it->second.first;
  *launches = it == ctx->timer.acc.end() ? 0 : it->second.second;
  PFX_API_END(ctx)
}

pfx_status pfx_ctx_last_stats(pfx_ctx* ctx, const char* what, int64_t* value) {
  PFX_API_BEGIN
  if (!ctx || !what || !value) throw Error(PFX_ERR_INVALID, "null argument");
  if (ctx->reports.any()) {
    PFX_HIP(hipStreamSynchronize(ctx->stream));
    pfx::reports_resolve(ctx);
  }
  auto it = ctx->stats.find(what);
  if (it == ctx->stats.end()) throw Error(PFX_ERR_INVALID, std::string("unknown stat ") + what);
  *value = it->second;
  PFX_API_END(ctx)
}

pfx_status pfx_radius_search(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                             const float* qx, const float* qy, const float* qz, int64_t nq, double radius,
                             int64_t* counts, int32_t* idx, float* d2, int64_t cap) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || nq < 0 || (n && (!x || !y || !z)) || (nq && (!qx || !qy || !qz || !counts)))
    throw Error(PFX_ERR_INVALID, "radius_search: invalid arguments");
  if (idx && (cap <= 0 || !d2)) throw Error(PFX_ERR_INVALID, "radius_search: idx needs cap > 0 and d2");
  float* dx = stage_in(ctx, "in_x", x, n);
  float* dy = stage_in(ctx, "in_y", y, n);
  float* dz = stage_in(ctx, "in_z", z, n);
  float* dqx = stage_in(ctx, "in_qx", qx, nq);
  float* dqy = stage_in(ctx, "in_qy", qy, nq);
  float* dqz = stage_in(ctx, "in_qz", qz, nq);
  int64_t* dc = ctx->buf("out_counts").as<int64_t>(nq + 1);
  int32_t* di = idx ? ctx->buf("out_idx").as<int32_t>(nq * cap + 1) : nullptr;
  float* dd = idx ? ctx->buf("out_d2").as<float>(nq * cap + 1) : nullptr;
  pfx::radius_search_dev(ctx, dx, dy, dz, n, dqx, dqy, dqz, nq, radius, dc, di, dd, cap);
  if (nq) PFX_HIP(hipMemcpyAsync(counts, dc, sizeof(int64_t) * nq, hipMemcpyDeviceToHost, ctx->stream));
  if (idx && nq) {
    PFX_HIP(hipMemcpyAsync(idx, di, sizeof(int32_t) * nq * cap, hipMemcpyDeviceToHost, ctx->stream));
    PFX_HIP(hipMemcpyAsync(d2, dd, sizeof(float) * nq * cap, hipMemcpyDeviceToHost, ctx->stream));
  }
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

static void knn_rule(In3 s, int64_t n, In3 q, int64_t nq, int32_t k, const int64_t* counts, const int32_t* idx,
                     const float* d2) {
  args_rule("knn_search", n, all_set(s), nq, all_set(q, counts, idx, d2));
  pfx::knn_k_rule(k, "knn_search");
  pfx::knn_count_rule(n, nq, "knn_search");
}

pfx_status pfx_knn_search_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                              const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq, int32_t k,
                              int64_t* d_counts, int32_t* d_idx, float* d_d2) {
  PFX_API_BEGIN
  check_ctx(ctx);
  knn_rule({d_x, d_y, d_z}, n, {d_qx, d_qy, d_qz}, nq, k, d_counts, d_idx, d_d2);
  pfx::knn_search_dev(ctx, d_x, d_y, d_z, n, d_qx, d_qy, d_qz, nq, k, d_counts, d_idx, d_d2);
  PFX_API_END(ctx)
}

pfx_status pfx_knn_search(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const float* qx,
                          const float* qy, const float* qz, int64_t nq, int32_t k, int64_t* counts, int32_t* idx,
                          float* d2) {
  PFX_API_BEGIN
  check_ctx(ctx);
  knn_rule({x, y, z}, n, {qx, qy, qz}, nq, k, counts, idx, d2);
  const Dev3 s = stage3(ctx, "in_", x, y, z, n), q = stage3(ctx, "in_q", qx, qy, qz, nq);
  int64_t* dc = ctx->buf("out_counts").as<int64_t>(nq + 1);
  int32_t* di = ctx->buf("out_idx").as<int32_t>(nq * k + 1);
  float* dd = ctx->buf("out_d2").as<float>(nq * k + 1);
  pfx::knn_search_dev(ctx, s.x, s.y, s.z, n, q.x, q.y, q.z, nq, k, dc, di, dd);
  finish_host(ctx, nq, {{counts, dc, 1}, {idx, di, k}, {d2, dd, k}});
  PFX_API_END(ctx)
}

static void normals_knn_rule(In3 p, int64_t n, int32_t k, const float* nx, const float* ny, const float* nz,
                             const float* curvature) {
  args_rule("normals_knn", n, all_set(p, nx, ny, nz, curvature), 0, true);
  pfx::knn_k_rule(k, "normals_knn");
  pfx::knn_count_rule(n, 0, "normals_knn");
}

pfx_status pfx_normals_knn_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                               int32_t k, const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                               float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  normals_knn_rule({d_x, d_y, d_z}, n, k, d_nx, d_ny, d_nz, d_curvature);
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_knn_dev(ctx, d_x, d_y, d_z, n, k, viewpoint ? viewpoint : vp0, d_nx, d_ny, d_nz, d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_knn(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, int32_t k,
                           const float viewpoint[3], float* nx, float* ny, float* nz, float* curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  normals_knn_rule({x, y, z}, n, k, nx, ny, nz, curvature);
  const Dev3 d = stage3(ctx, "in_", x, y, z, n);
  float* o = ctx->buf("out_normals").as<float>(4 * n + 4);
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_knn_dev(ctx, d.x, d.y, d.z, n, k, viewpoint ? viewpoint : vp0, o, o + n, o + 2 * n, o + 3 * n);
  finish_host(ctx, n, {{nx, o, 1}, {ny, o + n, 1}, {nz, o + 2 * n, 1}, {curvature, o + 3 * n, 1}});
  PFX_API_END(ctx)
}

pfx_status pfx_normals_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                           double radius, const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                           float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z || !d_nx || !d_ny || !d_nz || !d_curvature)))
    throw Error(PFX_ERR_INVALID, "normals: invalid arguments");
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_dev(ctx, d_x, d_y, d_z, n, radius, viewpoint ? viewpoint : vp0, d_nx, d_ny, d_nz, d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_fast_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                double radius, const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                                float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z || !d_nx || !d_ny || !d_nz || !d_curvature)))
    throw Error(PFX_ERR_INVALID, "normals_fast: invalid arguments");
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_fast_dev(ctx, d_x, d_y, d_z, n, radius, viewpoint ? viewpoint : vp0, d_nx, d_ny, d_nz, d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_fast(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, double radius,
                            const float viewpoint[3], float* nx, float* ny, float* nz, float* curvature) {
  PFX_API_BEGIN
  normals_host(ctx, pfx::normals_fast_dev, "normals_fast", x, y, z, n, radius, viewpoint, nx, ny, nz, curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_launch_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                  double radius, const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                                  float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z || !d_nx || !d_ny || !d_nz || !d_curvature)))
    throw Error(PFX_ERR_INVALID, "normals: invalid arguments");
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_launch_dev(ctx, d_x, d_y, d_z, n, radius, viewpoint ? viewpoint : vp0, d_nx, d_ny, d_nz, d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_grid_launch_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                       double radius) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z))) throw Error(PFX_ERR_INVALID, "normals grid: invalid arguments");
  pfx::normals_grid_launch_dev(ctx, d_x, d_y, d_z, n, radius);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_gate_dev(pfx_ctx* ctx, void* hip_event) {
  PFX_API_BEGIN
  check_ctx(ctx);
  ctx->lists_gate = static_cast<hipEvent_t>(hip_event);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_finish_dev(pfx_ctx* ctx, int32_t* rerun) {
  PFX_API_BEGIN
  check_ctx(ctx);
  const bool stood = pfx::normals_finish_dev(ctx);
  if (rerun) *rerun = stood ? 0 : 1;
  PFX_API_END(ctx)
}

pfx_status pfx_normals_prepare_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                   double radius) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z)))
    throw Error(PFX_ERR_INVALID, "normals prepare: invalid arguments");
  pfx::normals_prepare_dev(ctx, d_x, d_y, d_z, n, radius);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_subset_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                  double radius, const uint8_t* d_mask, int32_t want, const float viewpoint[3],
                                  float* d_nx, float* d_ny, float* d_nz, float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z || !d_mask || !d_nx || !d_ny || !d_nz || !d_curvature)))
    throw Error(PFX_ERR_INVALID, "normals subset: invalid arguments");
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_subset_dev(ctx, d_x, d_y, d_z, n, radius, d_mask, want, viewpoint ? viewpoint : vp0, d_nx, d_ny, d_nz,
                          d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_lists_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                 double radius, float* d_nx, float* d_ny, float* d_nz, float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0 || (n && (!d_x || !d_y || !d_z || !d_nx || !d_ny || !d_nz || !d_curvature)))
    throw Error(PFX_ERR_INVALID, "normals lists: invalid arguments");
  pfx::normals_lists_dev(ctx, d_x, d_y, d_z, n, radius, d_nx, d_ny, d_nz, d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals_chains_dev(pfx_ctx* ctx, pfx_ctx* lists_ctx, const uint8_t* d_mask, int32_t want,
                                  const float viewpoint[3], float* d_nx, float* d_ny, float* d_nz,
                                  float* d_curvature) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!lists_ctx || lists_ctx->device != ctx->device || !d_nx || !d_ny || !d_nz || !d_curvature)
    throw Error(PFX_ERR_INVALID, "normals chains: invalid arguments");
  const float vp0[3] = {0.f, 0.f, 0.f};
  pfx::normals_chains_dev(ctx, lists_ctx, d_mask, want, viewpoint ? viewpoint : vp0, d_nx, d_ny, d_nz, d_curvature);
  PFX_API_END(ctx)
}

pfx_status pfx_normals(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, double radius,
                       const float viewpoint[3], float* nx, float* ny, float* nz, float* curvature) {
  PFX_API_BEGIN
  normals_host(ctx, pfx::normals_dev, "normals", x, y, z, n, radius, viewpoint, nx, ny, nz, curvature);
  PFX_API_END(ctx)
}

// FPFH's rule, with no radius test at the boundary.  `queries_set`: the device forms always need the
// query arrays, the host form stages none under same_as_surface.
static void fpfh_rule(In3 s, In3 n, int64_t n_surface, bool queries_set, int64_t nq, int same_as_surface,
                      const float* out) {
  args_rule("fpfh", n_surface, all_set(s, n), nq, queries_set && out);
  if (same_as_surface && nq != n_surface)
    throw Error(PFX_ERR_INVALID, "fpfh: same_as_surface requires nq == n_surface");
}

static void fpfh_dev_checked(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                             const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                             const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq,
                             int same_as_surface, double radius, float* d_out, bool after_normals) {
  check_ctx(ctx);
  fpfh_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, n_surface, all_set(d_qx, d_qy, d_qz), nq, same_as_surface,
            d_out);
  pfx::fpfh_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nq, same_as_surface,
                radius, d_out, after_normals);
}

pfx_status pfx_fpfh_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                        const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                        const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq,
                        int same_as_surface, double radius, float* d_out) {
  PFX_API_BEGIN
  fpfh_dev_checked(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nq, same_as_surface,
                   radius, d_out, false);
  PFX_API_END(ctx)
}

pfx_status pfx_fpfh_after_normals_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                      const float* d_snx, const float* d_sny, const float* d_snz,
                                      int64_t n_surface, const float* d_qx, const float* d_qy,
                                      const float* d_qz, int64_t nq, int same_as_surface, double radius,
                                      float* d_out) {
  PFX_API_BEGIN
  fpfh_dev_checked(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nq, same_as_surface,
                   radius, d_out, true);
  PFX_API_END(ctx)
}

pfx_status pfx_fpfh_prepare_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                int64_t n_surface, double radius) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n_surface < 0 || !(radius > 0.0) || (n_surface && (!d_sx || !d_sy || !d_sz)))
    throw Error(PFX_ERR_INVALID, "fpfh_prepare: invalid arguments");
  pfx::fpfh_prepare_dev(ctx, d_sx, d_sy, d_sz, n_surface, radius);
  PFX_API_END(ctx)
}

pfx_status pfx_fpfh_prepare_queries_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                        int64_t n_surface, const float* d_qx, const float* d_qy,
                                        const float* d_qz, int64_t nq, double radius) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n_surface < 0 || nq < 0 || !(radius > 0.0) || (n_surface && (!d_sx || !d_sy || !d_sz)) ||
      (nq && (!d_qx || !d_qy || !d_qz)))
    throw Error(PFX_ERR_INVALID, "fpfh_prepare_queries: invalid arguments");
  pfx::fpfh_prepare_queries_dev(ctx, d_sx, d_sy, d_sz, n_surface, d_qx, d_qy, d_qz, nq, radius);
  PFX_API_END(ctx)
}

pfx_status pfx_fpfh(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                    const float* sny, const float* snz, int64_t n_surface, const float* qx, const float* qy,
                    const float* qz, int64_t nq, int same_as_surface, double radius, float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  fpfh_rule({sx, sy, sz}, {snx, sny, snz}, n_surface, same_as_surface || all_set(qx, qy, qz), nq, same_as_surface,
            out);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
  const Dev3 q = same_as_surface ? s : stage3(ctx, "in_q", qx, qy, qz, nq);
  float* dout = ctx->buf("out_fpfh").as<float>(nq * 33 + 1);
  pfx::fpfh_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, nq, same_as_surface, radius, dout);
  finish_host(ctx, nq, {{out, dout, 33}}, pfx::kRepFpfh, pfx::kRepFpfh);
  PFX_API_END(ctx)
}

pfx_status pfx_fpfh_support_mask_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                     int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz,
                                     int64_t nq, double radius, uint8_t* d_mask) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n_surface < 0 || nq < 0 || (n_surface && (!d_sx || !d_sy || !d_sz || !d_mask)) ||
      (nq && (!d_qx || !d_qy || !d_qz)))
    throw Error(PFX_ERR_INVALID, "fpfh support mask: invalid arguments");
  pfx::fpfh_support_mask_dev(ctx, d_sx, d_sy, d_sz, n_surface, d_qx, d_qy, d_qz, nq, radius, d_mask);
  PFX_API_END(ctx)
}

pfx_status pfx_fpfh_support_ball_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                     int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz,
                                     int64_t nq, double radius, uint8_t* d_mask) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n_surface < 0 || nq < 0 || (n_surface && (!d_sx || !d_sy || !d_sz || !d_mask)) ||
      (nq && (!d_qx || !d_qy || !d_qz)))
    throw Error(PFX_ERR_INVALID, "fpfh support ball: invalid arguments");
  pfx::fpfh_support_ball_dev(ctx, d_sx, d_sy, d_sz, n_surface, d_qx, d_qy, d_qz, nq, radius, d_mask);
  PFX_API_END(ctx)
}

// SHOT's rule, with no radius test at the boundary
static void shot_rule(In3 s, In3 n, int64_t n_surface, In3 q, int64_t nq, const float* desc, const float* rf) {
  args_rule("shot", n_surface, all_set(s, n), nq, all_set(q, desc, rf));
}

pfx_status pfx_shot_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                        const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                        const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq, double radius,
                        float* d_desc, float* d_rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  shot_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, n_surface, {d_qx, d_qy, d_qz}, nq, d_desc, d_rf);
  pfx::shot_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nq, radius, d_desc, d_rf);
  PFX_API_END(ctx)
}

pfx_status pfx_shot(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                    const float* sny, const float* snz, int64_t n_surface, const float* qx, const float* qy,
                    const float* qz, int64_t nq, double radius, float* desc, float* rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  shot_rule({sx, sy, sz}, {snx, sny, snz}, n_surface, {qx, qy, qz}, nq, desc, rf);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
  const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq);
  float* ddesc = ctx->buf("out_shot").as<float>(nq * 352 + 1);
  float* drf = ctx->buf("out_rf").as<float>(nq * 9 + 1);
  pfx::shot_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, nq, radius, ddesc, drf);
  finish_host(ctx, nq, {{desc, ddesc, 352}, {rf, drf, 9}});  // (SHOT posts no reports)
  PFX_API_END(ctx)
}

static void shot_color_rule(In3 s, In3 n, const uint32_t* srgb, int64_t n_surface, In3 q, const uint32_t* qrgb,
                            int64_t nq, double radius, const float* desc, const float* rf) {
  args_rule("shot_color", n_surface, all_set(s, n, srgb), nq, all_set(q, qrgb, desc, rf), radius > 0.0);
}

pfx_status pfx_shot_color_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                              const float* d_snx, const float* d_sny, const float* d_snz,
                              const uint32_t* d_srgb, int64_t n_surface, const float* d_qx,
                              const float* d_qy, const float* d_qz, const uint32_t* d_qrgb, int64_t nq,
                              double radius, float* d_desc, float* d_rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  shot_color_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, d_srgb, n_surface, {d_qx, d_qy, d_qz}, d_qrgb, nq,
                  radius, d_desc, d_rf);
  pfx::shot_color_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, d_srgb, n_surface, d_qx, d_qy, d_qz, d_qrgb, nq,
                      radius, d_desc, d_rf);
  PFX_API_END(ctx)
}

pfx_status pfx_shot_color(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                          const float* sny, const float* snz, const uint32_t* srgb, int64_t n_surface,
                          const float* qx, const float* qy, const float* qz, const uint32_t* qrgb, int64_t nq,
                          double radius, float* desc, float* rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  shot_color_rule({sx, sy, sz}, {snx, sny, snz}, srgb, n_surface, {qx, qy, qz}, qrgb, nq, radius, desc, rf);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
  // (the packed colours are staged as the 32-bit words they are)
  float* drgb = stage_in(ctx, "in_rgb", reinterpret_cast<const float*>(srgb), n_surface);
  const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq);
  float* dqrgb = stage_in(ctx, "in_qrgb", reinterpret_cast<const float*>(qrgb), nq);
  float* ddesc = ctx->buf("out_shot_color").as<float>(nq * 1344 + 1);
  float* drf = ctx->buf("out_rf").as<float>(nq * 9 + 1);
  pfx::shot_color_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, reinterpret_cast<const uint32_t*>(drgb), n_surface, q.x, q.y,
                      q.z, reinterpret_cast<const uint32_t*>(dqrgb), nq, radius, ddesc, drf);
  finish_host(ctx, nq, {{desc, ddesc, 1344}, {rf, drf, 9}});  // (SHOT colour posts no reports)
  PFX_API_END(ctx)
}

static void pfh_rule(In3 s, In3 n, int64_t n_surface, In3 q, int64_t nq, double radius, const float* out) {
  args_rule("pfh", n_surface, all_set(s, n), nq, all_set(q, out), radius > 0.0);
}

pfx_status pfx_pfh_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, const float* d_snx,
                       const float* d_sny, const float* d_snz, int64_t n_surface, const float* d_qx,
                       const float* d_qy, const float* d_qz, int64_t nq, double radius, float* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  pfh_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, n_surface, {d_qx, d_qy, d_qz}, nq, radius, d_out);
  pfx::pfh_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nq, radius, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_pfh(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                   const float* sny, const float* snz, int64_t n_surface, const float* qx, const float* qy,
                   const float* qz, int64_t nq, double radius, float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  pfh_rule({sx, sy, sz}, {snx, sny, snz}, n_surface, {qx, qy, qz}, nq, radius, out);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
  const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq);
  float* dout = ctx->buf("out_pfh").as<float>(nq * 125 + 1);
  pfx::pfh_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, nq, radius, dout);
  finish_host(ctx, nq, {{out, dout, 125}}, pfx::kRepPfh, pfx::kRepPfh);
  PFX_API_END(ctx)
}

void pfx_spin_params_default(pfx_spin_params* p) {
  if (!p) return;
  p->image_width = 8;
  p->support_angle_cos = 0.0;
  p->min_pts_neighb = 0;
  p->radial = 0;
  p->angular = 0;
}

// (the surface normals are optional: needed only under a support angle)
static void spin_rule(In3 s, In3 n, int64_t n_surface, In3 q, In3 qn, int64_t nq, double radius,
                      const pfx_spin_params* p, const float* out) {
  args_rule("spin_image", n_surface, all_set(s), nq, all_set(q, qn, out), p && radius > 0.0);
  if (p->radial != 0 || p->angular != 0)
    throw Error(PFX_ERR_UNSUPPORTED, "spin_image: the radial structure and the angular domain are not supported");
  if (p->image_width < 1 || p->image_width > 16)
    throw Error(PFX_ERR_INVALID, "spin_image: image_width must be in [1, 16]");
  if (!(p->support_angle_cos >= 0.0 && p->support_angle_cos <= 1.0))
    throw Error(PFX_ERR_INVALID, "spin_image: support_angle_cos must be in [0, 1]");
  if (p->min_pts_neighb < 0) throw Error(PFX_ERR_INVALID, "spin_image: min_pts_neighb must be >= 0");
  if (p->support_angle_cos > 0.0 && n_surface && !all_set(n))
    throw Error(PFX_ERR_INVALID, "spin_image: a support angle needs the surface normals");
}

pfx_status pfx_spin_image_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                              const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                              const float* d_qx, const float* d_qy, const float* d_qz, const float* d_qnx,
                              const float* d_qny, const float* d_qnz, int64_t nq, double radius,
                              const pfx_spin_params* params, float* d_out, double* d_raw, double* d_sums) {
  PFX_API_BEGIN
  check_ctx(ctx);
  spin_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, n_surface, {d_qx, d_qy, d_qz}, {d_qnx, d_qny, d_qnz}, nq,
            radius, params, d_out);
  pfx::spin_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, d_qnx, d_qny, d_qnz, nq,
                radius, *params, d_out, d_raw, d_sums);
  PFX_API_END(ctx)
}

pfx_status pfx_spin_image(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                          const float* sny, const float* snz, int64_t n_surface, const float* qx, const float* qy,
                          const float* qz, const float* qnx, const float* qny, const float* qnz, int64_t nq,
                          double radius, const pfx_spin_params* params, float* out, double* raw, double* sums) {
  PFX_API_BEGIN
  check_ctx(ctx);
  spin_rule({sx, sy, sz}, {snx, sny, snz}, n_surface, {qx, qy, qz}, {qnx, qny, qnz}, nq, radius, params, out);
  const bool normals = params->support_angle_cos > 0.0 && n_surface;
  const int64_t S = (int64_t)(params->image_width + 1) * (2 * params->image_width + 1);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface);
  const Dev3 n = normals ? stage3(ctx, "in_n", snx, sny, snz, n_surface) : Dev3{nullptr, nullptr, nullptr};
  const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq), a = stage3(ctx, "in_qn", qnx, qny, qnz, nq);
  float* dout = ctx->buf("out_spin").as<float>(nq * S + 1);
  double* draw = raw ? ctx->buf("out_spin_raw").as<double>(nq * S + 1) : nullptr;
  double* dsums = sums ? ctx->buf("out_spin_sums").as<double>(nq + 1) : nullptr;
  pfx::spin_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, a.x, a.y, a.z, nq, radius, *params, dout,
                draw, dsums);
  finish_host(ctx, nq, {{out, dout, S}, {raw, draw, S}, {sums, dsums, 1}}, pfx::kRepSpin, pfx::kRepSpin);
  PFX_API_END(ctx)
}

// (`dev`: the device form tells the whole-cloud path by the pointers themselves)
static void igrad_rule(In3 s, const float* si, int64_t n_surface, In3 q, In3 qn, int64_t nq, int same, bool dev,
                       double radius, const float* out) {
  args_rule("intensity_gradient", n_surface, all_set(s, si), nq, all_set(q, qn, out), radius > 0.0);
  if (same && (nq != n_surface || (dev && (q.x != s.x || q.y != s.y || q.z != s.z))))
    throw Error(PFX_ERR_INVALID, "intensity_gradient: same_as_surface needs the queries to be the surface");
}

pfx_status pfx_intensity_gradient_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                      const float* d_si, int64_t n_surface, const float* d_qx, const float* d_qy,
                                      const float* d_qz, const float* d_qnx, const float* d_qny, const float* d_qnz,
                                      int64_t nq, int32_t same_as_surface, double radius, float* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  igrad_rule({d_sx, d_sy, d_sz}, d_si, n_surface, {d_qx, d_qy, d_qz}, {d_qnx, d_qny, d_qnz}, nq, same_as_surface,
             true, radius, d_out);
  pfx::igrad_dev(ctx, d_sx, d_sy, d_sz, d_si, n_surface, d_qx, d_qy, d_qz, d_qnx, d_qny, d_qnz, nq, same_as_surface,
                 radius, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_intensity_gradient(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* si,
                                  int64_t n_surface, const float* qx, const float* qy, const float* qz,
                                  const float* qnx, const float* qny, const float* qnz, int64_t nq,
                                  int32_t same_as_surface, double radius, float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  igrad_rule({sx, sy, sz}, si, n_surface, {qx, qy, qz}, {qnx, qny, qnz}, nq, same_as_surface, false, radius, out);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface);
  float* dsi = stage_in(ctx, "in_i", si, n_surface);
  // (the whole-cloud path reads the surface's own arrays as its queries)
  const Dev3 q = same_as_surface ? s : stage3(ctx, "in_q", qx, qy, qz, nq);
  const Dev3 n = stage3(ctx, "in_qn", qnx, qny, qnz, nq);
  float* dout = ctx->buf("out_igrad").as<float>(nq * 3 + 1);
  pfx::igrad_dev(ctx, s.x, s.y, s.z, dsi, n_surface, q.x, q.y, q.z, n.x, n.y, n.z, nq, same_as_surface, radius, dout);
  finish_host(ctx, nq, {{out, dout, 3}}, pfx::kRepIgrad, pfx::kRepRift);
  PFX_API_END(ctx)
}

static void rift_rule(In3 s, In3 g, int64_t n_surface, In3 c, int64_t nq, double radius, int D, int G,
                      const float* out) {
  args_rule("rift", n_surface, all_set(s, g), nq, all_set(c, out), radius > 0.0);
  if (D < 1 || D > 16 || G < 1 || G > 16)
    throw Error(PFX_ERR_INVALID, "rift: nr_distance_bins and nr_gradient_bins must be in [1, 16]");
}

pfx_status pfx_rift_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, const float* d_sgx,
                        const float* d_sgy, const float* d_sgz, int64_t n_surface, const float* d_cx,
                        const float* d_cy, const float* d_cz, int64_t nq, double radius, int32_t nr_distance_bins,
                        int32_t nr_gradient_bins, float* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  rift_rule({d_sx, d_sy, d_sz}, {d_sgx, d_sgy, d_sgz}, n_surface, {d_cx, d_cy, d_cz}, nq, radius, nr_distance_bins,
            nr_gradient_bins, d_out);
  pfx::rift_dev(ctx, d_sx, d_sy, d_sz, d_sgx, d_sgy, d_sgz, n_surface, d_cx, d_cy, d_cz, nq, radius,
                nr_distance_bins, nr_gradient_bins, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_rift(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* sgx,
                    const float* sgy, const float* sgz, int64_t n_surface, const float* cx, const float* cy,
                    const float* cz, int64_t nq, double radius, int32_t nr_distance_bins, int32_t nr_gradient_bins,
                    float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  rift_rule({sx, sy, sz}, {sgx, sgy, sgz}, n_surface, {cx, cy, cz}, nq, radius, nr_distance_bins, nr_gradient_bins,
            out);
  const int64_t S = (int64_t)nr_distance_bins * nr_gradient_bins;
  // (the gradients ride in the normals' buffers)
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), g = stage3(ctx, "in_n", sgx, sgy, sgz, n_surface);
  const Dev3 c = stage3(ctx, "in_q", cx, cy, cz, nq);
  float* dout = ctx->buf("out_rift").as<float>(nq * S + 1);
  pfx::rift_dev(ctx, s.x, s.y, s.z, g.x, g.y, g.z, n_surface, c.x, c.y, c.z, nq, radius, nr_distance_bins,
                nr_gradient_bins, dout);
  finish_host(ctx, nq, {{out, dout, S}}, pfx::kRepIgrad, pfx::kRepRift);
  PFX_API_END(ctx)
}

// (the bound on sigma keeps every int cast of the window in range)
static void ispin_rule(In3 s, const float* si, int64_t n_surface, In3 c, int64_t nq, double radius, int D, int I,
                       float sigma, const float* out) {
  args_rule("intensity_spin", n_surface, all_set(s, si), nq, all_set(c, out), radius > 0.0);
  if (D < 1 || D > 16 || I < 1 || I > 16)
    throw Error(PFX_ERR_INVALID, "intensity_spin: nr_distance_bins and nr_intensity_bins must be in [1, 16]");
  if (!(sigma >= 0.0f && sigma <= 1048576.0f))
    throw Error(PFX_ERR_INVALID, "intensity_spin: sigma must be in [0, 2^20]");
}

pfx_status pfx_intensity_spin_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                  const float* d_si, int64_t n_surface, const float* d_cx, const float* d_cy,
                                  const float* d_cz, int64_t nq, double radius, int32_t nr_distance_bins,
                                  int32_t nr_intensity_bins, float sigma, float* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  ispin_rule({d_sx, d_sy, d_sz}, d_si, n_surface, {d_cx, d_cy, d_cz}, nq, radius, nr_distance_bins,
             nr_intensity_bins, sigma, d_out);
  pfx::ispin_dev(ctx, d_sx, d_sy, d_sz, d_si, n_surface, d_cx, d_cy, d_cz, nq, radius, nr_distance_bins,
                 nr_intensity_bins, sigma, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_intensity_spin(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* si,
                              int64_t n_surface, const float* cx, const float* cy, const float* cz, int64_t nq,
                              double radius, int32_t nr_distance_bins, int32_t nr_intensity_bins, float sigma,
                              float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  ispin_rule({sx, sy, sz}, si, n_surface, {cx, cy, cz}, nq, radius, nr_distance_bins, nr_intensity_bins, sigma, out);
  const int64_t S = (int64_t)nr_distance_bins * nr_intensity_bins;
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface);
  float* dsi = stage_in(ctx, "in_i", si, n_surface);
  const Dev3 c = stage3(ctx, "in_q", cx, cy, cz, nq);
  float* dout = ctx->buf("out_ispin").as<float>(nq * S + 1);
  pfx::ispin_dev(ctx, s.x, s.y, s.z, dsi, n_surface, c.x, c.y, c.z, nq, radius, nr_distance_bins, nr_intensity_bins,
                 sigma, dout);
  finish_host(ctx, nq, {{out, dout, S}}, pfx::kRepIspin, pfx::kRepIspin);
  PFX_API_END(ctx)
}

static void moments_rule(In3 s, int64_t n_surface, In3 q, int64_t nq, double radius, const float* out) {
  args_rule("moment_invariants", n_surface, all_set(s), nq, all_set(q, out), radius > 0.0);
}

pfx_status pfx_moment_invariants_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                     int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz,
                                     int64_t nq, double radius, float* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  moments_rule({d_sx, d_sy, d_sz}, n_surface, {d_qx, d_qy, d_qz}, nq, radius, d_out);
  pfx::moments_dev(ctx, d_sx, d_sy, d_sz, n_surface, d_qx, d_qy, d_qz, nq, radius, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_moment_invariants(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                                 const float* qx, const float* qy, const float* qz, int64_t nq, double radius,
                                 float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  moments_rule({sx, sy, sz}, n_surface, {qx, qy, qz}, nq, radius, out);
  if (nq) {  // (without queries nothing is staged, run or resolved)
    const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), q = stage3(ctx, "in_q", qx, qy, qz, nq);
    float* dout = ctx->buf("out_moments").as<float>(nq * 3 + 1);
    pfx::moments_dev(ctx, s.x, s.y, s.z, n_surface, q.x, q.y, q.z, nq, radius, dout);
    finish_host(ctx, nq, {{out, dout, 3}}, pfx::kRepMoments, pfx::kRepPcurv);
  }
  PFX_API_END(ctx)
}

static void pcurv_rule(In3 s, In3 n, int64_t n_surface, In3 q, In3 qn, int64_t nq, double radius, const float* out) {
  args_rule("principal_curvatures", n_surface, all_set(s, n), nq, all_set(q, qn, out), radius > 0.0);
}

pfx_status pfx_principal_curvatures_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                        const float* d_snx, const float* d_sny, const float* d_snz,
                                        int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz,
                                        const float* d_qnx, const float* d_qny, const float* d_qnz, int64_t nq,
                                        double radius, float* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  pcurv_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, n_surface, {d_qx, d_qy, d_qz}, {d_qnx, d_qny, d_qnz}, nq,
             radius, d_out);
  pfx::pcurv_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, d_qnx, d_qny, d_qnz, nq,
                 radius, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_principal_curvatures(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz,
                                    const float* snx, const float* sny, const float* snz, int64_t n_surface,
                                    const float* qx, const float* qy, const float* qz, const float* qnx,
                                    const float* qny, const float* qnz, int64_t nq, double radius, float* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  pcurv_rule({sx, sy, sz}, {snx, sny, snz}, n_surface, {qx, qy, qz}, {qnx, qny, qnz}, nq, radius, out);
  if (nq) {  // (without queries nothing is staged, run or resolved)
    const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
    const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq), a = stage3(ctx, "in_qn", qnx, qny, qnz, nq);
    float* dout = ctx->buf("out_pcurv").as<float>(nq * 5 + 1);
    pfx::pcurv_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, a.x, a.y, a.z, nq, radius, dout);
    finish_host(ctx, nq, {{out, dout, 5}}, pfx::kRepMoments, pfx::kRepPcurv);
  }
  PFX_API_END(ctx)
}

void pfx_board_params_default(pfx_board_params* p) {
  if (!p) return;
  p->tangent_radius = 0.0f;
  p->margin_thresh = 0.85f;
  p->find_holes = 0;
  p->check_margin_array_size = 24;
  p->hole_size_prob_thresh = 0.2f;
  p->steep_thresh = 0.1f;
}

static void board_rule(In3 s, In3 n, int64_t n_surface, In3 q, int64_t nq, double radius, const pfx_board_params* p,
                       const float* rf) {
  args_rule("board_lrf", n_surface, all_set(s, n), nq, all_set(q, rf), p && radius > 0.0);
  if (!(p->tangent_radius >= 0.0f) || std::isinf(p->tangent_radius))
    throw Error(PFX_ERR_INVALID, "board_lrf: tangent_radius must be finite and >= 0");
  if (!(p->margin_thresh >= 0.0f) || std::isinf(p->margin_thresh))
    throw Error(PFX_ERR_INVALID, "board_lrf: margin_thresh must be finite and >= 0");
  if (p->find_holes != 0)
    throw Error(PFX_ERR_UNSUPPORTED, "board_lrf: find_holes is not supported (PCL seeds its angular bins from "
                                     "rand(), so the frames depend on the process's history)");
}

pfx_status pfx_board_lrf_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                             const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                             const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq, double radius,
                             const pfx_board_params* params, float* d_rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  board_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, n_surface, {d_qx, d_qy, d_qz}, nq, radius, params, d_rf);
  pfx::board_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nq, radius, *params, d_rf);
  PFX_API_END(ctx)
}

pfx_status pfx_board_lrf(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                         const float* sny, const float* snz, int64_t n_surface, const float* qx, const float* qy,
                         const float* qz, int64_t nq, double radius, const pfx_board_params* params, float* rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  board_rule({sx, sy, sz}, {snx, sny, snz}, n_surface, {qx, qy, qz}, nq, radius, params, rf);
  if (nq) {  // (without queries nothing is staged, run or resolved)
    const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
    const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq);
    float* drf = ctx->buf("out_board").as<float>(nq * 9 + 1);
    pfx::board_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, nq, radius, *params, drf);
    finish_host(ctx, nq, {{rf, drf, 9}}, pfx::kRepBoard, pfx::kRepBoard);
  }
  PFX_API_END(ctx)
}

static void boundary_rule(In3 s, int64_t n_surface, In3 q, In3 qn, int64_t nq, double radius, float angle_threshold,
                          const uint8_t* out) {
  args_rule("boundary", n_surface, all_set(s), nq, all_set(q, qn, out),
            radius > 0.0 && !std::isnan(angle_threshold));
  if (angle_threshold < (float)(M_PI / 64.0))
    throw Error(PFX_ERR_UNSUPPORTED, "boundary: angle_threshold is below pi / 64 (the kernel compares the angles "
                                     "across 256 bins and never within one: a gap below two bin widths could hide)");
}

pfx_status pfx_boundary_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, int64_t n_surface,
                            const float* d_qx, const float* d_qy, const float* d_qz, const float* d_qnx,
                            const float* d_qny, const float* d_qnz, int64_t nq, double radius, float angle_threshold,
                            uint8_t* d_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  boundary_rule({d_sx, d_sy, d_sz}, n_surface, {d_qx, d_qy, d_qz}, {d_qnx, d_qny, d_qnz}, nq, radius, angle_threshold,
                d_out);
  pfx::boundary_dev(ctx, d_sx, d_sy, d_sz, n_surface, d_qx, d_qy, d_qz, d_qnx, d_qny, d_qnz, nq, radius,
                    angle_threshold, d_out);
  PFX_API_END(ctx)
}

pfx_status pfx_boundary(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                        const float* qx, const float* qy, const float* qz, const float* qnx, const float* qny,
                        const float* qnz, int64_t nq, double radius, float angle_threshold, uint8_t* out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  boundary_rule({sx, sy, sz}, n_surface, {qx, qy, qz}, {qnx, qny, qnz}, nq, radius, angle_threshold, out);
  if (nq) {  // (without queries nothing is staged, run or resolved)
    const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), q = stage3(ctx, "in_q", qx, qy, qz, nq);
    const Dev3 a = stage3(ctx, "in_qn", qnx, qny, qnz, nq);
    uint8_t* dout = ctx->buf("out_boundary").as<uint8_t>(nq + 1);
    pfx::boundary_dev(ctx, s.x, s.y, s.z, n_surface, q.x, q.y, q.z, a.x, a.y, a.z, nq, radius, angle_threshold, dout);
    finish_host(ctx, nq, {{out, dout, 1}}, pfx::kRepBoundary, pfx::kRepBoundary);  // (Rows carries any row type)
  }
  PFX_API_END(ctx)
}

// The points are the surface side of the one argument rule; there is no query side.
static void smooth_clusters_rule(In3 p, In3 nrm, int64_t n, float tolerance, double eps_angle, int32_t min_points,
                                 const int32_t* labels, const int64_t* n_clusters) {
  args_rule("smooth_clusters", n, all_set(p, nrm, labels), 0, true, n_clusters != nullptr);
  if (!(tolerance > 0.0f)) throw Error(PFX_ERR_INVALID, "smooth_clusters: the tolerance must be > 0");
  if (std::isnan(eps_angle)) throw Error(PFX_ERR_INVALID, "smooth_clusters: eps_angle is NaN");
  if (min_points < 1) throw Error(PFX_ERR_INVALID, "smooth_clusters: min_points must be >= 1");
  if (n >= (int64_t(1) << 31)) throw Error(PFX_ERR_INVALID, "smooth_clusters: 2^31 points or more");
}

pfx_status pfx_smooth_clusters_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                   const float* d_nx, const float* d_ny, const float* d_nz, int64_t n,
                                   float tolerance, double eps_angle, int32_t min_points, int32_t* d_labels,
                                   int64_t* d_n_clusters) {
  PFX_API_BEGIN
  check_ctx(ctx);
  smooth_clusters_rule({d_x, d_y, d_z}, {d_nx, d_ny, d_nz}, n, tolerance, eps_angle, min_points, d_labels,
                       d_n_clusters);
  pfx::smooth_clusters_dev(ctx, d_x, d_y, d_z, d_nx, d_ny, d_nz, n, tolerance, eps_angle, min_points, d_labels,
                           d_n_clusters);
  PFX_API_END(ctx)
}

pfx_status pfx_smooth_clusters(pfx_ctx* ctx, const float* x, const float* y, const float* z, const float* nx,
                               const float* ny, const float* nz, int64_t n, float tolerance, double eps_angle,
                               int32_t min_points, int32_t* labels, int64_t* n_clusters) {
  PFX_API_BEGIN
  check_ctx(ctx);
  smooth_clusters_rule({x, y, z}, {nx, ny, nz}, n, tolerance, eps_angle, min_points, labels, n_clusters);
  const Dev3 p = stage3(ctx, "in_", x, y, z, n), a = stage3(ctx, "in_n", nx, ny, nz, n);
  int32_t* dlab = ctx->buf("out_labels").as<int32_t>(n + 1);
  int64_t* dn = ctx->buf("out_count").as<int64_t>(1);
  pfx::smooth_clusters_dev(ctx, p.x, p.y, p.z, a.x, a.y, a.z, n, tolerance, eps_angle, min_points, dlab, dn);
  PFX_HIP(hipMemcpyAsync(n_clusters, dn, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  finish_host(ctx, n, {{labels, (const int32_t*)dlab, 1}});
  PFX_API_END(ctx)
}

void pfx_cvfh_params_default(pfx_cvfh_params* p) {
  if (!p) return;
  const float leaf_size = 0.005f;
  p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0f;
  p->radius_normals = leaf_size * 3;
  p->cluster_tolerance = leaf_size * 3;
  p->eps_angle_threshold = 0.125f;
  p->curvature_threshold = 0.03f;
  p->min_points = 50;
  p->normalize_bins = 0;
}

// The surface is the surface side and the indices the query side of the one argument rule (NULL
// indices: every surface point, so the counts must agree); the outputs are needed where cap allows a
// row.  Then the family's own rules, with their own texts.
static void cvfh_rule(In3 s, In3 nrm, const float* curv, int64_t n_surface, const int32_t* indices, int64_t n_indices,
                      const pfx_cvfh_params* p, const float* out, int64_t cap, const int64_t* n_rows) {
  args_rule("cvfh", n_surface, all_set(s, nrm, curv), n_indices, true,
            p && n_rows && cap >= 0 && (cap == 0 || out) && (indices || n_indices == n_surface) &&
                (n_indices == 0 || n_surface > 0) && n_surface < (int64_t(1) << 31));
  if (!(p->radius_normals > 0.0f)) throw Error(PFX_ERR_INVALID, "cvfh: radius_normals must be > 0");
  if (!(p->cluster_tolerance > 0.0f)) throw Error(PFX_ERR_INVALID, "cvfh: cluster_tolerance must be > 0");
  if (std::isnan(p->eps_angle_threshold)) throw Error(PFX_ERR_INVALID, "cvfh: eps_angle_threshold is NaN");
  if (p->min_points < 1) throw Error(PFX_ERR_INVALID, "cvfh: min_points must be >= 1");
  if (n_indices > (int64_t(1) << 24))
    throw Error(PFX_ERR_CAPACITY, "cvfh: more than 2^24 indexed points (a float bin stops counting exactly)");
}

pfx_status pfx_cvfh_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, const float* d_snx,
                        const float* d_sny, const float* d_snz, const float* d_scurvature, int64_t n_surface,
                        const int32_t* d_indices, int64_t n_indices, const pfx_cvfh_params* params, float* d_out,
                        int64_t cap, int64_t* d_n_rows, float* d_centroids, float* d_dominant_normals,
                        int32_t* d_labels) {
  PFX_API_BEGIN
  check_ctx(ctx);
  cvfh_rule({d_sx, d_sy, d_sz}, {d_snx, d_sny, d_snz}, d_scurvature, n_surface, d_indices, n_indices, params, d_out,
            cap, d_n_rows);
  pfx::cvfh_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, d_scurvature, n_surface, d_indices, n_indices, *params,
                d_out, cap, d_n_rows, d_centroids, d_dominant_normals, d_labels);
  PFX_API_END(ctx)
}

pfx_status pfx_cvfh(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                    const float* sny, const float* snz, const float* scurvature, int64_t n_surface,
                    const int32_t* indices, int64_t n_indices, const pfx_cvfh_params* params, float* out, int64_t cap,
                    int64_t* n_rows, float* centroids, float* dominant_normals, int32_t* labels) {
  PFX_API_BEGIN
  check_ctx(ctx);
  cvfh_rule({sx, sy, sz}, {snx, sny, snz}, scurvature, n_surface, indices, n_indices, params, out, cap, n_rows);
  *n_rows = 0;
  if (n_indices) {  // (without points nothing is staged or run)
    if (indices)  // (checked here, before anything is copied; the device form checks in its filter)
      for (int64_t i = 0; i < n_indices; ++i)
        if (indices[i] < 0 || indices[i] >= n_surface)
          throw Error(PFX_ERR_INVALID, "cvfh: an index is outside the surface");
    const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), a = stage3(ctx, "in_n", snx, sny, snz, n_surface);
    const float* dcurv = stage_in(ctx, "in_curv", scurvature, n_surface);
    int32_t* didx = nullptr;
    if (indices) {
      didx = ctx->buf("in_indices").as<int32_t>(n_indices);
      PFX_HIP(hipMemcpyAsync(didx, indices, sizeof(int32_t) * n_indices, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a cluster has min_points points or more of the n_indices)
    const int64_t room = std::min<int64_t>(cap, std::max<int64_t>(1, n_indices / params->min_points));
    float* dout = ctx->buf("out_cvfh").as<float>(room * (PFX_CVFH_DIM + 6) + 1);
    float *dcen = dout + room * PFX_CVFH_DIM, *ddn = dcen + room * 3;
    int32_t* dlab = ctx->buf("out_labels").as<int32_t>(n_indices + 1);
    int64_t* dn = ctx->buf("out_count").as<int64_t>(1);
    try {
      *n_rows = pfx::cvfh_dev(ctx, s.x, s.y, s.z, a.x, a.y, a.z, dcurv, n_surface, didx, n_indices, *params, dout,
                              room, dn, dcen, ddn, dlab);
    } catch (const Error& e) {
      if (e.code != PFX_ERR_CAPACITY) throw;
      PFX_HIP(hipMemcpyAsync(n_rows, dn, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
      PFX_HIP(hipStreamSynchronize(ctx->stream));
      throw;
    }
    rows_out(ctx, labels, (const int32_t*)dlab, n_indices, 1);
    finish_host(ctx, *n_rows, {{out, (const float*)dout, PFX_CVFH_DIM}, {centroids, (const float*)dcen, 3},
                               {dominant_normals, (const float*)ddn, 3}});
  } else {
    for (const char* st : {"cvfh_filtered", "cvfh_clusters", "cvfh_edges", "cvfh_cc_rounds", "cvfh_rows"})
      ctx->stats[st] = 0;
  }
  PFX_API_END(ctx)
}

// Both shape contexts' rule.  `normals_set`: the 3DSC needs the surface normals, the USC has none;
// `frames_set`: the USC needs the frames, the 3DSC has none.
static void sc_rule(const char* what, In3 s, bool normals_set, int64_t n_surface, In3 q, bool frames_set, int64_t nq,
                    double radius, double min_radius, double density_radius, const float* desc, const float* rf) {
  args_rule(what, n_surface, all_set(s) && normals_set, nq, all_set(q, desc, rf) && frames_set);
  if (!(radius > 0.0) || !(min_radius > 0.0) || !(density_radius > 0.0))
    throw Error(PFX_ERR_INVALID, std::string(what) + ": every radius must be > 0");
  if (radius < min_radius)  // PCL's initCompute refuses this
    throw Error(PFX_ERR_INVALID, std::string(what) + ": the search radius is below the minimal radius");
}

pfx_status pfx_shape_context_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                                 const float* d_snx, const float* d_sny, const float* d_snz, int64_t n_surface,
                                 const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq,
                                 double radius, double min_radius, double point_density_radius,
                                 const float* d_rnd, float* d_desc, float* d_rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  sc_rule("shape_context", {d_sx, d_sy, d_sz}, all_set(d_snx, d_sny, d_snz), n_surface, {d_qx, d_qy, d_qz}, true, nq,
          radius, min_radius, point_density_radius, d_desc, d_rf);
  pfx::sc_dev(ctx, d_sx, d_sy, d_sz, d_snx, d_sny, d_snz, n_surface, d_qx, d_qy, d_qz, nullptr, nq, radius,
              min_radius, point_density_radius, d_rnd, d_desc, d_rf);
  PFX_API_END(ctx)
}

pfx_status pfx_shape_context(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                             const float* sny, const float* snz, int64_t n_surface, const float* qx,
                             const float* qy, const float* qz, int64_t nq, double radius, double min_radius,
                             double point_density_radius, const float* rnd, float* desc, float* rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  sc_rule("shape_context", {sx, sy, sz}, all_set(snx, sny, snz), n_surface, {qx, qy, qz}, true, nq, radius,
          min_radius, point_density_radius, desc, rf);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), n = stage3(ctx, "in_n", snx, sny, snz, n_surface);
  const Dev3 q = stage3(ctx, "in_q", qx, qy, qz, nq);
  float* drnd = rnd ? stage_in(ctx, "in_sc_rnd", rnd, 3 * nq) : nullptr;
  float* ddesc = ctx->buf("out_sc").as<float>(nq * 1980 + 1);
  float* drf = ctx->buf("out_sc_rf").as<float>(nq * 9 + 1);
  pfx::sc_dev(ctx, s.x, s.y, s.z, n.x, n.y, n.z, n_surface, q.x, q.y, q.z, nullptr, nq, radius, min_radius,
              point_density_radius, drnd, ddesc, drf);
  finish_host(ctx, nq, {{desc, ddesc, 1980}, {rf, drf, 9}}, pfx::kRepSc, pfx::kRepLrf);
  PFX_API_END(ctx)
}

pfx_status pfx_usc_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, int64_t n_surface,
                       const float* d_qx, const float* d_qy, const float* d_qz, const float* d_frames, int64_t nq,
                       double radius, double min_radius, double point_density_radius, float* d_desc,
                       float* d_rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  sc_rule("usc", {d_sx, d_sy, d_sz}, true, n_surface, {d_qx, d_qy, d_qz}, all_set(d_frames), nq, radius, min_radius,
          point_density_radius, d_desc, d_rf);
  pfx::sc_dev(ctx, d_sx, d_sy, d_sz, nullptr, nullptr, nullptr, n_surface, d_qx, d_qy, d_qz, d_frames, nq, radius,
              min_radius, point_density_radius, nullptr, d_desc, d_rf);
  PFX_API_END(ctx)
}

pfx_status pfx_usc(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                   const float* qx, const float* qy, const float* qz, const float* frames, int64_t nq,
                   double radius, double min_radius, double point_density_radius, float* desc, float* rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  sc_rule("usc", {sx, sy, sz}, true, n_surface, {qx, qy, qz}, all_set(frames), nq, radius, min_radius,
          point_density_radius, desc, rf);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), q = stage3(ctx, "in_q", qx, qy, qz, nq);
  float* dfr = stage_in(ctx, "in_sc_frames", frames, 9 * nq);
  float* ddesc = ctx->buf("out_sc").as<float>(nq * 1980 + 1);
  float* drf = ctx->buf("out_sc_rf").as<float>(nq * 9 + 1);
  // (sc_dev tells the USC by its frames, and without queries they may be null)
  if (nq)
    pfx::sc_dev(ctx, s.x, s.y, s.z, nullptr, nullptr, nullptr, n_surface, q.x, q.y, q.z, dfr, nq, radius, min_radius,
                point_density_radius, nullptr, ddesc, drf);
  finish_host(ctx, nq, {{desc, ddesc, 1980}, {rf, drf, 9}}, pfx::kRepSc, pfx::kRepLrf);
  PFX_API_END(ctx)
}

static void lrf_rule(In3 s, int64_t n_surface, In3 q, int64_t nq, double radius, const float* rf) {
  args_rule("shot_lrf", n_surface, all_set(s), nq, all_set(q, rf), radius > 0.0);
}

pfx_status pfx_shot_lrf_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz,
                            int64_t n_surface, const float* d_qx, const float* d_qy, const float* d_qz, int64_t nq,
                            double radius, float* d_rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  lrf_rule({d_sx, d_sy, d_sz}, n_surface, {d_qx, d_qy, d_qz}, nq, radius, d_rf);
  pfx::shot_lrf_dev(ctx, d_sx, d_sy, d_sz, n_surface, d_qx, d_qy, d_qz, nq, radius, d_rf);
  PFX_API_END(ctx)
}

pfx_status pfx_shot_lrf(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t n_surface,
                        const float* qx, const float* qy, const float* qz, int64_t nq, double radius, float* rf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  lrf_rule({sx, sy, sz}, n_surface, {qx, qy, qz}, nq, radius, rf);
  const Dev3 s = stage3(ctx, "in_", sx, sy, sz, n_surface), q = stage3(ctx, "in_q", qx, qy, qz, nq);
  float* drf = ctx->buf("out_sc_rf").as<float>(nq * 9 + 1);
  pfx::shot_lrf_dev(ctx, s.x, s.y, s.z, n_surface, q.x, q.y, q.z, nq, radius, drf);
  finish_host(ctx, nq, {{rf, drf, 9}}, pfx::kRepSc, pfx::kRepLrf);
  PFX_API_END(ctx)
}

pfx_status pfx_rng_uniform01(uint32_t seed, int64_t skip, int64_t n, float* out) {
  if (skip < 0 || n < 0 || (n && !out)) return PFX_ERR_INVALID;
  pfx::rng_uniform01(seed, skip, n, out);
  return PFX_OK;
}

pfx_status pfx_range_image_planar(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                  const pfx_camera* cam, float* out_points) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!cam || !out_points || n < 0 || cam->width <= 0 || cam->height <= 0)
    throw Error(PFX_ERR_INVALID, "range_image: invalid arguments");
  float* dx = stage_in(ctx, "in_x", x, n);
  float* dy = stage_in(ctx, "in_y", y, n);
  float* dz = stage_in(ctx, "in_z", z, n);
  int64_t npx = (int64_t)cam->width * cam->height;
  float4* d = ctx->buf("out_ri").as<float4>(npx);
  pfx::range_image_dev(ctx, dx, dy, dz, n, *cam, d);
  PFX_HIP(hipMemcpyAsync(out_points, d, sizeof(float4) * npx, hipMemcpyDeviceToHost, ctx->stream));
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

pfx_status pfx_narf_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                  const pfx_camera* cam, const pfx_narf_params* params, int32_t* out, int64_t cap,
                                  int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!cam || !params || !n_out || n < 0 || (cap > 0 && !out))
    throw Error(PFX_ERR_INVALID, "narf: invalid arguments");
  std::vector<int32_t> kp;
  pfx::narf_dev(ctx, d_x, d_y, d_z, n, *cam, *params, kp);
  *n_out = (int64_t)kp.size();
  if ((int64_t)kp.size() > cap) throw Error(PFX_ERR_CAPACITY, "narf: output capacity too small");
  if (!kp.empty()) std::memcpy(out, kp.data(), sizeof(int32_t) * kp.size());
  PFX_API_END(ctx)
}

pfx_status pfx_narf_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                              const pfx_camera* cam, const pfx_narf_params* params, int32_t* out, int64_t cap,
                              int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (n < 0) throw Error(PFX_ERR_INVALID, "narf: invalid arguments");
  float* dx = stage_in(ctx, "in_x", x, n);
  float* dy = stage_in(ctx, "in_y", y, n);
  float* dz = stage_in(ctx, "in_z", z, n);
  pfx_status s = pfx_narf_keypoints_dev(ctx, dx, dy, dz, n, cam, params, out, cap, n_out);
  if (s != PFX_OK) return s;
  PFX_API_END(ctx)
}

pfx_status pfx_narf_debug_image(pfx_ctx* ctx, const char* which, void* out, int64_t count) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!which || !out) throw Error(PFX_ERR_INVALID, "narf_debug: null argument");
  pfx::narf_debug(ctx, which, out, count);
  PFX_API_END(ctx)
}

// The cloud is the surface side and pixel_idx the query side of the one argument rule; the outputs
// are needed where cap allows a row.  Then the family's own rules: the camera's.
static void narf_desc_rule(In3 c, int64_t n, const pfx_camera* cam, const int32_t* pixel_idx, int64_t nk,
                           const pfx_narf_desc_params* p, const float* desc, const float* pose, const int32_t* row_key,
                           int64_t cap, const int64_t* n_out) {
  args_rule("narf_descriptors", n, all_set(c), nk, all_set(pixel_idx),
            cam && p && n_out && cap >= 0 && (cap == 0 || all_set(desc, pose, row_key)) && nk <= (int64_t(1) << 28) &&
                p->support_size > 0.0f);  // (a NaN support_size fails the comparison)
  pfx::narf_camera_rule(*cam, "narf_descriptors");
}

pfx_status pfx_narf_descriptors_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                    const pfx_camera* cam, const int32_t* d_pixel_idx, int64_t nk,
                                    const pfx_narf_desc_params* params, float* d_desc, float* d_pose,
                                    int32_t* d_row_key, int64_t cap, int64_t* d_n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  narf_desc_rule({d_x, d_y, d_z}, n, cam, d_pixel_idx, nk, params, d_desc, d_pose, d_row_key, cap, d_n_out);
  pfx::narf_desc_dev(ctx, d_x, d_y, d_z, n, *cam, d_pixel_idx, nk, *params, d_desc, d_pose, d_row_key, cap, d_n_out);
  PFX_API_END(ctx)
}

pfx_status pfx_narf_descriptors(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                const pfx_camera* cam, const int32_t* pixel_idx, int64_t nk,
                                const pfx_narf_desc_params* params, float* desc, float* pose, int32_t* row_key,
                                int64_t cap, int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  narf_desc_rule({x, y, z}, n, cam, pixel_idx, nk, params, desc, pose, row_key, cap, n_out);
  *n_out = 0;
  if (nk) {  // (without entries nothing is staged, run or resolved)
    const Dev3 c = stage3(ctx, "in_", x, y, z, n);
    int32_t* dpix = ctx->buf("in_pixel_idx").as<int32_t>(nk);
    PFX_HIP(hipMemcpyAsync(dpix, pixel_idx, sizeof(int32_t) * nk, hipMemcpyHostToDevice, ctx->stream));
    const int64_t rows = std::min<int64_t>(cap, 5 * nk);  // (no entry gives more than 5)
    float* ddesc = ctx->buf("out_narf_desc").as<float>(rows * 48 + 1);
    float* dpose = ddesc + rows * 36;
    int32_t* dkey = ctx->buf("out_narf_desc_key").as<int32_t>(rows + 1);
    int64_t* dn = ctx->buf("out_count").as<int64_t>(1);
    pfx::narf_desc_dev(ctx, c.x, c.y, c.z, n, *cam, dpix, nk, *params, ddesc, dpose, dkey, rows, dn);
    PFX_HIP(hipMemcpyAsync(n_out, dn, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    finish_host(ctx, 0, {}, pfx::kRepNarfDesc, pfx::kRepNarfDesc);
    if (*n_out > cap) throw Error(PFX_ERR_CAPACITY, "narf_descriptors: output capacity too small");
    finish_host(ctx, *n_out, {{desc, ddesc, 36}, {pose, dpose, 12}, {row_key, dkey, 1}});
  }
  PFX_API_END(ctx)
}

static void point_indices_rule(In3 c, int64_t n, In3 k, int64_t nk, float tol, const int32_t* out, int64_t cap,
                               const int64_t* n_out) {
  args_rule("point_indices", n, all_set(c), nk, all_set(k),
            n_out && cap >= 0 && (cap == 0 || out) && !std::isnan(tol) && n < (int64_t(1) << 31));
}

pfx_status pfx_point_indices_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                                 const float* d_kx, const float* d_ky, const float* d_kz, int64_t nk, float tol,
                                 int32_t* d_out, int64_t cap, int64_t* d_n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  point_indices_rule({d_x, d_y, d_z}, n, {d_kx, d_ky, d_kz}, nk, tol, d_out, cap, d_n_out);
  pfx::point_indices_dev(ctx, d_x, d_y, d_z, n, d_kx, d_ky, d_kz, nk, tol, d_out, cap, d_n_out);
  PFX_API_END(ctx)
}

pfx_status pfx_point_indices(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const float* kx,
                             const float* ky, const float* kz, int64_t nk, float tol, int32_t* out, int64_t cap,
                             int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  point_indices_rule({x, y, z}, n, {kx, ky, kz}, nk, tol, out, cap, n_out);
  *n_out = 0;
  if (nk && n) {
    const Dev3 c = stage3(ctx, "in_", x, y, z, n), k = stage3(ctx, "in_q", kx, ky, kz, nk);
    const int64_t room = n > INT64_MAX / nk ? cap : std::min<int64_t>(cap, nk * n);  // (every pair at most)
    int32_t* dout = ctx->buf("out_point_indices").as<int32_t>(room + 1);
    int64_t* dn = ctx->buf("out_count").as<int64_t>(1);
    pfx::point_indices_dev(ctx, c.x, c.y, c.z, n, k.x, k.y, k.z, nk, tol, dout, room, dn);
    PFX_HIP(hipMemcpyAsync(n_out, dn, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    finish_host(ctx, 0, {});
    if (*n_out > cap) throw Error(PFX_ERR_CAPACITY, "point_indices: output capacity too small");
    finish_host(ctx, *n_out, {{out, dout, 1}});
  }
  PFX_API_END(ctx)
}

pfx_status pfx_grid_debug(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, double radius,
                          int32_t mode, int32_t* perm, uint32_t* skeys, float* sp, int32_t* cell_start,
                          int64_t cell_start_cap, double* params, int64_t* info) {
  PFX_API_BEGIN
  check_ctx(ctx);
  pfx::Grid& G = ctx->grid_a;
  hipStream_t st = ctx->stream;
  if (mode < -1 || mode > 1 || n < 0) throw Error(PFX_ERR_INVALID, "grid_debug: invalid arguments");
  if (mode >= 0) {
    if (n && (!x || !y || !z)) throw Error(PFX_ERR_INVALID, "grid_debug: null cloud");
    float* dx = stage_in(ctx, "dbg_x", x, n);
    float* dy = stage_in(ctx, "dbg_y", y, n);
    float* dz = stage_in(ctx, "dbg_z", z, n);
    pfx::build_grid(ctx, G, dx, dy, dz, n, radius, /*use_hint=*/mode == 1);
    int word = 0;
    const bool counted = G.counted;
    bool rerun = false;
    if (G.oob) {  // a caller's read of the validation word, and its exact rerun
      int* h = ctx->readback<int>();
      PFX_HIP(hipMemcpyAsync(h, G.oob, sizeof(int), hipMemcpyDeviceToHost, st));
      PFX_HIP(hipStreamSynchronize(st));
      word = *h;
      G.oob = nullptr;
      pfx::note_grid_word(ctx, G, word);
      if (word != 0) {
        pfx::build_grid(ctx, G, dx, dy, dz, n, radius);
        rerun = true;
      }
    }
    ctx->stats["grid_debug_word"] = word;
    ctx->stats["grid_debug_builder"] = counted ? 1 : 0;
    ctx->stats["grid_debug_rerun"] = rerun ? 1 : 0;
  } else if (n != G.n) {
    throw Error(PFX_ERR_INVALID, "grid_debug: the grid holds another point count");
  }
  const int64_t C = G.ncells;
  if (cell_start && cell_start_cap < C + 2) throw Error(PFX_ERR_CAPACITY, "grid_debug: cell_start buffer too small");
  if (perm && n) PFX_HIP(hipMemcpyAsync(perm, G.perm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  if (skeys && n) PFX_HIP(hipMemcpyAsync(skeys, G.skeys, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
  if (sp && n) PFX_HIP(hipMemcpyAsync(sp, G.sp, sizeof(float) * 4 * n, hipMemcpyDeviceToHost, st));
  if (cell_start)
    PFX_HIP(hipMemcpyAsync(cell_start, G.cell_start, sizeof(int32_t) * (C + 2), hipMemcpyDeviceToHost, st));
  PFX_HIP(hipStreamSynchronize(st));
  if (params) {
    params[0] = G.dox; params[1] = G.doy; params[2] = G.doz; params[3] = G.dinv;
  }
  if (info) {
    info[0] = G.nx; info[1] = G.ny; info[2] = G.nz; info[3] = C;
    info[4] = ctx->stats["grid_debug_word"];
    info[5] = ctx->stats["grid_debug_builder"];
    info[6] = ctx->stats["grid_debug_rerun"];
    info[7] = pfx::kGridFatCap;
  }
  PFX_API_END(ctx)
}

}  // extern "C"

// ---- keypoints.h:227-229: cloud_keypoints->points.push_back(cloud->points[keypoints[i]]) ----
namespace {
__global__ void k_gather_points(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                int64_t n, const int32_t* __restrict__ idx, int64_t k, float* __restrict__ kx,
                                float* __restrict__ ky, float* __restrict__ kz) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= k) return;
  int32_t p = idx[i];
  kx[i] = x[p];
  ky[i] = y[p];
  kz[i] = z[p];
}
}  // namespace

extern "C" pfx_status pfx_gather_points_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                            int64_t n, const int32_t* idx, int64_t k, float* d_kx, float* d_ky,
                                            float* d_kz, int64_t cap, int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!n_out || k < 0 || cap < 0 || (k && !idx)) throw Error(PFX_ERR_INVALID, "gather_points: invalid arguments");
  // the reference reads cloud->points[pixel_index] unchecked (out of bounds when the index is
  // >= cloud size); the guarded mapping keeps only in-range indices, in order
  std::vector<int32_t> keep;
  keep.reserve((size_t)k);
  for (int64_t i = 0; i < k; ++i)
    if (idx[i] >= 0 && idx[i] < n) keep.push_back(idx[i]);
  if ((int64_t)keep.size() > cap)
    throw Error(PFX_ERR_CAPACITY, "gather_points: " + std::to_string(keep.size()) + " in-range keypoints, output holds " +
                                      std::to_string(cap));
  *n_out = (int64_t)keep.size();
  if (keep.empty()) return PFX_OK;
  int32_t* d_idx = ctx->buf("gather_idx").as<int32_t>(keep.size());
  // through the context's pinned block (an async DMA copy; the stream is synchronised first, so
  // a previous call's copy out of that block has completed)
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  int32_t* h_idx = static_cast<int32_t*>(ctx->pinned(sizeof(int32_t) * keep.size()));
  std::memcpy(h_idx, keep.data(), sizeof(int32_t) * keep.size());
  PFX_HIP(hipMemcpyAsync(d_idx, h_idx, sizeof(int32_t) * keep.size(), hipMemcpyHostToDevice, ctx->stream));
  k_gather_points<<<(unsigned)pfx::ceil_div((int64_t)keep.size(), 256), 256, 0, ctx->stream>>>(
      d_x, d_y, d_z, n, d_idx, (int64_t)keep.size(), d_kx, d_ky, d_kz);
  pfx::check_launch("k_gather_points");
  PFX_API_END(ctx)
}

namespace {
void check_match_args(const float* src, int64_t ns, int64_t ss, const float* tgt, int64_t nt, int64_t ts,
                      int32_t dim) {
  if (dim <= 0 || ns < 0 || nt < 0 || ss < dim || ts < dim || (ns && !src) || (nt && !tgt))
    throw Error(PFX_ERR_INVALID, "correspondences: invalid arguments");
}
}  // namespace

extern "C" pfx_status pfx_nearest_descriptors_dev(pfx_ctx* ctx, const float* d_src, int64_t n_src,
                                                  int64_t src_stride, const float* d_tgt, int64_t n_tgt,
                                                  int64_t tgt_stride, int32_t dim, int32_t* d_s2t,
                                                  float* d_s2t_dist, int32_t* d_t2s, float* d_t2s_dist) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_match_args(d_src, n_src, src_stride, d_tgt, n_tgt, tgt_stride, dim);
  if (n_src && !d_s2t) throw Error(PFX_ERR_INVALID, "nearest_descriptors: null output");
  pfx::match_nearest_dev(ctx, d_src, n_src, src_stride, d_tgt, n_tgt, tgt_stride, dim, d_s2t, d_s2t_dist, d_t2s,
                         d_t2s_dist);
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_nearest_descriptors(pfx_ctx* ctx, const float* src, int64_t n_src, int64_t src_stride,
                                              const float* tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                                              int32_t* s2t, float* s2t_dist) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_match_args(src, n_src, src_stride, tgt, n_tgt, tgt_stride, dim);
  if (n_src && !s2t) throw Error(PFX_ERR_INVALID, "nearest_descriptors: null output");
  const int64_t cs = n_src ? (n_src - 1) * src_stride + dim : 0, ct = n_tgt ? (n_tgt - 1) * tgt_stride + dim : 0;
  float* ds = stage_in(ctx, "in_match_src", src, cs);
  float* dt = stage_in(ctx, "in_match_tgt", tgt, ct);
  int32_t* di = ctx->buf("out_match_i").as<int32_t>(n_src + 1);
  float* dd = ctx->buf("out_match_d").as<float>(n_src + 1);
  pfx::match_nearest_dev(ctx, ds, n_src, src_stride, dt, n_tgt, tgt_stride, dim, di, dd, nullptr, nullptr);
  if (n_src) {
    PFX_HIP(hipMemcpyAsync(s2t, di, sizeof(int32_t) * n_src, hipMemcpyDeviceToHost, ctx->stream));
    if (s2t_dist) PFX_HIP(hipMemcpyAsync(s2t_dist, dd, sizeof(float) * n_src, hipMemcpyDeviceToHost, ctx->stream));
  }
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_correspondences_dev(pfx_ctx* ctx, const float* d_src, int64_t n_src, int64_t src_stride,
                                              const float* d_tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                                              int32_t* d_query, int32_t* d_match, int64_t cap, int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_match_args(d_src, n_src, src_stride, d_tgt, n_tgt, tgt_stride, dim);
  if (!n_out || cap < 0 || (cap && (!d_query || !d_match)))
    throw Error(PFX_ERR_INVALID, "correspondences: invalid output arguments");
  const int64_t n = pfx::correspondences_dev(ctx, d_src, n_src, src_stride, d_tgt, n_tgt, tgt_stride, dim, d_query,
                                             d_match, cap);
  *n_out = n;
  if (n > cap) throw Error(PFX_ERR_CAPACITY, "correspondences: " + std::to_string(n) + " pairs > cap");
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_correspondences(pfx_ctx* ctx, const float* src, int64_t n_src, int64_t src_stride,
                                          const float* tgt, int64_t n_tgt, int64_t tgt_stride, int32_t dim,
                                          int32_t* query, int32_t* match, int64_t cap, int64_t* n_out) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_match_args(src, n_src, src_stride, tgt, n_tgt, tgt_stride, dim);
  if (!n_out || cap < 0 || (cap && (!query || !match)))
    throw Error(PFX_ERR_INVALID, "correspondences: invalid output arguments");
  // the last row needs only `dim` floats of its stride
  const int64_t cs = n_src ? (n_src - 1) * src_stride + dim : 0, ct = n_tgt ? (n_tgt - 1) * tgt_stride + dim : 0;
  float* ds = stage_in(ctx, "in_match_src", src, cs);
  float* dt = stage_in(ctx, "in_match_tgt", tgt, ct);
  int32_t* dq = ctx->buf("out_match_q").as<int32_t>(n_src + 1);
  int32_t* dm = ctx->buf("out_match_m").as<int32_t>(n_src + 1);
  const int64_t n = pfx::correspondences_dev(ctx, ds, n_src, src_stride, dt, n_tgt, tgt_stride, dim, dq, dm, n_src);
  *n_out = n;
  if (n > cap) throw Error(PFX_ERR_CAPACITY, "correspondences: " + std::to_string(n) + " pairs > cap");
  if (n) {
    PFX_HIP(hipMemcpyAsync(query, dq, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    PFX_HIP(hipMemcpyAsync(match, dm, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
  }
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_pcd_read_header(const char* path, pfx_pcd_header* out) {
  if (!path || !out) return PFX_ERR_INVALID;
  std::string err;
  try {
    return pfx::pcd_read_header(path, out, err);
  } catch (...) {
    return PFX_ERR_INVALID;
  }
}

extern "C" pfx_status pfx_pcd_load_xyz_dev(pfx_ctx* ctx, const char* path, float* d_x, float* d_y, float* d_z,
                                           int64_t cap, int64_t* n_out, pfx_pcd_header* hdr) {
  PFX_API_BEGIN
  check_ctx(ctx);
  if (!path || !n_out || cap < 0 || (cap && (!d_x || !d_y || !d_z)))
    throw Error(PFX_ERR_INVALID, "pcd load: invalid arguments");
  const int64_t n = pfx::pcd_load_xyz_dev(ctx, path, d_x, d_y, d_z, cap, hdr);
  *n_out = n;
  if (n > cap) throw Error(PFX_ERR_CAPACITY, "pcd load: " + std::to_string(n) + " points > cap");
  PFX_API_END(ctx)
}

namespace {
void check_points(const float* x, const float* y, const float* z, int64_t n, const char* what) {
  if (n < 0 || (n && (!x || !y || !z))) throw Error(PFX_ERR_INVALID, std::string(what) + ": invalid point arrays");
}
void check_iss(double sal, double nm, int32_t min_nb, double t21, double t32) {
  if (!(sal > 0.0) || !(nm > 0.0) || min_nb <= 0 || !(t21 > 0.0) || !(t32 > 0.0))
    throw Error(PFX_ERR_INVALID, "iss: radii, thresholds and min neighbours must be > 0 (ISSKeypoint3D::initCompute)");
}
}  // namespace

extern "C" pfx_status pfx_cloud_resolution_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                               int64_t n, double* resolution) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(d_x, d_y, d_z, n, "cloud_resolution");
  if (!resolution) throw Error(PFX_ERR_INVALID, "cloud_resolution: null output");
  *resolution = pfx::cloud_resolution_dev(ctx, d_x, d_y, d_z, n);
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_cloud_resolution(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                           double* resolution) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(x, y, z, n, "cloud_resolution");
  if (!resolution) throw Error(PFX_ERR_INVALID, "cloud_resolution: null output");
  float* dx = stage_in(ctx, "in_x", x, n);
  float* dy = stage_in(ctx, "in_y", y, n);
  float* dz = stage_in(ctx, "in_z", z, n);
  *resolution = pfx::cloud_resolution_dev(ctx, dx, dy, dz, n);
  PFX_API_END(ctx)
}

namespace {
// the detectors' "n_out / cap / idx" arguments
void check_keypoints_out(const int64_t* n_out, int64_t cap, const int32_t* idx, const char* what) {
  if (!n_out || cap < 0 || (cap && !idx)) throw Error(PFX_ERR_INVALID, std::string(what) + ": invalid output arguments");
}
// the late report of a result that the caller's arrays cannot hold (the counts are already stored)
void check_capacity(bool over, const char* what, int64_t count, const char* unit) {
  if (over) throw Error(PFX_ERR_CAPACITY, std::string(what) + ": " + std::to_string(count) + " " + unit + " > cap");
}
void check_harris(double radius, int32_t non_max) {
  if (!(radius > 0.0)) throw Error(PFX_ERR_INVALID, "harris3d: radius must be > 0");
  if (!non_max) throw Error(PFX_ERR_UNSUPPORTED, "harris3d: only non-maximum suppression is on the accelerated path");
}
// the host forms' outputs that every Harris variant shares, staged on the device
struct HarrisOut {
  int32_t* idx;
  float *resp, *corners;
  int32_t* cidx;
};
HarrisOut harris_out(pfx_ctx* ctx, int64_t n, const float* response, const float* corners,
                     const int32_t* corner_idx) {
  return HarrisOut{ctx->buf("out_h3_idx").as<int32_t>(n + 1),
                   response ? ctx->buf("out_h3_resp").as<float>(n + 1) : nullptr,
                   corners ? ctx->buf("out_h3_corners").as<float>(3 * (n + 1)) : nullptr,
                   corner_idx ? ctx->buf("out_h3_cidx").as<int32_t>(n + 1) : nullptr};
}
void harris_back(pfx_ctx* ctx, const HarrisOut& d, int64_t n, int64_t k, int64_t nc, int32_t* idx, float* response,
                 float* corners, int32_t* corner_idx) {
  rows_out(ctx, idx, d.idx, k, 1);
  rows_out(ctx, response, d.resp, n, 1);
  rows_out(ctx, corners, d.corners, nc, 3);
  rows_out(ctx, corner_idx, d.cidx, nc, 1);
}
}  // namespace

extern "C" pfx_status pfx_iss_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                            int64_t n, double salient_radius, double non_max_radius,
                                            int32_t min_neighbors, double threshold21, double threshold32,
                                            int32_t* d_idx, int64_t cap, int64_t* n_out, double* d_third) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(d_x, d_y, d_z, n, "iss");
  check_iss(salient_radius, non_max_radius, min_neighbors, threshold21, threshold32);
  check_keypoints_out(n_out, cap, d_idx, "iss");
  const int64_t k = pfx::iss_keypoints_dev(ctx, d_x, d_y, d_z, n, salient_radius, non_max_radius, min_neighbors,
                                           threshold21, threshold32, d_idx, cap, d_third);
  *n_out = k;
  check_capacity(k > cap, "iss", k, "keypoints");
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_iss_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                        double salient_radius, double non_max_radius, int32_t min_neighbors,
                                        double threshold21, double threshold32, int32_t* idx, int64_t cap,
                                        int64_t* n_out, double* third) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(x, y, z, n, "iss");
  check_iss(salient_radius, non_max_radius, min_neighbors, threshold21, threshold32);
  check_keypoints_out(n_out, cap, idx, "iss");
  const Dev3 d = stage3(ctx, "in_", x, y, z, n);
  int32_t* di = ctx->buf("out_iss_idx").as<int32_t>(n + 1);
  double* dt = third ? ctx->buf("out_iss_third").as<double>(n + 1) : nullptr;
  const int64_t k = pfx::iss_keypoints_dev(ctx, d.x, d.y, d.z, n, salient_radius, non_max_radius, min_neighbors,
                                           threshold21, threshold32, di, n, dt);
  *n_out = k;
  check_capacity(k > cap, "iss", k, "keypoints");
  rows_out(ctx, idx, di, k, 1);
  rows_out(ctx, third, dt, n, 1);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_uniform_sampling_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                               int64_t n, double radius, int32_t* d_idx, int64_t cap, int64_t* n_out,
                                               int32_t* d_leaf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(d_x, d_y, d_z, n, "uniform_sampling");
  check_keypoints_out(n_out, cap, d_idx, "uniform_sampling");
  pfx::uniform_radius_rule(radius);
  *n_out = 0;
  const int64_t k = pfx::uniform_sampling_dev(ctx, d_x, d_y, d_z, n, radius, d_idx, cap, d_leaf);
  *n_out = k;
  check_capacity(k > cap, "uniform_sampling", k, "keypoints");
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_uniform_sampling(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                           double radius, int32_t* idx, int64_t cap, int64_t* n_out, int32_t* leaf) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(x, y, z, n, "uniform_sampling");
  check_keypoints_out(n_out, cap, idx, "uniform_sampling");
  pfx::uniform_radius_rule(radius);
  *n_out = 0;
  const Dev3 d = stage3(ctx, "in_", x, y, z, n);
  int32_t* di = ctx->buf("out_uniform_idx").as<int32_t>(n + 1);
  int32_t* dl = leaf ? ctx->buf("out_uniform_leaf").as<int32_t>(n + 1) : nullptr;
  const int64_t k = pfx::uniform_sampling_dev(ctx, d.x, d.y, d.z, n, radius, di, n, dl);
  *n_out = k;
  check_capacity(k > cap, "uniform_sampling", k, "keypoints");
  rows_out(ctx, idx, di, k, 1);
  rows_out(ctx, leaf, dl, k, 1);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_harris3d_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                                 int64_t n, double radius, float threshold, int32_t non_max,
                                                 int32_t refine, int32_t* d_idx, int64_t cap, int64_t* n_out,
                                                 float* d_response, float* d_corners, int64_t* n_corners,
                                                 int32_t* d_corner_idx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(d_x, d_y, d_z, n, "harris3d");
  check_harris(radius, non_max);
  check_keypoints_out(n_out, cap, d_idx, "harris3d");
  int64_t nc = 0;
  const int64_t k = pfx::harris3d_dev(ctx, d_x, d_y, d_z, n, radius, threshold, refine, d_idx, cap, d_response,
                                      d_corners, &nc, d_corner_idx);
  *n_out = k;
  if (n_corners) *n_corners = nc;
  check_capacity(k > cap || (d_corners && nc > cap), "harris3d", std::max(k, nc), "keypoints/corners");
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_harris3d_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n,
                                             double radius, float threshold, int32_t non_max, int32_t refine,
                                             int32_t* idx, int64_t cap, int64_t* n_out, float* response,
                                             float* corners, int64_t* n_corners, int32_t* corner_idx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(x, y, z, n, "harris3d");
  check_harris(radius, non_max);
  check_keypoints_out(n_out, cap, idx, "harris3d");
  const Dev3 d = stage3(ctx, "in_", x, y, z, n);
  const HarrisOut o = harris_out(ctx, n, response, corners, corner_idx);
  int64_t nc = 0;
  const int64_t k = pfx::harris3d_dev(ctx, d.x, d.y, d.z, n, radius, threshold, refine, o.idx, n, o.resp, o.corners,
                                      &nc, o.cidx);
  *n_out = k;
  if (n_corners) *n_corners = nc;
  check_capacity(k > cap || (corners && nc > cap), "harris3d", std::max(k, nc), "keypoints/corners");
  harris_back(ctx, o, n, k, nc, idx, response, corners, corner_idx);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_harris6d_keypoints_dev(pfx_ctx* ctx, const float* d_x, const float* d_y, const float* d_z,
                                                 const uint32_t* d_rgb, int64_t n, double radius, float threshold,
                                                 int32_t non_max, int32_t refine, int32_t* d_idx, int64_t cap,
                                                 int64_t* n_out, float* d_response, float* d_corners,
                                                 int64_t* n_corners, float* d_grad, int32_t* d_corner_idx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(d_x, d_y, d_z, n, "harris6d");
  if (n && !d_rgb) throw Error(PFX_ERR_INVALID, "harris6d: null rgb");
  check_harris(radius, non_max);
  check_keypoints_out(n_out, cap, d_idx, "harris6d");
  int64_t nc = 0;
  const int64_t k = pfx::harris6d_dev(ctx, d_x, d_y, d_z, d_rgb, n, radius, threshold, refine, d_idx, cap, d_response,
                                      d_corners, &nc, d_grad, d_corner_idx);
  *n_out = k;
  if (n_corners) *n_corners = nc;
  check_capacity(k > cap || (d_corners && nc > cap), "harris6d", std::max(k, nc), "keypoints/corners");
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_harris6d_keypoints(pfx_ctx* ctx, const float* x, const float* y, const float* z,
                                             const uint32_t* rgb, int64_t n, double radius, float threshold,
                                             int32_t non_max, int32_t refine, int32_t* idx, int64_t cap,
                                             int64_t* n_out, float* response, float* corners, int64_t* n_corners,
                                             float* grad, int32_t* corner_idx) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(x, y, z, n, "harris6d");
  if (n && !rgb) throw Error(PFX_ERR_INVALID, "harris6d: null rgb");
  check_harris(radius, non_max);
  check_keypoints_out(n_out, cap, idx, "harris6d");
  const Dev3 d = stage3(ctx, "in_", x, y, z, n);
  uint32_t* dc_rgb = ctx->buf("in_rgb").as<uint32_t>(n + 1);
  if (n) PFX_HIP(hipMemcpyAsync(dc_rgb, rgb, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
  const HarrisOut o = harris_out(ctx, n, response, corners, corner_idx);
  float* dg = grad ? ctx->buf("out_h6_grad").as<float>(3 * (n + 1)) : nullptr;
  int64_t nc = 0;
  const int64_t k = pfx::harris6d_dev(ctx, d.x, d.y, d.z, dc_rgb, n, radius, threshold, refine, o.idx, n, o.resp,
                                      o.corners, &nc, dg, o.cidx);
  *n_out = k;
  if (n_corners) *n_corners = nc;
  check_capacity(k > cap || (corners && nc > cap), "harris6d", std::max(k, nc), "keypoints/corners");
  harris_back(ctx, o, n, k, nc, idx, response, corners, corner_idx);
  rows_out(ctx, grad, dg, n, 3);
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_ransac_rejector(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns,
                                          const float* tx, const float* ty, const float* tz, int64_t nt,
                                          const int32_t* query, const int32_t* match, int64_t n, double threshold,
                                          int32_t max_iterations, int32_t* keep, int64_t* n_keep,
                                          float* transformation) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(sx, sy, sz, ns, "ransac");
  check_points(tx, ty, tz, nt, "ransac");
  if (n < 0 || (n && (!query || !match || !keep)) || !n_keep || !transformation || !(threshold > 0.0) ||
      max_iterations < 0)
    throw Error(PFX_ERR_INVALID, "ransac: invalid arguments");
  int64_t iters = 0;
  *n_keep = pfx::ransac_rejector(ctx, sx, sy, sz, ns, tx, ty, tz, nt, query, match, n, threshold, max_iterations,
                                 keep, transformation, &iters);
  ctx->stats["ransac_iterations"] = iters;
  PFX_API_END(ctx)
}

// ---- ICP alignment (pfx_icp.hip) ----
extern "C" void pfx_icp_params_default(pfx_icp_params* p) {
  if (!p) return;
  p->max_correspondence_distance = std::sqrt(std::numeric_limits<double>::max());
  p->max_iterations = 10;
  p->transformation_epsilon = 0.0;
  p->euclidean_fitness_epsilon = -std::numeric_limits<double>::max();
}

namespace {
void icp_store(const pfx::IcpResult& r, float* transformation, double* fitness, int32_t* converged,
               int32_t* iterations, int32_t* state) {
  std::memcpy(transformation, r.T, sizeof(r.T));
  *fitness = r.fitness;
  *converged = r.converged;
  *iterations = r.iterations;
  *state = r.state;
}
bool icp_args_ok(const pfx_icp_params* params, const float* transformation, const double* fitness,
                 const int32_t* converged, const int32_t* iterations, const int32_t* state, const float* ax,
                 const float* ay, const float* az) {
  const int aligned = (ax != nullptr) + (ay != nullptr) + (az != nullptr);
  return params && transformation && fitness && converged && iterations && state && (aligned == 0 || aligned == 3);
}
}  // namespace

extern "C" pfx_status pfx_icp_dev(pfx_ctx* ctx, const float* d_sx, const float* d_sy, const float* d_sz, int64_t ns,
                                  const float* d_tx, const float* d_ty, const float* d_tz, int64_t nt,
                                  const pfx_icp_params* params, const float* guess, float* transformation,
                                  double* fitness, int32_t* converged, int32_t* iterations, int32_t* state,
                                  float* d_ax, float* d_ay, float* d_az) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(d_sx, d_sy, d_sz, ns, "icp");
  check_points(d_tx, d_ty, d_tz, nt, "icp");
  if (!icp_args_ok(params, transformation, fitness, converged, iterations, state, d_ax, d_ay, d_az))
    throw Error(PFX_ERR_INVALID, "icp: invalid arguments");
  pfx::IcpResult r;
  pfx::icp_dev(ctx, d_sx, d_sy, d_sz, ns, d_tx, d_ty, d_tz, nt, *params, guess, r, d_ax, d_ay, d_az);
  icp_store(r, transformation, fitness, converged, iterations, state);
  PFX_API_END(ctx)
}

extern "C" pfx_status pfx_icp(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns,
                              const float* tx, const float* ty, const float* tz, int64_t nt,
                              const pfx_icp_params* params, const float* guess, float* transformation,
                              double* fitness, int32_t* converged, int32_t* iterations, int32_t* state, float* ax,
                              float* ay, float* az) {
  PFX_API_BEGIN
  check_ctx(ctx);
  check_points(sx, sy, sz, ns, "icp");
  check_points(tx, ty, tz, nt, "icp");
  if (!icp_args_ok(params, transformation, fitness, converged, iterations, state, ax, ay, az))
    throw Error(PFX_ERR_INVALID, "icp: invalid arguments");
  float* dsx = stage_in(ctx, "icp_in_sx", sx, ns);
  float* dsy = stage_in(ctx, "icp_in_sy", sy, ns);
  float* dsz = stage_in(ctx, "icp_in_sz", sz, ns);
  float* dtx = stage_in(ctx, "icp_in_tx", tx, nt);
  float* dty = stage_in(ctx, "icp_in_ty", ty, nt);
  float* dtz = stage_in(ctx, "icp_in_tz", tz, nt);
  float* da = ax ? ctx->buf("icp_out_aligned").as<float>(3 * (size_t)(ns + 1)) : nullptr;
  pfx::IcpResult r;
  pfx::icp_dev(ctx, dsx, dsy, dsz, ns, dtx, dty, dtz, nt, *params, guess, r, da, da ? da + ns : nullptr,
               da ? da + 2 * ns : nullptr);
  if (ax && ns) {
    PFX_HIP(hipMemcpyAsync(ax, da, sizeof(float) * ns, hipMemcpyDeviceToHost, ctx->stream));
    PFX_HIP(hipMemcpyAsync(ay, da + ns, sizeof(float) * ns, hipMemcpyDeviceToHost, ctx->stream));
    PFX_HIP(hipMemcpyAsync(az, da + 2 * ns, sizeof(float) * ns, hipMemcpyDeviceToHost, ctx->stream));
  }
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  icp_store(r, transformation, fitness, converged, iterations, state);
  PFX_API_END(ctx)
}
