// pfx_knn.hip -- exact k-nearest-neighbour search (pcl::KdTreeFLANN::nearestKSearch, FLANN's
// KNNSimpleResultSet) and NormalEstimationOMP with setKSearch(k), by DESIGN.md "k-NN: the contract":
// a finite query receives the min(k, m) finite surface points of smallest key (d2, index), ascending,
// d2 = flann_d2 (float, q - p, no FMA).  Exact float-d2 ties are broken by index, where FLANN breaks
// them by the order its tree visits the leaves.
//
// Design (MI355X): a uniform grid, no kd-tree, as the cloud resolution's 2-nearest search.
//   k_knn: one wave per query, the queries in cell order.  The wave scans the 3x3x3 block of
//     the query's cell 64 candidates at a time and keeps, in its own LDS region, the keys below the
//     k-th smallest seen so far: candidates under the threshold are appended through a ballot, and
//     when the region fills the wave sorts it (pfx_wave_sort.h), keeps the first k and lowers the
//     threshold.  The row is certified when the block is the whole grid, or when its k-th d2 is at
//     most `bound`, a float below the d2 of every point outside the block (DESIGN.md gives the
//     argument).  An uncertified query goes to a queue.
//   The queue is searched again on a grid of doubled cell, for a bounded number of rounds; when the
//   queue is short (queue x points <= kKnnBruteWork) or the rounds are spent, it is answered
//   exhaustively: k_knn_scan spreads each query's scan of every finite point over up to 256 waves
//   (the same selection per slice), k_knn_merge selects the row from their partial rows.
//   k_knn_normals: lane per point, in cell order; the nine float sums in row order, then
//     finish_normal (pfx_normal_math.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "pfx_internal.h"
#include "pfx_neighbors.h"
#include "pfx_normal_math.h"
#include "pfx_wave_sort.h"

namespace pfx {
namespace {

constexpr int kKnnMaxK = PFX_KNN_MAX_K;
// a wave's region holds the k kept keys and one more batch of 64 candidates
static_assert(kKnnMaxK + 64 <= kWaveSortCap, "PFX_KNN_MAX_K: the wave's LDS region cannot hold a row and a batch");
constexpr int kKnnRounds = 6;                   // grids built per call at most (the cell doubles)
constexpr int64_t kKnnBruteWork = 1 << 24;      // queue x finite points answered exhaustively at once
enum { kcFail = 0, kcSkip = 1, kcWords = 2 };   // the search kernels' counters
// the exhaustive scan: points per wave, waves per query at most, bytes of partial rows at most
constexpr int64_t kKnnSlice = 2048;
constexpr int kKnnMaxParts = 256;
constexpr int64_t kKnnPartBytes = int64_t(256) << 20;

__global__ void __launch_bounds__(256) k_knn_prefill(int64_t* __restrict__ counts, int64_t nq,
                                                     int32_t* __restrict__ idx, float* __restrict__ d2,
                                                     int64_t rows) {
  const float nan = __builtin_nanf("");
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < rows; i += (int64_t)gridDim.x * 256) {
    if (i < nq) counts[i] = 0;
    if (idx) idx[i] = -1;
    if (d2) d2[i] = nan;
  }
}

// cell key of every query on grid g (clamped into it: the order only serves locality); non-finite
// queries sort behind every cell
__global__ void __launch_bounds__(256) k_knn_qkeys(GridView g, const float* __restrict__ qx,
                                                   const float* __restrict__ qy, const float* __restrict__ qz,
                                                   int64_t nq, uint32_t* __restrict__ keys,
                                                   int32_t* __restrict__ vals) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  if (i >= nq) return;
  const float x = qx[i], y = qy[i], z = qz[i];
  uint32_t key = (uint32_t)((int64_t)g.nx * g.ny * g.nz);
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    int64_t cx = (int64_t)floor(((double)x - g.ox) * g.inv);
    int64_t cy = (int64_t)floor(((double)y - g.oy) * g.inv);
    int64_t cz = (int64_t)floor(((double)z - g.oz) * g.inv);
    cx = cx < 0 ? 0 : (cx > g.nx - 1 ? g.nx - 1 : cx);
    cy = cy < 0 ? 0 : (cy > g.ny - 1 ? g.ny - 1 : cy);
    cz = cz < 0 ? 0 : (cz > g.nz - 1 ? g.nz - 1 : cz);
    key = (uint32_t)((cx * g.ny + cy) * g.nz + cz);
  }
  keys[i] = key;
  vals[i] = (int32_t)i;
}

// the 3x3x3 block of the query's cell (query_runs' clamped cell) holds every cell of the grid
__device__ __forceinline__ bool block_is_grid(const GridView& g, float qx, float qy, float qz) {
  int64_t cx = (int64_t)floor(((double)qx - g.ox) * g.inv);
  int64_t cy = (int64_t)floor(((double)qy - g.oy) * g.inv);
  int64_t cz = (int64_t)floor(((double)qz - g.oz) * g.inv);
  cx = cx < -2 ? -2 : (cx > g.nx + 1 ? g.nx + 1 : cx);
  cy = cy < -2 ? -2 : (cy > g.ny + 1 ? g.ny + 1 : cy);
  cz = cz < -2 ? -2 : (cz > g.nz + 1 ? g.nz + 1 : cz);
  return cx - 1 <= 0 && cx + 1 >= g.nx - 1 && cy - 1 <= 0 && cy + 1 >= g.ny - 1 && cz - 1 <= 0 &&
         cz + 1 >= g.nz - 1;
}

// A wave's selection of the kk smallest keys of a candidate stream, in its own LDS region `key`:
// push() takes one candidate per lane (valid or not) and keeps those below the threshold; when fewer
// than 64 slots are free the region is sorted, cut to kk keys and the threshold lowered to the kk-th.
// finish() leaves the min(cnt, kk) smallest keys sorted in key[0..cnt).  Every lane of the wave makes
// the same calls.
struct WaveTopK {
  uint64_t* key;
  int kk, cap, cnt;
  uint64_t thr;  // keys below it can still be among the kk smallest
  __device__ __forceinline__ WaveTopK(uint64_t* region, int kk_)
      // the region in use: the kept keys and a batch fit below it, and a short row sorts a short region
      : key(region), kk(kk_), cap(kk_ <= 64 ? 128 : (kk_ <= 192 ? 256 : kWaveSortCap)), cnt(0), thr(~0ull) {}
  __device__ __forceinline__ void push(bool valid, uint64_t kv, int lane) {
    const bool hit = valid && kv < thr;
    const uint64_t m = __ballot(hit);
    if (hit) key[cnt + __popcll(m & lanemask_lt())] = kv;  // cnt <= cap - 64 here
    cnt += __popcll(m);
    if (cnt > cap - 64) {  // (then cnt >= kk: cap - 64 >= kk)
      wave_sort_keys(key, cnt, lane);
      cnt = kk;
      thr = key[kk - 1];
    }
  }
  __device__ __forceinline__ void finish(int lane) {
    wave_sort_keys(key, cnt, lane);
    if (cnt > kk) cnt = kk;
  }
};

__device__ __forceinline__ void write_row(const uint64_t* key, int cnt, int64_t q, int k, int lane,
                                          int64_t* __restrict__ counts, int32_t* __restrict__ idx,
                                          float* __restrict__ d2) {
  const int64_t row = q * k;
  for (int m = lane; m < cnt; m += 64) {
    const uint64_t kv = key[m];
    idx[row + m] = key_idx(kv);
    if (d2) d2[row + m] = key_d2(kv);
  }
  if (lane == 0) counts[q] = cnt;
}

// One wave per query `order[w]` (order == nullptr: query w), w < work.  kk = min(k, finite points)
// >= 1.  The candidates are the points of the query's block; the row is written when certified, the
// query pushed to failq otherwise.  d2 nullable.
__global__ void __launch_bounds__(256) k_knn(GridView g, const float* __restrict__ qx, const float* __restrict__ qy,
                                             const float* __restrict__ qz, const int32_t* __restrict__ order,
                                             int64_t work, int k, int kk, float bound, int64_t* __restrict__ counts,
                                             int32_t* __restrict__ idx, float* __restrict__ d2,
                                             int32_t* __restrict__ failq, int* __restrict__ ctr) {
  __shared__ uint64_t s_key[4][kWaveSortCap];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= work) return;  // wave-uniform; no workgroup barrier below
  const int32_t q = order ? order[w] : (int32_t)w;
  const float x = qx[q], y = qy[q], z = qz[q];
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
    if (lane == 0) atomicAdd(ctr + kcSkip, 1);
    return;
  }
  WaveTopK sel(s_key[wv], kk);
  Runs R;
  query_runs(g, x, y, z, R);
  const uint32_t T = (uint32_t)R.pref[9];
  for (uint32_t t0 = 0; t0 < T; t0 += 64) {
    const uint32_t t = t0 + lane;
    uint64_t kv = 0;
    if (t < T) {
      const int32_t pos = run_pos(R, (int32_t)t);
      const float4 c = g.sp[pos];
      kv = nb_key(flann_d2(x, y, z, c.x, c.y, c.z), g.perm[pos]);
    }
    sel.push(t < T, kv, lane);
  }
  sel.finish(lane);
  if (block_is_grid(g, x, y, z) || (sel.cnt == kk && key_d2(sel.key[kk - 1]) <= bound))
    write_row(sel.key, sel.cnt, q, k, lane, counts, idx, d2);
  else if (lane == 0)
    failq[atomicAdd(ctr + kcFail, 1)] = q;
}

// The exhaustive scan of the queued queries, in two steps so that one query's scan of every finite
// point is spread over `parts` waves.  k_knn_scan: wave w takes slice w % parts of the finite points
// (the grid's sorted positions) for query queue[w / parts] and leaves its kk smallest keys, sorted and
// padded with ~0, in part[w * kk ..).  k_knn_merge: one wave per query selects the kk smallest of
// its parts' keys -- the full ordered row -- and writes it.
__global__ void __launch_bounds__(256) k_knn_scan(GridView g, const float* __restrict__ qx,
                                                  const float* __restrict__ qy, const float* __restrict__ qz,
                                                  const int32_t* __restrict__ queue, int64_t work, int parts, int kk,
                                                  uint64_t* __restrict__ part) {
  __shared__ uint64_t s_key[4][kWaveSortCap];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= work * parts) return;  // wave-uniform; no workgroup barrier below
  const int32_t q = queue[w / parts];
  const float x = qx[q], y = qy[q], z = qz[q];
  const uint32_t nf = (uint32_t)grid_nfinite(g);
  const uint32_t chunk = (nf + parts - 1) / parts, p0 = (uint32_t)(w % parts) * chunk;
  const uint32_t p1 = p0 + chunk < nf ? p0 + chunk : nf;  // (p0 may lie beyond nf: an empty slice)
  WaveTopK sel(s_key[wv], kk);
  for (uint32_t t0 = p0; t0 < p1; t0 += 64) {
    const uint32_t t = t0 + lane;
    uint64_t kv = 0;
    if (t < p1) {
      const float4 c = g.sp[t];
      kv = nb_key(flann_d2(x, y, z, c.x, c.y, c.z), g.perm[t]);
    }
    sel.push(t < p1, kv, lane);
  }
  sel.finish(lane);
  for (int m = lane; m < kk; m += 64) part[w * kk + m] = m < sel.cnt ? sel.key[m] : ~0ull;
}

__global__ void __launch_bounds__(256) k_knn_merge(const int32_t* __restrict__ queue, int64_t work, int parts, int k,
                                                   int kk, const uint64_t* __restrict__ part,
                                                   int64_t* __restrict__ counts, int32_t* __restrict__ idx,
                                                   float* __restrict__ d2) {
  __shared__ uint64_t s_key[4][kWaveSortCap];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wv;
  if (w >= work) return;  // wave-uniform; no workgroup barrier below
  WaveTopK sel(s_key[wv], kk);
  const uint64_t* mine = part + w * parts * kk;
  const int T = parts * kk;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int t = t0 + lane;
    const uint64_t kv = t < T ? mine[t] : ~0ull;
    sel.push(kv != ~0ull, kv, lane);
  }
  sel.finish(lane);
  write_row(sel.key, sel.cnt, queue[w], k, lane, counts, idx, d2);
}

// NormalEstimation::computePointNormal over the row of each finite point (lane per point, in the
// grid's cell order): the nine sequential float sums in row order, then finish_normal
__global__ void __launch_bounds__(256) k_knn_normals(GridView g, int k, const int64_t* __restrict__ counts,
                                                     const int32_t* __restrict__ idx, float vpx, float vpy, float vpz,
                                                     float* __restrict__ nx, float* __restrict__ ny,
                                                     float* __restrict__ nz, float* __restrict__ curv) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= grid_nfinite(g)) return;
  const int32_t i = g.perm[p];
  const float4 q = g.sp[p];
  const int c = (int)counts[i];
  const int32_t* row = idx + (int64_t)i * k;
  float a[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int m = 0; m < c; ++m) {
    const int32_t j = row[m];
    const float px = g.ux[j], py = g.uy[j], pz = g.uz[j];
#pragma unroll
    for (int t = 0; t < 9; ++t) a[t] = a[t] + chain_term(t, px, py, pz);
  }
  float o[4];
  finish_normal(a, c, q.x, q.y, q.z, vpx, vpy, vpz, o);
  nx[i] = o[0];
  ny[i] = o[1];
  nz[i] = o[2];
  curv[i] = o[3];
}

__global__ void __launch_bounds__(256) k_knn_nan4(float* __restrict__ a, float* __restrict__ b, float* __restrict__ c,
                                                  float* __restrict__ d, int64_t n) {
  const float v = __builtin_nanf("");
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    a[i] = v;
    b[i] = v;
    c[i] = v;
    d[i] = v;
  }
}

// the first cell edge: 1.3 times the radius of the ball expected to hold k points, were the points
// spread evenly over the bounding volume, or over the bounding box's faces, whichever is smaller
// (scans are surfaces).  Zero extents are widened to a thousandth of the largest; a single point
// (or n copies of one) takes 1.  Any positive value gives the exact answer.
double first_cell(const double lo[3], const double hi[3], int64_t n, int k) {
  double ext = 0.0, e[3];
  for (int d = 0; d < 3; ++d) ext = std::max(ext, hi[d] - lo[d]);
  if (!(ext > 0.0) || n <= 0) return 1.0;
  for (int d = 0; d < 3; ++d) e[d] = std::max(hi[d] - lo[d], ext * 1e-3);
  const double pi = 3.14159265358979323846;
  const double vol = e[0] * e[1] * e[2], area = 2.0 * (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]);
  const double hv = std::cbrt(0.75 / pi * (double)k * vol / (double)n);
  const double hs = std::sqrt((double)k * area / (pi * (double)n));
  const double h = 1.3 * std::min(hv, hs);
  return (h > 0.0 && std::isfinite(h)) ? h : 1.0;
}

// the certification bound of a grid asked for cell edge h (DESIGN.md "k-NN: kernels and
// certification"): below the float d2 of every point outside a query's block; negative (nothing is
// certified by distance) where float cannot hold it as a normal, finite number
float certified_bound(double h) {
  const float b = (float)(h * h * (1.0 - 0x1p-21));
  return (std::isfinite(b) && b >= 0x1p-100f) ? b : -1.0f;
}

}  // namespace

void knn_k_rule(int32_t k, const char* what) {
  if (k < 1) throw Error(PFX_ERR_INVALID, std::string(what) + ": k must be >= 1");
  if (k > kKnnMaxK)
    throw Error(PFX_ERR_CAPACITY, std::string(what) + ": k = " + std::to_string(k) + " > PFX_KNN_MAX_K");
}

void knn_count_rule(int64_t n, int64_t nq, const char* what) {
  if (n >= (int64_t(1) << 28) || nq >= (int64_t(1) << 28))
    throw Error(PFX_ERR_CAPACITY, std::string(what) + ": k-NN supports < 2^28 points and queries");
}

void knn_search_dev(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const float* qx,
                    const float* qy, const float* qz, int64_t nq, int32_t k, int64_t* counts, int32_t* idx,
                    float* d2, bool fill_rows) {
  knn_k_rule(k, "knn_search");
  PFX_CHECK(n >= 0 && nq >= 0, "knn_search: negative point count");
  knn_count_rule(n, nq, "knn_search");
  hipStream_t st = ctx->stream;
  int64_t s_first = 0, s_requeued = 0, s_exh = 0, s_skip = 0, s_rounds = 0;
  const auto publish = [&]() {
    ctx->stats["knn_queries"] = nq;
    ctx->stats["knn_rounds"] = s_rounds;
    ctx->stats["knn_first"] = s_first;
    ctx->stats["knn_requeued"] = s_requeued;
    ctx->stats["knn_exhaustive"] = s_exh;
    ctx->stats["knn_skipped"] = s_skip;
  };
  if (nq == 0) {
    publish();
    return;
  }
  TimeScope total(ctx, "knn", true);
  {
    const int64_t rows = fill_rows ? nq * k : nq;
    k_knn_prefill<<<(unsigned)std::min<int64_t>(ceil_div(rows, 256), 4096), 256, 0, st>>>(
        counts, nq, fill_rows ? idx : nullptr, fill_rows ? d2 : nullptr, rows);
    check_launch("k_knn_prefill");
  }
  if (n == 0) {
    publish();
    return;
  }
  Grid& G = ctx->grid_b;
  double lo[3], hi[3];
  points_bbox(ctx, G, x, y, z, n, lo, hi);
  double h = first_cell(lo, hi, n, k);
  const bool same = qx == x && qy == y && qz == z && nq == n;
  int* ctr = ctx->buf("knn_ctr").as<int>(kcWords);
  int32_t* qa = ctx->buf("knn_qa").as<int32_t>(nq);
  int32_t* qb = ctx->buf("knn_qb").as<int32_t>(nq);
  int* h_ctr = ctx->readback<int>();
  int64_t nfin = -1;
  int kk = 0;
  const int32_t* queue = nullptr;
  int32_t* fail = qa;
  int64_t work = 0;
  for (int round = 0;; ++round) {
    build_grid(ctx, G, x, y, z, n, h);
    ++s_rounds;
    const GridView g = view(G);
    if (round == 0) {
      int32_t nf = 0;
      PFX_HIP(hipMemcpyAsync(&nf, G.cell_start + G.ncells, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      PFX_HIP(hipStreamSynchronize(st));
      nfin = nf;
      if (nfin == 0) break;  // no surface: every row stays empty
      kk = (int)std::min<int64_t>(k, nfin);
      if (same) {  // the surface is the queries: the grid's own order, its finite points
        queue = G.perm;
        work = nfin;
        s_skip = nq - nfin;
      } else {
        TimeScope ts(ctx, "knn_order");
        uint32_t* keys = ctx->buf("knn_keys").as<uint32_t>(2 * nq);
        int32_t* vals = ctx->buf("knn_vals").as<int32_t>(nq);
        int bits = 1;
        while ((int64_t(1) << bits) <= G.ncells) ++bits;
        size_t tb = 0;
        PFX_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys, keys + nq, vals, qb, (size_t)nq, 0, bits, st));
        void* tmp = ctx->buf("knn_tmp").get(tb + 16);
        k_knn_qkeys<<<(unsigned)ceil_div(nq, 256), 256, 0, st>>>(g, qx, qy, qz, nq, keys, vals);
        check_launch("k_knn_qkeys");
        PFX_HIP(rocprim::radix_sort_pairs(tmp, tb, keys, keys + nq, vals, qb, (size_t)nq, 0, bits, st));
        queue = qb;  // (read by this round only: the next one's failures go to qb after it)
        work = nq;
      }
    }
    PFX_HIP(hipMemsetAsync(ctr, 0, kcWords * sizeof(int), st));
    {
      TimeScope ts(ctx, "knn_search");
      k_knn<<<(unsigned)ceil_div(work, 4), 256, 0, st>>>(g, qx, qy, qz, queue, work, k, kk, certified_bound(h),
                                                               counts, idx, d2, fail, ctr);
      check_launch("k_knn");
    }
    PFX_HIP(hipMemcpyAsync(h_ctr, ctr, kcWords * sizeof(int), hipMemcpyDeviceToHost, st));
    PFX_HIP(hipStreamSynchronize(st));
    const int64_t failed = h_ctr[kcFail];
    if (round == 0) {
      if (!same) s_skip = h_ctr[kcSkip];
      s_first = work - failed - (same ? 0 : s_skip);
    } else {
      s_requeued += work - failed;
    }
    if (failed == 0) break;
    if (failed * nfin <= kKnnBruteWork || round + 1 >= kKnnRounds) {
      TimeScope ts(ctx, "knn_exhaustive");
      // a wave per kKnnSlice points of a query's scan, as far as kKnnPartBytes of partial rows allow
      const int64_t row_bytes = (int64_t)kk * (int64_t)sizeof(uint64_t);
      const int parts = (int)std::max<int64_t>(
          1, std::min<int64_t>({(int64_t)kKnnMaxParts, ceil_div(nfin, kKnnSlice), kKnnPartBytes / (failed * row_bytes)}));
      uint64_t* part = ctx->buf("knn_part").as<uint64_t>((size_t)failed * parts * kk);
      k_knn_scan<<<(unsigned)ceil_div(failed * parts, 4), 256, 0, st>>>(g, qx, qy, qz, fail, failed, parts, kk, part);
      k_knn_merge<<<(unsigned)ceil_div(failed, 4), 256, 0, st>>>(fail, failed, parts, k, kk, part, counts, idx, d2);
      check_launch("k_knn_exhaustive");
      s_exh = failed;
      break;
    }
    queue = fail;
    work = failed;
    fail = fail == qa ? qb : qa;
    h *= 2.0;
  }
  publish();
}

void normals_knn_dev(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, int32_t k,
                     const float vp[3], float* nx, float* ny, float* nz, float* curv) {
  knn_k_rule(k, "normals_knn");
  if (n == 0) {
    knn_search_dev(ctx, x, y, z, 0, x, y, z, 0, k, nullptr, nullptr, nullptr, false);
    return;
  }
  hipStream_t st = ctx->stream;
  int64_t* counts = ctx->buf("knn_n_counts").as<int64_t>(n);
  int32_t* rows = ctx->buf("knn_n_rows").as<int32_t>((size_t)n * k);
  k_knn_nan4<<<(unsigned)std::min<int64_t>(ceil_div(n, 256), 4096), 256, 0, st>>>(nx, ny, nz, curv, n);
  check_launch("k_knn_nan4");
  knn_search_dev(ctx, x, y, z, n, x, y, z, n, k, counts, rows, nullptr, false);
  // the last grid of the search holds every finite point in cell order
  TimeScope ts(ctx, "knn_normals");
  k_knn_normals<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(view(ctx->grid_b), k, counts, rows, vp[0], vp[1], vp[2],
                                                            nx, ny, nz, curv);
  check_launch("k_knn_normals");
}

}  // namespace pfx
