// pfx_uniform.hip -- the reference's uniform-sampling keypoints (keypoints.h:274-290):
//
//   pcl::UniformSampling<PointXYZRGB> (PCL 1.7 keypoints/impl/uniform_sampling.hpp) with
//   setRadiusSearch(normal_radius_search_): one keypoint per occupied voxel of edge `radius`,
//   the point of the voxel with the smallest (diff, index), diff being PCL's squared norm of
//   (point, 1) - (cell, 0) -- the cell's integer coordinates, not its centre (DESIGN.md
//   "Uniform sampling: the contract").
//
// Design (MI355X): no table over the cells, so memory grows with n alone.
//   bounds:  the grids' bounding-box pass (pfx_grid.hip), one host wait; the cell range, the
//            extent checks and the number of key bits follow on the host
//   keys:    lane per point, key = leaf_idx << 32 | float_bits(diff), value = the point's index;
//            a non-finite point gets the all-ones key
//   sort:    one stable rocprim::radix_sort_pairs over the 32 + bits(cells - 1) bits in use: the
//            input is in index order, so the head of a run of equal leaf_idx is the smallest
//            (diff, index), and the runs come out in leaf order
//   heads:   lane per sorted position flags the run heads; rocprim::select compacts their
//            positions in order; after the second host wait (the count) a gather writes exactly
//            that many indices and leaves to the caller's arrays
#include <cmath>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "pfx_internal.h"

namespace pfx {
namespace {

constexpr uint64_t kNoKey = ~0ull;  // a point that takes no part (a leaf index stays below 2^31 - 1)

struct CellRange {
  float inv;
  int32_t min_i, min_j, min_k;
  uint32_t div_x, div_xy;  // div_x * div_y
};

// [0] the points that took part (k_uniform_keys), [1] the occupied cells (rocprim::select)
struct Counts {
  unsigned long long points, leaves;
};

__global__ void __launch_bounds__(256) k_uniform_keys(const float* __restrict__ x, const float* __restrict__ y,
                                                      const float* __restrict__ z, int64_t n, CellRange c,
                                                      uint64_t* __restrict__ key,
                                                      unsigned long long* __restrict__ n_points) {
  __shared__ unsigned int s_cnt[4];
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool in = false;
  if (t < n) {
    const float px = x[t], py = y[t], pz = z[t];
    in = isfinite(px) && isfinite(py) && isfinite(pz);
    uint64_t kv = kNoKey;
    if (in) {
      // one float multiply per axis; the products lie in [-2^31, 2^31) (checked on the bounds)
      const int32_t i = (int32_t)floorf(px * c.inv), j = (int32_t)floorf(py * c.inv),
                    k = (int32_t)floorf(pz * c.inv);
      const uint32_t leaf = (uint32_t)(i - c.min_i) + (uint32_t)(j - c.min_j) * c.div_x +
                            (uint32_t)(k - c.min_k) * c.div_xy;
      const float dx = px - (float)i, dy = py - (float)j, dz = pz - (float)k;
      const float diff = (dx * dx + dz * dz) + (dy * dy + 1.0f);  // Eigen's (a0 + a2) + (a1 + a3)
      kv = ((uint64_t)leaf << 32) | __float_as_uint(diff);
    }
    key[t] = kv;
  }
  const unsigned int cnt = (unsigned int)__popcll(__ballot(in));
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (total) atomicAdd(n_points, (unsigned long long)total);
  }
}

// the first element of every run of equal leaf_idx among the sorted keys
__global__ void __launch_bounds__(256) k_uniform_heads(const uint64_t* __restrict__ key, int64_t n,
                                                       uint8_t* __restrict__ flag) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const uint64_t kv = key[p];
  const uint32_t leaf = (uint32_t)(kv >> 32);
  flag[p] = kv != kNoKey && (p == 0 || (uint32_t)(key[p - 1] >> 32) != leaf);
}

__global__ void __launch_bounds__(256) k_uniform_gather(const uint64_t* __restrict__ key,
                                                        const int32_t* __restrict__ val,
                                                        const int32_t* __restrict__ head, int64_t k,
                                                        int32_t* __restrict__ out, int32_t* __restrict__ leaf) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= k) return;
  const int32_t p = head[j];
  out[j] = val[p];
  if (leaf) leaf[j] = (int32_t)(key[p] >> 32);
}

// (int)floorf(v * inv) of a bound, or PFX_ERR_CAPACITY when the product leaves int's range
int32_t bound_cell(double v, float inv) {
  const float prod = (float)v * inv;
  if (!(prod >= -2147483648.0f && prod < 2147483648.0f))
    throw Error(PFX_ERR_CAPACITY, "uniform_sampling: a coordinate times 1 / leaf lies outside [-2^31, 2^31)");
  return (int32_t)std::floor(prod);
}

}  // namespace

void uniform_radius_rule(double radius) {
  const float leaf = (float)radius;
  const float inv = 1.0f / leaf;
  PFX_CHECK(std::isfinite(leaf) && leaf > 0.0f && std::isfinite(inv),
            "uniform_sampling: the radius and its reciprocal must be finite and > 0 as floats");
}

int64_t uniform_sampling_dev(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, double radius,
                             int32_t* out, int64_t cap, int32_t* leaf_out) {
  PFX_CHECK(n >= 0 && n < (int64_t(1) << 31), "uniform_sampling: point count must be in [0, 2^31)");
  uniform_radius_rule(radius);
  const float inv = 1.0f / (float)radius;  // a float division, done once
  ctx->stats["uniform_points"] = 0;
  ctx->stats["uniform_leaves"] = 0;
  ctx->stats["uniform_cells"] = 0;
  if (n == 0) return 0;
  hipStream_t st = ctx->stream;
  TimeScope total(ctx, "uniform", true);
  double lo[3], hi[3];
  bool any;
  {
    TimeScope ts(ctx, "uniform_bbox");
    any = points_bbox_any(ctx, ctx->buf("uniform_minmax"), x, y, z, n, lo, hi);
  }
  if (!any) return 0;
  // the multiply and floor are monotone, so the cells of the bounds bound the cells
  int32_t min_b[3];
  int64_t div[3];
  for (int d = 0; d < 3; ++d) {
    min_b[d] = bound_cell(lo[d], inv);
    div[d] = (int64_t)bound_cell(hi[d], inv) - min_b[d] + 1;
  }
  constexpr int64_t kMaxCells = 2147483647;  // PCL's leaf index is an int
  // in int64 without overflow: every div is in [1, 2^32]
  if (div[0] > kMaxCells || div[1] > kMaxCells / div[0] || div[2] > kMaxCells / (div[0] * div[1]))
    throw Error(PFX_ERR_CAPACITY, "uniform_sampling: the bounding box holds more than 2^31 - 1 cells (" +
                                      std::to_string(div[0]) + " x " + std::to_string(div[1]) + " x " +
                                      std::to_string(div[2]) + "); PCL's int leaf index would overflow");
  const int64_t cells = div[0] * div[1] * div[2];
  int leaf_bits = 0;
  while (((cells - 1) >> leaf_bits) != 0) ++leaf_bits;
  const CellRange cr{inv, min_b[0], min_b[1], min_b[2], (uint32_t)div[0], (uint32_t)(div[0] * div[1])};

  uint64_t* key = ctx->buf("uniform_key").as<uint64_t>(n);
  uint64_t* skey = ctx->buf("uniform_skey").as<uint64_t>(n);
  int32_t* sval = ctx->buf("uniform_sval").as<int32_t>(n);
  uint8_t* flag = ctx->buf("uniform_flag").as<uint8_t>(n);
  int32_t* head = ctx->buf("uniform_head").as<int32_t>(n);
  Counts* cnt = ctx->buf("uniform_cnt").as<Counts>(1);
  const unsigned nb = (unsigned)ceil_div(n, 256);
  PFX_HIP(hipMemsetAsync(cnt, 0, sizeof(Counts), st));
  {
    TimeScope ts(ctx, "uniform_keys");
    k_uniform_keys<<<nb, 256, 0, st>>>(x, y, z, n, cr, key, &cnt->points);
    check_launch("k_uniform_keys");
  }
  {
    TimeScope ts(ctx, "uniform_sort");
    const rocprim::counting_iterator<int32_t> index(0);
    const unsigned end_bit = 32u + (unsigned)leaf_bits;
    size_t tb = 0;
    PFX_HIP(rocprim::radix_sort_pairs(nullptr, tb, key, skey, index, sval, (size_t)n, 0u, end_bit, st));
    void* tmp = ctx->buf("uniform_sort_tmp").get(tb + 16);
    PFX_HIP(rocprim::radix_sort_pairs(tmp, tb, key, skey, index, sval, (size_t)n, 0u, end_bit, st));
  }
  {
    TimeScope ts(ctx, "uniform_heads");
    k_uniform_heads<<<nb, 256, 0, st>>>(skey, n, flag);
    check_launch("k_uniform_heads");
  }
  {
    TimeScope ts(ctx, "uniform_compact");
    size_t tb = 0;
    PFX_HIP(rocprim::select(nullptr, tb, rocprim::counting_iterator<int32_t>(0), flag, head, &cnt->leaves, (size_t)n,
                            st));
    void* tmp = ctx->buf("uniform_select_tmp").get(tb + 16);
    PFX_HIP(rocprim::select(tmp, tb, rocprim::counting_iterator<int32_t>(0), flag, head, &cnt->leaves, (size_t)n,
                            st));
  }
  Counts* h = ctx->readback<Counts>();  // pinned
  PFX_HIP(hipMemcpyAsync(h, cnt, sizeof(Counts), hipMemcpyDeviceToHost, st));
  ctx->sync_spin(st);
  const int64_t k = (int64_t)h->leaves;
  ctx->stats["uniform_points"] = (int64_t)h->points;
  ctx->stats["uniform_leaves"] = k;
  ctx->stats["uniform_cells"] = cells;
  if (k > 0 && k <= cap) {
    TimeScope ts(ctx, "uniform_gather");
    k_uniform_gather<<<(unsigned)ceil_div(k, 256), 256, 0, st>>>(skey, sval, head, k, out, leaf_out);
    check_launch("k_uniform_gather");
  }
  return k;
}

}  // namespace pfx
