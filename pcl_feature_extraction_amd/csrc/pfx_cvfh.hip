// pfx_cvfh.hip -- CVFHEstimation<PointXYZRGB, Normal, VFHSignature308> (evaluation.cpp:649-675) and
// its clustering stage, pcl::extractEuclideanClustersSmooth, on gfx950.  DESIGN.md "CVFH" and "CVFH:
// the contract".
//
// Not one neighbourhood per query: a curvature filter, connected components on the radius graph, and
// one histogram of the whole point set per component.
//   filter      flags, then the count / scan / scatter compaction on wave ballots (order kept); the
//               filtered cloud F is padded with NaN points to the indexed count, so its size never
//               has to reach the host: a NaN point has no neighbour, no normal and no cluster
//   normals     normals_dev on F
//   components  hook and compress on two int32 words a point.  A round: every point takes the
//               smallest label among its edge neighbours (3 x 3 x 3 cells of the grid at the
//               tolerance, edge test per candidate, nothing stored) and atomicMin's it into the
//               parent word of its own root; then the parents are followed to their roots.  A round
//               reads only the labels the round before left and writes only through integer
//               atomicMin, so the labels after every round, and with them the number of rounds, are
//               the same on every run.  The rounds are queued eight at a time, each gated by the
//               flag the round before left on the device; the host looks once per eight.
//   ranking     component sizes (integer atomicAdd), the roots with min_points or more compacted in
//               index order: the cluster's row
//   means       one workgroup a cluster: 256 labels at a time, the members compacted in index order
//               into LDS, six lanes add their coordinate one member after the other
//   signature   the largest distance as atomicMax on the bits of a non-negative float; a 308-int
//               histogram per workgroup in LDS (integer atomics), one global integer atomicAdd per
//               non-zero bin; a last kernel turns the counts into floats with repeated_add
// No floating-point atomic anywhere: every output is a count or an ordered float sum.
#include <cmath>
#include <cstring>

#include "pfx_neighbors.h"
#include "pfx_pair_features.h"

namespace pfx {
namespace {

constexpr int kCcBatch = 8;  // hooking rounds queued between two looks of the host
// the words of one call (ints, one zeroed block, read back in one copy)
enum CvfhWord {
  kWEdges = 0,    // [0..1] u64
  kWRounds = 2,   // hooking rounds run
  kWClusters = 3,
  kWBadIndex = 4,  // an index outside the surface
  kWFiltered = 5,  // |F|
  kWChanged = 8,   // [8 .. 8 + kCcBatch): round k lowered a parent
  kWords = 16,
};
static_assert(kWChanged + kCcBatch <= kWords, "the rounds' flags fit the block");

// ---- order-keeping compaction of n flags: count, scan, scatter (the form of pfx_icp.hip) ----
__global__ void __launch_bounds__(256) k_cv_count(const uint8_t* __restrict__ flags, int64_t n, int* __restrict__ blk) {
  __shared__ int s_c[4];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const uint64_t m = __ballot(i < n && flags[i]);
  if ((tid & 63) == 0) s_c[tid >> 6] = __popcll(m);
  __syncthreads();
  if (tid == 0) blk[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

// exclusive scan of the block counts in place (one workgroup), total -> *n_out
__global__ void __launch_bounds__(256) k_cv_scan(int* __restrict__ blk, int64_t nb, int* __restrict__ n_out) {
  __shared__ int s_w[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += 256) {
    const int64_t b = b0 + tid;
    const int v = b < nb ? blk[b] : 0;
    const int incl = wave_incl_scan(v);
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    int base = carry;
    for (int w = 0; w < wv; ++w) base += s_w[w];
    if (b < nb) blk[b] = base + incl - v;
    carry += (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    __syncthreads();
  }
  if (tid == 0) *n_out = carry;
}

// pos[i] = the rank of flagged i among the flagged, -1 for the others
__global__ void __launch_bounds__(256) k_cv_scatter(const uint8_t* __restrict__ flags, int64_t n,
                                                    const int* __restrict__ blk, int32_t* __restrict__ pos) {
  __shared__ int s_c[4];
  const int tid = threadIdx.x, wv = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool keep = i < n && flags[i];
  const uint64_t m = __ballot(keep);
  if ((tid & 63) == 0) s_c[wv] = __popcll(m);
  __syncthreads();
  int p = blk[blockIdx.x] + __popcll(m & lanemask_lt());
  for (int w = 0; w < wv; ++w) p += s_c[w];
  if (i < n) pos[i] = keep ? p : -1;
}

void compact(pfx_ctx* ctx, const uint8_t* flags, int64_t n, int32_t* pos, int* d_total) {
  const int64_t nb = ceil_div(n, 256);
  int* blk = ctx->buf("cvfh_blk").as<int>((size_t)nb + 1);
  k_cv_count<<<(unsigned)nb, 256, 0, ctx->stream>>>(flags, n, blk);
  k_cv_scan<<<1, 256, 0, ctx->stream>>>(blk, nb, d_total);
  k_cv_scatter<<<(unsigned)nb, 256, 0, ctx->stream>>>(flags, n, blk, pos);
  check_launch("cvfh compaction");
}

// ---- the filter ----
__device__ __forceinline__ int32_t index_of(const int32_t* __restrict__ idx, int64_t p) {
  return idx ? idx[p] : (int32_t)p;
}

__global__ void __launch_bounds__(256) k_cvfh_filter(const float* __restrict__ curv, int64_t ns,
                                                     const int32_t* __restrict__ idx, int64_t np, float thr,
                                                     uint8_t* __restrict__ flags, int* __restrict__ w) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const int32_t i = index_of(idx, p);
  if (i < 0 || i >= ns) {  // reported by the call; nothing is read through it
    flags[p] = 0;
    w[kWBadIndex] = 1;
    return;
  }
  flags[p] = !(curv[i] > thr);  // (a NaN curvature is kept)
}

// F: the kept points in order, slots from |F| on stay NaN (filled before)
__global__ void __launch_bounds__(256) k_cvfh_gather(const float* __restrict__ sx, const float* __restrict__ sy,
                                                     const float* __restrict__ sz, const int32_t* __restrict__ idx,
                                                     int64_t np, const int32_t* __restrict__ pos,
                                                     float* __restrict__ fx, float* __restrict__ fy,
                                                     float* __restrict__ fz) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= np) return;
  const int32_t f = pos[p];
  if (f < 0) return;
  const int32_t i = index_of(idx, p);
  fx[f] = sx[i];
  fy[f] = sy[i];
  fz[f] = sz[i];
}

// the indexed point's label: its slot of F's, -1 when the filter dropped it
__global__ void __launch_bounds__(256) k_cvfh_labels(const int32_t* __restrict__ pos, const int32_t* __restrict__ flab,
                                                     int64_t np, int32_t* __restrict__ labels) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < np) labels[p] = pos[p] < 0 ? -1 : flab[pos[p]];
}

// ---- connected components ----
__global__ void __launch_bounds__(256) k_cc_init(int32_t* __restrict__ lab, int32_t* __restrict__ par,
                                                 int32_t* __restrict__ size, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    lab[i] = (int32_t)i;
    par[i] = (int32_t)i;
    size[i] = 0;
  }
}

// one hooking round over the finite points in grid order; round `k` of its batch runs when it is the
// first or the round before changed a parent
__global__ void __launch_bounds__(256)
k_cc_hook(GridView g, const float* __restrict__ nx, const float* __restrict__ ny, const float* __restrict__ nz, float tt,
          float dot_min, const int32_t* __restrict__ lab, int32_t* __restrict__ par, int* __restrict__ w, int k,
          int count_edges) {
  if (k > 0 && w[kWChanged + k - 1] == 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(w + kWRounds, 1);
  const int32_t nf = grid_nfinite(g);
  unsigned long long edges = 0;
  for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < nf; s += (int64_t)gridDim.x * 256) {
    const float4 q = g.sp[s];
    const int32_t i = g.perm[s];
    const float n0 = nx[i], n1 = ny[i], n2 = nz[i];
    const int32_t own = lab[i];
    int32_t m = own;
    Runs R;
    query_runs(g, q.x, q.y, q.z, R);
    const int32_t T = R.pref[9];
    for (int32_t t = 0; t < T; ++t) {
      const int32_t pos = run_pos(R, t);
      const float4 c = g.sp[pos];
      if (pos == s || !(flann_d2(q.x, q.y, q.z, c.x, c.y, c.z) < tt)) continue;
      const int32_t j = g.perm[pos];
      const float dot = (n0 * nx[j] + n1 * ny[j]) + n2 * nz[j];
      if (!(dot_min <= dot && dot <= 1.0f)) continue;  // (a NaN normal: no edge)
      m = min(m, lab[j]);
      edges += j < i;
    }
    if (m < own) {
      atomicMin(par + own, m);
      w[kWChanged + k] = 1;
    }
  }
  if (count_edges) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) edges += __shfl_xor(edges, o);
    if ((threadIdx.x & 63) == 0 && edges) atomicAdd(reinterpret_cast<unsigned long long*>(w + kWEdges), edges);
  }
}

// eight steps up the parents, from one array into another (nothing is read that this launch writes)
__global__ void __launch_bounds__(256) k_cc_jump(const int32_t* __restrict__ par, int32_t* __restrict__ out, int64_t n,
                                                 const int* __restrict__ w, int k) {
  if (w[kWChanged + k] == 0) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int32_t x = par[i];
#pragma unroll 1
  for (int h = 0; h < 7; ++h) {
    const int32_t y = par[x];
    if (y == x) break;
    x = y;
  }
  out[i] = x;
}

// every label to its root (a root is its own parent), and the parents ready for the next round
__global__ void __launch_bounds__(256) k_cc_compress(const int32_t* __restrict__ jumped, int32_t* __restrict__ lab,
                                                     int32_t* __restrict__ par, int64_t n, const int* __restrict__ w,
                                                     int k) {
  if (w[kWChanged + k] == 0) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int32_t x = lab[i];
  for (int32_t y = jumped[x]; y != x; y = jumped[x]) x = y;  // (the parents only descend: it ends)
  lab[i] = x;
  par[i] = x;
}

__global__ void __launch_bounds__(256) k_cc_sizes(GridView g, const int32_t* __restrict__ lab,
                                                  int32_t* __restrict__ size) {
  const int32_t nf = grid_nfinite(g);
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s < nf) atomicAdd(size + lab[g.perm[s]], 1);  // (a non-finite point is in no component)
}

__global__ void __launch_bounds__(256) k_cc_roots(const int32_t* __restrict__ lab, const int32_t* __restrict__ size,
                                                  int64_t n, int32_t min_points, uint8_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) flags[i] = lab[i] == i && size[i] >= min_points;
}

__global__ void __launch_bounds__(256) k_cc_labels(const int32_t* __restrict__ lab, const int32_t* __restrict__ size,
                                                   const int32_t* __restrict__ rank, int64_t n,
                                                   int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) labels[i] = size[lab[i]] > 0 ? rank[lab[i]] : -1;  // (size 0: a non-finite point)
}

// the smallest float T with acos((double)T) < eps, by bisection over the floats of [-1, 1] in their
// order; +inf when no float passes (then `T <= dot` never holds)
float acos_threshold(double eps) {
  auto pass = [&](float v) { return std::fabs(std::acos((double)v)) < eps; };
  auto key = [](float v) {  // an int that orders as the float does
    int32_t b;
    std::memcpy(&b, &v, 4);
    return b >= 0 ? (int64_t)b : -(int64_t)(b & 0x7fffffff);
  };
  auto unkey = [](int64_t k) {
    const int32_t b = k >= 0 ? (int32_t)k : (int32_t)(0x80000000u | (uint32_t)(-k));
    float v;
    std::memcpy(&v, &b, 4);
    return v;
  };
  if (!pass(1.0f)) return INFINITY;
  if (pass(-1.0f)) return -1.0f;
  int64_t lo = key(-1.0f), hi = key(1.0f);  // pass(hi), !pass(lo)
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (pass(unkey(mid))) hi = mid;
    else lo = mid;
  }
  return unkey(hi);
}

// The components of n points; labels: the cluster row or -1.  w: the call's zeroed words, all copied
// to h (pinned) at every look of the host.  Returns the number of clusters.
int64_t clusters_run(pfx_ctx* ctx, const float* x, const float* y, const float* z, const float* nx, const float* ny,
                     const float* nz, int64_t n, float tolerance, double eps_angle, int32_t min_points,
                     int32_t* labels, int* w, int* h) {
  hipStream_t st = ctx->stream;
  const double t = (double)tolerance;
  const float tt = (float)(t * t), dot_min = acos_threshold(eps_angle);
  const GridView g = feature_grid(ctx, x, y, z, n, t);
  const unsigned nb = (unsigned)ceil_div(n, 256);
  int32_t* lab = ctx->buf("cvfh_lab").as<int32_t>((size_t)n * 5);
  int32_t *par = lab + n, *jumped = par + n, *size = jumped + n, *rank = size + n;
  uint8_t* flags = ctx->buf("cvfh_root").as<uint8_t>((size_t)n);
  {
    TimeScope ts(ctx, "cvfh_components", true);
    k_cc_init<<<nb, 256, 0, st>>>(lab, par, size, n);
    check_launch("k_cc_init");
  }
  const unsigned hook_blocks = std::min<unsigned>(nb, 4096);
  for (bool first = true;; first = false) {
    {
      TimeScope ts(ctx, "cvfh_components", true);
      for (int k = 0; k < kCcBatch; ++k) {
        k_cc_hook<<<hook_blocks, 256, 0, st>>>(g, nx, ny, nz, tt, dot_min, lab, par, w, k, first && k == 0);
        k_cc_jump<<<nb, 256, 0, st>>>(par, jumped, n, w, k);
        k_cc_compress<<<nb, 256, 0, st>>>(jumped, lab, par, n, w, k);
      }
      check_launch("k_cc_hook");
    }
    {
      TimeScope ts(ctx, "cvfh_rank", true);
      k_cc_sizes<<<nb, 256, 0, st>>>(g, lab, size);
      k_cc_roots<<<nb, 256, 0, st>>>(lab, size, n, min_points, flags);
      compact(ctx, flags, n, rank, w + kWClusters);
      k_cc_labels<<<nb, 256, 0, st>>>(lab, size, rank, n, labels);
      check_launch("k_cc_labels");
    }
    PFX_HIP(hipMemcpyAsync(h, w, sizeof(int) * kWords, hipMemcpyDeviceToHost, st));
    ctx->sync_spin(st);
    if (h[kWChanged + kCcBatch - 1] == 0) break;
    // more than a batch of rounds: the flags and the sizes cleared, and on
    PFX_HIP(hipMemsetAsync(w + kWChanged, 0, sizeof(int) * kCcBatch, st));
    PFX_HIP(hipMemsetAsync(size, 0, sizeof(int32_t) * n, st));
  }
  unsigned long long edges;
  std::memcpy(&edges, h + kWEdges, sizeof(edges));
  ctx->stats["cvfh_edges"] = (int64_t)edges;
  ctx->stats["cvfh_cc_rounds"] = h[kWRounds];
  ctx->stats["cvfh_clusters"] = h[kWClusters];
  return h[kWClusters];
}

int* call_words(pfx_ctx* ctx) {
  int* w = ctx->buf("cvfh_words").as<int>(kWords);
  PFX_HIP(hipMemsetAsync(w, 0, sizeof(int) * kWords, ctx->stream));
  return w;
}

// ---- the clusters' mean point and normalised mean normal ----
// One workgroup a cluster.  256 labels at a time; the members' six floats go to LDS in index order
// (ballot ranks), then lane c of the first wave adds coordinate c member after member: Vector4f +=.
__global__ void __launch_bounds__(256)
k_cvfh_means(const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ fz,
             const float* __restrict__ fnx, const float* __restrict__ fny, const float* __restrict__ fnz,
             const int32_t* __restrict__ flab, int64_t n, float* __restrict__ cen, float* __restrict__ dn) {
  __shared__ float s_v[256][6];
  __shared__ int s_c[4];
  __shared__ float s_sum[6];
  const int tid = threadIdx.x, wv = tid >> 6, row = blockIdx.x;
  float sum = 0.0f;
  int members = 0;
  for (int64_t b = 0; b < n; b += 256) {
    const int64_t j = b + tid;
    const bool in = j < n && flab[j] == row;
    const uint64_t m = __ballot(in);
    if ((tid & 63) == 0) s_c[wv] = __popcll(m);
    __syncthreads();
    int p = __popcll(m & lanemask_lt());
    for (int u = 0; u < wv; ++u) p += s_c[u];
    const int cnt = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    if (in) {
      s_v[p][0] = fx[j];
      s_v[p][1] = fy[j];
      s_v[p][2] = fz[j];
      s_v[p][3] = fnx[j];
      s_v[p][4] = fny[j];
      s_v[p][5] = fnz[j];
    }
    __syncthreads();
    if (tid < 6)
      for (int e = 0; e < cnt; ++e) sum = sum + s_v[e][tid];
    members += cnt;
    __syncthreads();
  }
  if (tid < 6) s_sum[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    const float inv = 1.0f / (float)members;  // Eigen 3.2's `/=`: times the reciprocal
    const f3 c = scale3(mk3(s_sum[0], s_sum[1], s_sum[2]), inv);
    const f3 a = scale3(mk3(s_sum[3], s_sum[4], s_sum[5]), inv);
    const f3 d = scale3(a, 1.0f / sqrtf(sqn4(a)));  // Vector4f::normalize, w = 0
    cen[row * 3 + 0] = c.x;
    cen[row * 3 + 1] = c.y;
    cen[row * 3 + 2] = c.z;
    dn[row * 3 + 0] = d.x;
    dn[row * 3 + 1] = d.y;
    dn[row * 3 + 2] = d.z;
  }
}

// No cluster: the centroid of the whole surface and the mean of the indexed normals, non-finite ones
// skipped, as sequential float sums.  One workgroup stages 1,024 triples a time through LDS; three
// lanes add (the form of k_res_sequential).
__global__ void __launch_bounds__(256)
k_cvfh_fallback(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
                const float* __restrict__ snx, const float* __restrict__ sny, const float* __restrict__ snz, int64_t ns,
                const int32_t* __restrict__ idx, int64_t np, float* __restrict__ cen, float* __restrict__ dn) {
  constexpr int kStage = 1024;
  __shared__ float s_v[kStage][3];
  __shared__ uint8_t s_ok[kStage];
  const int tid = threadIdx.x;
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t n = pass == 0 ? ns : np;
    float sum = 0.0f;
    int cnt = 0;
    for (int64_t b = 0; b < n; b += kStage) {
      for (int e = tid; e < kStage; e += 256) {
        const int64_t j = b + e;
        float a = 0.f, c = 0.f, d = 0.f;
        bool ok = false;
        if (j < n) {
          const int64_t i = pass == 0 ? j : (int64_t)index_of(idx, j);
          if (i >= 0 && i < ns) {
            a = pass == 0 ? sx[i] : snx[i];
            c = pass == 0 ? sy[i] : sny[i];
            d = pass == 0 ? sz[i] : snz[i];
            ok = isfinite(a) && isfinite(c) && isfinite(d);
          }
        }
        s_v[e][0] = a;
        s_v[e][1] = c;
        s_v[e][2] = d;
        s_ok[e] = ok;
      }
      __syncthreads();
      if (tid < 3) {
        const int m = n - b < kStage ? (int)(n - b) : kStage;
        for (int e = 0; e < m; ++e)
          if (s_ok[e]) {
            sum = sum + s_v[e][tid];
            ++cnt;
          }
      }
      __syncthreads();
    }
    if (tid < 3) (pass == 0 ? cen : dn)[tid] = sum * (1.0f / (float)cnt);
  }
}

// ---- the signature ----
// the largest |p - c| of the indexed points of every row, as the bits of a non-negative float (-1:
// none); NaN distances are skipped
__global__ void __launch_bounds__(256)
k_cvfh_maxdist(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int64_t ns,
               const int32_t* __restrict__ idx, int64_t np, const float* __restrict__ cen, int* __restrict__ maxbits) {
  const int row = blockIdx.x;
  const f3 c = mk3(cen[row * 3], cen[row * 3 + 1], cen[row * 3 + 2]);
  int best = -1;
  for (int64_t p = (int64_t)blockIdx.y * 256 + threadIdx.x; p < np; p += (int64_t)gridDim.y * 256) {
    const int32_t i = index_of(idx, p);
    if (i < 0 || i >= ns) continue;
    const float d = sqrtf(sqn3(sub3(c, mk3(sx[i], sy[i], sz[i]))));
    if (d == d) best = max(best, __float_as_int(d));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o));
  if ((threadIdx.x & 63) == 0 && best >= 0) atomicMax(maxbits + row, best);
}

constexpr int kVfhShape = 45, kVfhVp = 128;

__global__ void __launch_bounds__(256)
k_cvfh_hist(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz,
            const float* __restrict__ snx, const float* __restrict__ sny, const float* __restrict__ snz, int64_t ns,
            const int32_t* __restrict__ idx, int64_t np, const float* __restrict__ cen, const float* __restrict__ dn,
            const int* __restrict__ maxbits, float vx, float vy, float vz, int* __restrict__ counts) {
  __shared__ int s_h[PFX_CVFH_DIM];
  const int row = blockIdx.x, tid = threadIdx.x;
  for (int b = tid; b < PFX_CVFH_DIM; b += 256) s_h[b] = 0;
  __syncthreads();
  const f3 c = mk3(cen[row * 3], cen[row * 3 + 1], cen[row * 3 + 2]);
  const f3 n1 = mk3(dn[row * 3], dn[row * 3 + 1], dn[row * 3 + 2]);
  const int mb = maxbits[row];
  const double factor = mb < 0 ? (double)__builtin_nanf("") : (double)__int_as_float(mb);
  f3 d = sub3(mk3(vx, vy, vz), c);
  d = scale3(d, 1.0f / sqrtf(sqn4(d)));  // Vector4f::normalize, w = 0
  for (int64_t p = (int64_t)blockIdx.y * 256 + tid; p < np; p += (int64_t)gridDim.y * 256) {
    const int32_t i = index_of(idx, p);
    if (i < 0 || i >= ns) continue;
    const f3 pt = mk3(sx[i], sy[i], sz[i]), nn = mk3(snx[i], sny[i], snz[i]);
    int h1, h2, h3;
    if (pair_bins<kVfhShape>(c, n1, pt, nn, h1, h2, h3)) {
      const float f4 = sqrtf(sqn4(sub3(pt, c)));
      const int h4 = bin_of<kVfhShape>((double)kVfhShape * ((double)f4 / factor));
      atomicAdd(&s_h[h1], 1);
      atomicAdd(&s_h[kVfhShape + h2], 1);
      atomicAdd(&s_h[2 * kVfhShape + h3], 1);
      atomicAdd(&s_h[3 * kVfhShape + h4], 1);
    }
    const double alpha = ((double)dot4(nn, d) + 1.0) * 0.5;
    atomicAdd(&s_h[4 * kVfhShape + bin_of<kVfhVp>(alpha * (double)kVfhVp)], 1);
  }
  __syncthreads();
  for (int b = tid; b < PFX_CVFH_DIM; b += 256)
    if (s_h[b]) atomicAdd(counts + (int64_t)row * PFX_CVFH_DIM + b, s_h[b]);
}

// counts -> floats: the bin is `count` additions of its increment
__global__ void __launch_bounds__(256) k_cvfh_rows(const int* __restrict__ counts, int64_t total, float incr_shape,
                                                   float incr_vp, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int b = (int)(e % PFX_CVFH_DIM);
  out[e] = repeated_add(b < 4 * kVfhShape ? incr_shape : incr_vp, counts[e]);
}

}  // namespace

void smooth_clusters_dev(pfx_ctx* ctx, const float* x, const float* y, const float* z, const float* nx, const float* ny,
                         const float* nz, int64_t n, float tolerance, double eps_angle, int32_t min_points,
                         int32_t* labels, int64_t* d_n_clusters) {
  hipStream_t st = ctx->stream;
  int64_t c = 0;
  ctx->stats["cvfh_edges"] = ctx->stats["cvfh_cc_rounds"] = ctx->stats["cvfh_clusters"] = 0;
  if (n > 0) c = clusters_run(ctx, x, y, z, nx, ny, nz, n, tolerance, eps_angle, min_points, labels, call_words(ctx),
                              ctx->readback<int>());
  k_fill<<<1, 256, 0, st>>>(d_n_clusters, (int64_t)1, c);
  check_launch("k_fill");
}

int64_t cvfh_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
                 const float* snz, const float* scurv, int64_t ns, const int32_t* indices, int64_t np,
                 const pfx_cvfh_params& prm, float* out, int64_t cap, int64_t* d_n_rows, float* centroids,
                 float* dominant_normals, int32_t* labels) {
  hipStream_t st = ctx->stream;
  for (const char* s : {"cvfh_filtered", "cvfh_clusters", "cvfh_edges", "cvfh_cc_rounds", "cvfh_rows"}) ctx->stats[s] = 0;
  if (np == 0) {
    k_fill<<<1, 256, 0, st>>>(d_n_rows, (int64_t)1, (int64_t)0);
    check_launch("k_fill");
    return 0;
  }
  const unsigned nb = (unsigned)ceil_div(np, 256);
  int* w = call_words(ctx);
  int* h = ctx->readback<int>();
  // ---- the filter, and F padded with NaN points to np ----
  uint8_t* flags = ctx->buf("cvfh_flags").as<uint8_t>((size_t)np);
  int32_t* pos = ctx->buf("cvfh_pos").as<int32_t>((size_t)np * 2);
  int32_t* flab = pos + np;
  float* fx = ctx->buf("cvfh_f").as<float>((size_t)np * 7);
  float *fy = fx + np, *fz = fy + np, *fnx = fz + np, *fny = fnx + np, *fnz = fny + np, *fcurv = fnz + np;
  {
    TimeScope ts(ctx, "cvfh_filter", true);
    k_cvfh_filter<<<nb, 256, 0, st>>>(scurv, ns, indices, np, prm.curvature_threshold, flags, w);
    compact(ctx, flags, np, pos, w + kWFiltered);
    k_fill<<<(unsigned)ceil_div(3 * np, 256), 256, 0, st>>>(fx, 3 * np, __builtin_nanf(""));
    k_cvfh_gather<<<nb, 256, 0, st>>>(sx, sy, sz, indices, np, pos, fx, fy, fz);
    check_launch("k_cvfh_gather");
  }
  // ---- its own normals (a fresh estimation: the viewpoint is the origin, not the call's) ----
  const float vp0[3] = {0.f, 0.f, 0.f};
  normals_dev(ctx, fx, fy, fz, np, (double)prm.radius_normals, vp0, fnx, fny, fnz, fcurv);
  // ---- the clusters; with fewer than min_points points in F no component reaches min_points ----
  const int64_t nc = clusters_run(ctx, fx, fy, fz, fnx, fny, fnz, np, prm.cluster_tolerance,
                                  (double)prm.eps_angle_threshold, prm.min_points, flab, w, h);
  if (h[kWBadIndex]) throw Error(PFX_ERR_INVALID, "cvfh: an index is outside the surface");
  const int64_t rows = nc > 0 ? nc : 1;
  ctx->stats["cvfh_filtered"] = h[kWFiltered];
  ctx->stats["cvfh_rows"] = rows;
  k_fill<<<1, 256, 0, st>>>(d_n_rows, (int64_t)1, rows);
  check_launch("k_fill");
  if (rows > cap)
    throw Error(PFX_ERR_CAPACITY, "cvfh: " + std::to_string(rows) + " rows (cap " + std::to_string(cap) + ")");
  if (labels) {
    k_cvfh_labels<<<nb, 256, 0, st>>>(pos, flab, np, labels);
    check_launch("k_cvfh_labels");
  }
  // ---- what every row is about ----
  float* cen = ctx->buf("cvfh_about").as<float>((size_t)rows * 6);
  float* dn = cen + rows * 3;
  {
    TimeScope ts(ctx, nc > 0 ? "cvfh_means" : "cvfh_fallback", true);
    if (nc > 0)
      k_cvfh_means<<<(unsigned)nc, 256, 0, st>>>(fx, fy, fz, fnx, fny, fnz, flab, np, cen, dn);
    else
      k_cvfh_fallback<<<1, 256, 0, st>>>(sx, sy, sz, snx, sny, snz, ns, indices, np, cen, dn);
    check_launch("k_cvfh_means");
  }
  // ---- the signatures ----
  int* counts = ctx->buf("cvfh_counts").as<int>((size_t)rows * (PFX_CVFH_DIM + 1));
  int* maxbits = counts + rows * PFX_CVFH_DIM;
  {
    TimeScope ts(ctx, "cvfh_signature", true);
    PFX_HIP(hipMemsetAsync(counts, 0, sizeof(int) * rows * PFX_CVFH_DIM, st));
    PFX_HIP(hipMemsetAsync(maxbits, 0xff, sizeof(int) * rows, st));  // -1: no distance yet
    // (rows x chunks) workgroups: the chunks fill the device once at a few rows
    const dim3 grid((unsigned)rows, (unsigned)std::min<int64_t>(nb, std::max<int64_t>(1, 2048 / rows)));
    k_cvfh_maxdist<<<grid, 256, 0, st>>>(sx, sy, sz, ns, indices, np, cen, maxbits);
    k_cvfh_hist<<<grid, 256, 0, st>>>(sx, sy, sz, snx, sny, snz, ns, indices, np, cen, dn, maxbits, prm.viewpoint[0],
                                      prm.viewpoint[1], prm.viewpoint[2], counts);
    const float incr_shape = prm.normalize_bins ? 100.0f / (float)(np - 1) : 1.0f;
    const float incr_vp = prm.normalize_bins ? (float)(100.0 / (double)np) : 1.0f;
    k_cvfh_rows<<<(unsigned)ceil_div(rows * PFX_CVFH_DIM, 256), 256, 0, st>>>(counts, rows * PFX_CVFH_DIM, incr_shape,
                                                                               incr_vp, out);
    check_launch("k_cvfh_rows");
  }
  if (centroids) PFX_HIP(hipMemcpyAsync(centroids, cen, sizeof(float) * rows * 3, hipMemcpyDeviceToDevice, st));
  if (dominant_normals)
    PFX_HIP(hipMemcpyAsync(dominant_normals, dn, sizeof(float) * rows * 3, hipMemcpyDeviceToDevice, st));
  return rows;
}

}  // namespace pfx
