// pfx_icp.hip -- the reference's ICP refinement (evaluation.cpp:863-885, icpAlign):
//
//   pcl::IterativeClosestPoint<PointXYZRGB,PointXYZRGB>::align      PCL 1.7.2 icp.hpp
//     correspondence estimation (1-NN, distance cap), Umeyama's rigid fit in float
//     (transformation_estimation_svd.hpp, Eigen 3.2 Umeyama.h), DefaultConvergenceCriteria,
//     getFitnessScore() -- the arithmetic is DESIGN.md "ICP: the contract", restated on the CPU
//     in tests/cpp/icp_ref.cpp (parity vs PCL unpinned there).
//
// Design (MI355X): the target lies in up to kIcpLevels uniform grids of cell h, 2h, 4h, 8h, built
// once per call.  One iteration is a fixed sequence of launches with every count kept on the
// device, and one host synchronisation:
//   search: lane per source point over the 3x3x3 block of the first grid; the nearest point is
//     certified when its d2 <= h^2 (1 - 1e-5): every point outside the block is farther than h,
//     and the margin covers the rounding of the float d2.  Uncertified queries go to a queue and
//     are retried on the next grid; a grid whose h^2 (1 - 1e-5) >= max_dist^2 certifies "no
//     correspondence" for what it cannot certify.  What is left after the last grid is scanned
//     exhaustively, four queries per workgroup pass.  Every level is launched unconditionally on the
//     device-side queue length; every loop is bounded by that length.
//   compaction: kept pairs in source order (ballot + block scan) into the correspondence list
//     (source xyz, target xyz, d2); list positions past the end hold NaN = "no term".
//   means: six sequential float chains over the list, one lane each, from LDS tiles that the other
//     waves of the workgroup stage one tile ahead.  Inherently serial (float sums do not commute).
//   sigma: one workgroup per depth block of PFX_ICP_GEMM_DEPTH list positions, nine chains each;
//     one wave then combines the blocks in order.
//   mean squared error: the exact integer sum of pfx_exact_sum.h over the list's d2; where the terms
//     do not fit it (full-size clouds), its sequential loop and a second synchronisation.
// The host reads 15 floats, the pair count and the sum, runs the 3x3 SVD (pfx_svd3.h), tests
// convergence and passes T to the next launch as a kernel argument.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "pfx_exact_sum.h"
#include "pfx_internal.h"
#include "pfx_neighbors.h"
#include "pfx_svd3.h"

namespace pfx {

constexpr int kIcpLevels = 4;
constexpr int kIcpGemmDepth = PFX_ICP_GEMM_DEPTH;
constexpr int kIcpTile = 1024;  // list positions per LDS tile of the mean chains
constexpr int kIcpPad = 4;      // row padding (floats): rows stay 16-byte aligned, 4 banks apart

struct IcpState {
  Grid lv[kIcpLevels];
};

void icp_release(pfx_ctx* ctx) {
  if (!ctx->icp) return;
  for (auto& g : ctx->icp->lv) g.release();
  delete ctx->icp;
  ctx->icp = nullptr;
}

namespace {

struct Mat4 {
  float m[16];
};

// everything the host reads once per iteration
struct IcpReadback {
  int cnt[8];  // [0] kept pairs n, [k] queue length entering level k (1..kIcpLevels: the last = exhaustive)
  float mean[6];   // source x y z, target x y z
  float sigma[9];  // row-major, sigma(i, j): i target axis, j source axis
  float pad;
  ResAcc acc;  // sum of the list's d2
};

__device__ __forceinline__ float qnanf() { return __int_as_float(0x7fc00000); }

// step 5 / step 7 of the contract: ((m0 x + m1 y) + m2 z) + m3 per row
__global__ void __launch_bounds__(256) k_icp_transform(const float* __restrict__ ix, const float* __restrict__ iy,
                                                       const float* __restrict__ iz, int64_t n, Mat4 T,
                                                       float* __restrict__ ox, float* __restrict__ oy,
                                                       float* __restrict__ oz) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = ix[i], y = iy[i], z = iz[i];
  ox[i] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  oy[i] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  oz[i] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
}

// nearest target point of each query from its 3x3x3 block (queue == nullptr: every source
// point); lowest target index among equal d2.  Certified -> nn_idx/nn_d2, certified none (and
// non-finite queries) -> index -1, the others -> failq.
__global__ void __launch_bounds__(256) k_icp_nn(GridView g, const float* __restrict__ wx, const float* __restrict__ wy,
                                                const float* __restrict__ wz, int64_t ns,
                                                const int32_t* __restrict__ queue, const int* __restrict__ n_queue,
                                                float hh, int none_ok, int32_t* __restrict__ nn_idx,
                                                float* __restrict__ nn_d2, int32_t* __restrict__ failq,
                                                int* __restrict__ n_fail) {
  const int64_t count = queue ? (int64_t)*n_queue : ns;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += stride) {
    const int32_t i = queue ? queue[t] : (int32_t)t;
    const float qx = wx[i], qy = wy[i], qz = wz[i];
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {
      nn_idx[i] = -1;
      nn_d2[i] = qnanf();
      continue;
    }
    Runs R;
    query_runs(g, qx, qy, qz, R);
    float bd = INFINITY;
    int32_t bi = -1;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
      const int32_t s = R.start[r], e = s + (R.pref[r + 1] - R.pref[r]);
#pragma unroll 2
      for (int32_t p = s; p < e; ++p) {
        const float4 c = g.sp[p];
        const float d = flann_d2(qx, qy, qz, c.x, c.y, c.z);
        if (d <= bd) {
          const int32_t j = g.perm[p];
          if (d < bd || bi < 0 || j < bi) {
            bd = d;
            bi = j;
          }
        }
      }
    }
    if (bi >= 0 && bd <= hh) {
      nn_idx[i] = bi;
      nn_d2[i] = bd;
    } else if (none_ok) {
      nn_idx[i] = -1;
      nn_d2[i] = qnanf();
    } else {
      failq[wave_push_slot(n_fail)] = i;  // at most one push per query and level: < ns entries
    }
  }
}

// exhaustive nearest of the queued queries: a workgroup takes kIcpBruteQ queries at a time over
// every finite target point (one target load serves all of them: the scan is bound by L2 traffic,
// not arithmetic); per lane the smallest (d2, index), then the minimum of the 64-bit keys
constexpr int kIcpBruteQ = 4;

__global__ void __launch_bounds__(256) k_icp_brute(GridView g, const float* __restrict__ wx,
                                                   const float* __restrict__ wy, const float* __restrict__ wz,
                                                   const int32_t* __restrict__ queue, const int* __restrict__ n_queue,
                                                   int32_t* __restrict__ nn_idx, float* __restrict__ nn_d2) {
  __shared__ unsigned long long s_k[kIcpBruteQ][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nq = *n_queue;
  const int32_t nf = grid_nfinite(g);
  for (int q0 = blockIdx.x * kIcpBruteQ; q0 < nq; q0 += gridDim.x * kIcpBruteQ) {  // uniform per workgroup
    float qx[kIcpBruteQ], qy[kIcpBruteQ], qz[kIcpBruteQ], bd[kIcpBruteQ];
    int32_t bi[kIcpBruteQ];
#pragma unroll
    for (int u = 0; u < kIcpBruteQ; ++u) {
      const int32_t i = queue[min(q0 + u, nq - 1)];  // a short last group repeats its last query
      qx[u] = wx[i];
      qy[u] = wy[i];
      qz[u] = wz[i];
      bd[u] = INFINITY;
      bi[u] = -1;
    }
    for (int32_t p = tid; p < nf; p += 256) {
      const float4 c = g.sp[p];
#pragma unroll
      for (int u = 0; u < kIcpBruteQ; ++u) {
        const float d = flann_d2(qx[u], qy[u], qz[u], c.x, c.y, c.z);
        if (d <= bd[u]) {  // rare after the first few points: the index is loaded only here
          const int32_t j = g.perm[p];
          if (d < bd[u] || bi[u] < 0 || j < bi[u]) {
            bd[u] = d;
            bi[u] = j;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kIcpBruteQ; ++u) {
      unsigned long long best = bi[u] >= 0 ? nb_key(bd[u], bi[u]) : ~0ull;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long k = __shfl_xor(best, o);
        best = k < best ? k : best;
      }
      if (lane == 0) s_k[u][wv] = best;
    }
    __syncthreads();
    if (tid < kIcpBruteQ && q0 + tid < nq) {
      unsigned long long best = s_k[tid][0];
      for (int w = 1; w < 4; ++w) best = s_k[tid][w] < best ? s_k[tid][w] : best;
      const bool any = best != ~0ull;
      const int32_t i = queue[q0 + tid];
      nn_idx[i] = any ? key_idx(best) : -1;
      nn_d2[i] = any ? key_d2(best) : qnanf();
    }
    __syncthreads();
  }
}

__device__ __forceinline__ bool icp_keep(const int32_t* nn_idx, const float* nn_d2, int64_t i, int64_t ns,
                                         double maxd2) {
  return i < ns && nn_idx[i] >= 0 && !((double)nn_d2[i] > maxd2);
}

// kept pairs per block of 256 source points
__global__ void __launch_bounds__(256) k_icp_count(const int32_t* __restrict__ nn_idx, const float* __restrict__ nn_d2,
                                                   int64_t ns, double maxd2, int* __restrict__ blk) {
  __shared__ int s_c[4];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const uint64_t m = __ballot(icp_keep(nn_idx, nn_d2, i, ns, maxd2));
  if ((tid & 63) == 0) s_c[tid >> 6] = __popcll(m);
  __syncthreads();
  if (tid == 0) blk[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

// exclusive scan of the block counts in place (one workgroup), total -> *n_out
__global__ void __launch_bounds__(256) k_icp_scan(int* __restrict__ blk, int64_t nb, int* __restrict__ n_out) {
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

// the list, in source order: rows 0..2 working source xyz, 3..5 target xyz, 6 d2 (row stride ld);
// list positions >= n get NaN in the d2 row ("no term" for the exact sum)
__global__ void __launch_bounds__(256) k_icp_scatter(const int32_t* __restrict__ nn_idx, const float* __restrict__ nn_d2,
                                                     int64_t ns, double maxd2, const int* __restrict__ blk,
                                                     const int* __restrict__ n_ptr, const float* __restrict__ wx,
                                                     const float* __restrict__ wy, const float* __restrict__ wz,
                                                     const float* __restrict__ tx, const float* __restrict__ ty,
                                                     const float* __restrict__ tz, float* __restrict__ L, int64_t ld) {
  __shared__ int s_c[4];
  const int tid = threadIdx.x, wv = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const bool keep = icp_keep(nn_idx, nn_d2, i, ns, maxd2);
  const uint64_t m = __ballot(keep);
  if ((tid & 63) == 0) s_c[wv] = __popcll(m);
  __syncthreads();
  int pos = blk[blockIdx.x] + __popcll(m & lanemask_lt());
  for (int w = 0; w < wv; ++w) pos += s_c[w];
  if (keep) {  // pos < n <= ns
    const int32_t j = nn_idx[i];
    L[pos] = wx[i];
    L[ld + pos] = wy[i];
    L[2 * ld + pos] = wz[i];
    L[3 * ld + pos] = tx[j];
    L[4 * ld + pos] = ty[j];
    L[5 * ld + pos] = tz[j];
    L[6 * ld + pos] = nn_d2[i];
  }
  if (i < ns && i >= *n_ptr) L[6 * ld + i] = qnanf();
}

// one tile of the six list rows into LDS by NT threads: every load of a thread is issued before its
// first LDS store (a load-store loop waits out one memory latency per element)
template <int NT>
__device__ __forceinline__ void icp_stage_tile(const float* __restrict__ L, int64_t ld, int64_t base, int n, int t,
                                               float (*s)[kIcpTile + kIcpPad]) {
  constexpr int kPer = 6 * kIcpTile / NT;
  static_assert(kPer * NT == 6 * kIcpTile, "tile not divisible among the threads");
  float v[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = t + NT * u, r = e / kIcpTile, k = e % kIcpTile;
    v[u] = base + k < n ? L[r * ld + base + k] : 0.0f;
  }
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = t + NT * u;
    s[e / kIcpTile][e % kIcpTile] = v[u];
  }
}

// the six means: sum_k v[k] in list order, started from the first term, times a = 1 / (float)n.
// Wave 0 adds (lane c = chain c) while waves 1..3 stage the next tile.
__global__ void __launch_bounds__(256) k_icp_means(const float* __restrict__ L, int64_t ld,
                                                   const int* __restrict__ n_ptr, float* __restrict__ mean) {
  __shared__ __attribute__((aligned(16))) float s[2][6][kIcpTile + kIcpPad];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = *n_ptr;
  const int ntiles = (n + kIcpTile - 1) / kIcpTile;
  icp_stage_tile<256>(L, ld, 0, n, tid, s[0]);
  __syncthreads();
  float acc = -0.0f;  // -0 + v == v for every v: the sum starts from its first term
  for (int t = 0; t < ntiles; ++t) {  // uniform per workgroup
    const int buf = t & 1;
    if (wv > 0) {
      if (t + 1 < ntiles) icp_stage_tile<192>(L, ld, (int64_t)(t + 1) * kIcpTile, n, tid - 64, s[buf ^ 1]);
    } else if (lane < 6) {
      const int cnt = min(kIcpTile, n - t * kIcpTile);
      const float* p = s[buf][lane];
      int k = 0;
#pragma unroll 4
      for (; k + 4 <= cnt; k += 4) {
        const float4 v = *reinterpret_cast<const float4*>(p + k);
        acc = acc + v.x;
        acc = acc + v.y;
        acc = acc + v.z;
        acc = acc + v.w;
      }
      for (; k < cnt; ++k) acc = acc + p[k];
    }
    __syncthreads();
  }
  if (tid < 6) mean[tid] = acc * (1.0f / (float)n);
}

// P_b(i, j) = sum over the depth block of dst_dm[i][k] * src_dm[j][k], from 0, in order
__global__ void __launch_bounds__(256) k_icp_sigma(const float* __restrict__ L, int64_t ld,
                                                   const int* __restrict__ n_ptr, const float* __restrict__ mean,
                                                   float* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) float s[6][kIcpGemmDepth + kIcpPad];
  const int tid = threadIdx.x;
  const int n = *n_ptr;
  const int64_t base = (int64_t)blockIdx.x * kIcpGemmDepth;
  if (base >= n) return;  // uniform per workgroup
  const int cnt = (int)min((int64_t)kIcpGemmDepth, n - base);
  constexpr int kPer = 6 * kIcpGemmDepth / 256;
  float v[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {  // every load issued before the first LDS store
    const int e = tid + 256 * u, r = e / kIcpGemmDepth, k = e % kIcpGemmDepth;
    v[u] = k < cnt ? L[r * ld + base + k] - mean[r] : 0.0f;
  }
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int e = tid + 256 * u;
    s[e / kIcpGemmDepth][e % kIcpGemmDepth] = v[u];
  }
  __syncthreads();
  if (tid < 9) {
    const float* d = s[3 + tid / 3];
    const float* c = s[tid % 3];
    float acc = 0.0f;
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) acc = acc + d[k] * c[k];
    P[(int64_t)blockIdx.x * 9 + tid] = acc;
  }
}

// sigma(i, j) = sum_b a P_b(i, j), from 0, in block order; the means ride along to the host
__global__ void __launch_bounds__(64) k_icp_combine(const float* __restrict__ P, const float* __restrict__ mean,
                                                    IcpReadback* __restrict__ rb) {
  const int tid = threadIdx.x;
  const int n = rb->cnt[0];
  const int nb = (n + kIcpGemmDepth - 1) / kIcpGemmDepth;
  const float a = 1.0f / (float)n;
  if (tid < 9) {
    float acc = 0.0f;
    for (int b = 0; b < nb; ++b) acc = acc + a * P[b * 9 + tid];
    rb->sigma[tid] = acc;
  }
  if (tid < 6) rb->mean[tid] = mean[tid];
}

// fitness terms: d2 of every source point that has a nearest target point, NaN otherwise
__global__ void __launch_bounds__(256) k_icp_terms(const int32_t* __restrict__ nn_idx, const float* __restrict__ nn_d2,
                                                   int64_t ns, float* __restrict__ term) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  term[i] = nn_idx[i] >= 0 ? nn_d2[i] : qnanf();
}

struct Search {
  IcpState* S;
  float hh[kIcpLevels];     // certification bound of each grid: h^2 (1 - 1e-5)
  int32_t *nn_idx, *qa, *qb;
  float* nn_d2;
  IcpReadback* rb;  // device
};

// launches one search of the ns queries; levels: grids to use (the last may certify "none" when
// its bound reaches maxd2); returns whether the exhaustive tail was launched
bool nn_search(pfx_ctx* ctx, const Search& s, const float* wx, const float* wy, const float* wz, int64_t ns,
               double maxd2, int levels) {
  hipStream_t st = ctx->stream;
  PFX_HIP(hipMemsetAsync(s.rb->cnt, 0, sizeof(int) * 8, st));
  const unsigned nblk = (unsigned)std::min<int64_t>(ceil_div(ns, 256), 2048);
  bool closed = false;
  for (int k = 0; k < levels; ++k) {
    const int none_ok = (double)s.hh[k] >= maxd2 ? 1 : 0;
    const int32_t* queue = k == 0 ? nullptr : ((k & 1) ? s.qa : s.qb);
    int32_t* fail = (k & 1) ? s.qb : s.qa;
    k_icp_nn<<<nblk, 256, 0, st>>>(view(s.S->lv[k]), wx, wy, wz, ns, queue, s.rb->cnt + k, s.hh[k], none_ok, s.nn_idx,
                                   s.nn_d2, fail, s.rb->cnt + k + 1);
    check_launch("k_icp_nn");
    if (none_ok) {
      closed = true;
      break;
    }
  }
  if (closed) return false;
  const int32_t* queue = (levels & 1) ? s.qa : s.qb;
  k_icp_brute<<<nblk, 256, 0, st>>>(view(s.S->lv[0]), wx, wy, wz, queue, s.rb->cnt + levels, s.nn_idx, s.nn_d2);
  check_launch("k_icp_brute");
  return true;
}

bool is_identity(const float* m) {
  for (int i = 0; i < 16; ++i)
    if (m[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
  return true;
}

}  // namespace

void icp_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, const float* tx,
             const float* ty, const float* tz, int64_t nt, const pfx_icp_params& prm, const float* guess,
             IcpResult& out, float* ax, float* ay, float* az) {
  PFX_CHECK(ns >= 0 && nt >= 0 && ns < (int64_t(1) << 31) && nt < (int64_t(1) << 31), "icp: point count out of range");
  PFX_CHECK(prm.max_correspondence_distance > 0.0 && prm.max_iterations >= 0 &&
                !std::isnan(prm.transformation_epsilon) && !std::isnan(prm.euclidean_fitness_epsilon),
            "icp: invalid parameters");
  hipStream_t st = ctx->stream;
  float final_T[16];
  for (int i = 0; i < 16; ++i) final_T[i] = guess ? guess[i] : ((i % 5 == 0) ? 1.0f : 0.0f);
  out.fitness = DBL_MAX;
  out.converged = 0;
  out.iterations = 0;
  out.state = PFX_ICP_NO_CORRESPONDENCES;
  std::memcpy(out.T, final_T, sizeof(final_T));
  int64_t& st_iter = ctx->stats["icp_iterations"];
  int64_t& st_state = ctx->stats["icp_state"];
  int64_t& st_corr = ctx->stats["icp_correspondences"];
  int64_t& st_rounds = ctx->stats["icp_nn_rounds"];
  int64_t& st_brute = ctx->stats["icp_brute"];
  int64_t& st_exact = ctx->stats["icp_exact_sum"];
  st_iter = 0;
  st_state = out.state;
  st_corr = st_rounds = st_brute = 0;
  st_exact = 1;
  if (ns == 0) return;
  TimeScope total(ctx, "icp", true);
  if (!ctx->icp) ctx->icp = new IcpState();
  IcpState& S = *ctx->icp;
  const double maxd = prm.max_correspondence_distance;
  const double maxd2 = maxd * maxd;

  // the grids: a first cell that puts a few tens of points into a block on a scanned surface
  // (half the mean spacing of the bounding volume, as the cloud resolution does), raised so that
  // the last grid reaches the distance cap where that costs at most a factor of 4
  double lo[3], hi[3];
  points_bbox(ctx, S.lv[0], tx, ty, tz, nt, lo, hi);
  double ext = 0.0, vol = 1.0;
  for (int d = 0; d < 3; ++d) ext = std::max(ext, hi[d] - lo[d]);
  for (int d = 0; d < 3; ++d) vol *= std::max(hi[d] - lo[d], ext * 1e-3);
  double h0 = (ext > 0.0 && nt > 0) ? 0.5 * std::cbrt(vol / (double)nt) : 1.0;
  const double reach = maxd * (1.0 + 1e-4) / (double)(1 << (kIcpLevels - 1));  // (inf / 8 = inf: no raise)
  if (reach > h0 && reach <= 4.0 * h0) h0 = reach;
  Search s;
  s.S = &S;
  int loop_levels = kIcpLevels;
  // cells h0, 2 h0, ...; the first one to reach the cap is cut down to it (the block that proves
  // "nothing within the cap" should be no larger than it must), and the doubling goes on from there
  const double cap_cell = maxd * (1.0 + 1e-4);
  bool cut = false;
  double hk = h0;
  for (int k = 0; k < kIcpLevels; ++k, hk *= 2.0) {
    if (!cut && hk >= cap_cell) {
      hk = cap_cell;
      cut = true;
    }
    build_grid(ctx, S.lv[k], tx, ty, tz, nt, hk);
    const double h = 1.0 / S.lv[k].dinv;  // the cell actually used
    s.hh[k] = (float)(h * h * (1.0 - 1e-5));
    if (loop_levels == kIcpLevels && (double)s.hh[k] >= maxd2) loop_levels = k + 1;
  }
  const int64_t ld = (ns + 3) & ~int64_t(3);
  const int64_t nblk = ceil_div(ns, 256), ndepth = ceil_div(ns, kIcpGemmDepth);
  float* w = ctx->buf("icp_work").as<float>(3 * ld);
  float *wx = w, *wy = w + ld, *wz = w + 2 * ld;
  float* L = ctx->buf("icp_list").as<float>(7 * ld);
  s.nn_idx = ctx->buf("icp_nn_idx").as<int32_t>(ns);
  s.nn_d2 = ctx->buf("icp_nn_d2").as<float>(ns);
  s.qa = ctx->buf("icp_qa").as<int32_t>(ns);
  s.qb = ctx->buf("icp_qb").as<int32_t>(ns);
  int* blk = ctx->buf("icp_blk").as<int>(nblk);
  float* mean = ctx->buf("icp_mean").as<float>(8);
  float* P = ctx->buf("icp_P").as<float>(9 * ndepth);
  ResPart* part = ctx->buf("icp_part").as<ResPart>(exact_sum_blocks(ns));
  double* seq = ctx->buf("icp_seq").as<double>(1);
  s.rb = ctx->buf("icp_rb").as<IcpReadback>(1);
  IcpReadback* h_rb = ctx->readback<IcpReadback>();  // pinned

  auto transform = [&](const float* ix, const float* iy, const float* iz, const float* T, float* ox, float* oy,
                       float* oz) {
    Mat4 M;
    std::memcpy(M.m, T, sizeof(M.m));
    k_icp_transform<<<(unsigned)nblk, 256, 0, st>>>(ix, iy, iz, ns, M, ox, oy, oz);
    check_launch("k_icp_transform");
  };
  auto note_search = [&](bool brute, int levels) {  // after a readback
    int rounds = 1;
    for (int k = 1; k < levels; ++k)
      if (h_rb->cnt[k] > 0) rounds = k + 1;
    st_rounds = std::max<int64_t>(st_rounds, rounds);
    if (brute) st_brute += h_rb->cnt[levels];
  };

  if (is_identity(final_T)) {
    PFX_HIP(hipMemcpyAsync(wx, sx, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    PFX_HIP(hipMemcpyAsync(wy, sy, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    PFX_HIP(hipMemcpyAsync(wz, sz, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
  } else {
    transform(sx, sy, sz, final_T, wx, wy, wz);
  }

  double prev_mse = DBL_MAX;
  int iterations = 0, state = PFX_ICP_NOT_CONVERGED;
  bool converged = false;
  for (;;) {
    bool brute;
    {
      TimeScope ts(ctx, "icp_nn");
      brute = nn_search(ctx, s, wx, wy, wz, ns, maxd2, loop_levels);
    }
    {
      TimeScope ts(ctx, "icp_compact");
      k_icp_count<<<(unsigned)nblk, 256, 0, st>>>(s.nn_idx, s.nn_d2, ns, maxd2, blk);
      k_icp_scan<<<1, 256, 0, st>>>(blk, nblk, s.rb->cnt);
      k_icp_scatter<<<(unsigned)nblk, 256, 0, st>>>(s.nn_idx, s.nn_d2, ns, maxd2, blk, s.rb->cnt, wx, wy, wz, tx, ty, tz,
                                                    L, ld);
      check_launch("k_icp_scatter");
    }
    {
      TimeScope ts(ctx, "icp_means");
      k_icp_means<<<1, 256, 0, st>>>(L, ld, s.rb->cnt, mean);
      check_launch("k_icp_means");
    }
    {
      TimeScope ts(ctx, "icp_sigma");
      k_icp_sigma<<<(unsigned)ndepth, 256, 0, st>>>(L, ld, s.rb->cnt, mean, P);
      k_icp_combine<<<1, 64, 0, st>>>(P, mean, s.rb);
      check_launch("k_icp_sigma");
    }
    {
      TimeScope ts(ctx, "icp_mse");
      exact_sum_launch(ctx, L + 6 * ld, ns, part, &s.rb->acc);
    }
    PFX_HIP(hipMemcpyAsync(h_rb, s.rb, sizeof(IcpReadback), hipMemcpyDeviceToHost, st));
    ctx->sync_spin(st);
    note_search(brute, loop_levels);
    const int n = h_rb->cnt[0];
    st_corr = n;
    if (n < 3) {
      state = PFX_ICP_NO_CORRESPONDENCES;
      converged = false;
      break;
    }
    // Umeyama's 3x3 part on the host: R = U S V^T of the float sigma, in double
    double sigma[9], R[9];
    for (int i = 0; i < 9; ++i) sigma[i] = (double)h_rb->sigma[i];
    umeyama_rotation3(sigma, R);
    float T[16];
    const float* ms = h_rb->mean;
    const float* mt = h_rb->mean + 3;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
      T[4 * i + 3] = mt[i] - ((T[4 * i] * ms[0] + T[4 * i + 1] * ms[1]) + T[4 * i + 2] * ms[2]);
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
    const ResAcc acc = h_rb->acc;  // (the pinned block is reused by the next readback)
    transform(wx, wy, wz, T, wx, wy, wz);
    float nf[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c)
        nf[4 * r + c] = ((T[4 * r] * final_T[c] + T[4 * r + 1] * final_T[4 + c]) + T[4 * r + 2] * final_T[8 + c]) +
                        T[4 * r + 3] * final_T[12 + c];
    std::memcpy(final_T, nf, sizeof(nf));
    ++iterations;
    if (iterations >= prm.max_iterations) {
      state = PFX_ICP_ITERATIONS;
      converged = true;
      break;
    }
    const double cos_angle = 0.5 * (double)(((T[0] + T[5]) + T[10]) - 1.0f);
    const double tr2 = (double)((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]);
    if (cos_angle >= 0.99999 && tr2 <= prm.transformation_epsilon) {
      state = PFX_ICP_TRANSFORM;
      converged = true;
      break;
    }
    if (!acc.exact) st_exact = 0;
    double mse;
    {
      // (not exact: the sequential loop over the n list positions, which hold the terms in order)
      TimeScope ts(ctx, "icp_mse");
      mse = exact_sum_finish(ctx, acc, L + 6 * ld, n, seq) / (double)n;
    }
    if (std::fabs(mse - prev_mse) < 1e-12) {
      state = PFX_ICP_ABS_MSE;
      converged = true;
      break;
    }
    if (std::fabs(mse - prev_mse) / prev_mse < prm.euclidean_fitness_epsilon) {
      state = PFX_ICP_REL_MSE;
      converged = true;
      break;
    }
    prev_mse = mse;
  }
  if (ax && ay && az) {
    PFX_HIP(hipMemcpyAsync(ax, wx, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    PFX_HIP(hipMemcpyAsync(ay, wy, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
    PFX_HIP(hipMemcpyAsync(az, wz, sizeof(float) * ns, hipMemcpyDeviceToDevice, st));
  }

  // getFitnessScore(): the original source under `final`, nearest target without a cap
  {
    TimeScope ts(ctx, "icp_fitness");
    float* f = L;  // the list is free now: rows 0..2 the transformed cloud, row 6 the terms
    transform(sx, sy, sz, final_T, f, f + ld, f + 2 * ld);
    const bool brute = nn_search(ctx, s, f, f + ld, f + 2 * ld, ns, INFINITY, kIcpLevels);
    k_icp_terms<<<(unsigned)nblk, 256, 0, st>>>(s.nn_idx, s.nn_d2, ns, L + 6 * ld);
    check_launch("k_icp_terms");
    exact_sum_launch(ctx, L + 6 * ld, ns, part, &s.rb->acc);
    PFX_HIP(hipMemcpyAsync(h_rb, s.rb, sizeof(IcpReadback), hipMemcpyDeviceToHost, st));
    ctx->sync_spin(st);
    note_search(brute, kIcpLevels);
    const ResAcc acc = h_rb->acc;
    if (acc.count) {
      if (!acc.exact) st_exact = 0;
      out.fitness = exact_sum_finish(ctx, acc, L + 6 * ld, ns, seq) / (double)(int64_t)acc.count;
    }
  }
  std::memcpy(out.T, final_T, sizeof(final_T));
  out.converged = converged ? 1 : 0;
  out.iterations = iterations;
  out.state = state;
  st_iter = iterations;
  st_state = state;
}

}  // namespace pfx
