// pfx_rift.hip -- IntensityGradientEstimation<PointXYZI, Normal, IntensityGradient,
// IntensityFieldAccessor<PointXYZI>> (evaluation.cpp:416-465, tools.h:40-54) and
// RIFTEstimation<PointXYZI, IntensityGradient, Histogram<32>> (evaluation.cpp:716-765) on gfx950.
// DESIGN.md "Intensity gradient and RIFT" and "RIFT: the contract".
//
// Intensity gradient, two shapes of one arithmetic (the same bits for the same query):
//   k_igrad_lists  the whole cloud: the normal estimation's FLANN-ordered lists, lane per list,
//                  igrad_lane (pfx_igrad.h) with the float accessor I(p) = si[p], demean = I - mean;
//   k_igrad_query  arbitrary queries: one 256-thread workgroup per query, the keys sorted in LDS
//                  (pfx_neighbors.h), the neighbours' (x, y, z, I) staged in LDS a chunk at a time,
//                  and one lane per accumulator: four sequential chains in the first pass (centroid,
//                  mean), nine in the second (the six upper sums of A, the three of b).
// RIFT (k_rift): one workgroup per query, the keys in LDS as in k_spin; per chunk of kRiftChunk
// neighbours every thread turns its neighbour into a record (d, mag, the gradient-bin weights, the
// distance bounds and the wrapped columns) and sets its bit in the chunk's row mask of each distance
// bin and column mask of each wrapped column it touches (64-bit integer atomics in LDS,
// order-free); then one lane per bin (D * G <= 256) takes the records of (row mask & column mask)
// in ascending order and adds them, its float accumulator in a register for the whole query.  No
// floating-point atomic.  (Every bin walking every record of the chunk instead took 1.9 times as
// long: DESIGN.md.)  The squared norm follows Eigen 3.2's float order (pfx_eigen_redux.h).
// Both run the two passes of pfx_two_pass.h and report late errors and statistics through the
// deferred reports (igrad_report, rift_report; no words of their own).  A NaN is written as
// 0x7fc00000, here and in the restatement.
#include <cfloat>
#include <cmath>
#include <cstring>

#include <string>

#include "pfx_eigen_redux.h"
#include "pfx_igrad.h"
#include "pfx_two_pass.h"

namespace pfx {
namespace {

constexpr int kRiftChunk = kTwoPassChunk;
constexpr int kRiftMaxBins = 16;     // per axis
constexpr int kNoCol = 31;           // a record's unused column slot (no bin has this column)

// the whole cloud: lane per list (LaneList; the rows of points off the lists were filled with NaN)
__global__ void __launch_bounds__(256) k_igrad_lists(GridView g, NbLists L, const float* __restrict__ si,
                                                     const float* __restrict__ nx, const float* __restrict__ ny,
                                                     const float* __restrict__ nz, float* __restrict__ out,
                                                     int* __restrict__ err) {
  __shared__ int32_t s_rt[kLaneListTable];
  __shared__ unsigned long long s_sum;
  __shared__ int s_max;
  const int tid = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + tid;
  const bool on = j < L.nq;  // (every thread reaches the barriers)
  if (tid == 0) {
    s_sum = 0ull;
    s_max = 0;
  }
  __syncthreads();
  int k = 0;
  if (on) {
    const LaneList ll(g, L, j, s_rt);
    k = ll.k;
    const int32_t i = g.perm[ll.p];
    float o[3];
    if (!igrad_lane(g, ll, FloatIntensity{si}, i, nx, ny, nz, o)) o[0] = o[1] = o[2] = __uint_as_float(0x7fc00000u);
    out[3 * (int64_t)i] = canon_nan(o[0]);
    out[3 * (int64_t)i + 1] = canon_nan(o[1]);
    out[3 * (int64_t)i + 2] = canon_nan(o[2]);
  }
  // statistics: the waves' sums meet in LDS, one pair of global atomics per block (same-address
  // atomics serialise at the L2)
  unsigned long long sum = (unsigned long long)k;
  int mx = k;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += (unsigned long long)__shfl_xor((long long)sum, o);
    mx = max(mx, __shfl_xor(mx, o));
  }
  if ((tid & 63) == 0) {
    atomicAdd(&s_sum, sum);
    atomicMax(&s_max, mx);
  }
  __syncthreads();
  if (tid == 0 && s_sum) {
    atomicAdd(reinterpret_cast<unsigned long long*>(err + kWordNeighbors), s_sum);
    atomicMax(err + kWordKmax, s_max);
  }
}

// The 16 KiB behind the keys: the bucketed sort's scratch, then (the sort done) the records.
struct IgradAux {
  float4 rec[kRiftChunk];  // x, y, z, I of the chunk's neighbours
  float acc[16];           // centroid and mean, then the nine sums
};

// list (nullable): the queued queries with their device-side count; over (nullable): where a query
// with more than CAP neighbours is queued (else it is beyond every capacity: err[0]).
template <int CAP>
__global__ void __launch_bounds__(kRiftChunk) k_igrad_query(GridView g, const float* __restrict__ si,
                                                            const float* __restrict__ qx, const float* __restrict__ qy,
                                                            const float* __restrict__ qz, const float* __restrict__ qnx,
                                                            const float* __restrict__ qny, const float* __restrict__ qnz,
                                                            int64_t nq, float rr, const int32_t* __restrict__ list,
                                                            const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                            float* __restrict__ out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of IgradAux
  IgradAux& A = *reinterpret_cast<IgradAux*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const float nan = __uint_as_float(0x7fc00000u);
  // accumulator `tid` of the second pass multiplies components ia and ib (3: the demeaned intensity)
  const int t9 = tid < 9 ? tid : 0;  // (the other lanes only stage records)
  const int ia = t9 < 3 ? 0 : t9 < 5 ? 1 : t9 == 5 ? 2 : t9 - 6;
  const int ib = t9 < 3 ? t9 : t9 < 5 ? t9 - 2 : t9 == 5 ? 2 : 3;
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    // (a non-finite query has no candidate run: k = 0)
    const int k = two_pass_neighbors<CAP>(g, qx[q], qy[q], qz[q], rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) count_neighbors(k, err);
    if (k < 3) {
      if (tid < 3) out[3 * q + tid] = nan;
      continue;
    }
    __syncthreads();  // the sort is done with its scratch
    float a = 0.f;
    for (int c0 = 0; c0 < k; c0 += kRiftChunk) {
      const int m = min(kRiftChunk, k - c0);
      if (tid < m) {
        const int32_t idx = key_idx(keys[c0 + tid]);
        A.rec[tid] = make_float4(g.ux[idx], g.uy[idx], g.uz[idx], si[idx]);
      }
      __syncthreads();
      if (tid < 4) {
        const float* rp = reinterpret_cast<const float*>(A.rec) + tid;
        for (int j = 0; j < m; ++j) a = a + rp[4 * j];
      }
      __syncthreads();
    }
    // centroid /= float(k): Eigen 3.2 multiplies by the reciprocal; the mean divides
    if (tid < 4) A.acc[tid] = tid < 3 ? a * (1.0f / (float)k) : a / (float)k;
    __syncthreads();
    const float ca = A.acc[ia], cb = A.acc[ib];
    a = 0.f;
    for (int c0 = 0; c0 < k; c0 += kRiftChunk) {
      const int m = min(kRiftChunk, k - c0);
      if (tid < m) {
        const int32_t idx = key_idx(keys[c0 + tid]);
        A.rec[tid] = make_float4(g.ux[idx], g.uy[idx], g.uz[idx], si[idx]);
      }
      __syncthreads();
      if (tid < 9) {
        const float* rp = reinterpret_cast<const float*>(A.rec);
        for (int j = 0; j < m; ++j) {
          if (!isfinite(rp[4 * j + 3])) continue;  // the raw intensity
          const float pa = rp[4 * j + ia] - ca, pb = rp[4 * j + ib] - cb;
          a = a + pa * pb;
        }
      }
      __syncthreads();
    }
    if (tid < 9) A.acc[4 + tid] = a;
    __syncthreads();
    if (tid == 0) {
      float s[9], o[3];
#pragma unroll
      for (int e = 0; e < 9; ++e) s[e] = A.acc[4 + e];
      const float nv[3] = {qnx[q], qny[q], qnz[q]};
      igrad_finish(s, nv, o);
      out[3 * q] = canon_nan(o[0]);
      out[3 * q + 1] = canon_nan(o[1]);
      out[3 * q + 2] = canon_nan(o[2]);
    }
    __syncthreads();  // A is read before the next query's sort scratch overwrites it
  }
}

struct RiftAux {
  float d[kRiftChunk], mag[kRiftChunk];
  float wg[3][kRiftChunk];  // 1 - |g - gi| of gi = g_lo, g_lo + 1, g_lo + 2 (g_lo .. g_hi are at most three)
  // d_lo | d_hi << 8 | the wrapped column (gi + G) % G of each gi << 16, 21, 26 (kNoCol: beyond g_hi)
  int bounds[kRiftChunk];
  float sq[kRiftMaxBins * kRiftMaxBins];
  float inv;
  unsigned long long mask[2][2 * kRiftMaxBins][kRiftChunk / 64];  // rows 0..15 distance bins, 16..31 columns
};
static_assert(sizeof(RiftAux) <= kTwoPassAuxBytes, "the records fit the sort scratch");
static_assert(sizeof(IgradAux) <= kTwoPassAuxBytes, "the records fit the sort scratch");

template <int CAP>
__global__ void __launch_bounds__(kRiftChunk) k_rift(GridView g, const float* __restrict__ sgx,
                                                     const float* __restrict__ sgy, const float* __restrict__ sgz,
                                                     const float* __restrict__ qx, const float* __restrict__ qy,
                                                     const float* __restrict__ qz, int64_t nq, float rr, float rad,
                                                     int D, int G, const int32_t* __restrict__ list,
                                                     const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                     float* __restrict__ out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of RiftAux
  RiftAux& A = *reinterpret_cast<RiftAux*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const int S = D * G;
  const int my_d = tid % D, my_g = tid / D;  // storage index d + D * g = the output index
  const float eps = FLT_EPSILON;
  const float dden = rad + eps, gden = (float)M_PI + eps;
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    const int k = two_pass_neighbors<CAP>(g, cx, cy, cz, rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) count_neighbors(k, err);
    if (k == 0) {  // (PCL leaves the previous query's matrix: a deliberate deviation)
      if (tid < S) out[q * S + tid] = __uint_as_float(0x7fc00000u);
      continue;
    }
    __syncthreads();  // the sort is done with its scratch
    float acc = 0.f;
    for (int i = tid; i < 2 * kRiftMaxBins * (kRiftChunk / 64); i += kRiftChunk) (&A.mask[0][0][0])[i] = 0ull;
    __syncthreads();
    int par = 0;
    for (int c0 = 0; c0 < k; c0 += kRiftChunk) {
      const int m = min(kRiftChunk, k - c0);
      for (int i = tid; i < 2 * kRiftMaxBins * (kRiftChunk / 64); i += kRiftChunk) (&A.mask[par ^ 1][0][0])[i] = 0ull;
      if (tid < m) {
        const uint64_t key = keys[c0 + tid];
        const int32_t idx = key_idx(key);
        const float g0 = sgx[idx], g1 = sgy[idx], g2 = sgz[idx];
        const float mag = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
        const float vx = g.ux[idx] - cx, vy = g.uy[idx] - cy, vz = g.uz[idx] - cz;
        const float vn = sqrtf((vx * vx + vy * vy) + vz * vz);
        const float u0 = vx / vn, u1 = vy / vn, u2 = vz / vn;  // normalized(): no zero test
        float ang = acosf_glibc(((g0 * u0 + g1 * u1) + g2 * u2) / mag);
        if (!isfinite(ang)) ang = 0.f;
        const float d = (float)D * sqrtf(key_d2(key)) / dden;
        const float gg = (float)G * ang / gden;
        const int d_lo = max((int)ceilf(d - 1.0f), 0), d_hi = min((int)floorf(d + 1.0f), D - 1);
        // (g_hi - g_lo <= 2: g - 1 in (g_lo - 1, g_lo] and fl(g + 1) >= g_lo + 3 cannot both hold)
        const int g_lo = (int)ceilf(gg - 1.0f), g_hi = (int)floorf(gg + 1.0f);
        A.d[tid] = d;
        A.mag[tid] = mag;
        // (the integer remainder by a run-time G costs tens of instructions: once per neighbour
        // here, not once per neighbour and bin below)
        int b = (d_lo & 255) | ((d_hi & 255) << 8);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int gi = g_lo + t;
          A.wg[t][tid] = 1.0f - fabsf(gg - (float)gi);
          b |= (gi <= g_hi ? (gi + G) % G : kNoCol) << (16 + 5 * t);
        }
        A.bounds[tid] = b;
        const unsigned long long bit = 1ull << (tid & 63);
        for (int di = d_lo; di <= d_hi; ++di) atomicOr(&A.mask[par][di][tid >> 6], bit);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int col = (b >> (16 + 5 * t)) & 31;
          if (col != kNoCol) atomicOr(&A.mask[par][kRiftMaxBins + col][tid >> 6], bit);
        }
      }
      __syncthreads();
      if (tid < S) {
        for (int wd64 = 0; wd64 * 64 < m; ++wd64) {
          unsigned long long hit = A.mask[par][my_d][wd64] & A.mask[par][kRiftMaxBins + my_g][wd64];
          while (hit) {  // ascending: a bin's additions stay in neighbour order
            const int j = wd64 * 64 + __builtin_ctzll(hit);
            hit &= hit - 1;
            const int b = A.bounds[j];
            const float wd = 1.0f - fabsf(A.d[j] - (float)my_d);
            const float mag = A.mag[j];
#pragma unroll
            for (int t = 0; t < 3; ++t)
              if (((b >> (16 + 5 * t)) & 31) == my_g) acc = acc + (wd * A.wg[t][j]) * mag;
          }
        }
      }
      par ^= 1;
      __syncthreads();  // the records are read before the next chunk's overwrite them
    }
    if (tid < S) A.sq[tid] = acc * acc;
    __syncthreads();
    if (tid == 0) A.inv = 1.0f / sqrtf(eigen_redux_sum_f(A.sq, S));
    __syncthreads();
    if (tid < S) out[q * S + tid] = canon_nan(acc * A.inv);
    __syncthreads();  // A is read before the next query's sort scratch overwrites it
  }
}

}  // namespace

int rift_cap_small() { return kTwoPassCapSmall; }

void igrad_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* si, int64_t ns,
               const float* qx, const float* qy, const float* qz, const float* qnx, const float* qny,
               const float* qnz, int64_t nq, int same, double r, float* out) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  if (same) {
    // the lists first: their build reads its counts back, and the words below are per call
    float* nx = ctx->buf("ig_nx").as<float>(ns);
    float* ny = ctx->buf("ig_ny").as<float>(ns);
    float* nz = ctx->buf("ig_nz").as<float>(ns);
    float* cv = ctx->buf("ig_cv").as<float>(ns);
    normals_lists_dev(ctx, sx, sy, sz, ns, r, nx, ny, nz, cv);
    const NbLists& L = ctx->normals->L;
    int* err = report_words(ctx, kRepIgrad);
    fill_nan(ctx, out, 3 * ns);  // points off the lists (non-finite) keep a NaN row
    PFX_CHECK(!L.compact, "intensity_gradient: the lane-per-list kernel reads 32-bit lists");
    if (L.nq > 0) {
      TimeScope ts(ctx, "intensity_gradient_cloud", true);
      k_igrad_lists<<<(unsigned)ceil_div(L.nq, 256), 256, 0, st>>>(view(ctx->grid_a), L, si, qnx, qny, qnz, out, err);
      check_launch("k_igrad_lists");
    }
    report_post(ctx, kRepIgrad, err);
    return;
  }
  int* err = report_words(ctx, kRepIgrad);
  if (ns == 0) {
    fill_nan(ctx, out, 3 * nq);
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    const float rr = (float)(r * r);
    TimeScope ts(ctx, "intensity_gradient", true);
    two_pass(ctx, ns, nq, "igrad_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_igrad_query<cap()>, blocks, lds, st, g, si, qx, qy, qz, qnx, qny, qnz, nq, rr, list,
                               n_list, over, out, err);
             });
    check_launch("k_igrad_query");
  }
  report_post(ctx, kRepIgrad, err);
}

void rift_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* sgx, const float* sgy,
              const float* sgz, int64_t ns, const float* cx, const float* cy, const float* cz, int64_t nq, double r,
              int D, int G, float* out) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, kRepRift);
  if (ns == 0) {
    fill_nan(ctx, out, nq * D * G);
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    const float rr = (float)(r * r), rad = (float)r;
    TimeScope ts(ctx, "rift", true);
    two_pass(ctx, ns, nq, "rift_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_rift<cap()>, blocks, lds, st, g, sgx, sgy, sgz, cx, cy, cz, nq, rr, rad, D, G, list,
                               n_list, over, out, err);
             });
    check_launch("k_rift");
  }
  report_post(ctx, kRepRift, err);
}

// (the stat "igrad_queued" has never been written)
void igrad_report(pfx_ctx* ctx, const int* h) { two_pass_report(ctx, h, "igrad", "intensity_gradient", false); }
void rift_report(pfx_ctx* ctx, const int* h) { two_pass_report(ctx, h, "rift", "rift"); }

}  // namespace pfx
