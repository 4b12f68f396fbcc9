// pfx_moments.hip -- MomentInvariantsEstimation<PointXYZRGB, MomentInvariants> (evaluation.cpp:554-572)
// and PrincipalCurvaturesEstimation<PointXYZRGB, Normal, PrincipalCurvatures> (evaluation.cpp:696-715)
// on gfx950.  DESIGN.md "Moment invariants and principal curvatures" and "Moments and curvatures: the
// contract".
//
// One kernel, k_moments<CAP, PCURV>, in the shape of k_igrad_query (pfx_rift.hip): one 256-thread
// workgroup per query, the keys sorted in LDS (pfx_neighbors.h), the neighbours' records staged in
// LDS a chunk of kMomChunk at a time, one lane per accumulator: three sequential float chains in
// the first pass (the centroid), six in the second (the products of the demeaned records).  The
// record is the neighbour's xyz (moment invariants) or its normal projected onto the tangent plane
// of the query normal (principal curvatures: every thread projects its own neighbour, only the
// chains are serial).  Thread 0 does the closed-form finish.  No floating-point atomic.
// Both follow spin's two-pass capacity scheme (kMomCapSmall keys, then the queued pass with kMomCap)
// and report late errors and statistics through pinned memory in stream order (moments_resolve).
// A NaN is written as 0x7fc00000, here and in the restatement.
#include <cstring>

#include <algorithm>
#include <string>

#include "pfx_device_math.h"
#include "pfx_internal.h"
#include "pfx_neighbors.h"

namespace pfx {
namespace {

constexpr int kMomCapSmall = 2048;  // keys of the first pass (bucketed sort: 2 x 16 KiB of LDS)
constexpr int kMomCap = 16384;      // keys of the second pass (128 KiB: one workgroup per CU)
constexpr int kMomChunk = 256;      // neighbours per chunk of records = the block size

// err words (ints) of either call.  Sticky until reported: [0] largest k beyond kMomCap.  Per
// call: [2] queued queries, [3] max k, [4..5] neighbours (u64).
constexpr int kErrWords = 8;
struct MomReadback {
  int mi[kErrWords];
  int pc[kErrWords];
};

__device__ __forceinline__ float canon_nan(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v; }

__global__ void k_moments_fill(float* __restrict__ p, int64_t n, float v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

// The 16 KiB behind the keys: the bucketed sort's scratch, then (the sort done) the records.
struct MomAux {
  float4 rec[kMomChunk];  // x, y, z of the chunk's neighbours, or their projected normals (w unused)
  float acc[12];          // the centroid, then the six sums
};
static_assert(sizeof(MomAux) <= sizeof(uint64_t) * kMomCapSmall, "the records fit the sort scratch");

// j1 j2 j3 of mu200 mu020 mu002 mu110 mu101 mu011, each expression as C++ parses it
__device__ __forceinline__ void moments_finish(const float s[6], float o[3]) {
  const float mu200 = s[0], mu020 = s[1], mu002 = s[2], mu110 = s[3], mu101 = s[4], mu011 = s[5];
  o[0] = canon_nan(mu200 + mu020 + mu002);
  o[1] = canon_nan(mu200 * mu020 + mu200 * mu002 + mu020 * mu002 - mu110 * mu110 - mu101 * mu101 - mu011 * mu011);
  o[2] = canon_nan(mu200 * mu020 * mu002 + 2.0f * mu110 * mu101 * mu011 - mu002 * mu110 * mu110 -
                   mu020 * mu101 * mu101 - mu200 * mu011 * mu011);
}

// pcl::eigen33(cov, evals), pcl::computeCorrespondingEigenVector(cov, evals[2], v), pc1, pc2 of
// the sums c00 c01 c02 c11 c12 c22
__device__ __forceinline__ void pcurv_finish(const float s[6], int k, float o[5]) {
  Sym3 cov, sm;
  cov.a00 = s[0]; cov.a01 = s[1]; cov.a02 = s[2];
  cov.a10 = s[1]; cov.a11 = s[3]; cov.a12 = s[4];
  cov.a20 = s[2]; cov.a21 = s[4]; cov.a22 = s[5];
  const float sc = scaleSym(cov, sm);
  float ev[3];
  computeRoots(sm.a00, sm.a01, sm.a02, sm.a11, sm.a12, sm.a22, ev);
  const float e1 = ev[1] * sc, e2 = ev[2] * sc;
  // the second scaling gives the same matrix; the diagonal loses (root2 * scale) / scale, which is
  // not always root2 in bits
  float picked;
  const f3 v = nullVector(sm, e2 / sc, &picked);
  const float rk = 1.0f / (float)k;
  o[0] = canon_nan(v.x);
  o[1] = canon_nan(v.y);
  o[2] = canon_nan(v.z);
  o[3] = canon_nan(e2 * rk);
  o[4] = canon_nan(e1 * rk);
}

// a query with more than CAP neighbours: queued for the second pass, or beyond every capacity
__device__ __forceinline__ void over_or_err(int k, int64_t q, int32_t* over, int* err) {
  if (over) over[atomicAdd(err + 2, 1)] = (int32_t)q;
  else { atomicMax(err, k); atomicMax(err + 3, k); }
}

// list (nullable): the queued queries with their device-side count; over (nullable): where a query
// with more than CAP neighbours is queued (else it is beyond every capacity: err[0]).
// PCURV: snx / sny / snz are the surface normals and qnx / qny / qnz the query normals (else unread).
template <int CAP, bool PCURV>
__global__ void __launch_bounds__(kMomChunk) k_moments(GridView g, const float* __restrict__ snx,
                                                       const float* __restrict__ sny, const float* __restrict__ snz,
                                                       const float* __restrict__ qx, const float* __restrict__ qy,
                                                       const float* __restrict__ qz, const float* __restrict__ qnx,
                                                       const float* __restrict__ qny, const float* __restrict__ qnz,
                                                       int64_t nq, float rr, const int32_t* __restrict__ list,
                                                       const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                       float* __restrict__ out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of MomAux
  MomAux& A = *reinterpret_cast<MomAux*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  constexpr int W = PCURV ? 5 : 3;  // floats of a row
  const int tid = threadIdx.x;
  const float nan = __uint_as_float(0x7fc00000u);
  // accumulator `tid` of the second pass multiplies components ia and ib: mu200 mu020 mu002 mu110
  // mu101 mu011, or the covariance's 00 01 02 11 12 22
  const int t6 = tid < 6 ? tid : 0;  // (the other lanes only stage records)
  const int ia = PCURV ? (t6 < 3 ? 0 : t6 < 5 ? 1 : 2) : (t6 < 3 ? t6 : t6 == 5 ? 1 : 0);
  const int ib = PCURV ? (t6 < 3 ? t6 : t6 < 5 ? t6 - 2 : 2) : (t6 < 3 ? t6 : t6 == 3 ? 1 : 2);
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    // (a non-finite query has no candidate run: k = 0)
    const int k = CAP == kMomCapSmall
                      ? sorted_neighbors_bucketed(g, qx[q], qy[q], qz[q], rr, keys, keys + CAP, CAP, &s_count, SB)
                      : sorted_neighbors(g, qx[q], qy[q], qz[q], rr, keys, CAP, &s_count);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) {
      atomicAdd(reinterpret_cast<unsigned long long*>(err + 4), (unsigned long long)k);
      atomicMax(err + 3, k);
    }
    if (k == 0) {
      if (tid < W) out[W * q + tid] = nan;
      continue;
    }
    // M = Identity - n n^T.  The empty asm pins each coefficient in a register: otherwise the
    // compiler folds (0 - p) * x into x * (-p), which is -0 where x86 code (IEEE: 0 - (+0) = +0)
    // gets +0
    float M[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (PCURV) {
      const float nv[3] = {qnx[q], qny[q], qnz[q]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        float m0 = (r == 0 ? 1.0f : 0.0f) - nv[r] * nv[0];
        float m1 = (r == 1 ? 1.0f : 0.0f) - nv[r] * nv[1];
        float m2 = (r == 2 ? 1.0f : 0.0f) - nv[r] * nv[2];
        asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2));
        M[3 * r] = m0;
        M[3 * r + 1] = m1;
        M[3 * r + 2] = m2;
      }
    }
    auto stage = [&](int c0, int m) {
      if (tid < m) {
        const int32_t idx = key_idx(keys[c0 + tid]);
        if (PCURV) {
          const float n0 = snx[idx], n1 = sny[idx], n2 = snz[idx];
          A.rec[tid] = make_float4((M[0] * n0 + M[1] * n1) + M[2] * n2, (M[3] * n0 + M[4] * n1) + M[5] * n2,
                                   (M[6] * n0 + M[7] * n1) + M[8] * n2, 0.f);
        } else {
          A.rec[tid] = make_float4(g.ux[idx], g.uy[idx], g.uz[idx], 0.f);
        }
      }
    };
    __syncthreads();  // the sort is done with its scratch
    float a = 0.f;
    for (int c0 = 0; c0 < k; c0 += kMomChunk) {
      const int m = min(kMomChunk, k - c0);
      stage(c0, m);
      __syncthreads();
      if (tid < 3) {
        const float* rp = reinterpret_cast<const float*>(A.rec) + tid;
        for (int j = 0; j < m; ++j) a = a + rp[4 * j];
      }
      __syncthreads();
    }
    // centroid /= float(k): Eigen 3.2 multiplies by the reciprocal
    if (tid < 3) A.acc[tid] = a * (1.0f / (float)k);
    __syncthreads();
    const float ca = A.acc[ia], cb = A.acc[ib];
    a = 0.f;
    for (int c0 = 0; c0 < k; c0 += kMomChunk) {
      const int m = min(kMomChunk, k - c0);
      stage(c0, m);
      __syncthreads();
      if (tid < 6) {
        const float* rp = reinterpret_cast<const float*>(A.rec);
        for (int j = 0; j < m; ++j) {
          const float pa = rp[4 * j + ia] - ca, pb = rp[4 * j + ib] - cb;
          a = a + pa * pb;
        }
      }
      __syncthreads();
    }
    if (tid < 6) A.acc[3 + tid] = a;
    __syncthreads();
    if (tid == 0) {
      float s[6], o[W];
#pragma unroll
      for (int e = 0; e < 6; ++e) s[e] = A.acc[3 + e];
      if (PCURV) pcurv_finish(s, k, o);
      else moments_finish(s, o);
#pragma unroll
      for (int e = 0; e < W; ++e) out[W * q + e] = o[e];
    }
    __syncthreads();  // A is read before the next query's sort scratch overwrites it
  }
}

int* err_words(pfx_ctx* ctx, const char* name) {
  DevBuf& eb = ctx->buf(name);
  const bool fresh = !eb.ptr;
  int* err = eb.as<int>(kErrWords);
  if (fresh) PFX_HIP(hipMemsetAsync(err, 0, 2 * sizeof(int), ctx->stream));               // the sticky words
  PFX_HIP(hipMemsetAsync(err + 2, 0, (kErrWords - 2) * sizeof(int), ctx->stream));  // the per-call words
  return err;
}

// the surface grid prepared ahead (pfx_fpfh_prepare_dev: coordinates only), else built here
GridView feature_grid(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, double r) {
  const bool grid_ready = ctx->prep_x == sx && ctx->prep_n == ns && ctx->prep_r == r;
  if (grid_ready) fpfh_validate_grid(ctx);  // (a speculative prepared grid: exact after this)
  ctx->prep_x = nullptr;  // one-shot
  ctx->prep_n = -1;
  ctx->prep_qx = nullptr;
  ctx->prep_nq = -1;
  if (!grid_ready) build_grid(ctx, ctx->grid_b, sx, sy, sz, ns, r);
  return view(ctx->grid_b);
}

constexpr size_t kAuxBytes = sizeof(uint64_t) * kMomCapSmall;
constexpr size_t kLdsSmall = sizeof(uint64_t) * kMomCapSmall + kAuxBytes;
constexpr size_t kLdsLarge = sizeof(uint64_t) * kMomCap + kAuxBytes;

template <bool PCURV>
void launch(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
            const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, const float* qnx,
            const float* qny, const float* qnz, int64_t nq, double r, float* out) {
  if (nq == 0) return;
  constexpr int W = PCURV ? 5 : 3;
  hipStream_t st = ctx->stream;
  int* err = err_words(ctx, PCURV ? "pcurv_err" : "moments_err");
  if (ns == 0) {  // every k is 0
    k_moments_fill<<<(unsigned)ceil_div(W * nq, 256), 256, 0, st>>>(out, W * nq, __builtin_nanf(""));
    check_launch("k_moments_fill");
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    // a neighbourhood can only outgrow the first pass when the surface has more points than that
    const bool second_pass = ns > kMomCapSmall;
    int32_t* over = second_pass ? ctx->buf(PCURV ? "pcurv_over" : "moments_over").as<int32_t>((size_t)nq) : nullptr;
    const float rr = (float)(r * r);
    TimeScope ts(ctx, PCURV ? "principal_curvatures" : "moment_invariants", true);
    k_moments<kMomCapSmall, PCURV><<<(unsigned)std::min<int64_t>(nq, 1 << 20), kMomChunk, kLdsSmall, st>>>(
        g, snx, sny, snz, qx, qy, qz, qnx, qny, qnz, nq, rr, nullptr, nullptr, over, out, err);
    if (second_pass) {
      PFX_HIP(hipFuncSetAttribute((const void*)k_moments<kMomCap, PCURV>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsLarge));
      // longer lists: the count stays on the device
      k_moments<kMomCap, PCURV><<<(unsigned)std::min<int64_t>(nq, 256), kMomChunk, kLdsLarge, st>>>(
          g, snx, sny, snz, qx, qy, qz, qnx, qny, qnz, nq, rr, over, err + 2, nullptr, out, err);
    }
    check_launch("k_moments");
  }
  if (!ctx->moments_rb_mem) PFX_HIP(hipHostMalloc(&ctx->moments_rb_mem, sizeof(MomReadback), hipHostMallocDefault));
  MomReadback* rb = static_cast<MomReadback*>(ctx->moments_rb_mem);
  PFX_HIP(hipMemcpyAsync(PCURV ? rb->pc : rb->mi, err, sizeof(int) * kErrWords, hipMemcpyDeviceToHost, st));
  (PCURV ? ctx->pcurv_pending : ctx->moments_pending) = true;
}

}  // namespace

int moments_cap_small() { return kMomCapSmall; }

void moments_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, const float* qx,
                 const float* qy, const float* qz, int64_t nq, double r, float* out) {
  launch<false>(ctx, sx, sy, sz, nullptr, nullptr, nullptr, ns, qx, qy, qz, nullptr, nullptr, nullptr, nq, r, out);
}

void pcurv_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
               const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, const float* qnx,
               const float* qny, const float* qnz, int64_t nq, double r, float* out) {
  launch<true>(ctx, sx, sy, sz, snx, sny, snz, ns, qx, qy, qz, qnx, qny, qnz, nq, r, out);
}

// After a synchronisation of ctx's stream: the last moments_dev's and pcurv_dev's statistics and
// their capacity errors, each reported once.
void moments_resolve(pfx_ctx* ctx) {
  for (int which = 0; which < 2; ++which) {
    bool& pending = which ? ctx->pcurv_pending : ctx->moments_pending;
    if (!pending) continue;
    pending = false;
    const MomReadback* rb = static_cast<const MomReadback*>(ctx->moments_rb_mem);
    const int* h = which ? rb->pc : rb->mi;
    unsigned long long nb;
    std::memcpy(&nb, h + 4, sizeof(nb));
    const std::string name = which ? "pcurv" : "moments";
    ctx->stats[name + "_neighbors"] = (int64_t)nb;
    ctx->stats[name + "_kmax"] = h[3];
    ctx->stats[name + "_queued"] = h[2];
    if (h[0] > 0) {
      const int cap = h[0];
      int* err = ctx->buf(which ? "pcurv_err" : "moments_err").as<int>(kErrWords);
      PFX_HIP(hipMemsetAsync(err, 0, 2 * sizeof(int), ctx->stream));  // reported once
      throw Error(PFX_ERR_CAPACITY, (which ? "principal_curvatures" : "moment_invariants") +
                                        std::string(": a query has ") + std::to_string(cap) + " neighbours (> " +
                                        std::to_string(kMomCap) + " supported)");
    }
  }
}

}  // namespace pfx
