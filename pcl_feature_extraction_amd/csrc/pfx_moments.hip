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
// Both run the two passes of pfx_two_pass.h and report late errors and statistics through the
// deferred reports (moments_report, pcurv_report; no words of their own).
// A NaN is written as 0x7fc00000, here and in the restatement.
#include "pfx_two_pass.h"

namespace pfx {
namespace {

constexpr int kMomChunk = kTwoPassChunk;

// The 16 KiB behind the keys: the bucketed sort's scratch, then (the sort done) the records.
struct MomAux {
  float4 rec[kMomChunk];  // x, y, z of the chunk's neighbours, or their projected normals (w unused)
  float acc[12];          // the centroid, then the six sums
};
static_assert(sizeof(MomAux) <= kTwoPassAuxBytes, "the records fit the sort scratch");

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
    const int k = two_pass_neighbors<CAP>(g, qx[q], qy[q], qz[q], rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) count_neighbors(k, err);
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

template <bool PCURV>
void launch(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
            const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, const float* qnx,
            const float* qny, const float* qnz, int64_t nq, double r, float* out) {
  if (nq == 0) return;
  constexpr int W = PCURV ? 5 : 3;
  constexpr ReportSlot slot = PCURV ? kRepPcurv : kRepMoments;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, slot);
  if (ns == 0) {  // every k is 0
    fill_nan(ctx, out, W * nq);
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    const float rr = (float)(r * r);
    TimeScope ts(ctx, PCURV ? "principal_curvatures" : "moment_invariants", true);
    two_pass(ctx, ns, nq, PCURV ? "pcurv_over" : "moments_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_moments<cap(), PCURV>, blocks, lds, st, g, snx, sny, snz, qx, qy, qz, qnx, qny, qnz,
                               nq, rr, list, n_list, over, out, err);
             });
    check_launch("k_moments");
  }
  report_post(ctx, slot, err);
}

}  // namespace

int moments_cap_small() { return kTwoPassCapSmall; }

void moments_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, const float* qx,
                 const float* qy, const float* qz, int64_t nq, double r, float* out) {
  launch<false>(ctx, sx, sy, sz, nullptr, nullptr, nullptr, ns, qx, qy, qz, nullptr, nullptr, nullptr, nq, r, out);
}

void pcurv_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
               const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, const float* qnx,
               const float* qny, const float* qnz, int64_t nq, double r, float* out) {
  launch<true>(ctx, sx, sy, sz, snx, sny, snz, ns, qx, qy, qz, qnx, qny, qnz, nq, r, out);
}

void moments_report(pfx_ctx* ctx, const int* h) { two_pass_report(ctx, h, "moments", "moment_invariants"); }
void pcurv_report(pfx_ctx* ctx, const int* h) { two_pass_report(ctx, h, "pcurv", "principal_curvatures"); }

}  // namespace pfx
