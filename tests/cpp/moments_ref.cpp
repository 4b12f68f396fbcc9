// moments_ref.cpp -- TEST INFRASTRUCTURE ONLY: CPU restatements of the two contracts of
// pfx_moments.hip as DESIGN.md states them ("Moments and curvatures: the contract"):
//   moments_ref  PCL 1.7 MomentInvariantsEstimation (features/impl/moment_invariants.hpp);
//   pcurv_ref    PCL 1.7 PrincipalCurvaturesEstimation (features/impl/principal_curvatures.hpp) with
//                pcl::eigen33 (values) and pcl::computeCorrespondingEigenVector (common/impl/eigen.hpp).
// Built by tests/moments_ref.py into a shared object; never linked into libpfx.  Plain sequential
// float arithmetic in FLANN neighbour order on the oracle's NeighborGrid, with the oracle's
// scaleMatrix, computeRoots and nullVector (oracle/or_common.h), the project's standing statement
// of eigen33.  Every NaN is written as 0x7fc00000, as the kernels do.
#include <cstring>

#include <algorithm>
#include <cmath>

#include "or_common.h"

using namespace orc;

namespace {

inline float canon_nan(float v) {
  if (v == v) return v;
  const uint32_t u = 0x7fc00000u;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

}  // namespace

extern "C" {

// out: nq x 3 (j1 j2 j3).  reversed != 0 walks every neighbourhood from its last neighbour to its
// first.  stats (nullable, 2): sum of k, max k.  counts (nullable, nq): k of every row.
void moments_ref(const float* sx, const float* sy, const float* sz, i64 ns, const float* qx, const float* qy,
                 const float* qz, i64 nq, double r, int reversed, float* out, i64* stats, i64* counts) {
  NeighborGrid g;
  g.build(sx, sy, sz, ns, r);
  std::vector<int> idx;
  std::vector<float> d2;
  i64 nb = 0, kmax = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* o = out + 3 * q;
    g.radius(qx[q], qy[q], qz[q], r, idx, d2);  // (d2, index) ascending; empty for a non-finite query
    const int k = (int)idx.size();
    nb += k;
    kmax = std::max<i64>(kmax, k);
    if (counts) counts[q] = k;
    if (reversed) std::reverse(idx.begin(), idx.end());
    if (k == 0) {
      o[0] = o[1] = o[2] = canon_nan(NAN);
      continue;
    }
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      cx += sx[p];
      cy += sy[p];
      cz += sz[p];
    }
    const float rk = 1.0f / (float)k;  // centroid /= float(k): Eigen 3.2 multiplies by the reciprocal
    cx *= rk;
    cy *= rk;
    cz *= rk;
    float mu200 = 0.f, mu020 = 0.f, mu002 = 0.f, mu110 = 0.f, mu101 = 0.f, mu011 = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      const float t0 = sx[p] - cx, t1 = sy[p] - cy, t2 = sz[p] - cz;
      mu200 += t0 * t0;
      mu020 += t1 * t1;
      mu002 += t2 * t2;
      mu110 += t0 * t1;
      mu101 += t0 * t2;
      mu011 += t1 * t2;
    }
    o[0] = canon_nan(mu200 + mu020 + mu002);
    o[1] = canon_nan(mu200 * mu020 + mu200 * mu002 + mu020 * mu002 - mu110 * mu110 - mu101 * mu101 - mu011 * mu011);
    o[2] = canon_nan(mu200 * mu020 * mu002 + 2 * mu110 * mu101 * mu011 - mu002 * mu110 * mu110 -
                     mu020 * mu101 * mu101 - mu200 * mu011 * mu011);
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
  }
}

// out: nq x 5 (pcx pcy pcz pc1 pc2).  stats (nullable, 3): sum of k, max k, rows where
// (root2 * scale) / scale differs from root2 in bits.
void pcurv_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
               const float* snz, i64 ns, const float* qx, const float* qy, const float* qz, const float* qnx,
               const float* qny, const float* qnz, i64 nq, double r, int reversed, float* out, i64* stats,
               i64* counts) {
  NeighborGrid g;
  g.build(sx, sy, sz, ns, r);
  std::vector<int> idx;
  std::vector<float> d2;
  std::vector<float> P;
  i64 nb = 0, kmax = 0, detours = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* o = out + 5 * q;
    g.radius(qx[q], qy[q], qz[q], r, idx, d2);
    const int k = (int)idx.size();
    nb += k;
    kmax = std::max<i64>(kmax, k);
    if (counts) counts[q] = k;
    if (reversed) std::reverse(idx.begin(), idx.end());
    if (k == 0) {
      for (int e = 0; e < 5; ++e) o[e] = canon_nan(NAN);
      continue;
    }
    const float nv[3] = {qnx[q], qny[q], qnz[q]};
    float M[3][3];  // Identity - n n^T
    for (int row = 0; row < 3; ++row)
      for (int c = 0; c < 3; ++c) M[row][c] = (row == c ? 1.0f : 0.0f) - nv[row] * nv[c];
    P.resize(3 * (size_t)k);
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      const float m0 = snx[p], m1 = sny[p], m2 = snz[p];
      float* pr = &P[3 * (size_t)i];
      for (int row = 0; row < 3; ++row) pr[row] = (M[row][0] * m0 + M[row][1] * m1) + M[row][2] * m2;
      c0 += pr[0];
      c1 += pr[1];
      c2 += pr[2];
    }
    const float rk = 1.0f / (float)k;  // centroid /= float(k): the reciprocal
    c0 *= rk;
    c1 *= rk;
    c2 *= rk;
    float s00 = 0.f, s01 = 0.f, s02 = 0.f, s11 = 0.f, s12 = 0.f, s22 = 0.f;
    for (int i = 0; i < k; ++i) {
      const float* pr = &P[3 * (size_t)i];
      const float d0 = pr[0] - c0, d1 = pr[1] - c1, d2v = pr[2] - c2;
      s00 += d0 * d0;
      s01 += d0 * d1;
      s02 += d0 * d2v;
      s11 += d1 * d1;
      s12 += d1 * d2v;
      s22 += d2v * d2v;
    }
    const float cov[3][3] = {{s00, s01, s02}, {s01, s11, s12}, {s02, s12, s22}};
    // pcl::eigen33(cov, evals)
    float sm[3][3], scale, roots[3];
    scaleMatrix(cov, sm, scale);
    computeRoots(sm, roots);
    const float e1 = roots[1] * scale, e2 = roots[2] * scale;
    // pcl::computeCorrespondingEigenVector(cov, evals[2], v): the same scaling, then evals[2] / scale
    const float lambda = e2 / scale;
    if (f2w(lambda) != f2w(roots[2])) ++detours;
    const V3 v = nullVector(sm, lambda);
    o[0] = canon_nan(v.x);
    o[1] = canon_nan(v.y);
    o[2] = canon_nan(v.z);
    o[3] = canon_nan(e2 * rk);
    o[4] = canon_nan(e1 * rk);
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
    stats[2] = detours;
  }
}

}  // extern "C"
