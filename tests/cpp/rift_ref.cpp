// rift_ref.cpp -- TEST INFRASTRUCTURE ONLY: CPU restatements of the two contracts of pfx_rift.hip as
// DESIGN.md states them ("Intensity gradient and RIFT", "RIFT: the contract"):
//   igrad_ref  PCL 1.7 IntensityGradientEstimation with the float accessor I(p) = si[p],
//              demean = I - mean (the rule of oracle/or_keypoints.cpp:482-490 without the colour
//              write-back and without Harris6D's normalisation);
//   rift_ref   PCL 1.7 RIFTEstimation (features/impl/rift.hpp).
// Built by tests/rift_ref.py into a shared object; never linked into libpfx.  Plain sequential
// float arithmetic in FLANN neighbour order on the oracle's NeighborGrid (oracle/or_common.h) and
// its ColPivHouseholderQR restatement (orc_colpiv_solve3f of oracle/or_keypoints.cpp, compiled in).  The squared norm of the RIFT matrix is Eigen 3.2's float sum (pfx_eigen_redux.h,
// shared with the kernel and pinned on its own by tests/test_rift_ref.py).  Every NaN is written as
// 0x7fc00000, as the kernels do.
#include <cfloat>
#include <cstring>

#include <algorithm>
#include <cmath>

#include "../../pcl_feature_extraction_amd/csrc/pfx_eigen_redux.h"
#include "or_common.h"

using namespace orc;

// oracle/or_keypoints.cpp (compiled into this object by tests/rift_ref.py): n systems, a column-major
extern "C" int orc_colpiv_solve3f(const float* a, const float* b, i64 n, float* x);

namespace {

inline void colpiv_solve3(const float a[9], const float rhs[3], float x[3]) { orc_colpiv_solve3f(a, rhs, 1, x); }

inline float canon_nan(float v) {
  if (v == v) return v;
  const uint32_t u = 0x7fc00000u;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

}  // namespace

extern "C" {

// Eigen 3.2's sum() of n floats
float rift_eigen_sum_f(const float* m, int n) { return pfx::eigen_redux_sum_f(m, n); }

// out: nq x 3.  reversed != 0 walks every neighbourhood from its last neighbour to its first.
// stats (nullable, 2): sum of k, max k.
void igrad_ref(const float* sx, const float* sy, const float* sz, const float* si, i64 ns, const float* qx,
               const float* qy, const float* qz, const float* qnx, const float* qny, const float* qnz, i64 nq,
               double r, int reversed, float* out, i64* stats) {
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
    if (reversed) std::reverse(idx.begin(), idx.end());
    if (k < 3) {
      o[0] = o[1] = o[2] = canon_nan(NAN);
      continue;
    }
    float cx = 0.f, cy = 0.f, cz = 0.f, mean = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      cx += sx[p];
      cy += sy[p];
      cz += sz[p];
      mean += si[p];
    }
    const float rk = 1.0f / (float)k;  // centroid /= float(k): Eigen 3.2 multiplies by the reciprocal
    cx *= rk;
    cy *= rk;
    cz *= rk;
    mean /= (float)k;
    float A00 = 0.f, A01 = 0.f, A02 = 0.f, A11 = 0.f, A12 = 0.f, A22 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      if (!std::isfinite(si[p])) continue;  // the raw intensity
      const float px = sx[p] - cx, py = sy[p] - cy, pz = sz[p] - cz;
      const float iv = si[p] - mean;
      A00 += px * px;
      A01 += px * py;
      A02 += px * pz;
      A11 += py * py;
      A12 += py * pz;
      A22 += pz * pz;
      b0 += px * iv;
      b1 += py * iv;
      b2 += pz * iv;
    }
    const float A[9] = {A00, A01, A02, A01, A11, A12, A02, A12, A22};
    const float bv[3] = {b0, b1, b2};
    float xs[3];
    colpiv_solve3(A, bv, xs);
    const float nv[3] = {qnx[q], qny[q], qnz[q]};
    for (int row = 0; row < 3; ++row) {  // (Identity - n n^T) x
      const float m0 = (row == 0 ? 1.0f : 0.0f) - nv[row] * nv[0];
      const float m1 = (row == 1 ? 1.0f : 0.0f) - nv[row] * nv[1];
      const float m2 = (row == 2 ? 1.0f : 0.0f) - nv[row] * nv[2];
      o[row] = canon_nan((m0 * xs[0] + m1 * xs[1]) + m2 * xs[2]);
    }
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
  }
}

// out: nq x D G, out[gi * D + di].  stats (nullable, 2): sum of k, max k.
void rift_ref(const float* sx, const float* sy, const float* sz, const float* sgx, const float* sgy,
              const float* sgz, i64 ns, const float* cx, const float* cy, const float* cz, i64 nq, double r, int D,
              int G, int reversed, float* out, i64* stats) {
  const int S = D * G;
  const float eps = FLT_EPSILON, rad = (float)r;
  NeighborGrid g;
  g.build(sx, sy, sz, ns, r);
  std::vector<int> idx;
  std::vector<float> d2;
  std::vector<float> m((size_t)S), sq((size_t)S);  // column-major: m[di + D * gi]
  i64 nb = 0, kmax = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* o = out + q * S;
    g.radius(cx[q], cy[q], cz[q], r, idx, d2);
    const int k = (int)idx.size();
    nb += k;
    kmax = std::max<i64>(kmax, k);
    if (k == 0) {  // (PCL leaves the previous query's matrix: a deliberate deviation)
      for (int i = 0; i < S; ++i) o[i] = canon_nan(NAN);
      continue;
    }
    if (reversed) {
      std::reverse(idx.begin(), idx.end());
      std::reverse(d2.begin(), d2.end());
    }
    std::fill(m.begin(), m.end(), 0.0f);
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      const float g0 = sgx[p], g1 = sgy[p], g2 = sgz[p];
      const float mag = sqrtf((g0 * g0 + g1 * g1) + g2 * g2);
      const float vx = sx[p] - cx[q], vy = sy[p] - cy[q], vz = sz[p] - cz[q];
      const float vn = sqrtf((vx * vx + vy * vy) + vz * vz);
      const float u0 = vx / vn, u1 = vy / vn, u2 = vz / vn;  // normalized(): a true division, no zero test
      float ang = acosf(((g0 * u0 + g1 * u1) + g2 * u2) / mag);
      if (!std::isfinite(ang)) ang = 0.f;
      const float d = (float)D * sqrtf(d2[(size_t)i]) / (rad + eps);
      const float gg = (float)G * ang / ((float)M_PI + eps);
      const int d_lo = std::max((int)ceilf(d - 1), 0), d_hi = std::min((int)floorf(d + 1), D - 1);
      const int g_lo = (int)ceilf(gg - 1), g_hi = (int)floorf(gg + 1);
      for (int gi = g_lo; gi <= g_hi; ++gi)
        for (int di = d_lo; di <= d_hi; ++di) {
          const float w = (1 - fabsf(d - di)) * (1 - fabsf(gg - gi));
          m[(size_t)(di + D * ((gi + G) % G))] += w * mag;
        }
    }
    for (int i = 0; i < S; ++i) sq[(size_t)i] = m[(size_t)i] * m[(size_t)i];
    const float inv = 1.0f / sqrtf(pfx::eigen_redux_sum_f(sq.data(), S));
    for (int i = 0; i < S; ++i) o[i] = canon_nan(m[(size_t)i] * inv);
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
  }
}

}  // extern "C"
