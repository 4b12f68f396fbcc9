// pfh_ref.cpp -- TEST INFRASTRUCTURE ONLY: a CPU restatement of PCL 1.7 PFHEstimation
// (features/impl/pfh.hpp, use_cache_ = false) as DESIGN.md "PFH-125: the contract" states it,
// on the oracle's arithmetic helpers (oracle/or_common.h: NeighborGrid, dot4 / sqn4,
// atan2f_glibc).  Built by tests/pfh_ref.py into a shared object; never linked into libpfx.
// Plain sequential `+= hist_incr` in FLANN pair order, single-threaded like PCL's class.
#include <climits>

#include "or_common.h"

using namespace orc;

namespace {

// pcl::computePairFeatures (features/src/pfh.cpp) on Vector4f maps (w forced to 0); false for
// a degenerate pair (f4 == 0 or v_norm == 0)
bool pairFeatures(V3 p1, V3 n1, V3 p2, V3 n2, float& f1, float& f2, float& f3, float& f4) {
  V3 dp = sub(p2, p1);
  f4 = std::sqrt(sqn4(dp));
  if (f4 == 0.0f) { f1 = f2 = f3 = f4 = 0.0f; return false; }
  V3 n1c = n1, n2c = n2;
  float angle1 = dot4(n1c, dp) / f4;
  float angle2 = dot4(n2c, dp) / f4;
  // `acos (fabs (angle))` resolves to ::acos(double) in PCL 1.7's pfh.cpp
  if (std::acos(std::fabs((double)angle1)) > std::acos(std::fabs((double)angle2))) {
    n1c = n2; n2c = n1;
    dp = mul(dp, -1.0f);
    f3 = -angle2;
  } else {
    f3 = angle1;
  }
  V3 v = cross(dp, n1c);
  float v_norm = std::sqrt(sqn4(v));
  if (v_norm == 0.0f) { f1 = f2 = f3 = f4 = 0.0f; return false; }
  v = mul(v, 1.0f / v_norm);  // `v /= v_norm` (Eigen 3.2: times the reciprocal)
  V3 w = cross(n1c, v);
  f2 = dot4(v, n2c);
  f1 = atan2f_glibc(dot4(w, n2c), dot4(n1c, n2c));
  return true;
}

int clampBin(double v, int nbins) {
  // static_cast<int>(floor(v)); x86 cvttsd2si gives INT_MIN for NaN -> clamped to 0
  if (!(v == v)) return 0;
  double f = std::floor(v);
  int h = (f >= 2147483647.0 || f < -2147483648.0) ? INT_MIN : (int)f;
  if (h < 0) h = 0;
  if (h >= nbins) h = nbins - 1;
  return h;
}

}  // namespace

extern "C" {

// out: nq x 125; pairs_out (nullable): sum over the queries of k (k - 1) / 2
int pfh_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
            const float* snz, i64 ns, const float* qx, const float* qy, const float* qz, i64 nq, double r,
            float* out, i64* pairs_out) {
  const int nr_split = 5;
  const float d_pi = 1.0f / (2.0f * (float)M_PI);
  NeighborGrid g;
  g.build(sx, sy, sz, ns, r);
  std::vector<int> idx;
  std::vector<float> d2;
  i64 pairs = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* h = out + q * 125;
    g.radius(qx[q], qy[q], qz[q], r, idx, d2);  // (d2, index) ascending; empty for a non-finite query
    const size_t k = idx.size();
    if (k == 0) {
      for (int b = 0; b < 125; ++b) h[b] = kNaN;
      continue;
    }
    for (int b = 0; b < 125; ++b) h[b] = 0.0f;
    const float hist_incr = 100.0f / (float)(k * (k - 1) / 2);
    pairs += (i64)(k * (k - 1) / 2);
    for (size_t i_idx = 0; i_idx < k; ++i_idx) {
      for (size_t j_idx = 0; j_idx < i_idx; ++j_idx) {
        const int a = idx[i_idx], b = idx[j_idx];
        float f1, f2, f3, f4;
        if (!pairFeatures(v3(sx[a], sy[a], sz[a]), v3(snx[a], sny[a], snz[a]), v3(sx[b], sy[b], sz[b]),
                          v3(snx[b], sny[b], snz[b]), f1, f2, f3, f4))
          continue;
        const int b1 = clampBin(nr_split * ((f1 + M_PI) * d_pi), nr_split);
        const int b2 = clampBin(nr_split * ((f2 + 1.0) * 0.5), nr_split);
        const int b3 = clampBin(nr_split * ((f3 + 1.0) * 0.5), nr_split);
        h[b1 + nr_split * b2 + nr_split * nr_split * b3] += hist_incr;
      }
    }
  }
  if (pairs_out) *pairs_out = pairs;
  return 0;
}

}  // extern "C"
