// intensity_spin_ref.cpp -- TEST INFRASTRUCTURE ONLY: the CPU restatement of the contract of
// pfx_intensity_spin.hip as DESIGN.md states it ("Intensity spin: the contract"): PCL 1.7
// IntensitySpinEstimation::computeIntensitySpinImage (features/impl/intensity_spin.hpp) with the
// exponential of pcl_feature_extraction_amd/csrc/pfx_expf.h, which this file compiles as the kernel
// does.  Built by tests/intensity_spin_ref.py into a shared object; never linked into libpfx.  Plain
// sequential float arithmetic in FLANN neighbour order on the oracle's NeighborGrid
// (oracle/or_common.h).  Every NaN is written as 0x7fc00000, as the kernel does.
#include <cfloat>
#include <cstring>

#include <algorithm>
#include <cmath>

#include "../../pcl_feature_extraction_amd/csrc/pfx_expf.h"
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

float ispin_expf(float x) { return pfx::pfx_expf(x); }

// the host C library's expf, for the comparison of tests/test_pfx_expf.py
float ispin_libm_expf(float x) { return expf(x); }

// |pfx_expf - expf| in ulps over n arguments: hist[0..2] counts 0, 1 and more; mismatch counts the
// arguments at which exactly one is a NaN, or exactly one is zero or infinite.  Returns the first
// argument more than one ulp apart (or 0).
float ispin_expf_compare(const float* x, i64 n, i64* hist, i64* mismatch) {
  float worst = 0.0f;
  for (i64 i = 0; i < n; ++i) {
    const float a = pfx::pfx_expf(x[i]), b = expf(x[i]);
    if (a != a || b != b) {
      *mismatch += (a != a) != (b != b);
      hist[0] += 1;
      continue;
    }
    if ((a == 0.0f) != (b == 0.0f) || std::isinf(a) != std::isinf(b)) *mismatch += 1;
    int32_t ua, ub;  // non-negative floats: the bit patterns are ordered as the values
    std::memcpy(&ua, &a, sizeof(ua));
    std::memcpy(&ub, &b, sizeof(ub));
    const i64 diff = ua > ub ? (i64)ua - ub : (i64)ub - ua;
    hist[diff > 2 ? 2 : diff] += 1;
    if (diff > 1 && worst == 0.0f) worst = x[i];
  }
  return worst;
}

// out: nq x D I, out[dj * I + ii].  reversed != 0 walks every neighbourhood from its last neighbour to
// its first.  stats (nullable, 2): sum of k, max k.
void ispin_ref(const float* sx, const float* sy, const float* sz, const float* si, i64 ns, const float* cx,
               const float* cy, const float* cz, i64 nq, double r, int D, int I, float sigma, int reversed,
               float* out, i64* stats) {
  const int S = D * I;
  const float eps = FLT_EPSILON, rad = (float)r;
  NeighborGrid g;
  g.build(sx, sy, sz, ns, r);
  std::vector<int> idx;
  std::vector<float> d2;
  std::vector<float> bin((size_t)S);  // bin[dj * I + ii]
  i64 nb = 0, kmax = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* o = out + q * S;
    g.radius(cx[q], cy[q], cz[q], r, idx, d2);  // (d2, index) ascending; empty for a non-finite centre
    const int k = (int)idx.size();
    nb += k;
    kmax = std::max<i64>(kmax, k);
    if (k == 0) {
      for (int i = 0; i < S; ++i) o[i] = canon_nan(NAN);
      continue;
    }
    if (reversed) {
      std::reverse(idx.begin(), idx.end());
      std::reverse(d2.begin(), d2.end());
    }
    float mn = FLT_MAX, mx = -FLT_MAX;
    for (int n = 0; n < k; ++n) {
      const float v = si[idx[(size_t)n]];
      mn = v < mn ? v : mn;
      mx = mx < v ? v : mx;
    }
    const float dden = rad + eps, iden = (mx - mn) + eps;
    std::fill(bin.begin(), bin.end(), 0.0f);
    for (int n = 0; n < k; ++n) {
      const float d = ((float)D * sqrtf(d2[(size_t)n])) / dden;
      const float iv = ((float)I * (si[idx[(size_t)n]] - mn)) / iden;
      if (!std::isfinite(iv)) continue;  // contributes nothing
      if (sigma > 0.0f) {
        const float t = 3 * sigma;
        const float c = 1.0f / ((2.0f * sigma) * sigma);
        const int d_lo = std::max((int)floorf(d - t), 0), d_hi = std::min((int)ceilf(d + t), D - 1);
        const int i_lo = std::max((int)floorf(iv - t), 0), i_hi = std::min((int)ceilf(iv + t), I - 1);
        for (int ii = i_lo; ii <= i_hi; ++ii)
          for (int dj = d_lo; dj <= d_hi; ++dj) {
            const float a = d - (float)dj;
            const float b = iv - (float)ii;
            const float w = pfx::pfx_expf((-(a * a)) * c - (b * b) * c);
            bin[(size_t)(dj * I + ii)] += w;
          }
      } else {
        const int dj = (int)d, ii = (int)iv;
        if (dj >= D || ii >= I) continue;  // PCL writes out of bounds: dropped (a deliberate deviation)
        bin[(size_t)(dj * I + ii)] += 1.0f;
      }
    }
    for (int i = 0; i < S; ++i) o[i] = canon_nan(bin[(size_t)i]);
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
  }
}

}  // extern "C"
