// spin_ref.cpp -- TEST INFRASTRUCTURE ONLY: a CPU restatement of PCL 1.7 SpinImageEstimation
// (features/impl/spin_image.hpp, neither radial nor angular, the rotation axis = the input normal)
// as DESIGN.md "Spin images: the contract" states it, on the oracle's arithmetic helpers
// (oracle/or_common.h: NeighborGrid, dot4 / sqn4).  Built by tests/spin_ref.py into a shared
// object; never linked into libpfx.  Plain sequential `+=` into a double matrix in FLANN
// neighbour order, single-threaded like PCL's class.  The matrix sum is Eigen 3.2's
// (pfx_eigen_redux.h, shared with the kernel and pinned on its own by tests/test_spin_ref.py).
#include <cfloat>

#include <algorithm>

#include "../../pcl_feature_extraction_amd/csrc/pfx_eigen_redux.h"
#include "or_common.h"

using namespace orc;

extern "C" {

// Eigen 3.2's sum() of n doubles
double spin_eigen_sum(const double* m, int n) { return pfx::eigen_redux_sum(m, n); }

// out: nq x S floats, S = (W + 1)(2W + 1); raw (nullable): nq x S doubles before normalisation;
// sums (nullable): nq doubles.  snx / sny / snz nullable unless support_cos > 0.  reversed != 0
// walks every neighbourhood from its last neighbour to its first (the order test's teeth).
// stats (nullable, 6): sum of k, max k, rows with too few neighbours, rows with a cosine out of
// range, the first row of either kind (-1: none).  An offending row is left as zeros.
// Returns the number of offending rows.
int spin_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
             const float* snz, i64 ns, const float* qx, const float* qy, const float* qz, const float* ax,
             const float* ay, const float* az, i64 nq, double r, int W, double support_cos, int min_pts,
             int reversed, float* out, double* raw, double* sums, i64* stats) {
  const int rows = W + 1, cols = 2 * W + 1, S = rows * cols;
  const double bin_size = r / W / std::sqrt(2.0);
  const double lim = 1.0 + 10 * std::numeric_limits<float>::epsilon();
  NeighborGrid g;
  g.build(sx, sy, sz, ns, r);
  std::vector<int> idx;
  std::vector<float> d2;
  std::vector<double> m((size_t)S);  // column-major, as Eigen's ArrayXXd: m[alpha_bin + rows * beta_bin]
  i64 nb = 0, kmax = 0, few = 0, bad = 0, first_few = -1, first_bad = -1;
  for (i64 q = 0; q < nq; ++q) {
    float* o = out + q * S;
    for (int i = 0; i < S; ++i) o[i] = 0.0f;
    if (raw) for (int i = 0; i < S; ++i) raw[q * S + i] = 0.0;
    if (sums) sums[q] = 0.0;
    g.radius(qx[q], qy[q], qz[q], r, idx, d2);  // (d2, index) ascending; empty for a non-finite query
    const int k = (int)idx.size();
    nb += k;
    kmax = std::max<i64>(kmax, k);
    if (k < min_pts) {  // PCL throws
      ++few;
      if (first_few < 0) first_few = q;
      continue;
    }
    if (reversed) std::reverse(idx.begin(), idx.end());
    std::fill(m.begin(), m.end(), 0.0);
    const V3 axis = v3(ax[q], ay[q], az[q]);
    bool thrown = false;
    for (int i = 0; i < k && !thrown; ++i) {
      const int p = idx[(size_t)i];
      if (support_cos > 0.0) {
        double c = (double)dot4(axis, v3(snx[p], sny[p], snz[p]));
        if (std::fabs(c) > lim) { thrown = true; break; }
        c = std::max(-1.0, std::min(1.0, c));
        if (std::fabs(c) < support_cos) continue;  // counter-directed normals are kept
      }
      const V3 d = sub(v3(sx[p], sy[p], sz[p]), v3(qx[q], qy[q], qz[q]));
      const double dn = (double)std::sqrt(sqn4(d));
      if (std::fabs(dn) < 10 * std::numeric_limits<float>::epsilon()) continue;
      double cs = (double)dot4(d, axis) / dn;
      if (std::fabs(cs) > lim) { thrown = true; break; }
      cs = std::max(-1.0, std::min(1.0, cs));  // libstdc++: a NaN cosine becomes exactly 1.0
      double beta = dn * cs;
      double alpha = dn * std::sqrt(1.0 - cs * cs);
      if (std::fabs(beta) >= bin_size * W || alpha >= bin_size * W) continue;  // outside the cylinder
      int beta_bin = (int)std::floor(beta / bin_size) + W;
      int alpha_bin = (int)std::floor(alpha / bin_size);
      if (alpha_bin == W) {
        alpha_bin--;
        alpha = bin_size * (alpha_bin + 1) - std::numeric_limits<double>::epsilon();
      }
      if (beta_bin == 2 * W) {
        beta_bin--;
        beta = bin_size * (beta_bin - W + 1) - std::numeric_limits<double>::epsilon();
      }
      const double a = alpha / bin_size - (double)alpha_bin;
      const double b = beta / bin_size - (double)(beta_bin - W);
      // (PCL would write outside its array: never taken for finite input, skipped as the kernel does)
      if (alpha_bin < 0 || alpha_bin >= W || beta_bin < 0 || beta_bin >= 2 * W) continue;
      m[(size_t)(alpha_bin + rows * beta_bin)] += (1 - a) * (1 - b);
      m[(size_t)(alpha_bin + 1 + rows * beta_bin)] += a * (1 - b);
      m[(size_t)(alpha_bin + rows * (beta_bin + 1))] += (1 - a) * b;
      m[(size_t)(alpha_bin + 1 + rows * (beta_bin + 1))] += a * b;
    }
    if (thrown) {
      ++bad;
      if (first_bad < 0) first_bad = q;
      continue;
    }
    if (raw)
      for (int a = 0; a < rows; ++a)
        for (int b = 0; b < cols; ++b) raw[q * S + a * cols + b] = m[(size_t)(a + rows * b)];
    if (k > 1) {  // the neighbour count, not the number that contributed
      const double sum = pfx::eigen_redux_sum(m.data(), S);
      if (sums) sums[q] = sum;
      const double inv = 1.0 / sum;  // Eigen 3.2's `/=` by a scalar multiplies by the reciprocal
      for (int i = 0; i < S; ++i) m[(size_t)i] = m[(size_t)i] * inv;
    }
    for (int a = 0; a < rows; ++a)
      for (int b = 0; b < cols; ++b) o[a * cols + b] = (float)m[(size_t)(a + rows * b)];
  }
  if (stats) {
    stats[0] = nb; stats[1] = kmax; stats[2] = few; stats[3] = bad; stats[4] = first_few; stats[5] = first_bad;
  }
  return (int)(few + bad);
}

}  // extern "C"
