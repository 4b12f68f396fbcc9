// boundary_ref.cpp -- TEST INFRASTRUCTURE ONLY: the CPU restatement of the contract of pfx_boundary.hip
// as DESIGN.md states it ("Boundary: the contract"): PCL 1.7 BoundaryEstimation (features/impl/
// boundary.hpp): getCoordinateSystemOnPlane, then isBoundaryPoint's loop in its own shape -- the angles
// of the neighbours into an array, std::sort, the running maximum of the adjacent differences and of
// the wrap term, compared with the threshold at the end.
// Built by tests/boundary_ref.py into a shared object; never linked into libpfx.  The neighbours are
// found by brute force over the surface, in surface order (the result does not depend on it: the
// angles are sorted).  atan2f is the host libm's (glibc).
#include <cfloat>
#include <cmath>
#include <cstdint>

#include <algorithm>
#include <vector>

typedef int64_t i64;

namespace {

const float kPiF = (float)M_PI;

inline bool finite3(float a, float b, float c) { return std::isfinite(a) && std::isfinite(b) && std::isfinite(c); }

// PCL's getCoordinateSystemOnPlane: v = Eigen's generic unitOrthogonal of (n, 0), u = n cross v
inline void plane_axes(const float n[3], float u[3], float v[3]) {
  int m = 0;
  float am = std::fabs(n[0]);
  for (int i = 1; i < 3; ++i)
    if (std::fabs(n[i]) > am) {
      m = i;
      am = std::fabs(n[i]);
    }
  const int s = (m == 0) ? 1 : 0;
  const float len = std::sqrt(n[s] * n[s] + n[m] * n[m]);
  const float inv = 1.0f / len;
  v[0] = v[1] = v[2] = 0.0f;
  v[m] = -n[s] * inv;
  v[s] = n[m] * inv;
  u[0] = n[1] * v[2] - n[2] * v[1];
  u[1] = n[2] * v[0] - n[0] * v[2];
  u[2] = n[0] * v[1] - n[1] * v[0];
}

}  // namespace

extern "C" {

// out: nq bytes (0, 1, 255).  stats (nullable, 3): the sum of k, the largest k, the number of 1s.
// counts (nullable, nq): every row's k.  max_gap (nullable, nq): the running maximum PCL compares
// with the threshold (from FLT_MIN; NaN where the row has no angle).
void boundary_ref(const float* sx, const float* sy, const float* sz, i64 ns, const float* qx, const float* qy,
                  const float* qz, const float* qnx, const float* qny, const float* qnz, i64 nq, double r,
                  float angle_threshold, uint8_t* out, i64* stats, i64* counts, float* max_gap) {
  const float rr = (float)(r * r);
  i64 nb = 0, kmax = 0, flagged = 0;
  std::vector<i64> nbrs;
  std::vector<float> angles;
  for (i64 q = 0; q < nq; ++q) {
    const float px = qx[q], py = qy[q], pz = qz[q];
    nbrs.clear();
    if (finite3(px, py, pz))
      for (i64 i = 0; i < ns; ++i) {
        if (!finite3(sx[i], sy[i], sz[i])) continue;
        const float dx = px - sx[i], dy = py - sy[i], dz = pz - sz[i];
        const float d2 = ((0.0f + dx * dx) + dy * dy) + dz * dz;
        if (d2 < rr) nbrs.push_back(i);
      }
    const i64 k = (i64)nbrs.size();
    nb += k;
    kmax = std::max(kmax, k);
    if (counts) counts[q] = k;
    if (max_gap) max_gap[q] = NAN;
    if (k == 0) {
      out[q] = 255;
      continue;
    }
    out[q] = 0;
    if (k < 3) continue;
    const float n[3] = {qnx[q], qny[q], qnz[q]};
    float u[3], v[3];
    plane_axes(n, u, v);
    if (!finite3(u[0], u[1], u[2]) || !finite3(v[0], v[1], v[2])) continue;
    angles.clear();
    bool nan_angle = false;
    for (i64 i : nbrs) {
      const float d0 = sx[i] - px, d1 = sy[i] - py, d2 = sz[i] - pz;
      if (d0 == 0.0f && d1 == 0.0f && d2 == 0.0f) continue;
      const float du = (u[0] * d0 + u[1] * d1) + u[2] * d2;
      const float dv = (v[0] * d0 + v[1] * d1) + v[2] * d2;
      const float a = ::atan2f(dv, du);
      nan_angle = nan_angle || a != a;
      angles.push_back(a);
    }
    const size_t cp = angles.size();
    if (cp == 0 || nan_angle) continue;
    std::sort(angles.begin(), angles.end());
    float max_dif = FLT_MIN, dif;
    for (size_t i = 0; i < cp - 1; ++i) {
      dif = angles[i + 1] - angles[i];
      if (max_dif < dif) max_dif = dif;
    }
    dif = 2 * kPiF - angles[cp - 1] + angles[0];
    if (max_dif < dif) max_dif = dif;
    if (max_gap) max_gap[q] = max_dif;
    if (max_dif > angle_threshold) {
      out[q] = 1;
      ++flagged;
    }
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
    stats[2] = flagged;
  }
}

}  // extern "C"
