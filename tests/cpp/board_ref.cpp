// board_ref.cpp -- TEST INFRASTRUCTURE ONLY: the CPU restatement of the contract of pfx_board.hip as
// DESIGN.md states it ("BOARD: the contract"): PCL 1.7 BOARDLocalReferenceFrameEstimation
// (features/impl/board.hpp) without hole analysis, its plane fit taken from the double scatter
// matrix through Eigen 3.2's SelfAdjointEigenSolver (oracle/or_common.h selfadjoint_eigen3) in
// place of PCL's float JacobiSVD.
// Built by tests/board_ref.py into a shared object; never linked into libpfx.  Plain sequential
// loops in FLANN neighbour order on the oracle's NeighborGrid, two searches where PCL makes two.
// Every NaN is written as 0x7fc00000, as the kernel does.
#include <cfloat>
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

inline void nan_row(float* o) {
  for (int e = 0; e < 9; ++e) o[e] = canon_nan(NAN);
}

}  // namespace

extern "C" {

// rf: nq x 9 (x, y, z axis).  reversed != 0 walks the support's sums from its last neighbour to its
// first (the scan for the most inclined normal keeps its order).  stats (nullable, 2): sum and max
// of the number of neighbours at max(r, tangent_radius), what the kernel gathers.  counts (nullable,
// nq): that number for every row.  chosen (nullable, nq): the surface index of the neighbour that
// gives the x axis, -1 where none does.
void board_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
               const float* snz, i64 ns, const float* qx, const float* qy, const float* qz, i64 nq, double r,
               float tangent_radius, float margin_thresh, int reversed, float* rf, i64* stats, i64* counts,
               i64* chosen) {
  const double rt = (double)tangent_radius;
  const bool second = tangent_radius != 0.0f && r != rt;
  NeighborGrid g, gt;
  g.build(sx, sy, sz, ns, r);
  if (second) gt.build(sx, sy, sz, ns, rt);
  const float radius2 = tangent_radius * tangent_radius;
  const float margin2 = (margin_thresh * margin_thresh) * radius2;
  std::vector<int> idx, tidx;
  std::vector<float> d2, td2;
  i64 nb = 0, kmax = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* o = rf + 9 * q;
    const float px = qx[q], py = qy[q], pz = qz[q];
    g.radius(px, py, pz, r, idx, d2);  // (d2, index) ascending; empty for a non-finite query
    if (second) gt.radius(px, py, pz, rt, tidx, td2);
    const i64 gathered = (i64)std::max(idx.size(), second ? tidx.size() : (size_t)0);
    nb += gathered;
    kmax = std::max(kmax, gathered);
    if (counts) counts[q] = gathered;
    if (chosen) chosen[q] = -1;
    const int k = (int)idx.size();
    if (k < 6) {
      nan_row(o);
      continue;
    }
    std::vector<int> walk(idx);
    if (reversed) std::reverse(walk.begin(), walk.end());
    // the plane fit: the centroid, then the scatter matrix of the demeaned points in double
    float cx = 0.f, cy = 0.f, cz = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = walk[(size_t)i];
      cx = cx + sx[p];
      cy = cy + sy[p];
      cz = cz + sz[p];
    }
    cx = cx / (float)k;
    cy = cy / (float)k;
    cz = cz / (float)k;
    double xx = 0.0, xy = 0.0, xz = 0.0, yy = 0.0, yz = 0.0, zz = 0.0;
    for (int i = 0; i < k; ++i) {
      const int p = walk[(size_t)i];
      const float a0 = sx[p] - cx, a1 = sy[p] - cy, a2 = sz[p] - cz;
      xx = xx + (double)a0 * (double)a0;
      xy = xy + (double)a0 * (double)a1;
      xz = xz + (double)a0 * (double)a2;
      yy = yy + (double)a1 * (double)a1;
      yz = yz + (double)a1 * (double)a2;
      zz = zz + (double)a2 * (double)a2;
    }
    const double cov[9] = {xx, xy, xz, xy, yy, yz, xz, yz, zz};
    double ev[3], V[3][3];
    selfadjoint_eigen3(cov, ev, V);
    float z0 = (float)V[0][0], z1 = (float)V[0][1], z2 = (float)V[0][2];
    // disambiguation: towards the mean of the support's normals (NaN normals included)
    float mx = 0.f, my = 0.f, mz = 0.f;
    for (int i = 0; i < k; ++i) {
      const int p = walk[(size_t)i];
      mx = mx + snx[p];
      my = my + sny[p];
      mz = mz + snz[p];
    }
    const float mn = std::sqrt((mx * mx + my * my) + mz * mz);
    mx = mx / mn;
    my = my / mn;
    mz = mz / mn;
    if ((z0 * mx + z1 * my) + z2 * mz < 0.f) {
      z0 = -z0;
      z1 = -z1;
      z2 = -z2;
    }
    // the tangent set replaces the support
    const std::vector<int>& ti = second ? tidx : idx;
    const std::vector<float>& td = second ? td2 : d2;
    const int kt = (int)ti.size();
    // the most inclined normal among the margin neighbours, else among all
    float min_cos = FLT_MAX;
    int best = -1;
    bool margin_found = false;
    for (int i = 0; i < kt; ++i) {
      if (!(td[(size_t)i] > margin2)) continue;
      margin_found = true;
      const int p = ti[(size_t)i];
      const float c = (z0 * snx[p] + z1 * sny[p]) + z2 * snz[p];
      if (c < min_cos) {
        min_cos = c;
        best = p;
      }
    }
    if (!margin_found)
      for (int i = 0; i < kt; ++i) {
        const int p = ti[(size_t)i];
        const float c = (z0 * snx[p] + z1 * sny[p]) + z2 * snz[p];
        if (c < min_cos) {
          min_cos = c;
          best = p;
        }
      }
    if (best < 0) {
      nan_row(o);
      continue;
    }
    if (chosen) chosen[q] = best;
    // directedOrthogonalAxis
    const float bx = sx[best], by = sy[best], bz = sz[best];
    const float ox = bx - px, oy = by - py, oz = bz - pz;
    const float t = (z0 * ox + z1 * oy) + z2 * oz;
    const float jx = bx - t * z0, jy = by - t * z1, jz = bz - t * z2;
    float x0 = jx - px, x1 = jy - py, x2 = jz - pz;
    const float xn = std::sqrt((x0 * x0 + x1 * x1) + x2 * x2);
    x0 = x0 / xn;
    x1 = x1 / xn;
    x2 = x2 / xn;
    o[0] = canon_nan(x0);
    o[1] = canon_nan(x1);
    o[2] = canon_nan(x2);
    o[3] = canon_nan(z1 * x2 - z2 * x1);
    o[4] = canon_nan(z2 * x0 - z0 * x2);
    o[5] = canon_nan(z0 * x1 - z1 * x0);
    o[6] = canon_nan(z0);
    o[7] = canon_nan(z1);
    o[8] = canon_nan(z2);
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
  }
}

}  // extern "C"
