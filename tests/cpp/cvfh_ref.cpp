// cvfh_ref.cpp -- TEST INFRASTRUCTURE ONLY: the CPU restatement of the contract of pfx_cvfh.hip as
// DESIGN.md states it ("CVFH: the contract"): PCL 1.7 CVFHEstimation::computeFeature with
// extractEuclideanClustersSmooth and VFHEstimation::computePointSPFHSignature, on the oracle's
// arithmetic helpers (oracle/or_common.h: NeighborGrid, dot4 / sqn4, atan2f_glibc).  Built by
// tests/cvfh_ref.py into a shared object; never linked into libpfx.
// The clustering is PCL's in its own shape: a seed, a queue, a radius search per queued point, acos
// per candidate.  The normals of the filtered cloud are an argument (the tests take them from the
// oracle's normal estimation); the bins are plain sequential `+= incr` loops.
#include <climits>

#include <algorithm>

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

bool finite3(float a, float b, float c) { return std::isfinite(a) && std::isfinite(b) && std::isfinite(c); }

// the edge's angle test, as PCL writes it
bool smooth(float dot, double eps) { return std::fabs(std::acos((double)dot)) < eps; }

float normalDot(const float* nx, const float* ny, const float* nz, i64 i, i64 j) {
  return (nx[i] * nx[j] + ny[i] * ny[j]) + nz[i] * nz[j];
}

// extractEuclideanClustersSmooth.  labels: the cluster (numbered by seed) or -1.  stats (3): edges
// (each once), the hooking rounds of the kernel's scheme (see below), clusters.
void clusters(const float* x, const float* y, const float* z, const float* nx, const float* ny, const float* nz, i64 n,
              float tolerance, double eps, int min_points, int32_t* labels, i64* stats) {
  const double t = (double)tolerance;
  NeighborGrid g;
  g.build(x, y, z, n, t);
  std::vector<std::vector<int> > adj((size_t)n);
  std::vector<int> idx;
  std::vector<float> d2;
  i64 edges = 0;
  for (i64 i = 0; i < n; ++i) {
    g.radius(x[i], y[i], z[i], t, idx, d2);  // d^2 < (float)(t t); empty for a non-finite point
    for (int j : idx)
      if (j != i && smooth(normalDot(nx, ny, nz, i, j), eps)) {
        adj[(size_t)i].push_back(j);
        edges += j < i;
      }
  }
  // PCL's queue growth
  std::vector<char> processed((size_t)n, 0);
  std::vector<int> queue;
  i64 found = 0;
  for (i64 i = 0; i < n; ++i) labels[i] = -1;
  for (i64 i = 0; i < n; ++i) {
    if (processed[(size_t)i] || !finite3(x[i], y[i], z[i])) continue;
    queue.assign(1, (int)i);
    processed[(size_t)i] = 1;
    for (size_t s = 0; s < queue.size(); ++s)
      for (int j : adj[(size_t)queue[s]])
        if (!processed[(size_t)j]) {
          processed[(size_t)j] = 1;
          queue.push_back(j);
        }
    if ((i64)queue.size() >= (i64)min_points) {
      for (int j : queue) labels[j] = (int32_t)found;
      ++found;
    }
  }
  // The rounds the kernel's scheme takes (a statistic, not a result): every point's root takes the
  // smallest root label among the point's edge neighbours, then every label goes to its root; until
  // a round changes nothing (that round counts).
  std::vector<int> lab((size_t)n), par((size_t)n);
  for (i64 i = 0; i < n; ++i) lab[(size_t)i] = par[(size_t)i] = (int)i;
  i64 rounds = 0;
  for (bool changed = n > 0; changed;) {
    changed = false;
    ++rounds;
    for (i64 i = 0; i < n; ++i) {
      int m = lab[(size_t)i];
      for (int j : adj[(size_t)i]) m = std::min(m, lab[(size_t)j]);
      if (m < lab[(size_t)i]) {
        par[(size_t)lab[(size_t)i]] = std::min(par[(size_t)lab[(size_t)i]], m);
        changed = true;
      }
    }
    for (i64 i = 0; i < n; ++i) {
      int r = lab[(size_t)i];
      while (par[(size_t)r] != r) r = par[(size_t)r];
      lab[(size_t)i] = r;
    }
    for (i64 i = 0; i < n; ++i) par[(size_t)i] = lab[(size_t)i];
  }
  if (stats) { stats[0] = edges; stats[1] = rounds; stats[2] = found; }
}

}  // namespace

extern "C" {

struct cvfh_ref_params {
  float viewpoint[3];
  float radius_normals, cluster_tolerance, eps_angle_threshold, curvature_threshold;
  int32_t min_points, normalize_bins;
};

// the smallest float T with acos((double)T) < eps by bisection over the float bit patterns of
// [-1, 1]; +inf when there is none
float cvfh_acos_threshold(double eps) {
  if (!smooth(1.0f, eps)) return INFINITY;
  if (smooth(-1.0f, eps)) return -1.0f;
  // keys that order as the floats do: negative floats descend with their bits
  int64_t lo = -(int64_t)(f2w(-1.0f) & 0x7fffffff), hi = f2w(1.0f);
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    const float v = mid >= 0 ? w2f((int32_t)mid) : w2f((int32_t)(0x80000000u | (uint32_t)(-mid)));
    if (smooth(v, eps)) hi = mid; else lo = mid;
  }
  return hi >= 0 ? w2f((int32_t)hi) : w2f((int32_t)(0x80000000u | (uint32_t)(-hi)));
}

int cvfh_smooth(float dot, double eps) { return smooth(dot, eps) ? 1 : 0; }

void smooth_clusters_ref(const float* x, const float* y, const float* z, const float* nx, const float* ny,
                         const float* nz, i64 n, float tolerance, double eps, int32_t min_points, int32_t* labels,
                         i64* stats) {
  clusters(x, y, z, nx, ny, nz, n, tolerance, eps, min_points, labels, stats);
}

// keep[p] = the curvature filter's verdict on indexed point p (indices nullable: all)
void cvfh_filter_ref(const float* curv, const int32_t* indices, i64 np, float threshold, uint8_t* keep) {
  for (i64 p = 0; p < np; ++p) keep[p] = !(curv[indices ? indices[p] : p] > threshold);
}

// (fnx, fny, fnz): the normals of the filtered cloud, one per kept point in order (nf of them, as
// cvfh_filter_ref keeps them), estimated at radius_normals from the origin.
// rows: cap x 308, counts: cap x 308, centroids / dominant: cap x 3, labels: np, stats (5): filtered,
// clusters, edges, rounds, rows.  Returns the number of rows (nothing beyond cap is written).
i64 cvfh_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny, const float* snz,
             const float* scurv, i64 ns, const int32_t* indices, i64 np, const cvfh_ref_params* prm, const float* fnx,
             const float* fny, const float* fnz, i64 nf, float* rows, int32_t* counts, float* centroids,
             float* dominant, int32_t* labels, i64 cap, i64* stats) {
  for (int s = 0; s < 5; ++s) stats[s] = 0;
  if (np == 0) return 0;
  std::vector<i64> in;  // indexed positions the filter keeps
  for (i64 p = 0; p < np; ++p)
    if (!(scurv[indices ? indices[p] : p] > prm->curvature_threshold)) in.push_back(p);
  if ((i64)in.size() != nf) return -1;
  std::vector<float> fx((size_t)nf), fy((size_t)nf), fz((size_t)nf);
  for (i64 f = 0; f < nf; ++f) {
    const i64 i = indices ? indices[in[(size_t)f]] : in[(size_t)f];
    fx[(size_t)f] = sx[i]; fy[(size_t)f] = sy[i]; fz[(size_t)f] = sz[i];
  }
  std::vector<int32_t> flab((size_t)nf, -1);
  i64 cs[3] = {0, 0, 0};
  // (PCL skips this with fewer than min_points points in F; no component could reach min_points
  // then, so only the edge and round statistics tell the difference, and they describe F's graph)
  cs[1] = 1;  // (an empty F: the one round that changes nothing)
  if (nf > 0)
    clusters(fx.data(), fy.data(), fz.data(), fnx, fny, fnz, nf, prm->cluster_tolerance,
             (double)prm->eps_angle_threshold, prm->min_points, flab.data(), cs);
  const i64 nc = cs[2], nrows = nc > 0 ? nc : 1;
  stats[0] = nf; stats[1] = nc; stats[2] = cs[0]; stats[3] = cs[1]; stats[4] = nrows;
  for (i64 p = 0; p < np; ++p) labels[p] = -1;
  for (i64 f = 0; f < nf; ++f) labels[in[(size_t)f]] = flab[(size_t)f];
  if (nrows > cap) return nrows;
  std::vector<V3> cen((size_t)nrows), dom((size_t)nrows);
  for (i64 c = 0; c < nc; ++c) {  // members in ascending index order, Vector4f +=
    V3 sp = v3(0, 0, 0), sn = v3(0, 0, 0);
    i64 size = 0;
    for (i64 f = 0; f < nf; ++f)
      if (flab[(size_t)f] == c) {
        sp = add(sp, v3(fx[(size_t)f], fy[(size_t)f], fz[(size_t)f]));
        sn = add(sn, v3(fnx[f], fny[f], fnz[f]));
        ++size;
      }
    const float inv = 1.0f / (float)size;  // Eigen 3.2's `/=`: times the reciprocal
    const V3 a = mul(sn, inv);
    cen[(size_t)c] = mul(sp, inv);
    dom[(size_t)c] = mul(a, 1.0f / std::sqrt(sqn4(a)));  // Vector4f::normalize, w = 0
  }
  if (nc == 0) {  // the centroid of the whole surface and the mean of the indexed normals
    V3 sp = v3(0, 0, 0), sn = v3(0, 0, 0);
    i64 cp = 0, cn = 0;
    for (i64 i = 0; i < ns; ++i)
      if (finite3(sx[i], sy[i], sz[i])) { sp = add(sp, v3(sx[i], sy[i], sz[i])); ++cp; }
    for (i64 p = 0; p < np; ++p) {
      const i64 i = indices ? indices[p] : p;
      if (finite3(snx[i], sny[i], snz[i])) { sn = add(sn, v3(snx[i], sny[i], snz[i])); ++cn; }
    }
    cen[0] = mul(sp, 1.0f / (float)cp);
    dom[0] = mul(sn, 1.0f / (float)cn);
  }
  const float d_pi = 1.0f / (2.0f * (float)M_PI);
  const float incr_shape = prm->normalize_bins ? 100.0f / (float)(np - 1) : 1.0f;
  const float incr_vp = prm->normalize_bins ? (float)(100.0 / (double)np) : 1.0f;
  for (i64 r = 0; r < nrows; ++r) {
    const V3 c = cen[(size_t)r], n1 = dom[(size_t)r];
    centroids[r * 3] = c.x; centroids[r * 3 + 1] = c.y; centroids[r * 3 + 2] = c.z;
    dominant[r * 3] = n1.x; dominant[r * 3 + 1] = n1.y; dominant[r * 3 + 2] = n1.z;
    float* h = rows + r * 308;
    int32_t* cnt = counts + r * 308;
    for (int b = 0; b < 308; ++b) { h[b] = 0.0f; cnt[b] = 0; }
    bool any = false;
    float factor = 0.0f;
    for (i64 p = 0; p < np; ++p) {
      const i64 i = indices ? indices[p] : p;
      const float d = std::sqrt(sqn3(sub(c, v3(sx[i], sy[i], sz[i]))));
      if (d != d) continue;
      if (!any || d > factor) factor = d;
      any = true;
    }
    if (!any) factor = kNaN;
    V3 dvp = sub(v3(prm->viewpoint[0], prm->viewpoint[1], prm->viewpoint[2]), c);
    dvp = mul(dvp, 1.0f / std::sqrt(sqn4(dvp)));
    for (i64 p = 0; p < np; ++p) {
      const i64 i = indices ? indices[p] : p;
      const V3 pt = v3(sx[i], sy[i], sz[i]), nn = v3(snx[i], sny[i], snz[i]);
      float f1, f2, f3, f4;
      if (pairFeatures(c, n1, pt, nn, f1, f2, f3, f4)) {
        const int b1 = clampBin(45 * ((f1 + M_PI) * d_pi), 45);
        const int b2 = clampBin(45 * ((f2 + 1.0) * 0.5), 45);
        const int b3 = clampBin(45 * ((f3 + 1.0) * 0.5), 45);
        const int b4 = clampBin(45 * ((double)f4 / (double)factor), 45);
        h[b1] += incr_shape; h[45 + b2] += incr_shape; h[90 + b3] += incr_shape; h[135 + b4] += incr_shape;
        ++cnt[b1]; ++cnt[45 + b2]; ++cnt[90 + b3]; ++cnt[135 + b4];
      }
      const double alpha = ((double)dot4(nn, dvp) + 1.0) * 0.5;
      const int bv = clampBin(alpha * 128, 128);
      h[180 + bv] += incr_vp;
      ++cnt[180 + bv];
    }
  }
  return nrows;
}

}  // extern "C"
