// =====================================================================================
//  tests/cpp/icp_ref.cpp  --  TEST INFRASTRUCTURE ONLY (parity vs real PCL UNPINNED)
//
//  CPU restatement of pcl::IterativeClosestPoint<PointXYZRGB,PointXYZRGB>::align as the
//  reference's icpAlign runs it (evaluation.cpp:863-885), after DESIGN.md "ICP: the contract":
//  PCL 1.7.2 icp.hpp, correspondence_estimation.hpp, transformation_estimation_svd.hpp,
//  default_convergence_criteria.hpp and Eigen 3.2 Umeyama.h, reconstructed from memory.  The
//  step numbers below are the contract's.  All float math is binary32, left to right, no FMA
//  (built with -O2 -ffp-contract=off).  The 3x3 SVD, the sign of S and the rank-2 rule are
//  oracle/or_ransac.cpp's umeyama3 (a restatement choice).  The nearest-neighbour search is a
//  uniform grid scanned in growing shells: exact, with the lowest target index among equal d2.
// =====================================================================================
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "or_common.h"
#include "pfx.h"  // PFX_ICP_GEMM_DEPTH: the depth block shared with the kernel

namespace {

typedef int64_t i64;
const int kIcpGemmDepth = PFX_ICP_GEMM_DEPTH;

// ---- oracle/or_ransac.cpp's 3x3 pieces (verbatim arithmetic) --------------------------------
void svd3(const double A[9], double U[9], double d[3], double V[9]) {
  double B[9];
  std::memcpy(B, A, sizeof(B));
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int i = 0; i < 3; ++i) {
          alpha += B[3 * i + p] * B[3 * i + p];
          beta += B[3 * i + q] * B[3 * i + q];
          gamma += B[3 * i + p] * B[3 * i + q];
        }
        if (gamma == 0.0 || std::fabs(gamma) <= 1e-15 * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double bp = B[3 * i + p], bq = B[3 * i + q];
          B[3 * i + p] = c * bp - s * bq;
          B[3 * i + q] = s * bp + c * bq;
          const double vp = V[3 * i + p], vq = V[3 * i + q];
          V[3 * i + p] = c * vp - s * vq;
          V[3 * i + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  for (int j = 0; j < 3; ++j) d[j] = std::sqrt(B[j] * B[j] + B[3 + j] * B[3 + j] + B[6 + j] * B[6 + j]);
  for (int i = 0; i < 2; ++i) {
    int k = i;
    for (int j = i + 1; j < 3; ++j)
      if (d[j] > d[k]) k = j;
    if (k != i) {
      std::swap(d[i], d[k]);
      for (int r = 0; r < 3; ++r) {
        std::swap(B[3 * r + i], B[3 * r + k]);
        std::swap(V[3 * r + i], V[3 * r + k]);
      }
    }
  }
  for (int j = 0; j < 3; ++j)
    for (int r = 0; r < 3; ++r) U[3 * r + j] = d[j] > 0.0 ? B[3 * r + j] / d[j] : 0.0;
  if (!(d[1] > 0.0)) {
    const double ux = U[0], uy = U[3], uz = U[6];
    double a[3] = {0.0, 0.0, 0.0};
    const double ax = std::fabs(ux), ay = std::fabs(uy), az = std::fabs(uz);
    if (ax <= ay && ax <= az) a[0] = 1.0; else if (ay <= az) a[1] = 1.0; else a[2] = 1.0;
    double v[3] = {uy * a[2] - uz * a[1], uz * a[0] - ux * a[2], ux * a[1] - uy * a[0]};
    const double nv = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (nv > 0.0) for (int r = 0; r < 3; ++r) U[3 * r + 1] = v[r] / nv;
    if (!(d[0] > 0.0)) { U[0] = 1.0; U[3] = 0.0; U[6] = 0.0; U[1] = 0.0; U[4] = 1.0; U[7] = 0.0; }
  }
  if (!(d[2] > 0.0)) {
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }
}

double det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

void rotation3(const double sigma[9], double R[9]) {
  double U[9], d[3], V[9];
  svd3(sigma, U, d, V);
  double S[3] = {1.0, 1.0, 1.0};
  if (det3(sigma) < 0.0) S[2] = -1.0;
  int rank = 0;
  for (int i = 0; i < 3; ++i)
    if (!(std::fabs(d[i]) <= std::fabs(d[0]) * 1e-12)) ++rank;
  double Sd[3] = {S[0], S[1], S[2]};
  if (rank == 2) {
    if (det3(U) * det3(V) > 0.0) {
      Sd[0] = Sd[1] = Sd[2] = 1.0;
    } else {
      Sd[0] = S[0]; Sd[1] = S[1]; Sd[2] = -1.0;
    }
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double acc = (U[3 * i] * Sd[0]) * V[3 * j];
      acc += (U[3 * i + 1] * Sd[1]) * V[3 * j + 1];
      acc += (U[3 * i + 2] * Sd[2]) * V[3 * j + 2];
      R[3 * i + j] = acc;
    }
}

// ---- exact nearest neighbour on a uniform grid ----------------------------------------------
inline i64 iabs(i64 v) { return v < 0 ? -v : v; }
inline bool finite3(float x, float y, float z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

struct RefGrid {
  const float *x, *y, *z;
  double h, inv, o[3];
  i64 d[3];
  std::vector<int32_t> start, idx;

  i64 cell_of(double v, int a) const {
    const double c = std::floor((v - o[a]) * inv);
    return (i64)std::max(-1e12, std::min(1e12, c));
  }
  void build(const float* tx, const float* ty, const float* tz, i64 n) {
    x = tx; y = ty; z = tz;
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    i64 nf = 0;
    for (i64 i = 0; i < n; ++i) {
      if (!finite3(x[i], y[i], z[i])) continue;
      const double p[3] = {x[i], y[i], z[i]};
      for (int a = 0; a < 3; ++a) {
        lo[a] = nf ? std::min(lo[a], p[a]) : p[a];
        hi[a] = nf ? std::max(hi[a], p[a]) : p[a];
      }
      ++nf;
    }
    double ext = 0.0, vol = 1.0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, hi[a] - lo[a]);
    for (int a = 0; a < 3; ++a) vol *= std::max(hi[a] - lo[a], ext * 1e-3);
    h = (ext > 0.0 && nf > 0) ? 0.5 * std::cbrt(vol / (double)nf) : 1.0;
    for (;;) {
      double total = 1.0;
      for (int a = 0; a < 3; ++a) {
        d[a] = (i64)std::floor((hi[a] - lo[a]) / h) + 1;
        total *= (double)d[a];
      }
      if (total <= 4194304.0) break;
      h *= 1.3;
    }
    inv = 1.0 / h;
    for (int a = 0; a < 3; ++a) o[a] = lo[a];
    const i64 C = d[0] * d[1] * d[2];
    start.assign((size_t)C + 1, 0);
    std::vector<i64> key((size_t)n, -1);
    for (i64 i = 0; i < n; ++i) {
      if (!finite3(x[i], y[i], z[i])) continue;
      i64 c[3] = {cell_of(x[i], 0), cell_of(y[i], 1), cell_of(z[i], 2)};
      for (int a = 0; a < 3; ++a) c[a] = std::max<i64>(0, std::min(d[a] - 1, c[a]));
      key[(size_t)i] = (c[0] * d[1] + c[1]) * d[2] + c[2];
      ++start[(size_t)key[(size_t)i] + 1];
    }
    for (i64 c = 0; c < C; ++c) start[(size_t)c + 1] += start[(size_t)c];
    idx.assign((size_t)nf, 0);
    std::vector<int32_t> cur(start.begin(), start.end() - 1);
    for (i64 i = 0; i < n; ++i)
      if (key[(size_t)i] >= 0) idx[(size_t)cur[(size_t)key[(size_t)i]]++] = (int32_t)i;
  }
  inline void scan_cell(i64 cx, i64 cy, i64 cz, float qx, float qy, float qz, float& bd, int32_t& bj) const {
    const i64 c = (cx * d[1] + cy) * d[2] + cz;
    for (int32_t p = start[(size_t)c]; p < start[(size_t)c + 1]; ++p) {
      const int32_t j = idx[(size_t)p];
      const float dx = qx - x[j], dy = qy - y[j], dz = qz - z[j];
      const float dd = (dx * dx + dy * dy) + dz * dz;  // step 2
      if (bj < 0 || dd < bd || (dd == bd && j < bj)) {
        bd = dd;
        bj = j;
      }
    }
  }
  // the nearest finite target point (smallest d2, lowest index among equals); cap2: nothing
  // whose d2 exceeds it is wanted (the search may stop there).  False when there is none.
  bool nearest(float qx, float qy, float qz, double cap2, int32_t& bj, float& bd) const {
    bj = -1;
    bd = std::numeric_limits<float>::infinity();
    if (idx.empty()) return false;
    const i64 c[3] = {cell_of(qx, 0), cell_of(qy, 1), cell_of(qz, 2)};
    i64 r0 = 0, rmax = 0;
    for (int a = 0; a < 3; ++a) {
      r0 = std::max(r0, c[a] < 0 ? -c[a] : (c[a] >= d[a] ? c[a] - (d[a] - 1) : 0));
      rmax = std::max(rmax, std::max(iabs(c[a]), iabs(c[a] - (d[a] - 1))));
    }
    for (i64 r = r0; r <= rmax; ++r) {
      const i64 x0 = std::max<i64>(0, c[0] - r), x1 = std::min(d[0] - 1, c[0] + r);
      const i64 y0 = std::max<i64>(0, c[1] - r), y1 = std::min(d[1] - 1, c[1] + r);
      const i64 z0 = std::max<i64>(0, c[2] - r), z1 = std::min(d[2] - 1, c[2] + r);
      for (i64 cx = x0; cx <= x1; ++cx)
        for (i64 cy = y0; cy <= y1; ++cy) {
          if (iabs(cx - c[0]) == r || iabs(cy - c[1]) == r) {
            for (i64 cz = z0; cz <= z1; ++cz) scan_cell(cx, cy, cz, qx, qy, qz, bd, bj);
          } else {
            if (c[2] - r >= 0 && c[2] - r < d[2]) scan_cell(cx, cy, c[2] - r, qx, qy, qz, bd, bj);
            if (r > 0 && c[2] + r >= 0 && c[2] + r < d[2]) scan_cell(cx, cy, c[2] + r, qx, qy, qz, bd, bj);
          }
        }
      // every unseen point is farther than r h on some axis; the margin covers the float d2
      const double seen2 = ((double)r * h) * ((double)r * h) * (1.0 - 1e-5);
      if (bj >= 0 && (double)bd < seen2) break;
      if (seen2 > cap2) break;
    }
    return bj >= 0;
  }
};

// steps 5 and 7: ((m0 x + m1 y) + m2 z) + m3 per row
inline void apply(const float T[16], float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// host seconds of the last icp_ref call by stage (scripts/icp_time.py): search + list, means,
// sigma, the rest of the loop, fitness score
double g_stage[5];
struct Lap {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void to(int k) {
    const auto n = std::chrono::steady_clock::now();
    g_stage[k] += std::chrono::duration<double>(n - t).count();
    t = n;
  }
};

}  // namespace

extern "C" {

void icp_ref_stage_seconds(double* out) { std::memcpy(out, g_stage, sizeof(g_stage)); }

void icp_ref_transform(const float* x, const float* y, const float* z, i64 n, const float* T, float* ox, float* oy,
                       float* oz) {
  for (i64 i = 0; i < n; ++i) apply(T, x[i], y[i], z[i], ox[i], oy[i], oz[i]);
}

// first_*: the correspondences of the first iteration (ns entries each, *n_first used);
// aligned: 3 ns floats (x row, y row, z row) -- every output pointer but T/fitness/state nullable
int icp_ref(const float* sx, const float* sy, const float* sz, i64 ns, const float* tx, const float* ty,
            const float* tz, i64 nt, double max_dist, int max_iterations, double transformation_epsilon,
            double euclidean_fitness_epsilon, const float* guess, float* T_out, double* fitness, int* converged,
            int* iterations_out, int* state_out, i64* n_last, i64* n_first, int32_t* first_src, int32_t* first_tgt,
            float* first_d2, float* aligned) {
  // step 1
  for (double& v : g_stage) v = 0.0;
  Lap lap;
  RefGrid G;
  G.build(tx, ty, tz, nt);
  float final_T[16];
  bool identity = true;
  for (int i = 0; i < 16; ++i) {
    const float e = (i % 5 == 0) ? 1.0f : 0.0f;
    final_T[i] = guess ? guess[i] : e;
    if (final_T[i] != e) identity = false;
  }
  std::vector<float> wx(sx, sx + ns), wy(sy, sy + ns), wz(sz, sz + ns);
  if (!identity)
    for (i64 i = 0; i < ns; ++i) apply(final_T, sx[i], sy[i], sz[i], wx[(size_t)i], wy[(size_t)i], wz[(size_t)i]);
  double prev_mse = DBL_MAX;
  int iterations = 0, state = 0;
  bool conv = false;
  const double cap2 = max_dist * max_dist;
  std::vector<float> ls[3], lt[3], ld2;
  if (n_last) *n_last = 0;
  if (n_first) *n_first = 0;
  for (;;) {
    // step 2
    for (int a = 0; a < 3; ++a) { ls[a].clear(); lt[a].clear(); }
    ld2.clear();
    for (i64 i = 0; i < ns; ++i) {
      const float qx = wx[(size_t)i], qy = wy[(size_t)i], qz = wz[(size_t)i];
      if (!finite3(qx, qy, qz)) continue;
      int32_t j;
      float d2;
      if (!G.nearest(qx, qy, qz, cap2, j, d2)) continue;
      if ((double)d2 > cap2) continue;
      if (iterations == 0 && first_src) {
        first_src[ld2.size()] = (int32_t)i;
        first_tgt[ld2.size()] = j;
        first_d2[ld2.size()] = d2;
      }
      ls[0].push_back(qx); ls[1].push_back(qy); ls[2].push_back(qz);
      lt[0].push_back(tx[j]); lt[1].push_back(ty[j]); lt[2].push_back(tz[j]);
      ld2.push_back(d2);
    }
    const i64 n = (i64)ld2.size();
    if (iterations == 0 && n_first) *n_first = n;
    if (n_last) *n_last = n;
    lap.to(0);
    // step 3
    if (n < 3) {
      state = 5;
      conv = false;
      break;
    }
    // step 4
    const float a = 1.0f / (float)n;
    float ms[3], mt[3];
    for (int c = 0; c < 3; ++c) {
      float s = ls[c][0], t = lt[c][0];
      for (i64 k = 1; k < n; ++k) s = s + ls[c][(size_t)k];
      for (i64 k = 1; k < n; ++k) t = t + lt[c][(size_t)k];
      ms[c] = s * a;
      mt[c] = t * a;
    }
    lap.to(1);
    float sigma[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        float acc = 0.0f;
        for (i64 b = 0; b < n; b += kIcpGemmDepth) {
          const i64 e = std::min(n, b + (i64)kIcpGemmDepth);
          float P = 0.0f;
          for (i64 k = b; k < e; ++k) P = P + (lt[i][(size_t)k] - mt[i]) * (ls[j][(size_t)k] - ms[j]);
          acc = acc + a * P;
        }
        sigma[3 * i + j] = acc;
      }
    lap.to(2);
    double sd[9], R[9];
    for (int i = 0; i < 9; ++i) sd[i] = (double)sigma[i];
    rotation3(sd, R);
    float T[16];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)R[3 * i + j];
      T[4 * i + 3] = mt[i] - ((T[4 * i] * ms[0] + T[4 * i + 1] * ms[1]) + T[4 * i + 2] * ms[2]);
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
    // step 5
    for (i64 i = 0; i < ns; ++i) {
      float ox, oy, oz;
      apply(T, wx[(size_t)i], wy[(size_t)i], wz[(size_t)i], ox, oy, oz);
      wx[(size_t)i] = ox; wy[(size_t)i] = oy; wz[(size_t)i] = oz;
    }
    float nf[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c)
        nf[4 * r + c] = ((T[4 * r] * final_T[c] + T[4 * r + 1] * final_T[4 + c]) + T[4 * r + 2] * final_T[8 + c]) +
                        T[4 * r + 3] * final_T[12 + c];
    std::memcpy(final_T, nf, sizeof(nf));
    ++iterations;
    // step 6
    if (iterations >= max_iterations) {
      state = 1;
      conv = true;
      break;
    }
    const double cos_angle = 0.5 * (double)(((T[0] + T[5]) + T[10]) - 1.0f);
    const double tr2 = (double)((T[3] * T[3] + T[7] * T[7]) + T[11] * T[11]);
    if (cos_angle >= 0.99999 && tr2 <= transformation_epsilon) {
      state = 2;
      conv = true;
      break;
    }
    double sum = 0.0;
    for (i64 k = 0; k < n; ++k) sum += (double)ld2[(size_t)k];
    const double mse = sum / (double)n;
    if (std::fabs(mse - prev_mse) < 1e-12) {
      state = 3;
      conv = true;
      break;
    }
    if (std::fabs(mse - prev_mse) / prev_mse < euclidean_fitness_epsilon) {
      state = 4;
      conv = true;
      break;
    }
    prev_mse = mse;
    lap.to(3);
  }
  lap.to(3);
  // step 7
  double fsum = 0.0;
  i64 fcount = 0;
  for (i64 i = 0; i < ns; ++i) {
    if (!finite3(sx[i], sy[i], sz[i])) continue;
    float qx, qy, qz;
    apply(final_T, sx[i], sy[i], sz[i], qx, qy, qz);
    int32_t j;
    float d2;
    if (!finite3(qx, qy, qz) || !G.nearest(qx, qy, qz, std::numeric_limits<double>::infinity(), j, d2)) continue;
    fsum += (double)d2;
    ++fcount;
  }
  lap.to(4);
  *fitness = fcount ? fsum / (double)fcount : DBL_MAX;
  std::memcpy(T_out, final_T, sizeof(final_T));
  *converged = conv ? 1 : 0;
  *iterations_out = iterations;
  *state_out = state;
  if (aligned)
    for (i64 i = 0; i < ns; ++i) {
      aligned[i] = wx[(size_t)i];
      aligned[ns + i] = wy[(size_t)i];
      aligned[2 * ns + i] = wz[(size_t)i];
    }
  return 0;
}

}  // extern "C"
