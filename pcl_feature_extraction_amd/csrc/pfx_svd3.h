// pfx_svd3.h -- the 3x3 part of Umeyama's rigid fit, host and device: one-sided Jacobi SVD in
// double, determinant, and the rotation U S V^T.  RANSAC scores its hypotheses with it on the
// device (pfx_ransac.hip); ICP fits its per-iteration transformation with it on the host
// (pfx_icp.hip).  Restated in oracle/or_ransac.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define PFX_HD __host__ __device__

namespace pfx {

// one-sided Jacobi SVD of a 3x3 (row-major) in double: A = U diag(d) V^T, d descending >= 0,
// U and V orthonormal (U completed by cross products where d is 0)
PFX_HD inline void svd3(const double A[9], double U[9], double d[3], double V[9]) {
  double B[9];
  for (int i = 0; i < 9; ++i) B[i] = A[i];
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
        if (gamma == 0.0 || fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
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
  for (int j = 0; j < 3; ++j)
    d[j] = sqrt(B[j] * B[j] + B[3 + j] * B[3 + j] + B[6 + j] * B[6 + j]);
  // sort descending (columns of B and V follow)
  for (int i = 0; i < 2; ++i) {
    int k = i;
    for (int j = i + 1; j < 3; ++j)
      if (d[j] > d[k]) k = j;
    if (k != i) {
      double tmp = d[i];
      d[i] = d[k];
      d[k] = tmp;
      for (int r = 0; r < 3; ++r) {
        tmp = B[3 * r + i]; B[3 * r + i] = B[3 * r + k]; B[3 * r + k] = tmp;
        tmp = V[3 * r + i]; V[3 * r + i] = V[3 * r + k]; V[3 * r + k] = tmp;
      }
    }
  }
  // U columns: B columns / d; zero singular values completed to an orthonormal basis
  for (int j = 0; j < 3; ++j)
    for (int r = 0; r < 3; ++r) U[3 * r + j] = d[j] > 0.0 ? B[3 * r + j] / d[j] : 0.0;
  if (!(d[1] > 0.0)) {  // rank <= 1: any unit vector orthogonal to u0
    const double ux = U[0], uy = U[3], uz = U[6];
    double a[3] = {0.0, 0.0, 0.0};
    const double ax = fabs(ux), ay = fabs(uy), az = fabs(uz);
    if (ax <= ay && ax <= az) a[0] = 1.0; else if (ay <= az) a[1] = 1.0; else a[2] = 1.0;
    double v[3] = {uy * a[2] - uz * a[1], uz * a[0] - ux * a[2], ux * a[1] - uy * a[0]};
    const double nv = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (nv > 0.0) for (int r = 0; r < 3; ++r) U[3 * r + 1] = v[r] / nv;
    if (!(d[0] > 0.0)) { U[0] = 1.0; U[3] = 0.0; U[6] = 0.0; U[1] = 0.0; U[4] = 1.0; U[7] = 0.0; }
  }
  if (!(d[2] > 0.0)) {  // u2 = u0 x u1
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
  }
}

PFX_HD inline double det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Umeyama's rotation from the 3x3 covariance sigma (row-major): U S V^T with Eigen's sign of S
// (det(sigma) < 0) and its rank-2 rule
PFX_HD inline void umeyama_rotation3(const double sigma[9], double R[9]) {
  double U[9], d[3], V[9];
  svd3(sigma, U, d, V);
  double S[3] = {1.0, 1.0, 1.0};
  if (det3(sigma) < 0.0) S[2] = -1.0;
  int rank = 0;
  for (int i = 0; i < 3; ++i)
    if (!(fabs(d[i]) <= fabs(d[0]) * 1e-12)) ++rank;
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

}  // namespace pfx
