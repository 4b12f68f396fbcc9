// pfx_igrad.h -- IntensityGradientEstimation::computePointIntensityGradient, stated once:
// the tail every shape of the gradient ends in (igrad_finish) and the lane-per-list two-pass loop
// (igrad_lane) of Harris6D's k_intensity_gradient (pfx_harris.hip) and of the whole-cloud
// k_igrad_lists (pfx_rift.hip).  What differs between the two is the intensity accessor.
#pragma once
#include "pfx_eigen6.h"
#include "pfx_nblist.h"

namespace pfx {

// s = A00 A01 A02 A11 A12 A22 b0 b1 b2:  x = colPivHouseholderQr(A).solve(b),
// gradient = (Identity - n n^T) x
__device__ __forceinline__ void igrad_finish(const float s[9], const float nv[3], float o[3]) {
  const float A[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]};
  const float bv[3] = {s[6], s[7], s[8]};
  float xs[3];
  colpiv_solve3f(A, bv, xs);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    // The empty asm pins each coefficient in a register: otherwise the compiler folds
    // (0 - p) * x into x * (-p), which is -0 where the reference's x86 code (IEEE: 0 - (+0) = +0)
    // gets +0 -- the sign of zero gradient components
    float m0 = (r == 0 ? 1.0f : 0.0f) - nv[r] * nv[0];
    float m1 = (r == 1 ? 1.0f : 0.0f) - nv[r] * nv[1];
    float m2 = (r == 2 ? 1.0f : 0.0f) - nv[r] * nv[2];
    asm volatile("" : "+v"(m0), "+v"(m1), "+v"(m2));
    o[r] = (m0 * xs[0] + m1 * xs[1]) + m2 * xs[2];
  }
}

// ---- the intensity accessors: raw(q), demeaned(q, mean), and whether a neighbour whose raw
// intensity is not finite is left out of the nine sums ----

// IntensityFieldAccessor<PointXYZRGB>: I = float(299 r + 587 g + 114 b) * 0.001f
__device__ __forceinline__ float rgb_intensity(uint32_t c) {
  const int r = (int)((c >> 16) & 255u), g = (int)((c >> 8) & 255u), b = (int)(c & 255u);
  return (float)(299 * r + 587 * g + 114 * b) * 0.001f;
}
// static_cast<uint8_t>(float) as x86-64 gcc compiles it (cvttss2si, low byte): the demeaned
// intensities are far inside int32, where v_cvt_i32_f32 truncates the same way
__device__ __forceinline__ int u8_trunc(float v) { return ((int32_t)v) & 255; }
// IntensityFieldAccessor::demean (write I - mean back into r, g, b) followed by operator()
__device__ __forceinline__ float rgb_demeaned(uint32_t c, float mean) {
  const float iv = rgb_intensity(c) - mean;
  const int r = u8_trunc(iv * 3.34448160535f), g = u8_trunc(iv * 1.70357751278f), b = u8_trunc(iv * 8.77192982456f);
  return (float)(299 * r + 587 * g + 114 * b) * 0.001f;
}
struct RgbIntensity {  // Harris6D
  static constexpr bool kSkipNonFinite = false;  // (every packed colour has a finite intensity)
  const uint32_t* __restrict__ rgb;
  __device__ __forceinline__ float raw(int32_t q) const { return rgb_intensity(rgb[q]); }
  __device__ __forceinline__ float demeaned(int32_t q, float mean) const { return rgb_demeaned(rgb[q], mean); }
};
struct FloatIntensity {  // IntensityFieldAccessor<PointXYZI>
  static constexpr bool kSkipNonFinite = true;
  const float* __restrict__ si;
  __device__ __forceinline__ float raw(int32_t q) const { return si[q]; }
  __device__ __forceinline__ float demeaned(int32_t q, float mean) const { return si[q] - mean; }
};

// The gradient of the point whose list is ll, i its caller index: two passes over the
// FLANN-ordered neighbours (centroid and mean intensity, then the demeaned 3x3 system).
// False, o untouched, when k < 3 (IntensityGradientEstimation writes NaN there).
template <class Acc>
__device__ __forceinline__ bool igrad_lane(const GridView& g, const LaneList& ll, const Acc& acc, int32_t i,
                                           const float* __restrict__ nx, const float* __restrict__ ny,
                                           const float* __restrict__ nz, float o[3]) {
  const int k = ll.k;
  float cx = 0.f, cy = 0.f, cz = 0.f, mi = 0.f;
  for (int m = 0; m < k; ++m) {
    const int32_t q = ll.idx(g, m);
    cx += g.ux[q];
    cy += g.uy[q];
    cz += g.uz[q];
    mi += acc.raw(q);
  }
  const float rk = 1.0f / (float)k;  // centroid /= float(k): Eigen 3.2 reciprocal
  cx *= rk;
  cy *= rk;
  cz *= rk;
  mi /= (float)k;
  if (k < 3) return false;
  float s[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int m = 0; m < k; ++m) {
    const int32_t q = ll.idx(g, m);
    // a skipped neighbour adds an exact +0 term instead of taking a branch (a sum that starts at
    // +0 is never -0, so adding +0 leaves its bits)
    bool in = true;
    if constexpr (Acc::kSkipNonFinite) in = isfinite(acc.raw(q));
    const float px = g.ux[q] - cx, py = g.uy[q] - cy, pz = g.uz[q] - cz;
    const float iv = acc.demeaned(q, mi);
    s[0] += in ? px * px : 0.f;
    s[1] += in ? px * py : 0.f;
    s[2] += in ? px * pz : 0.f;
    s[3] += in ? py * py : 0.f;
    s[4] += in ? py * pz : 0.f;
    s[5] += in ? pz * pz : 0.f;
    s[6] += in ? px * iv : 0.f;
    s[7] += in ? py * iv : 0.f;
    s[8] += in ? pz * iv : 0.f;
  }
  const float nv[3] = {nx[i], ny[i], nz[i]};
  igrad_finish(s, nv, o);
  return true;
}

}  // namespace pfx
