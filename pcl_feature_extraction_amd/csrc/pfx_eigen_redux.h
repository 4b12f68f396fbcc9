// pfx_eigen_redux.h -- Eigen 3.2's `sum()` of a dynamic-size double array (Redux.h, redux_impl<
// scalar_sum_op, Derived, LinearVectorizedTraversal, NoUnrolling>, SSE2: packets of two doubles,
// storage 16-byte aligned so alignedStart = 0), restated operation for operation.  Plain C++ for
// the host restatement (tests/cpp/spin_ref.cpp) and the device (pfx_spin.hip) alike; DESIGN.md
// "Spin images: the contract" has the rule in words.
//
//   S <  2: m[0] (S == 1), sequential.
//   S >= 2: packet_res0 = (m[0], m[1]); when S >= 4 a second accumulator packet_res1 = (m[2], m[3])
//           and both advance by 4 up to 4 * (S / 4): four running sums over the indices = 0, 1, 2, 3
//           (mod 4); then packet_res0 += packet_res1 lane-wise: (s0 + s2, s1 + s3); then, when
//           S mod 4 >= 2, the next pair is added lane-wise; predux adds the two lanes; the last odd
//           element is added sequentially.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PFX_HD __host__ __device__ inline
#else
#define PFX_HD inline
#endif

namespace pfx {

// running sum number `lane` (0..3) of the unrolled loop: m[lane] + m[lane + 4] + ... below
// 4 * (S / 4).  Requires S >= 4.
PFX_HD double eigen_redux_lane(const double* m, int S, int lane) {
  const int end2 = (S / 4) * 4;
  double s = m[lane];
  for (int i = lane + 4; i < end2; i += 4) s = s + m[i];
  return s;
}

// the four running sums combined, the pair and the odd element of the tail.  Requires S >= 4.
PFX_HD double eigen_redux_finish(double s0, double s1, double s2, double s3, const double* m, int S) {
  const int end2 = (S / 4) * 4, end = (S / 2) * 2;
  double l0 = s0 + s2, l1 = s1 + s3;
  if (end > end2) {
    l0 = l0 + m[end2];
    l1 = l1 + m[end2 + 1];
  }
  double res = l0 + l1;
  for (int i = end; i < S; ++i) res = res + m[i];
  return res;
}

PFX_HD double eigen_redux_sum(const double* m, int S) {
  if (S < 4) {  // at most one packet: no second accumulator
    if (S <= 0) return 0.0;
    double res = S >= 2 ? m[0] + m[1] : m[0];
    for (int i = S >= 2 ? 2 : 1; i < S; ++i) res = res + m[i];
    return res;
  }
  return eigen_redux_finish(eigen_redux_lane(m, S, 0), eigen_redux_lane(m, S, 1), eigen_redux_lane(m, S, 2),
                            eigen_redux_lane(m, S, 3), m, S);
}

// ---- floats (SSE: packets of four, pfx_rift.hip and tests/cpp/rift_ref.cpp) ----
//   S <  4: no packet: m[0], then the rest sequentially.
//   S >= 4: packet_res0 = m[0..3]; when S >= 8 a second accumulator packet_res1 = m[4..7] and both
//           advance by 8 up to 8 * (S / 8): eight running sums over the indices mod 8; then
//           packet_res0 += packet_res1 lane-wise; then, when 4 * (S / 4) > 8 * (S / 8), the next
//           packet is added lane-wise; predux = (a0 + a2) + (a1 + a3); the scalar tail is added
//           left to right.
PFX_HD float eigen_redux_sum_f(const float* m, int S) {
  if (S <= 0) return 0.0f;
  if (S < 4) {
    float res = m[0];
    for (int i = 1; i < S; ++i) res = res + m[i];
    return res;
  }
  const int end4 = (S / 4) * 4, end8 = (S / 8) * 8;
  float a[4] = {m[0], m[1], m[2], m[3]};
  if (end8) {
    float b[4] = {m[4], m[5], m[6], m[7]};
    for (int i = 8; i < end8; i += 8)
      for (int l = 0; l < 4; ++l) {
        a[l] = a[l] + m[i + l];
        b[l] = b[l] + m[i + 4 + l];
      }
    for (int l = 0; l < 4; ++l) a[l] = a[l] + b[l];
    if (end4 > end8)
      for (int l = 0; l < 4; ++l) a[l] = a[l] + m[end8 + l];
  }
  float res = (a[0] + a[2]) + (a[1] + a[3]);
  for (int i = end4; i < S; ++i) res = res + m[i];
  return res;
}

}  // namespace pfx
