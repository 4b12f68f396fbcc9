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

}  // namespace pfx
