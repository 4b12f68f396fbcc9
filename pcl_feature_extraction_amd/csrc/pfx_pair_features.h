// pfx_pair_features.h -- pcl::computePairFeatures (features/src/pfh.cpp) and the histogram bin
// maps built on it, bit for bit as PCL 1.7 evaluates them on x86-64, shared by FPFH's SPFH stage
// (pfx_fpfh.hip, 11 bins per feature) and PFH (pfx_pfh.hip, 5 bins per feature), plus
// repeated_add, the closed form of PCL's `histogram[h] += hist_incr` loop.  NB is the number of
// bins per feature (nr_split / nr_bins_f*).
#pragma once
#include "pfx_device_math.h"

namespace pfx {

// PCL 1.7 `acos (fabs (a1)) > acos (fabs (a2))` (double acos, correctly rounded by glibc):
// acos is strictly decreasing and distinct floats >= 2^-26 map to distinct rounded values, so
// the test is |a1| < |a2|; below 2^-26 acos(x) rounds as H + (L - x), pi/2 = H + L.
// |a| > 1 (a normal parallel to the pair's direction, the float quotient rounded past 1): acos is
// NaN and PCL's comparison false -- no swap, whichever side it is on.  (The fast path never bins
// such a pair: |f3| is the larger |angle|, and within 1.5e-6 of 1 its bin map is within tolerance
// of the edge at 0 or NB; a pair whose v_norm is 0 is not binned there either.  This needs
// |n| <= 1 up to rounding: FPFH takes the normals as unit, PFH checks them per pair.)
__device__ __forceinline__ bool acos_greater(float a1, float a2) {
  float x1 = fabsf(a1), x2 = fabsf(a2);
  if (x1 > 1.0f || x2 > 1.0f) return false;
  if (x1 >= 1.4901161e-08f || x2 >= 1.4901161e-08f) return x1 < x2;
  const double H = 1.5707963267948966, L = 6.123233995736766e-17;
  return (H + (L - (double)x1)) > (H + (L - (double)x2));
}

template <int NB>
__device__ __forceinline__ int bin_of(double v) {
  if (!(v == v)) return 0;  // static_cast<int>(NaN) == INT_MIN on x86 -> clamped to 0
  double f = floor(v);
  int h = (f >= 2147483647.0 || f < -2147483648.0) ? (int)0x80000000 : (int)f;
  return h < 0 ? 0 : (h >= NB ? NB - 1 : h);
}

template <int NB>
__device__ __forceinline__ double f1_scaled(double f1) {
  const float d_pi = 1.0f / (2.0f * 3.14159265358979323846f);
  return (double)NB * ((f1 + 3.14159265358979323846) * (double)d_pi);
}

// bin of f1 = glibc's atan2f (PCL: `atan2f (w.dot (n2), n1.dot (n2))`, the fdlibm float routine,
// pfx_device_math.h).  The hardware float atan2 and glibc's are both within a few ulp (< 1e-5 rad)
// of the true value and the bin map is monotone, so when both ends of that interval fall in one
// bin the bin is exact; otherwise (a bin edge within 1e-5 rad) glibc's value is computed.
template <int NB>
__device__ __attribute__((noinline)) int bin_f1_exact(float y, float x) {
  return bin_of<NB>(f1_scaled<NB>((double)atan2f_glibc(y, x)));
}

template <int NB>
__device__ __forceinline__ int bin_f1(float y, float x) {
  const float f = atan2f(y, x);
  if (!(f == f)) return 0;  // NaN argument: the exact value is NaN too
  const int lo = bin_of<NB>(f1_scaled<NB>((double)f - 1e-5)), hi = bin_of<NB>(f1_scaled<NB>((double)f + 1e-5));
  return lo == hi ? lo : bin_f1_exact<NB>(y, x);
}

// pcl::computePairFeatures (features/src/pfh.cpp) + the three bin indices of
// computePointSPFHSignature / computePointPFHSignature; Vector4f maps with w = 0.  Returns
// computePairFeatures' result: false for a degenerate pair (f4 == 0 or v_norm == 0), whose bins
// are those of f = 0 (FPFH bins such a pair, PFH skips it).
template <int NB>
__device__ __forceinline__ bool pair_bins(f3 p1, f3 n1, f3 p2, f3 n2, int& h1, int& h2, int& h3) {
  f3 dp = sub3(p2, p1);
  const float f4 = sqrtf(sqn4(dp));
  const int b_zero_f1 = bin_of<NB>(f1_scaled<NB>(0.0)), b_zero = bin_of<NB>((double)NB * ((0.0 + 1.0) * 0.5));
  if (f4 == 0.0f) { h1 = b_zero_f1; h2 = h3 = b_zero; return false; }
  f3 n1c = n1, n2c = n2;
  const float angle1 = dot4(n1c, dp) / f4;
  const float angle2 = dot4(n2c, dp) / f4;
  float f3o;
  if (acos_greater(angle1, angle2)) {
    n1c = n2; n2c = n1;
    dp = scale3(dp, -1.0f);
    f3o = -angle2;
  } else {
    f3o = angle1;
  }
  f3 v = cross3(dp, n1c);
  const float v_norm = sqrtf(sqn4(v));
  if (v_norm == 0.0f) { h1 = b_zero_f1; h2 = h3 = b_zero; return false; }
  v = scale3(v, 1.0f / v_norm);  // `v /= v_norm`: Eigen 3.2 multiplies by the reciprocal
  const f3 w = cross3(n1c, v);
  const float f2 = dot4(v, n2c);
  h1 = bin_f1<NB>(dot4(w, n2c), dot4(n1c, n2c));
  h2 = bin_of<NB>((double)NB * (((double)f2 + 1.0) * 0.5));
  h3 = bin_of<NB>((double)NB * (((double)f3o + 1.0) * 0.5));
  return true;
}

// ---- fast path of pair_bins ----
// The same float operations as pair_bins up to the first division; then approximate quotients
// (v_rcp / v_rsq), a polynomial atan2 and the bin maps, each feature checked against its bin
// edges with a bound on |approximate - exact-path value| (fractions of a bin: tol).  Any check
// too close to call (an edge within the bound, |angle1| ~ |angle2|, non-finite normals, tiny
// angles) returns false and the caller runs the exact pair_bins.  Bounds (normals |n| <= 1.01):
//   f3 = dot/f4:            |approx - exact| <= 4e-7         used 1e-6
//   f2 = v . n2:            v components within 4e-7, dot    used 4e-6
//   f1 = atan2(w . n2, x):  y within 8e-6 -> 8e-6 / r, atan poly + ops 6e-7, CR rounding 1.2e-7
//                                                            used 1e-6 + 8e-6 / r
// (polynomial: max |atan_poly(a) - atan(a)| = 1.5e-7 on [0, 1] in float Horner, measured).
// The tolerances are feature-space bounds times the slope of the bin map, so they scale with NB.
__device__ __forceinline__ float atan_poly(float a) {
  const float z = a * a;
  float p = -0.00405456405133009f;
  p = p * z + 0.021862948313355446f;
  p = p * z + -0.0559123195707798f;
  p = p * z + 0.0964219719171524f;
  p = p * z + -0.1390862911939621f;
  p = p * z + 0.19946566224098206f;
  p = p * z + -0.33329859375953674f;
  p = p * z + 0.9999993443489075f;
  return p * a;
}

// float evaluation of the bin maps for the fast path: the exact maps are evaluated in double;
// the float forms below differ from them by at most 2.1e-6 bin units at NB = 11, less below (f1:
// pi rounding + the sum and product roundings, x NB/(2 pi); f2/f3: two roundings, x NB/2), so
// kBinMapSlack is added to each feature's tolerance -- no double-precision work per pair.
constexpr float kBinMapSlack = 3e-6f;

template <int NB>
__device__ __forceinline__ bool bin_fast_f(float v, float tol, int& h) {
  const float m = floorf(v);
  const float fr = v - m;  // exact (|v| < 2^23)
  if (!(fr > tol && fr < 1.0f - tol)) return false;  // also rejects NaN
  const int b = (int)m;
  h = b < 0 ? 0 : (b >= NB ? NB - 1 : b);
  return true;
}

// true: (h1, h2, h3) are pair_bins' bins (a pair with f4 == 0 gets the bins of f = 0, as there;
// a caller that skips invalid pairs tests p1 == p2 itself); false: run pair_bins
template <int NB>
__device__ __forceinline__ bool pair_bins_fast(f3 p1, f3 n1, f3 p2, f3 n2, int& h1, int& h2, int& h3) {
  f3 dp = sub3(p2, p1);
  const float s4 = sqn4(dp);
  if (s4 == 0.0f) {  // f4 == 0 in pair_bins
    h1 = bin_of<NB>(f1_scaled<NB>(0.0));
    h2 = h3 = bin_of<NB>((double)NB * ((0.0 + 1.0) * 0.5));
    return true;
  }
  if (!(isfinite(n1.x) && isfinite(n1.y) && isfinite(n1.z) && isfinite(n2.x) && isfinite(n2.y) && isfinite(n2.z)))
    return false;
  const float d1 = dot4(n1, dp), d2 = dot4(n2, dp);
  const float ad1 = fabsf(d1), ad2 = fabsf(d2);
  const float rf4 = __builtin_amdgcn_rsqf(s4);  // ~ 1 / f4
  if (fmaxf(ad1, ad2) * rf4 < 2e-8f) return false;  // acos_greater's tiny-angle branch
  bool swap;
  if (ad1 < ad2 * (1.0f - 4e-7f)) swap = true;        // |angle1| < |angle2|
  else if (ad1 > ad2 * (1.0f + 4e-7f)) swap = false;
  else return false;
  f3 n1c = n1, n2c = n2;
  float f3a;
  if (swap) {
    n1c = n2; n2c = n1;
    dp = scale3(dp, -1.0f);
    f3a = -d2 * rf4;
  } else {
    f3a = d1 * rf4;
  }
  const f3 v = cross3(dp, n1c);
  const float sv = sqn4(v);
  // (v_norm == 0 in pair_bins: the chosen normal is parallel to dp, so an |angle| may have rounded
  // past 1 and the swap above may not be PCL's -- the exact path decides)
  if (sv == 0.0f) return false;
  const f3 vh = scale3(v, __builtin_amdgcn_rsqf(sv));
  const f3 w = cross3(n1c, vh);
  const float f2a = dot4(vh, n2c);
  const float y = dot4(w, n2c), x = dot4(n1c, n2c);
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  if (!(mx > 1e-20f)) return false;
  float t = atan_poly(mn * __builtin_amdgcn_rcpf(mx));
  if (ay > ax) t = 1.57079637f - t;
  if (x < 0.0f) t = 3.14159274f - t;
  const float f1a = y < 0.0f ? -t : t;
  const float d_pi = 1.0f / (2.0f * 3.14159265358979323846f);
  const float tol1 = (1e-6f + 8e-6f * __builtin_amdgcn_rcpf(mx)) * (1.01f * (float)NB * d_pi) + kBinMapSlack;
  return bin_fast_f<NB>((f1a + 3.14159265358979323846f) * ((float)NB * d_pi), tol1, h1) &&
         bin_fast_f<NB>((f2a + 1.0f) * (0.5f * NB), 4e-6f * 0.5f * NB + kBinMapSlack, h2) &&
         bin_fast_f<NB>((f3a + 1.0f) * (0.5f * NB), 1e-6f * 0.5f * NB + kBinMapSlack, h3);
}

// c sequential float additions of incr starting from 0 (PCL's hist_incr loop), in O(binades):
// inside a binade of s every step adds the same multiple of ulp(s) (incr's position between two
// grid points does not depend on s; an exact half-way case needs one step first, see below);
// steps that would reach the next binade are taken one by one.
__device__ __forceinline__ float repeated_add(float incr, int c) {
  float s = 0.0f;
  int rem = c;
  while (rem > 0) {
    s = s + incr;
    --rem;
    if (rem == 0 || !(s > 0.0f) || !isfinite(s)) break;
    const int e = ilogbf(s);
    const double ulp = ldexp(1.0, e - 23), top = ldexp(1.0, e + 1);
    const double t = (double)incr / ulp;
    if (t - floor(t) == 0.5) {
      // tie: s + incr rounds to even, so one more step leaves s an even multiple of ulp, and from
      // there every step inside this binade adds the same amount (checked against the plain loop
      // for 100 / (k - 1), k < 6000, and random increments)
      s = s + incr;
      --rem;
      if (rem == 0 || ilogbf(s) != e) continue;
    }
    const double delta = (double)(s + incr) - (double)s;
    if (delta <= 0.0) {  // s no longer changes
      rem = 0;
      break;
    }
    int64_t n = (int64_t)ceil((top - (double)s) / delta) - 1;  // s + n delta < top
    if (n > rem) n = rem;
    if (n > 0) {
      s = (float)((double)s + (double)n * delta);
      rem -= (int)n;
    }
  }
  for (; rem > 0; --rem) s = s + incr;  // (after a break on a non-finite or zero sum)
  return s;
}

}  // namespace pfx
