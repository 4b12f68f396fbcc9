// pfx_expf.h -- one float exponential for host and device (DESIGN.md "Intensity spin: the contract").
//
// pfx_expf(x) is the contract's expf: the kernel (pfx_intensity_spin.hip) and the CPU restatement
// (tests/cpp/intensity_spin_ref.cpp) both compile this text, hipcc for gfx950 and for the host, g++
// for the restatement.  It uses IEEE double + - *, integer operations and bit casts, then one
// conversion to float; it calls no libm.  Without FMA contraction (-ffp-contract=off, which every
// build of it sets) the three compilers have no freedom left: the bits agree by construction.
//
// The design follows the table-driven expf published with glibc 2.27: in double,
//   z = x * 32/ln2,  k = round(z) (by adding and subtracting 1.5 * 2^52),  r = z - k in [-1/2, 1/2],
//   e^x = 2^(k/32) * 2^(r/32),  2^(k/32) = 2^(k div 32) * T[k mod 32],
//   2^(r/32) = 1 + c1 r + c2 r^2 + c3 r^3   (Taylor: c_j = (ln2/32)^j / j!; the first term left out
//   is below (ln2/64)^4 / 24 = 5.7e-10, a hundredth of half a float ulp),
// with the constants below correctly rounded from 50 decimal digits by scripts/pfx_expf_table.py.
// The result is within 0.51 ulp of e^x: faithfully rounded, so never more than 1 ulp from another
// faithfully rounded expf (tests/test_pfx_expf.py counts the 1-ulp differences from the host libm's).
//
// Edges: NaN -> NaN (0x7fc00000); x > 89 -> +infinity, and between 88.72284 and 89 the conversion
// overflows to it; x < -104 -> +0, and from about -103.98 (e^x <= 2^-150) the conversion rounds to
// it; results in the float denormal range come from that one conversion; +-0 -> 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PFX_EXPF_HD __host__ __device__
#else
#define PFX_EXPF_HD
#endif

namespace pfx {

PFX_EXPF_HD inline double expf_from_bits(uint64_t u) {
  double d;
  __builtin_memcpy(&d, &u, sizeof(d));
  return d;
}

PFX_EXPF_HD inline float pfx_expf(float x) {
  // 2^(i/32), i = 0 .. 31, as bits less i << 47 (adding k << 47 then sets the exponent of k div 32)
  const uint64_t T[32] = {
      0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
      0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
      0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
      0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
      0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
      0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
      0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
      0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull,
  };
  const double inv_ln2_n = expf_from_bits(0x40471547652b82feull);  // 32 / ln2
  const double c1 = expf_from_bits(0x3f962e42fefa39efull);         // ln2 / 32
  const double c2 = expf_from_bits(0x3f2ebfbdff82c58full);         // (ln2 / 32)^2 / 2
  const double c3 = expf_from_bits(0x3ebc6b08d704a0c0ull);         // (ln2 / 32)^3 / 6
  const double shift = expf_from_bits(0x4338000000000000ull);      // 1.5 * 2^52
  if (!(x == x)) {
    const uint32_t qnan = 0x7fc00000u;
    float f;
    __builtin_memcpy(&f, &qnan, sizeof(f));
    return f;
  }
  if (x > 89.0f) {
    const uint32_t inf = 0x7f800000u;
    float f;
    __builtin_memcpy(&f, &inf, sizeof(f));
    return f;
  }
  if (x < -104.0f) return 0.0f;
  const double z = inv_ln2_n * (double)x;
  double kd = z + shift;  // the integer nearest to z in the low bits of the mantissa
  uint64_t ki;
  __builtin_memcpy(&ki, &kd, sizeof(ki));
  kd = kd - shift;
  const double r = z - kd;
  const double s = expf_from_bits(T[ki & 31] + (ki << 47));  // 2^(k/32)
  const double r2 = r * r;
  const double p = (c3 * r + c2) * r2 + (c1 * r + 1.0);
  return (float)(p * s);
}

}  // namespace pfx
