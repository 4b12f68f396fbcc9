// shape_context_ref.cpp -- TEST INFRASTRUCTURE ONLY: the CPU restatement of the contract of
// pfx_shape_context.hip as DESIGN.md states it ("Shape contexts: the contract"):
//   sc_ref  PCL 1.7 ShapeContext3DEstimation (features/impl/3dsc.hpp) when `frames` is null,
//           UniqueShapeContext (features/impl/usc.hpp) with the caller's frames otherwise.
// Built by tests/shape_context_ref.py into a shared object; never linked into libpfx.  Plain
// sequential float arithmetic in FLANN neighbour order on the oracle's NeighborGrid and its Eigen 3.2
// helpers (oracle/or_common.h).  The generator is written out here (MT19937 with init_genrand, read
// through boost's uniform_01<float>), apart from the library's.  Every NaN is written as 0x7fc00000,
// as the kernels do.
#include <cfloat>
#include <cstring>

#include <algorithm>
#include <cmath>

#include "or_common.h"

using namespace orc;

namespace {

const int kAz = 12, kEl = 11, kRad = 15, kLen = 1980;

inline float canon_nan(float v) {
  if (v == v) return v;
  const uint32_t u = 0x7fc00000u;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

inline float rad2deg(float a) { return a * 57.29578f; }
inline float deg2rad(float a) { return a * 0.017453293f; }
inline bool equal(float a, float b) { return fabsf(a - b) < FLT_EPSILON; }

struct Tables {
  float radii[kRad + 1], theta_div[kEl + 1], phi_div[kAz + 1], lut[kEl * kRad];
};

void tables(double R, double rmin, Tables& T) {
  for (int j = 0; j <= kRad; ++j)
    T.radii[j] = (float)exp(log(rmin) + (double)((float)j / 15.0f) * log(R / rmin));
  for (int k = 0; k <= kEl; ++k) T.theta_div[k] = (float)k * (180.0f / 11.0f);
  for (int l = 0; l <= kAz; ++l) T.phi_div[l] = (float)l * 30.0f;
  const float integr_phi = deg2rad(T.phi_div[1]) - deg2rad(T.phi_div[0]);
  for (int k = 0; k < kEl; ++k) {
    const float integr_theta = cosf(deg2rad(T.theta_div[k])) - cosf(deg2rad(T.theta_div[k + 1]));
    for (int j = 0; j < kRad; ++j) {
      const float integr_r =
          T.radii[j + 1] * T.radii[j + 1] * T.radii[j + 1] - T.radii[j] * T.radii[j] * T.radii[j];
      const float V = integr_phi * integr_theta * integr_r;
      T.lut[k * kRad + j] = 1.0f / powf(V, 1.0f / 3.0f);
    }
  }
}

// MT19937 (Matsumoto and Nishimura's mt19937ar.c: init_genrand, genrand_int32)
struct Mt {
  uint32_t mt[624];
  int i;
  explicit Mt(uint32_t s) {
    mt[0] = s;
    for (i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
  }
  uint32_t next() {
    if (i >= 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % 624] & 0x7fffffffu);
        mt[k] = mt[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      i = 0;
    }
    uint32_t y = mt[i++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
};

// uniform_01<float>'s map of one raw output; false: not below 1, draw again
inline bool map01(uint32_t u, float& v) {
  v = (float)u * (1.0f / 4294967296.0f);
  return v < 1.0f;
}

}  // namespace

extern "C" {

void sc_ref_tables(double R, double rmin, float* radii, float* theta_div, float* phi_div, float* lut) {
  Tables T;
  tables(R, rmin, T);
  std::memcpy(radii, T.radii, sizeof(T.radii));
  std::memcpy(theta_div, T.theta_div, sizeof(T.theta_div));
  std::memcpy(phi_div, T.phi_div, sizeof(T.phi_div));
  std::memcpy(lut, T.lut, sizeof(T.lut));
}

void sc_ref_mt_raw(uint32_t seed, i64 n, uint32_t* out) {
  Mt e(seed);
  for (i64 i = 0; i < n; ++i) out[i] = e.next();
}

// the floats that n_raw raw outputs give; returns their number
i64 sc_ref_map01(const uint32_t* raw, i64 n_raw, float* out) {
  i64 m = 0;
  for (i64 i = 0; i < n_raw; ++i) {
    float v;
    if (map01(raw[i], v)) out[m++] = v;
  }
  return m;
}

void sc_ref_uniform01(uint32_t seed, i64 skip, i64 n, float* out) {
  Mt e(seed);
  for (i64 i = -skip; i < n; ++i) {
    float v;
    while (!map01(e.next(), v)) {
    }
    if (i >= 0) out[i] = v;
  }
}

// desc: nq x 1980, rf: nq x 9.  frames null: the 3DSC (snx / sny / snz, and rnd: 3 nq floats, the
// t-th drawing row takes rnd[3t .. 3t + 2]); else USC.  reversed != 0 walks every neighbourhood
// from its last neighbour to its first (the frame still comes from the nearest one).  stats
// (nullable, 6): sum of k, max k, drawing rows, neighbours skipped as too close, support points,
// rows with more than cap_small neighbours.
void sc_ref(const float* sx, const float* sy, const float* sz, const float* snx, const float* sny, const float* snz,
            i64 ns, const float* qx, const float* qy, const float* qz, const float* frames, const float* rnd,
            i64 nq, double R, double rmin, double rho, int reversed, int cap_small, float* desc, float* rf,
            i64* stats) {
  Tables T;
  tables(R, rmin, T);
  NeighborGrid g, gd;
  g.build(sx, sy, sz, ns, R);
  gd.build(sx, sy, sz, ns, rho);
  std::vector<int> dens((size_t)ns, 0);  // 0: not counted yet (a counted density is >= 1)
  std::vector<int> idx, idx2;
  std::vector<float> d2, d22;
  i64 nb = 0, kmax = 0, draws = 0, skipped = 0, support = 0, queued = 0;
  for (i64 q = 0; q < nq; ++q) {
    float* o = desc + q * kLen;
    float* f = rf + q * 9;
    const V3 org = v3(qx[q], qy[q], qz[q]);
    const bool finite_q = std::isfinite(org.x) && std::isfinite(org.y) && std::isfinite(org.z);
    g.radius(org.x, org.y, org.z, R, idx, d2);  // empty for a non-finite query
    const int k = (int)idx.size();
    // the density of every support point, once
    for (int i = 0; i < k; ++i) {
      const int p = idx[(size_t)i];
      if (dens[(size_t)p]) continue;
      gd.radius(sx[p], sy[p], sz[p], rho, idx2, d22);
      dens[(size_t)p] = (int)idx2.size();
      ++support;
    }
    bool dead = !finite_q;
    if (frames && finite_q)
      dead = !std::isfinite(frames[9 * q]) || !std::isfinite(frames[9 * q + 3]) || !std::isfinite(frames[9 * q + 6]);
    if (dead) {
      for (int i = 0; i < kLen; ++i) o[i] = canon_nan(NAN);
      for (int i = 0; i < 9; ++i) f[i] = 0.0f;
      continue;
    }
    nb += k;
    kmax = std::max<i64>(kmax, k);
    if (k > cap_small) ++queued;
    if (k == 0) {
      for (int i = 0; i < kLen; ++i) o[i] = frames ? 0.0f : canon_nan(NAN);
      for (int i = 0; i < 9; ++i) f[i] = frames ? canon_nan(frames[9 * q + i]) : 0.0f;
      continue;
    }
    V3 x, n;
    if (frames) {
      x = v3(frames[9 * q], frames[9 * q + 1], frames[9 * q + 2]);
      n = v3(frames[9 * q + 6], frames[9 * q + 7], frames[9 * q + 8]);
      for (int i = 0; i < 9; ++i) f[i] = canon_nan(frames[9 * q + i]);
    } else {
      const int p0 = idx[0];
      n = v3(snx[p0], sny[p0], snz[p0]);
      x = v3(rnd[3 * draws], rnd[3 * draws + 1], rnd[3 * draws + 2]);
      ++draws;
      if (!equal(n.z, 0.0f)) x.z = -(n.x * x.x + n.y * x.y) / n.z;
      else if (!equal(n.y, 0.0f)) x.y = -(n.x * x.x + n.z * x.z) / n.y;
      else if (!equal(n.x, 0.0f)) x.x = -(n.y * x.y + n.z * x.z) / n.x;
      x = normalize3(x);
      const V3 y = cross(n, x);
      const float fr[9] = {x.x, x.y, x.z, y.x, y.y, y.z, n.x, n.y, n.z};
      for (int i = 0; i < 9; ++i) f[i] = canon_nan(fr[i]);
    }
    for (int i = 0; i < kLen; ++i) o[i] = 0.0f;
    for (int it = 0; it < k; ++it) {
      const int i = reversed ? k - 1 - it : it;
      const int pi = idx[(size_t)i];
      if (equal(d2[(size_t)i], 0.0f)) {
        ++skipped;
        continue;
      }
      const float r = sqrtf(d2[(size_t)i]);
      const V3 p = v3(sx[pi], sy[pi], sz[pi]);
      const V3 po = sub(p, org);
      const float lambda = dot3(n, po);
      V3 proj = sub(p, mul(n, lambda));
      proj = sub(proj, org);
      proj = normalize3(proj);
      const V3 c = cross(x, proj);
      float phi = rad2deg(atan2f_glibc(sqrtf(sqn3(c)), dot3(x, proj)));
      if (dot3(c, n) < 0.0f) phi = 360.0f - phi;
      const V3 no = normalize3(sub(p, org));
      const float t = dot3(n, no);
      const float theta = rad2deg(acosf_glibc(std::min(1.0f, std::max(-1.0f, t))));
      int j = 0, kk = 0, l = 0;
      for (int rad = 1; rad <= kRad; ++rad)
        if (r <= T.radii[rad]) { j = rad - 1; break; }
      for (int ang = 1; ang <= kEl; ++ang)
        if (theta <= T.theta_div[ang]) { kk = ang - 1; break; }
      for (int ang = 1; ang <= kAz; ++ang)
        if (phi <= T.phi_div[ang]) { l = ang - 1; break; }
      const float w = (1.0f / (float)dens[(size_t)pi]) * T.lut[kk * kRad + j];
      o[l * (kEl * kRad) + kk * kRad + j] += w;
    }
  }
  if (stats) {
    stats[0] = nb;
    stats[1] = kmax;
    stats[2] = draws;
    stats[3] = skipped;
    stats[4] = support;
    stats[5] = queued;
  }
}

}  // extern "C"
