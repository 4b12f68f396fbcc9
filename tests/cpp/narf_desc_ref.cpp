// narf_desc_ref.cpp -- TEST INFRASTRUCTURE ONLY.  The CPU restatement of DESIGN.md "NARF
// descriptors: the contract" (PCL 1.7 Narf::extractFromRangeImage / extractDescriptor /
// getRotations and RangeImage::getNormalBasedUprightTransformation /
// getInterpolatedSurfaceProjection, as the project states them; parity with PCL itself is
// unpinned), and of Tools::getIndices (tools.h:91-102).  Written from that text on the oracle's
// arithmetic helpers (oracle/or_common.h: the Eigen 3.2 reduction order, eigen33_full, the glibc and
// correctly rounded math twins).  Built by tests/narf_desc_ref.py into a shared library; float32
// left to right, no FMA contraction.  The range image is an input (width x height x 4 floats as
// the oracle's orc_range_image_planar writes them), so a test may also write one by hand.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include <algorithm>
#include <vector>

#include "or_common.h"

using namespace orc;

namespace {

const float kInf = std::numeric_limits<float>::infinity();
const float kPi = (float)M_PI;

inline float deg2rad(float a) { return a * 0.017453293f; }

// lrint (round half even); a NaN and what lies beyond +-2^30 (undefined in PCL) saturate
inline int iround(float v) {
  if (!(v == v)) return -(1 << 30);
  if (v >= 1073741824.0f) return 1 << 30;
  if (v <= -1073741824.0f) return -(1 << 30);
  return (int)std::lrint(v);
}

inline float normAngle(float a) {
  return a >= 0 ? std::fmod(a + kPi, 2.0f * kPi) - kPi : -(std::fmod(kPi - a, 2.0f * kPi) - kPi);
}

struct Aff {  // row-major 3x4 [R | t]
  float m[12];
  V3 apply(V3 p) const {  // ((r0 x + r1 y) + r2 z) + t
    return v3(m[3] + (m[0] * p.x + m[1] * p.y + m[2] * p.z), m[7] + (m[4] * p.x + m[5] * p.y + m[6] * p.z),
              m[11] + (m[8] * p.x + m[9] * p.y + m[10] * p.z));
  }
  Aff inverse() const {  // Eigen::Isometry: R^T, -(R^T t)
    Aff r;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) r.m[i * 4 + j] = m[j * 4 + i];
      r.m[i * 4 + 3] = -((m[0 * 4 + i] * m[3] + m[1 * 4 + i] * m[7]) + m[2 * 4 + i] * m[11]);
    }
    return r;
  }
};

struct Image {
  int w, h;
  float cx, cy, fx, fy;
  Aff to_world, to_ri;
  const float* P;  // w * h * 4: x, y, z, range
  bool inImage(int x, int y) const { return x >= 0 && x < w && y >= 0 && y < h; }
  float range(int x, int y) const { return P[((size_t)y * w + x) * 4 + 3]; }
  bool isValid(int x, int y) const { return inImage(x, y) && std::isfinite(range(x, y)); }
  V3 point(int x, int y) const {
    const float* p = P + ((size_t)y * w + x) * 4;
    return v3(p[0], p[1], p[2]);
  }
  V3 sensorPos() const { return v3(to_world.m[3], to_world.m[7], to_world.m[11]); }
  void imagePoint(V3 pt, float& ix, float& iy, float& rng) const {  // RangeImagePlanar::getImagePoint
    V3 t = to_ri.apply(pt);
    if (t.z <= 0) { ix = iy = rng = -1.0f; return; }
    rng = std::sqrt(sqn3(t));
    ix = cx + fx * t.x / t.z - 0.0f;
    iy = cy + fy * t.y / t.z - 0.0f;
  }
  float rangeDifference(V3 q) const {  // RangeImage::getRangeDifference
    float ix, iy, rng;
    imagePoint(q, ix, iy, rng);
    const int x = iround(ix), y = iround(iy);
    if (!inImage(x, y)) return -kInf;
    const float r = range(x, y);
    if (std::isinf(r)) return r > 0.0f ? kInf : -kInf;
    return r - rng;
  }
};

void makeImage(int w, int h, float cx, float cy, float fx, float fy, const float* pose, int frame, const float* P,
               Image& I) {
  I.w = w; I.h = h; I.cx = cx; I.cy = cy; I.fx = fx; I.fy = fy; I.P = P;
  float F[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  if (frame == 1) {
    float L[4][4] = {{0, 0, 1, 0}, {-1, 0, 0, 0}, {0, -1, 0, 0}, {0, 0, 0, 1}};
    std::memcpy(F, L, sizeof(F));
  }
  float W[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      W[i][j] = ((pose[i * 4 + 0] * F[0][j] + pose[i * 4 + 1] * F[1][j]) + pose[i * 4 + 2] * F[2][j]) +
                pose[i * 4 + 3] * F[3][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) I.to_world.m[i * 4 + j] = W[i][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) I.to_ri.m[i * 4 + j] = W[j][i];
  for (int i = 0; i < 3; ++i)
    I.to_ri.m[i * 4 + 3] = -(I.to_ri.m[i * 4 + 0] * W[0][3] + I.to_ri.m[i * 4 + 1] * W[1][3] + I.to_ri.m[i * 4 + 2] * W[2][3]);
}

// the position of ring step i (after its move) of the ring of `radius` about (cx, cy)
inline void ringWalk(int radius, int i, int& x, int& y) {
  if (i <= 2 * radius) ++x; else if (i <= 4 * radius) ++y; else if (i <= 6 * radius) --x; else --y;
}

struct VecAvg {  // VectorAverage3f with add (sample, weight)
  int n = 0;
  float acc_w = 0.0f;
  V3 mean = {0, 0, 0};
  float cov[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  void add(V3 s, float w) {
    if (w == 0.0f) return;
    ++n;
    acc_w += w;
    const float alpha = w / acc_w;
    const V3 diff = sub(s, mean);
    const float d[3] = {diff.x, diff.y, diff.z};
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) cov[i][j] = (1.0f - alpha) * (cov[i][j] + alpha * d[i] * d[j]);
    mean = orc::add(mean, v3(alpha * diff.x, alpha * diff.y, alpha * diff.z));
  }
  V3 smallest() const {
    float m[3][3], ev[3];
    V3 evec[3];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) m[i][j] = (j >= i) ? cov[i][j] : cov[j][i];
    eigen33_full(m, evec, ev);
    return evec[0];
  }
};

inline float sqDist(V3 a, V3 b) {  // pcl::squaredEuclideanDistance: diff = b - a, left to right
  const float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return dx * dx + dy * dy + dz * dz;
}

// RangeImage::getSurfaceInformation as the keypoint path states it (oracle/or_narf.cpp
// surfaceInformation): radius 2, step 1, the 15 closest
bool surfaceInformation(const Image& I, int x, int y, V3 point, V3& normal, V3& mean) {
  const int radius = 2, step = 1, no_of_closest = 15;
  struct ND { float d; V3 p; };
  ND nb[25];
  int cnt = 0;
  for (int y2 = y - radius; y2 <= y + radius; y2 += step)
    for (int x2 = x - radius; x2 <= x + radius; x2 += step) {
      if (!I.isValid(x2, y2)) continue;
      nb[cnt].p = I.point(x2, y2);
      nb[cnt].d = sqDist(point, nb[cnt].p);
      ++cnt;
    }
  if (cnt == 0) return false;
  for (int i = 1; i < cnt; ++i) {  // insertion sort (stable), by distance
    ND v = nb[i];
    int j = i;
    while (j > 0 && v.d < nb[j - 1].d) { nb[j] = nb[j - 1]; --j; }
    nb[j] = v;
  }
  const int k = std::min(cnt, no_of_closest);
  const float max_d2 = nb[k - 1].d * 4.0f;
  VecAvg va;
  for (int i = 0; i < cnt; ++i) {
    if (nb[i].d > max_d2) break;
    va.add(nb[i].p, 1.0f);
  }
  if (va.n < 3) return false;
  normal = va.smallest();
  const V3 view = normalized3(sub(I.sensorPos(), point));
  if (dot3(normal, view) < 0.0f) normal = mul(normal, -1.0f);
  mean = va.mean;
  return true;
}

struct Stats { int64_t rows = 0, invalid = 0, pose_failed = 0, fallback = 0, ring_max = 0, background = 0; };

// step 2; 0: a pose, 1: a pose from the fallback normal, 2: failed
int uprightPose(const Image& I, V3 P, float max_dist, Aff& pose, Stats& st) {
  float ix, iy, rng;
  I.imagePoint(P, ix, iy, rng);
  const int cx = iround(ix), cy = iround(iy);
  const float max_d2 = max_dist * max_dist, max_dist_rec = 1.0f / max_dist;
  VecAvg va;
  bool still = true;
  for (int radius = 1; still; ++radius) {
    st.ring_max = std::max<int64_t>(st.ring_max, radius);
    int x = cx - radius - 1, y = cy - radius;
    still = false;
    for (int i = 0; i < 8 * radius; ++i) {
      ringWalk(radius, i, x, y);
      if (!I.isValid(x, y)) continue;
      const V3 q = I.point(x, y);
      const float d2 = sqn3(sub(q, P));
      if (d2 > max_d2) continue;
      still = true;
      va.add(q, std::sqrt(d2) * max_dist_rec);
    }
  }
  V3 normal, on_plane;
  int how = 0;
  if (va.n > 10) {
    normal = va.smallest();
    if (dot3(normal, normalized3(sub(va.mean, I.sensorPos()))) < 0.0f) normal = mul(normal, -1.0f);
    const float s = dot3(normal, va.mean) - dot3(normal, P);
    on_plane = v3(s * normal.x + P.x, s * normal.y + P.y, s * normal.z + P.z);
  } else {
    V3 mean;
    if (!surfaceInformation(I, cx, cy, P, normal, mean)) return 2;
    const float s = dot3(normal, mean) - dot3(normal, P);
    on_plane = v3(s * normal.x + P.x, s * normal.y + P.y, s * normal.z + P.z);
    how = 1;
  }
  const V3 t0 = normalized3(cross(v3(0.0f, 1.0f, 0.0f), normal));
  const V3 t1 = normalized3(cross(normal, t0));
  const V3 t2 = normalized3(normal);
  const V3 rows[3] = {t0, t1, t2};
  for (int i = 0; i < 3; ++i) {
    pose.m[i * 4 + 0] = rows[i].x;
    pose.m[i * 4 + 1] = rows[i].y;
    pose.m[i * 4 + 2] = rows[i].z;
    pose.m[i * 4 + 3] = -mv3(rows[i], on_plane);
  }
  for (float v : pose.m)  // a normal along (0, 1, 0), an overflow: no frame (undefined in PCL)
    if (!std::isfinite(v)) return 2;
  return how;
}

// steps 3 and 4: the 10 x 10 patch, -inf unseen, +inf background
void surfacePatch(const Image& I, const Aff& pose, float support, float* patch, Stats& st) {
  const float max_dist = 0.5f * support, cell = support / 10.0f;
  const float w2c = 1.0f / cell, w2c_off = 0.5f * 10 - 0.5f, c2w_off = -max_dist + 0.5f * cell;
  const Aff inv = pose.inverse();
  const V3 position = v3(inv.m[3], inv.m[7], inv.m[11]);
  float ix, iy, rng;
  I.imagePoint(position, ix, iy, rng);
  const int mx = iround(ix), my = iround(iy);
  for (int i = 0; i < 100; ++i) patch[i] = -kInf;
  bool still = true;
  for (int radius = 0; still; ++radius) {
    st.ring_max = std::max<int64_t>(st.ring_max, radius);
    int x = mx - radius - 1, y = my - radius;
    still = radius < 2;
    for (int i = 0; i < 8 * radius || (radius == 0 && i == 0); ++i) {
      ringWalk(radius, i, x, y);
      if (!I.isValid(x, y) || !I.isValid(x + 1, y + 1)) continue;
      const V3 p1 = pose.apply(I.point(x, y)), p2 = pose.apply(I.point(x + 1, y + 1));
      if (std::fabs(p1.z) > max_dist || std::fabs(p2.z) > max_dist) continue;
      const float c1x = w2c * p1.x + w2c_off, c1y = w2c * p1.y + w2c_off;
      const float c2x = w2c * p2.x + w2c_off, c2y = w2c * p2.y + w2c_off;
      for (int tri = 0; tri < 2; ++tri) {
        const int x3 = tri == 0 ? x : x + 1, y3 = tri == 0 ? y + 1 : y;
        if (!I.isValid(x3, y3)) continue;
        const V3 p3 = pose.apply(I.point(x3, y3));
        if (std::fabs(p3.z) > max_dist) continue;
        if ((p1.x < -max_dist && p2.x < -max_dist && p3.x < -max_dist) ||
            (p1.x > max_dist && p2.x > max_dist && p3.x > max_dist) ||
            (p1.y < -max_dist && p2.y < -max_dist && p3.y < -max_dist) ||
            (p1.y > max_dist && p2.y > max_dist && p3.y > max_dist))
          continue;
        still = true;
        const float c3x = w2c * p3.x + w2c_off, c3y = w2c * p3.y + w2c_off;
        const int x_lo = std::max(0, iround(std::ceil(std::min(c1x, std::min(c2x, c3x)))));
        const int x_hi = std::min(9, iround(std::floor(std::max(c1x, std::max(c2x, c3x)))));
        const int y_lo = std::max(0, iround(std::ceil(std::min(c1y, std::min(c2y, c3y)))));
        const int y_hi = std::min(9, iround(std::floor(std::max(c1y, std::max(c2y, c3y)))));
        if (x_lo > x_hi || y_lo > y_hi) continue;
        const float v0x = c3x - c1x, v0y = c3y - c1y, v1x = c2x - c1x, v1y = c2y - c1y;
        const float d00 = v0x * v0x + v0y * v0y, d01 = v0x * v1x + v0y * v1y, d11 = v1x * v1x + v1y * v1y;
        const float invd = 1.0f / (d00 * d11 - d01 * d01);
        for (int yc = y_lo; yc <= y_hi; ++yc)
          for (int xc = x_lo; xc <= x_hi; ++xc) {
            const float v2x = (float)xc - c1x, v2y = (float)yc - c1y;
            const float d02 = v0x * v2x + v0y * v2y, d12 = v1x * v2x + v1y * v2y;
            const float u = (d11 * d02 - d01 * d12) * invd, v = (d00 * d12 - d01 * d02) * invd;
            if (!(u > -0.01 && v >= -0.01 && u + v <= 1.01)) continue;
            const float value = p1.z + u * (p3.z - p1.z) + v * (p2.z - p1.z);
            float& c = patch[yc * 10 + xc];
            if (std::isinf(c) || value < c) c = value;
          }
      }
    }
  }
  // step 4: the unseen cells in front of something further than max_dist behind
  bool bg[100];
  for (int y = 0; y < 10; ++y)
    for (int x = 0; x < 10; ++x) {
      bg[y * 10 + x] = false;
      if (std::isfinite(patch[y * 10 + x])) continue;
      for (int y2 = y - 1; y2 <= y + 1 && !bg[y * 10 + x]; ++y2)
        for (int x2 = x - 1; x2 <= x + 1 && !bg[y * 10 + x]; ++x2) {
          if (x2 < 0 || x2 > 9 || y2 < 0 || y2 > 9) continue;
          const float nv = patch[y2 * 10 + x2];
          if (!std::isfinite(nv)) continue;
          const V3 fake = v3(cell * ((float)x + 0.6f * (float)(x - x2)) + c2w_off,
                             cell * ((float)y + 0.6f * (float)(y - y2)) + c2w_off, nv);
          if (I.rangeDifference(inv.apply(fake)) > max_dist) bg[y * 10 + x] = true;
        }
    }
  float out[100];
  for (int y = 0; y < 10; ++y)
    for (int x = 0; x < 10; ++x) {
      out[y * 10 + x] = patch[y * 10 + x];
      if (std::isfinite(patch[y * 10 + x])) continue;
      bool b = false;
      for (int y2 = std::max(0, y - 1); y2 <= std::min(9, y + 1); ++y2)
        for (int x2 = std::max(0, x - 1); x2 <= std::min(9, x + 1); ++x2) b = b || bg[y2 * 10 + x2];
      out[y * 10 + x] = b ? kInf : -kInf;
      st.background += b;
    }
  std::memcpy(patch, out, sizeof(out));
}

// step 5: getBlurredSurfacePatch (20, 1)
void blurredPatch(const float* patch, float support, float* blur) {
  float integral[400];
  for (int y = 0; y < 20; ++y)
    for (int x = 0; x < 20; ++x) {
      float v = patch[iround(std::floor(0.5f * (float)y)) * 10 + iround(std::floor(0.5f * (float)x))];
      if (std::isinf(v)) v = 0.5f * support;
      const float left = x > 0 ? integral[y * 20 + x - 1] : 0.0f, top = y > 0 ? integral[(y - 1) * 20 + x] : 0.0f;
      const float topleft = (x > 0 && y > 0) ? integral[(y - 1) * 20 + x - 1] : 0.0f;
      integral[y * 20 + x] = v + ((left + top) - topleft);
    }
  for (int y = 0; y < 20; ++y)
    for (int x = 0; x < 20; ++x) {
      const int top = std::max(-1, y - 2), left = std::max(-1, x - 2), right = std::min(19, x + 1),
                bottom = std::min(19, y + 1);
      const float norm = 1.0f / (float)((right - left) * (bottom - top));
      const float br = integral[bottom * 20 + right];
      const float tl = (top >= 0 && left >= 0) ? integral[top * 20 + left] : 0.0f;
      const float bl = left >= 0 ? integral[bottom * 20 + left] : 0.0f;
      const float tr = top >= 0 ? integral[top * 20 + right] : 0.0f;
      blur[y * 20 + x] = norm * (((br + tl) - bl) - tr);
    }
}

// step 6: extractDescriptor (36) at rotation rho
void descriptor(const float* blur, float support, float rho, float* d) {
  const float max_dist = 0.5f * support;
  const float wf = -2.0f * (2.0f - 1.0f) / ((2.0f + 1.0f) * 9.0f), wo = 2.0f * 2.0f / (2.0f + 1.0f);
  const float step = deg2rad(360.0f) / 36, cell = support / 20.0f, cf = 1.0f / cell, co = 0.5f * (support - cell);
  const float bpf = (max_dist - 0.5f * cell) / 10;
  for (int k = 0; k < 36; ++k) {
    const float angle = (float)k * step + rho;
    const float fx = sinf_cr(angle) * bpf, fy = -cosf_cr(angle) * bpf;
    float b[11];
    for (int j = 0; j <= 10; ++j) {
      const int bx = std::min(19, std::max(0, iround(cf * (fx * (float)j + co))));
      const int by = std::min(19, std::max(0, iround(cf * (fy * (float)j + co))));
      b[j] = blur[by * 20 + bx];
    }
    float s = 0.0f;
    for (int j = 0; j < 10; ++j) s += (wf * (float)j + wo) * (b[j + 1] - b[j]);
    d[k] = atan2f_glibc(s, max_dist) / deg2rad(180.0f);
  }
}

// step 7: getRotations; at most 5
int rotations(const float* d0, float* rot, float* score_out = nullptr) {
  const float step = deg2rad(360.0f) / 36;
  float score[36], smin = kInf, smax = -kInf;
  for (int s = 0; s < 36; ++s) {
    const float a = (float)s * step - kPi;
    float sc = 0.0f;
    for (int k = 0; k < 36; ++k) {
      const float w = 1.0f - std::fabs(normAngle(a - ((float)k * step - kPi))) / kPi;
      sc += d0[k] * (w * w);
    }
    sc = (1.0f / 36) * sc + 0.5f;
    score[s] = sc;
    smin = std::min(smin, sc);
    smax = std::max(smax, sc);
  }
  if (score_out) std::memcpy(score_out, score, sizeof(score));
  const float thr = smax - 0.2f * (smax - smin);
  bool alive[36];
  for (int s = 0; s < 36; ++s) alive[s] = !(score[s] <= thr);
  int n = 0;
  while (n < 5) {
    int best = -1;
    for (int s = 0; s < 36; ++s)
      if (alive[s] && (best < 0 || score[s] >= score[best])) best = s;
    if (best < 0) break;
    const float a = (float)best * step - kPi;
    rot[n++] = a;
    for (int s = 0; s < 36; ++s)
      if (alive[s] && std::fabs(normAngle(((float)s * step - kPi) - a)) < deg2rad(70.0f)) alive[s] = false;
  }
  return n;
}

// Rz (-rho) * pose: Eigen's AngleAxisf (-rho, UnitZ) as a matrix, times the 3 x 4
void rotatedPose(const Aff& pose, float rho, float* out) {
  const float c = cosf_cr(-rho), s = sinf_cr(-rho);
  const float R[3][3] = {{c, -s, 0.0f}, {s, c, 0.0f}, {0.0f, 0.0f, 1.0f}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j)
      out[i * 4 + j] = (R[i][0] * pose.m[j] + R[i][1] * pose.m[4 + j]) + R[i][2] * pose.m[8 + j];
}

}  // namespace

extern "C" {

// desc: 5 nk x 36, pose: 5 nk x 12, row_key / rot: 5 nk, stats: rows, invalid_pixels, pose_failed,
// fallback_normals, ring_max, background_cells.  dbg_patch (nullable): nk x 100, the patch after
// step 4; dbg_blur (nullable): nk x 400 (NaN rows where the entry gave no patch).
void narf_desc_ref(const float* ri, int w, int h, float cx, float cy, float fx, float fy, const float* sensor_pose,
                   int frame, const int32_t* pixel_idx, int64_t nk, float support, int rotation_invariant,
                   float* desc, float* pose_out, int32_t* row_key, float* rot_out, int64_t* n_out, int64_t* stats,
                   float* dbg_patch, float* dbg_blur) {
  Image I;
  makeImage(w, h, cx, cy, fx, fy, sensor_pose, frame, ri, I);
  Stats st;
  int64_t rows = 0;
  for (int64_t i = 0; i < nk; ++i) {
    if (dbg_patch) std::fill(dbg_patch + i * 100, dbg_patch + (i + 1) * 100, kNaN);
    if (dbg_blur) std::fill(dbg_blur + i * 400, dbg_blur + (i + 1) * 400, kNaN);
    const int32_t p = pixel_idx[i];
    if (p < 0 || (int64_t)p >= (int64_t)w * h || !std::isfinite(ri[(size_t)p * 4 + 3])) {
      ++st.invalid;
      continue;
    }
    const int y = p / w, x = p - y * w;
    Aff pose;
    const int how = uprightPose(I, I.point(x, y), 0.5f * support, pose, st);
    if (how == 2) {
      ++st.pose_failed;
      continue;
    }
    st.fallback += how == 1;
    float patch[100], blur[400], d0[36];
    surfacePatch(I, pose, support, patch, st);
    blurredPatch(patch, support, blur);
    if (dbg_patch) std::memcpy(dbg_patch + i * 100, patch, sizeof(patch));
    if (dbg_blur) std::memcpy(dbg_blur + i * 400, blur, sizeof(blur));
    descriptor(blur, support, 0.0f, d0);
    float rot[5] = {0.0f, 0, 0, 0, 0};
    const int nrot = rotation_invariant ? rotations(d0, rot) : 1;
    for (int r = 0; r < nrot; ++r, ++rows) {
      if (rotation_invariant) {
        descriptor(blur, support, rot[r], desc + rows * 36);
        rotatedPose(pose, rot[r], pose_out + rows * 12);
      } else {
        std::memcpy(desc + rows * 36, d0, sizeof(d0));
        std::memcpy(pose_out + rows * 12, pose.m, sizeof(pose.m));
      }
      row_key[rows] = (int32_t)i;
      rot_out[rows] = rot[r];
    }
  }
  st.rows = rows;
  *n_out = rows;
  const int64_t s[6] = {st.rows, st.invalid, st.pose_failed, st.fallback, st.ring_max, st.background};
  std::memcpy(stats, s, sizeof(s));
}

// step 7 alone: the rotations (at most 5) and the 36 scores of a descriptor at rotation 0
int narf_rotations_ref(const float* d0, float* rot, float* score) { return rotations(d0, rot, score); }

// steps 5 and 6 alone: the descriptor at rotation rho of a 10 x 10 patch
void narf_patch_descriptor_ref(const float* patch, float support, float rho, float* blur, float* d) {
  blurredPatch(patch, support, blur);
  descriptor(blur, support, rho, d);
}

// Tools::getIndices with Tools::areEqual: for each keypoint in order, every cloud index ascending
// with all three |differences| < tol.  Returns the count; writes at most cap.
int64_t point_indices_ref(const float* x, const float* y, const float* z, int64_t n, const float* kx, const float* ky,
                          const float* kz, int64_t nk, float tol, int32_t* out, int64_t cap) {
  int64_t m = 0;
  for (int64_t i = 0; i < nk; ++i)
    for (int64_t j = 0; j < n; ++j)
      if (std::fabs(kx[i] - x[j]) < tol && std::fabs(ky[i] - y[j]) < tol && std::fabs(kz[i] - z[j]) < tol) {
        if (m < cap) out[m] = (int32_t)j;
        ++m;
      }
  return m;
}

}  // extern "C"
