// pfx_range_image.h -- what the kernels on the planar range image share (pfx_narf.hip: the range
// image, the border extractor and the NARF keypoints; pfx_narf_desc.hip: the NARF descriptors):
// the image's geometry (RangeImagePlanar), VectorAverage3f, getSurfaceInformation and normAngle.
// Every function keeps the float operation order of its PCL statement.
#pragma once
#include <cstring>

#include "pfx_device_math.h"
#include "pfx_internal.h"

namespace pfx {

struct Aff { float m[12]; };  // row-major 3x4 [R | t]

struct Img {
  int w, h;
  float cx, cy, fx, fy, fxr, fyr;
  Aff to_world, to_ri;
};

__device__ __forceinline__ f3 aff_apply(const Aff& a, f3 p) {
  return mk3(a.m[3] + (a.m[0] * p.x + a.m[1] * p.y + a.m[2] * p.z),
             a.m[7] + (a.m[4] * p.x + a.m[5] * p.y + a.m[6] * p.z),
             a.m[11] + (a.m[8] * p.x + a.m[9] * p.y + a.m[10] * p.z));
}

__device__ __forceinline__ bool in_image(const Img& I, int x, int y) { return x >= 0 && x < I.w && y >= 0 && y < I.h; }

__device__ __forceinline__ f3 calc3d(const Img& I, float ix, float iy, float range) {
  float dx = (ix + 0.0f - I.cx) * I.fxr, dy = (iy + 0.0f - I.cy) * I.fyr;
  f3 p;
  p.z = range / (sqrtf(dx * dx + dy * dy + 1));
  p.x = dx * p.z;
  p.y = dy * p.z;
  return aff_apply(I.to_world, p);
}

__device__ __forceinline__ void image_point(const Img& I, f3 pt, float& ix, float& iy, float& range) {
  f3 t = aff_apply(I.to_ri, pt);
  if (t.z <= 0) { ix = iy = range = -1.0f; return; }
  range = sqrtf(sqn3(t));
  ix = I.cx + I.fx * t.x / t.z - 0.0f;
  iy = I.cy + I.fy * t.y / t.z - 0.0f;
}

__device__ __forceinline__ float sq_dist(float4 a, float4 b) {  // diff = b - a
  float dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ float4 get_point(const Img& I, const float4* __restrict__ P, int x, int y) {
  if (!in_image(I, x, y)) return make_float4(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), -INFINITY);
  return P[y * I.w + x];
}
__device__ __forceinline__ bool is_valid(const Img& I, const float4* __restrict__ P, int x, int y) {
  return in_image(I, x, y) && isfinite(P[y * I.w + x].w);
}

__device__ __forceinline__ float norm_angle(float a) {
  const float pi = 3.14159265358979323846f;
  return a >= 0 ? fmodf(a + pi, 2.0f * pi) - pi : -(fmodf(pi - a, 2.0f * pi) - pi);
}

// ---- VectorAverage3f -------------------------------------------------------------------------
struct VecAvg {
  int n;
  float acc_w;
  f3 mean;
  float c00, c01, c02, c11, c12, c22;
  __device__ void init() { n = 0; acc_w = 0.f; mean = mk3(0, 0, 0); c00 = c01 = c02 = c11 = c12 = c22 = 0.f; }
  __device__ void add(f3 s) {
    ++n;
    acc_w += 1.0f;
    float alpha = 1.0f / acc_w;
    f3 d = sub3(s, mean);
    mean = add3(mean, mk3(alpha * d.x, alpha * d.y, alpha * d.z));
    float om = 1.0f - alpha;
    // `(1.0f-alpha)*(covariance_(i, j) + alpha*diff[i]*diff[j])`: (alpha * d_i) * d_j
    c00 = om * (c00 + alpha * d.x * d.x);
    c01 = om * (c01 + alpha * d.x * d.y);
    c02 = om * (c02 + alpha * d.x * d.z);
    c11 = om * (c11 + alpha * d.y * d.y);
    c12 = om * (c12 + alpha * d.y * d.z);
    c22 = om * (c22 + alpha * d.z * d.z);
  }
  // add (sample, weight): add () is its weight = 1 case (1.0f / acc_w there, weight / acc_w here)
  __device__ void add_w(f3 s, float w) {
    if (w == 0.0f) return;
    ++n;
    acc_w += w;
    float alpha = w / acc_w;
    f3 d = sub3(s, mean);
    mean = add3(mean, mk3(alpha * d.x, alpha * d.y, alpha * d.z));
    float om = 1.0f - alpha;
    c00 = om * (c00 + alpha * d.x * d.x);
    c01 = om * (c01 + alpha * d.x * d.y);
    c02 = om * (c02 + alpha * d.x * d.z);
    c11 = om * (c11 + alpha * d.y * d.y);
    c12 = om * (c12 + alpha * d.y * d.z);
    c22 = om * (c22 + alpha * d.z * d.z);
  }
  __device__ void pca(float ev[3], f3 evec[3]) const {
    Sym3 m;
    m.a00 = c00; m.a01 = c01; m.a02 = c02;
    m.a10 = c01; m.a11 = c11; m.a12 = c12;
    m.a20 = c02; m.a21 = c12; m.a22 = c22;
    eigen33_full(m, evec, ev);
  }
};

// RangeImage::getSurfaceInformation (no-jumps part) around pixel (x, y) for `point`: the window
// of `radius` in steps of `step` (at most 25 pixels), the plane through the neighbours within
// four times the squared distance of the no_of_closest-th.  False with fewer than 3 of them.
__device__ __forceinline__ bool surface_information(const Img& I, const float4* __restrict__ P, int x, int y,
                                                    int radius, int step, int no_of_closest, float4 point,
                                                    f3& normal, f3& mean, float& maxd2) {
  float nd[25];
  float4 np[25];
  int cnt = 0;
  for (int y2 = y - radius; y2 <= y + radius; y2 += step)
    for (int x2 = x - radius; x2 <= x + radius; x2 += step) {
      if (!is_valid(I, P, x2, y2) || cnt >= 25) continue;
      float4 q = P[y2 * I.w + x2];
      float d = sq_dist(point, q);
      int j = cnt++;
      while (j > 0 && d < nd[j - 1]) { nd[j] = nd[j - 1]; np[j] = np[j - 1]; --j; }
      nd[j] = d;
      np[j] = q;
    }
  if (cnt == 0) return false;
  int k = cnt < no_of_closest ? cnt : no_of_closest;
  maxd2 = nd[k - 1];
  float lim = maxd2 * 4.0f;
  VecAvg va;
  va.init();
  for (int j = 0; j < cnt; ++j) {
    if (nd[j] > lim) break;
    va.add(mk3(np[j].x, np[j].y, np[j].z));
  }
  if (va.n < 3) return false;
  float ev[3];
  f3 evec[3];
  va.pca(ev, evec);
  normal = evec[0];
  f3 sensor = mk3(I.to_world.m[3], I.to_world.m[7], I.to_world.m[11]);
  f3 view = normalized3(sub3(sensor, mk3(point.x, point.y, point.z)));
  if (dot3(normal, view) < 0.0f) normal = scale3(normal, -1.0f);
  mean = va.mean;
  return true;
}

// the image of a camera: to_world = sensor_pose * coordinate-frame axes, to_ri its isometry inverse
inline Img make_img(const pfx_camera& c) {
  Img I;
  I.w = c.width; I.h = c.height;
  I.cx = c.center_x; I.cy = c.center_y; I.fx = c.focal_length_x; I.fy = c.focal_length_y;
  I.fxr = 1 / c.focal_length_x; I.fyr = 1 / c.focal_length_y;
  float F[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  if (c.coordinate_frame == 1) {
    float L[4][4] = {{0, 0, 1, 0}, {-1, 0, 0, 0}, {0, -1, 0, 0}, {0, 0, 0, 1}};
    std::memcpy(F, L, sizeof(F));
  }
  float W[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      W[i][j] = ((c.sensor_pose[i * 4 + 0] * F[0][j] + c.sensor_pose[i * 4 + 1] * F[1][j]) +
                 c.sensor_pose[i * 4 + 2] * F[2][j]) + c.sensor_pose[i * 4 + 3] * F[3][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) I.to_world.m[i * 4 + j] = W[i][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) I.to_ri.m[i * 4 + j] = W[j][i];
  for (int i = 0; i < 3; ++i)
    I.to_ri.m[i * 4 + 3] = -(I.to_ri.m[i * 4 + 0] * W[0][3] + I.to_ri.m[i * 4 + 1] * W[1][3] +
                             I.to_ri.m[i * 4 + 2] * W[2][3]);
  return I;
}

// the image size pfx_narf_keypoints* and pfx_narf_descriptors* accept (a 640 x 480 bitmap, a row
// per 1024-thread workgroup)
constexpr int kNarfMaxPixels = 9600 * 32;
constexpr int kNarfMaxWidth = 1024;

}  // namespace pfx
