// pfx_narf_desc.hip -- NarfDescriptor (evaluation.cpp:613-648) on the planar range image, and
// Tools::getIndices (tools.h:91-102), on gfx950.  DESIGN.md "NARF descriptors: the contract" states
// every operation; tests/cpp/narf_desc_ref.cpp is its CPU restatement, and the kernel gives its bits.
//
// k_narf_desc: one 64-thread workgroup (one wave) per entry of pixel_idx.  The long pole is the
// weighted VectorAverage3f of step 2, a serial chain of a few thousand dependent adds that must keep
// its order, so one lane runs it and more waves per entry would only wait; the device fills with
// entries instead (the workgroup holds 5.8 KB of LDS and few registers).
//   step 2  the wave tests 64 consecutive ring positions at a time, ballots for the ring's end and
//           compacts the surviving (Q, w) in ring order into an LDS queue that lane 0 consumes;
//   step 3  every lane rasterises the two triangles of one ring pixel into the 10 x 10 patch with
//           LDS atomicMin on an order-preserving integer key (the minimum is order-free);
//   steps 4-7  lane-parallel over the 100 cells, the 20 x 20 integral image by anti-diagonals, the
//           400 blurred cells, the 36 beams and the 36 scores; lane 0 selects the rotations.
// Rows go to fixed slots [nk][5]; k_count_scan and k_narf_desc_compact put them in keypoint order.
// k_point_indices: one keypoint per lane, the cloud in chunks and tiled through LDS, a counting and a
// writing pass around the same scan.  Nothing synchronises with the host; statistics through the deferred reports.
#include <algorithm>
#include <climits>

#include "pfx_range_image.h"

namespace pfx {
namespace {

enum { kWordRows = 0, kWordInvalid, kWordPoseFailed, kWordFallback, kWordRingMax, kWordBackground };
constexpr int kMaxRot = 5;         // rows of a keypoint (rotations at least 70 degrees apart)
constexpr float kPiF = 3.14159274101257324f;  // (float)M_PI

__device__ __forceinline__ float deg2rad(float a) { return a * 0.017453293f; }

// lrint (round half even); a NaN and what lies beyond +-2^30 (undefined in PCL) saturate
__device__ __forceinline__ int iround(float v) {
  if (!(v == v)) return -(1 << 30);
  if (v >= 1073741824.0f) return 1 << 30;
  if (v <= -1073741824.0f) return -(1 << 30);
  return (int)rintf(v);
}

// the pixel of ring step i (after its move): the ring of `r` about (cx, cy) starts left of its top
// left corner and walks right, down, left, up; r = 0 is the centre
__device__ __forceinline__ void ring_pos(int cx, int cy, int r, int i, int& x, int& y) {
  if (i <= 2 * r) { x = cx - r + i; y = cy - r; }
  else if (i <= 4 * r) { x = cx + r; y = cy - r + (i - 2 * r); }
  else if (i <= 6 * r) { x = cx + r - (i - 4 * r); y = cy + r; }
  else { x = cx - r; y = cy + r - (i - 6 * r); }
}

// float <-> an int that orders as the float does; its own inverse
__device__ __forceinline__ int order_key(float a) {
  const int b = __float_as_int(a);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

__device__ __forceinline__ f3 point_at(const Img& I, const float4* __restrict__ P, int x, int y) {
  const float4 q = P[y * I.w + x];
  return mk3(q.x, q.y, q.z);
}

struct DescLds {
  float4 queue[64];
  int key[100];
  float patch[100];
  int bg[100];
  float integral[400];
  float blur[400];
  float d0[36];
  float score[36];
  Aff pose, inv;
  float rot[kMaxRot];
  int nrot, how;
};

// RangeImage::getRangeDifference
__device__ __forceinline__ float range_difference(const Img& I, const float4* __restrict__ P, f3 q) {
  float ix, iy, rng;
  image_point(I, q, ix, iy, rng);
  const int x = iround(ix), y = iround(iy);
  if (!in_image(I, x, y)) return -INFINITY;
  const float r = P[y * I.w + x].w;
  if (isinf(r)) return r > 0.0f ? INFINITY : -INFINITY;
  return r - rng;
}

// step 3, one ring pixel: its two triangles into the patch keys; whether one survived
__device__ __forceinline__ bool raster_pixel(const Img& I, const float4* __restrict__ P, const Aff& pose, int x, int y,
                                             float max_dist, float w2c, float w2c_off, int* key) {
  if (!is_valid(I, P, x, y) || !is_valid(I, P, x + 1, y + 1)) return false;
  const f3 p1 = aff_apply(pose, point_at(I, P, x, y)), p2 = aff_apply(pose, point_at(I, P, x + 1, y + 1));
  if (fabsf(p1.z) > max_dist || fabsf(p2.z) > max_dist) return false;
  const float c1x = w2c * p1.x + w2c_off, c1y = w2c * p1.y + w2c_off;
  const float c2x = w2c * p2.x + w2c_off, c2y = w2c * p2.y + w2c_off;
  bool survived = false;
  for (int tri = 0; tri < 2; ++tri) {
    const int x3 = tri == 0 ? x : x + 1, y3 = tri == 0 ? y + 1 : y;
    if (!is_valid(I, P, x3, y3)) continue;
    const f3 p3 = aff_apply(pose, point_at(I, P, x3, y3));
    if (fabsf(p3.z) > max_dist) continue;
    if ((p1.x < -max_dist && p2.x < -max_dist && p3.x < -max_dist) ||
        (p1.x > max_dist && p2.x > max_dist && p3.x > max_dist) ||
        (p1.y < -max_dist && p2.y < -max_dist && p3.y < -max_dist) ||
        (p1.y > max_dist && p2.y > max_dist && p3.y > max_dist))
      continue;
    survived = true;
    const float c3x = w2c * p3.x + w2c_off, c3y = w2c * p3.y + w2c_off;
    const int x_lo = max(0, iround(ceilf(fminf(c1x, fminf(c2x, c3x)))));
    const int x_hi = min(9, iround(floorf(fmaxf(c1x, fmaxf(c2x, c3x)))));
    const int y_lo = max(0, iround(ceilf(fminf(c1y, fminf(c2y, c3y)))));
    const int y_hi = min(9, iround(floorf(fmaxf(c1y, fmaxf(c2y, c3y)))));
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
        atomicMin(&key[yc * 10 + xc], order_key(value));
      }
  }
  return survived;
}

// step 6: beam k of extractDescriptor (36) at rotation rho
__device__ __forceinline__ float beam_value(const float* blur, float support, float rho, int k) {
  const float max_dist = 0.5f * support;
  const float wf = -2.0f * (2.0f - 1.0f) / ((2.0f + 1.0f) * 9.0f), wo = 2.0f * 2.0f / (2.0f + 1.0f);
  const float step = deg2rad(360.0f) / 36, cell = support / 20.0f, cf = 1.0f / cell, co = 0.5f * (support - cell);
  const float bpf = (max_dist - 0.5f * cell) / 10;
  const float angle = (float)k * step + rho;
  const float fx = sinf_cr(angle) * bpf, fy = -cosf_cr(angle) * bpf;
  float s = 0.0f, prev = 0.0f;
  for (int j = 0; j <= 10; ++j) {
    const int bx = min(19, max(0, iround(cf * (fx * (float)j + co))));
    const int by = min(19, max(0, iround(cf * (fy * (float)j + co))));
    const float b = blur[by * 20 + bx];
    if (j > 0) s += (wf * (float)(j - 1) + wo) * (b - prev);
    prev = b;
  }
  return atan2f_glibc(s, max_dist) / deg2rad(180.0f);
}

__global__ void __launch_bounds__(64)
k_narf_desc(Img I, const float4* __restrict__ P, const int32_t* __restrict__ pixel_idx, float support, int rotinv,
            float* __restrict__ slot_desc, float* __restrict__ slot_pose, int* __restrict__ counts,
            int* __restrict__ stats) {
  __shared__ DescLds S;
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int p = pixel_idx[e];
  // ---- step 1 ----
  if (p < 0 || p >= I.w * I.h || !isfinite(P[p].w)) {
    if (lane == 0) {
      counts[e] = 0;
      atomicAdd(stats + kWordInvalid, 1);
    }
    return;
  }
  const float4 P4 = P[p];
  const f3 Pt = mk3(P4.x, P4.y, P4.z);
  const float max_dist = 0.5f * support;
  int ring_max = 0;
  // ---- step 2: getNormalBasedUprightTransformation ----
  int cx, cy;
  {
    float ix, iy, rng;
    image_point(I, Pt, ix, iy, rng);
    cx = iround(ix);
    cy = iround(iy);
  }
  VecAvg va;  // lane 0's
  va.init();
  {
    const float max_d2 = max_dist * max_dist, max_dist_rec = 1.0f / max_dist;
    for (int radius = 1;; ++radius) {
      ring_max = radius;
      bool still = false;
      const int npos = 8 * radius;
      for (int base = 0; base < npos; base += 64) {
        const int k = base + lane;
        bool ok = false;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < npos) {
          int x, y;
          ring_pos(cx, cy, radius, k, x, y);
          if (is_valid(I, P, x, y)) {
            q = P[y * I.w + x];
            const float d2 = sqn3(sub3(mk3(q.x, q.y, q.z), Pt));
            if (!(d2 > max_d2)) {
              ok = true;
              q.w = sqrtf(d2) * max_dist_rec;
            }
          }
        }
        still |= __ballot(ok) != 0;
        const bool push = ok && q.w != 0.0f;
        const uint64_t pm = __ballot(push);
        if (push) S.queue[__popcll(pm & __lanemask_lt())] = q;
        __syncthreads();
        if (lane == 0) {
          const int c = __popcll(pm);
          for (int j = 0; j < c; ++j) {
            const float4 s = S.queue[j];
            va.add_w(mk3(s.x, s.y, s.z), s.w);
          }
        }
        __syncthreads();
      }
      if (!still) break;
    }
  }
  if (lane == 0) {
    int how = 0;
    f3 normal = mk3(0.f, 0.f, 0.f), mean = mk3(0.f, 0.f, 0.f);
    const f3 sensor = mk3(I.to_world.m[3], I.to_world.m[7], I.to_world.m[11]);
    if (va.n > 10) {
      float ev[3];
      f3 evec[3];
      va.pca(ev, evec);
      normal = evec[0];
      mean = va.mean;
      if (dot3(normal, normalized3(sub3(mean, sensor))) < 0.0f) normal = scale3(normal, -1.0f);
    } else {
      float maxd2;
      how = surface_information(I, P, cx, cy, 2, 1, 15, P4, normal, mean, maxd2) ? 1 : 2;
    }
    if (how != 2) {
      const float s = dot3(normal, mean) - dot3(normal, Pt);
      const f3 on_plane = mk3(s * normal.x + Pt.x, s * normal.y + Pt.y, s * normal.z + Pt.z);
      const f3 t0 = normalized3(cross3(mk3(0.0f, 1.0f, 0.0f), normal));
      const f3 t1 = normalized3(cross3(normal, t0));
      const f3 t2 = normalized3(normal);
      const f3 rows[3] = {t0, t1, t2};
      bool finite = true;
      for (int i = 0; i < 3; ++i) {
        const float t = -mv3(rows[i], on_plane);
        S.pose.m[i * 4 + 0] = rows[i].x;
        S.pose.m[i * 4 + 1] = rows[i].y;
        S.pose.m[i * 4 + 2] = rows[i].z;
        S.pose.m[i * 4 + 3] = t;
        finite = finite && isfinite(rows[i].x) && isfinite(rows[i].y) && isfinite(rows[i].z) && isfinite(t);
      }
      if (!finite) how = 2;  // a normal along (0, 1, 0), an overflow: no frame
    }
    if (how != 2) {
      const float* m = S.pose.m;
      for (int i = 0; i < 3; ++i) {  // Eigen::Isometry inverse: R^T, -(R^T t)
        for (int j = 0; j < 3; ++j) S.inv.m[i * 4 + j] = m[j * 4 + i];
        S.inv.m[i * 4 + 3] = -((m[0 * 4 + i] * m[3] + m[1 * 4 + i] * m[7]) + m[2 * 4 + i] * m[11]);
      }
    }
    S.how = how;
  }
  for (int k = lane; k < 100; k += 64) S.key[k] = INT_MAX;
  __syncthreads();
  const int how = S.how;
  if (how == 2) {
    if (lane == 0) {
      counts[e] = 0;
      atomicAdd(stats + kWordPoseFailed, 1);
      atomicMax(stats + kWordRingMax, ring_max);
    }
    return;
  }
  // ---- step 3: getInterpolatedSurfaceProjection (pose, 10, support) ----
  const float cell = support / 10.0f;
  const float w2c = 1.0f / cell, w2c_off = 0.5f * 10 - 0.5f, c2w_off = -max_dist + 0.5f * cell;
  {
    float ix, iy, rng;
    image_point(I, mk3(S.inv.m[3], S.inv.m[7], S.inv.m[11]), ix, iy, rng);
    const int mx = iround(ix), my = iround(iy);
    for (int radius = 0;; ++radius) {
      ring_max = max(ring_max, radius);
      bool still = radius < 2;
      const int npos = radius == 0 ? 1 : 8 * radius;
      for (int base = 0; base < npos; base += 64) {
        const int k = base + lane;
        bool survived = false;
        if (k < npos) {
          int x, y;
          ring_pos(mx, my, radius, k, x, y);
          survived = raster_pixel(I, P, S.pose, x, y, max_dist, w2c, w2c_off, S.key);
        }
        still |= __ballot(survived) != 0;
      }
      if (!still) break;
    }
  }
  __syncthreads();
  // ---- step 4: background cells ----
  for (int k = lane; k < 100; k += 64) S.patch[k] = S.key[k] == INT_MAX ? -INFINITY : key_value(S.key[k]);
  __syncthreads();
  for (int k = lane; k < 100; k += 64) {
    const int y = k / 10, x = k - y * 10;
    bool bg = false;
    if (!isfinite(S.patch[k]))
      for (int y2 = y - 1; y2 <= y + 1 && !bg; ++y2)
        for (int x2 = x - 1; x2 <= x + 1 && !bg; ++x2) {
          if (x2 < 0 || x2 > 9 || y2 < 0 || y2 > 9) continue;
          const float nv = S.patch[y2 * 10 + x2];
          if (!isfinite(nv)) continue;
          const f3 fake = mk3(cell * ((float)x + 0.6f * (float)(x - x2)) + c2w_off,
                              cell * ((float)y + 0.6f * (float)(y - y2)) + c2w_off, nv);
          if (range_difference(I, P, aff_apply(S.inv, fake)) > max_dist) bg = true;
        }
    S.bg[k] = bg;
  }
  __syncthreads();
  int n_background = 0;
  for (int k = lane; k < 100 + 64 - 100 % 64; k += 64) {  // (whole waves: the ballot below)
    bool b = false;
    if (k < 100 && !isfinite(S.patch[k])) {
      const int y = k / 10, x = k - y * 10;
      for (int y2 = max(0, y - 1); y2 <= min(9, y + 1); ++y2)
        for (int x2 = max(0, x - 1); x2 <= min(9, x + 1); ++x2) b = b || S.bg[y2 * 10 + x2] != 0;
      S.patch[k] = b ? INFINITY : -INFINITY;
    }
    n_background += __popcll(__ballot(b));
  }
  __syncthreads();
  // ---- step 5: getBlurredSurfacePatch (20, 1) ----
  for (int d = 0; d < 39; ++d) {  // the integral image by anti-diagonals
    const int x = lane, y = d - lane;
    if (x < 20 && y >= 0 && y < 20) {
      float v = S.patch[iround(floorf(0.5f * (float)y)) * 10 + iround(floorf(0.5f * (float)x))];
      if (isinf(v)) v = 0.5f * support;
      const float left = x > 0 ? S.integral[y * 20 + x - 1] : 0.0f, top = y > 0 ? S.integral[(y - 1) * 20 + x] : 0.0f;
      const float topleft = (x > 0 && y > 0) ? S.integral[(y - 1) * 20 + x - 1] : 0.0f;
      S.integral[y * 20 + x] = v + ((left + top) - topleft);
    }
    __syncthreads();
  }
  for (int k = lane; k < 400; k += 64) {
    const int y = k / 20, x = k - y * 20;
    const int top = max(-1, y - 2), left = max(-1, x - 2), right = min(19, x + 1), bottom = min(19, y + 1);
    const float norm = 1.0f / (float)((right - left) * (bottom - top));
    const float br = S.integral[bottom * 20 + right];
    const float tl = (top >= 0 && left >= 0) ? S.integral[top * 20 + left] : 0.0f;
    const float bl = left >= 0 ? S.integral[bottom * 20 + left] : 0.0f;
    const float tr = top >= 0 ? S.integral[top * 20 + right] : 0.0f;
    S.blur[k] = norm * (((br + tl) - bl) - tr);
  }
  __syncthreads();
  // ---- step 6 at rotation 0 ----
  float d0 = 0.0f;
  if (lane < 36) {
    d0 = beam_value(S.blur, support, 0.0f, lane);
    S.d0[lane] = d0;
  }
  __syncthreads();
  // ---- step 7: getRotations ----
  int nrot = 1;
  if (rotinv) {
    const float step = deg2rad(360.0f) / 36;
    if (lane < 36) {
      const float a = (float)lane * step - kPiF;
      float sc = 0.0f;
      for (int k = 0; k < 36; ++k) {
        const float w = 1.0f - fabsf(norm_angle(a - ((float)k * step - kPiF))) / kPiF;
        sc += S.d0[k] * (w * w);
      }
      S.score[lane] = (1.0f / 36) * sc + 0.5f;
    }
    __syncthreads();
    if (lane == 0) {
      float smin = INFINITY, smax = -INFINITY;
      for (int s = 0; s < 36; ++s) {
        smin = fminf(smin, S.score[s]);
        smax = fmaxf(smax, S.score[s]);
      }
      const float thr = smax - 0.2f * (smax - smin);
      uint64_t alive = 0;
      for (int s = 0; s < 36; ++s)
        if (!(S.score[s] <= thr)) alive |= 1ull << s;
      int n = 0;
      while (n < kMaxRot) {
        int best = -1;
        for (int s = 0; s < 36; ++s)
          if ((alive >> s & 1) && (best < 0 || S.score[s] >= S.score[best])) best = s;
        if (best < 0) break;
        const float a = (float)best * step - kPiF;
        S.rot[n++] = a;
        for (int s = 0; s < 36; ++s)
          if ((alive >> s & 1) && fabsf(norm_angle(((float)s * step - kPiF) - a)) < deg2rad(70.0f))
            alive &= ~(1ull << s);
      }
      S.nrot = n;
    }
    __syncthreads();
    nrot = S.nrot;
  }
  // ---- the rows, into the entry's slots ----
  for (int r = 0; r < nrot; ++r) {
    const int64_t slot = e * kMaxRot + r;
    if (!rotinv) {
      if (lane < 36) slot_desc[slot * 36 + lane] = d0;
      if (lane < 12) slot_pose[slot * 12 + lane] = S.pose.m[lane];
    } else {
      const float rho = S.rot[r];
      if (lane < 36) slot_desc[slot * 36 + lane] = beam_value(S.blur, support, rho, lane);
      if (lane < 12) {  // Rz (-rho) * pose: AngleAxisf (-rho, UnitZ) as a matrix, times the 3 x 4
        const float c = cosf_cr(-rho), s = sinf_cr(-rho);
        const int i = lane >> 2, j = lane & 3;
        const float r0 = i == 0 ? c : i == 1 ? s : 0.0f, r1 = i == 0 ? -s : i == 1 ? c : 0.0f, r2 = i == 2 ? 1.0f : 0.0f;
        slot_pose[slot * 12 + lane] = (r0 * S.pose.m[j] + r1 * S.pose.m[4 + j]) + r2 * S.pose.m[8 + j];
      }
    }
  }
  if (lane == 0) {
    counts[e] = nrot;
    atomicAdd(stats + kWordRows, nrot);
    if (how == 1) atomicAdd(stats + kWordFallback, 1);
    atomicMax(stats + kWordRingMax, ring_max);
    atomicAdd(stats + kWordBackground, n_background);
  }
}

// exclusive scan of n counts by one workgroup: offsets[i] and the total
__global__ void __launch_bounds__(1024)
k_count_scan(const int* __restrict__ counts, int64_t n, int64_t* __restrict__ offsets, int64_t* __restrict__ total) {
  __shared__ long long part[1024];
  __shared__ long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + tid;
    const long long v = i < n ? counts[i] : 0;
    part[tid] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const long long add = tid >= o ? part[tid - o] : 0;
      __syncthreads();
      part[tid] += add;
      __syncthreads();
    }
    if (i < n) offsets[i] = carry + part[tid] - v;
    __syncthreads();
    if (tid == 1023) carry += part[1023];
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// the slots' rows in keypoint order; rows at or beyond cap are dropped (the total says so)
__global__ void __launch_bounds__(64)
k_narf_desc_compact(const float* __restrict__ slot_desc, const float* __restrict__ slot_pose,
                    const int* __restrict__ counts, const int64_t* __restrict__ offsets, float* __restrict__ desc,
                    float* __restrict__ pose, int32_t* __restrict__ row_key, int64_t cap) {
  const int lane = threadIdx.x;
  const int64_t e = blockIdx.x;
  const int c = counts[e];
  for (int r = 0; r < c; ++r) {
    const int64_t row = offsets[e] + r, slot = e * kMaxRot + r;
    if (row >= cap) return;
    if (lane < 36) desc[row * 36 + lane] = slot_desc[slot * 36 + lane];
    if (lane < 12) pose[row * 12 + lane] = slot_pose[slot * 12 + lane];
    if (lane == 0) row_key[row] = (int32_t)e;
  }
}

// Tools::getIndices: keypoint i = blockIdx.x * 64 + lane against chunk blockIdx.y of the cloud (`len`
// points, a multiple of the tile), tile by tile.  counts and offsets are [nk][chunks]: a keypoint's
// chunks ascend, so the scan over that order is the order of the reference's double loop.  The tile's
// tail is padded with NaN, which matches nothing, so the inner loop has a fixed length and unrolls.
constexpr int kIndexTile = 256;
template <bool WRITE>
__global__ void __launch_bounds__(64)
k_point_indices(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int64_t n,
                int64_t len, const float* __restrict__ kx, const float* __restrict__ ky, const float* __restrict__ kz,
                int64_t nk, float tol, int* __restrict__ counts, const int64_t* __restrict__ offsets,
                int32_t* __restrict__ out, int64_t cap) {
  __shared__ float4 tile[kIndexTile];
  const int lane = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  const int64_t slot = i * gridDim.y + blockIdx.y;
  const float nan = __builtin_nanf("");
  const float ax = i < nk ? kx[i] : nan, ay = i < nk ? ky[i] : nan, az = i < nk ? kz[i] : nan;
  int c = 0;
  int64_t pos = (WRITE && i < nk) ? offsets[slot] : 0;
  const int64_t begin = blockIdx.y * len, end = begin + len < n ? begin + len : n;
  for (int64_t base = begin; base < end; base += kIndexTile) {
    for (int t = lane; t < kIndexTile; t += 64) {
      const int64_t j = base + t;
      tile[t] = j < end ? make_float4(x[j], y[j], z[j], 0.f) : make_float4(nan, nan, nan, 0.f);
    }
    __syncthreads();
#pragma unroll 8
    for (int t = 0; t < kIndexTile; ++t) {
      const float4 p = tile[t];
      if (fabsf(ax - p.x) < tol && fabsf(ay - p.y) < tol && fabsf(az - p.z) < tol) {
        if (WRITE) {
          if (pos < cap) out[pos] = (int32_t)(base + t);
          ++pos;
        } else {
          ++c;
        }
      }
    }
    __syncthreads();
  }
  if (!WRITE && i < nk) counts[slot] = c;
}

}  // namespace

void narf_image_size_rule(const pfx_camera& cam, const char* what) {
  PFX_CHECK(cam.width > 0 && cam.height > 0 && (int64_t)cam.width * cam.height <= kNarfMaxPixels &&
                cam.width <= kNarfMaxWidth,
            std::string(what) + ": image larger than 640x480 pixels is not supported");
}

void narf_camera_rule(const pfx_camera& cam, const char* what) {
  narf_image_size_rule(cam, what);
  if (cam.noise_level != 0.0f)
    throw Error(PFX_ERR_UNSUPPORTED, std::string(what) + ": noise_level != 0 (running-average z-buffer) not supported");
}

void narf_desc_dev(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const pfx_camera& cam,
                   const int32_t* pixel_idx, int64_t nk, const pfx_narf_desc_params& prm, float* desc, float* pose,
                   int32_t* row_key, int64_t cap, int64_t* d_n_out) {
  hipStream_t st = ctx->stream;
  if (nk == 0) {
    PFX_HIP(hipMemsetAsync(d_n_out, 0, sizeof(int64_t), st));
    return;
  }
  const Img I = make_img(cam);
  float4* P = ctx->buf("narf_desc_ri").as<float4>((size_t)I.w * I.h);
  float* slot_desc = ctx->buf("narf_desc_slots").as<float>((size_t)nk * kMaxRot * 48);
  float* slot_pose = slot_desc + (size_t)nk * kMaxRot * 36;
  int* counts = ctx->buf("narf_desc_counts").as<int>((size_t)nk);
  int64_t* offsets = ctx->buf("narf_desc_offsets").as<int64_t>((size_t)nk);
  int* stats = report_words(ctx, kRepNarfDesc);
  range_image_dev(ctx, x, y, z, n, cam, P);
  {
    TimeScope ts(ctx, "narf_desc", true);
    k_narf_desc<<<(unsigned)nk, 64, 0, st>>>(I, P, pixel_idx, prm.support_size, prm.rotation_invariant != 0, slot_desc,
                                            slot_pose, counts, stats);
    check_launch("k_narf_desc");
    k_count_scan<<<1, 1024, 0, st>>>(counts, nk, offsets, d_n_out);
    check_launch("k_count_scan");
    k_narf_desc_compact<<<(unsigned)nk, 64, 0, st>>>(slot_desc, slot_pose, counts, offsets, desc, pose, row_key, cap);
    check_launch("k_narf_desc_compact");
  }
  report_post(ctx, kRepNarfDesc, stats);
}

void narf_desc_report(pfx_ctx* ctx, const int* h) {
  ctx->stats["narf_desc_rows"] = h[kWordRows];
  ctx->stats["narf_desc_invalid_pixels"] = h[kWordInvalid];
  ctx->stats["narf_desc_pose_failed"] = h[kWordPoseFailed];
  ctx->stats["narf_desc_fallback_normals"] = h[kWordFallback];
  ctx->stats["narf_desc_ring_max"] = h[kWordRingMax];
  ctx->stats["narf_desc_background_cells"] = h[kWordBackground];
}

void point_indices_dev(pfx_ctx* ctx, const float* x, const float* y, const float* z, int64_t n, const float* kx,
                       const float* ky, const float* kz, int64_t nk, float tol, int32_t* out, int64_t cap,
                       int64_t* d_n_out) {
  hipStream_t st = ctx->stream;
  if (nk == 0 || n == 0) {
    PFX_HIP(hipMemsetAsync(d_n_out, 0, sizeof(int64_t), st));
    return;
  }
  // the cloud in chunks of whole tiles, about 2048 points each, as long as the counts stay small
  int64_t chunks = std::max<int64_t>(1, std::min<int64_t>(ceil_div(n, 8 * kIndexTile), (int64_t(1) << 22) / nk));
  chunks = std::min<int64_t>(chunks, 65535);
  const int64_t len = ceil_div(ceil_div(n, chunks), kIndexTile) * kIndexTile;
  chunks = ceil_div(n, len);
  int* counts = ctx->buf("point_indices_counts").as<int>((size_t)(nk * chunks));
  int64_t* offsets = ctx->buf("point_indices_offsets").as<int64_t>((size_t)(nk * chunks));
  TimeScope ts(ctx, "point_indices", true);
  const dim3 grid((unsigned)ceil_div(nk, 64), (unsigned)chunks);
  k_point_indices<false><<<grid, 64, 0, st>>>(x, y, z, n, len, kx, ky, kz, nk, tol, counts, offsets, out, cap);
  check_launch("k_point_indices (count)");
  k_count_scan<<<1, 1024, 0, st>>>(counts, nk * chunks, offsets, d_n_out);
  check_launch("k_count_scan");
  k_point_indices<true><<<grid, 64, 0, st>>>(x, y, z, n, len, kx, ky, kz, nk, tol, counts, offsets, out, cap);
  check_launch("k_point_indices (write)");
}

}  // namespace pfx
