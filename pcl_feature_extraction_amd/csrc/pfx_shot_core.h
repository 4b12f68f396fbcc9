// pfx_shot_core.h -- the device code pfx_shot.hip (SHOT-352) and pfx_shot_color.hip (SHOT-1344) share:
// the interpolation geometry (shot_updates), the local reference frame phases, the per-bin
// ordered histogram binning, normalizeHistogram, and the split path's search + LRF kernels.
#pragma once
#include <cstdlib>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "pfx_eigen3.h"
#include "pfx_neighbors.h"

namespace pfx {
namespace {

#ifdef PFX_SHOT_PROFILE
// phase cycles (thread 0 of each workgroup): [7] sequential normalisations, [8] normalisation
// cycles; k_shot_lrf: [10] search + sort, [11] records, [12] LRF chains, [13] queries
__device__ unsigned long long g_shot_prof[16];
#define SPROF_T(v) long long v = (threadIdx.x == 0) ? clock64() : 0
#define SPROF_ADD(i, a, b) if (threadIdx.x == 0) atomicAdd(&g_shot_prof[i], (unsigned long long)((b) - (a)))
#else
#define SPROF_T(v)
#define SPROF_ADD(i, a, b)
#endif

#ifndef PFX_SHOT_GRID_MUL  // (A/B: the split kernels' grids, x this)
#define PFX_SHOT_GRID_MUL 4
#endif
constexpr int kCapSmall = 2048;  // sorted-neighbour capacity of the first pass (LDS keys, 5 WG/CU)
constexpr int kCap = 16384;      // second pass for the longer lists (1 WG/CU)
constexpr int kChunk = 256;   // neighbours staged per chunk
constexpr int kLen = 352, kBins = 10;
constexpr int kBinsC = 30, kLenC = 32 * (kBinsC + 1), kLenAll = kLen + kLenC;  // SHOT-1344's colour block
constexpr double kRad45 = 0.78539816339744830961566084581988;
constexpr double kRad90 = 1.5707963267948966192313216916398;
constexpr double kRad135 = 2.3561944901923449288469825374596;
constexpr double kRadPi78 = 2.7488935718910690836548129603691;

// the five (bin, value) updates of one neighbour (SHOTEstimation::interpolateSingleChannel with
// the bin distance of createBinDistanceShape); bin -1 = no update.  Order = PCL's order.
// COLOR (SHOTColorEstimation::interpolateDoubleChannel): every update mirrored on the colour
// block from the colour bin distance binDistC -- cbins are bins of that block (descriptor index
// - kLen), kBinsC + 1 slots per volume; the same radial, inclination and azimuth distances.
template <bool COLOR = false>
__device__ __forceinline__ void shot_updates(f3 delta, double distance, double binDist, f3 fx, f3 fy, f3 fz,
                                             double radius, int bins[5], float vals[5], double binDistC = 0.0,
                                             int* cbins = nullptr, float* cvals = nullptr) {
  for (int s = 0; s < 5; ++s) bins[s] = -1;
  if (COLOR)
    for (int s = 0; s < 5; ++s) cbins[s] = -1;
  const double radius3_4 = (radius * 3) / 4, radius1_4 = radius / 4, radius1_2 = radius / 2;
  double xIn = dot4(delta, fx), yIn = dot4(delta, fy), zIn = dot4(delta, fz);
  if (fabs(yIn) < 1E-30) yIn = 0;
  if (fabs(xIn) < 1E-30) xIn = 0;
  if (fabs(zIn) < 1E-30) zIn = 0;
  const int bit4 = ((yIn > 0) || ((yIn == 0.0) && (xIn < 0))) ? 1 : 0;
  const int bit3 = ((xIn > 0) || ((xIn == 0.0) && (yIn > 0))) ? !bit4 : bit4;
  int desc_index = ((bit4 << 3) + (bit3 << 2)) << 1;
  if ((xIn * yIn > 0) || (xIn == 0.0))
    desc_index += (fabs(xIn) >= fabs(yIn)) ? 0 : 4;
  else
    desc_index += (fabs(xIn) > fabs(yIn)) ? 4 : 0;
  desc_index += zIn > 0 ? 1 : 0;
  desc_index += (distance > radius1_2) ? 2 : 0;
  const int step_index = (int)floor(binDist + 0.5);
  const int volume_index = desc_index * (kBins + 1);
  binDist -= step_index;
  double intWeight = (1 - fabs(binDist));
  if (binDist > 0) {
    bins[0] = volume_index + ((step_index + 1) % kBins);
    vals[0] = (float)binDist;
  } else {
    bins[0] = volume_index + ((step_index - 1 + kBins) % kBins);
    vals[0] = -(float)binDist;
  }
  int step_c = 0;
  double intWeightC = 0.0;
  if (COLOR) {
    step_c = (int)floor(binDistC + 0.5);
    const int volume_c = desc_index * (kBinsC + 1);
    binDistC -= step_c;
    intWeightC = (1 - fabs(binDistC));
    if (binDistC > 0) {
      cbins[0] = volume_c + ((step_c + 1) % kBinsC);
      cvals[0] = (float)binDistC;
    } else {
      cbins[0] = volume_c + ((step_c - 1 + kBinsC) % kBinsC);
      cvals[0] = -(float)binDistC;
    }
  }
  if (distance > radius1_2) {
    const double rd = (distance - radius3_4) / radius1_2;
    if (distance > radius3_4) {
      intWeight += 1 - rd;
      if (COLOR) intWeightC += 1 - rd;
    } else {
      intWeight += 1 + rd;
      bins[1] = (desc_index - 2) * (kBins + 1) + step_index;
      vals[1] = -(float)rd;
      if (COLOR) {
        intWeightC += 1 + rd;
        cbins[1] = (desc_index - 2) * (kBinsC + 1) + step_c;
        cvals[1] = vals[1];
      }
    }
  } else {
    const double rd = (distance - radius1_4) / radius1_2;
    if (distance < radius1_4) {
      intWeight += 1 + rd;
      if (COLOR) intWeightC += 1 + rd;
    } else {
      intWeight += 1 - rd;
      bins[1] = (desc_index + 2) * (kBins + 1) + step_index;
      vals[1] = (float)rd;
      if (COLOR) {
        intWeightC += 1 - rd;
        cbins[1] = (desc_index + 2) * (kBinsC + 1) + step_c;
        cvals[1] = vals[1];
      }
    }
  }
  double ic = zIn / distance;
  if (ic < -1.0) ic = -1.0;
  if (ic > 1.0) ic = 1.0;
  const double incl = acos(ic);
  if (incl > kRad90 || (fabs(incl - kRad90) < 1e-30 && zIn <= 0)) {
    const double idist = (incl - kRad135) / kRad90;
    if (incl > kRad135) {
      intWeight += 1 - idist;
      if (COLOR) intWeightC += 1 - idist;
    } else {
      intWeight += 1 + idist;
      bins[2] = (desc_index + 1) * (kBins + 1) + step_index;
      vals[2] = -(float)idist;
      if (COLOR) {
        intWeightC += 1 + idist;
        cbins[2] = (desc_index + 1) * (kBinsC + 1) + step_c;
        cvals[2] = vals[2];
      }
    }
  } else {
    const double idist = (incl - kRad45) / kRad90;
    if (incl < kRad45) {
      intWeight += 1 + idist;
      if (COLOR) intWeightC += 1 + idist;
    } else {
      intWeight += 1 - idist;
      bins[2] = (desc_index - 1) * (kBins + 1) + step_index;
      vals[2] = (float)idist;
      if (COLOR) {
        intWeightC += 1 - idist;
        cbins[2] = (desc_index - 1) * (kBinsC + 1) + step_c;
        cvals[2] = vals[2];
      }
    }
  }
  if (yIn != 0.0 || xIn != 0.0) {
    const double azimuth = atan2(yIn, xIn);
    const int sel = desc_index >> 2;
    double ad = (azimuth - (-kRadPi78 + kRad45 * sel)) / kRad45;
    ad = fmax(-0.5, fmin(ad, 0.5));
    if (ad > 0) {
      intWeight += 1 - ad;
      bins[3] = ((desc_index + 4) % 32) * (kBins + 1) + step_index;
      vals[3] = (float)ad;
      if (COLOR) {
        intWeightC += 1 - ad;
        cbins[3] = ((desc_index + 4) % 32) * (kBinsC + 1) + step_c;
        cvals[3] = vals[3];
      }
    } else {
      intWeight += 1 + ad;
      bins[3] = ((desc_index - 4 + 32) % 32) * (kBins + 1) + step_index;
      vals[3] = -(float)ad;
      if (COLOR) {
        intWeightC += 1 + ad;
        cbins[3] = ((desc_index - 4 + 32) % 32) * (kBinsC + 1) + step_c;
        cvals[3] = vals[3];
      }
    }
  }
  bins[4] = volume_index + step_index;
  vals[4] = (float)intWeight;
  if (COLOR) {
    cbins[4] = desc_index * (kBinsC + 1) + step_c;
    cvals[4] = (float)intWeightC;
  }
}


// the seven distinct LRF chains: cov (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) and the weight sum
constexpr int kChains = 7;
constexpr int kMaskWords = kChunk / 64;

// the per-chunk bucketing state of a LEN-bin histogram (hist_chunk); thread t owns the bins
// t, t + 256, ...: kPer of them
template <int LEN>
struct HistUpd {
  static constexpr int kPer = (LEN + 255) / 256;
  uint64_t mask[kMaskWords][LEN];  // which neighbours of the chunk hit each bin (word-major:
                                   // the bin owners' reads are lane-consecutive)
  int off[LEN + 1];                // bucket offsets (exclusive scan of the hit counts)
  int seg[4 * kPer];               // the counts' scan: totals of the 64-bin segments
  uint32_t pw[LEN];                // per bin: hits from waves < 1, < 2, < 3 (a byte each)
  float val[5 * kChunk];           // the chunk's update values bucketed by bin, neighbour order
};

struct ShotLds {
  union {
    double lrf[kChains][kChunk];  // per-neighbour chain terms of one chunk (0 for invalid ones)
    HistUpd<kLen> upd;
    alignas(16) float hist[kLen];  // the finished histogram (written once the chunks are binned)
  };
  double cov[10];
  double axes[6];  // v1 (x axis), v3 (z axis)
  int lrf_l[4];    // normalisation: per-wave smallest lsb exponent and largest square
  float lrf_m[4];
  float rf[9];
  int n_invalid, zero_prefix, plusT, plusN, ok;
};

// ---- the phases of one query, shared by the fused and the split kernels ----

// A query's neighbour j for the frame and the histogram: its offset from the query (the float
// subtraction PCL's `delta` is) with its d2, and its normal.  NbKeys: from the FLANN keys and the
// caller-order arrays (the fused kernel); NbRecs: from the records k_shot_lrf writes (one float4
// of offset + d2 and one of normal per neighbour, two planes of kCapSmall per query), so the
// split kernels read a neighbour with one coalesced load instead of a key, then its point.
struct NbKeys {
  const uint64_t* keys;
  const float *ux, *uy, *uz, *nx, *ny, *nz;
  float cx, cy, cz;
  __device__ __forceinline__ float4 pt(int j) const {
    const uint64_t key = keys[j];
    const int32_t p = key_idx(key);
    return make_float4(ux[p] - cx, uy[p] - cy, uz[p] - cz, key_d2(key));
  }
  __device__ __forceinline__ float3 nrm(int j) const {
    const int32_t p = key_idx(keys[j]);
    return make_float3(nx[p], ny[p], nz[p]);
  }
};
struct NbRecs {
  const float4* __restrict__ pts;   // {dx, dy, dz, d2}
  const float4* __restrict__ nrms;  // {nx, ny, nz, 0}
  __device__ __forceinline__ float4 pt(int j) const { return pts[j]; }
  __device__ __forceinline__ float3 nrm(int j) const {
    const float4 v = nrms[j];
    return make_float3(v.x, v.y, v.z);
  }
};
// (a copy of the query: a zero offset -- a difference of finite floats is zero only when they are
// equal)
__device__ __forceinline__ bool nb_self(const float4& c) { return c.x == 0.0f && c.y == 0.0f && c.z == 0.0f; }

// SHOTLocalReferenceFrameEstimation's weighted double covariance over keys[0..k): S.cov (3x3
// row-major + the weight sum at [9]), S.n_invalid (copies of the query), S.zero_prefix.
// Every thread forms its neighbour's chain terms dist * (v_a * v_b) and dist exactly as the
// reference loop does; lanes 0..6 then add them in neighbour order (the only sequential part).
// An invalid neighbour (a copy of the query) contributes +0.0, which leaves a chain unchanged.
template <class Lds, class Src>
__device__ __forceinline__ void shot_lrf(Lds& S, double (*lrf)[kChunk], const Src& src, int k, double radius) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    S.n_invalid = 0; S.zero_prefix = 0; S.plusT = 0; S.plusN = 0;
  }
  double acc = 0.0;
  // the next chunk's neighbour is loaded while lanes 0..6 sum the current one
  float4 c_n = tid < k ? src.pt(tid) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < k; c0 += kChunk) {
    const int m = min(kChunk, k - c0);
    const float4 c = c_n;
    if (c0 + kChunk + tid < k) c_n = src.pt(c0 + kChunk + tid);
    __syncthreads();
    if (tid < m) {
      const bool valid = !nb_self(c);
      const double vx = (double)c.x, vy = (double)c.y, vz = (double)c.z;
      const double dist = radius - sqrt((double)c.w);
      lrf[0][tid] = valid ? dist * (vx * vx) : 0.0;
      lrf[1][tid] = valid ? dist * (vx * vy) : 0.0;
      lrf[2][tid] = valid ? dist * (vx * vz) : 0.0;
      lrf[3][tid] = valid ? dist * (vy * vy) : 0.0;
      lrf[4][tid] = valid ? dist * (vy * vz) : 0.0;
      lrf[5][tid] = valid ? dist * (vz * vz) : 0.0;
      lrf[6][tid] = valid ? dist : 0.0;
      if (!valid) atomicAdd(&S.n_invalid, 1);
      if (c.w == 0.0f) atomicAdd(&S.zero_prefix, 1);
    }
    __syncthreads();
    if (tid < kChains) {  // (32 terms loaded per round: one LDS latency per 32 dependent adds)
      const double* row = lrf[tid];
      int t = 0;
      for (; t + 32 <= m; t += 32) {
        double2 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = *reinterpret_cast<const double2*>(row + t + 2 * u);
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          acc = acc + v[u].x;
          acc = acc + v[u].y;
        }
      }
      for (; t < m; ++t) acc = acc + row[t];
    }
  }
  __syncthreads();
  if (tid < kChains) {  // chain -> cov[3a + b] (v_a v_b == v_b v_a exactly), cov[9] = weight sum
    constexpr int kSlot[kChains][2] = {{0, 0}, {1, 3}, {2, 6}, {4, 4}, {5, 7}, {8, 8}, {9, 9}};
    S.cov[kSlot[tid][0]] = acc;
    S.cov[kSlot[tid][1]] = acc;
  }
  __syncthreads();
}

// `cov_m /= sum` (Eigen 3.2: times the reciprocal), SelfAdjointEigenSolver<Matrix3d>: axes = the
// x (largest) and z (smallest) eigenvectors; false when the frame is undefined (PCL: NaN rows)
__device__ __forceinline__ bool shot_eigen(const double cov[10], int valid, double axes[6]) {
  if (valid < 5) return false;
  double ev[3], V[3][3];
  const double inv = 1.0 / cov[9];
  eigen_selfadjoint3<true>(cov[0] * inv, cov[3] * inv, cov[4] * inv, cov[6] * inv, cov[7] * inv, cov[8] * inv, ev,
                           V);
  if (!(isfinite(ev[0]) && isfinite(ev[1]) && isfinite(ev[2]))) return false;
  for (int i = 0; i < 3; ++i) { axes[i] = V[2][i]; axes[3 + i] = V[0][i]; }
  return true;
}

// sign disambiguation of S.axes over the valid neighbours, then S.rf (x, y = z cross x, z)
template <class Lds, class Src>
__device__ __forceinline__ void shot_frame(Lds& S, const Src& src, int k, int valid) {
  const int tid = threadIdx.x, lane = tid & 63;
  {
    const double v1x = S.axes[0], v1y = S.axes[1], v1z = S.axes[2];
    const double v3x = S.axes[3], v3y = S.axes[4], v3z = S.axes[5];
    int cT = 0, cN = 0;
    for (int j0 = tid; j0 < k; j0 += 4 * 256) {  // (four neighbours per thread in flight)
      float4 c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int j = j0 + 256 * u;
        c[u] = src.pt(j < k ? j : j0);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (j0 + 256 * u >= k || nb_self(c[u])) continue;
        const double vx = (double)c[u].x, vy = (double)c[u].y, vz = (double)c[u].z;
        if (((vx * v1x + vy * v1y) + vz * v1z) + 0.0 >= 0) ++cT;
        if (((vx * v3x + vy * v3y) + vz * v3z) + 0.0 >= 0) ++cN;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { cT += __shfl_xor(cT, o); cN += __shfl_xor(cN, o); }
    if (lane == 0) { atomicAdd(&S.plusT, cT); atomicAdd(&S.plusN, cN); }
  }
  __syncthreads();
  if (tid == 0) {
    double ax[2][3] = {{S.axes[0], S.axes[1], S.axes[2]}, {S.axes[3], S.axes[4], S.axes[5]}};
    const int counts[2] = {S.plusT, S.plusN};
    // the valid neighbours in order: the d2 == 0 prefix holds every invalid one
    const int zp = S.zero_prefix;
    int valid_in_prefix = 0;
    for (int j = 0; j < zp; ++j)
      if (!nb_self(src.pt(j))) ++valid_in_prefix;
    for (int w = 0; w < 2; ++w) {
      int plus = 2 * counts[w] - valid;
      if (plus == 0) {
        const int median = valid / 2;
        for (int i = -2; i <= 2; ++i) {
          const int ne = median - i;
          int j;
          if (ne < valid_in_prefix) {
            int seen = -1;
            for (j = 0; j < zp; ++j)
              if (!nb_self(src.pt(j)) && ++seen == ne) break;
          } else {
            j = zp + (ne - valid_in_prefix);
          }
          const float4 c = src.pt(j);
          const double vx = (double)c.x, vy = (double)c.y, vz = (double)c.z;
          if (((vx * ax[w][0] + vy * ax[w][1]) + vz * ax[w][2]) + 0.0 > 0) ++plus;
        }
        if (plus < 3)
          for (int c = 0; c < 3; ++c) ax[w][c] *= -1;
      } else if (plus < 0) {
        for (int c = 0; c < 3; ++c) ax[w][c] *= -1;
      }
    }
    const f3 x = mk3((float)ax[0][0], (float)ax[0][1], (float)ax[0][2]);
    const f3 z = mk3((float)ax[1][0], (float)ax[1][1], (float)ax[1][2]);
    const f3 y = cross3(z, x);
    S.rf[0] = x.x; S.rf[1] = x.y; S.rf[2] = x.z;
    S.rf[3] = y.x; S.rf[4] = y.y; S.rf[5] = y.z;
    S.rf[6] = z.x; S.rf[7] = z.y; S.rf[8] = z.z;
  }
}

// the LDS of the split path's frame kernels (shot_frame alone)
struct FrameLds {
  double axes[6];
  float rf[9];
  int zero_prefix, plusT, plusN;
};

// exponent of the least significant set bit of a finite nonzero float
__device__ __forceinline__ int lsb_exp_f(float v) {
  const uint32_t b = __float_as_uint(v);
  const int e = (int)((b >> 23) & 0xff);
  const uint32_t m = b & 0x7fffffu;
  const uint32_t full = e ? (m | 0x800000u) : m;
  return (e ? e : 1) - 150 + __builtin_ctz(full);
}

// The histogram's per-chunk binning.  Each neighbour adds to at most one bin per update statement
// (its <= 5 bins are distinct), so PCL's sequential order restricted to one bin is neighbour
// order.  Per chunk of m neighbours (one per thread): hit masks per bin -> counts -> offsets ->
// every update written to its bin's bucket at its rank among the bin's hits (a stable counting
// sort) -> each bin's owner (thread t: bins t, t + 256, ...; h[j] is bin t + 256 j) adds its
// bucket in order.  The masks must be zero on entry (they are left zero).
template <int LEN>
__device__ __forceinline__ void hist_chunk(HistUpd<LEN>& U, int m, const int bins[5], const float vals[5],
                                           float (&h)[HistUpd<LEN>::kPer]) {
  constexpr int P = HistUpd<LEN>::kPer;
  const int tid = threadIdx.x, lane = tid & 63;
  SPROF_T(h0t);
  if (tid < m) {
    const uint64_t bit = 1ull << (tid & 63);
#pragma unroll
    for (int s = 0; s < 5; ++s)
      if (bins[s] >= 0) atomicOr(reinterpret_cast<unsigned long long*>(&U.mask[tid >> 6][bins[s]]), bit);
  }
  __syncthreads();
  SPROF_T(h1t);
  SPROF_ADD(0, h0t, h1t);
  // hit counts -> exclusive offsets: thread t counts the bins it sums below, wave scans, the
  // 4 P segment totals through LDS
  static_assert(kMaskWords == 4, "one byte per lower wave");
  int c[P], inc[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int b = tid + 256 * j;
    c[j] = 0;
    if (256 * (j + 1) <= LEN || b < LEN) {
      uint32_t pw = 0;
#pragma unroll
      for (int w = 0; w < kMaskWords; ++w) {
        c[j] += __popcll(U.mask[w][b]);
        if (w < kMaskWords - 1) pw |= (uint32_t)c[j] << (8 * w);
      }
      U.pw[b] = pw;
    }
    inc[j] = c[j];
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int y[P];
#pragma unroll
    for (int j = 0; j < P; ++j) y[j] = __shfl_up(inc[j], o);
    if (lane >= o) {
#pragma unroll
      for (int j = 0; j < P; ++j) inc[j] += y[j];
    }
  }
  const int wv = tid >> 6;
  if (lane == 63) {
#pragma unroll
    for (int j = 0; j < P; ++j) U.seg[4 * j + wv] = inc[j];
  }
  __syncthreads();
  {
    int before = 0;  // hits of the bins below 256 j
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int b = tid + 256 * j;
      int p = before;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int sv = U.seg[4 * j + v];
        before += sv;
        if (v < wv) p += sv;
      }
      if (256 * (j + 1) <= LEN || b < LEN) U.off[b] = p + inc[j] - c[j];
    }
  }
  __syncthreads();
  SPROF_T(h2t);
  SPROF_ADD(1, h1t, h2t);
  if (tid < m) {  // scatter: rank = hits of the bin from lower neighbours of the chunk
    const int wq = tid >> 6;
    const uint64_t below = lanemask_lt();
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int bb = bins[s];
      if (bb < 0) continue;
      int r = __popcll(U.mask[wq][bb] & below);
      if (wq) r += (int)((U.pw[bb] >> (8 * (wq - 1))) & 0xffu);
      U.val[U.off[bb] + r] = vals[s];
    }
  }
  __syncthreads();
  SPROF_T(h3t);
  SPROF_ADD(2, h2t, h3t);
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int b = tid + 256 * j;
    if (256 * (j + 1) <= LEN || b < LEN) {
#pragma unroll
      for (int w = 0; w < kMaskWords; ++w) U.mask[w][b] = 0;  // ready for the next chunk
      const float* v = U.val + U.off[b];
      float a = h[j];
      int i = 0;
      for (; i + 4 <= c[j]; i += 4) {
        const float a0 = v[i], a1 = v[i + 1], a2 = v[i + 2], a3 = v[i + 3];
        a = a + a0; a = a + a1; a = a + a2; a = a + a3;
      }
      for (; i < c[j]; ++i) a = a + v[i];
      h[j] = a;
    }
  }
  __syncthreads();
  SPROF_T(h4t);
  SPROF_ADD(3, h3t, h4t);
}

template <int LEN>
__device__ __forceinline__ void hist_clear(HistUpd<LEN>& U) {
  for (int i = threadIdx.x; i < LEN; i += 256)
    for (int w = 0; w < kMaskWords; ++w) U.mask[w][i] = 0;
  __syncthreads();
}

// normalizeHistogram of the LEN entries in S.hist (h[j]: this thread's copy of entry
// t + 256 j, 0 past the end) and the outputs (rfo: the frame rows, nullable)
template <int LEN, class Lds>
__device__ __forceinline__ void hist_normalize(Lds& S, const float (&h)[(LEN + 255) / 256], float* __restrict__ d,
                                               float* __restrict__ rfo) {
  constexpr int P = (LEN + 255) / 256;
  static_assert(LEN % 16 == 0, "the sequential loop reads 16 entries a round");
  const int tid = threadIdx.x, lane = tid & 63;
  // normalizeHistogram: acc_norm += shot[j] * shot[j] (float squares, double sum, in bin order).
  // The squares are multiples of 2^L (L the smallest least-significant-bit exponent among the
  // nonzero ones) and non-negative, so when LEN x the largest stays below 2^(L + 53) every
  // partial sum is exact and any order gives PCL's value: a parallel sum; otherwise one lane
  // runs the sequential loop.
  {
    float sq[P];
#pragma unroll
    for (int j = 0; j < P; ++j) sq[j] = (256 * (j + 1) <= LEN || tid + 256 * j < LEN) ? h[j] * h[j] : 0.0f;
    double part = (double)sq[0];
    float mx = sq[0];
#pragma unroll
    for (int j = 1; j < P; ++j) {
      part += (double)sq[j];
      mx = fmaxf(mx, sq[j]);
    }
    int L = 1 << 20;
#pragma unroll
    for (int o = 0; o < P; ++o)
      if (sq[o] != 0.0f && isfinite(sq[o])) L = min(L, lsb_exp_f(sq[o]));
      else if (!(sq[o] == 0.0f)) L = -(1 << 20);  // non-finite: the sequential loop decides
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      part += __shfl_xor(part, o);
      mx = fmaxf(mx, __shfl_xor(mx, o));
      L = min(L, __shfl_xor(L, o));
    }
    if (lane == 0) {
      S.axes[tid >> 6] = part;  // (axes are dead here: four wave partials)
      S.lrf_l[tid >> 6] = L;
      S.lrf_m[tid >> 6] = mx;
    }
    __syncthreads();
    if (tid == 0) {
      const double tot = (S.axes[0] + S.axes[1]) + (S.axes[2] + S.axes[3]);
      const int Lm = min(min(S.lrf_l[0], S.lrf_l[1]), min(S.lrf_l[2], S.lrf_l[3]));
      const float mm = fmaxf(fmaxf(S.lrf_m[0], S.lrf_m[1]), fmaxf(S.lrf_m[2], S.lrf_m[3]));
      double acc_norm;
      if (mm == 0.0f) {
        acc_norm = 0.0;
      } else if (Lm > -(1 << 19) && (double)mm * LEN < ldexp(1.0, Lm + 53)) {
        acc_norm = tot;
      } else {
        acc_norm = 0;
        // (PCL's order; the squares read 16 at a time, so only the additions are sequential)
        for (int j = 0; j < LEN; j += 16) {
          float4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(S.hist + j + 4 * u);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            acc_norm += v[u].x * v[u].x;
            acc_norm += v[u].y * v[u].y;
            acc_norm += v[u].z * v[u].z;
            acc_norm += v[u].w * v[u].w;
          }
        }
#ifdef PFX_SHOT_PROFILE
        atomicAdd(&g_shot_prof[7], 1ull);
#endif
      }
      S.cov[0] = sqrt(acc_norm);
    }
    __syncthreads();
  }
  const float nrm = (float)S.cov[0];
  for (int i = tid; i < LEN; i += 256) d[i] = S.hist[i] / nrm;
  if (rfo && tid < 9) rfo[tid] = S.rf[tid];
  __syncthreads();
}

// the finished bins (h[j]: bin t + 256 j) -> S.hist, normalizeHistogram, the outputs
template <int LEN, class Lds>
__device__ __forceinline__ void hist_finish(Lds& S, const float (&h)[(LEN + 255) / 256], float* __restrict__ d,
                                            float* __restrict__ rfo) {
  const int tid = threadIdx.x;
  SPROF_T(pe0);
#pragma unroll
  for (int j = 0; j < (LEN + 255) / 256; ++j)
    if (256 * (j + 1) <= LEN || tid + 256 * j < LEN) S.hist[tid + 256 * j] = h[j];
  __syncthreads();
  hist_normalize<LEN>(S, h, d, rfo);
  SPROF_T(pe1);
  SPROF_ADD(8, pe0, pe1);
}

// a neighbour's (<= 5) histogram updates from the frame S.rf (fx, fy, fz)
__device__ __forceinline__ void nb_updates(const float4& c, const float3& nv, const f3& fx, const f3& fy,
                                           const f3& fz, double radius, int bins[5], float vals[5]) {
#pragma unroll
  for (int s = 0; s < 5; ++s) bins[s] = -1;
  const double distance = sqrt((double)c.w);
  if (isfinite(nv.x) && isfinite(nv.y) && isfinite(nv.z) && !(fabs(distance - 0.0) < 1E-15)) {
    double cosd = dot4(mk3(nv.x, nv.y, nv.z), fz);
    if (cosd > 1.0) cosd = 1.0;
    if (cosd < -1.0) cosd = -1.0;
    const double binDist = ((1.0 + cosd) * kBins) / 2;
    shot_updates(mk3(c.x, c.y, c.z), distance, binDist, fx, fy, fz, radius, bins, vals);
  }
}

// the SHOT histogram from S.rf, normalizeHistogram, outputs (the fused kernel: updates computed
// chunk by chunk)
template <class Src>
__device__ __forceinline__ void shot_hist(ShotLds& S, const Src& src, int k, double radius, float* __restrict__ d,
                                          float* __restrict__ rfo) {
  const int tid = threadIdx.x;
  float h[2] = {0.0f, 0.0f};
  hist_clear(S.upd);
  const f3 fx = mk3(S.rf[0], S.rf[1], S.rf[2]), fy = mk3(S.rf[3], S.rf[4], S.rf[5]),
           fz = mk3(S.rf[6], S.rf[7], S.rf[8]);
  for (int c0 = 0; c0 < k; c0 += kChunk) {
    const int m = min(kChunk, k - c0);
    int bins[5];
    float vals[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) bins[s] = -1;
    if (tid < m) nb_updates(src.pt(c0 + tid), src.nrm(c0 + tid), fx, fy, fz, radius, bins, vals);
    hist_chunk(S.upd, m, bins, vals, h);
  }
  hist_finish<kLen>(S, h, d, rfo);
}

// the split kernels' update records: one 32-B record per neighbour, {bin0 | bin1 << 16,
// bin2 | bin3 << 16, bin4 (low half), val0} + {val1, val2, val3, val4} (bins as int16, -1: none)
__device__ __forceinline__ void upd_pack(const int bins[5], const float vals[5], uint4& a, float4& b) {
  auto h = [](int v) { return (uint32_t)(uint16_t)(int16_t)v; };
  a = make_uint4(h(bins[0]) | (h(bins[1]) << 16), h(bins[2]) | (h(bins[3]) << 16), h(bins[4]),
                 __float_as_uint(vals[0]));
  b = make_float4(vals[1], vals[2], vals[3], vals[4]);
}
__device__ __forceinline__ void upd_unpack(const uint4& a, const float4& b, int bins[5], float vals[5]) {
  auto s = [](uint32_t v) { return (int)(int16_t)(uint16_t)v; };
  bins[0] = s(a.x); bins[1] = s(a.x >> 16); bins[2] = s(a.y); bins[3] = s(a.y >> 16); bins[4] = s(a.z);
  vals[0] = __uint_as_float(a.w); vals[1] = b.x; vals[2] = b.y; vals[3] = b.z; vals[4] = b.w;
}

template <int LEN = kLen>
__device__ __forceinline__ void shot_nan(float* __restrict__ d, float* __restrict__ rfo) {
  for (int i = threadIdx.x; i < LEN; i += 256) d[i] = __builtin_nanf("");
  if (threadIdx.x < 9) rfo[threadIdx.x] = __builtin_nanf("");
}

// the split kernels' views of the surface: caller index -> cell-sorted position, and the normals
// in cell order.  Two coalesced-read passes (the inverse permutation, then each caller-order
// normal written to its cell position) instead of one pass gathering three 4-byte normal
// components through the permutation (283 MB fetched per 1M points: a cache line per component).
// (round 5: the records gathered from caller-order packed copies instead -- one global round,
// not two -- measured 0.92 -> 0.97 ms: the cell-sorted gathers' locality wins)
__global__ void k_shot_ipos(const int32_t* __restrict__ perm, int64_t n, int32_t* __restrict__ ipos) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) ipos[perm[i]] = (int32_t)i;
}

// ---- split form: the single-lane eigen solve off the workgroups' critical path ----
// Per query state between the three kernels.  status: 0 frame pending / defined, 1 done (NaN
// written: non-finite query or no frame), 2 over the split capacity (the fused kernel's).
struct ShotQuery {
  double cov[10];
  double axes[6];
  int k, n_invalid, zero_prefix, status;
};

// the LDS of the LRF phase alone (kernel A; its chain terms live in the sort's scratch half of
// the keys, free once the keys are sorted: 34 KB a workgroup, four per CU)
struct LrfLds {
  double cov[10];
  int n_invalid, zero_prefix, plusT, plusN;
};

// A: sort + LRF covariance; the neighbour records (NbRecs: offset + d2, normal) kept in global
// memory for C (two planes of kCapSmall float4 per query).  LEN: the descriptor's row length
// (the NaN rows).  A normal record keeps snp's fourth component (0 from k_shot_prep; SHOT-1344's
// records carry the point's cell position there).
template <int LEN>
__global__ void __launch_bounds__(256) k_shot_lrf(GridView g, const float* __restrict__ qx,
                                                  const float* __restrict__ qy, const float* __restrict__ qz,
                                                  int64_t base, int64_t nq, int32_t* __restrict__ over,
                                                  int* __restrict__ n_over,
                                                  double radius, float* __restrict__ desc, float* __restrict__ rf_out,
                                                  float4* __restrict__ grec, ShotQuery* __restrict__ sq,
                                                  const int32_t* __restrict__ ipos, const float4* __restrict__ snp,
                                                  unsigned long long* __restrict__ nbr,
                                                  const int32_t* __restrict__ order) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // kCapSmall + kCapSmall scratch
  __shared__ LrfLds S;
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const float rr = (float)(radius * radius);
  // the queries in cell order (`order`, round 6), each XCD a contiguous eighth of them (blocks b
  // and b + 8 share an XCD): neighbouring queries' candidate blocks then come from the same L2
  // instead of each query scanning its r-block from HBM (r05: 2.0 GB fetched for 0.24 GB of
  // algorithmic bytes)
  int64_t l0 = blockIdx.x, lend = nq, lstep = gridDim.x;
  if (order && (gridDim.x & 7) == 0) {
    const int64_t per = (nq + 7) >> 3;
    l0 = (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    lend = min(nq, (int64_t)((blockIdx.x & 7) + 1) * per);
    lstep = gridDim.x >> 3;
  }
  for (int64_t l = l0; l < lend; l += lstep) {  // l: index in the batch, q: caller's
    const int64_t q = order ? order[base + l] : base + l;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    if (!(isfinite(cx) && isfinite(cy) && isfinite(cz))) {
      shot_nan<LEN>(desc + q * LEN, rf_out + q * 9);
      if (tid == 0) sq[l].status = 1;
      continue;
    }
    SPROF_T(l0);
    const int k = sorted_neighbors_bucketed(g, cx, cy, cz, rr, keys, keys + kCapSmall, kCapSmall, &s_count, SB);
    if (k > kCapSmall) {
      if (tid == 0) {
        over[atomicAdd(n_over, 1)] = (int32_t)q;
        sq[l].status = 2;
      }
      continue;
    }
    if (tid == 0) atomicAdd(nbr, (unsigned long long)k);
    SPROF_T(l1);
    SPROF_ADD(10, l0, l1);
    SPROF_ADD(13, 0, 1);
    // the keys (d2, caller index) in FLANN order -> the neighbour records, same order (read back
    // by this thread in shot_lrf, and by the frame and histogram kernel)
    // (four neighbours per thread in flight: two dependent global rounds for the whole list)
    float4* rp = grec + l * 2 * kCapSmall;
    for (int i0 = tid; i0 < k; i0 += 4 * 256) {
      uint64_t key[4];
      int32_t pos[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        key[u] = keys[min(i0 + 256 * u, k - 1)];
        pos[u] = ipos[key_idx(key[u])];
      }
      float4 c[4], nv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        c[u] = g.sp[pos[u]];
        nv[u] = snp[pos[u]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + 256 * u;
        if (i < k) {
          rp[i] = make_float4(c[u].x - cx, c[u].y - cy, c[u].z - cz, key_d2(key[u]));
          rp[kCapSmall + i] = nv[u];
        }
      }
    }
    __syncthreads();
    SPROF_T(l2);
    SPROF_ADD(11, l1, l2);
    static_assert(sizeof(double) * kChains * kChunk <= sizeof(uint64_t) * kCapSmall, "chain terms fit the sort scratch");
    shot_lrf(S, reinterpret_cast<double(*)[kChunk]>(keys + kCapSmall), NbRecs{rp, rp + kCapSmall}, k, radius);
    SPROF_T(l3);
    SPROF_ADD(12, l2, l3);
    if (tid < 10) sq[l].cov[tid] = S.cov[tid];
    if (tid == 0) {
      sq[l].k = k;
      sq[l].n_invalid = S.n_invalid;
      sq[l].zero_prefix = S.zero_prefix;
      sq[l].status = 0;
    }
    __syncthreads();
  }
}

// B: one lane per query, SelfAdjointEigenSolver<Matrix3d>
__global__ void __launch_bounds__(64) k_shot_eigen(ShotQuery* __restrict__ sq, int64_t nq) {
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= nq || sq[q].status != 0) return;
  double cov[10], axes[6];
  for (int i = 0; i < 10; ++i) cov[i] = sq[q].cov[i];
  if (shot_eigen(cov, sq[q].k - sq[q].n_invalid, axes)) {
    for (int i = 0; i < 6; ++i) sq[q].axes[i] = axes[i];
  } else {
    sq[q].status = 3;  // no frame: NaN rows (written by C)
  }
}

// cell key of each query on the surface grid (clamped into it; non-finite: past the last cell),
// for the cell-ordered processing of k_shot_lrf
__global__ void __launch_bounds__(256) k_shot_qkeys(GridView g, const float* __restrict__ qx,
                                                    const float* __restrict__ qy, const float* __restrict__ qz,
                                                    int64_t nq, uint32_t* __restrict__ keys,
                                                    int32_t* __restrict__ vals) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const float px = qx[i], py = qy[i], pz = qz[i];
  uint32_t key = (uint32_t)((int64_t)g.nx * g.ny * g.nz);
  if (isfinite(px) && isfinite(py) && isfinite(pz)) {
    int64_t ix = (int64_t)floor(((double)px - g.ox) * g.inv);
    int64_t iy = (int64_t)floor(((double)py - g.oy) * g.inv);
    int64_t iz = (int64_t)floor(((double)pz - g.oz) * g.inv);
    ix = ix < 0 ? 0 : (ix >= g.nx ? g.nx - 1 : ix);
    iy = iy < 0 ? 0 : (iy >= g.ny ? g.ny - 1 : iy);
    iz = iz < 0 ? 0 : (iz >= g.nz ? g.nz - 1 : iz);
    key = (uint32_t)((ix * g.ny + iy) * g.nz + iz);
  }
  keys[i] = key;
  vals[i] = (int32_t)i;
}

}  // namespace

// PFX_SHOT_ORDER=0: the split kernels take the queries in caller order (A/B)
inline bool shot_cell_order() {
  static const bool on = [] {
    const char* e = getenv("PFX_SHOT_ORDER");
    return !(e && e[0] == '0');
  }();
  return on;
}

}  // namespace pfx
