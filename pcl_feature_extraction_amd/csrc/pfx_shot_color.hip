// pfx_shot_color.hip -- SHOTColorEstimationOMP<PointXYZRGB,Normal,SHOT1344> (evaluation.cpp:786-805
// via Features<T>::compute, features.h:175-196) on gfx950.  DESIGN.md "SHOT-1344: the contract".
//
// The search, the sort and the local reference frame are pfx_shot.hip's (pfx_shot_core.h: the
// split path's k_shot_lrf / k_shot_eigen, the fused path's phases), so rf equals pfx_shot's bit
// for bit.  New here:
//   * RGB2CIELAB: the two tables are built on the host with PCL's expressions and uploaded; one
//     Lab record per surface point (cell order, next to the normal records) and per query;
//   * interpolateDoubleChannel: a neighbour's five shape updates and their five mirrors on the
//     colour block (shot_updates<true>), applied per bin in neighbour order by the same bucketing
//     as SHOT-352, one run for the 352 shape bins and one per 352-wide slice of the 992 colour
//     bins (PFX_SHOTC_PASS);
//   * normalizeHistogram over the 1344 entries.
#include <cmath>

#include "pfx_shot_core.h"

namespace pfx {
namespace {

constexpr int kLutRgb = 256, kLutXyz = 4000;

// colour bins binned per run by the split path's histogram kernel.  352: three runs through the
// shape run's 19 KB of LDS, eight workgroups per CU.  Measured on the 1M-point seabed, 10,000
// queries (DESIGN.md "SHOT-1344: measurement"): 352 -> 1.43 ms, 496 (two runs, 44 KB, three
// workgroups) -> 1.58 ms, 992 (one run, 64 KB, two workgroups) -> 1.76 ms; SHOT-352 0.81 ms.
#ifndef PFX_SHOTC_PASS
#define PFX_SHOTC_PASS 352
#endif

// SHOTColorEstimation::RGB2CIELAB, then PCL's L / 100, a / 120, b / 120.  lut: sRGB_LUT[256] +
// sXYZ_LUT[4000].  A table index past the end (y == 1.0f exactly for pure white: PCL reads out of
// bounds) is clamped to the last entry and reported in `clamped`.
__device__ __forceinline__ float4 rgb_lab(uint32_t rgb, const float* __restrict__ lut, bool& clamped) {
  const float fr = lut[(rgb >> 16) & 255u], fg = lut[(rgb >> 8) & 255u], fb = lut[rgb & 255u];
  const float x = (fr * 0.412453f + fg * 0.357580f) + fb * 0.180423f;
  const float y = (fr * 0.212671f + fg * 0.715160f) + fb * 0.072169f;
  const float z = (fr * 0.019334f + fg * 0.119193f) + fb * 0.950227f;
  float vx = x / 0.95047f, vy = y, vz = z / 1.08883f;
  const int ix = (int)(vx * 4000), iy = (int)(vy * 4000), iz = (int)(vz * 4000);
  clamped = ix >= kLutXyz || iy >= kLutXyz || iz >= kLutXyz;
  const float* __restrict__ xyz = lut + kLutRgb;
  vx = xyz[min(ix, kLutXyz - 1)];
  vy = xyz[min(iy, kLutXyz - 1)];
  vz = xyz[min(iz, kLutXyz - 1)];
  float L = 116.0f * vy - 16.0f;
  if (L > 100) L = 100.0f;
  float A = 500.0f * (vx - vy);
  if (A > 120) A = 120.0f;
  else if (A < -120) A = -120.0f;
  float B = 200.0f * (vy - vz);
  if (B > 120) B = 120.0f;
  else if (B < -120) B = -120.0f;
  return make_float4(L / 100.0f, A / 120.0f, B / 120.0f, 0.0f);
}

// the surface in cell order: normal records whose fourth component is the point's cell position
// (k_shot_lrf copies it into the neighbour records), and the Lab records at that position
__global__ void k_shotc_prep(const int32_t* __restrict__ ipos, int64_t n, const float* __restrict__ nx,
                             const float* __restrict__ ny, const float* __restrict__ nz,
                             const uint32_t* __restrict__ rgb, const float* __restrict__ lut,
                             float4* __restrict__ snp, float4* __restrict__ slab, int* __restrict__ n_clamped) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t pos = ipos[i];
  bool cl;
  slab[pos] = rgb_lab(rgb[i], lut, cl);
  snp[pos] = make_float4(nx[i], ny[i], nz[i], __int_as_float(pos));
  if (cl) atomicAdd(n_clamped, 1);
}

// the queries' Lab records (caller order)
__global__ void k_shotc_qlab(const uint32_t* __restrict__ rgb, int64_t nq, const float* __restrict__ lut,
                             float4* __restrict__ qlab, int* __restrict__ n_clamped) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nq) return;
  bool cl;
  qlab[i] = rgb_lab(rgb[i], lut, cl);
  if (cl) atomicAdd(n_clamped, 1);
}

// a neighbour's (<= 5 + 5) updates from the frame (fx, fy, fz) and the two Lab records.  The
// shape channel's skip rules (a non-finite normal, distance == 0) skip both channels.
__device__ __forceinline__ void nb_updates_color(const float4& c, const float3& nv, const float4& lab,
                                                 const float4& ref, const f3& fx, const f3& fy, const f3& fz,
                                                 double radius, int bins[5], float vals[5], int cbins[5],
                                                 float cvals[5]) {
#pragma unroll
  for (int s = 0; s < 5; ++s) { bins[s] = -1; cbins[s] = -1; }
  const double distance = sqrt((double)c.w);
  if (isfinite(nv.x) && isfinite(nv.y) && isfinite(nv.z) && !(fabs(distance - 0.0) < 1E-15)) {
    double cosd = dot4(mk3(nv.x, nv.y, nv.z), fz);
    if (cosd > 1.0) cosd = 1.0;
    if (cosd < -1.0) cosd = -1.0;
    const double binDist = ((1.0 + cosd) * kBins) / 2;
    // float differences, fabs and the sums in double (PCL's unqualified fabs)
    double cd = (fabs((double)(ref.x - lab.x)) + ((fabs((double)(ref.y - lab.y)) + fabs((double)(ref.z - lab.z))) / 2)) / 3;
    if (cd > 1.0) cd = 1.0;
    if (cd < 0.0) cd = 0.0;
    shot_updates<true>(mk3(c.x, c.y, c.z), distance, binDist, fx, fy, fz, radius, bins, vals, cd * kBinsC, cbins,
                       cvals);
  }
}

// ---- the histogram stage -------------------------------------------------------------
// W: the colour bins binned per run.  W == kLen: the colour runs reuse the shape run's LDS.
template <int W>
struct ColorUpd {
  HistUpd<kLen> us;
  HistUpd<W> uc_;
  __device__ __forceinline__ HistUpd<W>& uc() { return uc_; }
};
template <>
struct ColorUpd<kLen> {
  HistUpd<kLen> us;
  __device__ __forceinline__ HistUpd<kLen>& uc() { return us; }
};

template <int W>
struct ShotColorLds {
  union {
    double lrf[kChains][kChunk];
    ColorUpd<W> upd;
    alignas(16) float hist[kLenAll];
  };
  double cov[10];
  double axes[6];
  int lrf_l[4];
  float lrf_m[4];
  float rf[9];
  int n_invalid, zero_prefix, plusT, plusN, ok;
};

// a thread's bins: hs[j] = shape bin t + 256 j; hc[p][j] = colour bin p W + t + 256 j
template <int W>
struct ColorAcc {
  static constexpr int kRuns = (kLenC + W - 1) / W;
  float hs[2];
  float hc[kRuns][HistUpd<W>::kPer];
  __device__ __forceinline__ void clear() {
    hs[0] = hs[1] = 0.0f;
#pragma unroll
    for (int p = 0; p < kRuns; ++p)
#pragma unroll
      for (int j = 0; j < HistUpd<W>::kPer; ++j) hc[p][j] = 0.0f;
  }
};

template <int W>
__device__ __forceinline__ void shotc_clear(ColorUpd<W>& U) {
  hist_clear(U.us);
  if (W != kLen) hist_clear(U.uc());
}

// one chunk of m neighbours into both channels (the two never share a bin, so only the order
// inside a channel matters: each run is hist_chunk's stable per-bin order)
template <int W>
__device__ __forceinline__ void shotc_chunk(ColorUpd<W>& U, int m, const int bins[5], const float vals[5],
                                            const int cbins[5], const float cvals[5], ColorAcc<W>& A) {
  hist_chunk<kLen>(U.us, m, bins, vals, A.hs);
#pragma unroll
  for (int p = 0; p < ColorAcc<W>::kRuns; ++p) {
    int lb[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int b = cbins[s] - p * W;
      lb[s] = (b >= 0 && b < W) ? b : -1;
    }
    hist_chunk<W>(U.uc(), m, lb, cvals, A.hc[p]);
  }
}

// the 1344 entries -> S.hist, normalizeHistogram, the outputs
template <int W>
__device__ __forceinline__ void shotc_finish(ShotColorLds<W>& S, const ColorAcc<W>& A, float* __restrict__ d,
                                             float* __restrict__ rfo) {
  const int tid = threadIdx.x;
  // (hist shares its LDS with the bucketing state: the last run ended with a barrier)
#pragma unroll
  for (int j = 0; j < 2; ++j)
    if (tid + 256 * j < kLen) S.hist[tid + 256 * j] = A.hs[j];
#pragma unroll
  for (int p = 0; p < ColorAcc<W>::kRuns; ++p)
#pragma unroll
    for (int j = 0; j < HistUpd<W>::kPer; ++j) {
      const int b = tid + 256 * j;
      if (b < W && p * W + b < kLenC) S.hist[kLen + p * W + b] = A.hc[p][j];
    }
  __syncthreads();
  constexpr int P = (kLenAll + 255) / 256;
  float h[P];
#pragma unroll
  for (int j = 0; j < P; ++j) h[j] = tid + 256 * j < kLenAll ? S.hist[tid + 256 * j] : 0.0f;
  hist_normalize<kLenAll>(S, h, d, rfo);
}

// ---- fused form (the lists longer than kCapSmall): every phase of a query in one workgroup,
// the keys of kCap neighbours in LDS (128 KB), so the colour bins go through the shape run's
// bucketing state in three runs
struct NbKeysLab {
  const uint64_t* keys;
  const int32_t* __restrict__ ipos;
  const float4* __restrict__ slab;
  __device__ __forceinline__ float4 lab(int j) const { return slab[ipos[key_idx(keys[j])]]; }
};

__global__ void __launch_bounds__(256) k_shotc_long(GridView g, const float* __restrict__ nx,
                                                    const float* __restrict__ ny, const float* __restrict__ nz,
                                                    const float* __restrict__ qx, const float* __restrict__ qy,
                                                    const float* __restrict__ qz, const int32_t* __restrict__ list,
                                                    const int* __restrict__ n_list, const int32_t* __restrict__ ipos,
                                                    const float4* __restrict__ slab, const float4* __restrict__ qlab,
                                                    double radius, float* __restrict__ desc,
                                                    float* __restrict__ rf_out, int* __restrict__ err,
                                                    unsigned long long* __restrict__ nbr) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // kCap
  __shared__ ShotColorLds<kLen> S;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const float rr = (float)(radius * radius);
  const int64_t count = *n_list;
  for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
    const int64_t q = list[w];
    float* d = desc + q * kLenAll;
    float* rfo = rf_out + q * 9;
    const float cx = qx[q], cy = qy[q], cz = qz[q];  // (finite: the split pass wrote the others)
    const int k = sorted_neighbors(g, cx, cy, cz, rr, keys, kCap, &s_count);
    if (k > kCap) {
      if (tid == 0) atomicMax(err, k);
      continue;
    }
    if (tid == 0) atomicAdd(nbr, (unsigned long long)k);
    const NbKeys src{keys, g.ux, g.uy, g.uz, nx, ny, nz, cx, cy, cz};
    const NbKeysLab labs{keys, ipos, slab};
    shot_lrf(S, S.lrf, src, k, radius);
    const int valid = k - S.n_invalid;
    if (tid == 0) {
      double cov[10], axes[6];
      for (int i = 0; i < 10; ++i) cov[i] = S.cov[i];
      S.ok = shot_eigen(cov, valid, axes) ? 1 : 0;
      for (int i = 0; i < 6; ++i) S.axes[i] = axes[i];
    }
    __syncthreads();
    if (!S.ok) {
      shot_nan<kLenAll>(d, rfo);
      continue;
    }
    shot_frame(S, src, k, valid);
    __syncthreads();
    const f3 fx = mk3(S.rf[0], S.rf[1], S.rf[2]), fy = mk3(S.rf[3], S.rf[4], S.rf[5]),
             fz = mk3(S.rf[6], S.rf[7], S.rf[8]);
    const float4 ref = qlab[q];
    ColorAcc<kLen> A;
    A.clear();
    shotc_clear(S.upd);
    for (int c0 = 0; c0 < k; c0 += kChunk) {
      const int m = min(kChunk, k - c0);
      int bins[5], cbins[5];
      float vals[5], cvals[5];
#pragma unroll
      for (int s = 0; s < 5; ++s) { bins[s] = -1; cbins[s] = -1; }
      if (tid < m)
        nb_updates_color(src.pt(c0 + tid), src.nrm(c0 + tid), labs.lab(c0 + tid), ref, fx, fy, fz, radius, bins, vals,
                         cbins, cvals);
      shotc_chunk(S.upd, m, bins, vals, cbins, cvals, A);
    }
    shotc_finish(S, A, d, rfo);
  }
}

// ---- split form: k_shot_lrf<kLenAll> and k_shot_eigen (pfx_shot_core.h), then ----
// C: sign disambiguation and the update records of every neighbour: two planes of 32-B records
// per query (upd_pack: shape, then colour), 2 kCapSmall uint4 each
#ifndef PFX_SHOTC_FRAME_WG
#define PFX_SHOTC_FRAME_WG 2
#endif
__global__ void __launch_bounds__(256, PFX_SHOTC_FRAME_WG) k_shotc_frame(
    int64_t base, int64_t nq, double radius, float* __restrict__ desc, float* __restrict__ rf_out,
    const float4* __restrict__ grec, const ShotQuery* __restrict__ sq, uint4* __restrict__ upd,
    const int32_t* __restrict__ order, const float4* __restrict__ slab, const float4* __restrict__ qlab) {
  __shared__ FrameLds S;
  const int tid = threadIdx.x;
  for (int64_t l = blockIdx.x; l < nq; l += gridDim.x) {
    const int64_t q = order ? order[base + l] : base + l;
    const int status = sq[l].status;
    if (status == 1 || status == 2) continue;
    float* rfo = rf_out + q * 9;
    if (status == 3) {
      shot_nan<kLenAll>(desc + q * kLenAll, rfo);
      continue;
    }
    const int k = sq[l].k;
    const NbRecs src{grec + l * 2 * kCapSmall, grec + l * 2 * kCapSmall + kCapSmall};
    if (tid < 6) S.axes[tid] = sq[l].axes[tid];
    if (tid == 0) {
      S.zero_prefix = sq[l].zero_prefix;
      S.plusT = 0;
      S.plusN = 0;
    }
    __syncthreads();
    shot_frame(S, src, k, k - sq[l].n_invalid);
    __syncthreads();
    if (tid < 9) rfo[tid] = S.rf[tid];
    const f3 fx = mk3(S.rf[0], S.rf[1], S.rf[2]), fy = mk3(S.rf[3], S.rf[4], S.rf[5]),
             fz = mk3(S.rf[6], S.rf[7], S.rf[8]);
    const float4 ref = qlab[q];
    uint4* us = upd + l * 4 * kCapSmall;
    uint4* uc = us + 2 * kCapSmall;
    for (int j = tid; j < k; j += 256) {
      int bins[5], cbins[5];
      float vals[5], cvals[5];
      const float4 nv = src.nrms[j];  // {normal, cell position}
      nb_updates_color(src.pt(j), make_float3(nv.x, nv.y, nv.z), slab[__float_as_int(nv.w)], ref, fx, fy, fz, radius,
                       bins, vals, cbins, cvals);
      uint4 a;
      float4 b;
      upd_pack(bins, vals, a, b);
      us[2 * j] = a;
      reinterpret_cast<float4*>(us)[2 * j + 1] = b;
      upd_pack(cbins, cvals, a, b);
      uc[2 * j] = a;
      reinterpret_cast<float4*>(uc)[2 * j + 1] = b;
    }
    __syncthreads();  // S is rewritten by the next query
  }
}

// D: the histogram from the update records, normalisation, descriptor
#ifndef PFX_SHOTC_ACCUM_WG
#define PFX_SHOTC_ACCUM_WG (PFX_SHOTC_PASS == 352 ? 8 : 2)
#endif
__global__ void __launch_bounds__(256, PFX_SHOTC_ACCUM_WG) k_shotc_accum(int64_t base, int64_t nq,
                                                                         float* __restrict__ desc,
                                                                         const uint4* __restrict__ upd,
                                                                         const ShotQuery* __restrict__ sq,
                                                                         const int32_t* __restrict__ order) {
  constexpr int W = PFX_SHOTC_PASS;
  __shared__ ShotColorLds<W> S;
  const int tid = threadIdx.x;
  for (int64_t l = blockIdx.x; l < nq; l += gridDim.x) {
    if (sq[l].status != 0) continue;
    const int k = sq[l].k;
    const uint4* us = upd + l * 4 * kCapSmall;
    const uint4* uc = us + 2 * kCapSmall;
    ColorAcc<W> A;
    A.clear();
    shotc_clear(S.upd);
    // the next chunk's records are loaded while this one is binned
    uint4 a_n = make_uint4(0, 0, 0, 0), ca_n = a_n;
    float4 b_n = make_float4(0.f, 0.f, 0.f, 0.f), cb_n = b_n;
    if (tid < k) {
      a_n = us[2 * tid];
      b_n = reinterpret_cast<const float4*>(us)[2 * tid + 1];
      ca_n = uc[2 * tid];
      cb_n = reinterpret_cast<const float4*>(uc)[2 * tid + 1];
    }
    for (int c0 = 0; c0 < k; c0 += kChunk) {
      const int m = min(kChunk, k - c0);
      const uint4 a = a_n, ca = ca_n;
      const float4 b = b_n, cb = cb_n;
      if (c0 + kChunk + tid < k) {
        const int j = c0 + kChunk + tid;
        a_n = us[2 * j];
        b_n = reinterpret_cast<const float4*>(us)[2 * j + 1];
        ca_n = uc[2 * j];
        cb_n = reinterpret_cast<const float4*>(uc)[2 * j + 1];
      }
      int bins[5], cbins[5];
      float vals[5], cvals[5];
      upd_unpack(a, b, bins, vals);
      upd_unpack(ca, cb, cbins, cvals);
      if (tid >= m) {
#pragma unroll
        for (int s = 0; s < 5; ++s) { bins[s] = -1; cbins[s] = -1; }
      }
      shotc_chunk(S.upd, m, bins, vals, cbins, cvals, A);
    }
    shotc_finish(S, A, desc + (order ? (int64_t)order[base + l] : base + l) * kLenAll, nullptr);
  }
}

// RGB2CIELAB's tables exactly as PCL fills them (the host's powf): sRGB_LUT, then sXYZ_LUT
const float* lab_tables() {
  static float lut[kLutRgb + kLutXyz];
  static const bool once = [] {
    for (int i = 0; i < kLutRgb; ++i) {
      const float f = static_cast<float>(i) / 255.0f;
      if (f > 0.04045) lut[i] = powf((f + 0.055f) / 1.055f, 2.4f);
      else lut[i] = f / 12.92f;
    }
    for (int i = 0; i < kLutXyz; ++i) {
      const float f = static_cast<float>(i) / 4000.0f;
      if (f > 0.008856) lut[kLutRgb + i] = static_cast<float>(powf(f, 0.3333f));
      else lut[kLutRgb + i] = static_cast<float>((7.787 * f) + (16.0 / 116.0));
    }
    return true;
  }();
  (void)once;
  return lut;
}

}  // namespace

int64_t shot_color_cap_small() { return kCapSmall; }

void shot_color_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx,
                    const float* sny, const float* snz, const uint32_t* srgb, int64_t ns, const float* qx,
                    const float* qy, const float* qz, const uint32_t* qrgb, int64_t nq, double r, float* desc,
                    float* rf) {
  PFX_CHECK(r > 0.0, "shot_color: radius must be > 0");
  ctx->stats["shot_color_neighbors"] = 0;
  ctx->stats["shot_color_lut_clamped"] = 0;
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  // err[0]: longest list beyond kCap, [1]: lists beyond kCapSmall, [2..3]: neighbour sum, [4]:
  // colours whose table index was clamped
  int* err = ctx->buf("shotc_err").as<int>(6);
  unsigned long long* nbr = reinterpret_cast<unsigned long long*>(err + 2);
  int* n_clamped = err + 4;
  PFX_HIP(hipMemsetAsync(err, 0, 6 * sizeof(int), st));
  float* lut = ctx->buf("shotc_lut").as<float>(kLutRgb + kLutXyz);
  PFX_HIP(hipMemcpyAsync(lut, lab_tables(), sizeof(float) * (kLutRgb + kLutXyz), hipMemcpyHostToDevice, st));
  float4* qlab = ctx->buf("shotc_qlab").as<float4>((size_t)nq);
  k_shotc_qlab<<<(unsigned)ceil_div(nq, 256), 256, 0, st>>>(qrgb, nq, lut, qlab, n_clamped);
  if (ns == 0) {
    std::vector<float> nanv((size_t)nq * kLenAll, __builtin_nanf(""));
    int h_cl = 0;
    PFX_HIP(hipMemcpyAsync(desc, nanv.data(), sizeof(float) * nq * kLenAll, hipMemcpyHostToDevice, st));
    PFX_HIP(hipMemcpyAsync(rf, nanv.data(), sizeof(float) * nq * 9, hipMemcpyHostToDevice, st));
    PFX_HIP(hipMemcpyAsync(&h_cl, n_clamped, sizeof(int), hipMemcpyDeviceToHost, st));
    PFX_HIP(hipStreamSynchronize(st));
    ctx->stats["shot_color_lut_clamped"] = h_cl;
    return;
  }
  GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
  {
    TimeScope ts(ctx, "shot_color", true);
    int32_t* over = ctx->buf("shot_over").as<int32_t>(nq);
    int* n_over = err + 1;
    const size_t lds_s = 2 * sizeof(uint64_t) * kCapSmall, lds = sizeof(uint64_t) * kCap;
    PFX_HIP(hipFuncSetAttribute((const void*)k_shotc_long, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // SHOT-352's scratch under its own names, sized from the batch: the update records are twice
    // SHOT-352's per query, so the batch is half as long
    constexpr int64_t kSplitBatch = 8192;
    const int64_t bq = std::min<int64_t>(nq, kSplitBatch);
    float4* grec = ctx->buf("shot_recs").as<float4>((size_t)bq * 2 * kCapSmall);
    ShotQuery* sq = ctx->buf("shot_q").as<ShotQuery>((size_t)bq);
    uint4* upd = ctx->buf("shot_upd").as<uint4>((size_t)bq * 4 * kCapSmall);
    int32_t* ipos = ctx->buf("shot_ipos").as<int32_t>(ns);
    float4* snp = ctx->buf("shot_snp").as<float4>(ns);
    float4* slab = ctx->buf("shotc_slab").as<float4>(ns);
    k_shot_ipos<<<(unsigned)ceil_div(ns, 256), 256, 0, st>>>(ctx->grid_b.perm, ns, ipos);
    k_shotc_prep<<<(unsigned)ceil_div(ns, 256), 256, 0, st>>>(ipos, ns, snx, sny, snz, srgb, lut, snp, slab,
                                                              n_clamped);
    // the queries in cell order (results are per query: the order changes no value)
    int32_t* order = nullptr;
    if (shot_cell_order()) {
      const Grid& G = ctx->grid_b;
      int bits = 1;
      while ((int64_t(1) << bits) <= G.ncells) ++bits;
      uint32_t* qk = ctx->buf("shot_qkeys").as<uint32_t>((size_t)nq);
      uint32_t* qk2 = ctx->buf("shot_qkeys2").as<uint32_t>((size_t)nq);
      int32_t* qv = ctx->buf("shot_qvals").as<int32_t>((size_t)nq);
      order = ctx->buf("shot_order").as<int32_t>((size_t)nq);
      size_t tb = 0;
      PFX_HIP(rocprim::radix_sort_pairs(nullptr, tb, qk, qk2, qv, order, (size_t)nq, 0, bits, st));
      void* tmp = ctx->buf("shot_sort_tmp").get(tb + 16);
      k_shot_qkeys<<<(unsigned)ceil_div(nq, 256), 256, 0, st>>>(g, qx, qy, qz, nq, qk, qv);
      PFX_HIP(rocprim::radix_sort_pairs(tmp, tb, qk, qk2, qv, order, (size_t)nq, 0, bits, st));
    }
    for (int64_t q0 = 0; q0 < nq; q0 += kSplitBatch) {
      const int64_t m = std::min<int64_t>(kSplitBatch, nq - q0);
      // (a multiple of 8: k_shot_lrf's per-XCD ranges)
      const unsigned bl = (unsigned)(ceil_div(std::min<int64_t>(m, 256 * 10 * PFX_SHOT_GRID_MUL), 8) * 8);
      k_shot_lrf<kLenAll><<<bl, 256, lds_s, st>>>(g, qx, qy, qz, q0, m, over, n_over, r, desc, rf, grec, sq, ipos, snp,
                                                  nbr, order);
      k_shot_eigen<<<(unsigned)ceil_div(m, 64), 64, 0, st>>>(sq, m);
      k_shotc_frame<<<(unsigned)std::min<int64_t>(m, 256 * 16 * PFX_SHOT_GRID_MUL), 256, 0, st>>>(
          q0, m, r, desc, rf, grec, sq, upd, order, slab, qlab);
      k_shotc_accum<<<(unsigned)std::min<int64_t>(m, 256 * 16 * PFX_SHOT_GRID_MUL), 256, 0, st>>>(q0, m, desc, upd,
                                                                                                 sq, order);
    }
    // longer lists: grid sized for the worst case, the count stays on the device
    k_shotc_long<<<(unsigned)std::min<int64_t>(nq, 256 * 2), 256, lds, st>>>(g, snx, sny, snz, qx, qy, qz, over, n_over,
                                                                             ipos, slab, qlab, r, desc, rf, err, nbr);
    check_launch("k_shotc_long");
  }
  int h[6] = {};
  PFX_HIP(hipMemcpyAsync(h, err, sizeof(h), hipMemcpyDeviceToHost, st));
  PFX_HIP(hipStreamSynchronize(st));
  unsigned long long h_nbr = 0;
  memcpy(&h_nbr, h + 2, sizeof(h_nbr));
  ctx->stats["shot_color_neighbors"] = (int64_t)h_nbr;
  ctx->stats["shot_color_lut_clamped"] = h[4];
  if (h[0] > 0)
    throw Error(PFX_ERR_CAPACITY, "shot_color: a query has " + std::to_string(h[0]) + " neighbours (> " +
                                      std::to_string(kCap) + " supported)");
}

}  // namespace pfx
