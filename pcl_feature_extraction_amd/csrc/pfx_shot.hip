// pfx_shot.hip -- SHOTEstimationOMP<PointXYZRGB,Normal,SHOT352> (evaluation.cpp:766-785 via
// Features<T>::compute, features.h:175-196) on gfx950.  SURVEY A.7.
//
// One 256-thread workgroup per query:
//   1. radius neighbours in FLANN order (bitonic sort of (d2, caller index) keys in LDS);
//   2. SHOTLocalReferenceFrameEstimation::getLocalRF: the weighted double covariance is a set of
//      strictly ordered double chains (one lane per matrix entry + one for the weight sum) over
//      LDS-staged neighbour chunks; Eigen 3.2.0's SelfAdjointEigenSolver<Matrix3d> with
//      eigenvectors (pfx_eigen3.h, the oracle's operation sequence); sign disambiguation counts
//      reduced over the block;
//   3. SHOT: every neighbour's (up to) five interpolated bin updates are computed in parallel and
//      applied per bin in PCL's sequential order (each wave owns a quarter of the bins; lanes
//      that collide on a bin are serialised lowest-first); normalizeHistogram by one lane (double accumulation, as PCL).
// Descriptors and reference frames are bit-exact against the restatement.
#include "pfx_shot_core.h"

namespace pfx {
namespace {

// Fused form (the lists longer than the split path's capacity): every phase of a query in one
// workgroup.  CAP: LDS key capacity.  `list` (nullable): query subset with its device-side
// count; queries with more than CAP neighbours go to `over` (or raise err when over == nullptr).
template <int CAP>
__global__ void __launch_bounds__(256) k_shot(GridView g, const float* __restrict__ nx,
                                              const float* __restrict__ ny, const float* __restrict__ nz,
                                              const float* __restrict__ qx, const float* __restrict__ qy,
                                              const float* __restrict__ qz, int64_t nq,
                                              const int32_t* __restrict__ list, const int* __restrict__ n_list,
                                              int32_t* __restrict__ over, int* __restrict__ n_over,
                                              double radius, float* __restrict__ desc, float* __restrict__ rf_out,
                                              int* __restrict__ err, unsigned long long* __restrict__ nbr) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP (+ CAP sort scratch, first pass)
  __shared__ ShotLds S;
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const float rr = (float)(radius * radius);
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
    const int64_t q = list ? (int64_t)list[w] : w;
    float* d = desc + q * kLen;
    float* rfo = rf_out + q * 9;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    if (!(isfinite(cx) && isfinite(cy) && isfinite(cz))) {
      shot_nan(d, rfo);
      continue;
    }
    const int k = CAP == kCapSmall
                      ? sorted_neighbors_bucketed(g, cx, cy, cz, rr, keys, keys + CAP, CAP, &s_count, SB)
                      : sorted_neighbors(g, cx, cy, cz, rr, keys, CAP, &s_count);
    if (k > CAP) {
      if (tid == 0) {
        if (over) over[atomicAdd(n_over, 1)] = (int32_t)q;
        else atomicMax(err, k);
      }
      continue;
    }
    if (tid == 0) atomicAdd(nbr, (unsigned long long)k);
    const NbKeys src{keys, g.ux, g.uy, g.uz, nx, ny, nz, cx, cy, cz};
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
      shot_nan(d, rfo);
      continue;
    }
    shot_frame(S, src, k, valid);
    shot_hist(S, src, k, radius, d, rfo);
  }
}

// the normals in cell order (second pass of the surface views, after k_shot_ipos)
__global__ void k_shot_prep(const int32_t* __restrict__ ipos, int64_t n, const float* __restrict__ nx,
                            const float* __restrict__ ny, const float* __restrict__ nz, float4* __restrict__ snp) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) snp[ipos[i]] = make_float4(nx[i], ny[i], nz[i], 0.0f);
}

// C: sign disambiguation and the histogram updates of every neighbour, written as records (the
// double-precision interpolation of shot_updates, ~170 VGPRs: three workgroups per CU, with no
// barrier between a workgroup's neighbours)
#ifndef PFX_SHOT_HIST_WG
#define PFX_SHOT_HIST_WG 3
#endif
__global__ void __launch_bounds__(256, PFX_SHOT_HIST_WG) k_shot_frame(int64_t base, int64_t nq, double radius,
                                                                       float* __restrict__ desc,
                                                                       float* __restrict__ rf_out,
                                                                       const float4* __restrict__ grec,
                                                                       const ShotQuery* __restrict__ sq,
                                                                       uint4* __restrict__ upd,
                                                                       const int32_t* __restrict__ order) {
  __shared__ FrameLds S;
  const int tid = threadIdx.x;
  for (int64_t l = blockIdx.x; l < nq; l += gridDim.x) {
    const int64_t q = order ? order[base + l] : base + l;
    const int status = sq[l].status;
    if (status == 1 || status == 2) continue;
    float* rfo = rf_out + q * 9;
    if (status == 3) {
      shot_nan(desc + q * kLen, rfo);
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
    SPROF_T(f0t);
    shot_frame(S, src, k, k - sq[l].n_invalid);
    __syncthreads();
    SPROF_T(f1t);
    SPROF_ADD(6, f0t, f1t);
    if (tid < 9) rfo[tid] = S.rf[tid];
    const f3 fx = mk3(S.rf[0], S.rf[1], S.rf[2]), fy = mk3(S.rf[3], S.rf[4], S.rf[5]),
             fz = mk3(S.rf[6], S.rf[7], S.rf[8]);
    uint4* u = upd + l * 2 * kCapSmall;
    for (int j = tid; j < k; j += 256) {
      int bins[5];
      float vals[5];
      nb_updates(src.pt(j), src.nrm(j), fx, fy, fz, radius, bins, vals);
      uint4 a;
      float4 b;
      upd_pack(bins, vals, a, b);
      u[2 * j] = a;
      reinterpret_cast<float4*>(u)[2 * j + 1] = b;
    }
    __syncthreads();  // S is rewritten by the next query
    SPROF_T(f2t);
    SPROF_ADD(9, f1t, f2t);
    SPROF_ADD(14, 0, 1);
  }
}

// D: the histogram from the update records, normalisation, descriptor (no double-precision
// interpolation here: a light kernel, many workgroups per CU)
#ifndef PFX_SHOT_ACCUM_WG
#define PFX_SHOT_ACCUM_WG 8
#endif
__global__ void __launch_bounds__(256, PFX_SHOT_ACCUM_WG) k_shot_accum(int64_t base, int64_t nq, float* __restrict__ desc,
                                                    const uint4* __restrict__ upd,
                                                    const ShotQuery* __restrict__ sq,
                                                    const int32_t* __restrict__ order) {
  __shared__ ShotLds S;
  const int tid = threadIdx.x;
  for (int64_t l = blockIdx.x; l < nq; l += gridDim.x) {
    if (sq[l].status != 0) continue;
    const int k = sq[l].k;
    SPROF_T(a0t);
    const uint4* u = upd + l * 2 * kCapSmall;
    float h[2] = {0.0f, 0.0f};
    hist_clear(S.upd);
    // the next chunk's records are loaded while this one is binned
    uint4 a_n = make_uint4(0, 0, 0, 0);
    float4 b_n = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < k) {
      a_n = u[2 * tid];
      b_n = reinterpret_cast<const float4*>(u)[2 * tid + 1];
    }
    for (int c0 = 0; c0 < k; c0 += kChunk) {
      const int m = min(kChunk, k - c0);
      const uint4 a = a_n;
      const float4 b = b_n;
      if (c0 + kChunk + tid < k) {
        a_n = u[2 * (c0 + kChunk + tid)];
        b_n = reinterpret_cast<const float4*>(u)[2 * (c0 + kChunk + tid) + 1];
      }
      int bins[5];
      float vals[5];
      upd_unpack(a, b, bins, vals);
      if (tid >= m) {
#pragma unroll
        for (int s = 0; s < 5; ++s) bins[s] = -1;
      }
      hist_chunk(S.upd, m, bins, vals, h);
    }
    hist_finish<kLen>(S, h, desc + (order ? (int64_t)order[base + l] : base + l) * kLen, nullptr);
    SPROF_T(a1t);
    SPROF_ADD(4, a0t, a1t);
    SPROF_ADD(5, 0, 1);
  }
}

}  // namespace

void shot_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
              const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, int64_t nq, double r,
              float* desc, float* rf) {
  PFX_CHECK(r > 0.0, "shot: radius must be > 0");
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  if (ns == 0) {
    std::vector<float> nanv((size_t)nq * kLen, __builtin_nanf(""));
    PFX_HIP(hipMemcpyAsync(desc, nanv.data(), sizeof(float) * nq * kLen, hipMemcpyHostToDevice, st));
    PFX_HIP(hipMemcpyAsync(rf, nanv.data(), sizeof(float) * nq * 9, hipMemcpyHostToDevice, st));
    PFX_HIP(hipStreamSynchronize(st));
    return;
  }
  // the surface grid prepared ahead (pfx_fpfh_prepare_dev: coordinates only, e.g. while the normals
  // are estimated on another stream), else built here
  GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
  int* err = ctx->buf("shot_err").as<int>(4);
  unsigned long long* nbr = reinterpret_cast<unsigned long long*>(err + 2);
  PFX_HIP(hipMemsetAsync(err, 0, 4 * sizeof(int), st));
  {
    TimeScope ts(ctx, "shot", true);
    int32_t* over = ctx->buf("shot_over").as<int32_t>(nq);
    int* n_over = err + 1;
    const size_t lds_s = 2 * sizeof(uint64_t) * kCapSmall, lds = sizeof(uint64_t) * kCap;
    PFX_HIP(hipFuncSetAttribute((const void*)k_shot<kCap>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // lists <= kCapSmall: the split kernels in batches of kSplitBatch queries (sort + LRF
    // covariance per workgroup, the eigen solve one lane per query, frame + histogram per
    // workgroup; round 3: 1.93 -> 1.25 ms against every phase in one workgroup per query)
    {
      constexpr int64_t kSplitBatch = 16384;
      const int64_t bq = std::min<int64_t>(nq, kSplitBatch);
      float4* grec = ctx->buf("shot_recs").as<float4>((size_t)bq * 2 * kCapSmall);
      ShotQuery* sq = ctx->buf("shot_q").as<ShotQuery>((size_t)bq);
      uint4* upd = ctx->buf("shot_upd").as<uint4>((size_t)bq * 2 * kCapSmall);
      int32_t* ipos = ctx->buf("shot_ipos").as<int32_t>(ns);
      float4* snp = ctx->buf("shot_snp").as<float4>(ns);
      k_shot_ipos<<<(unsigned)ceil_div(ns, 256), 256, 0, st>>>(ctx->grid_b.perm, ns, ipos);
      k_shot_prep<<<(unsigned)ceil_div(ns, 256), 256, 0, st>>>(ipos, ns, snx, sny, snz, snp);
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
        k_shot_lrf<kLen><<<bl, 256, lds_s, st>>>(g, qx, qy, qz, q0, m, over, n_over, r, desc, rf, grec, sq, ipos, snp, nbr,
                                           order);
        k_shot_eigen<<<(unsigned)ceil_div(m, 64), 64, 0, st>>>(sq, m);
        k_shot_frame<<<(unsigned)std::min<int64_t>(m, 256 * 16 * PFX_SHOT_GRID_MUL), 256, 0, st>>>(q0, m, r, desc, rf,
                                                                                                  grec, sq, upd, order);
        k_shot_accum<<<(unsigned)std::min<int64_t>(m, 256 * 16 * PFX_SHOT_GRID_MUL), 256, 0, st>>>(q0, m, desc, upd, sq,
                                                                                                  order);
      }
    }
    // longer lists: grid sized for the worst case, the count stays on the device
    k_shot<kCap><<<(unsigned)std::min<int64_t>(nq, 256 * 2), 256, lds, st>>>(
        g, snx, sny, snz, qx, qy, qz, nq, over, n_over, nullptr, nullptr, r, desc, rf, err, nbr);
    check_launch("k_shot");
  }
  int h2[2] = {0, 0};  // err (a list beyond kCap), n_over (the lists the split kernels passed on)
  unsigned long long h_nbr = 0;
  PFX_HIP(hipMemcpyAsync(h2, err, sizeof(h2), hipMemcpyDeviceToHost, st));
  PFX_HIP(hipMemcpyAsync(&h_nbr, nbr, sizeof(h_nbr), hipMemcpyDeviceToHost, st));
  PFX_HIP(hipStreamSynchronize(st));
  const int h = h2[0];
  ctx->stats["shot_neighbors"] = (int64_t)h_nbr;
  // the queries the split kernels passed on to the fused kernel (lists above kCapSmall)
  ctx->stats["shot_queued"] = (int64_t)h2[1];
#ifdef PFX_SHOT_PROFILE
  {
    unsigned long long pr[16];
    PFX_HIP(hipMemcpyFromSymbol(pr, HIP_SYMBOL(g_shot_prof), sizeof(pr)));
    const double nq_ = (double)(pr[13] + !pr[13]);
    fprintf(stderr, "shot_accum normalisation %.0f cycles/query (%llu sequential)\n", pr[8] / nq_, pr[7]);
    const double na = (double)(pr[5] + !pr[5]), nf = (double)(pr[14] + !pr[14]);
    fprintf(stderr, "shot_accum cycles/query %.0f: masks %.0f counts %.0f scatter %.0f sums %.0f (%llu queries)\n",
            pr[4] / na, pr[0] / na, pr[1] / na, pr[2] / na, pr[3] / na, pr[5]);
    fprintf(stderr, "shot_frame cycles/query: frame %.0f updates %.0f\n", pr[6] / nf, pr[9] / nf);
    fprintf(stderr, "shot_lrf cycles/query: search+sort %.0f records %.0f chains %.0f\n", pr[10] / (double)(pr[13] + !pr[13]),
            pr[11] / (double)(pr[13] + !pr[13]), pr[12] / (double)(pr[13] + !pr[13]));
    const unsigned long long z[16] = {};
    PFX_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_shot_prof), z, sizeof(z)));
  }
#endif
  if (h > 0)
    throw Error(PFX_ERR_CAPACITY, "shot: a query has " + std::to_string(h) + " neighbours (> " +
                                      std::to_string(kCap) + " supported)");
}

}  // namespace pfx
