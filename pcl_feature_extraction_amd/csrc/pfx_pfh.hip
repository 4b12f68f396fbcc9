// pfx_pfh.hip -- PFHEstimation<PointXYZRGB,Normal,PFHSignature125> (evaluation.cpp:676-695) on
// gfx950.  DESIGN.md "PFH-125".
//
//   N(q)     = radius-r neighbours of query q in the surface (FLANN: d2 < (float)(r*r)), k = |N|
//   PFH(q)   = 5 x 5 x 5 bins of the pair features of every pair of N(q), k (k - 1) / 2 of them;
//              the later point of a pair in FLANN order (d2, index) is computePairFeatures' p1;
//              a pair whose features are invalid (f4 == 0 or v_norm == 0) adds nothing.  Each hit
//              adds the same float hist_incr = 100 / (k (k - 1) / 2), so a bin's value depends
//              only on its hit count: bins are counted in LDS (order-free) and materialised by
//              repeated_add.  No normalisation follows.
// A few workgroups per query: each stages the neighbours' records {x, y, z, d2 | nx, ny, nz, index}
// in LDS (k <= kPfhCapLds) and its threads walk their share of the triangular pair space (fast
// path of the pair features, exact path where that cannot decide).  Longer neighbourhoods are
// queued for a second pass whose records live in a per-workgroup slice of a ctx-owned global
// scratch buffer (k <= kPfhMaxK, where the pair count still fits 32 bits); beyond that the row is
// NaN and PFX_ERR_CAPACITY is reported after the next synchronisation (pfh_report).
#include <cstring>

#include "pfx_neighbors.h"
#include "pfx_pair_features.h"

namespace pfx {
namespace {

constexpr int kSplit = 5;            // nr_split: bins per feature
constexpr int kDesc = 125;           // PFHSignature125
#ifndef PFX_PFH_THREADS  // workgroup size (measured: DESIGN.md "PFH-125")
#define PFX_PFH_THREADS 512
#endif
#ifndef PFX_PFH_FAST  // 0: every pair through the exact path (measurement only)
#define PFX_PFH_FAST 1
#endif
constexpr int kPT = PFX_PFH_THREADS;  // 512: 8 waves, two workgroups per CU
constexpr int kPfhCapLds = 2048;     // neighbours staged in LDS: 64 KiB of records, 2 workgroups per CU
constexpr int kPfhMaxK = 65535;      // k (k - 1) / 2 < 2^31
constexpr int kOvfBlocks = 32;       // workgroups of the global-scratch pass
#ifndef PFX_PFH_MIN_SPLIT  // workgroups per query, at least (measured: DESIGN.md "PFH-125")
#define PFX_PFH_MIN_SPLIT 4
#endif
constexpr int kMinSplit = PFX_PFH_MIN_SPLIT, kMaxSplit = 16;
constexpr int kSplitBlocks = 8192;   // ... and as many as bring a call to about this many workgroups
constexpr int kCopies = 2 * (kPT / 64);  // counter copies: two per wave (lane parity)
constexpr int kCntStride = 128;      // ints per counter copy (125 used)
constexpr int kHeadInts = kCopies * kCntStride + 2 * (kPT / 64);  // counters + the gather's wave counts
static_assert(kHeadInts % 4 == 0, "the records that follow are float4");

// the exact path out of line (rare once the fast path is on): h1 + 5 h2 + 25 h3, or -1 for a pair
// computePairFeatures rejects
__device__ __attribute__((noinline)) int pfh_bin_exact(float p1x, float p1y, float p1z, float n1x, float n1y,
                                                       float n1z, float p2x, float p2y, float p2z, float n2x,
                                                       float n2y, float n2z) {
  int h1, h2, h3;
  if (!pair_bins<kSplit>(mk3(p1x, p1y, p1z), mk3(n1x, n1y, n1z), mk3(p2x, p2y, p2z), mk3(n2x, n2y, n2z), h1, h2, h3))
    return -1;
  return h1 + kSplit * h2 + kSplit * kSplit * h3;
}

// Neighbour records of q into ra / rb [0..min(k, cap)) in candidate order -- the same order in
// every workgroup that gathers q, so the workgroups sharing a query number its pairs alike (a
// cursor advanced by atomics would give each its own order).  Per round of kPT candidates: the
// waves' hit counts through LDS (wcnt: two buffers of kPT / 64 ints, alternating, so one barrier a
// round), every thread sums them for its wave's base.  Returns k (may exceed cap).  Every thread
// of the block calls it.
__device__ __forceinline__ int pfh_gather(const GridView& g, const float* __restrict__ snx,
                                          const float* __restrict__ sny, const float* __restrict__ snz, float qx,
                                          float qy, float qz, float rr, float4* ra, float4* rb, int cap, int* wcnt) {
  Runs R;
  query_runs(g, qx, qy, qz, R);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t T = R.pref[9];
  int k = 0, par = 0;
  for (int32_t t0 = 0; t0 < T; t0 += kPT, par ^= 1) {
    const int32_t t = t0 + tid;
    bool hit = false;
    int32_t pos = 0;
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    float d2 = 0.f;
    if (t < T) {
      pos = run_pos(R, t);
      c = g.sp[pos];
      d2 = flann_d2(qx, qy, qz, c.x, c.y, c.z);
      hit = d2 < rr;
    }
    const uint64_t m = __ballot(hit);
    int* wc = wcnt + par * (kPT / 64);
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    int base = k;
#pragma unroll
    for (int w = 0; w < kPT / 64; ++w) {
      const int n = wc[w];
      base += w < wv ? n : 0;
      k += n;
    }
    const int slot = base + __popcll(m & lanemask_lt());
    if (hit && slot < cap) {
      const int32_t idx = g.perm[pos];
      ra[slot] = make_float4(c.x, c.y, c.z, d2);
      rb[slot] = make_float4(snx[idx], sny[idx], snz[idx], __int_as_float(idx));
    }
  }
  __syncthreads();  // the records are written, and wcnt is free for the next call
  return k;
}

// GLOBAL = false: records in LDS (kPfhCapLds); a longer neighbourhood is pushed to `ovf`.
// GLOBAL = true: the queued queries (count read on the device), records in this workgroup's
// slice of `scratch` (2 * gcap float4).
// A query's pair space is shared by `split` workgroups (each gathers the neighbourhood itself and
// takes every split-th stride of pairs), so the longest neighbourhood of a call does not run on one
// CU while the others idle; the integer bin counts meet in hcount (kCntStride per query), k in
// kcount, and k_pfh_finalize turns them into PCL's floats.  The global-scratch pass runs unsplit.
// err: [0] largest k beyond kPfhMaxK (sticky), [1] queued queries, [2..3] pairs (u64), [4] max k
template <bool GLOBAL>
__global__ void __launch_bounds__(kPT) k_pfh(GridView g, const float* __restrict__ snx,
                                             const float* __restrict__ sny, const float* __restrict__ snz,
                                             const float* __restrict__ qx, const float* __restrict__ qy,
                                             const float* __restrict__ qz, int64_t nq, float rr,
                                             int split, int* __restrict__ hcount, int* __restrict__ kcount,
                                             int* __restrict__ err, int32_t* __restrict__ ovf,
                                             float4* __restrict__ scratch, int gcap) {
  // every LDS byte in the dynamic region (16-byte aligned base): counters, wave counts, then records
  extern __shared__ __attribute__((aligned(16))) int pfh_lds[];
  int* cnt = pfh_lds;
  int* wcnt = pfh_lds + kCopies * kCntStride;
  float4* ra = GLOBAL ? scratch + (size_t)blockIdx.x * 2 * gcap : reinterpret_cast<float4*>(pfh_lds + kHeadInts);
  const int cap = GLOBAL ? gcap : kPfhCapLds;
  float4* rb = ra + cap;
  const int tid = threadIdx.x;
  const int64_t count = GLOBAL ? (int64_t)err[1] : nq * split;
  unsigned long long* pairs = reinterpret_cast<unsigned long long*>(err + 2);
  for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
    const int64_t q = GLOBAL ? (int64_t)ovf[w] : w / split;
    const int sub = GLOBAL ? 0 : (int)(w - q * split);
    const int k = pfh_gather(g, snx, sny, snz, qx[q], qy[q], qz[q], rr, ra, rb, cap, wcnt);
    if (!GLOBAL && sub == 0 && tid == 0) {  // once per query
      kcount[q] = k;
      atomicMax(err + 4, k);
      // beyond every capacity: k_pfh_finalize writes a NaN row, and the sticky word reports
      // PFX_ERR_CAPACITY after the next synchronisation
      if (k > kPfhMaxK) atomicMax(err, k);
      else if (k > cap) ovf[atomicAdd(err + 1, 1)] = (int32_t)q;  // the global-scratch pass computes it
      else if (k > 1) atomicAdd(pairs, (unsigned long long)k * (unsigned long long)(k - 1) / 2);
    }
    if (k > cap || k == 0) {
      if (GLOBAL && k > cap && tid == 0) atomicMax(err, k);  // (not reached: gcap holds every queued query)
      continue;
    }
    if (GLOBAL && tid == 0) atomicAdd(pairs, (unsigned long long)k * (unsigned long long)(k - 1) / 2);
    for (int i = tid; i < kCopies * kCntStride; i += kPT) cnt[i] = 0;
    __syncthreads();
    // pairs (i, j), j < i < k, in row-major order of the triangle: pair number p = i (i - 1) / 2 + j;
    // thread t of part `sub` takes p = sub kPT + t, then every (split kPT)-th, and carries (i, j) along
    int* hc = cnt + ((tid >> 6) * 2 + (tid & 1)) * kCntStride;
    const int step = (GLOBAL ? 1 : split) * kPT;
    int i = 1, j = sub * kPT + tid;
    while (i < k && j >= i) { j -= i; ++i; }
    while (i < k) {
      const float4 ai = ra[i], bi = rb[i], aj = ra[j], bj = rb[j];
      // computePairFeatures (p1 = the later of the two in FLANN order, (d2, index) ascending)
      const bool i_later = nb_key(ai.w, __float_as_int(bi.w)) > nb_key(aj.w, __float_as_int(bj.w));
      const float4 a1 = i_later ? ai : aj, b1 = i_later ? bi : bj, a2 = i_later ? aj : ai, b2 = i_later ? bj : bi;
      const f3 p1 = mk3(a1.x, a1.y, a1.z), n1 = mk3(b1.x, b1.y, b1.z), p2 = mk3(a2.x, a2.y, a2.z),
               n2 = mk3(b2.x, b2.y, b2.z);
      // The fast path's bounds hold for unit normals (|n|^2 <= 1 + 1e-6: an |angle| then exceeds 1
      // by rounding only, which its f3 edge check sends to the exact path); other normals, NaN
      // included, take the exact path.  f4 == 0 (coincident points): the pair is skipped.
      int h = -1;
      if (sqn4(sub3(p2, p1)) != 0.0f) {
        int h1, h2, h3;
        if (PFX_PFH_FAST && sqn3(n1) <= 1.000001f && sqn3(n2) <= 1.000001f &&
            pair_bins_fast<kSplit>(p1, n1, p2, n2, h1, h2, h3))
          h = h1 + kSplit * h2 + kSplit * kSplit * h3;
        else
          h = pfh_bin_exact(p1.x, p1.y, p1.z, n1.x, n1.y, n1.z, p2.x, p2.y, p2.z, n2.x, n2.y, n2.z);
      }
      if (h >= 0) atomicAdd(&hc[h], 1);
      j += step;
      while (i < k && j >= i) { j -= i; ++i; }
    }
    __syncthreads();
    if (tid < kDesc) {
      int c = 0;
#pragma unroll
      for (int s = 0; s < kCopies; ++s) c += cnt[s * kCntStride + tid];
      if (c) atomicAdd(&hcount[q * kCntStride + tid], c);
    }
    __syncthreads();  // the counters are read before the next query clears them
  }
}

// PCL's float histogram: histogram[h] += 100 / (k (k - 1) / 2) once per valid pair (repeated_add);
// NaN rows for k == 0 (a non-finite query, no neighbour) and for k beyond kPfhMaxK
__global__ void __launch_bounds__(256) k_pfh_finalize(int64_t nq, const int* __restrict__ hcount,
                                                      const int* __restrict__ kcount, float* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nq * kDesc; e += (int64_t)gridDim.x * 256) {
    const int64_t q = e / kDesc;
    const int b = (int)(e - q * kDesc);
    const int k = kcount[q];
    if (k == 0 || k > kPfhMaxK) {
      out[e] = __builtin_nanf("");
      continue;
    }
    // `100.0f / static_cast<float> (k * (k - 1) / 2)` (size_t); k == 1: inf, and no pair to add
    const unsigned long long npairs = (unsigned long long)k * (unsigned long long)(k - 1) / 2;
    out[e] = repeated_add(100.0f / (float)npairs, hcount[q * kCntStride + b]);
  }
}

}  // namespace

int pfh_cap_lds() { return kPfhCapLds; }

void pfh_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
             const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, int64_t nq, double r,
             float* out) {
  PFX_CHECK(r > 0.0, "pfh: radius must be > 0");
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, kRepPfh);  // [0] sticky, [1..5] per call (pfh_report)
  if (ns == 0) {
    // no surface: every query has an empty neighbourhood -> NaN rows (PCL fills NaN)
    k_fill<<<(unsigned)ceil_div(nq * kDesc, 256), 256, 0, st>>>(out, nq * kDesc, __builtin_nanf(""));
    check_launch("k_fill");
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    const float rr = (float)(r * r);
    // a neighbourhood can only outgrow the LDS records when the surface has more points than that
    const bool overflow_pass = ns > kPfhCapLds;
    const int gcap = overflow_pass ? (int)std::min<int64_t>(ns, kPfhMaxK) : 0;
    int32_t* ovf = ctx->buf("pfh_ovf").as<int32_t>(nq);
    float4* scratch = overflow_pass ? ctx->buf("pfh_scratch").as<float4>((size_t)kOvfBlocks * 2 * gcap) : nullptr;
    int* hcount = ctx->buf("pfh_hcount").as<int>((size_t)nq * kCntStride);
    int* kcount = ctx->buf("pfh_kcount").as<int>((size_t)nq);
    // workgroups per query: enough parts that the longest neighbourhood is a small share of the
    // call and a few queries still fill the device (the counts, hence the rows, do not depend on it)
    const int split = (int)std::min<int64_t>(kMaxSplit, std::max<int64_t>(kMinSplit, ceil_div(kSplitBlocks, nq)));
    TimeScope ts(ctx, "pfh", true);
    PFX_HIP(hipMemsetAsync(hcount, 0, sizeof(int) * (size_t)nq * kCntStride, st));
    const size_t lds_head = sizeof(int) * kHeadInts, lds = lds_head + 2 * sizeof(float4) * kPfhCapLds;
    PFX_HIP(hipFuncSetAttribute((const void*)k_pfh<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // one workgroup per query (their costs differ by the square of k: dispatched as CUs free up)
    k_pfh<false><<<(unsigned)std::min<int64_t>(nq * split, 1 << 20), kPT, lds, st>>>(
        g, snx, sny, snz, qx, qy, qz, nq, rr, split, hcount, kcount, err, ovf, nullptr, 0);
    if (overflow_pass)
      k_pfh<true><<<kOvfBlocks, kPT, lds_head, st>>>(g, snx, sny, snz, qx, qy, qz, nq, rr, 1, hcount, kcount, err, ovf,
                                                     scratch, gcap);
    k_pfh_finalize<<<(unsigned)std::min<int64_t>(ceil_div(nq * kDesc, 256), 4096), 256, 0, st>>>(nq, hcount, kcount,
                                                                                                 out);
    check_launch("k_pfh");
  }
  report_post(ctx, kRepPfh, err);
}

// The last pfh_dev's statistics, and its capacity check (PFX_ERR_CAPACITY).
void pfh_report(pfx_ctx* ctx, const int* h) {
  unsigned long long pr;
  std::memcpy(&pr, h + 2, sizeof(pr));
  ctx->stats["pfh_pairs"] = (int64_t)pr;
  ctx->stats["pfh_global"] = h[1];
  ctx->stats["pfh_kmax"] = h[4];
  if (h[0] > 0)
    throw Error(PFX_ERR_CAPACITY, "pfh: a query has " + std::to_string(h[0]) + " neighbours (> " +
                                      std::to_string(kPfhMaxK) + " supported)");
}

}  // namespace pfx
