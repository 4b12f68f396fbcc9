// pfx_exact_sum.h -- PCL's sequential double sum of float terms, formed exactly in parallel.
//
// Every term is a float, so all are multiples of 2^L (L = ulp exponent of the smallest non-zero
// term); when the integer sum in units of 2^L stays below 2^53, every partial sum of the
// sequential loop is exact and equals the order-free integer sum.  Otherwise one workgroup runs
// the sequential loop (k_res_sequential).  A NaN term means "no term"; terms are >= 0.
// Users: the cloud resolution (pfx_iss.hip), ICP's mean squared error and fitness score
// (pfx_icp.hip).
#pragma once
#include <algorithm>
#include <cmath>

#include "pfx_internal.h"

namespace pfx {

// Exact sum of the terms.  Per block: count, smallest positive term (its ulp exponent L_b) and
// the integer sum in units of 2^L_b; the final pass rescales every block to the global L.
struct ResPart {
  unsigned long long count, isum;
  double dsum;
  unsigned int minbits, overflow;
};
struct ResAcc {
  unsigned long long count, isum;
  double dsum;
  int L, exact;
};

__device__ __forceinline__ int ulp_exp(unsigned int bits) {  // exponent of the ulp of a normal float
  return (int)((bits >> 23) & 0xff) - 150;
}

static __global__ void __launch_bounds__(256) k_res_partial(const float* __restrict__ term, int64_t n,
                                                     ResPart* __restrict__ part) {
  __shared__ unsigned long long s_c[4], s_i[4];
  __shared__ double s_d[4];
  __shared__ unsigned int s_m[4], s_o[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t stride = (int64_t)gridDim.x * 256;
  unsigned long long cnt = 0;
  unsigned int mn = 0xffffffffu;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += stride) {
    const float t = term[i];
    if (isnan(t)) continue;
    ++cnt;
    if (t > 0.0f) mn = min(mn, __float_as_uint(t));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    mn = min(mn, (unsigned int)__shfl_xor((int)mn, o));
  }
  if (lane == 0) {
    s_c[wv] = cnt;
    s_m[wv] = mn;
  }
  __syncthreads();
  mn = min(min(s_m[0], s_m[1]), min(s_m[2], s_m[3]));
  const int L = mn == 0xffffffffu ? 0 : ulp_exp(mn);
  unsigned long long is = 0;
  double ds = 0.0;
  unsigned int ovf = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n; i += stride) {
    const float t = term[i];
    if (!(t > 0.0f)) continue;  // NaN (no term) and zeros add nothing
    const unsigned int b = __float_as_uint(t);
    const int sh = ulp_exp(b) - L;  // t = m * 2^(L + sh)
    if (sh > 39) {
      ovf = 1;
      continue;
    }
    is += (unsigned long long)((b & 0x7fffffu) | 0x800000u) << sh;
    ds += (double)t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    is += __shfl_xor(is, o);
    ds += __shfl_xor(ds, o);
    ovf |= __shfl_xor(ovf, o);
  }
  if (lane == 0) {
    s_i[wv] = is;
    s_d[wv] = ds;
    s_o[wv] = ovf;
  }
  __syncthreads();
  if (tid == 0) {
    ResPart r;
    r.count = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    r.isum = s_i[0] + s_i[1] + s_i[2] + s_i[3];  // < 2^63 each: a wrap shows in dsum below
    r.dsum = (s_d[0] + s_d[1]) + (s_d[2] + s_d[3]);
    r.minbits = mn;
    r.overflow = s_o[0] | s_o[1] | s_o[2] | s_o[3];
    part[blockIdx.x] = r;
  }
}

// one wave: global L = min over blocks, then every block sum rescaled to 2^L (exactness checked)
static __global__ void __launch_bounds__(64) k_res_final(const ResPart* __restrict__ part, int nb, ResAcc* __restrict__ acc) {
  const int lane = threadIdx.x;
  unsigned int mn = 0xffffffffu;
  for (int b = lane; b < nb; b += 64) mn = min(mn, part[b].minbits);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mn = min(mn, (unsigned int)__shfl_xor((int)mn, o));
  const int L = mn == 0xffffffffu ? 0 : ulp_exp(mn);
  unsigned long long cnt = 0, is = 0;
  double ds = 0.0;
  int bad = 0;
  for (int b = lane; b < nb; b += 64) {
    const ResPart r = part[b];
    cnt += r.count;
    ds += r.dsum;
    if (r.overflow) bad = 1;
    if (r.isum == 0) continue;
    const int sh = ulp_exp(r.minbits) - L;
    // the block sum in units of 2^L must stay below 2^53 (and its own sum must not have wrapped)
    if (r.dsum >= ldexp(1.0, ulp_exp(r.minbits) + 62) || sh > 52 || r.isum >= (1ull << (53 - sh))) {
      bad = 1;
      continue;
    }
    is += r.isum << sh;  // < 2^53 per block, <= 16 blocks per lane: no wrap
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    is += __shfl_xor(is, o);
    ds += __shfl_xor(ds, o);
    bad |= __shfl_xor(bad, o);
  }
  if (lane == 0) {
    acc->count = cnt;
    acc->isum = is;
    acc->dsum = ds;
    acc->L = L;
    acc->exact = (!bad && is < (1ull << 53)) ? 1 : 0;
  }
}

// PCL's loop verbatim: one workgroup, terms staged through LDS, one lane adds in index order
static __global__ void __launch_bounds__(256) k_res_sequential(const float* __restrict__ term, int64_t n,
                                                        double* __restrict__ out) {
  __shared__ float s[4096];
  double sum = 0.0;
  for (int64_t b = 0; b < n; b += 4096) {
    for (int k = threadIdx.x; k < 4096; k += 256) s[k] = b + k < n ? term[b + k] : __int_as_float(0x7fc00000);
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll 16
      for (int k = 0; k < 4096; ++k) {
        const float t = s[k];
        if (!isnan(t)) sum += (double)t;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = sum;
}

// launches the two passes over term[0..n); *acc is complete in stream order
inline int exact_sum_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 256), 1), 1024); }
inline void exact_sum_launch(pfx_ctx* ctx, const float* term, int64_t n, ResPart* part, ResAcc* acc) {
  const int nblk = exact_sum_blocks(n);
  k_res_partial<<<nblk, 256, 0, ctx->stream>>>(term, n, part);
  k_res_final<<<1, 64, 0, ctx->stream>>>(part, nblk, acc);
  check_launch("k_res_sum");
}
// the sum from a completed ResAcc; when it is not exact, the sequential loop and one more
// synchronisation (seq: one device double)
inline double exact_sum_finish(pfx_ctx* ctx, const ResAcc& h_acc, const float* term, int64_t n, double* seq) {
  if (h_acc.exact != 0) return std::ldexp((double)h_acc.isum, h_acc.L);
  double sum = 0.0;
  k_res_sequential<<<1, 256, 0, ctx->stream>>>(term, n, seq);
  check_launch("k_res_sequential");
  PFX_HIP(hipMemcpyAsync(&sum, seq, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PFX_HIP(hipStreamSynchronize(ctx->stream));
  return sum;
}

}  // namespace pfx
