// pfx_intensity_spin.hip -- IntensitySpinEstimation<PointXYZI, Histogram<20>> (evaluation.cpp:466-514)
// on gfx950.  DESIGN.md "Intensity spin" and "Intensity spin: the contract".
//
// k_ispin: one 256-thread workgroup per centre, the keys sorted in LDS by the two passes of
// pfx_two_pass.h.  A first sweep over the keys finds the neighbourhood's intensity range (order-free:
// a minimum and a maximum that skip NaN).  Then, a sub-chunk of `tile` neighbours at a time:
//   weights  one thread per neighbour walks the D x I image and writes the neighbour's weight of
//            every bin, pfx_expf(...) inside its window and +0 outside, into its row of a tile in
//            the 16 KiB behind the keys (the row stride is odd: the writers' lanes fall on distinct
//            banks); this is where the time goes (up to D I double-precision exponentials a
//            neighbour) and every lane is busy with it;
//   sums     one lane per bin adds its column of the tile in ascending neighbour order into a float
//            accumulator that stays in a register for the whole centre (the lanes of a row's bins read
//            consecutive words).  An accumulator starts at +0 and receives only values >= +0 (or a
//            NaN, which stays), so adding the +0 of a bin outside the window changes no bit: the bin
//            lanes need no window test.
// No floating-point atomic, no reordered addition.  Late errors and statistics go through the
// deferred reports (ispin_report).  A NaN is written as 0x7fc00000, here and in the restatement.
#include <cfloat>
#include <cmath>

#include <string>

#include "pfx_expf.h"
#include "pfx_two_pass.h"

namespace pfx {
namespace {

constexpr int kIspinTileWords = (int)(kTwoPassAuxBytes / sizeof(float));  // floats of the weight tile
constexpr int kIspinMaxBins = 16;                                         // per axis

// row stride of the tile (odd) and neighbours of a sub-chunk, for S = D I bins
__host__ __device__ constexpr int ispin_stride(int S) { return S | 1; }
__host__ __device__ constexpr int ispin_tile_of(int S) {
  return kIspinTileWords / ispin_stride(S) < kTwoPassChunk ? kIspinTileWords / ispin_stride(S) : kTwoPassChunk;
}
static_assert(ispin_tile_of(kIspinMaxBins * kIspinMaxBins) >= 1, "the largest image has a row in the tile");
static_assert(ispin_tile_of(1) * ispin_stride(1) <= kIspinTileWords &&
                  ispin_tile_of(20) * ispin_stride(20) <= kIspinTileWords &&
                  ispin_tile_of(256) * ispin_stride(256) <= kIspinTileWords,
              "the tile fits the sort scratch");

// t = 3 sigma and c = 1 / (2 sigma sigma) (the host's floats); gauss == 0 is sigma == 0.
template <int CAP>
__global__ void __launch_bounds__(kTwoPassChunk) k_ispin(GridView g, const float* __restrict__ si,
                                                         const float* __restrict__ qx, const float* __restrict__ qy,
                                                         const float* __restrict__ qz, int64_t nq, float rr, float rad,
                                                         int D, int I, int gauss, float t, float c,
                                                         const int32_t* __restrict__ list,
                                                         const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                         float* __restrict__ out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of the tile
  float* tile = reinterpret_cast<float*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  __shared__ float s_mn[kTwoPassChunk / 64], s_mx[kTwoPassChunk / 64];
  const int tid = threadIdx.x;
  const int S = D * I, stride = ispin_stride(S), T = ispin_tile_of(S);
  const float eps = FLT_EPSILON;
  const float dden = rad + eps;
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    const int k = two_pass_neighbors<CAP>(g, qx[q], qy[q], qz[q], rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) count_neighbors(k, err);
    if (k == 0) {  // (a non-finite centre has no candidate run)
      if (tid < S) out[q * S + tid] = __uint_as_float(0x7fc00000u);
      continue;
    }
    __syncthreads();  // the sort is done with its scratch
    // the intensity range: a NaN fails both comparisons, and the order decides no value used later
    float mn = FLT_MAX, mx = -FLT_MAX;
    for (int n = tid; n < k; n += kTwoPassChunk) {
      const float v = si[key_idx(keys[n])];
      mn = v < mn ? v : mn;
      mx = mx < v ? v : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float a = __shfl_xor(mn, o), b = __shfl_xor(mx, o);
      mn = a < mn ? a : mn;
      mx = mx < b ? b : mx;
    }
    if ((tid & 63) == 0) {
      s_mn[tid >> 6] = mn;
      s_mx[tid >> 6] = mx;
    }
    __syncthreads();
    mn = s_mn[0];
    mx = s_mx[0];
#pragma unroll
    for (int w = 1; w < kTwoPassChunk / 64; ++w) {
      mn = s_mn[w] < mn ? s_mn[w] : mn;
      mx = mx < s_mx[w] ? s_mx[w] : mx;
    }
    const float iden = (mx - mn) + eps;
    float acc = 0.f;
    for (int c0 = 0; c0 < k; c0 += T) {
      const int m = min(T, k - c0);
      if (tid < m) {
        const uint64_t key = keys[c0 + tid];
        const float d = ((float)D * sqrtf(key_d2(key))) / dden;
        const float iv = ((float)I * (si[key_idx(key)] - mn)) / iden;
        // the window [d_lo, d_hi] x [i_lo, i_hi]; empty for an intensity coordinate that is no
        // number (x86's int casts of it make PCL's window empty too)
        int d_lo = 1, d_hi = 0, i_lo = 1, i_hi = 0;
        if (isfinite(iv)) {
          if (gauss) {
            d_lo = max((int)floorf(d - t), 0);
            d_hi = min((int)ceilf(d + t), D - 1);
            i_lo = max((int)floorf(iv - t), 0);
            i_hi = min((int)ceilf(iv + t), I - 1);
          } else {  // sigma == 0: the one bin, dropped when it lies beyond the image
            d_lo = d_hi = (int)d;
            i_lo = i_hi = (int)iv;
          }
        }
        float* row = tile + tid * stride;
        for (int dj = 0; dj < D; ++dj) {
          const float a = d - (float)dj;
          const float ea = (-(a * a)) * c;
          const bool din = dj >= d_lo && dj <= d_hi;
          for (int ii = 0; ii < I; ++ii) {
            float w = 0.0f;
            if (din && ii >= i_lo && ii <= i_hi) {
              const float b = iv - (float)ii;
              w = gauss ? pfx_expf(ea - (b * b) * c) : 1.0f;
            }
            row[dj * I + ii] = w;
          }
        }
      }
      __syncthreads();
      if (tid < S) {
        const float* col = tile + tid;
        for (int n = 0; n < m; ++n) acc = acc + col[n * stride];  // ascending: the neighbour order
      }
      __syncthreads();  // the tile is read before the next sub-chunk's weights overwrite it
    }
    if (tid < S) out[q * S + tid] = canon_nan(acc);
    // (the barrier above: the tile is read before the next centre's sort scratch overwrites it)
  }
}

}  // namespace

int ispin_cap_small() { return kTwoPassCapSmall; }
int ispin_tile_words() { return kIspinTileWords; }
int ispin_tile(int S) { return ispin_tile_of(S); }

void ispin_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* si, int64_t ns,
               const float* cx, const float* cy, const float* cz, int64_t nq, double r, int D, int I, float sigma,
               float* out) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, kRepIspin);
  if (ns == 0) {
    fill_nan(ctx, out, nq * D * I);
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    const float rr = (float)(r * r), rad = (float)r;
    const int gauss = sigma > 0.0f;
    const float t = 3 * sigma, c = gauss ? 1.0f / ((2.0f * sigma) * sigma) : 0.0f;
    TimeScope ts(ctx, "intensity_spin", true);
    two_pass(ctx, ns, nq, "ispin_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_ispin<cap()>, blocks, lds, st, g, si, cx, cy, cz, nq, rr, rad, D, I, gauss, t, c,
                               list, n_list, over, out, err);
             });
    check_launch("k_ispin");
  }
  report_post(ctx, kRepIspin, err);
}

void ispin_report(pfx_ctx* ctx, const int* h) { two_pass_report(ctx, h, "ispin", "intensity_spin"); }

}  // namespace pfx
