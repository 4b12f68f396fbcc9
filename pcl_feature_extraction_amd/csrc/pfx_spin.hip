// pfx_spin.hip -- SpinImageEstimation<PointXYZRGB,Normal,Histogram<153>> (evaluation.cpp:514-553)
// on gfx950.  DESIGN.md "Spin images" and "Spin images: the contract".
//
// One 256-thread workgroup per query:
//   1. radius neighbours in FLANN order, the keys in LDS (pfx_two_pass.h: the two passes);
//   2. per chunk of kSpinChunk neighbours every thread turns its neighbour into a record, the
//      four double weights of the bilinear update, and sets its bit in the chunk's row mask of
//      its alpha_bin and column mask of its beta_bin (64-bit integer atomics in LDS, order-free);
//      a neighbour that adds nothing sets no bit;
//   3. one thread per bin (S = (W + 1)(2W + 1) <= 561: up to three bins a thread): the records
//      that touch bin (a, b) are (row[a] | row[a - 1]) & (col[b] | col[b - 1]), and which of the
//      two row and column masks holds a record's bit says which corner the bin is of it.  The
//      thread takes the set bits in ascending order, four weight loads in flight, and adds them
//      one by one.  A bin's double accumulator stays in a register for the whole query and a
//      bin's additions are in FLANN neighbour order.  No floating-point atomic (every bin walking
//      every record of the chunk instead, an LDS broadcast per record, took twice the time:
//      DESIGN.md);
//   4. m.sum() in Eigen 3.2's order (pfx_eigen_redux.h: four lanes hold the four running sums,
//      one lane combines them), m *= 1 / sum for k > 1, the cast to float.
// Stream-ordered: errors and statistics go through the deferred reports (spin_report).
#include <cfloat>
#include <climits>
#include <cstring>

#include "pfx_eigen_redux.h"
#include "pfx_two_pass.h"

namespace pfx {
namespace {

constexpr int kSpinChunk = kTwoPassChunk;
constexpr int kSpinMaxW = 16;
constexpr int kSpinMaxS = (kSpinMaxW + 1) * (2 * kSpinMaxW + 1);  // 561
constexpr int kSpinPasses = (kSpinMaxS + kSpinChunk - 1) / kSpinChunk;  // bins per thread
constexpr int kSpinWords = kSpinChunk / 64;                       // mask words per chunk
constexpr int kSpinMaskRows = (kSpinMaxW + 2) + (2 * kSpinMaxW + 2);  // row masks, then column masks

// The family's own words.  Sticky: INT_MAX - the first row with too few neighbours / with a cosine
// out of range (0: none).  Per call: the rows with too few neighbours / a cosine out of range.
constexpr int kWordFewRow = kWordSticky, kWordBadRow = kWordSticky + 1;
constexpr int kWordFew = kWordOwn, kWordBad = kWordOwn + 1;

// The 16 KiB behind the keys: the bucketed sort's scratch, then (the sort done) the chunk's records
// and the finished matrix in Eigen's column-major order.
struct SpinAux {
  union {
    double w[kSpinChunk][4];    // (1-a)(1-b), a(1-b), (1-a)b, ab
    double mat[kSpinMaxS + 3];  // (after the last chunk)
  };
  // Two buffers (the other one is cleared while one is filled).  Row mask a + 1: the chunk's
  // records with alpha_bin == a; column mask b + 1 (behind the W + 2 row masks): beta_bin == b.
  // Mask 0 of either kind stays empty, so bin (a, b) reads masks a, a + 1 and b, b + 1.
  unsigned long long mask[2][kSpinMaskRows][kSpinWords];
  double lane[4];
  double sum, inv;
  int bad;
};
static_assert(sizeof(SpinAux) <= kTwoPassAuxBytes, "the records fit the sort scratch");

struct SpinParams {
  double bin_size, support_cos;
  float rr;
  int W, min_pts;
};

// `std::max (-1.0, std::min (1.0, c))` with libstdc++'s argument order, stated: a NaN compares
// false both times, so min returns its first argument, 1.0
__device__ __forceinline__ double clamp_cos(double c) {
  const double lo = c < 1.0 ? c : 1.0;
  return -1.0 < lo ? lo : -1.0;
}

// list (nullable): the queued queries with their device-side count; over (nullable): where a query
// with more than CAP neighbours is queued (else it is beyond every capacity: err[0]).
template <int CAP>
__global__ void __launch_bounds__(kSpinChunk) k_spin(GridView g, const float* __restrict__ snx,
                                                     const float* __restrict__ sny, const float* __restrict__ snz,
                                                     const float* __restrict__ qx, const float* __restrict__ qy,
                                                     const float* __restrict__ qz, const float* __restrict__ ax,
                                                     const float* __restrict__ ay, const float* __restrict__ az,
                                                     int64_t nq, const int32_t* __restrict__ list,
                                                     const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                     SpinParams P, float* __restrict__ out, double* __restrict__ raw,
                                                     double* __restrict__ sums, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of SpinAux
  SpinAux& A = *reinterpret_cast<SpinAux*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const int W = P.W, rows = W + 1, cols = 2 * W + 1, S = rows * cols;
  const double lim = 1.0 + (double)(10.0f * FLT_EPSILON), tiny = (double)(10.0f * FLT_EPSILON);
  const double edge = P.bin_size * W;
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    // (a non-finite query has no candidate run: k = 0)
    const int k = two_pass_neighbors<CAP>(g, cx, cy, cz, P.rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) {
      count_neighbors(k, err);
      A.bad = 0;
    }
    if (k < P.min_pts) {  // PCL throws: reported after the call, the row is unspecified
      if (tid == 0) {
        atomicAdd(err + kWordFew, 1);
        atomicMax(err + kWordFewRow, INT_MAX - (int)q);
      }
      continue;
    }
    const f3 axis = mk3(ax[q], ay[q], az[q]);
    double acc[kSpinPasses];
#pragma unroll
    for (int p = 0; p < kSpinPasses; ++p) acc[p] = 0.0;
    const int nmask = (3 * W + 4) * kSpinWords;  // the masks in use: W + 2 rows, 2W + 2 columns
    for (int i = tid; i < nmask; i += kSpinChunk) (&A.mask[0][0][0])[i] = 0ull;
    __syncthreads();  // A.bad and the first masks are clear, the sort is done with its scratch
    int par = 0;
    for (int c0 = 0; c0 < k; c0 += kSpinChunk, par ^= 1) {
      const int m = min(kSpinChunk, k - c0);
      // (the other buffer: read during the previous chunk, filled during the next)
      for (int i = tid; i < nmask; i += kSpinChunk) (&A.mask[par ^ 1][0][0])[i] = 0ull;
      if (tid < m) {
        const int32_t idx = key_idx(keys[c0 + tid]);
        double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
        bool bad = false, use = true;
        if (P.support_cos > 0.0) {
          const double c = (double)dot4(axis, mk3(snx[idx], sny[idx], snz[idx]));
          if (fabs(c) > lim) bad = true;
          else if (fabs(clamp_cos(c)) < P.support_cos) use = false;  // counter-directed normals stay
        }
        if (use && !bad) {
          const f3 d = sub3(mk3(g.ux[idx], g.uy[idx], g.uz[idx]), mk3(cx, cy, cz));
          const double dn = (double)sqrtf(sqn4(d));
          if (!(fabs(dn) < tiny)) {
            double cs = (double)dot4(d, axis) / dn;
            if (fabs(cs) > lim) {
              bad = true;
            } else {
              cs = clamp_cos(cs);
              double beta = dn * cs;
              double alpha = dn * sqrt(1.0 - cs * cs);
              if (!(fabs(beta) >= edge || alpha >= edge)) {  // inside the cylinder
                // (alpha / bin_size and beta / bin_size are formed once unless the bin was adjusted:
                // the same quotients PCL forms twice)
                double qb = beta / P.bin_size, qa = alpha / P.bin_size;
                int beta_bin = (int)floor(qb) + W;
                int alpha_bin = (int)floor(qa);
                if (alpha_bin == W) {
                  alpha_bin--;
                  alpha = P.bin_size * (alpha_bin + 1) - DBL_EPSILON;
                  qa = alpha / P.bin_size;
                }
                if (beta_bin == 2 * W) {
                  beta_bin--;
                  beta = P.bin_size * (beta_bin - W + 1) - DBL_EPSILON;
                  qb = beta / P.bin_size;
                }
                const double a = qa - (double)alpha_bin;
                const double b = qb - (double)(beta_bin - W);
                // (bins that rounding pushed outside the matrix would be a write out of PCL's
                // array: never taken for finite input, and never stored here)
                if (alpha_bin >= 0 && alpha_bin < W && beta_bin >= 0 && beta_bin < 2 * W) {
                  w0 = (1.0 - a) * (1.0 - b);
                  w1 = a * (1.0 - b);
                  w2 = (1.0 - a) * b;
                  w3 = a * b;
                  const unsigned long long bit = 1ull << (tid & 63);
                  atomicOr(&A.mask[par][alpha_bin + 1][tid >> 6], bit);
                  atomicOr(&A.mask[par][(W + 2) + beta_bin + 1][tid >> 6], bit);
                }
              }
            }
          }
        }
        A.w[tid][0] = w0;
        A.w[tid][1] = w1;
        A.w[tid][2] = w2;
        A.w[tid][3] = w3;
        if (bad) A.bad = 1;
      }
      __syncthreads();
#pragma unroll
      for (int p = 0; p < kSpinPasses; ++p) {
        const int L = tid + p * kSpinChunk;
        if (p * kSpinChunk < S && L < S) {
          double s = acc[p];
          const int aL = L % rows, bL = (W + 2) + L / rows;
          for (int wd = 0; wd * 64 < m; ++wd) {
            // ra / ca: the records one row / one column below this bin (it is their corner 1 / 2)
            const unsigned long long ra = A.mask[par][aL][wd], ca = A.mask[par][bL][wd];
            unsigned long long hit = (ra | A.mask[par][aL + 1][wd]) & (ca | A.mask[par][bL + 1][wd]);
            while (hit) {  // ascending: a bin's additions stay in neighbour order
              constexpr int U = 4;  // weight loads in flight (their addresses do not wait for the sum)
              bool h[U];
              double v[U];
#pragma unroll
              for (int u = 0; u < U; ++u) {
                h[u] = hit != 0;
                const int j = h[u] ? __builtin_ctzll(hit) : 0;
                hit &= hit - 1;
                v[u] = A.w[wd * 64 + j][(int)((ra >> j) & 1) | ((int)((ca >> j) & 1) << 1)];
              }
#pragma unroll
              for (int u = 0; u < U; ++u)
                if (h[u]) s = s + v[u];
            }
          }
          acc[p] = s;
        }
      }
      __syncthreads();  // the records are read before the next chunk's overwrite them
    }
#pragma unroll
    for (int p = 0; p < kSpinPasses; ++p) {
      const int L = tid + p * kSpinChunk;
      if (L < S) A.mat[L] = acc[p];
    }
    __syncthreads();
    if (k > 1) {  // the neighbour count, not the number that contributed
      if (tid < 4) A.lane[tid] = eigen_redux_lane(A.mat, S, tid);
      __syncthreads();
      if (tid == 0) {
        const double s = eigen_redux_finish(A.lane[0], A.lane[1], A.lane[2], A.lane[3], A.mat, S);
        A.sum = s;
        A.inv = 1.0 / s;  // Eigen 3.2's `/=` by a scalar multiplies by the reciprocal
      }
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < kSpinPasses; ++p) {
      const int L = tid + p * kSpinChunk;
      if (L < S) {
        const int64_t o = q * S + (int64_t)(L % rows) * cols + L / rows;
        // k > 1 with nothing contributing: 0 x inf.  No NaN enters the matrix, so a NaN here is one
        // the multiplication made: on x86-64 that is the default NaN, whose sign bit is set, and
        // the conversion to float keeps the sign.  Stated, not left to the device's default NaN.
        const float v = (float)(k > 1 ? acc[p] * A.inv : acc[p]);
        out[o] = v != v ? __uint_as_float(0xffc00000u) : v;
        if (raw) raw[o] = acc[p];
      }
    }
    if (tid == 0) {
      if (sums) sums[q] = k > 1 ? A.sum : 0.0;
      if (A.bad) {
        atomicAdd(err + kWordBad, 1);
        atomicMax(err + kWordBadRow, INT_MAX - (int)q);
      }
    }
    __syncthreads();  // A is read before the next query's sort scratch overwrites it
  }
}

// no surface: every neighbourhood is empty
__global__ void k_spin_empty(int64_t nq, int min_pts, int* __restrict__ err) {
  if (threadIdx.x == 0 && blockIdx.x == 0 && min_pts > 0) {
    err[kWordFew] = (int)(nq < INT_MAX ? nq : INT_MAX);
    atomicMax(err + kWordFewRow, INT_MAX);
  }
}

}  // namespace

int spin_cap_small() { return kTwoPassCapSmall; }
int spin_chunk() { return kSpinChunk; }

void spin_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
              const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, const float* ax,
              const float* ay, const float* az, int64_t nq, double r, const pfx_spin_params& prm, float* out,
              double* raw, double* sums) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  const int W = prm.image_width, S = (W + 1) * (2 * W + 1);
  int* err = report_words(ctx, kRepSpin);
  if (ns == 0) {
    PFX_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)nq * S, st));
    if (raw) PFX_HIP(hipMemsetAsync(raw, 0, sizeof(double) * (size_t)nq * S, st));
    if (sums) PFX_HIP(hipMemsetAsync(sums, 0, sizeof(double) * (size_t)nq, st));
    k_spin_empty<<<1, 64, 0, st>>>(nq, prm.min_pts_neighb, err);
    check_launch("k_spin_empty");
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    SpinParams P;
    P.bin_size = r / W / std::sqrt(2.0);  // left to right, in double
    P.support_cos = prm.support_angle_cos;
    P.rr = (float)(r * r);
    P.W = W;
    P.min_pts = prm.min_pts_neighb;
    TimeScope ts(ctx, "spin_image", true);
    two_pass(ctx, ns, nq, "spin_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_spin<cap()>, blocks, lds, st, g, snx, sny, snz, qx, qy, qz, ax, ay, az, nq, list,
                               n_list, over, P, out, raw, sums, err);
             });
    check_launch("k_spin");
  }
  report_post(ctx, kRepSpin, err);
}

// The last spin_dev's statistics and its errors (PFX_ERR_CAPACITY; PFX_ERR_INVALID where PCL throws).
void spin_report(pfx_ctx* ctx, const int* h) {
  unsigned long long nb;
  std::memcpy(&nb, h + kWordNeighbors, sizeof(nb));
  ctx->stats["spin_neighbors"] = (int64_t)nb;
  ctx->stats["spin_queued"] = h[kWordQueued];
  ctx->stats["spin_kmax"] = h[kWordKmax];
  ctx->stats["spin_too_few"] = h[kWordFew];
  ctx->stats["spin_bad_cos"] = h[kWordBad];
  const int cap = h[kWordOver], few = h[kWordFewRow], bad = h[kWordBadRow];
  if (cap > 0 || few > 0 || bad > 0) {
    if (cap > 0)
      throw Error(PFX_ERR_CAPACITY, "spin_image: a query has " + std::to_string(cap) + " neighbours (> " +
                                        std::to_string(kTwoPassCap) + " supported)");
    // the first offending row; a row breaks one rule only (too few neighbours stops it)
    if (few >= bad)
      throw Error(PFX_ERR_INVALID, "spin_image: query row " + std::to_string(INT_MAX - few) +
                                       " has too few neighbours (min_pts_neighb)");
    throw Error(PFX_ERR_INVALID, "spin_image: query row " + std::to_string(INT_MAX - bad) +
                                     " has a cosine out of range (|cos| > 1 + 10 FLT_EPSILON: an axis or normal"
                                     " that is not of unit length)");
  }
}

}  // namespace pfx
