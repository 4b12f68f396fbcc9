// pfx_board.hip -- BOARDLocalReferenceFrameEstimation<PointXYZRGB, Normal, ReferenceFrame>
// (evaluation.cpp:372-393) on gfx950, without hole analysis.  DESIGN.md "BOARD frames" and "BOARD:
// the contract".
//
// One kernel, k_board<CAP>, in the shape of k_moments (pfx_moments.hip): one 256-thread workgroup per
// centre, the keys sorted in LDS (pfx_neighbors.h), gathered once at max(r, tangent_radius).  The
// support and the tangent set are prefixes of the sorted keys (d2 is the same float in both), cut by
// their strict bounds; the margin neighbours (d2 > margin2) are a suffix of the tangent set.  The
// neighbours' records are staged in LDS a chunk of kBoardChunk at a time, one lane per accumulator:
//   first pass   three sequential float chains over the positions (the centroid) and three over the
//                normals (their sum), lanes 0..5;
//   second pass  six sequential double chains over the products of the demeaned positions;
//   thread 0     the eigen solve (pfx_eigen3.h) and the sign of z;
//   every lane   z . n of its neighbours of the scanned range, then a wave and a workgroup reduction
//                on (cos, position in the list) that returns the serial scan's first strict minimum;
//   thread 0     the axes.
// No floating-point atomic.  Both passes of pfx_two_pass.h; late errors and statistics through the
// deferred reports (board_report; no words of its own).  A NaN is written as 0x7fc00000, here and in
// the restatement.
#include <cfloat>
#include <climits>

#include "pfx_eigen3.h"
#include "pfx_two_pass.h"

namespace pfx {
namespace {

constexpr int kBoardChunk = kTwoPassChunk;

// The 16 KiB behind the keys: the bucketed sort's scratch, then (the sort done) the records.  The
// six chain lanes of the first pass read pos[j].xyz and nrm[j].xyz in one step.  Two tiles of 4 KiB
// back to back would put nrm[j] on the banks of pos[j] (a two-way conflict at every step); the four
// floats between them move it to the banks of pos[j + 1], so the step touches six banks: 4j, 4j + 1,
// 4j + 2 and 4j + 4, 4j + 5, 4j + 6.  The staging stores are one float4 per lane at a 16-byte
// stride in either tile, which has no conflict.
struct BoardAux {
  float4 pos[kBoardChunk];  // x, y, z of the chunk's neighbours; in the second pass minus the centroid
  float pad[4];
  float4 nrm[kBoardChunk];  // their normals (first pass only)
  double sums[6];           // xx xy xz yy yz zz of the demeaned positions
  float acc[6];             // the centroid, the normals' sum
  float z[3];               // the z axis, sign settled
  float wcos[kBoardChunk / 64];
  int wpos[kBoardChunk / 64];
};
static_assert(sizeof(BoardAux) <= kTwoPassAuxBytes, "the records fit the sort scratch");

// the number of keys[0..k) whose d2 is < bound (strict == true) or <= bound; keys ascending in d2.
// Every lane walks the same path (broadcast reads).  A NaN bound compares false: 0, or k.
template <bool kStrict>
__device__ __forceinline__ int keys_below(const uint64_t* keys, int k, float bound) {
  int lo = 0, hi = k;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float d2 = key_d2(keys[mid]);
    const bool below = kStrict ? d2 < bound : !(d2 > bound);
    if (below) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// (cos, position) b before a in the serial scan's order: the smaller cosine, ties to the earlier
// neighbour; a position of INT_MAX is "none"
__device__ __forceinline__ bool board_better(float ca, int ja, float cb, int jb) {
  return jb != INT_MAX && (ja == INT_MAX || cb < ca || (cb == ca && jb < ja));
}

// rr_g: the gather's bound, max(rr_s, rr_t); rr_s: the support's; rr_t: the tangent set's.
// list (nullable): the queued queries with their device-side count; over (nullable): where a query
// with more than CAP keys is queued (else it is beyond every capacity: err[0]).
template <int CAP>
__global__ void __launch_bounds__(kBoardChunk) k_board(GridView g, const float* __restrict__ snx,
                                                       const float* __restrict__ sny, const float* __restrict__ snz,
                                                       const float* __restrict__ qx, const float* __restrict__ qy,
                                                       const float* __restrict__ qz, int64_t nq, float rr_g, float rr_s,
                                                       float rr_t, float margin2, const int32_t* __restrict__ list,
                                                       const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                       float* __restrict__ out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of BoardAux
  BoardAux& A = *reinterpret_cast<BoardAux*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const float nan = __uint_as_float(0x7fc00000u);
  // accumulator `tid` of the second pass multiplies components ia and ib: xx xy xz yy yz zz
  const int t6 = tid < 6 ? tid : 0;  // (the other lanes only stage records)
  const int ia = t6 < 3 ? 0 : t6 < 5 ? 1 : 2;
  const int ib = t6 < 3 ? t6 : t6 < 5 ? t6 - 2 : 2;
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    const float px = qx[q], py = qy[q], pz = qz[q];
    // (a non-finite query has no candidate run: k = 0)
    const int k = two_pass_neighbors<CAP>(g, px, py, pz, rr_g, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) count_neighbors(k, err);
    const int ks = keys_below<true>(keys, k, rr_s);  // the support
    const int kt = keys_below<true>(keys, k, rr_t);  // the tangent set
    // the margin neighbours are [j0, kt); without one the scan takes the whole tangent set
    const int j0 = keys_below<false>(keys, kt, margin2);
    const int lo = j0 < kt ? j0 : 0;
    if (ks < 6 || kt == 0) {
      if (tid < 9) out[9 * q + tid] = nan;
      continue;
    }
    __syncthreads();  // the sort is done with its scratch
    // ---- first pass: the centroid and the normals' sum ----
    float a = 0.f;
    for (int c0 = 0; c0 < ks; c0 += kBoardChunk) {
      const int m = min(kBoardChunk, ks - c0);
      if (tid < m) {
        const int32_t idx = key_idx(keys[c0 + tid]);
        A.pos[tid] = make_float4(g.ux[idx], g.uy[idx], g.uz[idx], 0.f);
        A.nrm[tid] = make_float4(snx[idx], sny[idx], snz[idx], 0.f);
      }
      __syncthreads();
      if (tid < 6) {
        const float* rp = tid < 3 ? reinterpret_cast<const float*>(A.pos) + tid
                                  : reinterpret_cast<const float*>(A.nrm) + (tid - 3);
        for (int j = 0; j < m; ++j) a = a + rp[4 * j];
      }
      __syncthreads();
    }
    if (tid < 3) A.acc[tid] = a / (float)ks;
    else if (tid < 6) A.acc[tid] = a;
    __syncthreads();
    const float cx = A.acc[0], cy = A.acc[1], cz = A.acc[2];
    // ---- second pass: the six sums of the demeaned positions' products, in double ----
    double s = 0.0;
    for (int c0 = 0; c0 < ks; c0 += kBoardChunk) {
      const int m = min(kBoardChunk, ks - c0);
      if (tid < m) {
        const int32_t idx = key_idx(keys[c0 + tid]);
        A.pos[tid] = make_float4(g.ux[idx] - cx, g.uy[idx] - cy, g.uz[idx] - cz, 0.f);
      }
      __syncthreads();
      if (tid < 6) {
        const float* rp = reinterpret_cast<const float*>(A.pos);
        for (int j = 0; j < m; ++j) s = s + (double)rp[4 * j + ia] * (double)rp[4 * j + ib];
      }
      __syncthreads();
    }
    if (tid < 6) A.sums[tid] = s;
    __syncthreads();
    // ---- z: the eigenvector of the smallest eigenvalue, towards the normals' mean ----
    if (tid == 0) {
      double ev[3], V[3][3];
      eigen_selfadjoint3<true>(A.sums[0], A.sums[1], A.sums[3], A.sums[2], A.sums[4], A.sums[5], ev, V);
      float zx = (float)V[0][0], zy = (float)V[0][1], zz = (float)V[0][2];
      float mx = A.acc[3], my = A.acc[4], mz = A.acc[5];
      const float mn = sqrtf((mx * mx + my * my) + mz * mz);
      mx = mx / mn;
      my = my / mn;
      mz = mz / mn;
      if ((zx * mx + zy * my) + zz * mz < 0.f) {
        zx = -zx;
        zy = -zy;
        zz = -zz;
      }
      A.z[0] = zx;
      A.z[1] = zy;
      A.z[2] = zz;
    }
    __syncthreads();
    const float zx = A.z[0], zy = A.z[1], zz = A.z[2];
    // ---- the most inclined normal of [lo, kt): the first strict minimum of z . n ----
    float bc = FLT_MAX;  // (PCL's initial value: a cosine that is not below it, NaN included, never wins)
    int bj = INT_MAX;
    for (int j = lo + tid; j < kt; j += kBoardChunk) {
      const int32_t idx = key_idx(keys[j]);
      const float c = (zx * snx[idx] + zy * sny[idx]) + zz * snz[idx];
      if (c < bc) {  // (a thread's positions ascend: its first strict minimum)
        bc = c;
        bj = j;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float oc = __shfl_xor(bc, o);
      const int oj = __shfl_xor(bj, o);
      if (board_better(bc, bj, oc, oj)) {
        bc = oc;
        bj = oj;
      }
    }
    if ((tid & 63) == 0) {
      A.wcos[tid >> 6] = bc;
      A.wpos[tid >> 6] = bj;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kBoardChunk / 64; ++w)
        if (board_better(bc, bj, A.wcos[w], A.wpos[w])) {
          bc = A.wcos[w];
          bj = A.wpos[w];
        }
      float* o = out + 9 * q;
      if (bj == INT_MAX) {
#pragma unroll
        for (int e = 0; e < 9; ++e) o[e] = nan;
      } else {
        // directedOrthogonalAxis: the chosen neighbour projected onto the plane through p across z
        const int32_t idx = key_idx(keys[bj]);
        const float bx = g.ux[idx], by = g.uy[idx], bz = g.uz[idx];
        const float ox = bx - px, oy = by - py, oz = bz - pz;
        const float t = (zx * ox + zy * oy) + zz * oz;
        const float jx = bx - t * zx, jy = by - t * zy, jz = bz - t * zz;
        float xx = jx - px, xy = jy - py, xz = jz - pz;
        const float xn = sqrtf((xx * xx + xy * xy) + xz * xz);
        xx = xx / xn;
        xy = xy / xn;
        xz = xz / xn;
        o[0] = canon_nan(xx);
        o[1] = canon_nan(xy);
        o[2] = canon_nan(xz);
        o[3] = canon_nan(zy * xz - zz * xy);
        o[4] = canon_nan(zz * xx - zx * xz);
        o[5] = canon_nan(zx * xy - zy * xx);
        o[6] = canon_nan(zx);
        o[7] = canon_nan(zy);
        o[8] = canon_nan(zz);
      }
    }
    __syncthreads();  // the keys and A are read before the next query's gather overwrites them
  }
}

}  // namespace

int board_cap_small() { return kTwoPassCapSmall; }

void board_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
               const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, int64_t nq, double r,
               const pfx_board_params& prm, float* rf) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, kRepBoard);
  if (ns == 0) {  // every k is 0
    fill_nan(ctx, rf, 9 * nq);
  } else {
    // PCL searches again at double(tangent_radius) when it is set and differs from the radius
    const double rt = (double)prm.tangent_radius;
    const bool second = prm.tangent_radius != 0.0f && r != rt;
    const double rg = second && rt > r ? rt : r;
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, rg);
    const float rr_s = (float)(r * r), rr_t = second ? (float)(rt * rt) : rr_s;
    const float radius2 = prm.tangent_radius * prm.tangent_radius;
    const float margin2 = (prm.margin_thresh * prm.margin_thresh) * radius2;
    TimeScope ts(ctx, "board_lrf", true);
    two_pass(ctx, ns, nq, "board_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_board<cap()>, blocks, lds, st, g, snx, sny, snz, qx, qy, qz, nq, (float)(rg * rg),
                               rr_s, rr_t, margin2, list, n_list, over, rf, err);
             });
    check_launch("k_board");
  }
  report_post(ctx, kRepBoard, err);
}

void board_report(pfx_ctx* ctx, const int* h) { two_pass_report(ctx, h, "board", "board_lrf"); }

}  // namespace pfx
