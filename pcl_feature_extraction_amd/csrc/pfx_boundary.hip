// pfx_boundary.hip -- BoundaryEstimation<PointXYZRGB, Normal, Boundary> (evaluation.cpp:394-415) on
// gfx950.  DESIGN.md "Boundary points" and "Boundary: the contract".
//
// The result depends on the neighbour *set* alone, so nothing is sorted and no key list is kept: no
// capacity, no second pass, any k.  One kernel, k_boundary: one wave per query, four queries per
// 256-thread workgroup, no __syncthreads anywhere.  A wave
//   walks the query's nine candidate runs (pfx_neighbors.h), 4 x 64 candidates in flight;
//   compacts the (du, dv) of the candidates inside the radius into a wave-private LDS ring, so that
//   atan2f_glibc runs on full waves (about one candidate in six passes the radius test);
//   bins every angle into 256 wave-private bins that keep their smallest and largest angle as
//   order-preserving integers (LDS atomicMin / atomicMax: integer, so the order of arrival is
//   immaterial and the result deterministic; no floating-point atomic);
//   then every lane owns four consecutive bins, a ballot and a shuffle hand it the largest angle of
//   the previous non-empty lane, and a ballot ORs the lanes' verdicts.
// The gaps between the largest angle of one non-empty bin and the smallest of the next, and the wrap
// term, are the differences PCL forms on its sorted array that can exceed a threshold of two bin
// widths (DESIGN.md has the rounding argument); a smaller threshold is refused at the C-ABI.
// Statistics only through the deferred reports (boundary_report): nothing can go wrong late.
#include <climits>

#include "pfx_two_pass.h"
#include "pfx_wave_sort.h"

namespace pfx {
namespace {

constexpr int kBoundaryBins = 256;
constexpr int kBoundaryWaves = 4;                      // queries per workgroup
constexpr int kBoundaryRing = 128;                     // < 64 waiting + <= 64 pushed
constexpr int kWordFlagged = kWordOwn;                 // rows flagged 1
constexpr float kPiF = 3.14159274101257324f;           // (float)M_PI
constexpr float kBinsPerRad = (float)(128.0 / 3.14159265358979323846);

struct BoundaryWave {
  int mn[kBoundaryBins];  // the bins' smallest angle, INT_MAX when empty
  int mx[kBoundaryBins];  // ... and largest, INT_MIN when empty
  float2 ring[kBoundaryRing];
};

// float <-> an int that orders as the float does (-0 below +0); its own inverse
__device__ __forceinline__ int angle_key(float a) {
  const int b = __float_as_int(a);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float key_angle(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// one angle of every active lane into the bins; returns whether it is a NaN
__device__ __forceinline__ bool bin_angle(BoundaryWave& W, float2 d) {
  const float a = atan2f_glibc(d.y, d.x);
  const int b = min(kBoundaryBins - 1, (int)((a + kPiF) * kBinsPerRad));
  const int key = angle_key(a);
  atomicMin(&W.mn[b], key);
  atomicMax(&W.mx[b], key);
  return a != a;
}

__global__ void __launch_bounds__(64 * kBoundaryWaves)
k_boundary(GridView g, const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
           const float* __restrict__ qnx, const float* __restrict__ qny, const float* __restrict__ qnz, int64_t nq,
           float rr, float thr, uint8_t* __restrict__ out, int* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) BoundaryWave S[kBoundaryWaves];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  BoundaryWave& W = S[wave];
  unsigned long long s_nb = 0;  // this wave's statistics
  int s_kmax = 0, s_flagged = 0;
  for (int64_t q = (int64_t)blockIdx.x * kBoundaryWaves + wave; q < nq; q += (int64_t)gridDim.x * kBoundaryWaves) {
    const float px = qx[q], py = qy[q], pz = qz[q];
    // ---- the plane's axes: Eigen's unitOrthogonal of (n, 0), then u = n x v ----
    const float n0 = qnx[q], n1 = qny[q], n2 = qnz[q];
    int m = 0;  // the first largest |n_i|
    float am = fabsf(n0);
    if (fabsf(n1) > am) {
      m = 1;
      am = fabsf(n1);
    }
    if (fabsf(n2) > am) m = 2;
    // s = (m == 0) ? 1 : 0
    const float n_s = m == 0 ? n1 : n0, n_m = m == 0 ? n0 : m == 1 ? n1 : n2;
    const float len = sqrtf(n_s * n_s + n_m * n_m), inv = 1.0f / len;
    const float vm = -n_s * inv, vs = n_m * inv;
    const float v0 = m == 0 ? vm : vs, v1 = m == 1 ? vm : m == 0 ? vs : 0.f, v2 = m == 2 ? vm : 0.f;
    const float u0 = n1 * v2 - n2 * v1, u1 = n2 * v0 - n0 * v2, u2 = n0 * v1 - n1 * v0;
    const bool axes = isfinite(u0) && isfinite(u1) && isfinite(u2) && isfinite(v0) && isfinite(v1) && isfinite(v2);
    // ---- the bins, empty ----
    reinterpret_cast<int4*>(W.mn)[lane] = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
    reinterpret_cast<int4*>(W.mx)[lane] = make_int4(INT_MIN, INT_MIN, INT_MIN, INT_MIN);
    wave_lds_sync();
    // ---- the candidates ----
    Runs R;
    query_runs(g, px, py, pz, R);  // (a non-finite query has no candidate run: k = 0)
    const int32_t T = R.pref[9];
    int k = 0, waiting = 0;
    bool nan_angle = false;
    constexpr int U = 4;
    for (int32_t t0 = 0; t0 < T; t0 += U * 64) {
      int32_t p[U];
      float4 c[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t t = t0 + u * 64 + lane;
        p[u] = t < T ? run_pos(R, t) : -1;
        c[u] = g.sp[p[u] < 0 ? 0 : p[u]];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool in = p[u] >= 0 && flann_d2(px, py, pz, c[u].x, c[u].y, c[u].z) < rr;
        k += __popcll(__ballot(in));
        const float d0 = c[u].x - px, d1 = c[u].y - py, d2 = c[u].z - pz;
        const bool push = in && axes && !(d0 == 0.f && d1 == 0.f && d2 == 0.f);
        const uint64_t pm = __ballot(push);
        if (push)
          W.ring[waiting + __popcll(pm & lanemask_lt())] =
              make_float2((u0 * d0 + u1 * d1) + u2 * d2, (v0 * d0 + v1 * d1) + v2 * d2);
        waiting += __popcll(pm);
        if (waiting >= 64) {  // (wave-uniform) a full wave of angles, off the top of the ring
          wave_lds_sync();
          waiting -= 64;
          nan_angle |= bin_angle(W, W.ring[waiting + lane]);
          wave_lds_sync();  // read before the next push overwrites it
        }
      }
    }
    wave_lds_sync();
    if (lane < waiting) nan_angle |= bin_angle(W, W.ring[lane]);
    wave_lds_sync();
    // ---- the gap test: lane l owns bins 4 l .. 4 l + 3 ----
    const int4 bmn = reinterpret_cast<const int4*>(W.mn)[lane], bmx = reinterpret_cast<const int4*>(W.mx)[lane];
    const int lmn[4] = {bmn.x, bmn.y, bmn.z, bmn.w}, lmx[4] = {bmx.x, bmx.y, bmx.z, bmx.w};
    // (the bins ascend with the angle: a lane's smallest angle is its first non-empty bin's)
    const int lo = min(min(lmn[0], lmn[1]), min(lmn[2], lmn[3])), hi = max(max(lmx[0], lmx[1]), max(lmx[2], lmx[3]));
    const uint64_t full = __ballot(lo != INT_MAX);  // the lanes with an angle
    const uint64_t below = full & lanemask_lt();
    const int prev_lane = below ? 63 - __builtin_clzll(below) : lane;
    int prev = __shfl(hi, prev_lane);
    bool have = below != 0, gap = false;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lmn[j] != INT_MAX) {
        if (have && key_angle(lmn[j]) - key_angle(prev) > thr) gap = true;
        prev = lmx[j];
        have = true;
      }
    uint8_t verdict = 0;
    if (k == 0) {
      verdict = 255;  // PFX_BOUNDARY_NO_NEIGHBORS
    } else if (k >= 3 && full != 0 && !__ballot(nan_angle)) {
      const float a_min = key_angle(__shfl(lo, __builtin_ctzll(full)));
      const float a_max = key_angle(__shfl(hi, 63 - __builtin_clzll(full)));
      const bool wrap = (2.0f * kPiF - a_max) + a_min > thr;
      verdict = (__ballot(gap) != 0 || wrap) ? 1 : 0;
    }
    if (lane == 0) out[q] = verdict;
    s_nb += (unsigned long long)k;
    s_kmax = max(s_kmax, k);
    s_flagged += verdict == 1;
    wave_lds_sync();  // the bins are read before the next query empties them
  }
  if (lane == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(err + kWordNeighbors), s_nb);
    atomicMax(err + kWordKmax, s_kmax);
    atomicAdd(err + kWordFlagged, s_flagged);
  }
}

}  // namespace

void boundary_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, const float* qx,
                  const float* qy, const float* qz, const float* qnx, const float* qny, const float* qnz, int64_t nq,
                  double r, float angle_threshold, uint8_t* out) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, kRepBoundary);
  if (ns == 0) {  // every k is 0
    k_fill<<<(unsigned)ceil_div(nq, 256), 256, 0, st>>>(out, nq, (uint8_t)PFX_BOUNDARY_NO_NEIGHBORS);
    check_launch("k_fill");
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    TimeScope ts(ctx, "boundary", true);
    // every wave slot of the device once (eight workgroups of four waves a CU), the rest by stride
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div(nq, kBoundaryWaves), 2048);
    k_boundary<<<blocks, 64 * kBoundaryWaves, 0, st>>>(g, qx, qy, qz, qnx, qny, qnz, nq, (float)(r * r),
                                                       angle_threshold, out, err);
    check_launch("k_boundary");
  }
  report_post(ctx, kRepBoundary, err);
}

void boundary_report(pfx_ctx* ctx, const int* h) {
  two_pass_report(ctx, h, "boundary", "boundary", false);  // (kWordOver is never set: no capacity)
  ctx->stats["boundary_flagged"] = h[kWordFlagged];
}

}  // namespace pfx
