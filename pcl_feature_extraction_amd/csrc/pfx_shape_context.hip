// pfx_shape_context.hip -- ShapeContext3DEstimation<PointXYZRGB,Normal,ShapeContext1980>
// (evaluation.cpp:319-345), UniqueShapeContext<PointXYZRGB,ShapeContext1980> (:346-371) and the
// frames-only SHOTLocalReferenceFrameEstimation on gfx950.  DESIGN.md "Shape contexts",
// "Shape contexts: the contract".
//
//   k_sc_mark       one workgroup per query: the surface points of its ball (the support, by cell
//                   position) and whether the ball holds any point (a 3DSC row then draws);
//   k_sc_density    one wave per support point: the number of surface points in its rho-ball, a
//                   box scan of the grid's cells that the ball can reach (integer, order-free);
//   k_shape_context one 256-thread workgroup per query:
//     1. radius neighbours in FLANN order, the keys in LDS (pfx_two_pass.h: the two passes);
//     2. the frame: the caller's (USC), or the nearest neighbour's normal with the row's three
//        floats of the random stream, orthogonalised (3DSC; the row's place in the stream is the
//        number of earlier drawing rows, an exclusive scan of k_sc_mark's flags);
//     3. per chunk of kScChunk neighbours every thread turns its neighbour into a record
//        (bin, w) and sets its bit in the chunk mask of the bin's owner, thread bin % 256 (64-bit
//        integer atomics in LDS, order-free); a neighbour closer than the skip sets no bit;
//     4. every owner takes its set bits in ascending order and adds the records to its bins of
//        the 1,980 LDS accumulators: a bin's additions are one thread's, in FLANN neighbour
//        order.  No floating-point atomic.
//   k_sc_lrf        one workgroup per query: sorted neighbours, then pfx_shot_core.h's shot_lrf,
//                   shot_eigen and shot_frame, the frame alone.
// Stream-ordered: errors and statistics go through the deferred reports (sc_report, lrf_report).
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <random>

#include "pfx_shot_core.h"
#include "pfx_two_pass.h"

namespace pfx {
namespace {

constexpr int kScChunk = kTwoPassChunk;
constexpr int kScWords = kScChunk / 64;
constexpr int kScAz = 12, kScEl = 11, kScRad = 15;  // PCL 1.7's fixed bins
constexpr int kScLen = kScAz * kScEl * kScRad;     // 1980

// The shape contexts' own words (per call): the drawing rows, the neighbours skipped as too close,
// the support points.  The frames have none, and no statistics.
constexpr int kWordDraws = kWordOwn, kWordSkipped = kWordOwn + 1, kWordSupport = kWordOwn + 2;
static_assert(kCapSmall == kTwoPassCapSmall && kCap == kTwoPassCap, "k_sc_lrf: SHOT's capacities are the frame's");

// built on the host (the C library's cosf, powf, exp and log: the restatement's), read from LDS
struct ScTables {
  float radii[kScRad + 1];
  float theta_div[kScEl + 1];
  float phi_div[kScAz + 1];
  float lut[kScEl * kScRad];  // 1 / cbrt(bin volume): the same for every azimuth
};
constexpr int kTableWords = sizeof(ScTables) / sizeof(float);

inline float deg2rad_h(float a) { return a * 0.017453293f; }

void sc_tables(double R, double rmin, ScTables& T) {
  for (int j = 0; j <= kScRad; ++j)
    T.radii[j] = (float)std::exp(std::log(rmin) + (double)((float)j / 15.0f) * std::log(R / rmin));
  for (int k = 0; k <= kScEl; ++k) T.theta_div[k] = (float)k * (180.0f / 11.0f);
  for (int l = 0; l <= kScAz; ++l) T.phi_div[l] = (float)l * 30.0f;
  const float integr_phi = deg2rad_h(T.phi_div[1]) - deg2rad_h(T.phi_div[0]);
  for (int k = 0; k < kScEl; ++k) {
    const float integr_theta = cosf(deg2rad_h(T.theta_div[k])) - cosf(deg2rad_h(T.theta_div[k + 1]));
    for (int j = 0; j < kScRad; ++j) {
      const float a = T.radii[j + 1], b = T.radii[j];
      const float integr_r = a * a * a - b * b * b;
      const float V = integr_phi * integr_theta * integr_r;
      T.lut[k * kScRad + j] = 1.0f / powf(V, 1.0f / 3.0f);
    }
  }
}

__global__ void k_sc_tables(ScTables T, float* __restrict__ out) {
  const float* src = reinterpret_cast<const float*>(&T);
  for (int i = threadIdx.x; i < kTableWords; i += blockDim.x) out[i] = src[i];
}

__device__ __forceinline__ bool sc_equal(float a, float b) { return fabsf(a - b) < FLT_EPSILON; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// a row without a neighbour loop: every bin `v`, rf = `frame` (nullable: nine zeros)
__device__ __forceinline__ void sc_fill(float* __restrict__ d, float* __restrict__ rfo, float v,
                                        const float* __restrict__ frame) {
  for (int i = threadIdx.x; i < kScLen; i += kScChunk) d[i] = v;
  if (threadIdx.x < 9) rfo[threadIdx.x] = frame ? canon_nan(frame[threadIdx.x]) : 0.0f;
}

// the support (flags by cell position) and, where asked, whether each row draws
__global__ void __launch_bounds__(256) k_sc_mark(GridView g, const float* __restrict__ qx,
                                                 const float* __restrict__ qy, const float* __restrict__ qz,
                                                 int64_t nq, float rr, uint8_t* __restrict__ flags,
                                                 int32_t* __restrict__ draws, int* __restrict__ err) {
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    Runs R;
    const float x = qx[q], y = qy[q], z = qz[q];
    query_runs(g, x, y, z, R);  // (no candidate for a non-finite query)
    int any = 0;
    for (int32_t t = threadIdx.x; t < R.pref[9]; t += blockDim.x) {
      const int32_t p = run_pos(R, t);
      const float4 c = g.sp[p];
      if (flann_d2(x, y, z, c.x, c.y, c.z) < rr) {
        flags[p] = 1;
        any = 1;
      }
    }
    if (draws) {
      any = __syncthreads_or(any);
      if (threadIdx.x == 0) {
        draws[q] = any;
        if (any) atomicAdd(err + kWordDraws, 1);
      }
    }
  }
}

__device__ __forceinline__ int32_t cell_clamp(double v, int32_t n) {
  const int64_t c = (int64_t)floor(v);
  return (int32_t)(c < 0 ? 0 : (c > n - 1 ? n - 1 : c));
}

// flags: the support by cell position.  reach: rho with a margin far above the float rounding of
// d2.  A point with d2 < rho2 differs by less than reach in every coordinate, and the cell of a
// coordinate is monotone in it, so the box of cells between the cells of p - reach and p + reach
// holds the ball: at most 2 x 2 x 2 of the descriptor grid's cells while 2 rho <= R, against the 27
// of a neighbour search (a second grid with cells of rho was slower, its build included: DESIGN.md).
__global__ void __launch_bounds__(256) k_sc_density(GridView gs, const uint8_t* __restrict__ flags,
                                                    float rho2, double reach, int* __restrict__ dens,
                                                    int* __restrict__ err) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t nfin = grid_nfinite(gs);
  int nsup = 0;
  for (int64_t base = ((int64_t)blockIdx.x * 4 + wv) * 64; base < nfin; base += (int64_t)gridDim.x * 256) {
    const int64_t s = base + lane;
    uint64_t m = __ballot(s < nfin && flags[s] != 0);
    nsup += __popcll(m);
    while (m) {
      const int b = __builtin_ctzll(m);
      m &= m - 1;
      const float4 p = gs.sp[base + b];
      const int32_t x0 = cell_clamp(((double)p.x - reach - gs.ox) * gs.inv, gs.nx);
      const int32_t x1 = cell_clamp(((double)p.x + reach - gs.ox) * gs.inv, gs.nx);
      const int32_t y0 = cell_clamp(((double)p.y - reach - gs.oy) * gs.inv, gs.ny);
      const int32_t y1 = cell_clamp(((double)p.y + reach - gs.oy) * gs.inv, gs.ny);
      const int32_t z0 = cell_clamp(((double)p.z - reach - gs.oz) * gs.inv, gs.nz);
      const int32_t z1 = cell_clamp(((double)p.z + reach - gs.oz) * gs.inv, gs.nz);
      int c = 0;
      for (int32_t ix = x0; ix <= x1; ++ix)
        for (int32_t iy = y0; iy <= y1; ++iy) {
          const int64_t row = ((int64_t)ix * gs.ny + iy) * gs.nz;
          const int32_t a = gs.cell_start[row + z0], e = gs.cell_start[row + z1 + 1];
          // four candidates per lane in flight (branch-free: clamped positions, a <= tt < e)
          constexpr int U = 4;
          for (int32_t t = a + lane; t < e; t += U * 64) {
            float4 c4[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int32_t tt = t + 64 * u;
              c4[u] = gs.sp[tt < e ? tt : t];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
              c += (t + 64 * u < e && flann_d2(p.x, p.y, p.z, c4[u].x, c4[u].y, c4[u].z) < rho2) ? 1 : 0;
          }
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
      if (lane == 0) dens[gs.perm[base + b]] = c;
    }
  }
  if (lane == 0 && nsup) atomicAdd(err + kWordSupport, nsup);
}

// The 16 KiB behind the keys: the bucketed sort's scratch, then (the sort done) the chunk's records
// and the owners' masks.
struct ScAux {
  unsigned long long mask[kScWords][kScChunk];  // [word][owner]: the owners' reads are lane-consecutive
  int bin[kScChunk];
  float w[kScChunk];
};
static_assert(sizeof(ScAux) <= kTwoPassAuxBytes, "the records fit the sort scratch");

// list (nullable): the queued queries with their device-side count; over (nullable): where a query
// with more than CAP neighbours is queued (else it is beyond every capacity: err[0]).
// USC: frames (nq x 9) are the caller's; else snx / sny / snz, rnd and rank make the frame.
template <int CAP, bool USC>
__global__ void __launch_bounds__(kScChunk) k_shape_context(
    GridView g, const float* __restrict__ snx, const float* __restrict__ sny, const float* __restrict__ snz,
    const float* __restrict__ qx, const float* __restrict__ qy, const float* __restrict__ qz,
    const float* __restrict__ frames, const float* __restrict__ rnd, const int32_t* __restrict__ rank,
    const int* __restrict__ dens, int64_t nq, const int32_t* __restrict__ list, const int* __restrict__ n_list,
    int32_t* __restrict__ over, const float* __restrict__ tables, float rr, float* __restrict__ desc,
    float* __restrict__ rf_out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP, then the 16 KiB of ScAux
  ScAux& A = *reinterpret_cast<ScAux*>(keys + CAP);
  __shared__ BucketLds SB;
  __shared__ int s_count;
  __shared__ ScTables T;
  __shared__ float acc[kScLen];
  __shared__ float s_rf[9];
  __shared__ int s_skip;
  const int tid = threadIdx.x;
  for (int i = tid; i < kTableWords; i += kScChunk) reinterpret_cast<float*>(&T)[i] = tables[i];
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t wi = blockIdx.x; wi < count; wi += gridDim.x) {
    const int64_t q = list ? (int64_t)list[wi] : wi;
    float* d = desc + q * kScLen;
    float* rfo = rf_out + q * 9;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    const float* frame = USC ? frames + q * 9 : nullptr;
    bool dead = !finite3(cx, cy, cz);
    if (USC) dead = dead || !finite3(frame[0], frame[3], frame[6]);
    if (dead) {
      sc_fill(d, rfo, __uint_as_float(0x7fc00000u), nullptr);
      continue;
    }
    const int k = two_pass_neighbors<CAP>(g, cx, cy, cz, rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err(k, q, over, err);
      continue;
    }
    if (tid == 0) count_neighbors(k, err);
    if (k == 0) {  // 3DSC: NaN, no frame, no draw; USC: an empty histogram in the caller's frame
      sc_fill(d, rfo, USC ? 0.0f : __uint_as_float(0x7fc00000u), frame);
      continue;
    }
    if (tid == 0) {
      s_skip = 0;
      if (USC) {
        for (int i = 0; i < 9; ++i) s_rf[i] = frame[i];
      } else {
        // the nearest neighbour's normal (the first key: the lowest index among equal distances)
        const int32_t i0 = key_idx(keys[0]);
        const f3 n = mk3(snx[i0], sny[i0], snz[i0]);
        const int64_t t = rank[q];
        f3 x = mk3(rnd[3 * t], rnd[3 * t + 1], rnd[3 * t + 2]);
        if (!sc_equal(n.z, 0.0f)) x.z = -(n.x * x.x + n.y * x.y) / n.z;
        else if (!sc_equal(n.y, 0.0f)) x.y = -(n.x * x.x + n.z * x.z) / n.y;
        else if (!sc_equal(n.x, 0.0f)) x.x = -(n.y * x.y + n.z * x.z) / n.x;
        x = normalize3(x);
        const f3 y = cross3(n, x);
        s_rf[0] = x.x; s_rf[1] = x.y; s_rf[2] = x.z;
        s_rf[3] = y.x; s_rf[4] = y.y; s_rf[5] = y.z;
        s_rf[6] = n.x; s_rf[7] = n.y; s_rf[8] = n.z;
      }
    }
    for (int i = tid; i < kScLen; i += kScChunk) acc[i] = 0.0f;
#pragma unroll
    for (int w = 0; w < kScWords; ++w) A.mask[w][tid] = 0ull;
    __syncthreads();  // the frame, the cleared bins and masks (the sort is done with its scratch)
    const f3 o = mk3(cx, cy, cz);
    const f3 x = mk3(s_rf[0], s_rf[1], s_rf[2]), n = mk3(s_rf[6], s_rf[7], s_rf[8]);
    for (int c0 = 0; c0 < k; c0 += kScChunk) {
      const int m = min(kScChunk, k - c0);
      if (tid < m) {
        const uint64_t key = keys[c0 + tid];
        const int32_t idx = key_idx(key);
        const float d2 = key_d2(key);
        if (sc_equal(d2, 0.0f)) {
          atomicAdd(&s_skip, 1);
        } else {
          const float r = sqrtf(d2);
          const f3 p = mk3(g.ux[idx], g.uy[idx], g.uz[idx]);
          const f3 po = sub3(p, o);
          const float lambda = dot3(n, po);
          f3 proj = sub3(p, scale3(n, lambda));
          proj = sub3(proj, o);
          proj = normalize3(proj);
          const f3 c = cross3(x, proj);
          float phi = atan2f_glibc(sqrtf(sqn3(c)), dot3(x, proj)) * 57.29578f;
          if (dot3(c, n) < 0.0f) phi = 360.0f - phi;
          const f3 no = normalize3(po);
          float t = dot3(n, no);
          t = -1.0f < t ? t : -1.0f;  // std::max(-1.0f, t): a NaN becomes -1
          t = t < 1.0f ? t : 1.0f;    // std::min(1.0f, .)
          const float theta = acosf_glibc(t) * 57.29578f;
          // the first division that holds the value, 0 when none does (descending: the lowest wins)
          int j = 0, kk = 0, l = 0;
          for (int i = kScRad; i >= 1; --i) j = r <= T.radii[i] ? i - 1 : j;
          for (int i = kScEl; i >= 1; --i) kk = theta <= T.theta_div[i] ? i - 1 : kk;
          for (int i = kScAz; i >= 1; --i) l = phi <= T.phi_div[i] ? i - 1 : l;
          const int bin = l * (kScEl * kScRad) + kk * kScRad + j;
          A.bin[tid] = bin;
          A.w[tid] = (1.0f / (float)dens[idx]) * T.lut[kk * kScRad + j];
          atomicOr(&A.mask[tid >> 6][bin & (kScChunk - 1)], 1ull << (tid & 63));
        }
      }
      __syncthreads();
      for (int wd = 0; wd * 64 < m; ++wd) {
        unsigned long long hit = A.mask[wd][tid];
        if (hit) {
          A.mask[wd][tid] = 0ull;  // ready for the next chunk
          while (hit) {            // ascending: a bin's additions stay in neighbour order
            const int jn = wd * 64 + __builtin_ctzll(hit);
            hit &= hit - 1;
            const int b = A.bin[jn];
            acc[b] = acc[b] + A.w[jn];
          }
        }
      }
      __syncthreads();  // the records are read before the next chunk's overwrite them
    }
    for (int i = tid; i < kScLen; i += kScChunk) d[i] = acc[i];
    if (tid < 9) rfo[tid] = canon_nan(s_rf[tid]);
    if (tid == 0 && s_skip) atomicAdd(err + kWordSkipped, s_skip);
    __syncthreads();  // acc, s_rf and A are read before the next query overwrites them
  }
}

// no surface: every neighbourhood is empty
template <bool USC>
__global__ void __launch_bounds__(kScChunk) k_sc_empty(const float* __restrict__ qx, const float* __restrict__ qy,
                                                       const float* __restrict__ qz,
                                                       const float* __restrict__ frames, int64_t nq,
                                                       float* __restrict__ desc, float* __restrict__ rf_out) {
  for (int64_t q = blockIdx.x; q < nq; q += gridDim.x) {
    const float* frame = USC ? frames + q * 9 : nullptr;
    const bool live = USC && finite3(qx[q], qy[q], qz[q]) && finite3(frame[0], frame[3], frame[6]);
    sc_fill(desc + q * kScLen, rf_out + q * 9, live ? 0.0f : __uint_as_float(0x7fc00000u), live ? frame : nullptr);
  }
}

// SHOTLocalReferenceFrameEstimation alone: pfx_shot's frames, bit for bit
template <int CAP>
__global__ void __launch_bounds__(256) k_sc_lrf(GridView g, const float* __restrict__ qx,
                                                const float* __restrict__ qy, const float* __restrict__ qz,
                                                int64_t nq, const int32_t* __restrict__ list,
                                                const int* __restrict__ n_list, int32_t* __restrict__ over,
                                                double radius, float* __restrict__ rf_out, int* __restrict__ err) {
  extern __shared__ __attribute__((aligned(16))) uint64_t keys[];  // CAP (+ CAP sort scratch, first pass)
  __shared__ ShotLds S;
  __shared__ BucketLds SB;
  __shared__ int s_count;
  const int tid = threadIdx.x;
  const float rr = (float)(radius * radius);
  const int64_t count = list ? (int64_t)*n_list : nq;
  for (int64_t w = blockIdx.x; w < count; w += gridDim.x) {
    const int64_t q = list ? (int64_t)list[w] : w;
    float* rfo = rf_out + q * 9;
    const float cx = qx[q], cy = qy[q], cz = qz[q];
    if (!finite3(cx, cy, cz)) {
      if (tid < 9) rfo[tid] = __builtin_nanf("");
      continue;
    }
    const int k = two_pass_neighbors<CAP>(g, cx, cy, cz, rr, keys, &s_count, SB);
    if (k > CAP) {
      if (tid == 0) over_or_err<false>(k, q, over, err);
      continue;
    }
    const NbKeys src{keys, g.ux, g.uy, g.uz, nullptr, nullptr, nullptr, cx, cy, cz};
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
      if (tid < 9) rfo[tid] = __builtin_nanf("");
      continue;
    }
    shot_frame(S, src, k, valid);
    __syncthreads();
    if (tid < 9) rfo[tid] = S.rf[tid];
    __syncthreads();  // S is rewritten by the next query
  }
}

float next_uniform01(std::mt19937& eng) {
  for (;;) {
    const float v = (float)(uint32_t)eng() * (1.0f / 4294967296.0f);
    if (v < 1.0f) return v;  // (float)u32 rounds to 2^32 for the 128 largest values: drawn again
  }
}

template <bool USC>
void sc_launch(pfx_ctx* ctx, const GridView& g, const float* snx, const float* sny, const float* snz, int64_t ns,
               const float* qx, const float* qy, const float* qz, const float* frames, const float* rnd,
               const int32_t* rank, const int* dens, int64_t nq, const float* tables, float rr, float* desc,
               float* rf, int* err) {
  two_pass(ctx, ns, nq, "sc_over", err,
           [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
             two_pass_launch(k_shape_context<cap(), USC>, blocks, lds, ctx->stream, g, snx, sny, snz, qx, qy, qz,
                             frames, rnd, rank, dens, nq, list, n_list, over, tables, rr, desc, rf, err);
           });
  check_launch("k_shape_context");
}

}  // namespace

int sc_cap_small() { return kTwoPassCapSmall; }

void rng_uniform01(uint32_t seed, int64_t skip, int64_t n, float* out) {
  std::mt19937 eng(seed);  // init_genrand(seed)
  for (int64_t i = 0; i < skip; ++i) (void)next_uniform01(eng);
  for (int64_t i = 0; i < n; ++i) out[i] = next_uniform01(eng);
}

// frames == nullptr: 3DSC (snx / sny / snz; rnd nullable: the stream of seed 12345 from its start);
// else USC (the normals and rnd are not read)
void sc_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, const float* snx, const float* sny,
            const float* snz, int64_t ns, const float* qx, const float* qy, const float* qz, const float* frames,
            int64_t nq, double R, double rmin, double rho, const float* rnd, float* desc, float* rf) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  const bool usc = frames != nullptr;
  int* err = report_words(ctx, kRepSc);
  if (ns == 0) {
    const unsigned bl = (unsigned)std::min<int64_t>(nq, 1 << 16);
    if (usc) k_sc_empty<true><<<bl, kScChunk, 0, st>>>(qx, qy, qz, frames, nq, desc, rf);
    else k_sc_empty<false><<<bl, kScChunk, 0, st>>>(qx, qy, qz, frames, nq, desc, rf);
    check_launch("k_sc_empty");
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, R);
    const float rr = (float)(R * R);
    // the support, and the rows that draw with their places in the stream
    uint8_t* flags = ctx->buf("sc_flags").as<uint8_t>((size_t)ns);
    int32_t* draws = usc ? nullptr : ctx->buf("sc_draws").as<int32_t>((size_t)nq);
    int32_t* rank = usc ? nullptr : ctx->buf("sc_rank").as<int32_t>((size_t)nq);
    int* dens = ctx->buf("sc_dens").as<int>((size_t)ns);
    float* tables = ctx->buf("sc_tables").as<float>(kTableWords);
    if (!usc && !rnd) {
      // the default stream's first floats stay on the device; longer query lists extend them
      DevBuf& rb = ctx->buf("sc_rnd");
      if (!rb.ptr || ctx->sc_rnd_n < 3 * nq) {
        std::vector<float> h((size_t)(3 * nq));
        rng_uniform01(12345u, 0, 3 * nq, h.data());
        float* dr = rb.as<float>((size_t)(3 * nq));
        PFX_HIP(hipMemcpyAsync(dr, h.data(), sizeof(float) * h.size(), hipMemcpyHostToDevice, st));
        PFX_HIP(hipStreamSynchronize(st));  // (h leaves scope; once per context and size)
        ctx->sc_rnd_n = 3 * nq;
      }
      rnd = static_cast<const float*>(rb.ptr);
    }
    {
      TimeScope ts(ctx, "sc_density", true);
      PFX_HIP(hipMemsetAsync(flags, 0, (size_t)ns, st));
      k_sc_mark<<<(unsigned)std::min<int64_t>(nq, 8192), 256, 0, st>>>(g, qx, qy, qz, nq, rr, flags, draws, err);
      check_launch("k_sc_mark");
      if (!usc) {
        size_t tb = 0;
        PFX_HIP(rocprim::exclusive_scan(nullptr, tb, draws, rank, 0, (size_t)nq, rocprim::plus<int32_t>(), st));
        void* tmp = ctx->buf("sc_scan_tmp").get(tb + 16);
        PFX_HIP(rocprim::exclusive_scan(tmp, tb, draws, rank, 0, (size_t)nq, rocprim::plus<int32_t>(), st));
      }
      const float rho2 = (float)(rho * rho);
      const double reach = rho * (1.0 + 1e-5);
      const unsigned bl = (unsigned)std::min<int64_t>(ceil_div(ns, 256), 256 * 16);
      k_sc_density<<<bl, 256, 0, st>>>(g, flags, rho2, reach, dens, err);
      check_launch("k_sc_density");
    }
    ScTables T;
    sc_tables(R, rmin, T);
    k_sc_tables<<<1, 256, 0, st>>>(T, tables);
    check_launch("k_sc_tables");
    TimeScope ts(ctx, "shape_context", true);
    if (usc) sc_launch<true>(ctx, g, snx, sny, snz, ns, qx, qy, qz, frames, rnd, rank, dens, nq, tables, rr, desc, rf, err);
    else sc_launch<false>(ctx, g, snx, sny, snz, ns, qx, qy, qz, frames, rnd, rank, dens, nq, tables, rr, desc, rf, err);
  }
  report_post(ctx, kRepSc, err);
}

void shot_lrf_dev(pfx_ctx* ctx, const float* sx, const float* sy, const float* sz, int64_t ns, const float* qx,
                  const float* qy, const float* qz, int64_t nq, double r, float* rf) {
  if (nq == 0) return;
  hipStream_t st = ctx->stream;
  int* err = report_words(ctx, kRepLrf);
  if (ns == 0) {
    fill_nan(ctx, rf, nq * 9);
  } else {
    const GridView g = feature_grid(ctx, sx, sy, sz, ns, r);
    TimeScope ts(ctx, "shot_lrf", true);
    // (no records behind the keys: the first pass holds its keys and their sort scratch, the second its keys)
    two_pass(ctx, ns, nq, "sc_lrf_over", err,
             [&](auto cap, unsigned blocks, size_t lds, const int32_t* list, const int* n_list, int32_t* over) {
               two_pass_launch(k_sc_lrf<cap()>, blocks, lds, st, g, qx, qy, qz, nq, list, n_list, over, r, rf, err);
             },
             2 * sizeof(uint64_t) * kTwoPassCapSmall, sizeof(uint64_t) * kTwoPassCap);
    check_launch("k_sc_lrf");
  }
  report_post(ctx, kRepLrf, err);
}

void sc_report(pfx_ctx* ctx, const int* h) {
  ctx->stats["sc_draws"] = h[kWordDraws];
  ctx->stats["sc_skipped_close"] = h[kWordSkipped];
  ctx->stats["sc_support"] = h[kWordSupport];
  two_pass_report(ctx, h, "sc", "shape_context");
}

void lrf_report(pfx_ctx*, const int* h) {
  if (h[kWordOver] > 0)
    throw Error(PFX_ERR_CAPACITY, "shot_lrf: a query has " + std::to_string(h[kWordOver]) + " neighbours (> " +
                                      std::to_string(kTwoPassCap) + " supported)");
}

}  // namespace pfx
