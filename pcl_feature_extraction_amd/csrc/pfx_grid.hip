// pfx_grid.hip -- uniform-grid spatial index (replaces the FLANN kd-tree that
// search::KdTree<PointXYZRGB> builds at features.h:192 / tools.h:29).
//
// Layout in HBM (all SoA, 4-byte elements):
//   sx/sy/sz[n]     point coordinates sorted by linear cell key  (coalesced run reads)
//   perm[n]         sorted position -> caller point index         (FLANN tie-break key)
//   cell_start[C+2] first sorted position of each cell (cells in key order), C = nx*ny*nz <= 2^26
// Cells are >= r (r*(1+1e-6)), so the radius ball of a query lies in its 3x3x3 cell block;
// with row-major keys (x, y, z) the block is 9 contiguous runs of 3 z-cells.
// Non-finite points get key C and sort behind every cell (never a neighbour, as PCL's
// kd-tree skips them).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "pfx_internal.h"

namespace pfx {
namespace {

__device__ __forceinline__ uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ord2f(uint32_t u) {
  uint32_t b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f;
  memcpy(&f, &b, 4);
  return f;
}

// per-block bounds (ordered-uint encoding: min slots start at 0xffffffff, max at 0), reduced on
// the host -- no device-side initialisation (a pageable H2D copy) before the launch
constexpr int kBboxBlocks = 1024;
__global__ void __launch_bounds__(256) k_bbox(const float* __restrict__ x, const float* __restrict__ y,
                                              const float* __restrict__ z, int64_t n,
                                              uint32_t* __restrict__ mm) {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float p[3] = {x[i], y[i], z[i]};
    if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) continue;
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], p[d]); hi[d] = fmaxf(hi[d], p[d]); }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[d] = fminf(lo[d], __shfl_xor(lo[d], off));
      hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], off));
    }
  }
  __shared__ float s_lo[3][4], s_hi[3][4];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) { s_lo[d][wv] = lo[d]; s_hi[d][wv] = hi[d]; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float l = fminf(fminf(s_lo[d][0], s_lo[d][1]), fminf(s_lo[d][2], s_lo[d][3]));
      const float h = fmaxf(fmaxf(s_hi[d][0], s_hi[d][1]), fmaxf(s_hi[d][2], s_hi[d][3]));
      const bool any = l <= h;
      mm[blockIdx.x * 6 + d] = any ? f2ord(l) : 0xffffffffu;
      mm[blockIdx.x * 6 + 3 + d] = any ? f2ord(h) : 0u;
    }
  }
}

// the per-block bounds reduced to one (min x, y, z, max x, y, z) record at mm[6 * nblocks]
__global__ void __launch_bounds__(256) k_bbox_reduce(uint32_t* __restrict__ mm, int nblocks) {
  __shared__ uint32_t s[6][256];
  const int t = threadIdx.x;
  uint32_t r[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  for (int b = t; b < nblocks; b += 256)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      r[d] = min(r[d], mm[b * 6 + d]);
      r[3 + d] = max(r[3 + d], mm[b * 6 + 3 + d]);
    }
#pragma unroll
  for (int d = 0; d < 6; ++d) s[d][t] = r[d];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o)
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        s[d][t] = min(s[d][t], s[d][t + o]);
        s[3 + d][t] = max(s[3 + d][t], s[3 + d][t + o]);
      }
    __syncthreads();
  }
  if (t < 6) mm[nblocks * 6 + t] = s[t][0];
}

__device__ __forceinline__ uint64_t lanemask_lt64() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// the mapping point -> cell of both builders
struct CellMap {
  double inv, ox, oy, oz, hx, hy, hz;
  int32_t nx, ny, nz;
};

// linear cell key of a point (C = nx * ny * nz for a non-finite one)
// oob (nullable, speculative bounds): counts the finite points outside [lo, hi] (clamped keys
// are then not a valid grid; the caller rebuilds on exact bounds)
__device__ __forceinline__ uint32_t point_key(const CellMap& m, float px, float py, float pz,
                                              int* __restrict__ oob) {
  uint32_t key = (uint32_t)((int64_t)m.nx * m.ny * m.nz);
  if (isfinite(px) && isfinite(py) && isfinite(pz)) {
    // (exactly the points the clamp below would move: cell index outside [0, dims))
    if (oob && ((double)px < m.ox || (double)py < m.oy || (double)pz < m.oz || (double)px > m.hx ||
                (double)py > m.hy || (double)pz > m.hz))
      atomicAdd(oob, 1);
    int64_t ix = (int64_t)floor(((double)px - m.ox) * m.inv);
    int64_t iy = (int64_t)floor(((double)py - m.oy) * m.inv);
    int64_t iz = (int64_t)floor(((double)pz - m.oz) * m.inv);
    ix = ix < 0 ? 0 : (ix >= m.nx ? m.nx - 1 : ix);
    iy = iy < 0 ? 0 : (iy >= m.ny ? m.ny - 1 : iy);
    iz = iz < 0 ? 0 : (iz >= m.nz ? m.nz - 1 : iz);
    key = (uint32_t)((ix * m.ny + iy) * m.nz + iz);
  }
  return key;
}

__global__ void __launch_bounds__(256) k_cell_keys(const float* __restrict__ x, const float* __restrict__ y,
                                                   const float* __restrict__ z, int64_t n, CellMap m,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                   int* __restrict__ oob) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  keys[i] = point_key(m, x[i], y[i], z[i], oob);
  vals[i] = (uint32_t)i;
}

// ---- the counting-sort builder (speculative builds): the cell key is bounded, so one count per
// cell, one scan and one scatter replace the radix sort, and the order inside a cell (ascending
// caller index, the radix sort's stability) is restored cell by cell afterwards.
// The counts live in cell_start: [0, C) the cells, [C] 0, [C + 1, C + 1 + blocks) the non-finite
// points of each 256-point block of the cloud; one exclusive scan turns them into the cells'
// first positions, the finite count at [C] and each block's first tail position.

constexpr int kCountBlock = 256;
constexpr int64_t kGridCountMaxPoints = int64_t(1) << 18;  // the default builder above this: radix sort
// lanes of a wave with one key share one atomic, for the first keys of the wave (a scan-ordered
// cloud has 1-3 keys per wave; a shuffled one ~64, whose lanes then count on their own)
constexpr int kAggRounds = 4;

__global__ void __launch_bounds__(256) k_count_zero(int32_t* __restrict__ p, int64_t m, int* __restrict__ oob) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *oob = 0;
}

// P1: key and arrival rank of every point.  A finite point's rank is the old value of its cell's
// count (any order: k_count_order restores the index order); a non-finite one's is its rank among
// the non-finite points of its block, in index order (so the tail needs no reordering).
__global__ void __launch_bounds__(kCountBlock) k_count_keys(const float* __restrict__ x, const float* __restrict__ y,
                                                            const float* __restrict__ z, int64_t n, CellMap m,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ rank,
                                                            int32_t* __restrict__ counts, int* __restrict__ oob) {
  const int64_t i = blockIdx.x * (int64_t)kCountBlock + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t C = (uint32_t)((int64_t)m.nx * m.ny * m.nz);
  const bool live = i < n;
  uint32_t key = C;
  if (live) key = point_key(m, x[i], y[i], z[i], oob);
  const bool fin = live && key != C;
  // (every lane stays in the wave-wide steps below)
  uint64_t todo = __ballot(fin);
  int leader = lane, offs = 0, cnt = 1;
  for (int it = 0; it < kAggRounds && todo; ++it) {
    const int l = __builtin_ctzll(todo);
    const uint32_t k = (uint32_t)__shfl((int)key, l);
    const uint64_t same = __ballot(fin && key == k);
    if (fin && key == k) {
      leader = l;
      offs = __popcll(same & lanemask_lt64());
      cnt = __popcll(same);
    }
    todo &= ~same;
  }
  int base = 0;
  if (fin && lane == leader) base = atomicAdd(&counts[key], cnt);
  base = __shfl(base, leader);
  uint32_t r = (uint32_t)(base + offs);
  // non-finite points: ballot prefix inside the block
  __shared__ int s_nf[kCountBlock / 64];
  const bool nf = live && !fin;
  const uint64_t bm = __ballot(nf);
  if (lane == 0) s_nf[wv] = __popcll(bm);
  __syncthreads();
  if (nf) {
    int before = __popcll(bm & lanemask_lt64());
    for (int w = 0; w < wv; ++w) before += s_nf[w];
    r = (uint32_t)before;
  }
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kCountBlock / 64; ++w) total += s_nf[w];
    counts[(int64_t)C + 1 + blockIdx.x] = total;
  }
  if (live) {
    keys[i] = key;
    rank[i] = r;
  }
}

// P3: every point to slot (first position of its cell + arrival rank) of the scratch, packed
// (x, y, z, caller index); the cell key of a slot is already final (one key per cell)
__global__ void __launch_bounds__(kCountBlock) k_count_scatter(const float* __restrict__ x, const float* __restrict__ y,
                                                               const float* __restrict__ z, int64_t n, uint32_t C,
                                                               const uint32_t* __restrict__ keys,
                                                               const uint32_t* __restrict__ rank,
                                                               const int32_t* __restrict__ cell_start,
                                                               float4* __restrict__ scr, uint32_t* __restrict__ skeys) {
  const int64_t i = blockIdx.x * (int64_t)kCountBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t key = keys[i];
  const int64_t at = key < C ? (int64_t)key : (int64_t)C + 1 + blockIdx.x;
  const int64_t slot = (int64_t)cell_start[at] + rank[i];
  scr[slot] = make_float4(x[i], y[i], z[i], __uint_as_float((uint32_t)i));
  skeys[slot] = key;
}

// P4: the point of slot s goes to (first position of its cell + the number of smaller caller
// indices in the cell); a cell above kGridFatCap points is left unordered and reported through
// the validation word (the m^2 reads of a cell stay bounded), the non-finite tail is in order.
// The caller indices of every cell that reaches into the workgroup's 256 slots are staged in LDS
// first (at most a cap's worth on either side: a longer cell is fat and skipped), so the m reads
// per point are LDS broadcasts (the same loop on global loads took 108 us per build in the step).
constexpr int kOrderWin = 256 + 2 * kGridFatCap;
__global__ void __launch_bounds__(256) k_count_order(const float4* __restrict__ scr, const uint32_t* __restrict__ skeys,
                                                     int64_t n, uint32_t C, int32_t* __restrict__ cell_start,
                                                     int32_t* __restrict__ perm, float* __restrict__ sx,
                                                     float* __restrict__ sy, float* __restrict__ sz,
                                                     float4* __restrict__ sp, int* __restrict__ oob) {
  __shared__ uint32_t s_idx[kOrderWin];
  __shared__ int64_t s_win[2];
  const int64_t s0 = blockIdx.x * (int64_t)256, s = s0 + threadIdx.x;
  if (s == 0) cell_start[(int64_t)C + 1] = (int32_t)n;  // (held block 0's tail position until here)
  if (threadIdx.x == 0) {
    const int64_t last = s0 + 255 < n ? s0 + 255 : n - 1;
    const uint32_t k0 = skeys[s0], k1 = skeys[last];
    int64_t w0 = s0, w1 = s0;  // (a workgroup of tail slots stages nothing)
    if (k0 < C) {
      w0 = cell_start[k0];
      w1 = cell_start[(k1 < C ? k1 : C - 1) + 1];
      w0 = w0 > s0 - kGridFatCap ? w0 : s0 - kGridFatCap;
      w1 = w1 < s0 + 256 + kGridFatCap ? w1 : s0 + 256 + kGridFatCap;
    }
    s_win[0] = w0;
    s_win[1] = w1;
  }
  __syncthreads();
  const int64_t w0 = s_win[0], w1 = s_win[1];
  for (int64_t t = w0 + threadIdx.x; t < w1; t += 256) s_idx[t - w0] = __float_as_uint(scr[t].w);
  __syncthreads();
  if (s >= n) return;
  const uint32_t key = skeys[s];
  const float4 v = scr[s];
  const uint32_t idx = __float_as_uint(v.w);
  int64_t d = s;
  if (key < C) {
    const int32_t start = cell_start[key], end = cell_start[key + 1];
    if (end - start > kGridFatCap) {
      if (s == start) atomicOr(oob, kGridFatBit);
      return;
    }
    const uint32_t* cell = s_idx + (start - w0);
    const int m = end - start;
    int before = 0;
    for (int t = 0; t < m; ++t) before += cell[t] < idx ? 1 : 0;
    d = (int64_t)start + before;
  }
  perm[d] = (int32_t)idx;
  sx[d] = v.x;
  sy[d] = v.y;
  sz[d] = v.z;
  sp[d] = make_float4(v.x, v.y, v.z, 0.0f);
}

// cell_start[0, m) = v: a plain kernel launch (hipMemsetD32Async spent ~70 us of host time per
// call in the HIP API trace, on the critical path of the grid build)
__global__ void __launch_bounds__(256) k_fill_i32(int32_t* __restrict__ p, int64_t m, int32_t v) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = v;
}

// first sorted position of every occupied cell (cells are then completed by a suffix minimum)
__global__ void __launch_bounds__(256) k_mark_starts(const uint32_t* __restrict__ skeys, int64_t n,
                                                     int32_t* __restrict__ cell_start) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = skeys[i];
  if (i == 0 || skeys[i - 1] != k) cell_start[k] = (int32_t)i;
}

__global__ void __launch_bounds__(256) k_gather_sorted(const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ z, int64_t n,
                                                       const uint32_t* __restrict__ perm,
                                                       float* __restrict__ sx, float* __restrict__ sy,
                                                       float* __restrict__ sz, float4* __restrict__ sp) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t p = perm[i];
  const float a = x[p], b = y[p], c = z[p];
  sx[i] = a;
  sy[i] = b;
  sz[i] = c;
  sp[i] = make_float4(a, b, c, 0.0f);
}

// exact builds: does any cell hold more than kGridFatCap points?  (flag zeroed by the build)
__global__ void __launch_bounds__(256) k_fat_cells(const int32_t* __restrict__ cell_start, int64_t ncells,
                                                   int* __restrict__ flag) {
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c < ncells && cell_start[c + 1] - cell_start[c] > kGridFatCap) *flag = 1;
}

}  // namespace

// bounds of the finite points: per-block partials read back once (pinned) and reduced here
static bool bbox_dev(pfx_ctx* ctx, DevBuf& scratch, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                     double lo[3], double hi[3]) {
  hipStream_t st = ctx->stream;
  uint32_t* mm = scratch.as<uint32_t>(6 * (kBboxBlocks + 1));
  // ~4 points per thread over up to 1,024 workgroups, reduced on the device (one 24-B readback);
  // 128 workgroups of ~30 points per thread took 28 us alone, 160 us beside NARF's range-image
  // projection (headline A/B: 168.0 vs 168.3 Mpoints/s, within noise)
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n, 1024), 1), kBboxBlocks);
  {
    TimeScope ts(ctx, "grid_bbox");
    k_bbox<<<blocks, 256, 0, st>>>(d_x, d_y, d_z, n, mm);
    k_bbox_reduce<<<1, 256, 0, st>>>(mm, blocks);
    check_launch("k_bbox");
  }
  uint32_t* h = ctx->readback<uint32_t>();  // pinned
  PFX_HIP(hipMemcpyAsync(h, mm + 6 * blocks, sizeof(uint32_t) * 6, hipMemcpyDeviceToHost, st));
  ctx->sync_spin(st);
  uint32_t r[6];
  for (int d = 0; d < 6; ++d) r[d] = h[d];
  const bool any = r[0] != 0xffffffffu && r[3] != 0u;
  for (int d = 0; d < 3; ++d) {
    lo[d] = any ? ord2f(r[d]) : 0.0;
    hi[d] = any ? ord2f(r[3 + d]) : 0.0;
  }
  return any;
}

void points_bbox(pfx_ctx* ctx, Grid& g, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                 double lo[3], double hi[3]) {
  bbox_dev(ctx, g.b_minmax, d_x, d_y, d_z, n, lo, hi);
}

bool points_bbox_any(pfx_ctx* ctx, DevBuf& scratch, const float* d_x, const float* d_y, const float* d_z, int64_t n,
                     double lo[3], double hi[3]) {
  return bbox_dev(ctx, scratch, d_x, d_y, d_z, n, lo, hi);
}

// fork_gather (the normal estimation's opt-in, honoured by hinted radix builds only): the sorted
// coordinates are gathered on the context's side stream while the cell starts are completed here;
// the caller owes ctx->join_side() before anything reads sx / sy / sz / sp (nothing between the
// sort and the list kernels does: the list set-up reads cell_start and skeys).
void build_grid(pfx_ctx* ctx, Grid& g, const float* d_x, const float* d_y, const float* d_z,
                int64_t n, double radius, bool use_hint, bool fork_gather) {
  PFX_CHECK(n >= 0 && n < (int64_t(1) << 31), "point count must be in [0, 2^31)");
  PFX_CHECK(radius > 0.0, "radius must be > 0");
  ctx->join_side(ctx->stream);  // (a gather still forked would write into this build's arrays)
  if (&g == &ctx->grid_b) {  // a grid prepared ahead for the next fpfh_dev no longer holds
    ctx->prep_x = nullptr;
    ctx->prep_n = -1;
    ctx->prep_qx = nullptr;
    ctx->prep_nq = -1;
  }
  hipStream_t st = ctx->stream;
  ++g.gen;
  g.n = n;
  g.ux = d_x; g.uy = d_y; g.uz = d_z;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  g.oob = nullptr;
  g.hint_user |= use_hint;
  if (use_hint && g.have_hint && n > 0) {
    // speculative: the previous exact bounds, widened (no bounds pass, no host round trip)
    for (int d = 0; d < 3; ++d) {
      lo[d] = g.hint_lo[d];
      hi[d] = g.hint_hi[d];
    }
    g.oob = g.b_oob.as<int>(1);
  } else if (n > 0) {
    bbox_dev(ctx, g.b_minmax, d_x, d_y, d_z, n, lo, hi);
    // the hint for the next speculative build: 10 % wider on every side, plus two cells (scans of
    // one sensor keep their extent)
    for (int d = 0; d < 3; ++d) {
      const double m = 0.1 * (hi[d] - lo[d]) + 2.0 * radius;
      g.hint_lo[d] = lo[d] - m;
      g.hint_hi[d] = hi[d] + m;
    }
    g.have_hint = true;
  }
  double cell = radius * (1.0 + 1e-6);
  const double max_cells = double(1 << 26);
  int64_t dims[3];
  for (int it = 0; it < 64; ++it) {
    for (int d = 0; d < 3; ++d) dims[d] = (int64_t)std::floor((hi[d] - lo[d]) / cell) + 1;
    double total = double(dims[0]) * double(dims[1]) * double(dims[2]);
    if (total <= max_cells) break;
    cell *= std::cbrt(total / max_cells) * 1.01;
  }
  g.cell = (float)cell;
  g.inv = (float)(1.0 / cell);
  g.ox = (float)lo[0]; g.oy = (float)lo[1]; g.oz = (float)lo[2];
  g.nx = (int32_t)dims[0]; g.ny = (int32_t)dims[1]; g.nz = (int32_t)dims[2];
  g.ncells = dims[0] * dims[1] * dims[2];
  // exact double parameters used by both builder and queries
  const double inv = 1.0 / cell;
  g.inv = (float)inv;
  const int64_t C = g.ncells;

  const CellMap cm{inv, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], g.nx, g.ny, g.nz};
  g.dinv = inv;
  g.dox = lo[0]; g.doy = lo[1]; g.doz = lo[2];
  g.perm = g.b_perm.as<int32_t>(n + 1);
  g.sx = g.b_sx.as<float>(n + 1);
  g.sy = g.b_sy.as<float>(n + 1);
  g.sz = g.b_sz.as<float>(n + 1);
  g.sp = g.b_sp.as<float4>(n + 1);
  uint32_t* keys = g.b_keys.as<uint32_t>(n + 1);
  uint32_t* keys2 = g.b_keys2.as<uint32_t>(n + 1);
  uint32_t* vals = g.b_vals.as<uint32_t>(n + 1);
  g.skeys = keys2;  // cell key per sorted position

  // Speculative builds of small clouds take the counting-sort builder, unless this grid has shown
  // a fat cell: 6 launches instead of 16 where the build is launch-bound (configs[1], 100k
  // points).  Its per-point atomics run at the chip-wide atomic rate (k_count_keys: 77 us per 1M
  // points, ~13 G atomics/s) and slow the kernels of the other stream meanwhile (headline, 1M
  // points: 203-205 against 209-212 Mpoints/s with the radix sort), so larger clouds keep the
  // radix sort.  PFX_GRID_BUILD=sort|count forces either builder at any size (A/B runs).  Exact
  // builds always use the radix sort: their callers have no validation word to read, and the
  // counting builder may leave a fat cell unordered.
  if (g.oob && g.fat_pending) {  // the last exact build's finding (normally long complete)
    PFX_HIP(hipEventSynchronize(g.fat_ev));
    g.fat_pending = false;
    g.fat = *g.h_fat != 0;
  }
  const char* mode = std::getenv("PFX_GRID_BUILD");
  const bool want_count = mode && std::strcmp(mode, "count") == 0
                              ? true
                              : (mode && std::strcmp(mode, "sort") == 0 ? false : n <= kGridCountMaxPoints);
  g.counted = g.oob != nullptr && n > 0 && want_count && !g.fat;
  ++ctx->stats[g.counted ? "grid_count_builds" : "grid_sort_builds"];
  if (g.oob && !g.counted) ++ctx->stats["grid_hinted_sort_builds"];
  if (g.counted) {
    const int64_t blocks = ceil_div(n, kCountBlock);
    const int64_t m = C + 1 + blocks;  // cell counts, [C] = 0, per-block non-finite counts
    size_t scan_bytes = 0;
    PFX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (int32_t*)nullptr, (int32_t*)nullptr, int32_t(0), (size_t)m,
                                    rocprim::plus<int32_t>(), st));
    void* tmp = g.b_tmp.get(scan_bytes + 16);
    g.cell_start = g.b_start.as<int32_t>(m + 1);
    float4* scr = g.b_scr.as<float4>(n + 1);
    TimeScope ts(ctx, "grid_build");
    k_count_zero<<<(unsigned)std::min<int64_t>(ceil_div(m, 256), 2048), 256, 0, st>>>(g.cell_start, m, g.oob);
    k_count_keys<<<(unsigned)blocks, kCountBlock, 0, st>>>(d_x, d_y, d_z, n, cm, keys, vals, g.cell_start, g.oob);
    check_launch("k_count_keys");
    PFX_HIP(rocprim::exclusive_scan(tmp, scan_bytes, g.cell_start, g.cell_start, int32_t(0), (size_t)m,
                                    rocprim::plus<int32_t>(), st));
    k_count_scatter<<<(unsigned)blocks, kCountBlock, 0, st>>>(d_x, d_y, d_z, n, (uint32_t)C, keys, vals, g.cell_start,
                                                              scr, keys2);
    k_count_order<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(scr, keys2, n, (uint32_t)C, g.cell_start, g.perm, g.sx,
                                                              g.sy, g.sz, g.sp, g.oob);
    check_launch("k_count_order");
    return;
  }

  // onesweep radix sort even at ~1M keys: the default config switches to merge sort below 2^20
  // items (30+ block-merge launches, ~0.4 ms at 1M points on gfx950)
  using SortCfg = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                                             rocprim::default_config, 0>;
  int bits = 1;
  while ((int64_t(1) << bits) <= C) ++bits;
  // size every scratch buffer before the first launch (no realloc behind pending work)
  size_t sort_bytes = 0, scan_bytes = 0;
  PFX_HIP(rocprim::radix_sort_pairs<SortCfg>(nullptr, sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                    (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)std::max<int64_t>(n, 1),
                                    0, bits, st));
  auto rev = rocprim::make_reverse_iterator(static_cast<int32_t*>(nullptr));
  PFX_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, rev, rev, (size_t)(C + 1), rocprim::minimum<int32_t>(), st));
  void* tmp = g.b_tmp.get(std::max(sort_bytes, scan_bytes) + 16);
  g.cell_start = g.b_start.as<int32_t>(C + 2);
  {
    TimeScope ts(ctx, "grid_build");
    // cell_start[c] = first sorted position with key >= c: mark the first position of every
    // occupied cell, then a suffix minimum fills the empty cells (no per-point atomics)
    k_fill_i32<<<(unsigned)std::min<int64_t>(ceil_div(C + 2, 256), 2048), 256, 0, st>>>(g.cell_start, C + 2,
                                                                                       (int32_t)n);
    if (g.oob) k_fill_i32<<<1, 64, 0, st>>>(g.oob, 1, 0);
    if (n > 0) {
      k_cell_keys<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(d_x, d_y, d_z, n, cm, keys, vals, g.oob);
      check_launch("k_cell_keys");
      PFX_HIP(rocprim::radix_sort_pairs<SortCfg>(tmp, sort_bytes, keys, keys2, vals,
                                        reinterpret_cast<uint32_t*>(g.perm), (size_t)n, 0, bits, st));
      const bool forked = fork_gather && g.oob != nullptr;
      if (forked) ctx->fork_side(st);
      const auto gather = [&](hipStream_t s) {
        k_gather_sorted<<<(unsigned)ceil_div(n, 256), 256, 0, s>>>(d_x, d_y, d_z, n, reinterpret_cast<uint32_t*>(g.perm),
                                                                   g.sx, g.sy, g.sz, g.sp);
        check_launch("k_gather_sorted");
      };
      if (forked) gather(ctx->side);
      k_mark_starts<<<(unsigned)ceil_div(n, 256), 256, 0, st>>>(keys2, n, g.cell_start);
      auto r = rocprim::make_reverse_iterator(g.cell_start + C + 1);
      PFX_HIP(rocprim::inclusive_scan(tmp, scan_bytes, r, r, (size_t)(C + 1), rocprim::minimum<int32_t>(), st));
      if (!forked) gather(st);
    }
  }
  if (!g.oob && n > 0 && g.hint_user) {
    // an exact build says whether the counting builder could order this cloud's cells; the next
    // hinted build of this grid reads the answer
    int* d_fat = g.b_fat.as<int>(1);
    if (!g.h_fat) PFX_HIP(hipHostMalloc((void**)&g.h_fat, 64, hipHostMallocDefault));
    if (!g.fat_ev) PFX_HIP(hipEventCreateWithFlags(&g.fat_ev, hipEventDisableTiming));
    if (g.fat_pending) PFX_HIP(hipEventSynchronize(g.fat_ev));  // (an unread earlier answer: superseded)
    k_fill_i32<<<1, 64, 0, st>>>(d_fat, 1, 0);
    k_fat_cells<<<(unsigned)ceil_div(C, 256), 256, 0, st>>>(g.cell_start, C, d_fat);
    check_launch("k_fat_cells");
    PFX_HIP(hipMemcpyAsync(g.h_fat, d_fat, sizeof(int), hipMemcpyDeviceToHost, st));
    PFX_HIP(hipEventRecord(g.fat_ev, st));
    g.fat_pending = true;
  }
}

}  // namespace pfx
