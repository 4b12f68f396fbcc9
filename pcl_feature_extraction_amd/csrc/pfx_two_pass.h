// pfx_two_pass.h -- the frame of the descriptors that give a query one 256-thread workgroup and hold
// its FLANN-ordered neighbour keys in LDS (spin images, intensity gradient, RIFT, intensity spin images,
// shape contexts, moments and curvatures, SHOT's frames alone, BOARD's frames).  DESIGN.md "The descriptors'
// common frame".
//
// Two passes: every query with kTwoPassCapSmall keys and the bucketed sort; a query with more
// neighbours is queued on the device for the second pass with kTwoPassCap keys and the bitonic sort
// (one workgroup per CU).  More than that is PFX_ERR_CAPACITY, reported late (pfx_internal.h, the
// deferred reports).  Behind the keys lie kTwoPassAuxBytes: the bucketed sort's scratch and, the
// sort done, the family's records of one chunk of kTwoPassChunk neighbours.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <type_traits>

#include "pfx_neighbors.h"

namespace pfx {

constexpr int kTwoPassCapSmall = 2048;  // keys of the first pass (bucketed sort: 2 x 16 KiB of LDS)
constexpr int kTwoPassCap = 16384;      // keys of the second pass (128 KiB: one workgroup per CU)
constexpr int kTwoPassChunk = 256;      // neighbours per chunk of records = the block size
constexpr size_t kTwoPassAuxBytes = sizeof(uint64_t) * kTwoPassCapSmall;
constexpr size_t kTwoPassLdsSmall = sizeof(uint64_t) * kTwoPassCapSmall + kTwoPassAuxBytes;
constexpr size_t kTwoPassLdsLarge = sizeof(uint64_t) * kTwoPassCap + kTwoPassAuxBytes;

// A slot's words (ints).  Sticky until reported: kWordOver, then the family's own from kWordSticky.
// Per call: the rest, the family's own from kWordOwn.
enum TwoPassWord {
  kWordOver = 0,       // largest k beyond kTwoPassCap
  kWordSticky = 1,     // [1..3]
  kWordQueued = 4,     // queries queued for the second pass
  kWordKmax = 5,       // max k
  kWordNeighbors = 6,  // [6..7] neighbours (u64)
  kWordOwn = 8,        // [8..11]
};

// The sorted keys of a query's neighbours in keys[0..k); returns k (> CAP: nothing sorted).  The
// first pass's scratch is the CAP words behind the keys.
template <int CAP>
__device__ __forceinline__ int two_pass_neighbors(const GridView& g, float qx, float qy, float qz, float rr,
                                                  uint64_t* keys, int* s_count, BucketLds& SB) {
  return CAP == kTwoPassCapSmall ? sorted_neighbors_bucketed(g, qx, qy, qz, rr, keys, keys + CAP, CAP, s_count, SB)
                                 : sorted_neighbors(g, qx, qy, qz, rr, keys, CAP, s_count);
}

// a query with more than CAP neighbours (one thread): queued for the second pass, or, without a
// queue, beyond every capacity.  STATS: the family reports kWordKmax.
template <bool STATS = true>
__device__ __forceinline__ void over_or_err(int k, int64_t q, int32_t* over, int* err) {
  if (over) {
    over[atomicAdd(err + kWordQueued, 1)] = (int32_t)q;
  } else {
    atomicMax(err + kWordOver, k);
    if (STATS) atomicMax(err + kWordKmax, k);
  }
}

// an admitted query's k into the statistics (one thread)
__device__ __forceinline__ void count_neighbors(int k, int* err) {
  atomicAdd(reinterpret_cast<unsigned long long*>(err + kWordNeighbors), (unsigned long long)k);
  atomicMax(err + kWordKmax, k);
}

// kern<<<blocks, kTwoPassChunk, lds>>>(args...); dynamic LDS beyond the 64 KiB that every kernel may
// use (the second pass) is asked for first
template <class Kern, class... Args>
void two_pass_launch(Kern kern, unsigned blocks, size_t lds, hipStream_t st, Args... args) {
  if (lds > (64u << 10))
    PFX_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<blocks, kTwoPassChunk, lds, st>>>(args...);
}

// The two passes over nq queries of a surface of ns points.  launch(cap, blocks, lds, list, n_list,
// over) launches the family's kernel of capacity cap() (an std::integral_constant) through
// two_pass_launch.  First pass: every query, one workgroup each, dispatched as CUs free up; queries
// beyond its capacity go to `over` (the buffer over_name), their count to err[kWordQueued].  Second
// pass: the queued ones (the count stays on the device); it exists only when the surface has more
// points than the first pass holds, else `over` is null and never reached.
template <class Launch>
void two_pass(pfx_ctx* ctx, int64_t ns, int64_t nq, const char* over_name, int* err, Launch&& launch,
              size_t lds_small = kTwoPassLdsSmall, size_t lds_large = kTwoPassLdsLarge) {
  const bool second_pass = ns > kTwoPassCapSmall;
  int32_t* over = second_pass ? ctx->buf(over_name).as<int32_t>((size_t)nq) : nullptr;
  launch(std::integral_constant<int, kTwoPassCapSmall>(), (unsigned)std::min<int64_t>(nq, 1 << 20), lds_small,
         (const int32_t*)nullptr, (const int*)nullptr, over);
  if (second_pass)
    launch(std::integral_constant<int, kTwoPassCap>(), (unsigned)std::min<int64_t>(nq, 256), lds_large,
           (const int32_t*)over, (const int*)(err + kWordQueued), (int32_t*)nullptr);
}

// What every family's finish step shares: the statistics `stat`_neighbors, _kmax and _queued of the
// words h, and the capacity error under the call's name `what`.
inline void two_pass_report(pfx_ctx* ctx, const int* h, const std::string& stat, const char* what,
                            bool queued = true) {
  unsigned long long nb;
  std::memcpy(&nb, h + kWordNeighbors, sizeof(nb));
  ctx->stats[stat + "_neighbors"] = (int64_t)nb;
  ctx->stats[stat + "_kmax"] = h[kWordKmax];
  if (queued) ctx->stats[stat + "_queued"] = h[kWordQueued];
  if (h[kWordOver] > 0)
    throw Error(PFX_ERR_CAPACITY, what + std::string(": a query has ") + std::to_string(h[kWordOver]) +
                                      " neighbours (> " + std::to_string(kTwoPassCap) + " supported)");
}

// n floats of NaN (a call without a surface: every neighbourhood is empty)
inline void fill_nan(pfx_ctx* ctx, float* p, int64_t n) {
  if (n <= 0) return;
  k_fill<<<(unsigned)ceil_div(n, 256), 256, 0, ctx->stream>>>(p, n, __builtin_nanf(""));
  check_launch("k_fill");
}

}  // namespace pfx
