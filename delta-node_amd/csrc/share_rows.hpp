// share_rows.hpp — what the kernels over k tiled share rows have in common
// (share_check.hip check_kernel, share_robust.hip robust_kernel; the verdict
// count and the weights block also check_records.hip): DESIGN.md §4.29.  A fix
// to the work split, the loads, the load/arithmetic pipeline or the counters
// is made here once.
//
// Work split: one element per lane, a wave owns 64 consecutive elements (a
// quarter of a 256-element tile), the four waves of a workgroup the four
// quarters of one tile, and workgroups stride over the tiles (the cyclic
// schedule of shamir_m521.hip wave_sched; grid_cap() workgroups at most).
// Lanes at or past n_elem are masked off for the whole body: they load and
// store nothing.
//
// Loads: a wave's load of one limb plane is one 256-byte instruction through
// the tile's buffer descriptor, non-temporal.  Two row buffers: the 17 loads
// of share i + 1 are issued before the multiply-adds of share i.  k is a
// run-time count, so the loop runs two shares per round, each buffer refilled
// in place, and every load of the steady state is unconditional (a load under
// a branch makes the wait behind it count only what both paths issued).
//
// Row bases, weights, signs and powers are kernel arguments indexed by the
// wave-uniform share counter: scalar loads, SGPRs.
#pragma once

#include <hip/hip_runtime.h>

#include "check_core.hpp"
#include "dn_internal.hpp"
#include "m521_device.hpp"

namespace dn {

constexpr int kRowsBlock = 256;
static_assert(kRowsBlock / 64 * 64 == kTile, "a workgroup's waves are the quarters of one tile");

// The syndrome weights of a launch (check_plan.hpp), embedded in the kernel arguments.
struct CheckWeights {
  uint32_t c[DN_M521_CHECK_MAX_R][DN_MAX_RESOLVE];   // |w_i| x_i^j
  uint32_t xp[DN_M521_CHECK_MAX_R][DN_MAX_RESOLVE];  // x_i^j
  uint32_t k;
  uint32_t neg;
};

inline void weights_fill(CheckWeights& w, const dn_m521_check_plan_t& plan) {
  for (int i = 0; i < plan.k; ++i)
    for (int j = 0; j < plan.r; ++j) {
      w.c[j][i] = static_cast<uint32_t>(plan.c[j][i]);
      w.xp[j][i] = plan.xp[j][i];
    }
  w.k = static_cast<uint32_t>(plan.k);
  w.neg = plan.neg;
}

// Workgroups per launch: one per tile, at most grid_cap().
inline uint32_t rows_grid(uint64_t ntiles) {
  const uint64_t cap = grid_cap();
  return static_cast<uint32_t>(ntiles < cap ? ntiles : cap);
}

// c[j] = |w_i| x_i^j for j < R, and share i's sign as check_mac takes it (scalar loads).
template <int R, int N>
__device__ __forceinline__ uint32_t syndrome_weights(const CheckWeights& wt, uint32_t i, uint32_t (&c)[N]) {
  static_assert(R <= N, "the syndromes are the first R chains");
#pragma unroll
  for (int j = 0; j < R; ++j) c[j] = wt.c[j][i];
  return 0u - ((wt.neg >> i) & 1u);
}

// Element w of the tile behind r, as it lies in memory (load_fe_b without the
// mask): the top plane is masked where check_mac consumes it, so that no load
// is waited for before its row's turn.
__device__ __forceinline__ void rows_load(rsrc_t r, uint32_t w, uint32_t (&y)[kChkLimbs]) {
  const uint32_t o4 = w * 4u, o2 = w * 2u;
#pragma unroll
  for (int l = 0; l < 16; ++l) y[l] = __builtin_amdgcn_raw_buffer_load_b32(r, o4, l * 4 * kTile, kNt);
  y[16] = static_cast<uint32_t>(__builtin_amdgcn_raw_buffer_load_b16(r, o2, static_cast<int>(kHiOffset), kNt));
}

// S[j] = sum_i +-c_i[j] y_i over element w (a live lane's) of tile `tile` of
// the rows rows(0 .. k - 1), k >= 2: N unreduced chains.  weights(i, c) fills
// share i's N weights and returns its sign (both wave-uniform).
template <int N, typename Weights, typename Rows>
__device__ __forceinline__ void rows_accumulate(Weights weights, Rows rows, uint32_t k, uint32_t tile, uint32_t w,
                                                uint32_t (&S)[N][kChkAcc]) {
#pragma unroll
  for (int j = 0; j < N; ++j)
#pragma unroll
    for (int l = 0; l < kChkAcc; ++l) S[j][l] = 0u;
  const auto load = [&](uint32_t i, uint32_t (&y)[kChkLimbs]) {
    rows_load(tile_rsrc(tile_base(rows(i), tile)), w, y);
  };
  const auto add = [&](uint32_t i, const uint32_t (&y)[kChkLimbs]) {
    uint32_t c[N];
    const uint32_t sign = weights(i, c);
    check_mac<N>(S, y, c, sign);
  };
  uint32_t y0[kChkLimbs], y1[kChkLimbs];
  load(0u, y0);
  uint32_t i = 0;
  for (; i + 2 < k; i += 2) {  // rows i + 1 and i + 2 exist
    load(i + 1u, y1);
    add(i, y0);
    // (the scheduler otherwise gathers both rows' loads in front of both rows' arithmetic)
    __builtin_amdgcn_sched_barrier(0);
    load(i + 2u, y0);
    add(i + 1u, y1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (i + 1 < k) {  // two rows left: i (loaded) and i + 1
    load(i + 1u, y1);
    add(i, y0);
    add(i + 1u, y1);
  } else {
    add(i, y0);
  }
}

// body(tile, w, e) for every live element e = tile * 256 + w of this lane:
// quarter q of the tiles blockIdx.x, blockIdx.x + gridDim.x, ...
template <typename Body>
__device__ __forceinline__ void rows_walk(uint64_t n_elem, Body body) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t ntiles = (n_elem + kTile - 1) / kTile;  // < 2^32 (the entry point): a tile index fits u32
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (64 bits: t + gridDim.x may pass 2^32)
    const uint32_t tile = static_cast<uint32_t>(t);
    const uint32_t w = q * 64u + lane;
    const uint64_t e = static_cast<uint64_t>(tile) * kTile + w;
    if (e >= n_elem) continue;  // a dead lane (of the last tile): nothing read, nothing written
    body(tile, w, e);
  }
}

// counts[0] += the wave's inconsistent elements, counts[1] += those with a
// located culprit (LOCATED): one atomic per wave and counter, only where
// non-zero.  The live lanes are a prefix of the wave (a dead lane that is
// present votes "consistent"), so the adding lane is lane 0.
template <bool LOCATED>
__device__ __forceinline__ void verdict_count(uint32_t* counts, uint8_t verdict) {
  const bool first = (threadIdx.x & 63u) == 0u;
  const uint64_t bad = __ballot(verdict != kChkConsistent);
  if (bad != 0ull && first) atomicAdd(counts, static_cast<uint32_t>(__popcll(bad)));
  if constexpr (LOCATED) {
    const uint64_t found = __ballot(verdict < kChkUnexplained);
    if (found != 0ull && first) atomicAdd(counts + 1, static_cast<uint32_t>(__popcll(found)));
  }
}

}  // namespace dn
