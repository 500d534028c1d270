// share_robust.hip — the robust reconstruct (dn_m521_robust_plan,
// dn_m521_reconstruct_robust): f(0) per element from k >= t + 2
// tiled share vectors, past one bad share per element, in one launch that reads
// every row once.
//
// Per element the R = k - t syndromes and T' = sum_m |A_m| (+-y_m), the
// all-k Lagrange sum over its common denominator, are accumulated together,
// unreduced, 18 limbs each: check_mac<R + 1>, chain R weighted by |A_m|
// (robust_plan.hpp).  The verdict is check_verdict's; a consistent or
// unexplained lane divides T' by D_all, a lane whose share i is located forms
// |w_i| T' - |A_i| S_0 and divides by |w_i| D_all (robust_core.hpp, the same
// text the host rehearsal runs).  HBM-bound on clean data: 66 k bytes read and
// 66 or 8 written per element next to (R + 1) k 17 multiply-adds.
//
// Work split and loads are share_check.hip's: one element per lane, a wave a
// quarter of a 256-element tile, workgroups striding over the tiles; one
// 256-byte non-temporal buffer load per limb plane; two row buffers, the 17
// loads of share i + 1 issued before the multiply-adds of share i, two shares
// per round so that every steady-state load is unconditional.
//
// The correction is wave-uniform, candidate by candidate: for i = 0 .. k - 1
// the lanes whose verdict is i finish together, with |w_i|, |A_i| and the
// division constants of |w_i| D_all read from the kernel arguments at the
// uniform index i (scalar loads, SGPRs); a ballot skips a candidate none of
// the wave's lanes has by a scalar branch, and a wave without a located lane
// skips the loop.  On clean data no lane enters it.
//
// Everything a launch needs travels in its arguments (about 2.4 KB): no device
// table, no staging buffer, nothing to synchronise.  Lanes at or past n_elem
// are masked off for the whole body.
#include <hip/hip_runtime.h>

#include "dn_internal.hpp"
#include "m521_device.hpp"
#include "robust_core.hpp"
#include "robust_plan.hpp"

namespace dn {

struct RobustArgs {
  const uint8_t* shares[DN_MAX_RESOLVE];
  uint32_t c[DN_M521_CHECK_MAX_R][DN_MAX_RESOLVE];   // |w_i| x_i^j
  uint32_t a[DN_MAX_RESOLVE];                        // |A_i|
  uint32_t xp[DN_M521_CHECK_MAX_R][DN_MAX_RESOLVE];  // x_i^j
  dn_m521_div_small_t div[DN_MAX_RESOLVE + 1];       // [i]: |w_i| D_all; [kRobustAll]: D_all
  uint8_t* out_fe;
  int64_t* out_u64;
  uint32_t* counts;
  uint8_t* culprit;
  uint64_t n_elem;
  uint32_t k;
  uint32_t neg;
  uint32_t negate;
};
static_assert(sizeof(RobustArgs) <= 4096, "the launch's constants ride in the 4 KB kernel-argument segment");

constexpr int kRobustBlock = 256;
static_assert(kRobustBlock / 64 * 64 == kTile, "a workgroup's waves are the quarters of one tile");

enum RobustOut { kRobustField, kRobustInt64 };

// Share row i of the single vector (a later records form passes its own).
struct RobustRows {
  const RobustArgs& a;
  __device__ __forceinline__ const uint8_t* operator()(uint32_t i) const { return a.shares[i]; }
};

// Element w of the tile behind r, as it lies in memory: the top plane is
// masked where check_mac consumes it, so no load is waited for before its turn.
__device__ __forceinline__ void robust_load(rsrc_t r, uint32_t w, uint32_t (&y)[kChkLimbs]) {
  const uint32_t o4 = w * 4u, o2 = w * 2u;
#pragma unroll
  for (int l = 0; l < 16; ++l) y[l] = __builtin_amdgcn_raw_buffer_load_b32(r, o4, l * 4 * kTile, kNt);
  y[16] = static_cast<uint32_t>(__builtin_amdgcn_raw_buffer_load_b16(r, o2, static_cast<int>(kHiOffset), kNt));
}

// S[j] += +-c[j][i] y for j < R and S[R] += +-|A_i| y (share i's weights and sign: scalar loads).
template <int R>
__device__ __forceinline__ void robust_add(const RobustArgs& a, uint32_t i, uint32_t (&S)[R + 1][kChkAcc],
                                           const uint32_t (&y)[kChkLimbs]) {
  uint32_t c[R + 1];
#pragma unroll
  for (int j = 0; j < R; ++j) c[j] = a.c[j][i];
  c[R] = a.a[i];
  check_mac<R + 1>(S, y, c, 0u - ((a.neg >> i) & 1u));
}

// The R + 1 finished chains of element w (a live lane's) of tile `tile` of the rows row(0..k-1).
template <int R, typename Row>
__device__ __forceinline__ void robust_accumulate(const RobustArgs& a, Row row, uint32_t tile, uint32_t w,
                                                  uint32_t (&S)[R + 1][kChkAcc]) {
#pragma unroll
  for (int j = 0; j <= R; ++j)
#pragma unroll
    for (int l = 0; l < kChkAcc; ++l) S[j][l] = 0u;
  uint32_t y0[kChkLimbs], y1[kChkLimbs];
  const uint32_t k = a.k;  // >= 3
  robust_load(tile_rsrc(tile_base(row(0u), tile)), w, y0);
  uint32_t i = 0;
  for (; i + 2 < k; i += 2) {  // rows i + 1 and i + 2 exist
    robust_load(tile_rsrc(tile_base(row(i + 1u), tile)), w, y1);
    robust_add<R>(a, i, S, y0);
    // (the scheduler otherwise gathers both rows' loads in front of both rows' arithmetic)
    __builtin_amdgcn_sched_barrier(0);
    robust_load(tile_rsrc(tile_base(row(i + 2u), tile)), w, y0);
    robust_add<R>(a, i + 1u, S, y1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (i + 1 < k) {  // two rows left: i (loaded) and i + 1
    robust_load(tile_rsrc(tile_base(row(i + 1u), tile)), w, y1);
    robust_add<R>(a, i, S, y0);
    robust_add<R>(a, i + 1u, S, y1);
  } else {
    robust_add<R>(a, i, S, y0);
  }
}

template <int R, int OUT>
__global__ void __launch_bounds__(kRobustBlock) robust_kernel(const RobustArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t ntiles = (a.n_elem + kTile - 1) / kTile;  // < 2^32 (the entry point): a tile index fits u32
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (64 bits: t + gridDim.x may pass 2^32)
    const uint32_t tile = static_cast<uint32_t>(t);
    const uint32_t w = q * 64u + lane;
    const uint64_t e = static_cast<uint64_t>(tile) * kTile + w;
    if (e >= a.n_elem) continue;  // a dead lane (of the last tile): nothing read, nothing written
    uint32_t S[R + 1][kChkAcc];
    robust_accumulate<R>(a, RobustRows{a}, tile, w, S);
    const uint32_t k = a.k;
    const uint8_t verdict =
        check_verdict<R>(robust_syndromes<R>(S), static_cast<int>(k), [&a](int j, int s) { return a.xp[j][s]; });
    uint32_t f[kChkLimbs];
    if (verdict >= kChkUnexplained) robust_plain(S[R], a.div[kRobustAll], a.negate, f);
    // the correction, wave-uniform: candidate i's constants in SGPRs, a candidate without lanes skipped
    const uint64_t found = __ballot(verdict < kChkUnexplained);
    if (found != 0ull) {
#pragma unroll 1
      for (uint32_t i = 0; i < k; ++i) {
        const uint64_t mine = __ballot(verdict == i);
        if (mine == 0ull) continue;
        // (a lane's bit of the ballot, not `verdict == i`: under that branch the compiler replaces i by
        // the lane's verdict, and the constants come by vector loads)
        if ((mine >> lane) & 1ull) robust_located(S[0], S[R], a.c[0][i], a.a[i], a.div[i], a.negate, f);
      }
    }
    if constexpr (OUT == kRobustField) {
      store_fe_b(tile_rsrc(tile_base(a.out_fe, tile)), w, f);
    } else {
      __builtin_nontemporal_store(static_cast<int64_t>(f[0] | (static_cast<uint64_t>(f[1]) << 32)), a.out_u64 + e);
    }
    if (a.culprit) a.culprit[e] = verdict;
    // one atomic per wave and counter (the live lanes are a prefix of the wave: its first lane adds)
    const uint64_t bad = __ballot(verdict != kChkConsistent);
    if (bad != 0ull && lane == 0u) atomicAdd(a.counts, static_cast<uint32_t>(__popcll(bad)));
    if (found != 0ull && lane == 0u) atomicAdd(a.counts + 1, static_cast<uint32_t>(__popcll(found)));
  }
}

// Workgroups per launch: one per tile, at most 16384 (as share_check.hip
// check_grid; DN_GRID_CAP overrides it in the tuning build).
static uint32_t robust_grid(uint64_t ntiles) {
  const char* s = tune_env("DN_GRID_CAP");
  const int v = s ? std::atoi(s) : 0;
  const uint64_t cap = v > 0 ? static_cast<uint64_t>(v) : 16384u;
  return static_cast<uint32_t>(ntiles < cap ? ntiles : cap);
}

template <int OUT>
static void launch_robust(int r, dim3 g, hipStream_t s, const RobustArgs& a) {
  switch (r) {
    case 2: hipLaunchKernelGGL((robust_kernel<2, OUT>), g, dim3(kRobustBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((robust_kernel<3, OUT>), g, dim3(kRobustBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((robust_kernel<4, OUT>), g, dim3(kRobustBlock), 0, s, a); break;
  }
}

}  // namespace dn

using namespace dn;

extern "C" int dn_m521_robust_plan(const uint64_t* xs, int k, int threshold, dn_m521_robust_plan_t* out) {
  char why[160] = "";
  const int rc = robust_plan_build(xs, k, threshold, out, why, sizeof(why));
  return rc == DN_OK ? DN_OK : set_error(rc, "%s", why);
}

extern "C" int dn_m521_reconstruct_robust(const void* const* share_vecs, const dn_m521_robust_plan_t* plan,
                                          void* out_fe, int64_t* out_u64, uint32_t* counts, uint8_t* culprit,
                                          uint64_t n_elem, void* stream) {
  const char* name = "dn_m521_reconstruct_robust";
  if (n_elem == 0) return DN_OK;
  if (!plan || !share_vecs || !counts) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if ((out_fe != nullptr) == (out_u64 != nullptr))
    return set_error(DN_ERR_ARG, "%s: exactly one of out_fe and out_u64", name);
  if (!robust_plan_wellformed(*plan)) return set_error(DN_ERR_ARG, "%s: malformed plan", name);
  const uint64_t ntiles = (n_elem + kTile - 1) / kTile;
  if (ntiles > (1ull << 32) - 1) return set_error(DN_ERR_ARG, "%s: more than 2^32 tiles", name);
  const dn_m521_check_plan_t& chk = plan->check;
  RobustArgs a{};
  for (int i = 0; i < chk.k; ++i) {
    if (!share_vecs[i]) return set_error(DN_ERR_ARG, "%s: null share vector %d", name, i);
    a.shares[i] = static_cast<const uint8_t*>(share_vecs[i]);
    for (int j = 0; j < chk.r; ++j) {
      a.c[j][i] = static_cast<uint32_t>(chk.c[j][i]);
      a.xp[j][i] = chk.xp[j][i];
    }
    a.a[i] = plan->a[i];
    a.div[i] = plan->div[i];
  }
  a.div[kRobustAll] = plan->div[kRobustAll];
  a.out_fe = static_cast<uint8_t*>(out_fe);
  a.out_u64 = out_u64;
  a.counts = counts;
  a.culprit = culprit;
  a.n_elem = n_elem;
  a.k = static_cast<uint32_t>(chk.k);
  a.neg = chk.neg;
  a.negate = plan->negate;
  const dim3 g(robust_grid(ntiles));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (out_fe) launch_robust<kRobustField>(chk.r, g, s, a);
  else launch_robust<kRobustInt64>(chk.r, g, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: launch failed: %s", name, hipGetErrorString(err));
  return DN_OK;
}
