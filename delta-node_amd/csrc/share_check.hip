// share_check.hip — the share consistency check (dn_m521_check_plan,
// dn_m521_check_shares): do the k > t shares of an element lie
// on one polynomial of degree < t, and if not, which single share is off?
//
// Per element the R = k - t syndromes S_j = sum_i +-c[j][i] y_i (check_plan.hpp)
// are accumulated unreduced, 18 limbs each, and tested for 0 mod p once
// (check_core.hpp, the same text the host rehearsal runs).  Every row is read
// once and one byte per element is written: HBM-bound, 66 k + 1 bytes per
// element next to R k 17 multiply-adds.
//
// Work split: one element per lane, a wave owns 64 consecutive elements (a
// quarter of a 256-element tile), the four waves of a workgroup the four
// quarters of one tile, and workgroups stride over the tiles (the cyclic
// schedule of shamir_m521.hip wave_sched with grid_for's cap; both are local
// to that unit).  A wave's load of one limb plane is one 256-byte instruction
// through the tile's buffer descriptor, non-temporal (m521_device.hpp
// load_fe_b's loads, raw: the top plane is masked where check_mac consumes it,
// so that no load is waited for before its row's turn).  Two row buffers: the
// 17 loads of share i + 1 are issued before the multiply-adds of share i.  k is
// a run-time count — eight instantiations (R x culprit or not), none per k —
// so the loop runs two shares per round, each buffer refilled in place, and
// every load of the steady state is unconditional (a load under a branch makes
// the wait behind it count only what both paths issued).
//
// Registers: 18 R accumulator limbs + 2 x 17 row limbs (R = 4: 106) and the
// multiply-add temporaries; no scratch at any R (DESIGN.md §4.26 has the
// table).  Row bases, weights, signs and powers are kernel arguments indexed
// by the wave-uniform share counter: scalar loads, SGPRs.  Lanes at or past
// n_elem are masked off for the whole body: they load and store nothing.
#include <hip/hip_runtime.h>

#include "check_core.hpp"
#include "check_plan.hpp"
#include "dn_internal.hpp"
#include "m521_device.hpp"

namespace dn {

struct CheckArgs {
  const uint8_t* shares[DN_MAX_RESOLVE];
  uint32_t c[DN_M521_CHECK_MAX_R][DN_MAX_RESOLVE];   // |w_i| x_i^j
  uint32_t xp[DN_M521_CHECK_MAX_R][DN_MAX_RESOLVE];  // x_i^j
  uint32_t* counts;
  uint8_t* culprit;
  uint64_t n_elem;
  uint32_t k;
  uint32_t neg;
};

constexpr int kCheckBlock = 256;
constexpr int kCheckWaves = kCheckBlock / 64;
static_assert(kCheckWaves * 64 == kTile, "a workgroup's waves are the quarters of one tile");

// Share row i of the single vector (a later list or records form passes its own).
struct CheckRows {
  const CheckArgs& a;
  __device__ __forceinline__ const uint8_t* operator()(uint32_t i) const { return a.shares[i]; }
};

// Element w of the tile behind r, as it lies in memory (load_fe_b without the mask).
__device__ __forceinline__ void check_load(rsrc_t r, uint32_t w, uint32_t (&y)[kChkLimbs]) {
  const uint32_t o4 = w * 4u, o2 = w * 2u;
#pragma unroll
  for (int l = 0; l < 16; ++l) y[l] = __builtin_amdgcn_raw_buffer_load_b32(r, o4, l * 4 * kTile, kNt);
  y[16] = static_cast<uint32_t>(__builtin_amdgcn_raw_buffer_load_b16(r, o2, static_cast<int>(kHiOffset), kNt));
}

// S[j] += +-c[j][i] y for share i (its weights and sign: scalar loads).
template <int R>
__device__ __forceinline__ void check_add(const CheckArgs& a, uint32_t i, uint32_t (&S)[R][kChkAcc],
                                          const uint32_t (&y)[kChkLimbs]) {
  uint32_t c[R];
#pragma unroll
  for (int j = 0; j < R; ++j) c[j] = a.c[j][i];
  check_mac<R>(S, y, c, 0u - ((a.neg >> i) & 1u));
}

// The culprit byte of element w (a live lane's) of tile `tile` of the rows row(0..k-1).
template <int R, bool CULPRIT, typename Row>
__device__ __forceinline__ uint8_t check_element(const CheckArgs& a, Row row, uint32_t tile, uint32_t w) {
  uint32_t S[R][kChkAcc];
#pragma unroll
  for (int j = 0; j < R; ++j)
#pragma unroll
    for (int l = 0; l < kChkAcc; ++l) S[j][l] = 0u;
  uint32_t y0[kChkLimbs], y1[kChkLimbs];
  const uint32_t k = a.k;  // >= 2
  check_load(tile_rsrc(tile_base(row(0u), tile)), w, y0);
  uint32_t i = 0;
  for (; i + 2 < k; i += 2) {  // rows i + 1 and i + 2 exist
    check_load(tile_rsrc(tile_base(row(i + 1u), tile)), w, y1);
    check_add<R>(a, i, S, y0);
    // (the scheduler otherwise gathers both rows' loads in front of both rows' arithmetic)
    __builtin_amdgcn_sched_barrier(0);
    check_load(tile_rsrc(tile_base(row(i + 2u), tile)), w, y0);
    check_add<R>(a, i + 1u, S, y1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (i + 1 < k) {  // two rows left: i (loaded) and i + 1
    check_load(tile_rsrc(tile_base(row(i + 1u), tile)), w, y1);
    check_add<R>(a, i, S, y0);
    check_add<R>(a, i + 1u, S, y1);
  } else {
    check_add<R>(a, i, S, y0);
  }
  if constexpr (CULPRIT) {
    return check_verdict<R>(S, static_cast<int>(k), [&a](int j, int s) { return a.xp[j][s]; });
  } else {
    return check_consistent<R>(S) ? kChkConsistent : kChkUnexplained;
  }
}

template <int R, bool CULPRIT>
__global__ void __launch_bounds__(kCheckBlock) check_kernel(const CheckArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t ntiles = (a.n_elem + kTile - 1) / kTile;  // < 2^32 (the entry point): a tile index fits u32
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (64 bits: t + gridDim.x may pass 2^32)
    const uint32_t tile = static_cast<uint32_t>(t);
    const uint32_t w = q * 64u + lane;
    const uint64_t e = static_cast<uint64_t>(tile) * kTile + w;
    if (e >= a.n_elem) continue;  // a dead lane (of the last tile): nothing read, nothing written
    const uint8_t verdict = check_element<R, CULPRIT>(a, CheckRows{a}, tile, w);
    if constexpr (CULPRIT) a.culprit[e] = verdict;
    // one atomic per wave and counter (the live lanes are a prefix of the wave: its first lane adds)
    const uint64_t bad = __ballot(verdict != kChkConsistent);
    if (bad != 0ull && lane == 0u) atomicAdd(a.counts, static_cast<uint32_t>(__popcll(bad)));
    if constexpr (CULPRIT) {
      const uint64_t found = __ballot(verdict < kChkUnexplained);
      if (found != 0ull && lane == 0u) atomicAdd(a.counts + 1, static_cast<uint32_t>(__popcll(found)));
    }
  }
}

// Workgroups per launch: one per tile, at most 16384 (as shamir_m521.hip
// grid_for; DN_GRID_CAP overrides it in the tuning build).
static uint32_t check_grid(uint64_t ntiles) {
  const char* s = tune_env("DN_GRID_CAP");
  const int v = s ? std::atoi(s) : 0;
  const uint64_t cap = v > 0 ? static_cast<uint64_t>(v) : 16384u;
  return static_cast<uint32_t>(ntiles < cap ? ntiles : cap);
}

template <bool CULPRIT>
static void launch_check(int r, dim3 g, hipStream_t s, const CheckArgs& a) {
  switch (r) {
    case 1: hipLaunchKernelGGL((check_kernel<1, CULPRIT>), g, dim3(kCheckBlock), 0, s, a); break;
    case 2: hipLaunchKernelGGL((check_kernel<2, CULPRIT>), g, dim3(kCheckBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((check_kernel<3, CULPRIT>), g, dim3(kCheckBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((check_kernel<4, CULPRIT>), g, dim3(kCheckBlock), 0, s, a); break;
  }
}

}  // namespace dn

using namespace dn;

extern "C" int dn_m521_check_plan(const uint64_t* xs, int k, int threshold, dn_m521_check_plan_t* out) {
  char why[160] = "";
  const int rc = check_plan_build(xs, k, threshold, out, why, sizeof(why));
  return rc == DN_OK ? DN_OK : set_error(rc, "%s", why);
}

extern "C" int dn_m521_check_shares(const void* const* share_vecs, const dn_m521_check_plan_t* plan, uint32_t* counts,
                                    uint8_t* culprit, uint64_t n_elem, void* stream) {
  const char* name = "dn_m521_check_shares";
  if (n_elem == 0) return DN_OK;
  if (!plan || !share_vecs || !counts) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  if (!check_plan_wellformed(*plan)) return set_error(DN_ERR_ARG, "%s: malformed plan", name);
  const uint64_t ntiles = (n_elem + kTile - 1) / kTile;
  if (ntiles > (1ull << 32) - 1) return set_error(DN_ERR_ARG, "%s: more than 2^32 tiles", name);
  CheckArgs a{};
  for (int i = 0; i < plan->k; ++i) {
    if (!share_vecs[i]) return set_error(DN_ERR_ARG, "%s: null share vector %d", name, i);
    a.shares[i] = static_cast<const uint8_t*>(share_vecs[i]);
    for (int j = 0; j < plan->r; ++j) {
      a.c[j][i] = static_cast<uint32_t>(plan->c[j][i]);
      a.xp[j][i] = plan->xp[j][i];
    }
  }
  a.counts = counts;
  a.culprit = culprit;
  a.n_elem = n_elem;
  a.k = static_cast<uint32_t>(plan->k);
  a.neg = plan->neg;
  const dim3 g(check_grid(ntiles));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (culprit) launch_check<true>(plan->r, g, s, a);
  else launch_check<false>(plan->r, g, s, a);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: launch failed: %s", name, hipGetErrorString(err));
  return DN_OK;
}
