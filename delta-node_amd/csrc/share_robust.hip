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
// The work split, the loads and the two-buffer pipeline over the rows are
// share_rows.hpp's (rows_accumulate<R + 1>, and rows_walk's loop written out in
// the kernel), shared with share_check.hip; this unit holds the verdict, the
// correction and the store.
//
// The correction is wave-uniform, candidate by candidate: for i = 0 .. k - 1
// the lanes whose verdict is i finish together, with |w_i|, |A_i| and the
// division constants of |w_i| D_all read from the kernel arguments at the
// uniform index i (scalar loads, SGPRs); a ballot skips a candidate none of
// the wave's lanes has by a scalar branch, and a wave without a located lane
// skips the loop.  On clean data no lane enters it.
//
// The two-error form (TWO, a plan of dn_m521_robust_plan2 with errors == 2;
// DESIGN.md §4.31) then takes the elements left unexplained through the
// wave-cooperative pair search of robust_pair.hpp: the element's four
// canonical syndromes go through 272 bytes of LDS per wave, the wave's lanes
// test one pair each, the owning lane corrects.  A wave without such an element
// pays one ballot; the one-error instantiations hold none of it.
//
// Everything a launch needs travels in its arguments (about 2.4 KB): no device
// table, no staging buffer, nothing to synchronise.  Lanes at or past n_elem
// are masked off for the whole body.
#include <hip/hip_runtime.h>

#include "dn_internal.hpp"
#include "robust_core.hpp"
#include "robust_pair.hpp"
#include "robust_plan.hpp"
#include "share_rows.hpp"

namespace dn {

struct RobustArgs {
  const uint8_t* shares[DN_MAX_RESOLVE];
  CheckWeights wt;
  uint32_t a[DN_MAX_RESOLVE];                   // |A_i|
  dn_m521_div_small_t div[DN_MAX_RESOLVE + 1];  // [i]: |w_i| D_all; [kRobustAll]: D_all
  uint8_t* out_fe;
  int64_t* out_u64;
  uint32_t* counts;
  uint8_t* culprit;
  uint64_t n_elem;
  uint32_t negate;
};
static_assert(sizeof(RobustArgs) <= 4096, "the launch's constants ride in the 4 KB kernel-argument segment");

enum RobustOut { kRobustField, kRobustInt64 };

template <int R, int OUT, bool TWO = false>
__global__ void __launch_bounds__(kRowsBlock) robust_kernel(const RobustArgs a) {
  static_assert(!TWO || R == 4, "two errors are located from four syndromes");
  // rows_walk's loop, written out: with this body as its lambda the field form's registers are
  // allocated otherwise (235 -> 219 VGPRs at R = 4) and it runs 1.7 % slower
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t ntiles = (a.n_elem + kTile - 1) / kTile;  // < 2^32 (the entry point): a tile index fits u32
  for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {  // (64 bits: t + gridDim.x may pass 2^32)
    const uint32_t tile = static_cast<uint32_t>(t);
    const uint32_t w = q * 64u + lane;
    const uint64_t e = static_cast<uint64_t>(tile) * kTile + w;
    if (e >= a.n_elem) continue;  // a dead lane (of the last tile): nothing read, nothing written
    const uint32_t k = a.wt.k;  // >= 3
    // the R syndromes and, chain R, T' weighted by |A_i| (share row i of the single vector; a later
    // records form passes its own)
    uint32_t S[R + 1][kChkAcc];
    rows_accumulate<R + 1>(
        [&a](uint32_t i, uint32_t (&c)[R + 1]) {
          c[R] = a.a[i];
          return syndrome_weights<R>(a.wt, i, c);
        },
        [&a](uint32_t i) { return a.shares[i]; }, k, tile, w, S);
    uint8_t verdict =
        check_verdict<R>(robust_syndromes<R>(S), static_cast<int>(k), [&a](int j, int s) { return a.wt.xp[j][s]; });
    uint32_t f[kChkLimbs];
    if (verdict >= kChkUnexplained) robust_plain(S[R], a.div[kRobustAll], a.negate, f);
    if constexpr (TWO) {  // the pairs: a wave's window is its own, so no workgroup barrier
      __shared__ uint32_t s_pair[kRowsBlock / 64][kPairWords];
      robust_pair_wave(a, s_pair[q], S, verdict, f);
    }
    // the correction, wave-uniform: candidate i's constants in SGPRs, a candidate without lanes skipped
    if (__ballot(verdict < kChkUnexplained) != 0ull) {
#pragma unroll 1
      for (uint32_t i = 0; i < k; ++i) {
        const uint64_t mine = __ballot(verdict == i);
        if (mine == 0ull) continue;
        // (a lane's bit of the ballot, not `verdict == i`: under that branch the compiler replaces i by
        // the lane's verdict, and the constants come by vector loads)
        if ((mine >> lane) & 1ull) robust_located(S[0], S[R], a.wt.c[0][i], a.a[i], a.div[i], a.negate, f);
      }
    }
    if constexpr (OUT == kRobustField) {
      store_fe_b(tile_rsrc(tile_base(a.out_fe, tile)), w, f);
    } else {
      __builtin_nontemporal_store(static_cast<int64_t>(f[0] | (static_cast<uint64_t>(f[1]) << 32)), a.out_u64 + e);
    }
    if (a.culprit) a.culprit[e] = verdict;
    verdict_count<true>(a.counts, verdict);
  }
}

template <int OUT>
static void launch_robust(int r, dim3 g, hipStream_t s, const RobustArgs& a) {
  switch (r) {
    case 2: hipLaunchKernelGGL((robust_kernel<2, OUT>), g, dim3(kRowsBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((robust_kernel<3, OUT>), g, dim3(kRowsBlock), 0, s, a); break;
    case 4: hipLaunchKernelGGL((robust_kernel<4, OUT>), g, dim3(kRowsBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((robust_kernel<4, OUT, true>), g, dim3(kRowsBlock), 0, s, a); break;  // two errors
  }
}

}  // namespace dn

using namespace dn;

extern "C" int dn_m521_robust_plan(const uint64_t* xs, int k, int threshold, dn_m521_robust_plan_t* out) {
  char why[160] = "";
  const int rc = robust_plan_build(xs, k, threshold, out, why, sizeof(why));
  return rc == DN_OK ? DN_OK : set_error(rc, "%s", why);
}

extern "C" int dn_m521_robust_plan2(const uint64_t* xs, int k, int threshold, int errors,
                                    dn_m521_robust_plan_t* out) {
  char why[160] = "";
  const int rc = robust_plan_build2(xs, k, threshold, errors, out, why, sizeof(why));
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
    a.a[i] = plan->a[i];
    a.div[i] = plan->div[i];
  }
  weights_fill(a.wt, chk);
  a.div[kRobustAll] = plan->div[kRobustAll];
  a.out_fe = static_cast<uint8_t*>(out_fe);
  a.out_u64 = out_u64;
  a.counts = counts;
  a.culprit = culprit;
  a.n_elem = n_elem;
  a.negate = plan->negate;
  const dim3 g(rows_grid(ntiles));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int form = plan->max_errors == 2u ? 5 : chk.r;  // (wellformed: two errors only with r == 4)
  if (out_fe) launch_robust<kRobustField>(form, g, s, a);
  else launch_robust<kRobustInt64>(form, g, s, a);
  return launch_status(name);
}
