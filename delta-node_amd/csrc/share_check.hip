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
// The work split, the loads and the two-buffer pipeline over the rows are
// share_rows.hpp's (rows_walk, rows_accumulate), shared with share_robust.hip;
// this unit holds the verdict.  k is a run-time count — eight instantiations
// (R x culprit or not), none per k.
//
// Registers: 18 R accumulator limbs + 2 x 17 row limbs (R = 4: 106) and the
// multiply-add temporaries; no scratch at any R (DESIGN.md §4.26 has the
// table).
#include <hip/hip_runtime.h>

#include "check_plan.hpp"
#include "dn_internal.hpp"
#include "share_rows.hpp"

namespace dn {

struct CheckArgs {
  const uint8_t* shares[DN_MAX_RESOLVE];
  CheckWeights wt;
  uint32_t* counts;
  uint8_t* culprit;
  uint64_t n_elem;
};

template <int R, bool CULPRIT>
__global__ void __launch_bounds__(kRowsBlock) check_kernel(const CheckArgs a) {
  rows_walk(a.n_elem, [&a](uint32_t tile, uint32_t w, uint64_t e) {
    uint32_t S[R][kChkAcc];
    // (share row i of the single vector; a later list or records form passes its own)
    rows_accumulate<R>([&a](uint32_t i, uint32_t (&c)[R]) { return syndrome_weights<R>(a.wt, i, c); },
                       [&a](uint32_t i) { return a.shares[i]; }, a.wt.k, tile, w, S);
    uint8_t verdict;
    if constexpr (CULPRIT) {
      verdict = check_verdict<R>(S, static_cast<int>(a.wt.k), [&a](int j, int s) { return a.wt.xp[j][s]; });
      a.culprit[e] = verdict;
    } else {
      verdict = check_consistent<R>(S) ? kChkConsistent : kChkUnexplained;
    }
    verdict_count<CULPRIT>(a.counts, verdict);
  });
}

template <bool CULPRIT>
static void launch_check(int r, dim3 g, hipStream_t s, const CheckArgs& a) {
  switch (r) {
    case 1: hipLaunchKernelGGL((check_kernel<1, CULPRIT>), g, dim3(kRowsBlock), 0, s, a); break;
    case 2: hipLaunchKernelGGL((check_kernel<2, CULPRIT>), g, dim3(kRowsBlock), 0, s, a); break;
    case 3: hipLaunchKernelGGL((check_kernel<3, CULPRIT>), g, dim3(kRowsBlock), 0, s, a); break;
    default: hipLaunchKernelGGL((check_kernel<4, CULPRIT>), g, dim3(kRowsBlock), 0, s, a); break;
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
  }
  weights_fill(a.wt, *plan);
  a.counts = counts;
  a.culprit = culprit;
  a.n_elem = n_elem;
  const dim3 g(rows_grid(ntiles));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (culprit) launch_check<true>(plan->r, g, s, a);
  else launch_check<false>(plan->r, g, s, a);
  return launch_status(name);
}
