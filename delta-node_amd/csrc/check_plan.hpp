// check_plan.hpp — the integer parity-check weights of a share consistency
// check (dn_m521_check_plan; the kernel is share_check.hip, the arithmetic it
// runs check_core.hpp).
//
// For distinct abscissas x_1..x_k, P_i = prod_{m != i} |x_i - x_m| and
// D = lcm_i P_i give the signed integers w_i = +-D / P_i (negative when an odd
// number of abscissas lie above x_i) with sum_i w_i x_i^j f(x_i) = 0 for every
// f of degree < t and j < r = k - t.  The plan holds c[j][i] = |w_i| x_i^j,
// the signs and the powers x_i^j, all exact (128-bit intermediates, as
// dn_m521_lagrange forms its rationals; whatever leaves them is unsupported).
//
// kCheckMaxC is the kernel's bound: it multiplies one share limb by c[j][i] in
// a single 32 x 32 -> 64 bit step, and k <= 16 terms c * Y (Y < 2^521) then
// sum to less than 2^557, inside the 18 limbs it keeps a syndrome in
// (check_core.hpp).  Plain C++: no HIP header.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dn_shamir.h"

namespace dn {

constexpr uint64_t kCheckMaxC = 1ull << 32;

namespace check_detail {
using u128 = unsigned __int128;
constexpr u128 kLim = static_cast<u128>(1) << 126;

inline u128 gcd(u128 a, u128 b) {
  while (b) {
    const u128 t = a % b;
    a = b;
    b = t;
  }
  return a;
}
// *out = a * b unless it would pass kLim.
inline bool mul(u128 a, u128 b, u128* out) {
  if (a != 0 && b > kLim / a) return false;
  *out = a * b;
  return true;
}
}  // namespace check_detail

// Fills *out and returns DN_OK, or a DN_ERR_* code with the reason in why[why_len].
inline int check_plan_build(const uint64_t* xs, int k, int threshold, dn_m521_check_plan_t* out, char* why,
                            size_t why_len) {
  using namespace check_detail;
  auto fail = [&](int code, const char* msg) {
    snprintf(why, why_len, "%s", msg);
    return code;
  };
  if (!out || (k > 0 && !xs)) return fail(DN_ERR_ARG, "dn_m521_check_plan: null pointer");
  if (threshold < 1) return fail(DN_ERR_ARG, "dn_m521_check_plan: threshold below 1");
  // dn_m521_lagrange's checks, in its order and words (shamir.py:70-83)
  if (k < 1) return fail(DN_ERR_ARG, "not enough values to unpack (expected 2, got 0)");
  if (k < threshold) {
    snprintf(why, why_len, "need at least %d shares", threshold);
    return DN_ERR_TOO_FEW;
  }
  for (int i = 0; i < k; ++i)
    for (int j = i + 1; j < k; ++j)
      if (xs[i] == xs[j]) return fail(DN_ERR_DISTINCT, "shares must be distinct");
  if (k == 1) return fail(DN_ERR_EMPTY, "reduce() of empty iterable with no initial value");
  if (k > DN_MAX_RESOLVE) {
    snprintf(why, why_len, "dn_m521_check_plan: more than %d shares", DN_MAX_RESOLVE);
    return DN_ERR_UNSUPPORTED;
  }
  // the check's own limits
  const int r = k - threshold;
  if (r == 0)
    return fail(DN_ERR_UNSUPPORTED, "dn_m521_check_plan: as many shares as the threshold: no spare share to check");
  if (r > DN_M521_CHECK_MAX_R) {
    snprintf(why, why_len, "dn_m521_check_plan: more than %d spare shares", DN_M521_CHECK_MAX_R);
    return DN_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < k; ++i)
    if (xs[i] == 0) return fail(DN_ERR_UNSUPPORTED, "dn_m521_check_plan: abscissa 0");
  const char* wide = "dn_m521_check_plan: the weights of these abscissas leave 128 bits";
  u128 P[DN_MAX_RESOLVE], D = 1;
  uint32_t neg = 0;
  for (int i = 0; i < k; ++i) {
    P[i] = 1;
    for (int m = 0; m < k; ++m) {
      if (m == i) continue;
      if (xs[m] > xs[i]) neg ^= 1u << i;
      if (!mul(P[i], xs[m] > xs[i] ? xs[m] - xs[i] : xs[i] - xs[m], &P[i])) return fail(DN_ERR_UNSUPPORTED, wide);
    }
    if (!mul(D / gcd(D, P[i]), P[i], &D)) return fail(DN_ERR_UNSUPPORTED, wide);
  }
  memset(out, 0, sizeof(*out));
  out->k = k;
  out->r = r;
  out->neg = neg;
  for (int i = 0; i < k; ++i) {
    u128 c = D / P[i], xp = 1;
    for (int j = 0; j < r; ++j) {
      if (j > 0 && (!mul(c, xs[i], &c) || !mul(xp, xs[i], &xp))) return fail(DN_ERR_UNSUPPORTED, wide);
      if (c >> 63) return fail(DN_ERR_UNSUPPORTED, "dn_m521_check_plan: a weight of 2^63 or more");
      if (c >= kCheckMaxC)
        return fail(DN_ERR_UNSUPPORTED, "dn_m521_check_plan: a weight of 2^32 or more (the kernel's one-limb bound)");
      out->c[j][i] = static_cast<uint64_t>(c);
      out->xp[j][i] = static_cast<uint32_t>(xp);  // x_i^j <= c[j][i] < 2^32
    }
  }
  return DN_OK;
}

// What the device entry point requires of a plan it did not build.
inline bool check_plan_wellformed(const dn_m521_check_plan_t& p) {
  if (p.k < 2 || p.k > DN_MAX_RESOLVE || p.r < 1 || p.r > DN_M521_CHECK_MAX_R || p.r >= p.k) return false;
  for (int j = 0; j < p.r; ++j)
    for (int i = 0; i < p.k; ++i)
      if (p.c[j][i] == 0 || p.c[j][i] >= kCheckMaxC || p.xp[j][i] == 0) return false;
  return true;
}

}  // namespace dn
