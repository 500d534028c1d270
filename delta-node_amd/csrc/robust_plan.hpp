// robust_plan.hpp — the integers of a robust reconstruct (dn_m521_robust_plan;
// the kernel is share_robust.hip, the arithmetic it runs robust_core.hpp;
// DESIGN.md §4.28).
//
// On top of check_plan.hpp's parity-check weights w_i (the plan is built by
// check_plan_build itself: one validation, its codes, messages and order) the
// plan holds the Lagrange weights at 0 of ALL k abscissas over their least
// common denominator, lambda_m = A_m / D_all, and per candidate i the constants
// of the one exact division a corrected element ends with:
//   f(0) = (w_i T - A_i S_0) / (w_i D_all),   T = sum_m A_m y_m,
// and of the division by D_all alone that every other element ends with.  For
// positive abscissas sign(A_m) = (-1)^(k-1) sign(w_m): the kernel accumulates
// sum_m |A_m| (+-y_m) with the syndromes' own per-share negation and negates
// the quotient when k is even, so the plan keeps magnitudes only.
//
// Bounds: |A_m| < 2^32 (kCheckMaxC: T is one more chain of check_mac, below
// 2^557 for k <= 16) and every divisor's odd part below 2^16 (one
// exact_div_small; its power of two is a rotation).  128-bit exact arithmetic as
// check_plan.hpp; whatever leaves it is unsupported.  Plain C++: no HIP header.
#pragma once

#include "check_plan.hpp"

namespace dn {

constexpr uint32_t kRobustMaxD = 1u << 16;
constexpr int kRobustAll = DN_MAX_RESOLVE;  // div[kRobustAll]: D_all alone

namespace robust_detail {
using check_detail::u128;

// a^{-1} mod m for gcd(a, m) = 1, m < 2^32.
inline uint32_t inv_mod(uint64_t a, uint64_t m) {
  int64_t t0 = 0, t1 = 1;
  uint64_t r0 = m, r1 = a % m;
  while (r1) {
    const uint64_t q = r0 / r1, r2 = r0 - q * r1;
    const int64_t t2 = t0 - static_cast<int64_t>(q) * t1;
    r0 = r1, r1 = r2, t0 = t1, t1 = t2;
  }
  return static_cast<uint32_t>(t0 < 0 ? t0 + static_cast<int64_t>(m) : t0);
}

// v = d 2^shift, d odd -> *out; false when d >= kRobustMaxD.
inline bool div_small(u128 v, dn_m521_div_small_t* out) {
  memset(out, 0, sizeof(*out));
  while ((v & 1) == 0) {
    v >>= 1;
    ++out->shift;
  }
  if (v >= kRobustMaxD) return false;
  const uint32_t d = out->d = static_cast<uint32_t>(v);
  if (d == 1) return true;
  uint32_t inv32 = d;  // Newton: x <- x (2 - d x), 5 steps from 3 correct bits
  for (int it = 0; it < 5; ++it) inv32 *= 2u - d * inv32;
  out->d_inv32 = inv32;
  uint64_t pw = 1;  // 2^521 mod d, then p mod d
  for (int b = 0; b < 521; ++b) pw = (pw * 2) % d;
  out->p_inv_d = inv_mod((pw + d - 1) % d, d);  // (p is prime and d < p: invertible)
  out->d_recip = UINT64_MAX / d;
  uint64_t wv = 1;
  for (int l = 0; l < DN_M521_LIMBS; ++l) {
    out->w[l] = static_cast<uint32_t>(wv);
    wv = (wv << 32) % d;
  }
  return true;
}
}  // namespace robust_detail

// Fills *out and returns DN_OK, or a DN_ERR_* code with the reason in why[why_len].
inline int robust_plan_build(const uint64_t* xs, int k, int threshold, dn_m521_robust_plan_t* out, char* why,
                             size_t why_len) {
  using namespace check_detail;
  auto fail = [&](int code, const char* msg) {
    snprintf(why, why_len, "%s", msg);
    return code;
  };
  if (!out) return fail(DN_ERR_ARG, "dn_m521_check_plan: null pointer");
  dn_m521_check_plan_t check;
  const int rc = check_plan_build(xs, k, threshold, &check, why, why_len);
  if (rc != DN_OK) return rc;
  if (check.r == 1)
    return fail(DN_ERR_UNSUPPORTED, "dn_m521_robust_plan: one spare share detects only: nothing to correct with");
  const char* wide = "dn_m521_robust_plan: the Lagrange weights of these abscissas leave 128 bits";
  // lambda_m = num_m / den_m in lowest terms, num_m = prod_{j != m} x_j, den_m = prod_{j != m} |x_j - x_m|
  u128 num[DN_MAX_RESOLVE], den[DN_MAX_RESOLVE], D = 1;
  for (int m = 0; m < k; ++m) {
    num[m] = den[m] = 1;
    for (int j = 0; j < k; ++j) {
      if (j == m) continue;
      if (!mul(num[m], xs[j], &num[m]) ||
          !mul(den[m], xs[j] > xs[m] ? xs[j] - xs[m] : xs[m] - xs[j], &den[m]))
        return fail(DN_ERR_UNSUPPORTED, wide);
    }
    const u128 g = gcd(num[m], den[m]);
    num[m] /= g;
    den[m] /= g;
    if (!mul(D / gcd(D, den[m]), den[m], &D)) return fail(DN_ERR_UNSUPPORTED, wide);
  }
  memset(out, 0, sizeof(*out));
  out->check = check;
  out->negate = (k & 1) ? 0u : 1u;
  for (int m = 0; m < k; ++m) {
    u128 a;
    if (!mul(num[m], D / den[m], &a)) return fail(DN_ERR_UNSUPPORTED, wide);
    if (a >= kCheckMaxC)
      return fail(DN_ERR_UNSUPPORTED,
                  "dn_m521_robust_plan: a Lagrange weight of 2^32 or more (the kernel's one-limb bound)");
    out->a[m] = static_cast<uint32_t>(a);
  }
  const char* big = "dn_m521_robust_plan: a divisor with an odd part of 2^16 or more (one exact division)";
  if (!robust_detail::div_small(D, &out->div[kRobustAll])) return fail(DN_ERR_UNSUPPORTED, big);
  for (int i = 0; i < k; ++i) {
    u128 v;
    if (!mul(D, check.c[0][i], &v)) return fail(DN_ERR_UNSUPPORTED, wide);
    if (!robust_detail::div_small(v, &out->div[i])) return fail(DN_ERR_UNSUPPORTED, big);
  }
  return DN_OK;
}

// What the pair test and the pair correction (robust_pair.hpp) ask of the abscissas:
// per pair, x_i + x_j and x_i x_j below 2^32 (one-limb multipliers) and an odd part of |x_j - x_i| below
// 2^16 (the one division whose constants the kernel computes itself).  (Behind check_plan_build at
// r = 4 none of them can fire, x_i^3 <= c[3][i] < 2^32 being the stronger bound; they are stated and
// checked on their own so that the finish does not lean on a bound made for something else.)
inline int robust_pair_bounds(const uint64_t* xs, int k, char* why, size_t why_len) {
  auto fail = [&](const char* msg) {
    snprintf(why, why_len, "%s", msg);
    return DN_ERR_UNSUPPORTED;
  };
  for (int j = 1; j < k; ++j)
    for (int i = 0; i < j; ++i) {
      if (xs[i] >= kCheckMaxC || xs[j] >= kCheckMaxC || xs[i] + xs[j] >= kCheckMaxC || xs[i] * xs[j] >= kCheckMaxC)
        return fail("dn_m521_robust_plan2: x_i + x_j or x_i x_j of 2^32 or more (the pair test's one-limb bound)");
      uint64_t d = xs[j] > xs[i] ? xs[j] - xs[i] : xs[i] - xs[j];
      while (d && (d & 1) == 0) d >>= 1;
      if (d >= kRobustMaxD)
        return fail("dn_m521_robust_plan2: a difference x_j - x_i with an odd part of 2^16 or more (one exact division)");
    }
  return DN_OK;
}

// robust_plan_build for `errors` bad shares per element (dn_m521_robust_plan2).  errors == 1 is
// robust_plan_build; errors == 2 also needs r == 4 and robust_pair_bounds, and records the mode in
// out->max_errors.
inline int robust_plan_build2(const uint64_t* xs, int k, int threshold, int errors, dn_m521_robust_plan_t* out,
                              char* why, size_t why_len) {
  auto fail = [&](int code, const char* msg) {
    snprintf(why, why_len, "%s", msg);
    return code;
  };
  if (errors != 1 && errors != 2) return fail(DN_ERR_ARG, "dn_m521_robust_plan2: errors must be 1 or 2");
  int rc = robust_plan_build(xs, k, threshold, out, why, why_len);
  if (rc != DN_OK || errors == 1) return rc;
  if (out->check.r != 4)
    return fail(DN_ERR_UNSUPPORTED,
                "dn_m521_robust_plan2: two errors per element need exactly four spare shares (k == threshold + 4)");
  if ((rc = robust_pair_bounds(xs, k, why, why_len)) != DN_OK) return rc;
  out->max_errors = 2u;
  return DN_OK;
}

// What the device entry point requires of a plan it did not build.
inline bool robust_plan_wellformed(const dn_m521_robust_plan_t& p) {
  if (!check_plan_wellformed(p.check) || p.check.r < 2 || p.negate > 1u) return false;
  if (p.max_errors > 2u || (p.max_errors == 2u && p.check.r != 4)) return false;
  for (int i = 0; i <= DN_MAX_RESOLVE; ++i) {
    if (i >= p.check.k && i != kRobustAll) continue;
    const dn_m521_div_small_t& q = p.div[i];
    if ((q.d & 1u) == 0 || q.d >= kRobustMaxD || q.shift >= 521u) return false;
    if (q.d > 1u && (q.d * q.d_inv32 != 1u || q.p_inv_d >= q.d || q.d_recip != UINT64_MAX / q.d)) return false;
    for (int l = 0; l < DN_M521_LIMBS; ++l)
      if (q.d > 1u && q.w[l] >= q.d) return false;
  }
  for (int i = 0; i < p.check.k; ++i)
    if (p.a[i] == 0) return false;
  return true;
}

}  // namespace dn
