// robust_core.hpp — the per-element finish of the robust reconstruct
// (robust_kernel, share_robust.hip), mod p = 2^521 - 1.
//
// check_mac<R + 1> has accumulated, unreduced in 18 limbs each, the R syndromes
// S_0 .. S_{R-1} and, as chain R, T' = sum_m |A_m| Y_m with the syndromes' own
// per-share negation: T' == (-1)^(k-1) T, T = sum_m A_m y_m (robust_plan.hpp).
// The verdict is check_verdict's on the first R chains.  Then
//   consistent or unexplained   f = canon(T') / D_all;
//   share i located             N = |w_i| canon(T') + |A_i| (p - canon(S_0))
//                               (< 2^554: the same 18 limbs, the same
//                               multiply-add), f = canon(N) / (|w_i| D_all);
//   k even                      f = p - f;
//   shares i < j located        (two errors, r = 4) robust_pair.hpp, where the
//                               signs are derived the same way: A_l / w_l =
//                               (-1)^(k-1) |A_l| / |w_l|, and the sign of
//                               x_j - x_i decides whether f gains or loses.
// A division by d 2^e, d odd and below 2^16, is exact_div_small's (add the m p
// that makes the value divisible by d, m = -r p^{-1} mod d; divide limb by
// limb from the low end with d^{-1} mod 2^32; the quotient is canonical) and a
// right rotation of the 521-bit string by e (2^521 == 1), here in the portable
// spelling: m521_device.hpp's names device builtins.
//
// One text, host and device: tests/host/robust_core_check.cpp runs on the CPU
// exactly what the kernel runs.  Plain C++: no HIP header.
#pragma once

#include "check_core.hpp"
#include "dn_shamir.h"

namespace dn {

// x mod d for d < 2^32, recip = floor((2^64-1)/d) (Barrett: the estimate is low by at most one).
DN_SEG_HD uint32_t robust_mod_small(uint64_t x, uint32_t d, uint64_t recip) {
  const uint64_t q = static_cast<uint64_t>((static_cast<unsigned __int128>(x) * recip) >> 64);
  uint64_t r = x - q * d;
  if (r >= d) r -= d;
  return static_cast<uint32_t>(r);
}

// v / q.d mod p for canonical v and odd 3 <= q.d < 2^16 (m521_device.hpp exact_div_small).
DN_SEG_HD void robust_exact_div(uint32_t (&v)[kChkLimbs], const dn_m521_div_small_t& q) {
  uint64_t acc = 0;
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) acc += static_cast<uint64_t>(v[l]) * q.w[l];  // < 17 * 2^48
  const uint32_t rm = robust_mod_small(acc, q.d, q.d_recip);
  const uint32_t m = robust_mod_small(static_cast<uint64_t>(rm ? q.d - rm : 0u) * q.p_inv_d, q.d, q.d_recip);
  // u = v + m p = v - m + m 2^521 (the borrow chain as an add of ~0 limbs: v - m = v + ~m + 1 - 2^544)
  v[16] += m << 9;
  uint32_t cc;
  v[0] = check_addc(v[0], ~m, 1u, &cc);
  DN_CHK_UNROLL
  for (int l = 1; l < kChkLimbs; ++l) v[l] = check_addc(v[l], 0xFFFFFFFFu, cc, &cc);
  // u / d, exact, low limb first (GMP's divexact_1): q_l = (u_l - borrow) d^{-1} mod 2^32, borrow = hi(q_l d)
  uint32_t b = 0u;
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) {
    const uint32_t s = v[l], x = s - b;
    const uint32_t ql = x * q.d_inv32;
    b = static_cast<uint32_t>((static_cast<uint64_t>(ql) * q.d) >> 32) + (x > s ? 1u : 0u);
    v[l] = ql;
  }
}

// v / 2^e mod p for canonical v, 1 <= e <= 31: the 521-bit string rotated right (canonical again).
DN_SEG_HD void robust_rotr(uint32_t (&v)[kChkLimbs], uint32_t e) {
  const uint32_t low = v[0] & ((1u << e) - 1u);
  DN_CHK_UNROLL
  for (int l = 0; l < 16; ++l) v[l] = (v[l] >> e) | (v[l + 1] << (32u - e));
  v[16] >>= e;
  if (e <= 9u) {
    v[16] |= low << (9u - e);
  } else {
    v[15] |= low << (41u - e);
    v[16] |= low >> (e - 9u);
  }
}

// canonical v -> +-v / (q.d 2^q.shift) mod p, canonical; negate: 0 or 1.
DN_SEG_HD void robust_divide(uint32_t (&v)[kChkLimbs], const dn_m521_div_small_t& q, uint32_t negate) {
  if (q.d > 1u) robust_exact_div(v, q);
  DN_CHK_ROLLED
  for (uint32_t e = q.shift; e != 0u;) {
    const uint32_t s = e > 31u ? 31u : e;
    robust_rotr(v, s);
    e -= s;
  }
  if (negate) {  // p - v: the complement within 521 bits, and 0 stays 0
    uint32_t any = v[16];
    DN_CHK_UNROLL
    for (int l = 0; l < 16; ++l) any |= v[l];
    if (any != 0u) {
      DN_CHK_UNROLL
      for (int l = 0; l < 16; ++l) v[l] = ~v[l];
      v[16] = ~v[16] & kChkTop;
    }
  }
}

// The result of an element without a located share: f = +-canon(T') / D_all.
DN_SEG_HD void robust_plain(const uint32_t (&T)[kChkAcc], const dn_m521_div_small_t& all, uint32_t negate,
                            uint32_t (&f)[kChkLimbs]) {
  check_fold(T, f);
  check_canon(f);
  robust_divide(f, all, negate);
}

// The result of an element whose share i is located: w = |w_i|, a = |A_i|, q the constants of |w_i| D_all.
DN_SEG_HD void robust_located(const uint32_t (&S0)[kChkAcc], const uint32_t (&T)[kChkAcc], uint32_t w, uint32_t a,
                              const dn_m521_div_small_t& q, uint32_t negate, uint32_t (&f)[kChkLimbs]) {
  uint32_t n0[kChkLimbs], N[1][kChkAcc];
  check_fold(T, f);
  check_canon(f);
  check_fold(S0, n0);
  check_canon(n0);
  DN_CHK_UNROLL
  for (int l = 0; l < kChkAcc; ++l) N[0][l] = 0u;
  const uint32_t cw[1] = {w}, ca[1] = {a};
  check_mac<1>(N, f, cw, 0u);
  check_mac<1>(N, n0, ca, 0xFFFFFFFFu);
  check_fold(N[0], f);
  check_canon(f);
  robust_divide(f, q, negate);
}

// The first R of the R + 1 chains, as check_verdict takes them.
template <int R>
DN_SEG_HD uint32_t (&robust_syndromes(uint32_t (&S)[R + 1][kChkAcc]))[R][kChkAcc] {
  return *reinterpret_cast<uint32_t(*)[R][kChkAcc]>(&S);
}

}  // namespace dn
