// robust_pair.hpp — the two-error finish of the robust reconstruct
// (robust_kernel, share_robust.hip; robust_records_kernel, robust_records.hip;
// DESIGN.md §4.31), mod p = 2^521 - 1: what an element that no single share
// explains goes through when the plan has four spare shares (r = 4).
//
// The k shares of an element are a Reed-Solomon word of minimum distance
// r + 1 = 5, so two errors are uniquely decodable.  With the signed syndromes
// S_m = sum_l w_l x_l^m y_l, m = 0 .. 3 (what check_mac accumulates, mod p):
//   pair test   errors confined to shares i and j give, for m = 0 and 1,
//                 S_{m+2} - (x_i + x_j) S_{m+1} + x_i x_j S_m == 0:
//               canon(S_{m+2}) + (x_i + x_j) (p - canon(S_{m+1})) + x_i x_j canon(S_m)
//               (< 2^555: the 18 limbs and the multiply-add of check_explains)
//               folds to 0 or p.  Run after the single-share test has failed,
//               at most one pair passes and both its errors are non-zero: two
//               passing pairs would differ by a code word of weight <= 4.
//   correction  delta = x_j - x_i,
//                 U_i = x_j S_0 - S_1 = w_i delta e_i,
//                 U_j = S_1 - x_i S_0 = w_j delta e_j,
//                 f(0) = T / D_all - A_i U_i / (w_i D_all delta)
//                                  - A_j U_j / (w_j D_all delta).
//   signs       the plan keeps magnitudes.  As in robust_located, T = nu T' with
//               nu = (-1)^(k-1) and A_l = nu sign(w_l) |A_l|, so A_l / w_l =
//               nu |A_l| / |w_l|: the sign of w (check.neg) enters through the
//               accumulation alone (U is formed from the signed syndromes) and
//                 f(0) = nu [ T' / D_all - sign(delta) X / |delta| ],
//                 X = |A_i| U_i / (|w_i| D_all) + |A_j| U_j / (|w_j| D_all),
//               every quotient taken with the plan's negation (nu = -1 for
//               even k), so f = (nu T'/D_all) -+ (nu X/|delta|) for delta >< 0.
//   divisors    |w_i| D_all, |w_j| D_all and D_all are the plan's div[i], div[j]
//               and div[kRobustAll]; |delta| is the one new divisor, and its
//               constants are computed here, where they are needed
//               (robust_div_consts): nothing is tabulated per pair.
// Every multiplier is one limb: x_i + x_j and x_i x_j by the plan's bound
// (robust_plan.hpp robust_pair_bounds), x and |A| by the existing ones.
//
// The syndromes come canonical from a small window of 4 x 17 words (the wave's
// LDS window on the device, an array on the host): the owner of an element
// writes them once (robust_pair_publish), every lane of the wave reads them to
// test one pair each (robust_pair_wave, device only), the owner corrects.
//
// One text, host and device: tests/host/robust_pair_check.cpp runs on the CPU
// exactly what the kernel runs.  Plain C++ up to robust_pair_wave.
#pragma once

#include "robust_core.hpp"
#if defined(__HIPCC__)
#include "wire_geom.hpp"  // lds_order
#endif

namespace dn {

constexpr int kPairWords = 4 * kChkLimbs;  // the window: canon(S_0) .. canon(S_3)
constexpr uint8_t kPairBase = 16;          // the culprit byte of pair i < j: 16 + j (j - 1) / 2 + i

// Pair number idx = j (j - 1) / 2 + i  ->  i < j.
DN_SEG_HD void robust_pair_of(uint32_t idx, uint32_t* i, uint32_t* j) {
  uint32_t jj = 1;
  DN_CHK_ROLLED
  while ((jj + 1u) * jj / 2u <= idx) ++jj;
  *j = jj;
  *i = idx - jj * (jj - 1u) / 2u;
}

// The constants of a division by v = d 2^shift (1 <= v < 2^32), d odd; false
// (and *q unusable) when d >= 2^16.  What robust_plan.hpp's div_small computes
// on the host, in 32- and 64-bit steps a lane can take: Newton's iteration for
// d^{-1} mod 2^32, the residues 2^(32 l) mod d by repeated reduction, p mod d
// from 2^521 = 2^512 2^9, p^{-1} mod d by Euclid.
DN_SEG_HD bool robust_div_consts(uint32_t v, dn_m521_div_small_t* q) {
  q->shift = 0u;
  DN_CHK_ROLLED
  while ((v & 1u) == 0u) {
    v >>= 1;
    ++q->shift;
  }
  const uint32_t d = q->d = v;
  q->d_inv32 = q->p_inv_d = q->reserved = 0u;
  q->d_recip = 0u;
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) q->w[l] = 0u;
  if (d >= (1u << 16)) return false;
  if (d == 1u) return true;
  uint32_t inv32 = d;  // x <- x (2 - d x): 3 correct bits, then 6, 12, 24, 48
  DN_CHK_UNROLL
  for (int it = 0; it < 5; ++it) inv32 *= 2u - d * inv32;
  q->d_inv32 = inv32;
  const uint64_t recip = q->d_recip = ~0ull / d;
  uint32_t wv = 1u;
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) {
    q->w[l] = wv;
    wv = robust_mod_small(static_cast<uint64_t>(wv) << 32, d, recip);
  }
  const uint32_t t521 = robust_mod_small(static_cast<uint64_t>(q->w[16]) << 9, d, recip);
  const uint32_t pm = t521 ? t521 - 1u : d - 1u;  // p mod d, not 0: p is prime and d < p
  int32_t t0 = 0, t1 = 1;                         // Euclid: |t| <= d < 2^16
  uint32_t r0 = d, r1 = pm;
  DN_CHK_ROLLED
  while (r1 != 0u) {
    const uint32_t qq = r0 / r1, r2 = r0 - qq * r1;
    const int32_t t2 = t0 - static_cast<int32_t>(qq) * t1;
    r0 = r1, r1 = r2, t0 = t1, t1 = t2;
  }
  q->p_inv_d = static_cast<uint32_t>(t0 < 0 ? t0 + static_cast<int32_t>(d) : t0);
  return true;
}

// win[m] = canon(S_m), m = 0 .. 3: the owner's four syndromes into the window.
DN_SEG_HD void robust_pair_publish(const uint32_t (&S)[5][kChkAcc], uint32_t* win) {
  DN_CHK_UNROLL  // (S lives in registers: no run-time index into it)
  for (int m = 0; m < 4; ++m) {
    uint32_t v[kChkLimbs];
    check_fold(S[m], v);
    check_canon(v);
    DN_CHK_UNROLL
    for (int l = 0; l < kChkLimbs; ++l) win[m * kChkLimbs + l] = v[l];
  }
}

// v = s[0 .. 16]
DN_SEG_HD void robust_pair_read(const uint32_t* s, uint32_t (&v)[kChkLimbs]) {
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) v[l] = s[l];
}

// canon(a * A + b * B) for canonical A, B and one-limb a, b; sb all ones takes p - B for B.
DN_SEG_HD void robust_pair_lin(uint32_t a, const uint32_t (&A)[kChkLimbs], uint32_t b, const uint32_t (&B)[kChkLimbs],
                               uint32_t sb, uint32_t (&out)[kChkLimbs]) {
  uint32_t N[1][kChkAcc];
  DN_CHK_UNROLL
  for (int l = 0; l < kChkAcc; ++l) N[0][l] = 0u;
  const uint32_t ca[1] = {a}, cb[1] = {b};
  check_mac<1>(N, A, ca, 0u);
  check_mac<1>(N, B, cb, sb);
  check_fold(N[0], out);
  check_canon(out);
}

// Whether errors in the shares at x_i and x_j alone explain the window's syndromes.
DN_SEG_HD bool robust_pair_test(const uint32_t* win, uint32_t xi, uint32_t xj) {
  const uint32_t sum[1] = {xi + xj}, prod[1] = {xi * xj};  // one limb each: the plan's bound
  bool ok = true;
  DN_CHK_ROLLED
  for (int m = 0; m < 2; ++m) {
    uint32_t N[1][kChkAcc], v[kChkLimbs];
    DN_CHK_UNROLL
    for (int l = 0; l < kChkLimbs; ++l) N[0][l] = win[(m + 2) * kChkLimbs + l];
    N[0][kChkLimbs] = 0u;
    robust_pair_read(win + (m + 1) * kChkLimbs, v);
    check_mac<1>(N, v, sum, 0xFFFFFFFFu);
    robust_pair_read(win + m * kChkLimbs, v);
    check_mac<1>(N, v, prod, 0u);
    check_fold(N[0], v);
    ok = ok && check_is_zero(v);
  }
  return ok;
}

// The result of an element whose shares i < j are located.  f holds, in and
// out, a canonical residue: in, robust_plain's nu T' / D_all; out, f(0).
// wi .. : |A_i|, |A_j| and the constants of |w_i| D_all, |w_j| D_all.
DN_SEG_HD void robust_pair_correct(const uint32_t* win, uint32_t xi, uint32_t xj, uint32_t ai, uint32_t aj,
                                   const dn_m521_div_small_t& qi, const dn_m521_div_small_t& qj, uint32_t negate,
                                   uint32_t (&f)[kChkLimbs]) {
  uint32_t s0[kChkLimbs], s1[kChkLimbs], u[kChkLimbs], X[kChkLimbs], zero[kChkLimbs];
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) zero[l] = 0u;
  robust_pair_read(win, s0);
  robust_pair_read(win + kChkLimbs, s1);
  // |A_i| U_i / (|w_i| D_all), U_i = x_j S_0 - S_1
  robust_pair_lin(xj, s0, 1u, s1, 0xFFFFFFFFu, u);
  robust_pair_lin(ai, u, 0u, zero, 0u, X);
  robust_divide(X, qi, 0u);
  // |A_j| U_j / (|w_j| D_all), U_j = S_1 - x_i S_0
  robust_pair_lin(1u, s1, xi, s0, 0xFFFFFFFFu, u);
  robust_pair_lin(aj, u, 0u, zero, 0u, u);
  robust_divide(u, qj, 0u);
  robust_pair_lin(1u, X, 1u, u, 0u, X);
  // nu X / |delta|, then f -+ it
  dn_m521_div_small_t qd;
  robust_div_consts(xj > xi ? xj - xi : xi - xj, &qd);
  robust_divide(X, qd, negate);
  robust_pair_lin(1u, f, 1u, X, xj > xi ? 0xFFFFFFFFu : 0u, f);
}

#if defined(__HIPCC__)
// The wave-cooperative pair search and correction (device only).  For each
// unexplained element of the wave in turn: its owner publishes the four
// canonical syndromes to `win` (kPairWords words of LDS that only this wave
// touches), every present lane tests one pair per round (36 pairs at k = 9: one
// round; 120 at k = 16: two), a ballot yields the pair, the owner corrects f
// and takes the pair's byte as its verdict.  A wave without an unexplained
// element pays the first ballot alone, and the search's state lives in LDS and
// in registers that are dead outside this rare branch.
// The present lanes must be a prefix of the wave (share_rows.hpp); A has
// RobustArgs' wt, a, div and negate.
template <typename A>
__device__ __forceinline__ void robust_pair_wave(const A& a, uint32_t* win, const uint32_t (&S)[5][kChkAcc],
                                                 uint8_t& verdict, uint32_t (&f)[kChkLimbs]) {
  uint64_t todo = __ballot(verdict == kChkUnexplained);
  if (todo == 0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t present = static_cast<uint32_t>(__popcll(__ballot(true)));
  const uint32_t k = a.wt.k, npairs = k * (k - 1u) / 2u;
#pragma unroll 1
  while (todo != 0ull) {
    const uint32_t owner = static_cast<uint32_t>(__builtin_ctzll(todo));
    todo &= todo - 1ull;
    if (lane == owner) robust_pair_publish(S, win);
    lds_order();
    uint32_t found = npairs;
#pragma unroll 1
    for (uint32_t base = 0; base < npairs && found == npairs; base += present) {
      const uint32_t idx = base + lane;
      bool hit = false;
      if (idx < npairs) {
        uint32_t i, j;
        robust_pair_of(idx, &i, &j);
        hit = robust_pair_test(win, a.wt.xp[1][i], a.wt.xp[1][j]);
      }
      const uint64_t hits = __ballot(hit);
      if (hits != 0ull) found = base + static_cast<uint32_t>(__builtin_ctzll(hits));
    }
    if (found != npairs && lane == owner) {
      uint32_t i, j;
      robust_pair_of(found, &i, &j);
      robust_pair_correct(win, a.wt.xp[1][i], a.wt.xp[1][j], a.a[i], a.a[j], a.div[i], a.div[j], a.negate, f);
      verdict = static_cast<uint8_t>(kPairBase + found);
    }
    lds_order();  // the window is free for the next element
  }
}
#endif

}  // namespace dn
