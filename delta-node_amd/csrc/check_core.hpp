// check_core.hpp — the per-element arithmetic of the share consistency check
// (check_kernel, share_check.hip), mod p = 2^521 - 1.
//
// A syndrome S_j = sum_i c[j][i] * Y_i is kept UNREDUCED in 18 u32 limbs,
// carries propagated: Y_i is share i's 521-bit value y, or ~y within 521 bits
// (= p - y == -y) where the weight is negative, as the reconstruct negates;
// c < 2^32 (check_plan.hpp kCheckMaxC), so one limb step is a single
// 32 x 32 + 64 -> 64 bit multiply-add and k <= 16 terms stay below 2^557.
// After the last share:
//   fold   v = (S mod 2^521) + (S >> 521)  == S (mod p),  v < 2^521 + 2^55;
//   zero   v == 0 (mod p)  iff  v is 0 or exactly p — and p is the usual one:
//          S = q p with q >= 1 folds to (2^521 - q) + (q - 1) = p, while limbs
//          all 0 need every Y_i = 0;
//   culprit  share i explains the element iff S_0 != 0 and, for j = 1 .. r-1,
//          S_j - x_i^j S_0 == 0: with N = p - canon(S_0) the value
//          v_j + x_i^j * N (< 2^554, the same 18 limbs and the same
//          multiply-add) folds to 0 or p.
//
// One text, host and device: tests/host/check_core_check.cpp runs on the CPU
// exactly what the kernel runs.  Plain C++: no HIP header.
#pragma once

#include <stdint.h>

#include "seg_plan.hpp"

// The limb and syndrome loops are unrolled in device code (they index
// registers); the loop over candidate shares stays a loop.
#if defined(__HIP_DEVICE_COMPILE__)
#define DN_CHK_UNROLL _Pragma("unroll")
#define DN_CHK_ROLLED _Pragma("unroll 1")
#else
#define DN_CHK_UNROLL
#define DN_CHK_ROLLED
#endif

namespace dn {

constexpr int kChkLimbs = 17;               // a field element
constexpr int kChkAcc = 18;                 // an unreduced syndrome
constexpr uint32_t kChkTop = 0x1FFu;        // bits 512..520 live in limb 16
constexpr uint8_t kChkConsistent = 0xFFu;   // the culprit byte of a consistent element
constexpr uint8_t kChkUnexplained = 0xFEu;  // inconsistent, and no single share explains it

// a + b + cin (cin 0 or 1), carry out in *cout.  The one primitive with two
// spellings: device code names the add-with-carry (from the 64-bit sum the
// compiler builds each limb's add out of zero-extended register pairs, twice
// the registers), the host compilers need not know that builtin.
DN_SEG_HD uint32_t check_addc(uint32_t a, uint32_t b, uint32_t cin, uint32_t* cout) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned co;
  const uint32_t r = __builtin_addc(a, b, cin, &co);
  *cout = co;
  return r;
#else
  const uint64_t s = static_cast<uint64_t>(a) + b + cin;
  *cout = static_cast<uint32_t>(s >> 32);
  return static_cast<uint32_t>(s);
#endif
}

// S[j] += c[j] * Y for j < R, Y = y ^ sign within 521 bits (sign 0 or all
// ones; bits 9.. of y[16] are ignored: the top plane is masked here, where it
// is consumed).  The R carry chains are independent and interleaved limb by
// limb.  The caller keeps every S[j] below 2^576.
template <int R>
DN_SEG_HD void check_mac(uint32_t (&S)[R][kChkAcc], const uint32_t (&y)[kChkLimbs], const uint32_t (&c)[R],
                         uint32_t sign) {
  // The product limbs come from a multiply-add chain whose addend is the
  // previous high word alone, and a separate add-with-carry chain brings them
  // into S (m521_device.hpp mul_small_add: an addend formed from S costs a
  // zero-extended register pair per limb).
  uint32_t hi[R], cc[R];
  DN_CHK_UNROLL
  for (int j = 0; j < R; ++j) hi[j] = cc[j] = 0u;
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) {
    const uint32_t yl = l < 16 ? (y[l] ^ sign) : ((y[16] ^ sign) & kChkTop);
    DN_CHK_UNROLL
    for (int j = 0; j < R; ++j) {
      const uint64_t t = static_cast<uint64_t>(c[j]) * yl + hi[j];
      hi[j] = static_cast<uint32_t>(t >> 32);
      S[j][l] = check_addc(S[j][l], static_cast<uint32_t>(t), cc[j], &cc[j]);
    }
  }
  DN_CHK_UNROLL
  for (int j = 0; j < R; ++j) S[j][kChkLimbs] += hi[j] + cc[j];
}

// v = (S mod 2^521) + (S >> 521): v == S (mod p) and v < 2^521 + 2^55 < 2^522.
DN_SEG_HD void check_fold(const uint32_t (&S)[kChkAcc], uint32_t (&v)[kChkLimbs]) {
  const uint32_t h0 = (S[16] >> 9) | (S[17] << 23), h1 = S[17] >> 9;
  uint32_t cc;
  v[0] = check_addc(S[0], h0, 0u, &cc);
  v[1] = check_addc(S[1], h1, cc, &cc);
  DN_CHK_UNROLL
  for (int l = 2; l < kChkLimbs; ++l) v[l] = check_addc(l < 16 ? S[l] : (S[16] & kChkTop), 0u, cc, &cc);
}

// v (< 2^522) == 0 (mod p): all limbs 0, or exactly p.
DN_SEG_HD bool check_is_zero(const uint32_t (&v)[kChkLimbs]) {
  uint32_t all = v[0], any = v[0];
  DN_CHK_UNROLL
  for (int l = 1; l < 16; ++l) {
    all &= v[l];
    any |= v[l];
  }
  return ((any | v[16]) == 0u) || (all == 0xFFFFFFFFu && v[16] == kChkTop);
}

// v (< 2^522) -> its canonical residue in [0, p): bit 521 comes back in at
// bit 0 (v - 2^521 < 2^55, so the sum stays below 2^521), then p -> 0.
DN_SEG_HD void check_canon(uint32_t (&v)[kChkLimbs]) {
  const uint32_t top = v[16] >> 9;
  v[16] &= kChkTop;
  uint32_t cc;
  v[0] = check_addc(v[0], top, 0u, &cc);
  DN_CHK_UNROLL
  for (int l = 1; l < kChkLimbs; ++l) v[l] = check_addc(v[l], 0u, cc, &cc);
  if (check_is_zero(v)) {
    DN_CHK_UNROLL
    for (int l = 0; l < kChkLimbs; ++l) v[l] = 0u;
  }
}

// vj - xp * S_0 == 0 (mod p), given vj (< 2^522) and n0 = canon(S_0), which
// check_mac negates (sign all ones: p - n0).
DN_SEG_HD bool check_explains(const uint32_t (&vj)[kChkLimbs], const uint32_t (&n0)[kChkLimbs], uint32_t xp) {
  uint32_t T[1][kChkAcc];
  DN_CHK_UNROLL
  for (int l = 0; l < kChkLimbs; ++l) T[0][l] = vj[l];
  T[0][kChkLimbs] = 0u;
  const uint32_t c[1] = {xp};
  check_mac<1>(T, n0, c, 0xFFFFFFFFu);
  uint32_t v[kChkLimbs];
  check_fold(T[0], v);
  return check_is_zero(v);
}

// The culprit byte of one element from its R finished syndromes: consistent,
// the index i of the one share with S_j == xp(j, i) * S_0 for every j >= 1
// (xp(j, i) = x_i^j), or unexplained.
template <int R, typename Xp>
DN_SEG_HD uint8_t check_verdict(uint32_t (&S)[R][kChkAcc], int k, Xp xp) {
  uint32_t v[R][kChkLimbs];
  bool zero[R], consistent = true;
  DN_CHK_UNROLL
  for (int j = 0; j < R; ++j) {
    check_fold(S[j], v[j]);
    zero[j] = check_is_zero(v[j]);
    consistent = consistent && zero[j];
  }
  if (consistent) return kChkConsistent;
  if (R == 1 || zero[0]) return kChkUnexplained;
  check_canon(v[0]);
  DN_CHK_ROLLED
  for (int i = 0; i < k; ++i) {
    bool ok = true;
    DN_CHK_UNROLL
    for (int j = 1; j < R; ++j) ok = ok && check_explains(v[j], v[0], xp(j, i));
    if (ok) return static_cast<uint8_t>(i);
  }
  return kChkUnexplained;
}

// Whether an element is consistent, from its R finished syndromes (the form
// without a culprit output: no candidate loop).
template <int R>
DN_SEG_HD bool check_consistent(const uint32_t (&S)[R][kChkAcc]) {
  bool consistent = true;
  DN_CHK_UNROLL
  for (int j = 0; j < R; ++j) {
    uint32_t v[kChkLimbs];
    check_fold(S[j], v);
    consistent = consistent && check_is_zero(v);
  }
  return consistent;
}

}  // namespace dn
