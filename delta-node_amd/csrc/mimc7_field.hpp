// mimc7_field.hpp — the BN254 field arithmetic of the MiMC7 kernels
// (mimc7_bn254.hip): 9 x 29-bit-limb Montgomery products with lazy round
// sums, the hash round and chain step, and the double -> field conversion.
//
// Shared by the kernels and by a host program that rehearses the same text
// against Python integers under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/host/mimc7_field_check.cpp), so that a
// change to this arithmetic is checked before it reaches a GPU.  Plain C++:
// no HIP header.
#pragma once

#include <math.h>
#include <stdint.h>

#include <cstring>

#include "mimc7_consts.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_MIMC_HD __host__ __device__ inline
#else
#define DN_MIMC_HD inline
#endif

namespace dn {
namespace mimc {

constexpr int L = 8;

constexpr int N = 9;                 // 29-bit limbs of the Montgomery form
constexpr uint32_t kM29 = (1u << 29) - 1;

struct Consts {
  uint32_t q[L];             // 32-bit limbs (float_to_field)
  uint32_t half_q[L];        // floor(q / 2), 32-bit limbs
  uint32_t q29[N];           // q, 29-bit limbs
  uint32_t qinv;             // -q^{-1} mod 2^29
  uint32_t r2[N];            // R^2 mod q, R = 2^261
  uint32_t cts[kRounds][N];  // round constants, Montgomery form
};

// ---- 256-bit helpers (host + device) ----
DN_MIMC_HD bool geq(const uint32_t a[L], const uint32_t b[L]) {
  for (int i = L - 1; i >= 0; --i) {
    if (a[i] != b[i]) return a[i] > b[i];
  }
  return true;
}

DN_MIMC_HD uint32_t sub_in(uint32_t a[L], const uint32_t b[L]) {  // a -= b, returns borrow
  uint64_t br = 0;
  for (int i = 0; i < L; ++i) {
    const uint64_t d = static_cast<uint64_t>(a[i]) - b[i] - br;
    a[i] = static_cast<uint32_t>(d);
    br = (d >> 63) & 1u;
  }
  return static_cast<uint32_t>(br);
}

DN_MIMC_HD uint32_t add_in(uint32_t a[L], const uint32_t b[L]) {  // a += b, returns carry
  uint64_t c = 0;
  for (int i = 0; i < L; ++i) {
    c += static_cast<uint64_t>(a[i]) + b[i];
    a[i] = static_cast<uint32_t>(c);
    c >>= 32;
  }
  return static_cast<uint32_t>(c);
}

// a = (a + b) mod q for a, b < q (q < 2^254 so a + b < 2^255: no carry out).
DN_MIMC_HD void addmod(uint32_t a[L], const uint32_t b[L], const uint32_t q[L]) {
  add_in(a, b);
  if (geq(a, q)) sub_in(a, q);
}

// ---- 29-bit limb form (host + device) ----
DN_MIMC_HD void to29(const uint32_t a[L], uint32_t o[N]) {
  for (int i = 0; i < N; ++i) {
    const int bit = 29 * i, w = bit / 32, sh = bit % 32;
    const uint64_t lo = a[w], hi = w + 1 < L ? a[w + 1] : 0u;
    o[i] = static_cast<uint32_t>(((hi << 32) | lo) >> sh) & kM29;
  }
}

DN_MIMC_HD void from29(const uint32_t o[N], uint32_t a[L]) {
  uint64_t acc = 0;
  int nb = 0, w = 0;
  for (int i = 0; i < N; ++i) {
    acc |= static_cast<uint64_t>(o[i]) << nb;
    nb += 29;
    while (nb >= 32 && w < L) {
      a[w++] = static_cast<uint32_t>(acc);
      acc >>= 32;
      nb -= 32;
    }
  }
  while (w < L) {
    a[w++] = static_cast<uint32_t>(acc);
    acc >>= 32;
  }
}

DN_MIMC_HD bool geq29(const uint32_t a[N], const uint32_t b[N]) {
  for (int i = N - 1; i >= 0; --i)
    if (a[i] != b[i]) return a[i] > b[i];
  return true;
}

DN_MIMC_HD void sub29_in(uint32_t a[N], const uint32_t b[N]) {  // a -= b (a >= b)
  uint32_t br = 0;
  for (int i = 0; i < N; ++i) {
    const uint32_t d = a[i] - b[i] - br;  // in (-2^30, 2^29)
    br = d >> 31;
    a[i] = d & kM29;
  }
}

// carries of limbs up to 2^32 - 1 into their neighbours (the value fits 9 limbs)
DN_MIMC_HD void norm29(uint32_t a[N]) {
  uint32_t c = 0;
  for (int i = 0; i < N; ++i) {
    const uint32_t v = a[i] + c;
    a[i] = v & kM29;
    c = v >> 29;
  }
}

// a = (a + b) mod q for a, b < q
DN_MIMC_HD void addmod29(uint32_t a[N], const uint32_t b[N], const uint32_t q[N]) {
  for (int i = 0; i < N; ++i) a[i] += b[i];
  norm29(a);
  if (geq29(a, q)) sub29_in(a, q);
}

// Montgomery product r = a b R^{-1} mod q for a, b < 3 q (normalized limbs),
// r < q.  Columns T[i + j] accumulate a_i b_j and m_i q_j (at most 18 products
// of < 2^58 plus a carry < 2^35: below 2^63).
DN_MIMC_HD void mont_mul(uint32_t r[N], const uint32_t a[N], const uint32_t b[N], const Consts& k) {
  uint64_t T[2 * N];
#pragma unroll
  for (int i = 0; i < 2 * N; ++i) T[i] = 0;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) T[i + j] += static_cast<uint64_t>(a[i]) * b[j];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t m = (static_cast<uint32_t>(T[i]) * k.qinv) & kM29;
#pragma unroll
    for (int j = 0; j < N; ++j) T[i + j] += static_cast<uint64_t>(m) * k.q29[j];
    T[i + 1] += T[i] >> 29;  // the low 29 bits of T[i] are now zero
  }
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint64_t v = T[N + i] + c;
    r[i] = static_cast<uint32_t>(v) & kM29;
    c = v >> 29;
  }
  if (geq29(r, k.q29)) sub29_in(r, k.q29);
}

// Montgomery square r = a^2 R^{-1} mod q (same bounds as mont_mul): the 36
// off-diagonal products once, against the doubled limb 2 a_j < 2^30 (each
// column still sums at most 9 products' worth, < 2^59 apiece for the doubled
// ones), plus the 9 squares — 45 instead of 81 multiply-adds before the
// reduction.
DN_MIMC_HD void mont_sqr(uint32_t r[N], const uint32_t a[N], const Consts& k) {
  uint64_t T[2 * N];
  uint32_t a2[N];
#pragma unroll
  for (int i = 0; i < N; ++i) a2[i] = a[i] << 1;
#pragma unroll
  for (int i = 0; i < 2 * N; ++i) T[i] = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    T[2 * i] += static_cast<uint64_t>(a[i]) * a[i];
#pragma unroll
    for (int j = i + 1; j < N; ++j) T[i + j] += static_cast<uint64_t>(a[i]) * a2[j];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t m = (static_cast<uint32_t>(T[i]) * k.qinv) & kM29;
#pragma unroll
    for (int j = 0; j < N; ++j) T[i + j] += static_cast<uint64_t>(m) * k.q29[j];
    T[i + 1] += T[i] >> 29;
  }
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint64_t v = T[N + i] + c;
    r[i] = static_cast<uint32_t>(v) & kM29;
    c = v >> 29;
  }
  if (geq29(r, k.q29)) sub29_in(r, k.q29);
}

// plain 32-bit limbs (< q) -> Montgomery form, and back (canonical)
DN_MIMC_HD void to_mont(uint32_t r[N], const uint32_t a[L], const Consts& k) {
  uint32_t a29[N];
  to29(a, a29);
  mont_mul(r, a29, k.r2, k);
}

DN_MIMC_HD void from_mont(uint32_t r[L], const uint32_t a[N], const Consts& k) {
  uint32_t one[N] = {1, 0, 0, 0, 0, 0, 0, 0, 0}, t[N];
  mont_mul(t, a, one, k);
  from29(t, r);
}

// mimc7_hash in Montgomery form: (r_13 + k) mod q in `out` (Montgomery).
DN_MIMC_HD void hash_m(uint32_t out[N], const uint32_t x[N], const uint32_t key[N], const Consts& k) {
  uint32_t r[N];
  for (int i = 0; i < N; ++i) r[i] = x[i];
  for (int c = 0; c < kRounds; ++c) {
    uint32_t t[N];
    for (int i = 0; i < N; ++i) t[i] = r[i] + key[i] + k.cts[c][i];  // < 3 q: not reduced
    norm29(t);
    // t^7 = t^4 t^3: depth 3 (t^2; t^4 and t^3 independent; their product)
    uint32_t t2[N], t3[N], t4[N];
    mont_sqr(t2, t, k);
    mont_sqr(t4, t2, k);
    mont_mul(t3, t2, t, k);
    mont_mul(r, t4, t3, k);
  }
  for (int i = 0; i < N; ++i) out[i] = r[i];
  addmod29(out, key, k.q29);
}

// One chain step of mimc7_hash_arr: r <- (r + x + mimc7_hash(x, r)) mod q.
DN_MIMC_HD void arr_step(uint32_t r[N], const uint32_t x[N], const Consts& k) {
  uint32_t h[N];
  hash_m(h, x, r, k);
  addmod29(r, x, k.q29);
  addmod29(r, h, k.q29);
}

// _float2mpz: field value (plain, < q) of min(a, q - a), a = int(v * 10^p);
// returns false if |v * 10^p| >= 2^253 (not handled on the device).
DN_MIMC_HD bool float_to_field(double v, double scale, uint32_t out[L], const Consts& k) {
  const double y = v * scale;  // the reference's float multiply
  for (int i = 0; i < L; ++i) out[i] = 0;
  if (y != y) return false;
  const double ay = y < 0 ? -y : y;
  if (!(ay < 14474011154664524427946373126085988481658748083205070504932198000989141204992.0))  // 2^253
    return false;
  // exact integer part of |y| as 8 limbs: mantissa * 2^e
  int e;
  const double m = frexp(ay, &e);  // ay = m 2^e, m in [0.5, 1)
  if (e <= 0) return true;         // |a| = 0
  uint64_t mant = static_cast<uint64_t>(ldexp(m, 53));  // 53-bit integer, ay = mant 2^(e-53)
  int sh = e - 53;
  if (sh < 0) {
    mant >>= -sh;  // truncation toward zero (int())
    sh = 0;
  }
  const int limb = sh / 32, bit = sh % 32;
  const unsigned __int128 wide = static_cast<unsigned __int128>(mant) << bit;  // < 2^117
  // out[limb + d] = word d of wide (d < 4), by select: a dynamic index into
  // out would put the array in scratch memory
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const int d = i - limb;
    out[i] = d >= 0 && d < 4 ? static_cast<uint32_t>(wide >> (32 * d)) : 0u;
  }
  const bool neg = y < 0;
  // a = +-out.  min(a, q - a): negative a -> a (value q - |a|); a > q/2 -> q - a.
  if (neg) {
    bool zero = true;
    for (int i = 0; i < L; ++i) zero &= out[i] == 0;
    if (!zero) {
      uint32_t t[L];
      for (int i = 0; i < L; ++i) t[i] = k.q[i];
      sub_in(t, out);
      for (int i = 0; i < L; ++i) out[i] = t[i];
    }
  } else if (!geq(k.half_q, out)) {  // a > floor(q/2)  <=>  a > q - a
    uint32_t t[L];
    for (int i = 0; i < L; ++i) t[i] = k.q[i];
    sub_in(t, out);
    for (int i = 0; i < L; ++i) out[i] = t[i];
  }
  return true;
}

// ---- host: constants ----
inline void make_consts(Consts& k) {
  const uint32_t* q = kQ32;
  std::memcpy(k.q, q, sizeof(k.q));
  to29(q, k.q29);
  // qinv = -q^{-1} mod 2^29 (Newton mod 2^32, then the low 29 bits)
  uint32_t inv = q[0];
  for (int i = 0; i < 5; ++i) inv *= 2u - q[0] * inv;
  k.qinv = (0u - inv) & kM29;
  // R^2 mod q, R = 2^261: double 1 (mod q) 522 times
  uint32_t v[L] = {1, 0, 0, 0, 0, 0, 0, 0};
  for (int it = 0; it < 2 * 29 * N; ++it) {
    uint32_t t[L];
    std::memcpy(t, v, sizeof(t));
    addmod(v, t, q);
  }
  to29(v, k.r2);
  // floor(q / 2)
  for (int i = 0; i < L; ++i) k.half_q[i] = (q[i] >> 1) | (i + 1 < L ? (q[i + 1] << 31) : 0u);
}

}  // namespace mimc
}  // namespace dn
