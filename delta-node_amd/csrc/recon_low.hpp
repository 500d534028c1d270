// recon_low.hpp — the low 64 bits of a reconstruct from the five limbs they
// depend on (reconstruct_low_kernel, shamir_m521.hip).
//
// For one-limb weights and d = 1 (lambda_i = +-a_i / 2^e, e <= 31) the full
// path computes S = sum_i a_i Y_i (Y_i = y_i, or ~y_i within 521 bits where
// the weight is negative), R = S mod p, r = rotr521(R, e), out = r mod 2^64.
// With S = q p + R = q 2^521 + (R - q):
//   L = sum_i a_i (Y_i mod 2^96)  mod 2^96      limbs 0..2
//   V = sum_i a_i (Y_i >> 480)                  limb 15 | hi << 32 (41 bits)
//   q = (V + A + 1) >> 41,  A = sum_i a_i       = floor(S / p)
//   out = (((L + q) mod 2^96) >> e) mod 2^64    (e + 64 <= 95)
// V + u = floor(S / 2^480) = q 2^41 + h for the carry 0 <= u < A out of the
// low 480 bits and h = floor((R - q) / 2^480) in [-1, 2^41), so the shift
// yields q for every R < p - (A + 2) 2^480; and L == R - q (mod 2^96) whether
// R >= q or not, because 2^521 == 0 there.  Exact for every result below
// 2^480; results within (A + 2) 2^480 of p are outside the contract.
//
// One function, host and device: tools/recon_low_check.cpp runs on the CPU
// exactly the code the kernel runs.  Plain C++: no HIP header.
#pragma once

#include <stdint.h>

#include "seg_plan.hpp"

namespace dn {

constexpr int kLowPlanes = 5;           // limbs read per share row
constexpr int kLowTopLimb = 15;         // y[3]: limb 15; y[4]: the 9-bit hi
constexpr uint32_t kLowTopMask = 0x1FFu;

// y[i] = {limb 0, limb 1, limb 2, limb 15, hi} of share i's element (hi is
// masked here, as load_fe masks it); a[i] = |a_i|; asum = sum_i a[i] < 2^24.
template <int K>
DN_SEG_HD uint64_t recon_low_word(const uint32_t (&y)[K][kLowPlanes], const uint32_t (&a)[K], uint32_t neg,
                                  uint32_t shift, uint32_t asum) {
  uint32_t l0 = 0u, l1 = 0u, l2 = 0u;  // L
  uint32_t v0 = 0u, v1 = 0u, v2 = 0u;  // V (< 2^65)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < K; ++i) {
    const bool n = (neg >> i) & 1u;
    const uint32_t y0 = n ? ~y[i][0] : y[i][0], y1 = n ? ~y[i][1] : y[i][1], y2 = n ? ~y[i][2] : y[i][2];
    const uint32_t t15 = n ? ~y[i][3] : y[i][3];
    const uint32_t hi = (n ? ~y[i][4] : y[i][4]) & kLowTopMask;
    const uint32_t ai = a[i];
    uint64_t t = static_cast<uint64_t>(ai) * y0 + l0;
    l0 = static_cast<uint32_t>(t);
    t = static_cast<uint64_t>(ai) * y1 + (static_cast<uint64_t>(l1) + (t >> 32));
    l1 = static_cast<uint32_t>(t);
    l2 += ai * y2 + static_cast<uint32_t>(t >> 32);
    t = static_cast<uint64_t>(ai) * t15 + v0;
    v0 = static_cast<uint32_t>(t);
    t = static_cast<uint64_t>(ai) * hi + (static_cast<uint64_t>(v1) + (t >> 32));
    v1 = static_cast<uint32_t>(t);
    v2 += static_cast<uint32_t>(t >> 32);
  }
  // q = (V + A + 1) >> 41  (< 2^25)
  uint64_t t = static_cast<uint64_t>(v0) + asum + 1u;
  t = static_cast<uint64_t>(v1) + (t >> 32);
  v1 = static_cast<uint32_t>(t);
  v2 += static_cast<uint32_t>(t >> 32);
  const uint32_t q = (v1 >> 9) | (v2 << 23);
  // L + q mod 2^96
  t = static_cast<uint64_t>(l0) + q;
  l0 = static_cast<uint32_t>(t);
  t = static_cast<uint64_t>(l1) + (t >> 32);
  l1 = static_cast<uint32_t>(t);
  l2 += static_cast<uint32_t>(t >> 32);
  const uint64_t lo = static_cast<uint64_t>(l0) | (static_cast<uint64_t>(l1) << 32);
  return shift ? (lo >> shift) | (static_cast<uint64_t>(l2) << (64u - shift)) : lo;
}

}  // namespace dn
