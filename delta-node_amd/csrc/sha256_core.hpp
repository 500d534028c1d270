// sha256_core.hpp — the SHA-256 arithmetic of the share commitment kernel
// (commit_sha256.hip): the round constants, the compression of one block with
// a rolling 16-word schedule, the block count of a message and the rule that
// turns "the dword at record byte p" into a padded message word (FIPS 180-4
// §5.1.1, §6.2).
//
// Shared by the kernel and by a host program that rehearses the same text
// against hashlib under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/host/sha256_check.cpp), so that the padding and the schedule are
// checked before they reach a GPU.  Plain C++: no HIP header.  Written so
// that the gfx950 compiler selects v_alignbit for the rotations, v_bitop3 for
// the three-input functions and v_add3 for the sums; nothing here multiplies.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_SHA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DN_SHA_HD inline __attribute__((always_inline))
#endif

namespace dn {
namespace sha {

DN_SHA_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
// The three-input functions.  Left to itself the gfx950 compiler builds each
// from two or three two-input instructions; it is told the v_bitop3 truth
// table here (a = 0xF0, b = 0xCC, c = 0xAA).
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
#define DN_SHA_OP3(a, b, c, table, plain) __builtin_amdgcn_bitop3_b32(a, b, c, table)
#else
#define DN_SHA_OP3(a, b, c, table, plain) (plain)
#endif
DN_SHA_HD uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return DN_SHA_OP3(a, b, c, 0x96, a ^ b ^ c); }
DN_SHA_HD uint32_t ch(uint32_t e, uint32_t f, uint32_t g) { return DN_SHA_OP3(e, f, g, 0xCA, (e & f) ^ (~e & g)); }
DN_SHA_HD uint32_t maj(uint32_t a, uint32_t b, uint32_t c) {
  return DN_SHA_OP3(a, b, c, 0xE8, (a & b) ^ (a & c) ^ (b & c));
}
DN_SHA_HD uint32_t big_sigma0(uint32_t x) { return xor3(rotr(x, 2), rotr(x, 13), rotr(x, 22)); }
DN_SHA_HD uint32_t big_sigma1(uint32_t x) { return xor3(rotr(x, 6), rotr(x, 11), rotr(x, 25)); }
DN_SHA_HD uint32_t small_sigma0(uint32_t x) { return xor3(rotr(x, 7), rotr(x, 18), x >> 3); }
DN_SHA_HD uint32_t small_sigma1(uint32_t x) { return xor3(rotr(x, 17), rotr(x, 19), x >> 10); }

// H(0) of FIPS 180-4 §5.3.3
DN_SHA_HD void init(uint32_t s[8]) {
  s[0] = 0x6a09e667u;
  s[1] = 0xbb67ae85u;
  s[2] = 0x3c6ef372u;
  s[3] = 0xa54ff53au;
  s[4] = 0x510e527fu;
  s[5] = 0x9b05688cu;
  s[6] = 0x1f83d9abu;
  s[7] = 0x5be0cd19u;
}

// One block: s += compression(s, w).  w holds the block's 16 message words on
// entry and is used up as the rolling schedule (word t lives in w[t & 15]).
// Fully unrolled: every index is a constant, so s and w stay in registers.
DN_SHA_HD void compress(uint32_t s[8], uint32_t w[16]) {
  static constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t a = s[0], b = s[1], c = s[2], d = s[3], e = s[4], f = s[5], g = s[6], h = s[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16)
      w[t & 15] += small_sigma1(w[(t - 2) & 15]) + w[(t - 7) & 15] + small_sigma0(w[(t - 15) & 15]);
    const uint32_t t1 = h + big_sigma1(e) + ch(e, f, g) + K[t] + w[t & 15];
    const uint32_t t2 = big_sigma0(a) + maj(a, b, c);
    h = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  s[0] += a;
  s[1] += b;
  s[2] += c;
  s[3] += d;
  s[4] += e;
  s[5] += f;
  s[6] += g;
  s[7] += h;
}

// Blocks of a len-byte message: its bytes, the 0x80 byte and the 8 length bytes.
DN_SHA_HD uint64_t blocks_of(uint64_t len) { return (len + 9 + 63) / 64; }

// The bytes of the record at and after block b's first byte, held to
// [-8, 64] (64: the block is all record; below 0 only in a last block that
// holds nothing but padding).  b < blocks_of(len).
DN_SHA_HD int32_t block_rest(uint64_t len, uint64_t b) {
  const int64_t rest = static_cast<int64_t>(len - 64 * b);
  return static_cast<int32_t>(rest > 64 ? 64 : rest);
}

// Message word from `raw`, the big-endian dword at a record byte p of which r
// bytes belong to the record (r = len - p; any value below 0 or above 4 says
// what 0 / 4 say, except that the 0x80 byte sits at r == 0 alone): the bytes
// at or past the record's end are masked off and 0x80 goes at byte len.
// Branch-free: two selects.
DN_SHA_HD uint32_t pad_word(uint32_t raw, int32_t r) {
  const uint32_t sh = 8u * (static_cast<uint32_t>(r) & 3u);
  const uint32_t keep = r >= 4 ? 0xFFFFFFFFu : (r <= 0 ? 0u : ~(0xFFFFFFFFu >> sh));
  const uint32_t mark = (r >= 0 && r < 4) ? (0x80000000u >> sh) : 0u;
  return (raw & keep) | mark;
}

// Block b of a len-byte record into w: get(p) is the big-endian dword at
// record byte p (p = 64 b + 4 j; whatever it returns for bytes at or past len
// is masked off, but it must be safe to call), last says b == blocks_of(len) - 1:
// words 14 and 15 of that block are the bit length.
template <class Get>
DN_SHA_HD void load_block(uint32_t w[16], Get get, uint64_t len, uint64_t b, bool last) {
  const int32_t rest = block_rest(len, b);
#pragma unroll
  for (int j = 0; j < 16; ++j) w[j] = pad_word(get(64 * b + 4 * j), rest - 4 * j);
  // (there both words are zero so far: len + 1 <= 64 b + 56)
  const uint64_t bits = len << 3;
  w[14] = last ? static_cast<uint32_t>(bits >> 32) : w[14];
  w[15] = last ? static_cast<uint32_t>(bits) : w[15];
}

// The digest of a whole message through the functions above (the host
// program's path, and the byte-serial shape of the kernel's): out[8], word i
// the big-endian dword at digest byte 4 i.
template <class Get>
DN_SHA_HD void digest(uint32_t out[8], Get get, uint64_t len) {
  init(out);
  const uint64_t nb = blocks_of(len);
  for (uint64_t b = 0; b < nb; ++b) {
    uint32_t w[16];
    load_block(w, get, len, b, b + 1 == nb);
    compress(out, w);
  }
}

}  // namespace sha
}  // namespace dn
