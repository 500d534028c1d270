// opcheck_ops.hpp — the operation table of the device-header suite (test
// infrastructure: part of lib/libdn_opcheck.so and of tests/host/opcheck_host.cpp,
// never of libdn_shamir.so).
//
// run_op(op, in, out) runs ONE case of one operation of m521_device.hpp /
// chacha_device.hpp, calling the header's functions the way the kernels do,
// on a fixed-width record of u32 words; tests/device_ops.py builds the
// records and holds the expected values.  The caller pre-fills `out` (the
// memory operations store into a 256-element tile that lies at the start of
// their out record, and the bytes they must leave alone are checked).
//
// Records (u32 words, little-endian limbs; a field element is 17 words):
//   op                in                                   out
//   kAddSmall         v[17] s                              v[17]
//   kFold/kReduce/kCanon  v[17]                            v[17]
//   kAddFe            v[17] u[17]                          v[17]
//   kTwice            c[17]                                D[17] (D != c)  D[17] (D aliasing c)
//   kMulSmallAdd      src[17] x c[17]                      v[17] (4-arg)   v[17] (in place, v = src)
//   kMemBuffer        v[17] w                              tile  load_fe_b[17]
//   kMemGlobal        v[17] w                              tile  load_fe[17] load_fe_cached[17]
//   kStoreReduced     D[17] w                              tile  D after[17]  load_fe_b[17]
//   kStoreReducedAt   D[17] w                              tile  D after[17]  load_fe_b[17]
//   kFd2..kFd7        c[7][17] n w xs[kFdEmit]             tile  share[kFdEmit][17]  D[7][17]
//   kMac1/2/17        rows  (a[17] y[17])[16]              S[34]  r[17]
//   kMulmod           x[17] c[17]                          r[17]
//   kRotr             v[17] e                              v[17]
//   kModSmall         x_lo x_hi d recip_lo recip_hi        r
//   kExactDiv         r[17] d d_inv32 p_inv_d recip_lo recip_hi w[17]   r[17]
//   kChachaBlock      key[8] n0 n1 rounds ctr_lo ctr_hi    x[16]
//   kPrngRejected     v[17]                                flag
//   kPrngRetry        key[8] n0 n1 rounds i_lo i_hi v[17]  v[17] (after the + 1 of prng_coeffs_of)
#pragma once

#include "chacha_device.hpp"
#include "m521_device.hpp"

namespace dn {
namespace opcheck {

enum Op : int32_t {
  kAddSmall = 0, kFold, kReduce, kCanon, kAddFe, kTwice, kMulSmallAdd,
  kMemBuffer, kMemGlobal, kStoreReduced, kStoreReducedAt,
  kFd2, kFd3, kFd4, kFd5, kFd6, kFd7,
  kMac1, kMac2, kMac17, kMulmod, kRotr, kModSmall, kExactDiv,
  kChachaBlock, kPrngRejected, kPrngRetry, kOpCount
};

constexpr int kTileWords = static_cast<int>(kTileBytes / 4);  // 4224
constexpr int kFdEmit = 70;     // abscissas whose share an fd case emits
constexpr int kFdMaxT = 7;
constexpr int kMacRows = 16;    // DN_MAX_RESOLVE
constexpr int kWideWords = 2 * kLimbs;

// words of one case's in / out record (0: no such op)
__host__ __device__ constexpr int in_words(int op) {
  switch (op) {
    case kAddSmall: return kLimbs + 1;
    case kFold: case kReduce: case kCanon: case kTwice: case kPrngRejected: return kLimbs;
    case kAddFe: case kMulmod: return 2 * kLimbs;
    case kMulSmallAdd: return 2 * kLimbs + 1;
    case kMemBuffer: case kMemGlobal: case kStoreReduced: case kStoreReducedAt: case kRotr: return kLimbs + 1;
    case kFd2: case kFd3: case kFd4: case kFd5: case kFd6: case kFd7: return kFdMaxT * kLimbs + 2 + kFdEmit;
    case kMac1: case kMac2: case kMac17: return 1 + kMacRows * 2 * kLimbs;
    case kModSmall: return 5;
    case kExactDiv: return 2 * kLimbs + 5;
    case kChachaBlock: return 13;
    case kPrngRetry: return 13 + kLimbs;
    default: return 0;
  }
}
__host__ __device__ constexpr int out_words(int op) {
  switch (op) {
    case kAddSmall: case kFold: case kReduce: case kCanon: case kAddFe: case kMulmod: case kRotr: case kExactDiv:
    case kPrngRetry: return kLimbs;
    case kTwice: case kMulSmallAdd: return 2 * kLimbs;
    case kMemBuffer: return kTileWords + kLimbs;
    case kMemGlobal: case kStoreReduced: case kStoreReducedAt: return kTileWords + 2 * kLimbs;
    case kFd2: case kFd3: case kFd4: case kFd5: case kFd6: case kFd7:
      return kTileWords + kFdEmit * kLimbs + kFdMaxT * kLimbs;
    case kMac1: case kMac2: case kMac17: return kWideWords + kLimbs;
    case kModSmall: case kPrngRejected: return 1;
    case kChachaBlock: return 16;
    default: return 0;
  }
}

__device__ __forceinline__ void get_fe(uint32_t v[kLimbs], const uint32_t* in) {
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) v[i] = in[i];
}
__device__ __forceinline__ void put_fe(uint32_t* out, const uint32_t v[kLimbs]) {
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) out[i] = v[i];
}
__device__ __forceinline__ uint64_t get_u64(const uint32_t* in) {
  return static_cast<uint64_t>(in[0]) | (static_cast<uint64_t>(in[1]) << 32);
}
__device__ __forceinline__ void get_key(ChachaKey& K, const uint32_t* in) {
#pragma unroll
  for (int i = 0; i < 8; ++i) K.k[i] = in[i];
  K.n0 = in[8];
  K.n1 = in[9];
  K.rounds = in[10] > 20u ? 20 : static_cast<int32_t>(in[10]);  // (a bad record must not spin a lane)
  K.pad = 0;
}

// The split's share loop (shamir_m521.hip split_body, !FOLD): fd_init, then
// per share store_reduced of D[0] followed by fd_step, every step 1..n.  The
// share of step x is read back from the tile when x is the next listed
// abscissa (xs ascending, 0 = unused).
template <int T>
__device__ __forceinline__ void run_fd(const uint32_t* in, uint32_t* out) {
  uint32_t D[T][kLimbs];
#pragma unroll
  for (int k = 0; k < T; ++k) get_fe(D[k], in + k * kLimbs);
  uint32_t n = in[kFdMaxT * kLimbs];
  if (n > 65535u) n = 65535u;
  const uint32_t w = in[kFdMaxT * kLimbs + 1] & 255u;
  const uint32_t* xs = in + kFdMaxT * kLimbs + 2;
  const rsrc_t r = tile_rsrc(reinterpret_cast<const uint8_t*>(out));
  uint32_t* shares = out + kTileWords;
  fd_init<T>(D);
  uint32_t e = 0u;
#pragma unroll 1
  for (uint32_t x = 1u; x <= n; ++x) {
    store_reduced(r, w, D[0]);
    if (e < static_cast<uint32_t>(kFdEmit) && xs[e] == x) {
      uint32_t v[kLimbs];
      load_fe_b(r, w, v);
      put_fe(shares + e * kLimbs, v);
      ++e;
    }
    fd_step<T>(D);
  }
#pragma unroll
  for (int k = 0; k < T; ++k) put_fe(out + kTileWords + (kFdEmit + k) * kLimbs, D[k]);
}

// The reconstruct's accumulation (shamir_m521.hip recon_rows / the runtime-k
// loop): S = sum_i a_i * y_i over A + 17 limbs, then recon_finish's
// reduce_wide with the kernels' value bound.
template <int A>
__device__ __forceinline__ void run_mac(const uint32_t* in, uint32_t* out) {
  constexpr int N = A + kLimbs;
  constexpr int VB = (A == kLimbs) ? 1046 : (521 + 32 * A + 4);
  uint32_t S[N];
#pragma unroll
  for (int i = 0; i < N; ++i) S[i] = 0u;
  uint32_t rows = in[0];
  if (rows > static_cast<uint32_t>(kMacRows)) rows = kMacRows;
#pragma unroll 1
  for (uint32_t i = 0; i < rows; ++i) {
    uint32_t a[A], y[kLimbs];
#pragma unroll
    for (int j = 0; j < A; ++j) a[j] = in[1 + i * 2 * kLimbs + j];
    get_fe(y, in + 1 + i * 2 * kLimbs + kLimbs);
    mac_wide<N, A>(S, a, y);
  }
#pragma unroll
  for (int i = 0; i < kWideWords; ++i) out[i] = i < N ? S[i] : 0u;
  uint32_t r[kLimbs];
  reduce_wide<N, VB>(S, r);
  put_fe(out + kWideWords, r);
}

__device__ inline void run_op(int32_t op, const uint32_t* in, uint32_t* out) {
  uint32_t v[kLimbs], u[kLimbs];
  switch (op) {
    case kAddSmall:
      get_fe(v, in);
      add_small(v, in[kLimbs]);
      put_fe(out, v);
      break;
    case kFold:
      get_fe(v, in);
      fold(v);
      put_fe(out, v);
      break;
    case kReduce:
      get_fe(v, in);
      reduce(v);
      put_fe(out, v);
      break;
    case kCanon:
      get_fe(v, in);
      canon(v);
      put_fe(out, v);
      break;
    case kAddFe:
      get_fe(v, in);
      get_fe(u, in + kLimbs);
      add_fe(v, u);
      put_fe(out, v);
      break;
    case kTwice:
      get_fe(u, in);
      twice(v, u);
      put_fe(out, v);
      twice(u, u);
      put_fe(out + kLimbs, u);
      break;
    case kMulSmallAdd: {
      uint32_t c[kLimbs];
      get_fe(u, in);
      get_fe(c, in + kLimbs + 1);
      mul_small_add(v, u, in[kLimbs], c);
      put_fe(out, v);
      mul_small_add(u, in[kLimbs], c);
      put_fe(out + kLimbs, u);
      break;
    }
    case kMemBuffer: {
      const uint32_t w = in[kLimbs] & 255u;
      const rsrc_t r = tile_rsrc(reinterpret_cast<const uint8_t*>(out));
      get_fe(v, in);
      store_fe_b(r, w, v);
      load_fe_b(r, w, u);
      put_fe(out + kTileWords, u);
      break;
    }
    case kMemGlobal: {
      const uint32_t w = in[kLimbs] & 255u;
      uint8_t* tb = reinterpret_cast<uint8_t*>(out);
      get_fe(v, in);
      store_fe(tb, w, v);
      load_fe(tb, w, u);
      put_fe(out + kTileWords, u);
      load_fe_cached(tb, w, u);
      put_fe(out + kTileWords + kLimbs, u);
      break;
    }
    case kStoreReduced:
    case kStoreReducedAt: {
      const uint32_t w = in[kLimbs] & 255u;
      const rsrc_t r = tile_rsrc(reinterpret_cast<const uint8_t*>(out));
      get_fe(v, in);
      if (op == kStoreReduced) store_reduced(r, w, v);
      else store_reduced_at(r, w * 4u, w * 2u, v);
      put_fe(out + kTileWords, v);
      load_fe_b(r, w, u);
      put_fe(out + kTileWords + kLimbs, u);
      break;
    }
    case kFd2: run_fd<2>(in, out); break;
    case kFd3: run_fd<3>(in, out); break;
    case kFd4: run_fd<4>(in, out); break;
    case kFd5: run_fd<5>(in, out); break;
    case kFd6: run_fd<6>(in, out); break;
    case kFd7: run_fd<7>(in, out); break;
    case kMac1: run_mac<1>(in, out); break;
    case kMac2: run_mac<2>(in, out); break;
    case kMac17: run_mac<kLimbs>(in, out); break;
    case kMulmod:
      get_fe(u, in);
      get_fe(v, in + kLimbs);
      {
        uint32_t r[kLimbs];
        mulmod(r, u, v);
        put_fe(out, r);
      }
      break;
    case kRotr: {
      uint32_t e = in[kLimbs];
      e = e < 1u ? 1u : e > 31u ? 31u : e;
      get_fe(v, in);
      rotr521(v, e);
      put_fe(out, v);
      break;
    }
    case kModSmall:
      out[0] = mod_small(get_u64(in), in[2], get_u64(in + 3));
      break;
    case kExactDiv:
      get_fe(v, in);
      get_fe(u, in + kLimbs + 5);
      exact_div_small(v, in[kLimbs], in[kLimbs + 1], in[kLimbs + 2], get_u64(in + kLimbs + 3), u);
      put_fe(out, v);
      break;
    case kChachaBlock: {
      ChachaKey K;
      get_key(K, in);
      uint32_t x[16];
      chacha_block(x, K, get_u64(in + 11));
#pragma unroll
      for (int i = 0; i < 16; ++i) out[i] = x[i];
      break;
    }
    case kPrngRejected:
      get_fe(v, in);
      out[0] = prng_rejected(v) ? 1u : 0u;
      break;
    case kPrngRetry: {
      ChachaKey K;
      get_key(K, in);
      get_fe(v, in + 13);
      prng_retry(v, K, get_u64(in + 11));
      add_small(v, 1u);
      put_fe(out, v);
      break;
    }
    default:
      break;
  }
}

}  // namespace opcheck
}  // namespace dn
