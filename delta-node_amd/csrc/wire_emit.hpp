// wire_emit.hpp — the sending side of the share wire codec (device): record
// lengths, one record's y laid into its wave's LDS window, the window written
// out, and the one-workgroup scan of block totals that turns lengths into
// byte positions.  encode_kernel (codec_m521.hip) and encode_many_kernel
// (codec_many.hip) build their records through these functions; the frame
// opener (codec_frame.hip) shares the scan.
//
// One wave = 64 consecutive elements = one contiguous run of records, bytes
// [A, B) of the wire.  Each lane lays its record into the wave's LDS window at
// its final byte position (mod 4, or mod 16 on the wide path, like the
// destination); the window then goes out as aligned chunks wholly inside
// [A, B) plus head / tail bytes, so global writes stay contiguous and wide and
// a neighbouring wave's bytes are never touched.
#pragma once

#include <hip/hip_runtime.h>

#include "m521_device.hpp"
#include "wire_geom.hpp"

namespace dn {

// Bytes of the minimal big-endian form of a non-zero 32-bit limb.
__device__ __forceinline__ uint32_t limb_bytes(uint32_t l) { return (32u - __builtin_clz(l) + 7u) / 8u; }

// Minimal big-endian byte length of a canonical 17-limb value (0 -> 0).
__device__ __forceinline__ uint32_t y_len(const uint32_t v[kLimbs]) {
  uint32_t len = 0;
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) {
    if (v[i]) len = 4u * i + limb_bytes(v[i]);
  }
  return len;
}

__device__ __forceinline__ void lds_put_bytes(uint8_t* sb, int32_t lo, int32_t hi, int32_t pos, uint32_t word) {
  // bytes of `word` (LE at LDS position pos) that fall inside [lo, hi)
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (pos + i >= lo && pos + i < hi) sb[pos + i] = static_cast<uint8_t>(word >> (8 * i));
}

// y's minimal big-endian bytes (ylen = y_len(v) of them, not 0) into window
// bytes [ys, ys + ylen) of the row sw.  They are the tail of the 68-byte
// big-endian image W_0..W_16 (W_m = bswap(limb 16 - m)) ending at the record
// end E, so with r = (68 - E) mod 4 every destination dword is one
// v_alignbyte of two neighbouring W words (static indices): dwords wholly
// inside [ys, E) go out as ds_write_b32, the two partial edge dwords byte by
// byte.
__device__ __forceinline__ void lay_y(uint32_t* sw, int32_t ys, int32_t ylen, const uint32_t v[kLimbs]) {
  uint8_t* sb = reinterpret_cast<uint8_t*>(sw);
  const int32_t E = ys + ylen;
  uint32_t W[kLimbs + 1];
#pragma unroll
  for (int m = 0; m < kLimbs; ++m) W[m] = __builtin_bswap32(v[kLimbs - 1 - m]);
  W[kLimbs] = 0u;
  const int32_t base = E - 4 * kLimbs;  // LDS position of image byte 0
  const uint32_t r = static_cast<uint32_t>(-base) & 3u;
  const int32_t d0 = (base + static_cast<int32_t>(r)) >> 2;  // dword holding image bytes r..r+3
  // dword d0 - 1: image bytes 0..r-1 at its top (r > 0)
  if (r) lds_put_bytes(sb, ys, E, 4 * (d0 - 1), __builtin_amdgcn_alignbyte(W[0], 0u, r));
#pragma unroll
  for (int m = 0; m < kLimbs; ++m) {
    const uint32_t u = __builtin_amdgcn_alignbyte(W[m + 1], W[m], r);
    const int32_t pos = 4 * (d0 + m);
    if (pos >= ys && pos + 4 <= E) sw[d0 + m] = u;
    else if (pos + 4 > ys && pos < E) lds_put_bytes(sb, ys, E, pos, u);
  }
}

// The wave's window (LDS byte 0 = wire byte A4) out to wire bytes [A, B) once
// every lane has laid its record: head bytes [A, a4), aligned body [a4, b4),
// tail [b4, B).  w16: `out` is 16-B aligned and A4 is the 16-B boundary at or
// below A, so the body goes out as 16-B stores (else 4-B ones from the 4-B
// boundary).
__device__ __forceinline__ void flush_window(const uint32_t* sw, uint8_t* __restrict__ out, uint64_t A, uint64_t B,
                                             uint64_t A4, bool w16, uint32_t lane) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(sw);
  lds_order();
  const uint64_t al = w16 ? 16u : 4u;
  const uint64_t a4 = (A + al - 1) & ~(al - 1), b4 = B & ~(al - 1);
  if (a4 > b4) {  // the whole range sits inside one aligned chunk
    for (uint64_t q = A + lane; q < B; q += 64) out[q] = sb[q - A4];
    return;
  }
  if (lane < a4 - A) out[A + lane] = sb[A + lane - A4];
  if (lane < B - b4) out[b4 + lane] = sb[b4 + lane - A4];
  if (w16) {
    const u32x4* sq = reinterpret_cast<const u32x4*>(sw);
    u32x4* oq = reinterpret_cast<u32x4*>(out + a4);
    const uint32_t base_q = static_cast<uint32_t>((a4 - A4) / 16);
    const uint32_t nq = static_cast<uint32_t>((b4 - a4) / 16);
    for (uint32_t q = lane; q < nq; q += 64) __builtin_nontemporal_store(sq[base_q + q], oq + q);
  } else {
    uint32_t* ow = reinterpret_cast<uint32_t*>(out + a4);
    const uint32_t base_w = static_cast<uint32_t>((a4 - A4) / 4);
    const uint32_t nw = static_cast<uint32_t>((b4 - a4) / 4);
    for (uint32_t q = lane; q < nw; q += 64) __builtin_nontemporal_store(sw[base_w + q], ow + q);
  }
}

// Exclusive scan of the nb block totals tot[] in place by one workgroup of
// kScanThreads threads; returns the grand total (in every thread).  The totals
// are staged in LDS as 32-bit words (a block's total fits: at most 4096 * 255
// bytes) with coalesced loads, each thread scans a contiguous run of them
// (padded rows: no bank conflicts), the run sums are scanned across threads in
// 64 bits.
constexpr uint32_t scan_slot(uint32_t i) { return i + i / kScanRun; }  // LDS word of a pass's total i
__device__ __forceinline__ uint64_t scan_block_totals(uint64_t* tot, uint64_t nb) {
  __shared__ uint32_t s[kScanLdsWords];
  __shared__ uint64_t s_w[kScanThreads / 64];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  uint64_t carry = 0;  // total of the previous passes
  const uint64_t passes = scan_passes(nb);
  for (uint64_t p = 0; p < passes; ++p) {
    const uint64_t base = p * kScanStage;
    const uint32_t m = scan_count(nb, p);
    for (uint32_t i = t; i < m; i += kScanThreads) s[scan_slot(i)] = static_cast<uint32_t>(tot[base + i]);
    __syncthreads();
    // thread t: totals kScanRun t .. kScanRun t + kScanRun - 1 of this pass
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanRun; ++j) {
      const uint32_t i = kScanRun * t + j;
      sum += i < m ? s[scan_slot(i)] : 0u;
    }
    uint64_t inc = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint64_t v = __shfl_up(inc, d);
      if (lane >= static_cast<uint32_t>(d)) inc += v;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint64_t wbase = 0, ptot = 0;
#pragma unroll
    for (int w = 0; w < static_cast<int>(kScanThreads / 64); ++w) {
      wbase += (w < static_cast<int>(wv)) ? s_w[w] : 0u;
      ptot += s_w[w];
    }
    uint64_t run = carry + wbase + inc - sum;
#pragma unroll
    for (uint32_t j = 0; j < kScanRun; ++j) {
      const uint32_t i = kScanRun * t + j;
      if (i < m) {
        const uint32_t v = s[scan_slot(i)];
        tot[base + i] = run;
        run += v;
      }
    }
    carry += ptot;
    __syncthreads();
  }
  return carry;
}

}  // namespace dn
