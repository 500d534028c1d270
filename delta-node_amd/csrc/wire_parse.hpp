// wire_parse.hpp — the receiving side of the share wire codec (device): one
// wave's window of 64 records brought to LDS, and one record parsed from
// untrusted bytes and untrusted offsets.  decode_kernel (codec_m521.hip),
// recon_records.hip and sum_records.hip all parse through these functions, so
// a clamp or a bounds check is fixed here once.
//
// One wave = 64 consecutive records = one contiguous byte window.  The wave
// stages the window in LDS with dword (or 16-byte) loads, then each lane
// rebuilds its limbs from the record's tail: LE limb i is the big-endian dword
// ending 4 i bytes before the record end, i.e. bswap of one v_alignbyte of two
// LDS dwords, masked to the bytes after the y start.  Windows larger than the
// LDS slice (records padded with leading zero bytes) take the byte-serial path.
// y is not reduced here; records whose y has more than 68 significant bytes,
// or whose x is longer than 8 bytes, parse as not ok.
#pragma once

#include <hip/hip_runtime.h>

#include "m521_device.hpp"
#include "wire_geom.hpp"

namespace dn {

typedef const __attribute__((address_space(4))) uint64_t* OffTab;  // read by scalar loads: no kernel writes offsets

// A wave's window of one wire (wave-uniform): records e0 .. eN - 1 are bytes
// [A, Bend), LDS byte 0 is A4 (the 16-B boundary at or below A where the wire
// is 16-B aligned, w16, else the 4-B one), and `lds` says that the window fits
// the LDS slice (else every lane parses its record from global memory).
struct Win {
  uint64_t A, Bend, A4;
  bool lds;
};

// Off: a plain pointer, or OffTab where the offsets may go through scalar loads.
template <typename Off>
__device__ __forceinline__ Win win_of(Off off, uint64_t in_bytes, bool w16, uint64_t e0, uint64_t eN) {
  Win r;
  r.A = off[e0];
  r.Bend = off[eN];
  r.A4 = w16 ? (r.A & ~15ull) : (r.A & ~3ull);
  r.lds = r.Bend >= r.A && r.Bend <= in_bytes && r.Bend - r.A4 <= static_cast<uint64_t>(kWinLimit);
  return r;
}

// A window on its way to LDS: the staging loop cut in two, the loads here and
// the LDS stores in stage_store (same addresses, same bytes as stage_direct).
struct Stage {
  uint32_t r[kStageRegs];
  uint32_t tail;
};

__device__ __forceinline__ void stage_load(Stage& s, const uint8_t* __restrict__ in, const Win& w, bool w16,
                                           uint32_t lane) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  if (w16) {
    const uint64_t B16 = w.Bend & ~15ull;
    const uint32_t nq = static_cast<uint32_t>((B16 - w.A4) / 16);
    const u32x4* inq = reinterpret_cast<const u32x4*>(in + w.A4);
#pragma unroll
    for (int j = 0; j < kStageQ; ++j) {
      const uint32_t q = lane + 64u * j;
      if (q < nq) {
        const u32x4 t = __builtin_nontemporal_load(inq + q);
        s.r[4 * j] = t.x;
        s.r[4 * j + 1] = t.y;
        s.r[4 * j + 2] = t.z;
        s.r[4 * j + 3] = t.w;
      }
    }
    if (lane < w.Bend - B16) s.tail = in[B16 + lane];
  } else {
    const uint64_t B4 = w.Bend & ~3ull;
    const uint32_t nw = static_cast<uint32_t>((B4 - w.A4) / 4);
    const uint32_t* inw = reinterpret_cast<const uint32_t*>(in + w.A4);
#pragma unroll
    for (int j = 0; j < kStageW; ++j) {
      const uint32_t q = lane + 64u * j;
      if (q < nw) s.r[j] = __builtin_nontemporal_load(inw + q);
    }
    if (lane < w.Bend - B4) s.tail = in[B4 + lane];
  }
}

__device__ __forceinline__ void stage_store(const Stage& s, uint32_t* S, const Win& w, bool w16, uint32_t lane) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  uint8_t* sb = reinterpret_cast<uint8_t*>(S);
  if (w16) {
    const uint64_t B16 = w.Bend & ~15ull;
    const uint32_t nq = static_cast<uint32_t>((B16 - w.A4) / 16);
    u32x4* Sq = reinterpret_cast<u32x4*>(S);
#pragma unroll
    for (int j = 0; j < kStageQ; ++j) {
      const uint32_t q = lane + 64u * j;
      if (q < nq) {
        u32x4 t;
        t.x = s.r[4 * j];
        t.y = s.r[4 * j + 1];
        t.z = s.r[4 * j + 2];
        t.w = s.r[4 * j + 3];
        Sq[q] = t;
      }
    }
    if (lane < w.Bend - B16) sb[B16 - w.A4 + lane] = static_cast<uint8_t>(s.tail);
  } else {
    const uint64_t B4 = w.Bend & ~3ull;
    const uint32_t nw = static_cast<uint32_t>((B4 - w.A4) / 4);
#pragma unroll
    for (int j = 0; j < kStageW; ++j) {
      const uint32_t q = lane + 64u * j;
      if (q < nw) S[q] = s.r[j];
    }
    if (lane < w.Bend - B4) sb[B4 - w.A4 + lane] = static_cast<uint8_t>(s.tail);
  }
}

// The staging loop without load-ahead: global -> registers -> LDS inside one
// loop (decode_kernel's form; fewer registers).
__device__ __forceinline__ void stage_direct(uint32_t* S, const uint8_t* __restrict__ in, const Win& w, bool w16,
                                             uint32_t lane) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  uint8_t* sb = reinterpret_cast<uint8_t*>(S);
  if (w16) {
    const uint64_t B16 = w.Bend & ~15ull;
    const uint32_t nq = static_cast<uint32_t>((B16 - w.A4) / 16);
    const u32x4* inq = reinterpret_cast<const u32x4*>(in + w.A4);
    u32x4* Sq = reinterpret_cast<u32x4*>(S);
    for (uint32_t q = lane; q < nq; q += 64) Sq[q] = __builtin_nontemporal_load(inq + q);
    if (lane < w.Bend - B16) sb[B16 - w.A4 + lane] = in[B16 + lane];
  } else {
    const uint64_t B4 = w.Bend & ~3ull;
    const uint32_t nw = static_cast<uint32_t>((B4 - w.A4) / 4);
    const uint32_t* inw = reinterpret_cast<const uint32_t*>(in + w.A4);
    for (uint32_t q = lane; q < nw; q += 64) S[q] = __builtin_nontemporal_load(inw + q);
    if (lane < w.Bend - B4) sb[B4 - w.A4 + lane] = in[B4 + lane];
  }
}

// The byte-serial parse of record [o, end) from global memory; the caller has
// checked o < end <= in_bytes.
__device__ __forceinline__ bool parse_global(const uint8_t* __restrict__ in, uint64_t o, uint64_t end, uint64_t& x,
                                             uint32_t v[kLimbs]) {
  bool ok = end > o;
  const uint32_t xlen = ok ? in[o] : 0u;
  x = 0;
  ok = ok && xlen <= 8 && o + 1 + xlen <= end;
  if (ok)
    for (uint32_t i = 0; i < xlen; ++i) x = (x << 8) | in[o + 1 + i];
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) v[i] = 0u;
  if (ok) {
    const uint64_t y0 = o + 1 + xlen;
    uint64_t skip = 0;  // leading zero bytes are allowed (bytes_to_int ignores them)
    while (y0 + skip < end && in[y0 + skip] == 0) ++skip;
    const uint64_t sig = end - y0 - skip;
    ok = sig <= 68;
    if (ok) {
      for (uint64_t i = 0; i < sig; ++i) {
        const uint32_t byte = in[end - 1 - i];
        v[i >> 2] |= byte << (8 * (i & 3));
      }
    }
  }
  return ok;
}

// The parse of record [oe, ee) from the staged window (S[k] = dword at window
// byte 4 k): v is zero unless the record is good.
__device__ __forceinline__ bool parse_lds(const uint32_t* S, const Win& w, uint64_t oe, uint64_t ee, uint64_t& x,
                                          uint32_t v[kLimbs]) {
  const uint8_t* sb = reinterpret_cast<const uint8_t*>(S);
#pragma unroll
  for (int i = 0; i < kLimbs; ++i) v[i] = 0u;
  x = 0;
  // untrusted offsets: the record must lie inside this wave's window
  bool ok = oe >= w.A && ee > oe && ee <= w.Bend;
  const int32_t o = static_cast<int32_t>(oe - w.A4), end = static_cast<int32_t>(ee - w.A4);
  const uint32_t xlen = ok ? sb[o] : 0u;
  ok = ok && xlen <= 8 && o + 1 + static_cast<int32_t>(xlen) <= end;
  if (ok) {
    for (uint32_t i = 0; i < xlen; ++i) x = (x << 8) | sb[o + 1 + i];
    int32_t ys = o + 1 + static_cast<int32_t>(xlen);
    for (; end - ys > 68; ++ys)  // leading zero bytes beyond 68 (rare)
      if (sb[ys]) {
        ok = false;
        break;
      }
    if (ok) {
#pragma unroll
      for (int i = 0; i < kLimbs; ++i) {
        const int32_t q = end - 4 * (i + 1);  // window position of limb i's top byte
        const int32_t nv = end - ys - 4 * i;  // bytes of limb i inside y
        const int32_t qa = q < -4 ? -4 : q;   // stay inside the padded slice
        const uint32_t lo = S[qa >> 2], hi = S[(qa >> 2) + 1];
        uint32_t t = __builtin_bswap32(__builtin_amdgcn_alignbyte(hi, lo, static_cast<uint32_t>(qa) & 3u));
        t = nv >= 4 ? t : (nv <= 0 ? 0u : (t & ((1u << (8 * nv)) - 1u)));
        v[i] = t;
      }
    }
  }
  return ok;
}

// How a wave that reads several wires brings a window to LDS (the wire loops
// of recon_records.hip and sum_records.hip):
//   kSerial  the whole window into registers (every load issued before the
//            first LDS store), then to LDS, then parsed
//   kAhead   the same with wire i + 1's loads issued before wire i's parse
//            and arithmetic
//   kDirect  stage_direct (a load and its LDS store per step): fewer registers
enum StageMode { kSerial = 0, kAhead = 1, kDirect = 2 };

}  // namespace dn
