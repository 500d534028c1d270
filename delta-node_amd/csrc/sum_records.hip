// sum_records.hip — the share-domain sum straight from wire records
// (dn_m521_sum_records): the m packed `_share_to_bytes` streams (shamir.py:28-33)
// that party x holds — share x of every member's tensor — in, their sum mod p
// as one tiled vector out, in one launch and without the m decoded vectors.
//
// Per element e and wire i the kernel parses record e of wire i with the
// functions decode_kernel (codec_m521.hip) and recon_records.hip parse with
// (wire_parse.hpp: the window staged in LDS, the byte-serial path for a window
// beyond the LDS slice, the treatment of untrusted offsets), reduces y (a
// 68-byte y exceeds 2^521), complements it within 521 bits where the wire is
// subtracted and adds it to a lazy 17-limb accumulator, as share_sum.hip adds
// its inputs: add, add, ..., one reduce().  There is no arithmetic of its own
// here: every primitive is m521_device.hpp's.
//
// One wave = 64 consecutive elements (decode_kernel's unit), one workgroup =
// one 256-element output tile, one LDS slice per wave, reused wire after wire
// (the wire loop below).  A wire's whole window is loaded into registers (at most 5
// 16-byte or 19 4-byte loads per lane, all issued before the first LDS store)
// and then stored to LDS: kSerial.  Loading wire i + 1 under wire i's parse
// (kAhead), and staging with decode_kernel's own loop (kDirect), were measured
// and did not pay; a fourth resident wave did (DN_SR_WAVES).
// A list beyond DN_M521_SUM_RECORDS_GROUP wires is chained by the entry point:
// every launch ends canonical and the next takes `out` as its acc, so the
// result does not depend on where the group boundaries fall.
//
// The wire descriptors, sign bits and alignment bits are kernel
// arguments indexed by the wave-uniform wire counter: scalar loads, no device
// table, nothing that synchronises (the call can be captured into a graph).
#include <hip/hip_runtime.h>

#include "dn_internal.hpp"
#include "m521_device.hpp"
#include "wire_parse.hpp"

namespace dn {
namespace sr {

constexpr int kBlock = 256;
constexpr int kGroup = DN_M521_SUM_RECORDS_GROUP;

struct Wire {
  const uint8_t* in;        // packed records
  uint64_t in_bytes;
  const uint64_t* offsets;  // uint64[n_elem + 1]
};

struct Args {
  Wire wire[kGroup];
  uint32_t neg[kGroup / 32];  // bit i of word i / 32: wire i is subtracted
  uint32_t w16[kGroup / 32];  // the same for: wire i is 16-B aligned (the wide staging path)
  const uint8_t* acc;         // tiled vector added to the sum, or null
  uint8_t* out;
  uint32_t* bad;  // [0] unrepresentable records, [1] records whose x is not `x`
  uint64_t n_elem;
  uint64_t x;  // the abscissa every record should carry
  uint32_t m;  // wires of this launch, 1 .. kGroup
};
static_assert(sizeof(Args) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");
// acc (< 2^521) and kGroup terms (each < 2^521) stay below 2^544
static_assert(kGroup % 32 == 0 && kGroup + 1 < (1 << 23), "sign words; lazy-form bound");

__device__ __forceinline__ bool bit_of(const uint32_t* words, uint32_t i) {
  return (words[i >> 5] >> (i & 31u)) & 1u;
}

// Wire i of one lane: its record parsed from the staged window (or from
// global memory where the window did not fit), y reduced — a 68-byte y exceeds
// 2^521 — complemented within 521 bits where the wire is subtracted (-y == p - y
// == ~y there) and added to the lazy accumulator; the wave's two counts.
__device__ __forceinline__ void wire_step(const Args& a, uint32_t i, const uint32_t* S, const Win& cw, uint64_t oe,
                                          uint64_t ee, bool valid, uint32_t (&acc)[kLimbs], uint32_t& nbad,
                                          uint32_t& nmis) {
  bool ok = false;
  uint64_t x = 0;
  if (valid) {
    uint32_t v[kLimbs];
    if (cw.lds) {
      ok = parse_lds(S, cw, oe, ee, x, v);
    } else {
      ok = oe < ee && ee <= a.wire[i].in_bytes && parse_global(a.wire[i].in, oe, ee, x, v);
    }
    if (ok) {
      reduce(v);
    } else {  // counted below; contributes y = 0, as the decoded vector would
#pragma unroll
      for (int l = 0; l < kLimbs; ++l) v[l] = 0u;
    }
    if (bit_of(a.neg, i)) {
#pragma unroll
      for (int l = 0; l < 16; ++l) v[l] = ~v[l];
      v[16] = (~v[16]) & kTopMask;
    }
    add_fe(acc, v);
  }
  nbad += static_cast<uint32_t>(__popcll(__ballot(valid && !ok)));
  nmis += static_cast<uint32_t>(__popcll(__ballot(valid && ok && x != a.x)));
}

template <int PF>
__device__ __forceinline__ void sum_body(const Args& a, uint32_t (*s_win)[kDecRowWords]) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t tile = blockIdx.x;  // one workgroup per 256-element output tile
  const uint64_t e0 = static_cast<uint64_t>(tile) * kTile + 64u * wv;
  const rsrc_t ro = tile_rsrc(tile_base(a.out, tile));

  uint32_t acc[kLimbs];
#pragma unroll
  for (int l = 0; l < kLimbs; ++l) acc[l] = 0u;
  if (e0 >= a.n_elem) {  // wave-uniform: a wave of padding lanes in the last tile, written as zero
    store_fe_b(ro, threadIdx.x, acc);
    return;
  }
  const uint64_t e = e0 + lane;
  const bool valid = e < a.n_elem;
  const uint64_t eN = e0 + 64 < a.n_elem ? e0 + 64 : a.n_elem;
  uint32_t* S = s_win[wv] + kWinPad / 4;  // S[j] = dword at window byte 4j
  const uint32_t m = a.m;
  // a lane reads its element of acc before it writes that element of out: acc may be out
  if (a.acc && valid) load_fe_b(tile_rsrc(tile_base(a.acc, tile)), threadIdx.x, acc);
  uint32_t nbad = 0u, nmis = 0u;  // wave-uniform counts

  if constexpr (PF == kDirect) {
    for (uint32_t i = 0; i < m; ++i) {
      const bool w16 = bit_of(a.w16, i);
      const Win cw = win_of((OffTab)a.wire[i].offsets, a.wire[i].in_bytes, w16, e0, eN);
      uint64_t oe = 0, ee = 0;
      if (valid) {
        oe = a.wire[i].offsets[e];
        ee = a.wire[i].offsets[e + 1];
      }
      if (cw.lds) stage_direct(S, a.wire[i].in, cw, w16, lane);
      lds_order();
      wire_step(a, i, S, cw, oe, ee, valid, acc, nbad, nmis);
      lds_order();  // the slice is free for the next window
    }
  } else {
    Stage st;
    Win nw = win_of((OffTab)a.wire[0].offsets, a.wire[0].in_bytes, bit_of(a.w16, 0), e0, eN);
    uint64_t noe = 0, nee = 0;
    if (nw.lds) stage_load(st, a.wire[0].in, nw, bit_of(a.w16, 0), lane);
    if (valid) {
      noe = a.wire[0].offsets[e];
      nee = a.wire[0].offsets[e + 1];
    }
    for (uint32_t i = 0; i < m; ++i) {
      const Win cw = nw;
      const uint64_t oe = noe, ee = nee;
      if (cw.lds) stage_store(st, S, cw, bit_of(a.w16, i), lane);
      lds_order();
      if (PF == kAhead && i + 1 < m) {  // wire i + 1's loads go out before wire i's parse and add
        const bool w16n = bit_of(a.w16, i + 1);
        nw = win_of((OffTab)a.wire[i + 1].offsets, a.wire[i + 1].in_bytes, w16n, e0, eN);
        if (nw.lds) stage_load(st, a.wire[i + 1].in, nw, w16n, lane);
        if (valid) {
          noe = a.wire[i + 1].offsets[e];
          nee = a.wire[i + 1].offsets[e + 1];
        }
      }
      wire_step(a, i, S, cw, oe, ee, valid, acc, nbad, nmis);
      lds_order();  // the slice is free for the next window
      if (PF == kSerial && i + 1 < m) {
        const bool w16n = bit_of(a.w16, i + 1);
        nw = win_of((OffTab)a.wire[i + 1].offsets, a.wire[i + 1].in_bytes, w16n, e0, eN);
        if (nw.lds) stage_load(st, a.wire[i + 1].in, nw, w16n, lane);
        if (valid) {
          noe = a.wire[i + 1].offsets[e];
          nee = a.wire[i + 1].offsets[e + 1];
        }
      }
    }
  }
  // acc < 2^521 * (m + 1) < 2^544: one reduce; lanes past n_elem hold zero and store zero
  reduce(acc);
  store_fe_b(ro, threadIdx.x, acc);
  if (lane == 0) {
    if (nbad) atomicAdd(a.bad, nbad);
    if (nmis) atomicAdd(a.bad + 1, nmis);
  }
}

// DN_SR_WAVES: the waves per SIMD the register allocator is asked for.  Left
// to itself (0) the kSerial form takes 142 VGPRs, 3 waves; held to 4 it fits
// 128 without scratch and runs 13-17 % faster at every measured shape (the
// kernel waits on memory: one more resident wave is one more window in
// flight).  5 would need 96 and spills 2.2 KB per lane.  DESIGN.md §4.18.
#ifndef DN_SR_WAVES
#define DN_SR_WAVES 4
#endif
#if DN_SR_WAVES > 0
#define DN_SR_OCCUPANCY __attribute__((amdgpu_waves_per_eu(DN_SR_WAVES, DN_SR_WAVES)))
#else
#define DN_SR_OCCUPANCY
#endif

template <int PF>
__global__ void __launch_bounds__(kBlock) DN_SR_OCCUPANCY sum_records_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_win[kBlock / 64][kDecRowWords];
  sum_body<PF>(a, s_win);
}

template <int PF>
static void launch_one(dim3 g, hipStream_t s, const Args& a) {
  hipLaunchKernelGGL((sum_records_kernel<PF>), g, dim3(kBlock), 0, s, a);
}

// The product form, and the A/B hook of the tuning build: DN_SR_STAGE=0/1/2
// selects one staging mode.
static void launch(dim3 g, hipStream_t s, const Args& a) {
#ifdef DN_TUNING
  if (const char* e = tune_env("DN_SR_STAGE")) {
    if (e[0] == '0') launch_one<kSerial>(g, s, a);
    else if (e[0] == '1') launch_one<kAhead>(g, s, a);
    else launch_one<kDirect>(g, s, a);
    return;
  }
#endif
  launch_one<kSerial>(g, s, a);
}

}  // namespace sr
}  // namespace dn

using namespace dn;

extern "C" int dn_m521_sum_records(const uint8_t* const* in, const uint64_t* in_bytes, const uint64_t* const* offsets,
                                   uint64_t m, uint64_t x, const uint8_t* negate, const void* acc, void* out,
                                   uint32_t* bad_counts, uint64_t n_elem, void* stream) {
  const char* name = "dn_m521_sum_records";
  if (n_elem == 0) return DN_OK;
  if (m == 0) return set_error(DN_ERR_ARG, "%s: no wire", name);
  if (!in || !in_bytes || !offsets || !out || !bad_counts) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  const uint64_t blocks = (n_elem + kTile - 1) / kTile;
  if (blocks >= (1ull << 31)) return set_error(DN_ERR_ARG, "%s: n_elem %llu needs 2^31 workgroups or more", name,
                                               (unsigned long long)n_elem);
  if (acc && acc != out) {
    const uint64_t a0 = reinterpret_cast<uint64_t>(acc), o0 = reinterpret_cast<uint64_t>(out);
    if ((a0 > o0 ? a0 - o0 : o0 - a0) < blocks * kTileBytes)
      return set_error(DN_ERR_ARG, "%s: acc overlaps out without being equal to it", name);
  }
  for (uint64_t i = 0; i < m; ++i) {
    if (!in[i] || !offsets[i]) return set_error(DN_ERR_ARG, "%s: null wire %llu", name, (unsigned long long)i);
    // the narrow path loads dwords from in + (an offset that is a multiple of 4)
    if (reinterpret_cast<uintptr_t>(in[i]) & 3u)
      return set_error(DN_ERR_ARG, "%s: wire %llu must be 4-byte aligned", name, (unsigned long long)i);
    if (reinterpret_cast<uintptr_t>(offsets[i]) & 7u)
      return set_error(DN_ERR_ARG, "%s: offsets of wire %llu must be 8-byte aligned", name, (unsigned long long)i);
  }
  bool w4 = false;
#ifdef DN_TUNING
  w4 = tune_env("DN_DECODE_W4") && tune_env("DN_DECODE_W4")[0] == '1';  // A/B: 4-B staging
#endif
  const dim3 g(static_cast<uint32_t>(blocks));
  hipStream_t s = static_cast<hipStream_t>(stream);
  // launch 1 writes out (from acc if given); each later launch adds the next group onto out
  for (uint64_t first = 0; first < m; first += sr::kGroup) {
    sr::Args a{};
    a.m = static_cast<uint32_t>(m - first < sr::kGroup ? m - first : sr::kGroup);
    for (uint32_t i = 0; i < a.m; ++i) {
      const uint64_t src = first + i;
      a.wire[i].in = in[src];
      a.wire[i].in_bytes = in_bytes[src];
      a.wire[i].offsets = offsets[src];
      if (negate && negate[src]) a.neg[i >> 5] |= 1u << (i & 31u);
      if (!w4 && (reinterpret_cast<uintptr_t>(in[src]) & 15u) == 0) a.w16[i >> 5] |= 1u << (i & 31u);
    }
    a.acc = first == 0 ? static_cast<const uint8_t*>(acc) : static_cast<const uint8_t*>(out);
    a.out = static_cast<uint8_t*>(out);
    a.bad = bad_counts;
    a.n_elem = n_elem;
    a.x = x;
    sr::launch(g, s, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  }
  return DN_OK;
}
