// codec_many.hip — the share wire encoder over a LIST of tensors
// (dn_m521_encode_shares_many).
//
// Reference (delta_node/crypto/shamir/shamir.py:28-33):
//   _share_to_bytes((x, y)) = bytes([len(xb)]) + xb + yb,
//   xb / yb = minimal big-endian bytes (0 -> b"").
// The wire of share x for a tensor list is the tensors' records back to back in
// element order (the concatenation's order) with one int64 offsets[n_total +
// 1]: exactly dn_m521_encode_shares on every tensor's row, concatenated and
// rebased.  Records carry no tile structure, so the receiver reads such a wire
// as the wire of one vector of n_total elements.
//
// The tensors stay in their own tiled blocks (as the segmented split leaves
// them), so the work space is (global tile, wire) — csrc/enc_plan.hpp.  Three
// launches build every wire of a call (up to kGroup wires per launch group,
// their descriptors in the kernel arguments; the segment table is read by
// scalar loads):
//   (1) one wave per (tile, wire): the tile's record bytes, from the top-limb
//       u16s (the low limbs only where a top limb is zero, odds 2^-9);
//   (2) one workgroup per wire: exclusive scan of the tile totals, wire total;
//   (3) one workgroup per (tile, wire): the records' in-tile prefix from the
//       lengths the encoder has anyway (wave scan, then across the 4 waves),
//       offsets[] at the global element index, records laid out in LDS at
//       their final byte positions and written as aligned chunks plus head /
//       tail bytes (wire_emit.hpp: encode_kernel's layout and stores).
// No per-element prefix array: scratch is 8 bytes per (tile, wire).
#include <hip/hip_runtime.h>

#include <cstring>

#include "dn_internal.hpp"
#include "enc_plan.hpp"
#include "m521_device.hpp"
#include "wire_emit.hpp"

namespace dn {
namespace em {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kGroup = 16;              // wires per launch group
static_assert(kBlock == static_cast<int>(kSegTile) && kTile == static_cast<int>(kSegTile), "one thread per tile word");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(4))) EncSegEnt* EncTab;  // read by scalar loads

struct Wire {
  uint64_t* offsets;  // uint64[n_total + 1]
  uint8_t* out;
  uint64_t xbe;       // x's minimal big-endian bytes, byte i in bits [8 i, 8 i + 8)
  uint32_t xlen;
  uint32_t row;       // the share row of every block this wire encodes
};

struct Args {
  const EncSegEnt* segs;  // nseg entries and the sentinel
  uint64_t* tile_tot;     // [nw][ntiles]: tile totals, after the scan their exclusive prefix
  uint64_t* totals;       // [nw]: each wire's length
  uint32_t nseg, ntiles;
  uint32_t nw;
  uint32_t w16;  // bit i: wire i's out is 16-B aligned (the wide store path)
  Wire wire[kGroup];
};
static_assert(sizeof(Args) <= 4096, "the kernel arguments must fit the 4 KB kernarg segment");

// y length of word w of a tile from limbs 15 .. 0 (the top limb was zero).
// (Inlined: a call would hand the descriptor over in VGPRs.)
__device__ __forceinline__ uint32_t y_len_low(rsrc_t r, uint32_t w) {
#pragma nounroll
  for (int i = 15; i >= 0; --i) {
    const uint32_t l = __builtin_amdgcn_raw_buffer_load_b32(r, w * 4u + static_cast<uint32_t>(i) * 4u * kTile, 0, 0);
    if (l) return 4u * i + limb_bytes(l);
  }
  return 0u;
}

// (1) One wave per (global tile, wire); lane j takes words 4 j .. 4 j + 3: one
// 8-B load of their top-limb u16s, lengths summed over the wave, words at or
// past the tensor's end counting 0 (their lanes are loaded with the rest of
// the tile's plane — the allocation covers them — and never looked at).
__global__ void __launch_bounds__(kBlock) tile_totals_kernel(Args a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
  if (g >= a.ntiles) return;  // wave-uniform; the kernel has no barrier
  const uint32_t i = blockIdx.y;
  const EncTab tab = (EncTab)a.segs;
  const uint32_t s = recon_seg_find(tab, a.nseg, g);
  const EncTile tl = enc_tile(tab, a.nseg, s, g, a.wire[i].row);
  const rsrc_t r = tile_rsrc(tab[s].base + tl.row_byte);
  const uint32_t xlen = a.wire[i].xlen;
  const uint32_t w0 = 4u * lane;
  uint32_t sum = 0;
  if (recon_live(tab[s].n_elem, tl.lt, w0)) {
    const u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(r, w0 * 2u, static_cast<int>(kHiOffset), kNt);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (recon_live(tab[s].n_elem, tl.lt, w0 + j)) {
        const uint32_t tp = ((j < 2 ? q.x : q.y) >> (16 * (j & 1))) & kTopMask;
        sum += 1u + xlen + (tp ? 64u + limb_bytes(tp) : y_len_low(r, w0 + j));
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
  if (lane == 0) a.tile_tot[static_cast<uint64_t>(i) * a.ntiles + g] = sum;
}

// (2) Exclusive scan of one wire's tile totals in one workgroup, and the
// wire's length (a tile's total is at most 256 * 75 bytes).
__global__ void __launch_bounds__(kScanThreads) scan_tiles_kernel(uint64_t* __restrict__ tile_tot, uint32_t ntiles,
                                                                  uint64_t* __restrict__ totals) {
  const uint64_t total = scan_block_totals(tile_tot + static_cast<uint64_t>(blockIdx.x) * ntiles, ntiles);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// (3) One workgroup per (global tile, wire), thread = word of the tile; one
// wave = 64 consecutive words = one contiguous run of records.  The records'
// offsets are the tile's scanned total plus the in-tile exclusive prefix of the
// lengths (dead words: 0).  Each lane lays its record into the wave's LDS
// window at its final byte position (mod 4, or mod 16 on the wide path, like
// the destination) exactly as encode_kernel does, and the window goes out as
// aligned chunks wholly inside the wave's byte range [A, B) plus head / tail
// bytes: a neighbouring range — the next wave's, or another workgroup's when
// the tile is a tensor's partial last one and the next tensor's first record
// follows inside the same dword — is never touched.
__global__ void __launch_bounds__(kBlock) encode_many_kernel(Args a) {
  __shared__ __attribute__((aligned(16))) uint32_t s_buf[kWaves][kEncRowWords];
  __shared__ uint32_t s_w[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const uint32_t g = blockIdx.x, i = blockIdx.y;
  const EncTab tab = (EncTab)a.segs;
  const uint32_t s = recon_seg_find(tab, a.nseg, g);
  const EncTile tl = enc_tile(tab, a.nseg, s, g, a.wire[i].row);
  const rsrc_t r = tile_rsrc(tab[s].base + tl.row_byte);
  const uint32_t xlen = a.wire[i].xlen;
  const uint64_t xbe = a.wire[i].xbe;
  const bool w16 = (a.w16 >> i) & 1u;
  const bool valid = recon_live(tab[s].n_elem, tl.lt, t);
  uint32_t v[kLimbs];
  uint32_t ylen = 0, len = 0;
  if (valid) {
    load_fe_b(r, t, v);
    ylen = y_len(v);
    len = 1u + xlen + ylen;
  }
  uint32_t inc = len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(inc, d);
    if (lane >= static_cast<uint32_t>(d)) inc += u;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  uint32_t wbase = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) wbase += (w < static_cast<int>(wv)) ? s_w[w] : 0u;
  const uint64_t vmask = __ballot(valid);
  if (!vmask) return;  // wave-uniform: the whole wave is past the tensor's end (behind the barrier)
  const uint64_t off = a.tile_tot[static_cast<uint64_t>(i) * a.ntiles + g] + wbase + inc - len;
  uint64_t* __restrict__ offsets = a.wire[i].offsets;
  uint8_t* __restrict__ out = a.wire[i].out;
  if (valid) {
    offsets[tl.e0 + t] = off;
    if (tl.ends_list && t + 1u == tl.live) offsets[tl.e0 + t + 1u] = off + len;
  }
  // the wave's byte range [A, B) (live words are a prefix of the tile: lane 0 is live)
  const uint64_t A = __shfl(off, 0);
  const uint32_t last = static_cast<uint32_t>(63 - __builtin_clzll(vmask));
  const uint64_t endl = off + len;
  const uint64_t B = __shfl(endl, last);
  const uint64_t A4 = w16 ? (A & ~15ull) : (A & ~3ull);  // LDS byte 0 of the window
  uint8_t* sb = reinterpret_cast<uint8_t*>(s_buf[wv]);
  if (valid) {
    const int32_t p = static_cast<int32_t>(off - A4);
    sb[p] = static_cast<uint8_t>(xlen);
    for (uint32_t j = 0; j < xlen; ++j) sb[p + 1 + j] = static_cast<uint8_t>(xbe >> (8u * j));
    if (ylen) lay_y(s_buf[wv], p + 1 + static_cast<int32_t>(xlen), static_cast<int32_t>(ylen), v);
  }
  flush_window(s_buf[wv], out, A, B, A4, w16, lane);
}

constexpr uint64_t table_bytes(uint64_t nseg) { return ((nseg + 1) * sizeof(EncSegEnt) + 15u) & ~15ull; }

}  // namespace em
}  // namespace dn

using namespace dn;

// scratch: the table's n_segments + 1 entries, then 8 bytes per (tile, wire).
extern "C" uint64_t dn_m521_encode_many_scratch_bytes(uint64_t n_segments, uint64_t total_tiles, uint64_t n_rows) {
  return em::table_bytes(n_segments) + total_tiles * n_rows * sizeof(uint64_t);
}

extern "C" int dn_m521_encode_shares_many(const uint64_t* n_elem, const void* const* blocks, const uint64_t* pitches,
                                          uint64_t n_segments, const uint32_t* rows, const uint64_t* xs,
                                          uint64_t* const* offsets, uint8_t* const* outs, const uint64_t* capacities,
                                          uint64_t n_rows, uint64_t* totals, void* scratch, uint64_t scratch_bytes,
                                          void* stream) {
  const char* name = "dn_m521_encode_shares_many";
  if (n_segments > kMaxSegments)
    return set_error(DN_ERR_ARG, "%s: %llu segments (at most %llu)", name, static_cast<unsigned long long>(n_segments),
                     static_cast<unsigned long long>(kMaxSegments));
  if (n_segments && !n_elem) return set_error(DN_ERR_ARG, "%s: null pointer", name);
  uint64_t nseg = 0, ntiles = 0, n_total = 0;
  for (uint64_t j = 0; j < n_segments; ++j) {
    if (!n_elem[j]) continue;  // an empty tensor: its block is not read
    if (n_elem[j] > (1ull << 40))
      return set_error(DN_ERR_ARG, "%s: tensor %llu too long", name, static_cast<unsigned long long>(j));
    ntiles += (n_elem[j] + kTile - 1) / kTile;
    n_total += n_elem[j];
    ++nseg;
  }
  if (!nseg || !n_rows) return DN_OK;
  if (ntiles >= (1ull << 31)) return set_error(DN_ERR_ARG, "%s: more than 2^31 tiles", name);
  if (!blocks || !pitches || !rows || !xs || !offsets || !outs || !capacities || !totals || !scratch)
    return set_error(DN_ERR_ARG, "%s: null pointer", name);
  for (uint64_t j = 0; j < n_segments; ++j) {
    if (!n_elem[j]) continue;
    if (!blocks[j]) return set_error(DN_ERR_ARG, "%s: null block of tensor %llu", name, static_cast<unsigned long long>(j));
    // the limbs are loaded as dwords from base + row * pitch + (a multiple of 4)
    if ((reinterpret_cast<uintptr_t>(blocks[j]) | pitches[j]) & 3u)
      return set_error(DN_ERR_ARG, "%s: block and row pitch of tensor %llu must be 4-byte aligned", name,
                       static_cast<unsigned long long>(j));
  }
  for (uint64_t i = 0; i < n_rows; ++i) {
    if (!offsets[i] || !outs[i])
      return set_error(DN_ERR_ARG, "%s: null pointer of wire %llu", name, static_cast<unsigned long long>(i));
    // the narrow path stores dwords at out + (an offset that is a multiple of 4)
    if (reinterpret_cast<uintptr_t>(outs[i]) & 3u)
      return set_error(DN_ERR_ARG, "%s: out of wire %llu must be 4-byte aligned", name,
                       static_cast<unsigned long long>(i));
    if (capacities[i] < dn_m521_encoded_capacity(n_total, xs[i]))
      return set_error(DN_ERR_ARG, "%s: capacity %llu < %llu of wire %llu", name,
                       static_cast<unsigned long long>(capacities[i]),
                       static_cast<unsigned long long>(dn_m521_encoded_capacity(n_total, xs[i])),
                       static_cast<unsigned long long>(i));
  }
  if (scratch_bytes < dn_m521_encode_many_scratch_bytes(n_segments, ntiles, n_rows))
    return set_error(DN_ERR_ARG, "%s: scratch too small", name);
  const uint64_t tab_bytes = (nseg + 1) * sizeof(EncSegEnt);
  StageBuf stage = stage_take(tab_bytes);
  if (!stage.p) return set_error(DN_ERR_HIP, "%s: pinned staging buffer", name);
  EncSegEnt* ent = static_cast<EncSegEnt*>(stage.p);
  uint64_t s = 0, t = 0, e = 0;
  for (uint64_t j = 0; j < n_segments; ++j) {
    if (!n_elem[j]) continue;
    ent[s++] = EncSegEnt{static_cast<uint32_t>(t), 0u, e, n_elem[j], static_cast<const uint8_t*>(blocks[j]), pitches[j]};
    t += (n_elem[j] + kTile - 1) / kTile;
    e += n_elem[j];
  }
  ent[s] = EncSegEnt{static_cast<uint32_t>(ntiles), 0u, n_total, 0u, nullptr, 0u};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (hipMemcpyAsync(scratch, stage.p, tab_bytes, hipMemcpyHostToDevice, st) != hipSuccess) {
    stage_give(stage, nullptr);
    return set_error(DN_ERR_HIP, "%s: table upload", name);
  }
  stage_give(stage, &st);
  uint64_t* tile_tot = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(scratch) + em::table_bytes(n_segments));
  for (uint64_t i0 = 0; i0 < n_rows; i0 += em::kGroup) {  // more wires: more launch groups over the same table
    em::Args a{};
    a.segs = static_cast<const EncSegEnt*>(scratch);
    a.tile_tot = tile_tot + i0 * ntiles;
    a.totals = totals + i0;
    a.nseg = static_cast<uint32_t>(nseg);
    a.ntiles = static_cast<uint32_t>(ntiles);
    a.nw = static_cast<uint32_t>(n_rows - i0 < em::kGroup ? n_rows - i0 : em::kGroup);
    for (uint32_t i = 0; i < a.nw; ++i) {
      em::Wire& w = a.wire[i];
      const uint64_t x = xs[i0 + i];
      w.offsets = offsets[i0 + i];
      w.out = outs[i0 + i];
      w.row = rows[i0 + i];
      while (w.xlen < 8 && (x >> (8 * w.xlen))) ++w.xlen;
      for (uint32_t b = 0; b < w.xlen; ++b) w.xbe |= ((x >> (8 * (w.xlen - 1 - b))) & 0xFFull) << (8 * b);
      if ((reinterpret_cast<uintptr_t>(w.out) & 15u) == 0) a.w16 |= 1u << i;
    }
    const uint32_t nt = a.ntiles;
    hipLaunchKernelGGL(em::tile_totals_kernel, dim3((nt + em::kWaves - 1) / em::kWaves, a.nw), dim3(em::kBlock), 0, st,
                       a);
    hipLaunchKernelGGL(em::scan_tiles_kernel, dim3(a.nw), dim3(kScanThreads), 0, st, a.tile_tot, nt, a.totals);
    hipLaunchKernelGGL(em::encode_many_kernel, dim3(nt, a.nw), dim3(em::kBlock), 0, st, a);
  }
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return set_error(DN_ERR_HIP, "%s: %s", name, hipGetErrorString(err));
  return DN_OK;
}
