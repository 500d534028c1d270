// seg_plan.hpp — where the 64 elements of one emission group land when the
// fused draw + split writes a LIST of share blocks (dn_mt19937_split_many_device).
//
// The global element range [0, n_total) is the concatenation of the list's
// non-empty tensors; tensor k owns [e_begin_k, e_begin_{k+1}) and has its own
// block of tiled share rows (256-element tiles of 66 * 256 bytes, row pitch
// row_bytes_k = vec_bytes(n_k)).  A group is 64 consecutive global elements
// from a multiple of 64, lane = element.  This header holds the arithmetic
// that turns (segment table, group) into stores — shared by the kernel
// (mt19937_device.hip, emit_split_seg) and by a host program that checks it
// against a per-element map (tests/host/many_plan_check.cpp): it is the one
// place where a mistake writes outside a block.  Plain C++: no HIP header.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DN_SEG_HD __host__ __device__ inline
#else
#define DN_SEG_HD inline
#endif

namespace dn {

constexpr uint32_t kSegTile = 256;                  // elements per layout tile (m521_device.hpp kTile)
constexpr uint32_t kSegTileBytes = 66u * kSegTile;  // (kTileBytes)
constexpr uint64_t kMaxSegments = 65536;

// One entry per non-empty tensor, in order, then a sentinel with e_begin =
// n_total (its other fields unused).  Device memory; entry 0 has e_begin 0.
struct SegEnt {
  uint64_t e_begin;    // the tensor's first global element
  uint8_t* shares;     // its share rows (row x - 1 at shares + (x - 1) * row_bytes)
  uint64_t row_bytes;  // vec_bytes(n_k)
};

// The segment that holds element e (e < n_total): the last k in [0, nseg) with
// e_begin_k <= e.  (Tab: a pointer to SegEnt — the kernel's is in the constant
// address space, so that the table is read by scalar loads.)
template <typename Tab>
DN_SEG_HD uint32_t seg_find(Tab t, uint32_t nseg, uint64_t e) {
  uint32_t lo = 0, hi = nseg;  // e_begin[lo] <= e < e_begin[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (t[mid].e_begin <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The segment of element e from a cursor on a nearby one (groups advance by 64
// elements: up in forward substreams, down in backward ones).
template <typename Tab>
DN_SEG_HD uint32_t seg_step(Tab t, uint32_t k, uint64_t e) {
  while (t[k + 1u].e_begin <= e) ++k;  // (the sentinel's n_total > e ends it)
  while (t[k].e_begin > e) --k;        // (entry 0's 0 <= e ends it)
  return k;
}

// The group [ebase, ebase + 64) lies in one tile of the segment [e_begin,
// e_next): its live elements (those below n_total) all belong to the segment,
// and the segment starts at a multiple of 64 (ebase is one), so the lanes'
// local indices ebase - e_begin + lane share a tile — the single-block store.
DN_SEG_HD bool seg_single_tile(uint64_t e_begin, uint64_t e_next, uint64_t ebase, uint64_t n_total) {
  return (e_begin & 63u) == 0u && (e_next - ebase >= 64u || e_next == n_total);
}

// The part of a group that falls into one segment: lanes [lane_lo, lane_hi)
// store into the segment's rows through one buffer descriptor per row, based
// at tile `tile0` of the row and `range` bytes long (clamped to the row's end);
// the lanes touch that tile and at most the next one.
struct SegPiece {
  uint32_t lane_lo, lane_hi;
  uint64_t tile0;  // descriptor base = row + tile0 * kSegTileBytes
  uint32_t range;  // descriptor bytes (<= 2 tiles)
  uint32_t w0;     // lane_lo's position in tile0 (< 256); lane L is at word w0 + L - lane_lo
};

// [e_begin, e_next) must intersect [ebase, min(ebase + 64, n_total)).
DN_SEG_HD SegPiece seg_piece(uint64_t e_begin, uint64_t e_next, uint64_t row_bytes, uint64_t ebase,
                             uint64_t n_total) {
  const uint64_t gend = n_total - ebase < 64u ? n_total : ebase + 64u;
  const uint64_t lo = e_begin > ebase ? e_begin : ebase, hi = e_next < gend ? e_next : gend;
  SegPiece p;
  p.lane_lo = static_cast<uint32_t>(lo - ebase);
  p.lane_hi = static_cast<uint32_t>(hi - ebase);
  const uint64_t l0 = lo - e_begin;  // local index of the piece's first element
  p.tile0 = l0 / kSegTile;
  p.w0 = static_cast<uint32_t>(l0 % kSegTile);
  const uint64_t left = row_bytes - p.tile0 * kSegTileBytes;  // bytes of the row from tile0 on
  p.range = left < 2u * kSegTileBytes ? static_cast<uint32_t>(left) : 2u * kSegTileBytes;
  return p;
}

// Byte offsets of word w (counted from tile0's first element, w < 512) from
// the descriptor's base, less the limb plane's own offset (limb i < 16: + i *
// 4 * 256; the 16-bit top plane: + 64 * 256): one tile's bytes more for a word
// in the second tile.
DN_SEG_HD uint32_t seg_voff32(uint32_t w) { return (w / kSegTile) * kSegTileBytes + (w % kSegTile) * 4u; }
DN_SEG_HD uint32_t seg_voff16(uint32_t w) { return (w / kSegTile) * kSegTileBytes + (w % kSegTile) * 2u; }

}  // namespace dn
