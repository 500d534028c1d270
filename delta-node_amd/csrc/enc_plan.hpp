// enc_plan.hpp — which tensor, which of its tiles and which wire positions one
// global tile of the segmented share encode is (dn_m521_encode_shares_many).
//
// The list's tensors keep their own tiled share blocks (256-element tiles, the
// last one partial; share row r of tensor k at base_k + r * pitch_k), so the
// work space is the global tile range of recon_plan.hpp: tensor k owns the
// tiles [tile_begin_k, tile_begin_{k+1}).  The wire, however, is ONE record
// stream over the concatenation: word w of local tile lt of tensor k is global
// element e_begin_k + 256 lt + w, and its record and offsets[] entry sit at
// that index.  This header holds the arithmetic that turns (table, global
// tile) into (segment, local tile, live words, global element index, row
// bytes) — shared by the kernels (codec_many.hip) and by a host program that
// checks it against a per-element map (tests/host/enc_plan_check.cpp): it is
// the one place where a mistake reads outside a block or writes another
// tensor's offsets.  Plain C++: no HIP header.
#pragma once

#include <stdint.h>

#include "recon_plan.hpp"

namespace dn {

// One entry per non-empty tensor, in order, then a sentinel with tile_begin =
// the total tile count and e_begin = n_total (its other fields unused).
// Device memory; entry 0 has tile_begin 0 and e_begin 0.  recon_seg_find /
// recon_seg_step work on it as they do on ReconSegEnt (they read tile_begin).
struct EncSegEnt {
  uint32_t tile_begin;  // the tensor's first global tile
  uint32_t reserved;
  uint64_t e_begin;     // the tensor's first global element
  uint64_t n_elem;
  const uint8_t* base;  // share row 0 of the tensor's block
  uint64_t pitch;       // bytes from one share row to the next
};

// Global tile g of segment s (tile_begin_s <= g < tile_begin_{s+1}), seen from
// share row `row`.
struct EncTile {
  uint32_t lt;        // the tensor's local tile
  uint32_t live;      // its words [0, live) are elements (1..256), the rest padding
  uint64_t e0;        // global element index of word 0
  uint64_t row_byte;  // the tile's first byte, from the block's base
  bool ends_list;     // word live - 1 is the list's last element (it writes offsets[n_total])
};

template <typename Tab>
DN_SEG_HD EncTile enc_tile(Tab t, uint32_t nseg, uint32_t s, uint32_t g, uint32_t row) {
  EncTile r;
  r.lt = g - t[s].tile_begin;
  const uint64_t n = t[s].n_elem;
  const uint64_t left = n - recon_elem(r.lt, 0u);  // > 0: lt < ceil(n / 256)
  r.live = left < kSegTile ? static_cast<uint32_t>(left) : kSegTile;
  r.e0 = t[s].e_begin + recon_elem(r.lt, 0u);
  r.row_byte = static_cast<uint64_t>(row) * t[s].pitch + recon_tile_offset(r.lt);
  r.ends_list = s + 1u == nseg && left <= kSegTile;
  return r;
}

// The list's element count (the sentinel's e_begin): offsets[] has one more entry.
template <typename Tab>
DN_SEG_HD uint64_t enc_n_total(Tab t, uint32_t nseg) {
  return t[nseg].e_begin;
}

}  // namespace dn
